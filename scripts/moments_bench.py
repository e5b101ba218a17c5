#!/usr/bin/env python3
"""What the per-pixel sample moments cost: Renderer.render_moments beside Renderer.render.

For Cornell and sphere223_in_cornell at 1024^2, depth 5 (dark scenes: flagged slabs) and for
Cornell with a small emission on every surface (dense slabs, the moments pass's worst case), in
one process: the same spp rendered by render() (fused accumulation) and by render_moments()
(every slab summed by pt_accumulate_moments_kernel, S and Q kept, nothing exported), in turn on
device buffers, `--reps` times each after a warm-up; the median kernel time (trace kernels), the
reduce time (accumulation kernels outside the trace kernels) and the whole call are reported with
the ratios moments / render. The two images are compared bit for bit first. Then one
render_converge at --rel: samples, rounds, unconverged pixels and times. Writes
<out>/<scene>.json (default profiles/moments) and prints each file's content as one JSON line.

    python3 scripts/moments_bench.py [--scenes cornell,cornell_glow,sphere223] [--res 1024] [--spp 1024]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathtracer-cpp_amd"))

import numpy as np  # noqa: E402


def make_scene(name, res):
    from ptamd import scenes
    if name.startswith("sphere"):
        return scenes.sphere_in_cornell(int(name[len("sphere"):]), (res, res))
    sc = scenes.cornell((res, res))
    if name == "cornell_glow":  # no path ends at +0: dense slabs
        e = np.random.default_rng(11).uniform(0.01, 0.2, (len(sc.mats), 3)).astype(np.float32)
        sc.mats = [m if m.type == scenes.EMIT else dataclasses.replace(m, emit=tuple(float(c) for c in e[i]))
                   for i, m in enumerate(sc.mats)]
    elif name != "cornell":
        raise KeyError(name)
    return sc


def timed(call, warmup, reps):
    """call() -> stats dict; medians of kernel_ms, reduce_ms and the call's wall time."""
    for _ in range(warmup):
        call()
    rows = []
    for _ in range(reps):
        t0 = time.perf_counter()
        st = call()
        rows.append((st["kernel_ms"], st["reduce_ms"], (time.perf_counter() - t0) * 1e3, st["rays"]))
    med = lambda i: statistics.median(r[i] for r in rows)
    return {"kernel_ms": med(0), "reduce_ms": med(1), "call_ms": med(2), "rays": rows[0][3], "reps": reps,
            "grays_per_s_call": rows[0][3] / med(2) / 1e6}


def bench_scene(name, res, spp, depth, rel, warmup, reps):
    import torch
    import ptamd
    sc = make_scene(name, res)
    cam = ptamd.Camera.from_spec(sc.camera)
    r = ptamd.Renderer(0)
    r.set_scene(ptamd.BVH.from_scene(sc))
    r.prepare()
    dev = torch.device("cuda", 0)
    a = torch.empty((res, res, 3), dtype=torch.float32, device=dev)
    b = torch.empty((res, res, 3), dtype=torch.float32, device=dev)
    plans = {}

    def render_call():
        _, st = r.render(cam, spp, depth, out=a)
        plans["render"] = r.plan()
        return st

    def moments_call():
        _, _, st = r.render_moments(cam, 0, spp, depth, out=b, want=())
        plans["moments"] = r.plan()
        return st

    render_call()
    moments_call()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "render_moments image differs from render"
    lines = {"render": timed(render_call, warmup, reps), "render_moments": timed(moments_call, warmup, reps)}
    for k in ("render", "moments"):
        lines["render" if k == "render" else "render_moments"].update(
            {p: plans[k][p] for p in ("kernel_path", "batch", "fused", "flags_pm", "trace_launches")})
    ratios = {k: lines["render_moments"][k] / lines["render"][k] for k in ("kernel_ms", "call_ms")}
    ratios["kernel_plus_reduce"] = ((lines["render_moments"]["kernel_ms"] + lines["render_moments"]["reduce_ms"]) /
                                    (lines["render"]["kernel_ms"] + lines["render"]["reduce_ms"]))
    t0 = time.perf_counter()
    _, mom, info = r.render_converge(cam, depth, rel, min_samples=16, max_samples=spp, out=b, want=("sem",))
    info["call_ms"] = (time.perf_counter() - t0) * 1e3
    info["rel"] = rel
    info["max_sem"] = float(mom["sem"].max())
    r.close()
    return {"scene": sc.name, "label": name, "tris": len(sc.tris), "res": [res, res], "spp": spp, "depth": depth,
            "device": torch.cuda.get_device_name(0), "lines": lines, "moments_over_render": ratios, "converge": info}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,cornell_glow,sphere223")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--rel", type=float, default=0.05)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        spp = args.spp if not name.startswith("sphere") else max(16, args.spp // 8)
        res = bench_scene(name, args.res, spp, args.depth, args.rel, args.warmup, args.reps)
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
