#!/usr/bin/env python3
"""Ray-query rates (pt_ctx_intersect) next to the depth-1 render of the same build and scene.

For Cornell and sphere223_in_cornell at 1024^2, in one process: the camera rays of sample 0
(the `ray` AOV) are the ray set; pt_ctx_intersect is timed on device buffers, closest hit and
any hit, in pixel order (coherent) and in a seeded random permutation (incoherent). The
yardstick is Renderer.render(depth=1): the existing megakernel, one BVH::intersect per sample
plus camera ray, shading and accumulation. Every line: warm-up calls, then calls until at
least --min-ms of HIP-event kernel time; Mray/s = rays / kernel time. Writes
<out>/<scene>.json (default profiles/query) and prints each file's content as one JSON line.

    python3 scripts/query_bench.py [--scenes cornell,sphere223] [--res 1024] [--min-ms 1000]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathtracer-cpp_amd"))

import numpy as np  # noqa: E402


def timed(call, warmup, min_ms):
    """call() -> (rays, kernel_ms); repeats until min_ms of kernel time."""
    for _ in range(warmup):
        call()
    rays = reps = 0
    kernel_ms = 0.0
    t0 = time.perf_counter()
    while kernel_ms < min_ms:
        r, ms = call()
        rays += r
        kernel_ms += ms
        reps += 1
    wall_ms = (time.perf_counter() - t0) * 1e3
    return {"mrays_per_s": rays / kernel_ms / 1e3, "kernel_ms": kernel_ms, "wall_ms": wall_ms, "calls": reps,
            "rays_per_call": rays // reps}


def bench_scene(name, res, min_ms, warmup, seed):
    import torch
    import ptamd
    from ptamd import scenes
    sc = scenes.cornell((res, res)) if name == "cornell" else scenes.sphere_in_cornell(int(name[len("sphere"):]), (res, res))
    bvh = ptamd.BVH.from_scene(sc)
    cam = ptamd.Camera.from_spec(sc.camera)
    r = ptamd.Renderer(0)
    r.set_scene(bvh)
    r.prepare()
    aov, ast = r.aov(cam, sample=0, channels=("ray", "tri"))
    rays = aov["ray"].reshape(-1, 6)
    n = rays.shape[0]
    dev = torch.device("cuda", 0)
    perm = np.random.default_rng(seed).permutation(n)
    sets = {}
    for label, order in (("coherent", None), ("incoherent", perm)):
        a = rays if order is None else rays[order]
        sets[label] = (torch.from_numpy(np.ascontiguousarray(a[:, 0:3])).to(dev),
                       torch.from_numpy(np.ascontiguousarray(a[:, 3:6])).to(dev))
    out_t = torch.empty(n, dtype=torch.float32, device=dev)
    out_i = torch.empty(n, dtype=torch.int32, device=dev)
    lines = {}
    placement = None
    for label, (to, td) in sets.items():
        for mode in ("closest", "any"):
            def call():
                _, st = r.intersect(to, td, any_hit=mode == "any", out=out_i if mode == "any" else (out_t, out_i))
                return st["rays"], st["kernel_ms"]
            lines[f"{mode}_{label}"] = timed(call, warmup, min_ms)
            _, st = r.intersect(to, td, any_hit=mode == "any", out=out_i if mode == "any" else (out_t, out_i))
            placement = {"lds_scene": st["lds_scene"], "lds_stack": st["lds_stack"]}
            lines[f"{mode}_{label}"]["hits"] = st["hits"]
    # the incoherent closest hits are the coherent ones, permuted (a check on the run itself)
    (t_p, tri_p), _ = r.intersect(*sets["incoherent"], out=(out_t, out_i))
    assert np.array_equal(tri_p.cpu().numpy(), aov["tri"].reshape(-1)[perm])
    spp = 256 if name == "cornell" else 64
    frame = torch.empty(res * res * 3, dtype=torch.float32, device=dev)
    paths = {}

    def render_call():
        _, st = r.render(cam, spp, 1, out=frame)
        paths["kernel"] = ptamd._lib.pt_stats.PATHS.get(st["kernel_path"], str(st["kernel_path"]))
        return st["rays"], st["kernel_ms"]
    lines["render_depth1"] = timed(render_call, max(1, warmup // 2), min_ms)
    lines["render_depth1"]["spp_per_call"] = spp
    lines["render_depth1"]["kernel"] = paths["kernel"]
    base = lines["render_depth1"]["mrays_per_s"]
    for k, v in lines.items():
        v["ratio_to_render_depth1"] = v["mrays_per_s"] / base
    r.close()
    return {"scene": sc.name, "tris": len(sc.tris), "res": [res, res], "rays": n, "camera_ray_hits": ast["hits"],
            "aov_kernel_ms": ast["kernel_ms"], "placement": placement, "permutation_seed": seed, "min_kernel_ms": min_ms,
            "device": torch.cuda.get_device_name(0), "lines": lines}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="cornell,sphere223")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--min-ms", type=float, default=1000.0, help="kernel time per line")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        res = bench_scene(name, args.res, args.min_ms, args.warmup, args.seed)
        with open(os.path.join(args.out, res["scene"] + ".json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
