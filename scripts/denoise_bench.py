#!/usr/bin/env python3
"""What the a-trous denoiser costs: Renderer.denoise beside Renderer.render and a device copy.

For Cornell and sphere223_in_cornell at 1024^2, depth 5, in one process: the frame is rendered at
--spp with its moments on the device, the guides are the AOV of sample 0, the variance is
Renderer.moments_variance. Then Renderer.denoise on device tensors at the default parameters, once
with every pass in the direct form (PT_DENOISE_LDS=0) and once with stride 1 in the LDS-tiled
form (PT_DENOISE_LDS=1), `--reps` times each after a warm-up: the median kernel time of every
pass (with the smallest and the largest beside it: the spread a decision between the forms is
judged against), of the pack step, of the whole call's kernels and the call's wall time. The two forms'
images are compared bit for bit first. Beside them: Renderer.render of the same frame (kernel and
call time), and a device-to-device copy of 48 bytes per pixel, which moves the 96 bytes per pixel
one pass must at least read (four 16-byte records) and write (two): the yardstick for "bound by
memory". Writes <out>/<scene>.json (default profiles/denoise) and prints each as one JSON line.

    python3 scripts/denoise_bench.py [--scenes cornell,sphere223] [--res 1024] [--spp 64]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathtracer-cpp_amd"))
os.environ["PT_TEST_HOOKS"] = "1"  # PT_DENOISE_LDS is a test hook


def make_scene(name, res):
    from ptamd import scenes
    if name.startswith("sphere"):
        return scenes.sphere_in_cornell(int(name[len("sphere"):]), (res, res))
    if name != "cornell":
        raise KeyError(name)
    return scenes.cornell((res, res))


def median(xs):
    return statistics.median(xs)


def time_denoise(r, color, guides, var, out, vout, warmup, reps):
    for _ in range(warmup):
        r.denoise(color, guides, var, out=out, var_out=vout)
    rows, walls = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        _, _, st = r.denoise(color, guides, var, out=out, var_out=vout)
        walls.append((time.perf_counter() - t0) * 1e3)
        rows.append(st)
    n = rows[0]["passes"]
    return {"form": rows[0]["form"], "pass_ms": [median(s["pass_ms"][i] for s in rows) for i in range(n)],
            "pass_ms_min": [min(s["pass_ms"][i] for s in rows) for i in range(n)],
            "pass_ms_max": [max(s["pass_ms"][i] for s in rows) for i in range(n)],
            "kernel_ms_min": min(s["kernel_ms"] for s in rows), "kernel_ms_max": max(s["kernel_ms"] for s in rows),
            "pack_ms": median(s["pack_ms"] for s in rows), "kernel_ms": median(s["kernel_ms"] for s in rows),
            "call_ms": median(walls), "reps": reps}


def time_copy(nbytes, warmup, reps):
    import torch
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    ms = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return median(ms)


def bench_scene(name, res, spp, depth, warmup, reps):
    import torch
    import ptamd
    sc = make_scene(name, res)
    cam = ptamd.Camera.from_spec(sc.camera)
    r = ptamd.Renderer(0)
    r.set_scene(ptamd.BVH.from_scene(sc))
    r.prepare()
    dev = torch.device("cuda", 0)
    noisy = torch.empty((res, res, 3), dtype=torch.float32, device=dev)
    _, mom, _ = r.render_moments(cam, 0, spp, depth, out=noisy, want=("sum", "sumsq"))
    aov, _ = r.aov(cam, sample=0, device=True)
    guides = ptamd.denoise_guides(aov)
    var = r.moments_variance(mom["sum"], mom["sumsq"], spp)
    outs = {}
    lines = {}
    for form in ("0", "1"):
        os.environ["PT_DENOISE_LDS"] = form
        out, vout = torch.empty_like(noisy), torch.empty_like(noisy)
        lines["direct" if form == "0" else "lds1"] = time_denoise(r, noisy, guides, var, out, vout, warmup, reps)
        outs[form] = (out, vout)
    del os.environ["PT_DENOISE_LDS"]
    for a, b in zip(outs["0"], outs["1"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the two forms differ"
    out, vout = torch.empty_like(noisy), torch.empty_like(noisy)
    lines["default"] = time_denoise(r, noisy, guides, var, out, vout, warmup, reps)
    assert torch.equal(out.view(torch.int32), outs["0"][0].view(torch.int32))
    img = torch.empty_like(noisy)
    rk, rw = [], []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        _, st = r.render(cam, spp, depth, out=img)
        if i >= warmup:
            rk.append(st["kernel_ms"])
            rw.append((time.perf_counter() - t0) * 1e3)
    copy_ms = time_copy(48 * res * res, warmup, reps)
    finite = torch.isfinite(outs["0"][0]).all().item()
    r.close()
    d = lines["default"]
    return {"scene": sc.name, "label": name, "tris": len(sc.tris), "res": [res, res], "spp": spp, "depth": depth,
            "device": torch.cuda.get_device_name(0), "denoise": lines,
            "render": {"kernel_ms": median(rk), "call_ms": median(rw)},
            "copy_48B_per_pixel_ms": copy_ms, "pass_bytes_per_pixel": 96, "output_finite": bool(finite),
            "default_kernel_over_render_kernel": d["kernel_ms"] / median(rk),
            "default_pass_over_copy": [p / copy_ms for p in d["pass_ms"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,sphere223")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        res = bench_scene(name, args.res, args.spp, args.depth, args.warmup, args.reps)
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
