#!/usr/bin/env python3
"""What the temporal reprojection costs: Renderer.temporal_accumulate beside one a-trous pass, a
device copy and the whole Renderer.render_temporal frame.

For Cornell and sphere223_in_cornell at 1024^2, depth 5, in one process: a frame of --spp samples is
rendered with its moments at the scene's camera and accumulated into a history; a second frame is
rendered from a camera translated by --shift pixels (at the depth of the room's middle) along x.
Then Renderer.temporal_accumulate of the second frame onto that history, on device tensors in
sample mode, `--reps` times after a warm-up: the median kernel time with the smallest and the
largest beside it, the call's wall time and the fraction of pixels that reused their history.
Beside it, from the same process: one stride-1 a-trous pass (Renderer.denoise with passes=1 on the
accumulated frame: its pass kernel and its pack kernel), a device-to-device copy of 102 bytes per
pixel, which moves the 204 bytes per pixel the call must read (68 of the current frame, 68 of the
previous history) and write (68 of the next one), and the whole render_temporal frame at --spp
along a path of such steps (its wall time and its parts). Writes <out>/<scene>.json (default
profiles/temporal) and prints each as one JSON line.

    python3 scripts/temporal_bench.py [--scenes cornell,sphere223] [--res 1024] [--spp 4]
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


def make_scene(name, res):
    from ptamd import scenes
    if name.startswith("sphere"):
        return scenes.sphere_in_cornell(int(name[len("sphere"):]), (res, res))
    if name != "cornell":
        raise KeyError(name)
    return scenes.cornell((res, res))


def median(xs):
    return statistics.median(xs)


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


FRAME_BYTES = 4 * (3 + 3 + 3 + 1 + 1 + 3 + 3)  # colour, var, normal, t, tri, emission, position
HIST_BYTES = 4 * (3 + 3 + 3 + 1 + 3 + 3 + 1)   # the seven planes of a history


def spread(xs):
    return {"median": median(xs), "min": min(xs), "max": max(xs)}


def moved(sc, dx):
    c = sc.camera
    return dataclasses.replace(c, pos=(c.pos[0] + dx, c.pos[1], c.pos[2]))


def frame(r, cam, spp, depth, seed):
    """(colour, variance, guides) of one frame as device tensors."""
    import torch
    import ptamd
    W, H = cam.res
    noisy = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    _, mom, _ = r.render_moments(cam, 0, spp, depth, seed=seed, out=noisy, want=("sum", "sumsq"))
    aov, _ = r.aov(cam, sample=0, seed=seed, device=True)
    return noisy, r.moments_variance(mom["sum"], mom["sumsq"], spp), ptamd.denoise_guides(aov)


def bench_scene(name, res, spp, depth, shift, warmup, reps):
    import torch
    import ptamd
    sc = make_scene(name, res)
    step = shift * 2 * 0.5773502691896257 / res * 780.0  # pixels -> units at z = 280 (fov 60 degrees, camera at z = -500)
    cam0, cam1 = ptamd.Camera.from_spec(sc.camera), ptamd.Camera.from_spec(moved(sc, step))
    r = ptamd.Renderer(0)
    r.set_scene(ptamd.BVH.from_scene(sc))
    r.prepare()
    c0, v0, g0 = frame(r, cam0, spp, depth, 1)
    hist, _ = r.temporal_accumulate(c0, g0, cam0, var=v0)
    c1, v1, g1 = frame(r, cam1, spp, depth, 2)
    out = ptamd.TemporalHistory.empty(res, res, like=c1)
    ks, walls, reused = [], [], 0
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        _, st = r.temporal_accumulate(c1, g1, cam1, hist, cam0, var=v1, out=out)
        if i >= warmup:
            ks.append(st["kernel_ms"])
            walls.append((time.perf_counter() - t0) * 1e3)
            reused = st["reused"]
    den, dvar = torch.empty_like(c1), torch.empty_like(c1)
    ps, packs = [], []
    for i in range(warmup + reps):
        _, _, st = r.denoise(out.color, g1, out.var, passes=1, out=den, var_out=dvar)
        if i >= warmup:
            ps.append(st["pass_ms"][0])
            packs.append(st["pack_ms"])
    form = st["form"][0]
    copy_bytes = (FRAME_BYTES + 2 * HIST_BYTES) // 2
    copy_ms = time_copy(copy_bytes * res * res, warmup, reps)
    img = torch.empty_like(c1)
    rows, fw = [], []
    for i in range(warmup + reps):
        cam = ptamd.Camera.from_spec(moved(sc, step * i))
        t0 = time.perf_counter()
        _, _, info = r.render_temporal(cam, spp, depth, seed=100 + i, reset=(i == 0), out=img)
        if i >= warmup:
            fw.append((time.perf_counter() - t0) * 1e3)
            rows.append(info)
    finite = torch.isfinite(img).all().item()
    r.close()
    k = spread(ks)
    return {"scene": sc.name, "label": name, "tris": len(sc.tris), "res": [res, res], "spp": spp, "depth": depth,
            "shift_pixels": shift, "device": torch.cuda.get_device_name(0), "reps": reps,
            "temporal": {"kernel_ms": k, "call_ms": median(walls), "reused": reused, "reused_fraction": reused / (res * res)},
            "atrous_stride1": {"form": form, "pass_ms": spread(ps), "pack_ms": median(packs)},
            "copy_ms": copy_ms, "copy_bytes_per_pixel": copy_bytes,
            "traffic_bytes_per_pixel": FRAME_BYTES + 2 * HIST_BYTES,
            "frame": {"call_ms": spread(fw), "render_ms": median(x["render_ms"] for x in rows),
                      "aov_ms": median(x["aov_ms"] for x in rows), "variance_ms": median(x["variance_ms"] for x in rows),
                      "temporal_kernel_ms": median(x["temporal"]["kernel_ms"] for x in rows),
                      "denoise_kernel_ms": median(x["denoise"]["kernel_ms"] for x in rows),
                      "reused_fraction": median(x["reused"] for x in rows) / (res * res)},
            "output_finite": bool(finite),
            "temporal_over_copy": k["median"] / copy_ms, "temporal_over_atrous_pass": k["median"] / median(ps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,sphere223")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--shift", type=float, default=3.5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        res = bench_scene(name, args.res, args.spp, args.depth, args.shift, args.warmup, args.reps)
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
