#!/usr/bin/env python3
"""What adaptive sampling saves: Renderer.render_adaptive beside the same call with
sparse_below = -1, which is render_converge (every pixel rendered to the last boundary).

For Cornell, Cornell with a small emission on every surface and sphere223_in_cornell at 1024^2,
depth 5, on one GPU in one process, at a target and max_samples where the run ends with a small
active tail. First the two results are compared: the pixels whose spp equals the converge run's
must be bit-equal in the image and the moments. Then the two calls are timed in turn on device
buffers, `--reps` times each after a warm-up (medians), and sum n_p is reported against npix * max
n_p. Last, the rate ratio behind the default switch point: one dense round and one per-pixel round
over every pixel that is not all zero (sparse_below = 1, a target nothing meets), rays per kernel
millisecond of each. Writes <out>/<scene>.json (default profiles/adaptive) and prints each file's
content as one JSON line.

    python3 scripts/adaptive_bench.py [--scenes cornell,cornell_glow,sphere223] [--res 1024]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathtracer-cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from moments_bench import make_scene  # noqa: E402

# rel, min_samples, max_samples per scene: a small tail of pixels is still active at max_samples.
# The dark scenes start at 512 samples: a pixel whose first min_samples samples are all zero counts
# as converged and would be frozen there, and at 64 samples 57 % of Cornell's pixels still are.
TARGETS = {"cornell": (0.5, 512, 8192), "cornell_glow": (0.1, 16, 1024), "sphere223": (0.5, 512, 8192)}
KEEP = ("rounds", "dense_rounds", "max_spp", "sparse_launches", "unconverged", "samples", "rays", "sparse_rays",
        "kernel_ms", "reduce_ms", "sparse_kernel_ms")


def bench_scene(name, res, depth, sparse_below, warmup, reps):
    import torch
    import ptamd
    rel, lo, hi = TARGETS[name]
    sc = make_scene(name, res)
    cam = ptamd.Camera.from_spec(sc.camera)
    r = ptamd.Renderer(0)
    r.set_scene(ptamd.BVH.from_scene(sc))
    r.prepare()
    dev = torch.device("cuda", 0)
    bufs = [torch.empty((res, res, 3), dtype=torch.float32, device=dev) for _ in range(2)]

    def call(below, out, want=()):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img, mom, spp, info = r.render_adaptive(cam, depth, rel, min_samples=lo, max_samples=hi, sparse_below=below,
                                                out=out, want=want)
        info["call_ms"] = (time.perf_counter() - t0) * 1e3
        return img, mom, spp, info

    cimg, cmom, cspp, cinfo = call(-1.0, bufs[0], ("sum", "sumsq"))
    aimg, amom, aspp, ainfo = call(sparse_below, bufs[1], ("sum", "sumsq"))
    assert int(cspp.min()) == int(cspp.max()) == cinfo["max_spp"]
    m = aspp == cspp
    assert torch.equal(aimg.view(torch.int32)[m], cimg.view(torch.int32)[m]), "image differs on pixels of equal spp"
    for k in ("sum", "sumsq"):
        assert torch.equal(amom[k].view(torch.int64)[m], cmom[k].view(torch.int64)[m]), k
    assert ainfo["samples"] == int(aspp.sum(dtype=torch.int64))
    kernel_path = r.plan()["kernel_path"]
    lines = {}
    for label, below, out in (("converge", -1.0, bufs[0]), ("adaptive", sparse_below, bufs[1])):
        lines[label] = []
    for i in range(warmup + reps):  # in turn
        for label, below, out in (("converge", -1.0, bufs[0]), ("adaptive", sparse_below, bufs[1])):
            info = call(below, out)[3]
            if i >= warmup:
                lines[label].append(info)
    npix = res * res
    summary = {}
    for label, rows in lines.items():
        summary[label] = {k: rows[0][k] for k in KEEP if k not in ("kernel_ms", "reduce_ms", "sparse_kernel_ms")}
        for k in ("call_ms", "kernel_ms", "reduce_ms", "sparse_kernel_ms"):
            summary[label][k] = statistics.median(x[k] for x in rows)
        summary[label]["call_ms_all"] = [x["call_ms"] for x in rows]
        summary[label]["uniform_samples"] = npix * rows[0]["max_spp"]
    # the rate ratio: 16 dense samples, then 16 per-pixel samples of every pixel that is not all zero
    rates = []
    for i in range(warmup + reps):
        info = r.render_adaptive(cam, depth, 1e-6, min_samples=16, max_samples=32, sparse_below=1.0, out=bufs[1], want=())[3]
        if i >= warmup and info["sparse_kernel_ms"] > 0:
            dense = (info["rays"] - info["sparse_rays"]) / (info["kernel_ms"] - info["sparse_kernel_ms"]) / 1e3
            sparse = info["sparse_rays"] / info["sparse_kernel_ms"] / 1e3
            rates.append((dense, sparse, info["samples"] / npix))
    rate = {"dense_mrays_per_s": statistics.median(x[0] for x in rates),
            "sparse_mrays_per_s": statistics.median(x[1] for x in rates),
            "mean_spp": rates[0][2]}
    rate["sparse_over_dense"] = rate["sparse_mrays_per_s"] / rate["dense_mrays_per_s"]
    rate["switch_constant_0p8"] = 0.8 * rate["sparse_over_dense"]
    r.close()
    return {"scene": sc.name, "label": name, "tris": len(sc.tris), "res": [res, res], "depth": depth, "rel": rel,
            "min_samples": lo, "max_samples": hi, "sparse_below": sparse_below, "kernel_path": kernel_path,
            "device": torch.cuda.get_device_name(0), "reps": reps, "lines": summary,
            "adaptive_over_converge_call": summary["adaptive"]["call_ms"] / summary["converge"]["call_ms"],
            "samples_over_uniform": summary["adaptive"]["samples"] / summary["adaptive"]["uniform_samples"],
            "rate": rate}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,cornell_glow,sphere223")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--sparse-below", type=float, default=0.0, help="0: the library's default")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        res = bench_scene(name, args.res, args.depth, args.sparse_below, args.warmup, args.reps)
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
