#!/usr/bin/env python3
"""What light sampling costs and what it buys: Renderer.render_nee beside Renderer.render and
Renderer.trace at equal samples per pixel.

For Cornell, modified Cornell (roughness 0.3) and sphere223_in_cornell (99k triangles) at 1024^2,
depth 5, in one process per scene, for each entry of --spp (default 4 and 1024):

  * the wall time of render_nee, of Renderer.render (the scene's own render kernel: the
    scene-specialised flat kernel where there is one) and of Renderer.trace along sample 0's camera
    rays with the same number of samples per ray (the same binary walk without light sampling), each
    `--reps` times after a warm-up: the median with the smallest and the largest beside it, and the
    kernel times the calls report;
  * shadow segments per path and the segments of each estimator;
  * the mean per-pixel sample variance of both estimators, from the moments (sum, sumsq) of
    render_moments and render_nee: mean over pixels and channels of (Q - S^2 / n) / (n - 1);
  * variance x time, the figure of merit (lower is better), and the ratio of the two;
  * with --mis, the same columns for the weighted estimator (render_nee(mis=True), the balance
    heuristic of DESIGN.md §3.24): wall and kernel ms, shadow segments per path, variance,
    variance x time, and its time and variance over the unweighted estimator's.

Writes <out>/<scene>.json (default profiles/nee) and prints each as one JSON line.

    python3 scripts/nee_bench.py [--scenes cornell,mcornell,sphere223] [--res 1024] [--spp 4,1024] [--mis]
"""
import argparse
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
    if name == "mcornell":
        return scenes.modified_cornell(0.3, (res, res))
    if name != "cornell":
        raise KeyError(name)
    return scenes.cornell((res, res))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def timed(fn, warmup, reps):
    """fn() -> stats dict of a synchronous call; (wall ms spread, kernel ms spread, last stats)."""
    wall, kern, st = [], [], None
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        st = fn()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(st["kernel_ms"])
    return spread(wall), spread(kern), st


def mean_variance(mom, n):
    S, Q = mom["sum"].double(), mom["sumsq"].double()
    return float(((Q - S * S / n) / (n - 1)).clamp_min(0).mean().item())


def bench_scene(name, res, spps, depth, warmup, reps, reps_long, mis=False):
    import torch
    import ptamd
    sc = make_scene(name, res)
    cam = ptamd.Camera.from_spec(sc.camera)
    r = ptamd.Renderer(0)
    r.set_scene(ptamd.BVH.from_scene(sc))
    r.prepare()
    out = torch.empty((res, res, 3), dtype=torch.float32, device="cuda:0")
    aov, _ = r.aov(cam, sample=0, seed=1, channels=("ray",), device=True)
    org = aov["ray"][..., 0:3].reshape(-1, 3).contiguous()
    dirs = aov["ray"][..., 3:6].reshape(-1, 3).contiguous()
    rgb = torch.empty((res * res, 3), dtype=torch.float32, device="cuda:0")
    rows = []
    for spp in spps:
        n = reps if spp <= 64 else reps_long
        nee_w, nee_k, nee_st = timed(lambda: r.render_nee(cam, spp, depth, seed=1, out=out)[2], warmup, n)
        ren_w, ren_k, ren_st = timed(lambda: r.render(cam, spp, depth, seed=1, out=out)[1], warmup, n)
        tr_w, tr_k, tr_st = timed(lambda: r.trace(org, dirs, depth, samples=spp, seed=1, out=rgb)[1], warmup, n)
        _, mom_ref, _ = r.render_moments(cam, 0, spp, depth, seed=1, out=out, want=("sum", "sumsq"))
        v_ref = mean_variance(mom_ref, spp)
        del mom_ref
        _, mom_nee, _ = r.render_nee(cam, spp, depth, seed=1, out=out, want=("sum", "sumsq"))
        v_nee = mean_variance(mom_nee, spp)
        del mom_nee
        paths = res * res * spp
        rows.append({
            "spp": spp, "reps": n,
            "render_nee_ms": nee_w, "render_nee_kernel_ms": nee_k,
            "render_ms": ren_w, "render_kernel_ms": ren_k,
            "trace_ms": tr_w, "trace_kernel_ms": tr_k,
            "segments": {"render_nee": nee_st["rays"], "render": ren_st["rays"], "trace": tr_st["rays"]},
            "shadow_segments_per_path": nee_st["shadow_rays"] / paths,
            "light_draws_per_path": nee_st["light_draws"] / paths,
            "launches": nee_st["launches"], "lds_scene": nee_st["lds_scene"], "lds_stack": nee_st["lds_stack"],
            "sample_variance": {"render": v_ref, "render_nee": v_nee, "ratio": v_nee / v_ref if v_ref else None},
            "variance_x_ms": {"render": v_ref * ren_w["median"], "render_nee": v_nee * nee_w["median"],
                              "ratio": (v_nee * nee_w["median"]) / (v_ref * ren_w["median"]) if v_ref else None},
            "nee_over_render_ms": nee_w["median"] / ren_w["median"], "nee_over_trace_ms": nee_w["median"] / tr_w["median"]})
        if mis:
            mis_w, mis_k, mis_st = timed(lambda: r.render_nee(cam, spp, depth, seed=1, out=out, mis=True)[2], warmup, n)
            _, mom_mis, _ = r.render_nee(cam, spp, depth, seed=1, out=out, want=("sum", "sumsq"), mis=True)
            v_mis = mean_variance(mom_mis, spp)
            del mom_mis
            rows[-1].update({
                "render_nee_mis_ms": mis_w, "render_nee_mis_kernel_ms": mis_k,
                "mis_shadow_segments_per_path": mis_st["shadow_rays"] / paths,
                "mis_over_nee_ms": mis_w["median"] / nee_w["median"],
                "mis_over_nee_kernel_ms": mis_k["median"] / nee_k["median"]})
            rows[-1]["segments"]["render_nee_mis"] = mis_st["rays"]
            rows[-1]["sample_variance"].update(render_nee_mis=v_mis, mis_over_nee=v_mis / v_nee if v_nee else None)
            rows[-1]["variance_x_ms"].update(render_nee_mis=v_mis * mis_w["median"],
                                             mis_over_nee=(v_mis * mis_w["median"]) / (v_nee * nee_w["median"]) if v_nee else None)
    lights, area = nee_st["lights"], nee_st["light_area"]
    r.close()
    return {"scene": sc.name, "label": name, "tris": len(sc.tris), "res": [res, res], "depth": depth,
            "device": torch.cuda.get_device_name(0), "lights": lights, "light_area": area, "runs": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,mcornell,sphere223")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", default="4,1024")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--reps-long", type=int, default=31, help="repetitions of the runs above 64 spp")
    ap.add_argument("--mis", action="store_true", help="also measure the weighted estimator, render_nee(mis=True)")
    ap.add_argument("--out", default=None, help="default profiles/nee, with --mis profiles/mis")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mis" if args.mis else "nee")
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        res = bench_scene(name, args.res, [int(s) for s in args.spp.split(",")], args.depth, args.warmup, args.reps,
                          args.reps_long, args.mis)
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
