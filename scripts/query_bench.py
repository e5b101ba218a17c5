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

--mode trace: path-tracing rates of pt_ctx_trace instead. The ray set is the same frame's camera
rays with the LCG states the render's samples have after their two camera draws (device
buffers), depth 5, 1 and 16 samples per ray; beside it pt_ctx_render of the same frame and
samples forced to the binary tree walk (PT_FLAT=0 PT_WIDE=0: the same walk and shading, its own
camera rays, flagged slab and fused accumulation) and the render on its default kernel. At one
sample the two images are compared bit for bit before anything is timed (with 16 the render
jitters a camera ray per sample, the trace repeats sample 0's). Mray/s = traced segments / kernel
time (trace: the path kernel alone; its in-order sum pass is reported beside it). Writes
<out>/<scene>.json (default profiles/paths).

--mode grad: pt_ctx_trace_grad (rgb and both gradients, device buffers, a seeded grad_rgb) beside
pt_ctx_trace on the same ray set, states, depth and samples as --mode trace, timed in turn on the
same visit. Mray/s = traced segments / the path kernel's time; the table form that ran is
reported, and where it is the per-block LDS table the global-atomics form (PT_GRAD_LDS=0) is timed
too, with its atomic bytes per second (8 B per non-zero channel added). The forward values are
compared bit for bit before anything is timed. Writes <out>/<scene>.json (default profiles/grad).

--mode nee_grad: pt_ctx_trace_nee_grad (rgb and both gradients, device buffers, dLoss/d rgb = 1,
the weighted estimator) beside pt_ctx_trace_nee_opt and pt_ctx_trace_grad on the same ray set,
depth and samples (default seeding), timed in turn on the same visit: the wall time of each call,
--reps times after a warm-up, as its median with the smallest and the largest beside it, and the
path kernel's time likewise. The forward values are compared bit for bit with trace_nee's before
anything is timed. Then the variance over --seeds independent seeds (one sample a ray) of d emit
summed over the light's triangles and of d color of the wall triangle with the largest gradient,
for trace_nee_grad and for trace_grad, and variance x wall ms of either. Writes <out>/<scene>.json
(default profiles/nee_grad).

--mode render_grad: one Renderer.render_grad call (pt_ctx_render_grad / pt_ctx_render_nee_grad,
device buffers, a seeded dLoss/d image, --spp samples a pixel) beside what it replaces, the
per-sample loop: the AOV rays of sample s, pt_sample_seed stepped twice, trace_grad(samples=1) with
grad_rgb / spp, the float64 tables and the float32 image added on the device. Both estimators (plain,
and light sampling with the weights), each timed as forward + gradients and as gradients only; the
wall time of each, --reps times after a warm-up, in turn, twice, as median / min / max. The forward
images are compared bit for bit and the gradients to 1e-9 relative before anything is timed. With a
library that lacks the new entry points (PT_LIB = an older build) only the loop is timed: its
run-to-run spread on the code the call replaces. Writes <out>/<scene>.json (default
profiles/render_grad).
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


def mix32(x):
    """pt_mix32 (include/pt_hip.h) on uint32 arrays."""
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def camera_states(npix, spp, seed):
    """(npix, spp) uint32: pt_sample_seed(pixel, s, seed) advanced by the camera's two LCG draws."""
    with np.errstate(over="ignore"):
        st = mix32(mix32(np.uint32(seed) * np.ones(1, np.uint32))[0] ^ np.arange(npix, dtype=np.uint32))
        st = mix32(st[:, None] + np.arange(spp, dtype=np.uint32)[None, :])
        for _ in range(2):
            st = st * np.uint32(1664525) + np.uint32(1013904223)
    return np.ascontiguousarray(st)


def bench_trace_scene(name, res, min_ms, warmup, depth=5):
    import torch
    import ptamd
    from ptamd import scenes
    sc = scenes.cornell((res, res)) if name == "cornell" else scenes.sphere_in_cornell(int(name[len("sphere"):]), (res, res))
    bvh = ptamd.BVH.from_scene(sc)
    cam = ptamd.Camera.from_spec(sc.camera)
    r = ptamd.Renderer(0)
    r.set_scene(bvh)
    r.prepare()
    aov, _ = r.aov(cam, sample=0, channels=("ray",))
    rays = aov["ray"].reshape(-1, 6)
    n = rays.shape[0]
    dev = torch.device("cuda", 0)
    to = torch.from_numpy(np.ascontiguousarray(rays[:, 0:3])).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(rays[:, 3:6])).to(dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    frame = torch.empty(res * res * 3, dtype=torch.float32, device=dev)
    lines = {}
    placement = None
    for spp in (1, 16):
        states = torch.from_numpy(camera_states(n, spp, ptamd.PT_SEED).view(np.int32)).to(dev)
        info = {}

        def trace_call():
            _, st = r.trace(to, td, depth, samples=spp, states=states, out=out)
            info.update(st)
            return st["rays"], st["kernel_ms"]

        def render_call(tree):
            if tree:
                os.environ["PT_FLAT"], os.environ["PT_WIDE"] = "0", "0"
            try:
                _, st = r.render(cam, spp, depth, out=frame)
            finally:
                os.environ.pop("PT_FLAT", None)
                os.environ.pop("PT_WIDE", None)
            info["kernel"] = ptamd._lib.pt_stats.PATHS.get(st["kernel_path"], str(st["kernel_path"]))
            info["render_reduce_ms"] = st["reduce_ms"]
            return st["rays"], st["kernel_ms"]

        # the run checks itself at one sample (the ray set is sample 0's camera rays: with more
        # samples the render jitters a ray per sample, the trace repeats the one it was given):
        # same rays, same states, same bits, same segment count
        t_rays, _ = trace_call()
        r_rays, _ = render_call(True)
        if spp == 1:
            assert t_rays == r_rays and torch.equal(out.reshape(-1).view(torch.int32), frame.view(torch.int32)), \
                f"{name}: trace and tree-walk render differ"
        key = f"trace_spp{spp}"
        lines[key] = timed(trace_call, warmup, min_ms)
        lines[key].update(sum_pass_ms_per_call=info["reduce_ms"], launches=info["launches"],
                          call_total_ms=info["total_ms"])
        placement = {k: info[k] for k in ("lds_scene", "lds_stack", "lds_records")}
        for tree in (True, False):
            key = f"render_{'tree' if tree else 'default'}_spp{spp}"
            lines[key] = timed(lambda: render_call(tree), max(1, warmup // 2), min_ms)
            lines[key].update(kernel=info["kernel"], sum_pass_ms_per_call=info["render_reduce_ms"])
        for k in (f"trace_spp{spp}", f"render_default_spp{spp}"):
            lines[k]["ratio_to_render_tree"] = lines[k]["mrays_per_s"] / lines[f"render_tree_spp{spp}"]["mrays_per_s"]
    r.close()
    return {"scene": sc.name, "tris": len(sc.tris), "res": [res, res], "rays": n, "depth": depth, "placement": placement,
            "min_kernel_ms": min_ms, "device": torch.cuda.get_device_name(0), "lines": lines}


def bench_grad_scene(name, res, min_ms, warmup, depth=5):
    import torch
    import ptamd
    from ptamd import scenes
    sc = scenes.cornell((res, res)) if name == "cornell" else scenes.sphere_in_cornell(int(name[len("sphere"):]), (res, res))
    bvh = ptamd.BVH.from_scene(sc)
    cam = ptamd.Camera.from_spec(sc.camera)
    r = ptamd.Renderer(0)
    r.set_scene(bvh)
    r.prepare()
    aov, _ = r.aov(cam, sample=0, channels=("ray",))
    rays = aov["ray"].reshape(-1, 6)
    n = rays.shape[0]
    dev = torch.device("cuda", 0)
    to = torch.from_numpy(np.ascontiguousarray(rays[:, 0:3])).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(rays[:, 3:6])).to(dev)
    tg = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (n, 3)).astype(np.float32)).to(dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    lines = {}
    forms = {}
    for spp in (1, 16):
        states = torch.from_numpy(camera_states(n, spp, ptamd.PT_SEED).view(np.int32)).to(dev)
        info = {}

        def trace_call():
            _, st = r.trace(to, td, depth, samples=spp, states=states, out=out)
            info["trace"] = st
            return st["rays"], st["kernel_ms"]

        def grad_call(global_form=False):
            if global_form:
                os.environ["PT_GRAD_LDS"] = "0"
            try:
                res_, st = r.trace_grad(to, td, tg, depth, samples=spp, states=states)
            finally:
                os.environ.pop("PT_GRAD_LDS", None)
            info["grad"], info["res"] = st, res_
            return st["rays"], st["kernel_ms"]

        t_rays, _ = trace_call()
        g_rays, _ = grad_call()
        assert t_rays == g_rays and torch.equal(out.view(torch.int32), info["res"]["rgb"].view(torch.int32)), \
            f"{name}: trace and trace_grad forward values differ"
        nonzero = int((info["res"]["color"] != 0).sum() + (info["res"]["emit"] != 0).sum())
        lds = info["grad"]["lds_table"]
        forms[f"spp{spp}"] = "lds" if lds else "global"
        todo = [("trace", trace_call), ("grad", grad_call)] + ([("grad_global", lambda: grad_call(True))] if lds else [])
        for label, call in todo:
            key = f"{label}_spp{spp}"
            lines[key] = timed(call, warmup, min_ms)
            if label != "trace":
                st = info["grad"]
                lines[key].update(terms_per_call=st["terms"], grad_ms_per_call=st["grad_ms"], lds_table=st["lds_table"],
                                  sum_pass_ms_per_call=st["reduce_ms"], call_total_ms=st["total_ms"],
                                  nonzero_outputs=nonzero)
                lines[key]["ratio_to_trace"] = lines[key]["mrays_per_s"] / lines[f"trace_spp{spp}"]["mrays_per_s"]
                # an upper bound of the atomic bytes: 3 channels x 8 B per term (zero channels are skipped)
                lines[key]["term_gbytes_per_s"] = st["terms"] * 24 * lines[key]["calls"] / lines[key]["kernel_ms"] / 1e6
    placement = {k: info["grad"][k] for k in ("lds_scene", "lds_stack", "lds_records")}
    r.close()
    return {"scene": sc.name, "tris": len(sc.tris), "res": [res, res], "rays": n, "depth": depth, "placement": placement,
            "table_form": forms, "min_kernel_ms": min_ms, "device": torch.cuda.get_device_name(0), "lines": lines}


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]), "min": xs[0],
            "max": xs[-1]}


def bench_nee_grad_scene(name, res, warmup, reps, seeds, depth=5, spp=1):
    import torch
    import ptamd
    from ptamd import scenes
    sc = scenes.cornell((res, res)) if name == "cornell" else scenes.sphere_in_cornell(int(name[len("sphere"):]), (res, res))
    bvh = ptamd.BVH.from_scene(sc)
    cam = ptamd.Camera.from_spec(sc.camera)
    r = ptamd.Renderer(0)
    r.set_scene(bvh)
    r.prepare()
    aov, _ = r.aov(cam, sample=0, channels=("ray",))
    rays = aov["ray"].reshape(-1, 6)
    n = rays.shape[0]
    dev = torch.device("cuda", 0)
    to = torch.from_numpy(np.ascontiguousarray(rays[:, 0:3])).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(rays[:, 3:6])).to(dev)
    tg = torch.ones((n, 3), dtype=torch.float32, device=dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    last = {}

    def nee_call(seed=1):
        _, st = r.trace_nee(to, td, depth, samples=spp, seed=seed, out=out, mis=True)
        last["nee"] = st
        return st

    def grad_call(seed=1):
        res_, st = r.trace_grad(to, td, tg, depth, samples=spp, seed=seed)
        last["grad"], last["grad_res"] = st, res_
        return st

    def nee_grad_call(seed=1):
        res_, st = r.trace_nee_grad(to, td, tg, depth, samples=spp, seed=seed, mis=True)
        last["nee_grad"], last["nee_grad_res"] = st, res_
        return st

    nee_call()
    nee_grad_call()
    assert last["nee"]["rays"] == last["nee_grad"]["rays"] and \
        torch.equal(out.view(torch.int32), last["nee_grad_res"]["rgb"].view(torch.int32)), \
        f"{name}: trace_nee and trace_nee_grad forward values differ"

    def timed_wall(call):
        for _ in range(warmup):
            call()
        wall, kern = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            st = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(st["kernel_ms"])
        return {"wall_ms": spread(wall), "kernel_ms": spread(kern), "rays_per_call": st["rays"],
                "mrays_per_s": st["rays"] / spread(kern)["median"] / 1e3}

    lines = {}
    for _ in range(2):  # in turn, twice: the second round's figures are kept beside the first's
        for label, call in (("trace_nee", nee_call), ("trace_grad", grad_call), ("trace_nee_grad", nee_grad_call)):
            lines.setdefault(label, []).append(timed_wall(call))
    st = last["nee_grad"]
    for row in lines["trace_nee_grad"]:
        row.update(terms_per_call=st["terms"], grad_ms_per_call=st["grad_ms"], lds_table=st["lds_table"],
                   shadow_rays=st["shadow_rays"], light_draws=st["light_draws"])
    med = {k: spread([row["wall_ms"]["median"] for row in v])["median"] for k, v in lines.items()}
    ratios = {"nee_grad_over_trace_nee_ms": med["trace_nee_grad"] / med["trace_nee"],
              "nee_grad_over_trace_grad_ms": med["trace_nee_grad"] / med["trace_grad"]}
    # variance over independent seeds
    lights = torch.from_numpy(ptamd.scene_lights(bvh)["tri"].astype(np.int64)).to(dev)
    grad_call()
    wall_tri = int(torch.argmax(last["grad_res"]["color"].abs().amax(dim=1)))
    samples = {"trace_grad": [], "trace_nee_grad": []}
    for s in range(seeds):
        grad_call(seed=101 + s)
        nee_grad_call(seed=101 + s)
        for label, key in (("trace_grad", "grad_res"), ("trace_nee_grad", "nee_grad_res")):
            g = last[key]
            samples[label].append(torch.cat([g["emit"][lights].sum(dim=0), g["color"][wall_tri]]).cpu().numpy())
    var = {}
    for label, xs in samples.items():
        xs = np.stack(xs)
        var[label] = {"mean_d_emit_light": xs[:, 0:3].mean(axis=0).tolist(), "var_d_emit_light": xs[:, 0:3].var(axis=0, ddof=1).tolist(),
                      "mean_d_color_wall": xs[:, 3:6].mean(axis=0).tolist(), "var_d_color_wall": xs[:, 3:6].var(axis=0, ddof=1).tolist()}
    ratio = {}
    for key in ("var_d_emit_light", "var_d_color_wall"):
        a, b = np.array(var["trace_nee_grad"][key]), np.array(var["trace_grad"][key])
        ratio[key] = (a / b).tolist()
        ratio[key + "_x_ms"] = (a * med["trace_nee_grad"] / (b * med["trace_grad"])).tolist()
    placement = {k: st[k] for k in ("lds_scene", "lds_stack", "lds_records", "lds_table")}
    r.close()
    return {"scene": sc.name, "tris": len(sc.tris), "res": [res, res], "rays": n, "depth": depth, "spp": spp, "mis": True,
            "placement": placement, "warmup": warmup, "reps": reps, "device": torch.cuda.get_device_name(0), "lines": lines,
            "wall_ms_median": med, "ratios": ratios,
            "variance": {"seeds": seeds, "wall_triangle": wall_tri, "lights": int(lights.numel()), "estimators": var,
                         "nee_grad_over_trace_grad": ratio}}


def bench_render_grad_scene(name, res, warmup, reps, depth=5, spp=4):
    import torch
    import ptamd
    from ptamd import scenes
    sc = scenes.cornell((res, res)) if name == "cornell" else scenes.sphere_in_cornell(int(name[len("sphere"):]), (res, res))
    bvh = ptamd.BVH.from_scene(sc)
    cam = ptamd.Camera.from_spec(sc.camera)
    r = ptamd.Renderer(0)
    r.set_scene(bvh)
    r.prepare()
    dev = torch.device("cuda", 0)
    n = res * res
    G = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (res, res, 3)).astype(np.float32)).to(dev)
    gs = (G / np.float32(spp)).reshape(n, 3).contiguous()
    have_call = hasattr(ptamd.lib(), "pt_ctx_render_grad")
    last = {}

    def loop(mode, want_rgb):
        want = (("rgb",) if want_rgb else ()) + ("color", "emit")
        states = torch.from_numpy(camera_states(n, spp, 1).view(np.int32)).to(dev)
        acc = color = emit = None
        for s in range(spp):
            a, _ = r.aov(cam, sample=s, channels=("ray",), device=True)
            ray = a["ray"].reshape(n, 6)
            o, d = ray[:, 0:3].contiguous(), ray[:, 3:6].contiguous()
            st = states[:, s].contiguous()
            if mode == "plain":
                x, _ = r.trace_grad(o, d, gs, depth, states=st, want=want)
            else:
                x, _ = r.trace_nee_grad(o, d, gs, depth, states=st, want=want, mis=True)
            color = x["color"] if color is None else color + x["color"]
            emit = x["emit"] if emit is None else emit + x["emit"]
            if want_rgb:
                acc = x["rgb"] if acc is None else acc + x["rgb"]
        torch.cuda.synchronize()
        last["loop"] = {"color": color, "emit": emit, "rgb": (acc / np.float32(spp)).reshape(res, res, 3) if want_rgb else None}

    def call(mode, want_rgb):
        want = (("rgb",) if want_rgb else ()) + ("color", "emit")
        x, st = r.render_grad(cam, G, spp, depth, want=want, light_sampling=mode != "plain", mis=mode != "plain")
        last["call"], last["call_st"] = x, st

    def timed_wall(f, *a):
        for _ in range(warmup):
            f(*a)
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f(*a)
            wall.append((time.perf_counter() - t0) * 1e3)
        return spread(wall)

    lines, checks = {}, {}
    for mode in ("plain", "nee_mis"):
        if have_call:
            loop(mode, True)
            call(mode, True)
            a, b = last["loop"], last["call"]
            assert torch.equal(a["rgb"].view(torch.int32), b["rgb"].view(torch.int32)), f"{name} {mode}: forward images differ"
            rel = max(float(((a[k] - b[k]).abs().max() / b[k].abs().max())) for k in ("color", "emit"))
            assert rel < 1e-9, f"{name} {mode}: gradients differ by {rel}"
            checks[mode] = {"rgb_bits_equal": True, "grad_max_rel_diff": rel, "terms": last["call_st"]["terms"],
                            "rays": last["call_st"]["rays"], "launches": last["call_st"]["launches"],
                            "placement": {k: last["call_st"][k] for k in ("lds_scene", "lds_stack", "lds_records", "lds_table")}}
        for _ in range(2):  # in turn, twice
            for want_rgb in (True, False):
                tag = f"{mode}_{'forward_and_gradients' if want_rgb else 'gradients_only'}"
                lines.setdefault("loop_" + tag, []).append(timed_wall(loop, mode, want_rgb))
                if have_call:
                    lines.setdefault("call_" + tag, []).append(timed_wall(call, mode, want_rgb))
    med = {k: spread([row["median"] for row in v])["median"] for k, v in lines.items()}
    ratios = {k[len("call_"):]: med[k] / med["loop_" + k[len("call_"):]] for k in med if k.startswith("call_")}
    r.close()
    return {"scene": sc.name, "tris": len(sc.tris), "res": [res, res], "depth": depth, "spp": spp, "warmup": warmup, "reps": reps,
            "device": torch.cuda.get_device_name(0), "library_has_render_grad": have_call, "checks": checks, "wall_ms": lines,
            "wall_ms_median": med, "call_over_loop": ratios}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="cornell,sphere223")
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--min-ms", type=float, default=1000.0, help="kernel time per line")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--mode", choices=("query", "trace", "grad", "nee_grad", "render_grad"), default="query")
    ap.add_argument("--reps", type=int, default=9, help="--mode nee_grad, render_grad: timed calls per line")
    ap.add_argument("--spp", type=int, default=4, help="--mode render_grad: samples per pixel")
    ap.add_argument("--seeds", type=int, default=32, help="--mode nee_grad: independent seeds of the variance")
    ap.add_argument("--out", default=None, help="default profiles/query, profiles/paths with --mode trace, profiles/grad with --mode grad, "
                    "profiles/nee_grad with --mode nee_grad, profiles/render_grad with --mode render_grad")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", {"trace": "paths", "grad": "grad", "nee_grad": "nee_grad", "render_grad": "render_grad"}.get(args.mode, "query"))
    if args.mode in ("trace", "grad"):
        os.environ["PT_TEST_HOOKS"] = "1"  # PT_FLAT / PT_WIDE pick the yardstick's kernel, PT_GRAD_LDS the table form
    os.makedirs(args.out, exist_ok=True)
    for name in args.scenes.split(","):
        if args.mode == "render_grad":
            res = bench_render_grad_scene(name, args.res, args.warmup, args.reps, spp=args.spp)
        elif args.mode == "nee_grad":
            res = bench_nee_grad_scene(name, args.res, args.warmup, args.reps, args.seeds)
        elif args.mode == "grad":
            res = bench_grad_scene(name, args.res, args.min_ms, args.warmup)
        elif args.mode == "trace":
            res = bench_trace_scene(name, args.res, args.min_ms, args.warmup)
        else:
            res = bench_scene(name, args.res, args.min_ms, args.warmup, args.seed)
        with open(os.path.join(args.out, res["scene"] + ".json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
