#!/usr/bin/env python3
"""Host overhead of a call along caller-supplied rays (Renderer.trace, trace_nee, trace_grad):
total_ms - kernel_ms - reduce_ms from the call's stats, 11 calls after 3 warm-ups, on the 1,048,576
camera rays of Cornell at 1024^2, 1 spp, depth 5, device tensors. ROOT: the checkout whose package
is measured (to compare two builds, run once per checkout); the figures are printed and written to
OUT/overhead_LABEL.json (profiles/caller_rays/parent_vs_branch.json holds the recorded ones).

  python scripts/caller_ray_overhead.py ROOT LABEL [OUT]"""
import json
import os
import statistics
import sys

root, label = os.path.abspath(sys.argv[1]), sys.argv[2]
out_dir = sys.argv[3] if len(sys.argv) > 3 else "."
sys.path.insert(0, os.path.join(root, "pathtracer-cpp_amd"))
import torch  # noqa: E402
import ptamd  # noqa: E402
from ptamd import scenes  # noqa: E402

assert os.path.abspath(ptamd.__file__).startswith(root), ptamd.__file__
sc = scenes.cornell((1024, 1024))
bvh = ptamd.BVH.from_scene(sc)
cam = ptamd.Camera.from_spec(sc.camera)
r = ptamd.Renderer(0)
r.set_scene(bvh)
aov, _ = r.aov(cam, sample=0, channels=("ray",), device=True)
ray = aov["ray"].reshape(-1, 6)
o, d = ray[:, 0:3].contiguous(), ray[:, 3:6].contiguous()
n = o.shape[0]
assert n == 1 << 20
torch.manual_seed(5)
g = (torch.rand((n, 3), device="cuda:0") * 2 - 1).contiguous()
out = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
calls = {
    "trace": lambda: r.trace(o, d, 5, out=out)[1],
    "trace_nee": lambda: r.trace_nee(o, d, 5, out=out)[1],
    "trace_grad": lambda: r.trace_grad(o, d, g, 5)[1],
}
res = {"label": label, "root": root}
for name, f in calls.items():
    for _ in range(3):
        f()
    rows = []
    for _ in range(11):
        st = f()
        rows.append({k: st[k] for k in ("total_ms", "kernel_ms", "reduce_ms", "launches", "rays") + (("grad_ms",) if "grad_ms" in st else ())})
    ov = [x["total_ms"] - x["kernel_ms"] - x["reduce_ms"] for x in rows]
    res[name] = {"overhead_ms": ov, "median": statistics.median(ov), "min": min(ov), "max": max(ov),
                 "kernel_ms_median": statistics.median(x["kernel_ms"] for x in rows),
                 "total_ms_median": statistics.median(x["total_ms"] for x in rows), "rows": rows}
    print(label, name, "overhead median %.4f ms  min %.4f  max %.4f  | kernel median %.3f ms, launches %d" %
          (res[name]["median"], min(ov), max(ov), res[name]["kernel_ms_median"], rows[0]["launches"]), flush=True)
r.close()
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"overhead_{label}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
