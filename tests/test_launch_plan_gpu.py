"""The launch plan of a render (test hook pt_debug_ctx_plan) on every kernel family and every
shrink / batching rule, against tests/golden/launch_plans.json: recorded on an MI355X from the
arithmetic as it stood before the host code was split into plan / buffers / launch steps, so a
restructuring of the host code that moves any figure shows here. The four figures of the last
launch that follow from the CU count (grid, chunk, static_items, acc_every) are recomputed
from the returned num_cus and blocks_per_cu by the pool rule restated in tests/_plans.py.

Where the fixture comes from: the hook and the split of the host code arrived in one commit, so
no revision holds the hook on the old render_range. tests/golden/launch_plans_hook.patch is that
state: applied to commit 5f9c6c1 (the last one with the 615-line render_range) it adds only the
hook, a few stores from render_range's locals, and its binding. The fixture was recorded from
that tree. To audit it, check out 5f9c6c1, apply the patch, take tests/_plans.py and this file
from here, build, and run `python tests/test_launch_plan_gpu.py OUT.json` on an MI355X: OUT.json
equals tests/golden/launch_plans.json. Record from that tree only, never from this one."""
import json
import os

import pytest

import _plans
import _refwalk as RW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")
POOL_KEYS = ("grid", "chunk", "static_items", "acc_every")
# three fused launches of 12 samples and a tail of 3 at 32 x 32 pixels: the automatic batch is
# 24 samples' slab (24 * 12 B * 1024 pixels), halved for the two alternating slabs
FUSED = {"PT_BATCH_BYTES": str(24 * 12 * 32 * 32), "PT_TAIL_DIV": "4"}

# id: (scene, (W, H), samples, depth, hooks, render arguments)
CASES = {
    "cornell_rtc": ("cornell", (64, 64), 16, 5, {}, {}),
    "modified_cornell_rtc": ("modified_cornell", (64, 64), 16, 5, {}, {}),
    "cornell_depth8": ("cornell", (64, 64), 16, 8, {}, {}),
    "cornell_table_fast": ("cornell", (64, 64), 16, 5, {"PT_RTC": "0"}, {}),
    "cornell_table": ("cornell", (64, 64), 16, 5, {"PT_RTC": "0", "PT_FLAT_FAST": "0"}, {}),
    "cornell_no_pairs": ("cornell", (64, 64), 16, 5, {"PT_PAIRS": "0"}, {}),
    "cornell_pair_queue16": ("cornell", (64, 64), 16, 5, {"PT_PAIR_QUEUE": "16"}, {}),
    "cornell_tree_lds": ("cornell", (64, 64), 16, 5, {"PT_FLAT": "0", "PT_WIDE": "0"}, {}),
    "cornell_tree_global": ("cornell", (64, 64), 16, 5, {"PT_FLAT": "0", "PT_WIDE": "0", "PT_LDS_SCENE_BYTES": "0"}, {}),
    "cornell_wide": ("cornell", (64, 64), 16, 5, {"PT_WIDE": "1"}, {}),
    "cornell_wide_umat_global": ("cornell", (64, 64), 16, 5, {"PT_WIDE": "1", "PT_UMAT_LDS_MAX": "0"}, {}),
    "random300_wide": ("random_7_300", (64, 64), 16, 5, {"PT_WIDE": "1"}, {}),
    # the two cases below that the issue names pin nothing beyond random300_wide: the scene's 62 wide
    # nodes all fit (no shrink), and its 300 materials are over the LDS limit with or without the hook;
    # random1500_wide_top64k and cornell_wide_umat_global reach those rules
    "random300_wide_top64k": ("random_7_300", (64, 64), 16, 5, {"PT_WIDE": "1", "PT_WIDE_TOP_BYTES": "65536"}, {}),
    # 310 wide nodes, all of them allowed in LDS: the top-of-tree shrink loop has to drop most
    "random1500_wide_top64k": ("random_7_1500", (64, 64), 16, 5, {"PT_WIDE": "1", "PT_WIDE_TOP_BYTES": "65536"}, {}),
    "random300_wide_umat_global": ("random_7_300", (64, 64), 16, 5, {"PT_WIDE": "1", "PT_UMAT_LDS_MAX": "0"}, {}),
    "random300_wide_ranges": ("random_7_300", (64, 64), 16, 5, {"PT_WIDE": "1", "PT_WIDE_SINGLE": "0"}, {}),
    "cornell_fused_tail": ("cornell", (32, 32), 40, 5, FUSED, {}),
    "cornell_fused_remainder": ("cornell", (32, 32), 40, 5, {"PT_BATCH_BYTES": FUSED["PT_BATCH_BYTES"]}, {}),
    "cornell_unfused": ("cornell", (32, 32), 40, 5, dict(FUSED, PT_FUSED_ACC="0"), {}),
    "cornell_fused_batch12": ("cornell", (32, 32), 40, 5, FUSED, {"batch_spp": 12}),
    "cornell_batch16_over_budget": ("cornell", (32, 32), 40, 5, FUSED, {"batch_spp": 16}),
    "cornell_fused_dense": ("cornell", (32, 32), 40, 5, dict(FUSED, PT_FLAGS="0"), {}),
    "cornell_part_1_of_2": ("cornell", (64, 64), 16, 5, {}, {"part_index": 1, "part_count": 2, "band_rows": 4}),
    "cornell_progressive": ("cornell", (64, 64), 16, 5, {}, {"s_first": 6}),
}


def _scene(name, res):
    if name == "modified_cornell":
        from ptamd import scenes
        return scenes.modified_cornell(0.3, tuple(res))
    return RW.make_scene(name, res)


def run_case(case, setenv, delenv):
    """The plan of the case's (last) render, on a context of its own: the hooks that pick the
    scene's kernels are read when the scene is set."""
    import ptamd
    name, res, spp, depth, hooks, args = CASES[case]
    for k, v in hooks.items():
        setenv(k, v)
    r = ptamd.Renderer(0)
    try:
        sc = _scene(name, res)
        r.set_scene(ptamd.BVH.from_scene(sc))
        r.prepare()
        cam = ptamd.Camera.from_spec(sc.camera)
        args = dict(args)
        s_first = args.pop("s_first", 0)
        if s_first:
            r.render_progressive(cam, 0, s_first, depth, **args)
            _, st = r.render_progressive(cam, s_first, spp - s_first, depth, **args)
        else:
            _, st = r.render(cam, spp, depth, **args)
        plan = r.plan()
        rows = r.part_rows(res[1], args.get("part_index", 0), args.get("part_count", 1), args.get("band_rows", 1))
    finally:
        r.close()
        for k in hooks:
            delenv(k)
    assert plan["kernel_path"] == st["kernel_path"] and plan["trace_launches"] == st["trace_launches"]
    return plan, {"npix": rows * res[0], "s_lo": s_first, "spp": spp}


def expected_pool(plan, shape):
    """grid, chunk, static_items and acc_every of the last launch, from the plan's other fields."""
    samples = _plans.launch_samples(shape["s_lo"], shape["spp"], plan["batch"], plan["tail"])
    assert len(samples) == plan["trace_launches"]
    items = -(-samples[-1] // plan["per_item"]) * shape["npix"]
    summing = plan["fused"] and len(samples) > 1
    return _plans.pool(items, plan["blocks_per_cu"], plan["num_cus"], 512 if plan["flat"] else 128,
                       acc_npix=shape["npix"] if summing else 0)


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_plan(case, recorded, monkeypatch):
    plan, shape = run_case(case, monkeypatch.setenv, monkeypatch.delenv)
    want = recorded[case]
    print(case, plan)
    assert {k: v for k, v in plan.items() if k not in POOL_KEYS} == {k: v for k, v in want.items() if k not in POOL_KEYS}
    assert {k: plan[k] for k in POOL_KEYS} == expected_pool(plan, shape)


def test_recorded_cases_cover_the_rules(recorded):
    """The fixture holds what each case is there for (a case that no longer reaches its rule
    would pin nothing)."""
    assert set(recorded) == set(CASES)
    R = recorded
    assert R["cornell_rtc"]["kernel_path"] == 3 and R["cornell_rtc"]["pair_queue"] == 512
    assert R["modified_cornell_rtc"]["pair_queue"] == 480 > R["cornell_depth8"]["pair_queue"] >= 256
    assert R["cornell_table_fast"]["kernel_path"] == 5 and R["cornell_table"]["kernel_path"] == 2
    assert R["cornell_no_pairs"]["pairs"] == 0 and R["cornell_pair_queue16"]["pair_queue"] == 16
    assert R["cornell_tree_lds"]["kernel_path"] == 1 and R["cornell_tree_global"]["kernel_path"] == 0
    wide = R["random300_wide"]
    assert wide["kernel_path"] == 4 and 0 < wide["wide_top"] < R["random300_wide_top64k"]["wide_top"]
    # the shrink loop keeps the 6 blocks of 161,280 / 6 = 26,880 B, and one more 128-B node would not
    shrunk = R["random1500_wide_top64k"]
    assert 0 < shrunk["wide_top"] < 310 and 26880 - 128 < shrunk["lds_bytes"] <= 26880 and shrunk["blocks_per_cu"] == 6
    assert R["cornell_wide"]["lds_scene"] == 1 and R["cornell_wide_umat_global"]["lds_scene"] == 0
    assert R["random300_wide_ranges"]["lds_bytes"] > wide["lds_bytes"]
    tail = R["cornell_fused_tail"]
    assert (tail["fused"], tail["batch"], tail["tail"], tail["trace_launches"], tail["flags_pm"]) == (1, 12, 3, 5, 1)
    assert tail["acc_every"] >= 1 and R["cornell_fused_remainder"]["tail"] == 0
    assert R["cornell_unfused"]["fused"] == 0 and R["cornell_unfused"]["flags_pm"] == 0
    assert R["cornell_fused_batch12"]["fused"] == 1 and R["cornell_batch16_over_budget"]["fused"] == 0
    assert R["cornell_fused_dense"]["flags_pm"] == -1
    assert R["cornell_progressive"]["trace_launches"] == 1


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pathtracer-cpp_amd"))
    os.environ["PT_TEST_HOOKS"] = "1"
    os.environ["PT_RTC_WAIT"] = "1"
    out = {}
    for case_id in sorted(CASES):
        out[case_id], shape_ = run_case(case_id, os.environ.__setitem__, os.environ.__delitem__)
        assert {k: out[case_id][k] for k in POOL_KEYS} == expected_pool(out[case_id], shape_), case_id
        print(case_id, out[case_id], flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
