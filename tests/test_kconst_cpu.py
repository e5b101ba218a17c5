"""The flat block's LDS layout (pt_flatlds.h) and the constants of the scene kernel's source
(PT_KCONST), without a device."""
import ctypes as C
import re

import pytest

import ptamd
from ptamd import scenes

BLOCK, WAVES = 256, 4
NAMES = ("tris", "mats", "next_ray", "best", "next_at", "boxtab", "queues", "rec_tri", "rec_cos", "bytes")
ALIGN = {"tris": 16, "mats": 16, "next_ray": 16, "best": 8, "next_at": 4, "boxtab": 2, "queues": 8, "rec_tri": 8,
         "rec_cos": 8}


def _layout(num_tris, box_tab_bytes, queue, rec):
    out = (C.c_uint32 * 10)()
    assert ptamd.lib().pt_debug_flat_lds(num_tris, box_tab_bytes, queue, rec, out) == 0
    return dict(zip(NAMES, out))


def _sizes(num_tris, box_tab_bytes, queue, rec):
    return {"tris": 16 * 3 * num_tris, "mats": 16 * 2 * num_tris, "next_ray": 16 * BLOCK, "best": 8 * BLOCK,
            "next_at": 4 * BLOCK, "boxtab": box_tab_bytes, "queues": 2 * WAVES * queue, "rec_tri": 2 * BLOCK * rec,
            "rec_cos": 4 * BLOCK * rec}


@pytest.mark.parametrize("num_tris", [1, 2, 12, 31, 32, 33, 34, 36, 63, 64, 500, 2000])
def test_layout_regions_aligned_disjoint_and_end_at_the_block_size(num_tris):
    """Every region starts at its alignment, none overlaps another, the last ends exactly at the
    bytes plan_flat asks of the launch, and only alignment padding (< 8 B) is added to the sum of
    the regions; the arrays a scene fixes do not move with the depth or the queue size."""
    fixed = None
    for box_tab_bytes in (0, 4, 40, 44):
        for depth in range(1, 17):
            rec = max(1, depth - 1)
            for queue in list(range(0, 513, 28 * 4)) + [4, 16, 64, 508, 512]:
                lay = _layout(num_tris, box_tab_bytes, queue, rec)
                size = _sizes(num_tris, box_tab_bytes, queue, rec)
                spans = sorted((lay[n], lay[n] + size[n], n) for n in size)
                for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
                    assert a1 <= b0, (an, bn, lay)
                for n, al in ALIGN.items():
                    assert lay[n] % al == 0, (n, lay)
                assert spans[0][0] == 0
                assert spans[-1][1] == lay["bytes"], lay
                assert 0 <= lay["bytes"] - sum(size.values()) < 8
                head = tuple(lay[n] for n in ("tris", "mats", "next_ray", "best", "next_at", "boxtab", "queues"))
                if box_tab_bytes == 0:
                    fixed = fixed or head
                    assert head == fixed  # scene-fixed: the same for every depth and queue size
                # the launch-sized regions come last
                assert lay["queues"] < lay["rec_tri"] or queue == 0
                assert max(lay[n] for n in ("tris", "mats", "next_ray", "best", "next_at", "boxtab")) <= lay["queues"]


def test_layout_hook_rejects_negative_sizes():
    out = (C.c_uint32 * 10)()
    assert ptamd.lib().pt_debug_flat_lds(-1, 0, 0, 1, out) != 0


def _source(scene):
    ref = ptamd._SceneRef(ptamd.BVH.from_scene(scene))
    buf = C.create_string_buffer(1 << 20)
    n = ptamd.lib().pt_rtc_check(C.byref(ref.s), buf, len(buf))
    assert n > 0, ptamd.lib().pt_last_error().decode()
    return buf.value.decode()


def _consts(src):
    m = re.search(r"kNumTri4 = (\d+), kNumMat4 = (\d+), kBoxTabBytes = (\d+), kThetaLanes = (\d+);\s*"
                  r"static constexpr bool kPairs = (true|false);", src)
    assert m, "the generated source holds no baked constants"
    return {"num_tri4": int(m.group(1)), "num_mat4": int(m.group(2)), "box_tab_bytes": int(m.group(3)),
            "theta_lanes": int(m.group(4)), "pairs": m.group(5) == "true"}


@pytest.mark.parametrize("name,theta", [("cornell", 0), ("mcornell", 32)])
def test_scene_kernel_source_carries_the_plans_constants(name, theta):
    """pt_rtc_check's source (the generator pt_ctx_set_scene uses) holds what the launch plan
    computes for the scene: 3 and 2 float4 per triangle, no box table, the pair queues on, and the
    theta table's lane bound (32 with a SPECULAR material, else 0: the table path is compiled out).
    The macro is on by default and compiles (pt_rtc_check returned a code object)."""
    sc = scenes.cornell((8, 8)) if name == "cornell" else scenes.modified_cornell(0.3, (8, 8))
    src = _source(sc)
    n = len(sc.tris)
    assert _consts(src) == {"num_tri4": 3 * n, "num_mat4": 2 * n, "box_tab_bytes": 0, "theta_lanes": theta, "pairs": True}
    assert "#ifndef PT_KCONST\n#define PT_KCONST 1\n#endif" in src
    assert "static constexpr bool kBaked = PT_KCONST != 0;" in src
    assert "#define PT_KCONST 0" not in src


def test_macro_off_and_hooks_reach_the_source(monkeypatch):
    """PT_RTC_DEFINES=PT_KCONST=0 defines the macro before its default, and the constants follow the
    hooks read when the source is made (PT_PAIRS, PT_THETA_LANES)."""
    sc = scenes.modified_cornell(0.3, (8, 8))
    monkeypatch.setenv("PT_RTC_DEFINES", "PT_KCONST=0")
    src = _source(sc)
    assert src.index("#define PT_KCONST 0\n") < src.index("#ifndef PT_KCONST")
    monkeypatch.delenv("PT_RTC_DEFINES")
    monkeypatch.setenv("PT_PAIRS", "0")
    monkeypatch.setenv("PT_THETA_LANES", "0")
    got = _consts(_source(sc))
    assert got["pairs"] is False and got["theta_lanes"] == 0
