"""Caller-built trees on the host (no device): every transform of tests/_trees.py on Cornell,
modified Cornell and the 296-triangle sphere scene is a tree pt_scene_validate accepts, packs
the way the transform implies (reachable nodes, depth, flat leaves, wide tree and its
records), verifies exactly as a wide tree, and is walked by pt_bvh_intersect as the oracle
walks it. The oracle's own walk of caller nodes is pinned to the compiled reference by the
fixtures of tests/golden/gen_trees.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _oracle as O
import _refwalk as RW
import _treecases as TC
import _trees as T
from conftest import GOLDEN, load_golden, scene_hash

SCENES = ["cornell", "mcornell", "sphere12"]
ALL = TC.VARIANTS + (f"merged{TC.K_BIG}",)


@pytest.fixture(scope="module")
def pt():
    import ptamd
    ptamd.build()
    return ptamd


def _validate(pt, bvh):
    ref = pt._SceneRef(bvh)  # keeps the arrays alive during the call
    info = np.zeros(4, np.int32)
    rc = pt.lib().pt_scene_validate(C.byref(ref.s), info.ctypes.data)
    return rc, dict(zip(("nodes", "depth", "leaves", "stack"), info.tolist()))


@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("name", SCENES)
def test_transform_validates_and_packs_as_implied(pt, name, variant):
    c = TC.case(name, variant)
    nt = len(c.idx)
    bvh = TC.to_bvh(pt, c)
    rc, info = _validate(pt, bvh)
    assert rc == 0, pt.lib().pt_last_error()
    sizes = T.leaf_sizes(c.nodes)
    assert info["nodes"] == T.reachable(c.nodes) and info["depth"] == T.depth(c.nodes)
    contained = variant not in TC.TREE_ONLY
    assert info["leaves"] == (len(sizes) if contained else 0)
    si = pt.scene_info(bvh)
    if variant.startswith("merged"):
        k = int(variant[6:])
        assert info["nodes"] < len(c.nodes) and 1 < max(sizes) <= k and sum(sizes) == nt
        # multi-triangle leaves: never the 48-B single-triangle records
        assert si["wide_record_bytes"] == (64 if si["wide_nodes"] else 0)
        if k <= 31:
            assert si["wide_nodes"] > 0 and si["wide_tris"] == nt
    elif variant == "root_leaf":
        assert info["nodes"] == 1 and info["depth"] == 0 and sizes == [nt] and si["wide_nodes"] == 0
    elif variant.startswith("chain"):
        assert info["depth"] == nt - 1 and info["nodes"] == 2 * nt - 1 and sizes == [1] * nt
        assert info["stack"] == (nt if variant == "chain_right" else 2)
        assert not np.array_equal(c.idx, np.arange(nt)) and sorted(c.idx.tolist()) == list(range(nt))
        assert si["wide_nodes"] > 0
    elif variant == "empty":
        assert sizes.count(0) == -(-len(c.base_idx) // 4) and sum(sizes) == nt and si["wide_tris"] == nt
    elif variant == "duplicated":
        assert sum(sizes) == nt + 1 and info["nodes"] == len(c.base_nodes) + 2
    elif variant == "dropped":
        assert sum(sizes) == nt - 1 and sizes.count(0) == 1
    elif variant == "uncontained":
        assert sum(sizes) == nt and c.nodes.tobytes() != c.base_nodes.tobytes()
    if not contained:
        assert si["wide_nodes"] == 0 and si["flat_leaves"] == 0


def test_k_big_drops_the_wide_tree_for_its_leaf_run(pt, monkeypatch):
    """merged(K_BIG) on the sphere scene: an interior root whose leaves sum to more than 255
    triangles under one wide node, so no wide tree is built at either width (the leaf ends are
    bytes), while merged(31) (8 x 31 = 248) always builds one."""
    c = TC.case("sphere12", f"merged{TC.K_BIG}")
    assert not T.is_leaf(c.nodes, 0) and sum(sorted(T.leaf_sizes(c.nodes))[-8:]) > 255
    for w in ("4", "8"):
        monkeypatch.setenv("PT_WIDE_W", w)
        assert pt.scene_info(TC.to_bvh(pt, c))["wide_nodes"] == 0
        for name in SCENES:
            si = pt.scene_info(TC.to_bvh(pt, TC.case(name, "merged31")))
            assert si["wide_nodes"] > 0 and si["wide_width"] == int(w)


@pytest.mark.parametrize("variant", TC.CONTAINED)
@pytest.mark.parametrize("name", SCENES)
def test_wide_tree_of_caller_tree_verifies(pt, monkeypatch, name, variant):
    """pt_debug_wide_verify: the wide tree of every caller tree that has one is exact at both
    widths and in every plane format. A root leaf has none (pack_scene builds a wide tree only
    under an interior root): the hook says so instead of reading the root's children."""
    bvh = TC.to_bvh(pt, TC.case(name, variant))
    ref = pt._SceneRef(bvh)
    for w in (4, 8):
        rc = pt.lib().pt_debug_wide_verify(C.byref(ref.s), w)
        if variant == "root_leaf":
            assert rc == pt._lib.PT_E_ARG and b"no wide tree" in pt.lib().pt_last_error()
        else:
            assert rc == 0, (w, pt.lib().pt_last_error())


@pytest.mark.parametrize("name,variant", [(n, v) for n in SCENES for v in ALL] + [("onetri", "root_leaf")])
def test_host_walk_matches_oracle_walk(pt, name, variant):
    """pt_bvh_intersect on the caller's nodes against tests/_refwalk.py on the same nodes:
    t bits and triangle ids, 256 seeded rays and the 16 with inf / NaN components."""
    c = TC.case(name, variant)
    o, d, t_ref, tri_ref = TC.expected(name, variant)
    bvh = TC.to_bvh(pt, c)
    t, tri = bvh.intersect(o, d)
    assert np.array_equal(RW.bits(t), RW.bits(t_ref)) and np.array_equal(tri, tri_ref)
    assert (tri_ref >= 0).any()
    if variant in ("dropped", "duplicated"):
        # the camera's centre ray hits the triangle the transform acts on in BVH::build's tree
        cam = TC.scene(name).camera
        o1, d1 = np.array([cam.pos], np.float32), np.array([cam.forward], np.float32)
        _, hit = bvh.intersect(o1, d1)
        assert c.tri >= 0 and (hit[0] != c.tri if variant == "dropped" else hit[0] == c.tri)
        assert c.tri not in tri.tolist() or variant == "duplicated"


def _rtc_source(pt, bvh):
    from test_capi import _rtc_source as src
    return src(pt, bvh)


def test_rtc_source_of_multi_triangle_leaves_compiles(pt):
    """The scene-specialised flat kernel of a merged(2) Cornell reads the leaf table's ranges
    (kSingleTri = false) and compiles for gfx950 (hipRTC, no device needed), as do the one-leaf
    kernels of root_leaf and of a genuine one-triangle scene (a single-triangle leaf)."""
    for variant, single, boxes in (("merged2", False, None), ("root_leaf", False, 1)):
        src = _rtc_source(pt, TC.to_bvh(pt, TC.case("cornell", variant)))
        assert f"kSingleTri = {'true' if single else 'false'};" in src, variant
        if boxes is not None:
            plain = src.split("#elif PT_SHARED_CLAMP\n")[1].split("#endif\n")[0].split("#else\n")[1]
            assert plain.count("const bool b") == boxes
    src = _rtc_source(pt, TC.to_bvh(pt, TC.case("onetri", "root_leaf")))
    assert "kSingleTri = true;" in src and "kMask32 = true;" in src


# ---------------------------------------------------------------- the oracle's walk, pinned
with open(os.path.join(GOLDEN, "trees.json")) as _f:
    TREES = json.load(_f)


@pytest.mark.parametrize("name", sorted(TREES["images"]))
def test_oracle_walk_of_caller_tree_matches_reference(name):
    """`_oracle.render(nodes=, idx=)` against the compiled reference rendering the same tree
    file (tests/golden/gen_trees.py): same bits. The reference prints no ray count; the
    oracle's count at generation time is recorded with the image and must not move."""
    m = TREES["images"][name]
    sc = TC.scene(m["scene"], m["res"])
    assert scene_hash(sc) == m["scene_sha256"]
    c = TC.case(m["scene"], m["variant"])
    import hashlib
    assert hashlib.sha256(T.dump_bvh_bytes(c.nodes, c.idx)).hexdigest() == m["tree_sha256"]
    img, rays = TC.oracle_image(m["scene"], m["variant"], tuple(m["res"]), m["spp"], m["depth"])
    ref = load_golden(name)
    assert img.shape == ref.shape and np.array_equal(RW.bits(img), RW.bits(ref))
    assert rays == m["oracle_rays"]
    # the tree matters: BVH::build's own tree gives another image or ray count where leaves
    # were emptied or dropped
    if m["variant"] == "dropped":
        base, _ = O.render(sc, m["spp"], m["depth"])
        assert not np.array_equal(RW.bits(base), RW.bits(ref))
