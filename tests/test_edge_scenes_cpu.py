"""Scenes at extreme coordinate scales and with exact ties (tests/_edgescenes.py) on the host: the
product builder against the oracle's, the configuration the GPU tests rely on, BVH.intersect and
BVH.trace against the restated walks, the oracle against the compiled reference, and floors that
keep every comparison from passing on an empty picture."""
import ctypes as C
import functools

import numpy as np
import pytest

import _edgescenes as E
import _oracle as O
import _reftrace as RT
import _refwalk as RW

RES = (16, 12)
F32 = np.float32


@pytest.fixture(scope="module")
def pt():
    import ptamd
    ptamd.lib()
    return ptamd


@functools.lru_cache(maxsize=None)
def _image(member, spp=8, res=RES):
    """The oracle's image and ray count (base scenes: member = the base's name)."""
    sc = E.make(member, res)
    img, rays = O.render(sc, spp, 5)
    img.setflags(write=False)
    return img, rays


def _differ(a, b):
    return (~RT.same_bits(a, b)).reshape(-1, 3).any(axis=1)


# ---------------------------------------------------------------- the inputs are not vacuous
@pytest.mark.parametrize("base", E.BASES)
def test_inputs_are_not_vacuous(base):
    """From the oracle alone: each family changes what it is meant to change, and what is compared
    later is a lit picture (or, for k >= 51, provably one primary ray per sample)."""
    W, H = RES
    base_img, _ = _image(base)
    lit0 = E.lit_share(base_img)
    shares = {"base": round(lit0, 3)}
    hit0 = E.first_hit_rate(base)
    assert lit0 > 0 and hit0 >= 0.9, (base, lit0, hit0)
    a, b = _image(f"{base}/doubled/base")[0], _image(f"{base}/doubled/alt")[0]
    assert _differ(a, b).mean() >= 0.5, (base, _differ(a, b).mean())
    assert E.lit_share(a) >= 0.5 * lit0 and E.lit_share(b) >= 0.5 * lit0
    assert _differ(_image(f"{base}/scaled/20")[0], base_img).any()
    shares["k20"] = round(E.lit_share(_image(f"{base}/scaled/20")[0]), 3)
    shares["k33"] = round(E.lit_share(_image(f"{base}/scaled/33")[0]), 3)
    assert shares["k20"] > 0
    r33, r34 = E.first_hit_rate(f"{base}/scaled/33"), E.first_hit_rate(f"{base}/scaled/34")
    assert 0 < r34 < r33, (base, r33, r34)
    assert E.first_hit_rate(f"{base}/scaled/-12") > 0.5 and E.lit_share(_image(f"{base}/scaled/-12")[0]) >= 0.5 * lit0
    for k in E.FAR_CAMERAS:  # rays from past 2^60 and 2^64 that still hit
        assert E.first_hit_rate(f"{base}/far_camera/{k}") >= 0.5
    for k in (51, 100):
        img, rays = _image(f"{base}/scaled/{k}")
        assert rays == W * H * 8 and not img.view(np.uint32).any()
    for kind in E.OUTLIER_KINDS:
        for m in "ds":
            img, _ = _image(f"{base}/outlier/{kind}/{m}")
            assert np.isfinite(img).all(), (base, kind, m)
            shares[f"{kind}/{m}"] = round(E.lit_share(img), 3)
            assert E.lit_share(img) >= 0.5 * lit0, (base, kind, m, E.lit_share(img), lit0)
    print(base, "lit shares", shares, "first-hit k33/k34", r33, r34)


@pytest.mark.parametrize("base", E.BASES)
def test_degenerate_triangles_are_never_hit(base):
    """The point and the segment (NaN normals) are hit on no segment of any camera path, and the
    image equals the base's except in pixels whose path meets the sliver."""
    member = f"{base}/degenerate"
    sc, verts, mtype, mvals, nodes, idx = E.arrays(member, RES)
    n = len(sc.tris)
    o, d, st = RT.camera_rays(sc, 1)
    P = RT.walk_paths(nodes, idx, verts, mtype, mvals, o, d, st, 5)
    assert not np.isin(P.tri, (n - 3, n - 2)).any()
    sliver = (P.tri == n - 1).any(axis=0)
    img, _ = O.render(sc, 1, 5)
    base_img, _ = O.render(E.base_scene(base, RES), 1, 5)
    assert not _differ(img, base_img)[~sliver].any()
    # the sliver can be hit: a ray straight at it is
    so = np.array([[275.0, 250.0 + 2.0 ** -15, 100.0]], dtype=F32)
    t, tri = RW.ref_walk(nodes, idx, verts, so, np.array([[0.0, 0.0, 1.0]], dtype=F32))
    if base == "cornell":  # nothing of Cornell stands between z = 100 and the sliver on this line
        assert tri[0] == n - 1 and t[0] == F32(150.0)


# ---------------------------------------------------------------- builder and configuration
def _rtc_source(pt, ref):
    buf = C.create_string_buffer(1 << 21)
    assert pt.lib().pt_rtc_check(C.byref(ref.s), buf, len(buf)) > 1000, pt.lib().pt_last_error()
    return buf.value.decode()


@pytest.mark.parametrize("member", E.MEMBERS)
def test_builder_and_configuration(pt, member):
    sc, verts, _, _, nodes, idx = E.arrays(member, RES)
    bvh = pt.BVH.from_scene(sc)
    bvh.build()
    assert np.array_equal(bvh.verts().view(np.uint32), verts.view(np.uint32))
    assert bvh.nodes.tobytes() == nodes.tobytes() and bvh.tri_idx.tobytes() == idx.tobytes()
    assert E.coords_big(member) == bool((np.abs(verts) >= F32(2.0 ** 60)).any())
    info = pt.scene_info(bvh)
    ref = pt._SceneRef(bvh)
    if E.one_leaf(member):
        assert nodes.shape[0] == 1 and info["flat_leaves"] == 1 and info["wide_nodes"] == 0, info
    else:
        assert nodes.shape[0] > 1 and info["flat_leaves"] != 1, info
    base = E.parse(member)[0]
    flat = 0 < info["flat_leaves"] <= 64
    assert flat == (base in E.FLAT_BASES or E.one_leaf(member)), info
    if flat:
        src = _rtc_source(pt, ref)
        want = "false" if E.coords_big(member) else "true"
        assert f"kTriFast = {want};" in src, member
    if info["wide_nodes"] > 0:
        for w in (4, 8):
            assert pt.lib().pt_debug_wide_verify(C.byref(ref.s), w) == 0, (member, w)
    elif not E.one_leaf(member):
        pytest.fail(f"{member}: a scene with a tree but no wide tree: {info}")


# ---------------------------------------------------------------- host walks against the restatements
@pytest.mark.parametrize("member", E.MEMBERS)
def test_host_intersect_and_trace(pt, member):
    sc, verts, mtype, mvals, nodes, idx = E.arrays(member, RES)
    bvh = pt.BVH.from_scene(sc)
    co, cd, states = RT.camera_rays(sc, 1)
    qo, qd = E.query_rays(member)
    o, d = np.concatenate([co, qo]), np.concatenate([cd, qd])
    t_ref, tri_ref = RW.ref_walk(nodes, idx, verts, o, d)
    t, tri = bvh.intersect(o, d)
    bad = np.flatnonzero((RW.bits(t) != RW.bits(t_ref)) | (tri != tri_ref))
    assert bad.size == 0, (member, bad[:5], t[bad[:5]], t_ref[bad[:5]], tri[bad[:5]], tri_ref[bad[:5]])
    want, _, segs = RT.trace(nodes, idx, verts, mtype, mvals, co, cd, states, 5)
    got, st = bvh.trace(co, cd, 5, states=states)
    RT.assert_same(got, want, member)
    assert st["rays"] == int(segs.sum())
    img, rays = O.render(sc, 1, 5)
    RT.assert_same(got, img.reshape(-1, 3), f"{member}: BVH.trace vs the oracle's render")
    assert rays == st["rays"]
    # the far rays are not all misses where the scene can be hit at all
    n0 = co.shape[0] + E.N_NEAR
    far = tri_ref[n0:n0 + E.N_FAR]
    family = E.parse(member)[1]
    if family != "scaled" or int(E.parse(member)[2][0]) < 33:
        assert (far >= 0).mean() > 0.25, (member, (far >= 0).mean())
    # the threshold rays: |a| one or two floats below EPS never hits its triangle; |a| the next
    # float does, unless something else comes first (at the base's own scale; at 2^20 and above
    # most such hits lie past t = 1e30)
    ec, et = E.eps_classes(member)
    own = tri_ref[n0 + E.N_FAR:] == et
    assert ec.size or (family == "scaled" and int(E.parse(member)[2][0]) >= 51)
    assert not own[ec < 2].any(), member
    if family != "scaled":
        assert own[ec == 2].mean() >= 0.75, member


@pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref/pt_ref not built")
@pytest.mark.parametrize("member", E.MEMBERS)
def test_oracle_matches_reference(member):
    """What pins the oracle itself outside ordinary scale."""
    sc = E.make(member, (24, 20))
    img, rays = O.render(sc, 4, 5)
    ref, meta = O.ref_run(sc, 4, 5)
    RT.assert_same(img.reshape(-1, 3), ref.reshape(-1, 3), member)
    assert meta["tris"] == len(sc.tris) and meta["nodes"] == E.arrays(member, (24, 20))[4].shape[0]
