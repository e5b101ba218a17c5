"""The light-sampling estimator without a device: the light table (pt_scene_lights), the host
form pt_bvh_trace_nee (bit-identical to the GPU's) through ptamd.BVH.trace_nee, its expected value
against trace()'s, and the argument handling. Expected values: tests/_refnee.py (the definition of
include/pt_hip.h restated over the oracle's primitives)."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import _oracle as O
import _refnee as RN
import _reftrace as RT
import _refwalk as RW
import _treecases as TC

F32 = np.float32
N = 256


@functools.lru_cache(maxsize=None)
def _bvh(name):
    import ptamd
    b = ptamd.BVH.from_scene(RT.make_scene(name))
    b.build()
    return b


def _same_table(got, want: RN.Lights):
    assert got["tri"].dtype == np.int32 and got["cdf"].dtype == np.float32
    assert np.array_equal(got["tri"], want.tri)
    assert np.array_equal(RW.bits(got["cdf"]), RW.bits(want.cdf))
    assert RW.bits(np.array([got["area"]]))[0] == RW.bits(np.array([want.area]))[0]


def test_scene_lights_matches_restatement():
    import ptamd
    for name, count in (("cornell", 2), ("random_7_300", None)):
        want = RN.lights(name)
        _same_table(ptamd.scene_lights(_bvh(name)), want)
        assert want.tri.size > 0 and (count is None or want.tri.size == count)
        assert (np.diff(want.cdf) > 0).all() and want.area == want.cdf[-1]
    # an EMIT triangle of zero emission and a degenerate one are no lights
    sc = RN.edge_lights_scene()
    verts, mtype, mvals = O.pack_scene(sc)
    want = RN.light_table(verts, mtype, mvals)
    got = ptamd.scene_lights(ptamd.BVH.from_scene(sc))
    _same_table(got, want)
    nt = verts.shape[0]
    assert (mtype[[nt - 2, nt - 1]] == RN.EMIT).all() and not np.isin([nt - 2, nt - 1], got["tri"]).any()
    _same_table(got, RN.lights("cornell"))  # Cornell's own two lights, and nothing else


@pytest.mark.parametrize("explicit", [False, True], ids=["seeded", "states"])
@pytest.mark.parametrize("name", RN.SCENES)
def test_pt_bvh_trace_nee_matches_restatement(name, explicit):
    o, d = RT.rays(name, N)
    P = RN.head(RN.paths(name, explicit=explicit), N)
    states = RT.explicit_states(512)[:N] if explicit else None
    shadows = changed = 0
    for depth in RN.DEPTHS:
        want, segs, sh, dr = RN.radiance(P, depth)
        got, st = _bvh(name).trace_nee(o, d, depth, states=states)
        assert got.dtype == np.float32 and got.shape == (N, 3)
        RT.assert_same(got, want, f"{name} depth {depth}")
        assert st["rays"] == int(segs.sum()) and st["shadow_rays"] == int(sh.sum()) and st["light_draws"] == int(dr.sum())
        assert st["paths"] == N and st["runaway"] == 0 and st["lights"] == P.lights.tri.size
        shadows += st["shadow_rays"]
        plain, _ = _bvh(name).trace(o, d, depth, states=states)
        changed += int((~RT.same_bits(got, plain).all(axis=1)).sum())
    assert shadows > 0 and changed > 0  # the comparison is not vacuous


@pytest.mark.parametrize("spp", [2, 7])
@pytest.mark.parametrize("name", ["random_7_300", "cornell+glow"])
def test_samples_sum_in_order(name, spp):
    o, d = RT.rays(name, 65)
    b = _bvh(name)
    want = RT.mean_of_samples(lambda st: b.trace_nee(o, d, 5, states=st)[0], 65, spp, 3)
    got, st = b.trace_nee(o, d, 5, samples=spp, seed=3)
    RT.assert_same(got, want, f"{name} spp {spp}")
    assert st["paths"] == 65 * spp
    got2, _ = b.trace_nee(o, d, 5, samples=spp, states=RT.sample_seeds(65, spp, 3))
    RT.assert_same(got2, want)


def test_nonfinite_rays():
    o, d, want, segs, sh = RN.nonfinite_expected()
    got, st = _bvh("random_7_300").trace_nee(o, d, 5)
    RT.assert_same(got, want, "non-finite rays")
    assert st["rays"] == segs > 16 and st["shadow_rays"] == sh
    assert RW.bits(want).any()  # assert_same accepts a NaN only where the restatement has one


def test_depth_zero():
    o, d = RT.rays("cornell+glow", N)
    got, st = _bvh("cornell+glow").trace_nee(o, d, 0)
    assert not RW.bits(got).any() and st["rays"] == 0 and st["shadow_rays"] == 0 and st["paths"] == N


@pytest.mark.parametrize("name,variant", RN.TREES)
def test_caller_built_trees(name, variant):
    """Multi-triangle leaves, a triangle in two leaves and one in none: the shadow test compares
    the caller's triangle indices, so a duplicated light is one light."""
    import ptamd
    o, d, want, segs, sh = RN.tree_expected(name, variant)
    got, st = TC.to_bvh(ptamd, TC.case(name, variant)).trace_nee(o, d, 5)
    RT.assert_same(got, want, f"{name} {variant}")
    assert st["rays"] == segs and st["shadow_rays"] == sh > 0


def test_scene_without_lights():
    """random_3_40 with its EMIT materials retyped DIFFUSE: no light draw is made, and the forward
    form agrees with trace()'s unwinding within 64 * 2^-24 relative per channel: at most 8 levels
    of 3 roundings plus 8 additions, every term non-negative (colours, emissions and cosines are
    >= 0), so there is no cancellation."""
    import ptamd
    sc = RT.make_scene("random_3_40")
    sc.mats = [dataclasses.replace(m, type=2) if m.type == RN.EMIT else m for m in sc.mats]
    b = ptamd.BVH.from_scene(sc)
    o, d = RT.rays("random_3_40", N)
    got, st = b.trace_nee(o, d, 8)
    ref, st0 = b.trace(o, d, 8)
    assert st["lights"] == 0 and st["shadow_rays"] == 0 and st["light_draws"] == 0 and st["rays"] == st0["rays"]
    assert np.isfinite(ref).all() and (ref > 0).any()
    assert (np.abs(got.astype(np.float64) - ref) <= 64 * 2.0 ** -24 * np.abs(ref.astype(np.float64))).all()


# ---------------------------------------------------------------- the expectation is trace()'s
SPP = 4096


@functools.lru_cache(maxsize=None)
def _camera_samples():
    """Cornell's own camera at 16 x 16: SPP host camera rays per pixel (sample s is
    `_reftrace.camera_rays` at seed s + 1, with the states after the camera's two draws)."""
    sc = RW.make_scene("cornell", (16, 16))
    o, d, st = zip(*(RT.camera_rays(sc, s + 1) for s in range(SPP)))
    return np.concatenate(o), np.concatenate(d), np.concatenate(st)


@functools.lru_cache(maxsize=None)
def _estimates(depth):
    """Per-sample values (SPP, 256, 3) float64 of both estimators on the same rays and states."""
    o, d, st = _camera_samples()
    b = _bvh("cornell")
    ref, _ = b.trace(o, d, depth, states=st)
    nee, _ = b.trace_nee(o, d, depth, states=st)
    return ref.reshape(SPP, 256, 3).astype(np.float64), nee.reshape(SPP, 256, 3).astype(np.float64)


def _pooled(x, pix):
    """Over the pixels `pix`: the mean, and the pooled (within-pixel) per-sample variance, per channel."""
    x = x[:, pix]
    return x.mean(axis=(0, 1)), x.var(axis=0, ddof=1).mean(axis=0), x.shape[0] * x.shape[1]


@pytest.mark.slow
@pytest.mark.parametrize("depth", [3, 5])
def test_same_expectation_and_lower_variance(depth):
    """1,048,576 paths per estimator. Image mean and the four 8 x 8 quadrant means agree within
    5 standard errors of the difference; that bound is at most 8 % of the reference's image mean
    (so the test cannot pass on noise alone); and light sampling lowers the per-sample variance."""
    ref, nee = _estimates(depth)
    px = np.arange(256).reshape(16, 16)
    regions = [px.ravel()] + [px[i:i + 8, j:j + 8].ravel() for i in (0, 8) for j in (0, 8)]
    for r, pix in enumerate(regions):
        m0, v0, n = _pooled(ref, pix)
        m1, v1, _ = _pooled(nee, pix)
        bound = 5 * np.sqrt(v0 / n + v1 / n)
        print(f"depth {depth} region {r}: ref {m0} nee {m1} z {(m1 - m0) / (bound / 5)} var ratio {v1 / v0}")
        assert (np.abs(m1 - m0) <= bound).all(), (depth, r, m0, m1, bound)
        if r == 0:
            assert (bound <= 0.08 * m0).all(), (depth, bound / m0)
            assert (v1 < v0).all(), (depth, v1 / v0)


def test_argument_handling():
    import ptamd
    from ptamd import _lib
    L = ptamd.lib()
    ref = ptamd._SceneRef(_bvh("cornell"))
    o, d = RT.rays("cornell", 4)
    rgb = np.zeros((4, 3), dtype=np.float32)
    st = _lib.pt_nee_stats()
    ok = _lib.pt_trace_params(5, 1, 1, None)

    def arg_error(rc):
        assert rc == _lib.PT_E_ARG
        assert L.pt_last_error()  # a message

    def host(scene=ref.s, org=o.ctypes.data, dirs=d.ctypes.data, n=4, prm=ok, out=rgb.ctypes.data):
        return L.pt_bvh_trace_nee(C.byref(scene) if scene is not None else None, org, dirs, n,
                                  C.byref(prm) if prm is not None else None, out, C.byref(st))

    assert host() == 0
    assert host(org=None, dirs=None, n=0, out=None) == 0  # n == 0
    arg_error(host(n=-1))
    arg_error(host(scene=None))
    arg_error(host(org=None))
    arg_error(host(dirs=None))
    arg_error(host(out=None))
    arg_error(host(prm=None))
    for depth, spp in ((-1, 1), (_lib.PT_MAX_DEPTH + 1, 1), (5, 0), (5, -3), (5, (1 << 20) + 1)):
        arg_error(host(prm=_lib.pt_trace_params(depth, spp, 1, None)))
    assert host(prm=_lib.pt_trace_params(_lib.PT_MAX_DEPTH, 1, 1, None)) == 0
    bad = _lib.pt_scene(ref.s.num_tris, ref.s.verts, ref.s.materials, ref.s.num_nodes, ref.s.nodes, None)
    arg_error(host(scene=bad))  # a scene pt_scene_validate refuses
    # the light table: a count without arrays, a negative cap, a refused scene
    count, area = C.c_int64(-1), C.c_float(-1)
    assert L.pt_scene_lights(C.byref(ref.s), None, None, 0, C.byref(count), C.byref(area)) == 0
    assert count.value == 2 and area.value > 0
    arg_error(L.pt_scene_lights(C.byref(ref.s), None, None, -1, C.byref(count), C.byref(area)))
    arg_error(L.pt_scene_lights(C.byref(bad), None, None, 0, C.byref(count), C.byref(area)))
    # a NULL context (no device needed for these returns)
    arg_error(L.pt_ctx_trace_nee(None, o.ctypes.data, d.ctypes.data, 4, C.byref(ok), rgb.ctypes.data, 0, C.byref(st)))
    arg_error(L.pt_ctx_trace_nee(None, None, None, 0, None, None, 0, None))
    arg_error(L.pt_ctx_render_nee(None, None, None, None, None, 0, None))
    with pytest.raises(ValueError):
        _bvh("cornell").trace_nee(o, d, 5, samples=2, states=np.zeros(4, dtype=np.uint32))
    for name in ("pt_scene_lights", "pt_bvh_trace_nee", "pt_ctx_trace_nee", "pt_ctx_render_nee"):
        assert hasattr(L, name) and name in _lib.EXPORTED
    assert C.sizeof(_lib.pt_nee_stats) == 88
