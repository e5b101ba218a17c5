"""The weighted light-sampling estimator (PT_NEE_MIS_BALANCE) without a device: the host form
pt_bvh_trace_nee_opt (bit-identical to the GPU's) through ptamd.BVH.trace_nee(mis=True) against
tests/_refmis.py (the definition of include/pt_hip.h restated over the oracle's primitives), the
unweighted mode of the new entry point, the options' checks, the bound on a sample and the
expectation where an emitter touches a diffuse surface."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import _refmis as RM
import _refnee as RN
import _reftrace as RT
import _refwalk as RW
import _treecases as TC

F32 = np.float32
N = 256
NEE_KEYS = ("rays", "paths", "runaway", "shadow_rays", "light_draws", "lights", "light_area")


@functools.lru_cache(maxsize=None)
def _bvh(name):
    import ptamd
    b = ptamd.BVH.from_scene(RM.tri3_scene() if name == "tri3" else RT.make_scene(name))
    b.build()
    return b


def _same_stats(a, b):
    assert {k: a[k] for k in NEE_KEYS} == {k: b[k] for k in NEE_KEYS}, (a, b)


@pytest.mark.parametrize("explicit", [False, True], ids=["seeded", "states"])
@pytest.mark.parametrize("name", RN.SCENES)
def test_pt_bvh_trace_nee_opt_matches_restatement(name, explicit):
    o, d = RT.rays(name, N)
    P = RM.head(RM.paths(name, explicit=explicit), N)
    states = RT.explicit_states(512)[:N] if explicit else None
    b = _bvh(name)
    hits = vis = changed = 0
    for depth in RN.DEPTHS:
        want, segs, sh, dr = RM.radiance(P, depth)
        got, st = b.trace_nee(o, d, depth, states=states, mis=True)
        assert got.dtype == np.float32 and got.shape == (N, 3)
        RT.assert_same(got, want, f"{name} depth {depth}")
        assert st["rays"] == int(segs.sum()) and st["shadow_rays"] == int(sh.sum()) and st["light_draws"] == int(dr.sum())
        assert st["paths"] == N and st["runaway"] == 0 and st["lights"] == P.lights.tri.size
        plain, st0 = b.trace_nee(o, d, depth, states=states)
        _same_stats(st, st0)  # the same draws and segments as the unweighted estimator
        changed += int((~RT.same_bits(got, plain).all(axis=1)).sum())
        h, v = RM.weighted_counts(P, depth)
        hits += h
        vis += v
    assert hits > 0 and vis > 0 and changed > 0, (hits, vis, changed)  # both weighted cases were taken


def test_edge_rays_match_restatement():
    """tri3's edge rays (the emitter touches the diffuse triangle): weights far from 0 and 1."""
    P = RM.edge_paths(N, 5)
    o, d = RM.edge_rays(N)
    for depth in (2, 5):
        want, segs, sh, dr = RM.radiance(P, depth)
        got, st = _bvh("tri3").trace_nee(o, d, depth, mis=True)
        RT.assert_same(got, want, f"tri3 edge rays depth {depth}")
        assert st["rays"] == int(segs.sum()) and st["shadow_rays"] == int(sh.sum()) and st["light_draws"] == int(dr.sum())
        h, v = RM.weighted_counts(P, depth)
        assert h > 0 and v > 0, (depth, h, v)


def _opt_call(L, name, mis, *args, reserved=(0, 0, 0), null=False):
    from ptamd import _lib
    opt = _lib.pt_nee_options(mis, reserved)
    return getattr(L, name)(*args, None if null else C.byref(opt))


def test_unweighted_mode_is_pt_bvh_trace_nee():
    """NULL options and PT_NEE_MIS_NONE: the existing function's bits and stats."""
    import ptamd
    from ptamd import _lib
    L = ptamd.lib()
    name = "random_7_300"
    ref = ptamd._SceneRef(_bvh(name))
    o, d = RT.rays(name, N)
    prm = _lib.pt_trace_params(5, 3, 7, None)
    want, st_w = _bvh(name).trace_nee(o, d, 5, samples=3, seed=7)
    assert st_w["shadow_rays"] > 0
    for null in (True, False):
        rgb = np.full((N, 3), -1.0, dtype=F32)
        st = _lib.pt_nee_stats()
        rc = _opt_call(L, "pt_bvh_trace_nee_opt", _lib.PT_NEE_MIS_NONE, C.byref(ref.s), o.ctypes.data, d.ctypes.data, N,
                       C.byref(prm), rgb.ctypes.data, C.byref(st), null=null)
        assert rc == 0
        RT.assert_same(rgb, want, f"null {null}")
        _same_stats(st.as_dict(), st_w)
    weighted, _ = _bvh(name).trace_nee(o, d, 5, samples=3, seed=7, mis=True)
    assert not RT.same_bits(weighted, want).all()


@pytest.mark.parametrize("spp", [2, 7])
@pytest.mark.parametrize("name", ["random_7_300", "cornell+glow"])
def test_samples_sum_in_order(name, spp):
    o, d = RT.rays(name, 65)
    b = _bvh(name)
    want = RT.mean_of_samples(lambda st: b.trace_nee(o, d, 5, states=st, mis=True)[0], 65, spp, 3)
    got, st = b.trace_nee(o, d, 5, samples=spp, seed=3, mis=True)
    RT.assert_same(got, want, f"{name} spp {spp}")
    assert st["paths"] == 65 * spp
    got2, _ = b.trace_nee(o, d, 5, samples=spp, states=RT.sample_seeds(65, spp, 3), mis=True)
    RT.assert_same(got2, want)


def test_nonfinite_rays():
    o, d, want, segs, sh = RM.nonfinite_expected()
    got, st = _bvh("random_7_300").trace_nee(o, d, 5, mis=True)
    RT.assert_same(got, want, "non-finite rays")
    assert st["rays"] == segs > 16 and st["shadow_rays"] == sh
    assert RW.bits(want).any()  # assert_same accepts a NaN only where the restatement has one
    assert (segs, sh) == RN.nonfinite_expected()[3:5]


def test_depth_zero():
    o, d = RT.rays("cornell+glow", N)
    got, st = _bvh("cornell+glow").trace_nee(o, d, 0, mis=True)
    assert not RW.bits(got).any() and st["rays"] == 0 and st["shadow_rays"] == 0 and st["paths"] == N


@pytest.mark.parametrize("name,variant", RN.TREES)
def test_caller_built_trees(name, variant):
    """Multi-triangle leaves, a triangle in two leaves and one in none: the weights use the table's
    A and the caller's triangle indices, so a duplicated light is weighted once."""
    import ptamd
    o, d, want, segs, sh, (hits, vis) = RM.tree_expected(name, variant)
    got, st = TC.to_bvh(ptamd, TC.case(name, variant)).trace_nee(o, d, 5, mis=True)
    RT.assert_same(got, want, f"{name} {variant}")
    assert st["rays"] == segs and st["shadow_rays"] == sh > 0
    assert (segs, sh) == RN.tree_expected(name, variant)[3:5]
    assert vis > 0 and hits >= 0, (hits, vis)  # 272 rays: few paths end on Cornell's small light


def test_scene_without_lights():
    """random_3_40 with its EMIT materials retyped DIFFUSE: no light draw is made and no weight is
    formed, so the result is trace_nee's bit for bit (and that is trace()'s within the forward
    form's rounding, tests/test_nee_cpu.py)."""
    import ptamd
    sc = RT.make_scene("random_3_40")
    sc.mats = [dataclasses.replace(m, type=2) if m.type == RN.EMIT else m for m in sc.mats]
    b = ptamd.BVH.from_scene(sc)
    o, d = RT.rays("random_3_40", N)
    got, st = b.trace_nee(o, d, 8, mis=True)
    plain, st0 = b.trace_nee(o, d, 8)
    ref, st1 = b.trace(o, d, 8)
    assert st["lights"] == 0 and st["shadow_rays"] == 0 and st["light_draws"] == 0 and st["rays"] == st1["rays"]
    _same_stats(st, st0)
    assert np.array_equal(RW.bits(got), RW.bits(plain)) and RW.bits(got).any()
    assert np.isfinite(ref).all() and (ref > 0).any()
    assert (np.abs(got.astype(np.float64) - ref) <= 64 * 2.0 ** -24 * np.abs(ref.astype(np.float64))).all()


def test_bad_options():
    import ptamd
    from ptamd import _lib
    L = ptamd.lib()
    ref = ptamd._SceneRef(_bvh("cornell"))
    o, d = RT.rays("cornell", 4)
    rgb = np.zeros((4, 3), dtype=F32)
    st = _lib.pt_nee_stats()
    prm = _lib.pt_trace_params(5, 1, 1, None)
    host = (C.byref(ref.s), o.ctypes.data, d.ctypes.data, 4, C.byref(prm), rgb.ctypes.data, C.byref(st))

    def arg_error(rc):
        assert rc == _lib.PT_E_ARG
        assert L.pt_last_error()  # a message

    assert _opt_call(L, "pt_bvh_trace_nee_opt", _lib.PT_NEE_MIS_BALANCE, *host) == 0
    for mis in (-1, 2, 7, 1 << 30):
        arg_error(_opt_call(L, "pt_bvh_trace_nee_opt", mis, *host))
    for mis in (_lib.PT_NEE_MIS_NONE, _lib.PT_NEE_MIS_BALANCE):
        for reserved in ((1, 0, 0), (0, -1, 0), (0, 0, 5)):
            arg_error(_opt_call(L, "pt_bvh_trace_nee_opt", mis, *host, reserved=reserved))
    # the existing checks still answer: n < 0, NULL arrays, a NULL context (no device needed for these returns)
    arg_error(_opt_call(L, "pt_bvh_trace_nee_opt", 1, C.byref(ref.s), o.ctypes.data, d.ctypes.data, -1, C.byref(prm),
                        rgb.ctypes.data, C.byref(st)))
    arg_error(_opt_call(L, "pt_bvh_trace_nee_opt", 1, C.byref(ref.s), None, d.ctypes.data, 4, C.byref(prm), rgb.ctypes.data,
                        C.byref(st)))
    arg_error(_opt_call(L, "pt_ctx_trace_nee_opt", 1, None, o.ctypes.data, d.ctypes.data, 4, C.byref(prm), rgb.ctypes.data, 0,
                        C.byref(st)))
    arg_error(_opt_call(L, "pt_ctx_trace_nee_opt", 9, None, o.ctypes.data, d.ctypes.data, 4, C.byref(prm), rgb.ctypes.data, 0,
                        C.byref(st)))
    arg_error(_opt_call(L, "pt_ctx_render_nee_opt", 1, None, None, None, None, None, 0, None))
    for name in ("pt_bvh_trace_nee_opt", "pt_ctx_trace_nee_opt", "pt_ctx_render_nee_opt"):
        assert hasattr(L, name) and name in _lib.EXPORTED
    assert C.sizeof(_lib.pt_nee_options) == 16 and (_lib.PT_NEE_MIS_NONE, _lib.PT_NEE_MIS_BALANCE) == (0, 1)


# ---------------------------------------------------------------- where the emitter touches a diffuse surface
@functools.lru_cache(maxsize=None)
def _edge_samples():
    """Blue channel (float64) of the 65,536 edge rays on tri3 at depth 2, states
    pt_sample_seed(i, 0, 1): trace(), the unweighted and the weighted estimator."""
    o, d = RM.edge_rays()
    b = _bvh("tri3")
    ref, _ = b.trace(o, d, 2)
    nee, _ = b.trace_nee(o, d, 2)
    mis, _ = b.trace_nee(o, d, 2, mis=True)
    return tuple(x[:, 2].astype(np.float64) for x in (ref, nee, mis))


def test_sample_bound_on_the_edge_rays():
    """At depth 2 on tri3 a blue sample is one direct term, at most 2 (T o color o emit = 1), plus
    one weighted EMIT hit, 2 c wb <= 2: at most 4, with 2^-20 relative for the roundings. The
    unweighted estimator's largest sample on the same rays and states is in the hundreds."""
    _, nee, mis = _edge_samples()
    print(f"largest sample: unweighted {nee.max()}, weighted {mis.max()}")
    assert nee.max() > 100
    assert np.isfinite(mis).all() and mis.min() >= 0
    assert mis.max() <= 4 * (1 + 2.0 ** -20)


def test_expectation_on_the_edge_rays():
    """The weighted mean and trace()'s differ by at most 5 standard errors of the difference, a
    bound that is at most 8 % of trace()'s mean; the weighted variance is below the unweighted."""
    ref, nee, mis = _edge_samples()
    n = ref.size
    m0, m1 = ref.mean(), mis.mean()
    v0, v1, vn = ref.var(ddof=1), mis.var(ddof=1), nee.var(ddof=1)
    bound = 5 * np.sqrt(v0 / n + v1 / n)
    print(f"trace {m0} +- {np.sqrt(v0 / n)}, unweighted {nee.mean()} +- {np.sqrt(vn / n)} (variance {vn}), "
          f"weighted {m1} +- {np.sqrt(v1 / n)} (variance {v1}), bound {bound / m0} of the mean")
    assert bound <= 0.08 * m0
    assert abs(m1 - m0) <= bound, (m0, m1, bound)
    assert v1 < vn, (v1, vn)


SPP = 4096


@functools.lru_cache(maxsize=None)
def _camera_samples():
    """Cornell's own camera at 16 x 16: SPP host camera rays per pixel (sample s is
    `_reftrace.camera_rays` at seed s + 1, with the states after the camera's two draws)."""
    sc = RW.make_scene("cornell", (16, 16))
    o, d, st = zip(*(RT.camera_rays(sc, s + 1) for s in range(SPP)))
    return np.concatenate(o), np.concatenate(d), np.concatenate(st)


def _pooled(x, pix):
    """Over the pixels `pix`: the mean, and the pooled (within-pixel) per-sample variance, per channel."""
    x = x[:, pix]
    return x.mean(axis=(0, 1)), x.var(axis=0, ddof=1).mean(axis=0), x.shape[0] * x.shape[1]


@pytest.mark.slow
@pytest.mark.parametrize("depth", [3, 5])
def test_same_expectation_and_lower_variance(depth):
    """1,048,576 paths per estimator on Cornell's camera rays. Image mean and the four 8 x 8
    quadrant means agree with trace()'s within 5 standard errors of the difference, a bound that is
    at most 8 % of the reference's image mean; the pooled variance is below trace()'s. The ratio
    to the unweighted estimator's variance is printed, not asserted."""
    o, d, st = _camera_samples()
    b = _bvh("cornell")
    ref, nee, mis = (x.reshape(SPP, 256, 3).astype(np.float64) for x in
                     (b.trace(o, d, depth, states=st)[0], b.trace_nee(o, d, depth, states=st)[0],
                      b.trace_nee(o, d, depth, states=st, mis=True)[0]))
    px = np.arange(256).reshape(16, 16)
    regions = [px.ravel()] + [px[i:i + 8, j:j + 8].ravel() for i in (0, 8) for j in (0, 8)]
    for r, pix in enumerate(regions):
        m0, v0, n = _pooled(ref, pix)
        m1, v1, _ = _pooled(mis, pix)
        _, vn, _ = _pooled(nee, pix)
        bound = 5 * np.sqrt(v0 / n + v1 / n)
        print(f"depth {depth} region {r}: ref {m0} mis {m1} z {(m1 - m0) / (bound / 5)} var / trace {v1 / v0} "
              f"var / unweighted {v1 / vn}")
        assert (np.abs(m1 - m0) <= bound).all(), (depth, r, m0, m1, bound)
        if r == 0:
            assert (bound <= 0.08 * m0).all(), (depth, bound / m0)
            assert (v1 < v0).all(), (depth, v1 / v0)
