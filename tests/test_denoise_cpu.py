"""The a-trous denoiser on the host (pt_image_denoise, pt_moments_variance; ptamd.denoise,
ptamd.moments_variance, ptamd.denoise_guides). No device is needed.

The yardstick is tests/_refdenoise.py: a float32 numpy restatement of the contract in
include/pt_hip.h, which shares no code with the library. The results are defined bit for bit, so
every comparison is of bits (NaN equals NaN)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as O
import _refdenoise as RD
import _reftrace as RT

F32, F64 = np.float32, np.float64

SIZES = [(1, 1), (1, 7), (5, 1), (37, 23), (64, 64)]  # (W, H)


def test_symbols_and_structs():
    import ptamd
    from ptamd import _lib
    L = ptamd.lib()
    for name in ("pt_moments_variance", "pt_ctx_moments_variance", "pt_image_denoise", "pt_ctx_denoise",
                 "pt_ctx_render_denoised"):
        assert hasattr(L, name) and name in _lib.EXPORTED
    assert L.pt_abi_version() == 3
    assert C.sizeof(_lib.pt_denoise_params) == 20
    assert C.sizeof(_lib.pt_denoise_guides) == 5 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.pt_denoise_stats) == 96
    assert C.sizeof(_lib.pt_denoised_stats) == 24 + 96
    for f in ("denoise", "moments_variance", "denoise_guides"):
        assert callable(getattr(ptamd, f))
    for f in ("denoise", "moments_variance", "render_denoised"):
        assert callable(getattr(ptamd.Renderer, f))


@functools.lru_cache(maxsize=None)
def reference(W, H, passes, with_var):
    color, var, g = RD.synthetic(W, H, seed=W * 100 + H)
    return RD.denoise(color, g, var if with_var else None, passes=passes)


@pytest.mark.parametrize("with_var", [True, False])
@pytest.mark.parametrize("W,H", SIZES)
def test_matches_the_restatement(W, H, with_var):
    import ptamd
    color, var, g = RD.synthetic(W, H, seed=W * 100 + H)
    for passes in [1, 2, 3, 4, 5] + ([8] if (W, H) == (37, 23) else []):
        want, want_v = reference(W, H, passes, with_var)
        got, got_v = ptamd.denoise(color, g, var if with_var else None, passes=passes)
        RD.assert_same(got, want, f"{W}x{H} passes {passes} var {with_var}")
        if with_var:
            RD.assert_same(got_v, want_v, f"{W}x{H} passes {passes} variance")
        else:
            assert got_v is None
    if W * H >= 20:  # the filter did something, and the seeded NaN stayed where it was
        want, _ = reference(W, H, 5, with_var)
        assert (RD.bits(want) != RD.bits(color)).mean() > 0.5
        assert np.isnan(want).sum() >= 1 and np.isnan(want[np.isnan(color).any(axis=-1)]).any()


def test_defaults_are_the_documented_ones():
    import ptamd
    color, var, g = RD.synthetic(37, 23, seed=5)
    want, want_v = RD.denoise(color, g, var, passes=5, sigma_l=1.0, sigma_z=0.01, npow=7, eps=1e-6)
    got, got_v = ptamd.denoise(color, g, var)
    RD.assert_same(got, want, "defaults")
    RD.assert_same(got_v, want_v, "defaults, variance")
    # and explicit parameters are honoured
    want, want_v = RD.denoise(color, g, var, passes=3, sigma_l=2.5, sigma_z=0.05, npow=2, eps=1e-3)
    got, got_v = ptamd.denoise(color, g, var, passes=3, sigma_l=2.5, sigma_z=0.05, normal_pow_log2=2, eps=1e-3)
    RD.assert_same(got, want, "explicit parameters")
    RD.assert_same(got_v, want_v, "explicit parameters, variance")
    assert not RD.same_bits(got, ptamd.denoise(color, g, var, passes=3)[0]).all()


def _call(W, H, color, var, g, prm, out, var_out):
    import ptamd
    from ptamd import _lib
    gs = _lib.pt_denoise_guides()
    for k, a in g.items():
        setattr(gs, k, a.ctypes.data if a is not None else None)
    p = _lib.pt_denoise_params(*prm) if prm is not None else None
    return ptamd.lib().pt_image_denoise(W, H, color.ctypes.data if color is not None else None,
                                        var.ctypes.data if var is not None else None, C.byref(gs),
                                        C.byref(p) if p is not None else None,
                                        out.ctypes.data if out is not None else None,
                                        var_out.ctypes.data if var_out is not None else None)


def test_out_may_alias_the_input():
    color, var, g = RD.synthetic(37, 23, seed=9)
    want, want_v = RD.denoise(color, g, var)
    c, v = color.copy(), var.copy()
    assert _call(37, 23, c, v, g, None, c, v) == 0  # NULL params: every default
    RD.assert_same(c, want, "in place")
    RD.assert_same(v, want_v, "in place, variance")


def test_argument_errors():
    from ptamd import _lib
    W, H = 6, 4
    color, var, g = RD.synthetic(W, H, nasty=False)
    out, vout = np.empty_like(color), np.empty_like(color)
    ok = (0, 0.0, 0.0, 0, 0.0)
    assert _call(W, H, color, var, g, ok, out, vout) == 0
    bad = [
        dict(W=0), dict(H=-1), dict(color=None), dict(out=None), dict(var=None),  # var_out without var
        dict(prm=(9, 0, 0, 0, 0)), dict(prm=(-1, 0, 0, 0, 0)), dict(prm=(0, 0, 0, 11, 0)), dict(prm=(0, 0, 0, -1, 0)),
        dict(prm=(0, -1.0, 0, 0, 0)), dict(prm=(0, 0, -0.5, 0, 0)), dict(prm=(0, 0, 0, 0, -1e-6)),
        dict(prm=(0, float("nan"), 0, 0, 0)), dict(prm=(0, 0, float("nan"), 0, 0)), dict(prm=(0, 0, 0, 0, float("nan"))),
    ] + [dict(g=dict(g, **{k: None})) for k in _lib.pt_denoise_guides.NAMES]
    for b in bad:
        a = dict(W=W, H=H, color=color, var=var, g=g, prm=ok, out=out, var_out=vout)
        a.update(b)
        assert _call(**a) == _lib.PT_E_ARG, b
    import ptamd
    assert b"position" in ptamd.lib().pt_last_error()
    assert _call(W, H, color, None, g, ok, out, None) == 0


def test_moments_variance():
    import ptamd
    rng = np.random.default_rng(4)
    x = rng.uniform(0, 3, (40, 9, 7, 3)).astype(F32).astype(F64)  # 40 samples of 9 x 7 pixels
    x[:, 0, 0] = 0.25      # no variance: d = 0
    x[:, 0, 1, 0] = 1e20   # large values
    x[:, 0, 2, 1] = 1e-30  # tiny values: Q - m cancels
    for n in (1, 2, 3, 16, 40):
        S, Q = x[:n].sum(axis=0), (x[:n] * x[:n]).sum(axis=0)
        got = ptamd.moments_variance(S, Q, n)
        assert got.dtype == F32 and got.shape == S.shape
        RD.assert_same(got, RD.variance(S, Q, n), f"n = {n}")
        if n < 2:
            assert np.isposinf(got).all()
    # per-pixel counts, some below 2; a NaN sum gives 0 (d > 0 is false), a negative d is clamped
    spp = rng.integers(0, 41, (9, 7)).astype(np.int32)
    spp[0, 0], spp[0, 1], spp[1, 0] = 0, 1, 2
    S, Q = np.zeros((9, 7, 3)), np.zeros((9, 7, 3))
    for (i, j), n in np.ndenumerate(spp):
        S[i, j], Q[i, j] = x[:n, i, j].sum(axis=0), (x[:n, i, j] ** 2).sum(axis=0)
    S[2, 2, 0], Q[3, 3, 1] = np.nan, -5.0
    got = ptamd.moments_variance(S, Q, spp=spp)
    RD.assert_same(got, RD.variance(S, Q, spp), "per-pixel n")
    assert np.isposinf(got[spp < 2]).all() and np.isfinite(got[spp >= 2]).all()
    assert got[2, 2, 0] == 0 or spp[2, 2] < 2
    # not sem * sem
    sem = np.sqrt(np.maximum(0, (Q - S * S / 16) / 15) / 16).astype(F32)
    assert (RD.bits(ptamd.moments_variance(S, Q, 16)) != RD.bits(sem * sem)).any()
    with pytest.raises(ValueError):
        ptamd.moments_variance(S, Q[:2], 4)
    with pytest.raises(ptamd.PTError):
        ptamd._lib.check(ptamd.lib().pt_moments_variance(None, None, 3, 4, None, None))


def test_denoise_guides_forms_the_hit_point():
    import ptamd
    rng = np.random.default_rng(8)
    ray = rng.standard_normal((5, 4, 6)).astype(F32) * F32(100)
    t = rng.uniform(0, 1e3, (5, 4)).astype(F32)
    aov = {"ray": ray, "t": t, "normal": ray[..., :3], "tri": np.zeros((5, 4), np.int32), "emission": ray[..., 3:]}
    g = ptamd.denoise_guides(aov)
    want = np.empty((5, 4, 3), dtype=F32)
    for k in range(3):
        m = (ray[..., 3 + k] * t).astype(F32)  # rounded before the addition
        want[..., k] = ray[..., k] + m
    assert g["position"].dtype == F32 and np.array_equal(RD.bits(g["position"]), RD.bits(want))
    fused = (ray[..., :3].astype(F64) + ray[..., 3:].astype(F64) * t[..., None].astype(F64)).astype(F32)
    assert (RD.bits(want) != RD.bits(fused)).any()  # the inputs tell the two apart
    assert all(g[k] is aov[k] for k in ("normal", "t", "tri", "emission"))


@pytest.mark.parametrize("name", ["cornell", "modified_cornell_r0.3"])
def test_quality(name):
    """16 independent oracle samples per pixel at 32 x 32, depth 5, guides from sample 0's camera
    rays, truth the oracle at 2048 spp: the filter at its defaults lowers the RMSE. Measured
    (bit-defined, so these are the values): cornell 0.0338 -> 0.0136 (ratio 0.404),
    modified_cornell_r0.3 0.0853 -> 0.0443 (ratio 0.519)."""
    import ptamd
    from ptamd import scenes
    sc = scenes.cornell((32, 32)) if name == "cornell" else scenes.modified_cornell(0.3, (32, 32))
    n = 16
    x = np.stack([O.render(sc, 1, 5, seed=100 + s)[0] for s in range(n)]).astype(F64)
    S, Q = x.sum(axis=0), (x * x).sum(axis=0)
    noisy = (S / n).astype(F32)
    var = ptamd.moments_variance(S, Q, n)
    o, d, _ = RT.camera_rays(sc, 100)
    t, tri = ptamd.BVH.from_scene(sc).intersect(o, d)
    verts, _, mvals = O.pack_scene(sc)
    hit = tri >= 0
    normal = np.zeros((32 * 32, 3), dtype=F32)
    normal[hit] = RD.tri_normal(verts, tri[hit], d[hit])
    emission = np.zeros((32 * 32, 3), dtype=F32)
    emission[hit] = mvals[tri[hit], 3:6]
    aov = {"ray": np.concatenate([o, d], axis=1).reshape(32, 32, 6), "t": t.reshape(32, 32), "tri": tri.reshape(32, 32),
           "normal": normal.reshape(32, 32, 3), "emission": emission.reshape(32, 32, 3)}
    den, _ = ptamd.denoise(noisy, ptamd.denoise_guides(aov), var)
    truth, _ = O.render(sc, 2048, 5)
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(F64) - truth.astype(F64)) ** 2)))
    e_noisy, e_den = rmse(noisy), rmse(den)
    print(f"{name}: RMSE noisy {e_noisy:.4f} denoised {e_den:.4f} ratio {e_den / e_noisy:.3f}")
    assert hit.any() and e_noisy > 0
    assert e_den < e_noisy
