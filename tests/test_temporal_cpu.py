"""Temporal reprojection on the host (pt_image_temporal; ptamd.temporal_accumulate,
ptamd.TemporalHistory). No device is needed.

The yardstick is tests/_reftemporal.py: a float32 numpy restatement of the contract in
include/pt_hip.h, which shares no code with the library. The results are defined bit for bit, so
every comparison is of bits (NaN equals NaN)."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import _oracle as O
import _refdenoise as RD
import _reftemporal as RT
import _reftrace as RTR

F32, F64 = np.float32, np.float64

SIZES = [(1, 1), (1, 7), (5, 1), (37, 23), (64, 64), (131, 67)]  # (W, H)
MODES = [RT.SAMPLE, RT.TEMPORAL]


def test_symbols_and_structs():
    import ptamd
    from ptamd import _lib
    L = ptamd.lib()
    for name in ("pt_image_temporal", "pt_ctx_temporal", "pt_ctx_render_temporal"):
        assert hasattr(L, name) and name in _lib.EXPORTED
    assert C.sizeof(_lib.pt_temporal_params) == 16
    assert C.sizeof(_lib.pt_temporal_history) == 7 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.pt_temporal_stats) == 24
    assert C.sizeof(_lib.pt_render_temporal_stats) == 48 + 24 + 96
    assert (ptamd.PT_TEMPORAL_VAR_SAMPLE, ptamd.PT_TEMPORAL_VAR_TEMPORAL) == (RT.SAMPLE, RT.TEMPORAL)
    assert callable(ptamd.temporal_accumulate) and callable(ptamd.TemporalHistory.empty)
    for f in ("temporal_accumulate", "render_temporal"):
        assert callable(getattr(ptamd.Renderer, f))
    h = ptamd.TemporalHistory.empty(5, 3)
    assert h.color.shape == (3, 5, 3) and h.hist.shape == (3, 5) and h.hist.dtype == np.int32 and not h.hist.any()
    assert tuple(h.planes()) == RT.NAMES


def cameras(s):
    import ptamd
    cur = ptamd.Camera(*RT.camera_spec(s.cam_cur))
    return cur, (cur if s.cam_prev is s.cam_cur else ptamd.Camera(*RT.camera_spec(s.cam_prev)))


@functools.lru_cache(maxsize=None)
def reference(W, H, move, mode):
    """The restatement's (next, reused) for the synthetic frame, on the library's cameras."""
    s = RT.synthetic(W, H, seed=W * 100 + H, move=move)
    cur, old = cameras(s)
    return RT.accumulate(s.color, s.guides, cur.c, old.c, s.prev, s.var, mode=mode)


def history(planes):
    import ptamd
    return ptamd.TemporalHistory(**{k: np.ascontiguousarray(planes[k]) for k in RT.NAMES})


def assert_history(got, want, what):
    for k in RT.NAMES:
        g = getattr(got, k)
        if k in ("hist", "cls"):
            assert g.dtype == np.int32 and np.array_equal(g, want[k]), f"{what}: {k}"
        else:
            RD.assert_same(g, want[k], f"{what}: {k}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("move", RT.MOVES)
@pytest.mark.parametrize("W,H", SIZES)
def test_matches_the_restatement(W, H, move, mode):
    import ptamd
    s = RT.synthetic(W, H, seed=W * 100 + H, move=move)
    cur, old = cameras(s)
    want, want_reused = reference(W, H, move, mode)
    hit = int((RD.classes(s.guides["tri"], s.guides["emission"]) != 0).sum())
    if move == "pixels" and W * H >= 20:
        # both branches are exercised, or the comparison below shows little (a single pixel or a
        # single row or column cannot promise this: the move takes most of it out of the image)
        assert 0.3 * hit <= want_reused <= 0.9 * hit, (want_reused, hit)
    if move == "turned":
        assert want_reused == 0
    if move == "far" and W >= 20:
        assert 0 < want_reused < 0.3 * hit
    got, reused = ptamd.temporal_accumulate(s.color, s.guides, cur, history(s.prev), old, var=s.var, variance_mode=mode)
    assert reused == want_reused
    assert_history(got, want, f"{W}x{H} {move} mode {mode}")
    # the default mode follows var
    dflt, r2 = ptamd.temporal_accumulate(s.color, s.guides, cur, history(s.prev), old,
                                         var=s.var if mode == RT.SAMPLE else None)
    assert r2 == want_reused
    assert_history(dflt, want, "default mode")
    if W * H >= 20 and move in ("none", "subpixel", "pixels"):
        c = want["color"]
        seeded = np.isnan(s.color).any(axis=-1)
        assert seeded.sum() == 1 and np.isnan(c[seeded]).any()  # a NaN of the current frame stays ...
        assert np.isfinite(c[~seeded]).all()  # ... and none of the history's enters
        assert want["hist"].max() <= 32 and want["hist"].min() == 1
        if move == "none":  # every pixel looks up itself: the planted counts at and above max_history end at 32
            assert (want["hist"] == 32).sum() >= 2
        if mode == RT.TEMPORAL:
            assert np.isposinf(want["var"][want["hist"] == 1]).all()


def test_first_frame_and_parameters():
    import ptamd
    s = RT.synthetic(37, 23, seed=3, move="pixels")
    cur, old = cameras(s)
    for mode in MODES:
        want, r = RT.accumulate(s.color, s.guides, cur.c, None, None, s.var, mode=mode)
        got, reused = ptamd.temporal_accumulate(s.color, s.guides, cur, var=s.var, variance_mode=mode)
        assert r == reused == 0 and (got.hist == 1).all()
        assert_history(got, want, f"first frame, mode {mode}")
        RD.assert_same(got.color, s.color, "first frame: c' = c")
    # explicit parameters are honoured
    kw = dict(max_history=5, sigma_z=0.002, normal_min=0.95)
    want, r = RT.accumulate(s.color, s.guides, cur.c, old.c, s.prev, s.var, **kw)
    got, reused = ptamd.temporal_accumulate(s.color, s.guides, cur, history(s.prev), old, var=s.var, **kw)
    assert r == reused and got.hist.max() == 5
    assert_history(got, want, "explicit parameters")
    dflt, _ = ptamd.temporal_accumulate(s.color, s.guides, cur, history(s.prev), old, var=s.var)
    assert not RD.same_bits(got.color, dflt.color).all()
    # the inputs are left as they were
    again = RT.synthetic(37, 23, seed=3, move="pixels")
    for k in RT.NAMES:
        assert np.array_equal(RD.bits(s.prev[k]) if s.prev[k].dtype == F32 else s.prev[k],
                              RD.bits(again.prev[k]) if s.prev[k].dtype == F32 else again.prev[k])


@pytest.mark.parametrize("max_history", [0, 4])
def test_a_static_camera_follows_the_recurrence(max_history):
    """cam_prev == cam_cur bit for bit: the lookup is pixel p itself with weight 1, so K frames
    reproduce c_N = (b*c_{N-1}) + (alpha*c) with alpha = 1/N, which sticks at 1/max_history."""
    import ptamd
    W, H, K = 37, 23, 6
    s = RT.synthetic(W, H, seed=11, move="none")
    cur, _ = cameras(s)
    rng = np.random.default_rng(5)
    frames = [rng.uniform(0, 2, (H, W, 3)).astype(F32) for _ in range(K)]
    hit = RD.classes(s.guides["tri"], s.guides["emission"]) != 0
    hist, acc = None, None
    for N, c in enumerate(frames, start=1):
        hist, reused = ptamd.temporal_accumulate(c, s.guides, cur, hist, cur if hist is not None else None,
                                                 max_history=max_history)
        assert reused == (0 if N == 1 else int(hit.sum()))
        n_eff = min(N, max_history or 32)
        alpha = F32(1) / F32(n_eff)
        b = F32(1) - alpha
        acc = c if N == 1 else np.where(hit[..., None], (b * acc) + (alpha * c), c)
        RD.assert_same(hist.color, acc, f"frame {N}")
        assert (hist.hist[hit] == n_eff).all() and (hist.hist[~hit] == 1).all()
    assert hit.any() and not hit.all()


def _frame(sc, seed0, spp, depth):
    """One frame of `spp` independent oracle samples: (mean, variance of the mean, guides)."""
    import ptamd
    W, H = sc.camera.res
    x = np.stack([O.render(sc, 1, depth, seed=seed0 + s)[0] for s in range(spp)]).astype(F64)
    S, Q = x.sum(axis=0), (x * x).sum(axis=0)
    o, d, _ = RTR.camera_rays(sc, seed0)
    t, tri = ptamd.BVH.from_scene(sc).intersect(o, d)
    verts, _, mvals = O.pack_scene(sc)
    hit = tri >= 0
    normal = np.zeros((W * H, 3), dtype=F32)
    normal[hit] = RD.tri_normal(verts, tri[hit], d[hit])
    emission = np.zeros((W * H, 3), dtype=F32)
    emission[hit] = mvals[tri[hit], 3:6]
    aov = {"ray": np.concatenate([o, d], axis=1).reshape(H, W, 6), "t": t.reshape(H, W), "tri": tri.reshape(H, W),
           "normal": normal.reshape(H, W, 3), "emission": emission.reshape(H, W, 3)}
    return (S / spp).astype(F32), ptamd.moments_variance(S, Q, spp), ptamd.denoise_guides(aov)


@functools.lru_cache(maxsize=None)
def _truth():
    from ptamd import scenes
    return O.render(scenes.cornell((32, 32)), 2048, 3)[0]


@pytest.mark.parametrize("path", ["static", "moving"])
def test_quality(path):
    """Cornell 32 x 32, depth 3, frames of 4 independent oracle samples per pixel, truth the oracle
    at 2048 spp from the last frame's camera: eight frames through accumulate + filter come closer
    to it than the last frame through the filter alone, for a static camera and for one that moves
    by about one pixel per frame (28 units along x; the last position is the scene's own camera).
    Measured (bit-defined, so these are the values), RMSE of the last frame 0.0515,
    of the last frame filtered alone 0.0362; static: accumulated 0.0362, accumulated + filtered
    0.0348; moving: accumulated 0.0282, accumulated + filtered 0.0297."""
    import ptamd
    from ptamd import scenes
    base = scenes.cornell((32, 32))
    K, spp, depth, step = 8, 4, 3, 28.0
    hist, cam_old, reused = None, None, []
    for f in range(K):
        dx = step * (K - 1 - f) if path == "moving" else 0.0
        pos = (base.camera.pos[0] - dx, base.camera.pos[1], base.camera.pos[2])
        sc = dataclasses.replace(base, camera=dataclasses.replace(base.camera, pos=pos))
        cam = ptamd.Camera.from_spec(sc.camera)
        noisy, var, g = _frame(sc, 1000 + 16 * f, spp, depth)
        hist, r = ptamd.temporal_accumulate(noisy, g, cam, hist, cam_old, var=var)
        reused.append(r)
        cam_old = cam
    alone, _ = ptamd.denoise(noisy, g, var)
    both, _ = ptamd.denoise(hist.color, g, hist.var)
    truth = _truth()
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(F64) - truth.astype(F64)) ** 2)))
    e_noisy, e_alone, e_acc, e_both = rmse(noisy), rmse(alone), rmse(hist.color), rmse(both)
    print(f"{path}: RMSE last frame {e_noisy:.4f}, filtered alone {e_alone:.4f}, accumulated {e_acc:.4f}, "
          f"accumulated + filtered {e_both:.4f}; reused {reused}")
    assert reused[0] == 0 and min(reused[1:]) > 0.5 * 32 * 32
    assert e_both < e_alone


def _call(W, H, cur, old, color, var, g, prev, nxt, prm):
    import ptamd
    from ptamd import _lib
    gs = _lib.pt_denoise_guides()
    for k, a in g.items():
        setattr(gs, k, a.ctypes.data if a is not None else None)
    hs = []
    for h in (prev, nxt):
        s = _lib.pt_temporal_history()
        for k, a in (h or {}).items():
            setattr(s, k, a.ctypes.data if a is not None else None)
        hs.append(s)
    p = _lib.pt_temporal_params(*prm) if prm is not None else None
    return ptamd.lib().pt_image_temporal(W, H, C.byref(cur.c) if cur is not None else None,
                                         C.byref(old.c) if old is not None else None,
                                         color.ctypes.data if color is not None else None,
                                         var.ctypes.data if var is not None else None, C.byref(gs),
                                         C.byref(hs[0]) if prev is not None else None,
                                         C.byref(hs[1]) if nxt is not None else None,
                                         C.byref(p) if p is not None else None, None)


def test_argument_errors():
    import ptamd
    from ptamd import _lib
    W, H = 6, 4
    s = RT.synthetic(W, H, seed=1, move="subpixel")
    cur, old = cameras(s)
    prev = {k: np.ascontiguousarray(v) for k, v in s.prev.items()}
    nxt = {k: np.zeros_like(v) for k, v in prev.items()}
    ok = (0, 0.0, 0.0, 0)
    base = dict(W=W, H=H, cur=cur, old=old, color=s.color, var=s.var, g=s.guides, prev=prev, nxt=nxt, prm=ok)
    assert _call(**base) == 0
    assert _call(**dict(base, prm=None)) == 0  # NULL params: every default
    assert _call(**dict(base, prev=None, old=None)) == 0
    assert _call(**dict(base, var=None)) == 0  # temporal mode by default
    assert _call(**dict(base, var=None, prm=(0, 0, 0, RT.TEMPORAL), prev=dict(prev, var=None))) == 0
    whole = np.zeros((2, H, W, 3), dtype=F32)  # two planes that share their middle
    bad = [
        dict(W=0), dict(H=-1), dict(W=1 << 16, H=(1 << 14) + 1),  # W*H > 2^30, checked before any array is read
        dict(cur=None), dict(color=None), dict(nxt=None), dict(old=None),  # prev without its camera
        dict(var=None, prm=(0, 0, 0, RT.SAMPLE)),  # sample mode needs var
        dict(prev=dict(prev, var=None)),  # ... and the previous var
        dict(prm=(-1, 0, 0, 0)), dict(prm=(65536, 0, 0, 0)), dict(prm=(0, -0.01, 0, 0)), dict(prm=(0, float("nan"), 0, 0)),
        dict(prm=(0, 0, 1.0, 0)), dict(prm=(0, 0, -0.5, 0)), dict(prm=(0, 0, float("nan"), 0)), dict(prm=(0, 0, 0, 3)),
        dict(prm=(0, 0, 0, -1)),
        dict(nxt=dict(nxt, color=prev["color"])),  # the same plane
        dict(nxt=dict(nxt, m2=prev["color"])),  # another plane of the previous history
        dict(prev=dict(prev, color=whole[0]), nxt=dict(nxt, color=whole.reshape(-1)[W * H:W * H + 3 * W * H])),  # partly
        dict(nxt=dict(nxt, hist=prev["cls"])),
    ] + [dict(g=dict(s.guides, **{k: None})) for k in _lib.pt_denoise_guides.NAMES] \
      + [dict(nxt=dict(nxt, **{k: None})) for k in RT.NAMES] \
      + [dict(prev=dict(prev, **{k: None})) for k in RT.NAMES]
    for b in bad:
        assert _call(**dict(base, **b)) == _lib.PT_E_ARG, b
    assert b"needed" in ptamd.lib().pt_last_error()
    assert _call(**dict(base, prm=(65535, 0, 0, 0))) == 0 and _call(**dict(base, prm=(1, 0, 0, 0))) == 0
    with pytest.raises(ValueError):
        ptamd.temporal_accumulate(s.color, s.guides, cur, history(s.prev))  # prev without prev_camera
    with pytest.raises(ValueError):
        ptamd.temporal_accumulate(s.color, s.guides, cur, history(dict(s.prev, hist=s.prev["hist"].astype(np.int64))), old)
