"""Material gradients of trace() without a device: the formulas of tests/_refgrad.py against a
complex-step derivative of the fold itself, then pt_bvh_trace_grad (ptamd.BVH.trace_grad) against
_refgrad within the derived any-order summation tolerance, and the argument handling of
pt_bvh_trace_grad / pt_ctx_trace_grad."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import _refgrad as RG
import _reftrace as RT
import _refwalk as RW
import _treecases as TC

F32 = np.float32
N = 257


@functools.lru_cache(maxsize=None)
def _bvh(name):
    import ptamd
    b = ptamd.BVH.from_scene(RT.make_scene(name))
    b.build()
    return b


def test_formulas_match_complex_step_of_the_fold():
    """_refgrad anchored on trace() itself: its float32 unwinding is `_reftrace.radiance`'s bits,
    and its analytic terms, evaluated in float64, equal the complex-step derivative (h = 1e-30) of
    the float64 unwinding of sum(grad_rgb * rgb), one colour and one emission channel at a time,
    on the 6 triangles with the most terms (64 paths of cornell+glow, depth 5)."""
    name, n, depth, h = "cornell+glow", 64, 5, 1e-30
    P = RT.head(RT.paths(name), n)
    g = RG.grad_rgb(n)
    RT.assert_same(RG.path_terms(P, depth, g).rgb, RT.radiance(P, depth)[0], "the helper's unwinding")
    t64 = RG.path_terms(P, depth, g, dtype=np.float64)
    S = RG.summarize(t64, P.mvals.shape[0])
    tris = np.argsort(-(S.count[0] + S.count[1]))[:6]
    assert (S.count[0][tris] > 0).all() and (S.count[1][tris] > 0).all()
    color, emit = P.mvals[:, 0:3].astype(np.complex128), P.mvals[:, 3:6].astype(np.complex128)
    g64 = g.astype(np.float64)
    checked = 0
    for tri in tris:
        for c in range(3):
            for kind, base in ((RG.COLOR, color), (RG.EMIT_K, emit)):
                pert = base.copy()
                pert[tri, c] += 1j * h
                args = (pert, emit) if kind == RG.COLOR else (color, pert)
                rgb = RG.path_terms(P, depth, g, 1, *args, dtype=np.complex128).rgb
                step = float((g64 * rgb.imag).sum() / h)
                want = S.exact[kind, tri, c]
                assert want != 0.0
                assert abs(step - want) <= 1e-12 * abs(want), (tri, c, kind, step, want)
                checked += 1
    assert checked == 36


def test_expected_gradients_are_not_vacuous():
    """On cornell+glow (257 rays, depth 5) the expected d color is non-zero on at least 8
    triangles and d emit on every first-hit triangle (the restatement alone: 30 and 31 triangles
    of 36 at these counts)."""
    P = RT.head(RT.paths("cornell+glow"), N)
    _, S = RG.expected("cornell+glow", N, 5)
    assert int((S.exact[RG.COLOR] != 0).any(axis=1).sum()) >= 8
    first = np.unique(P.tri[0][P.tri[0] >= 0])
    assert first.size >= 8 and (S.exact[RG.EMIT_K][first] != 0).any(axis=1).all()


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("name", ["cornell+glow", "random_7_300", "sphere12+glow"])
def test_host_path_matches_refgrad(name, spp):
    o, d = RT.rays(name, N)
    g = RG.grad_rgb(N)
    b = _bvh(name)
    for depth in (1, 2, 5):
        t, S = RG.expected(name, N, depth, spp)
        got, st = b.trace_grad(o, d, g, depth, samples=spp)
        RG.assert_within(got["color"], got["emit"], S, f"{name} depth {depth} spp {spp}")
        assert st["terms"] == S.terms > 0 and st["paths"] == N * spp
        rgb, st_t = b.trace(o, d, depth, samples=spp)
        RT.assert_same(got["rgb"], rgb, "rgb_out vs pt_bvh_trace")
        RT.assert_same(got["rgb"], RG.mean_rgb(t, spp), "rgb_out vs the helper")
        assert st["rays"] == st_t["rays"]
        assert (S.exact[RG.EMIT_K] != 0).any()
    assert (S.exact[RG.COLOR] != 0).any()  # depth 5


def test_single_paths_sum_in_k_order():
    """n = 1, spp = 1: the double sum in k order, bit for bit (32 rays of random_7_300, depth 8)."""
    name, depth = "random_7_300", 8
    P = RT.paths(name)
    o, d = RT.rays(name, 32)
    seeds = RT.sample_seeds(32, 1, 1)[:, 0]
    g = RG.grad_rgb(32)
    b = _bvh(name)
    bounces = 0
    for i in range(32):
        Pi = RT.Paths(P.tri[:, i:i + 1], P.cos[:, i:i + 1], P.state[:, i:i + 1], P.init[i:i + 1], P.mtype, P.mvals)
        t = RG.path_terms(Pi, depth, g[i:i + 1])
        S = RG.summarize(t, P.mvals.shape[0])
        got, st = b.trace_grad(o[i:i + 1], d[i:i + 1], g[i:i + 1], depth, states=seeds[i:i + 1])
        assert np.array_equal(got["color"].view(np.uint64), S.ordered[RG.COLOR].view(np.uint64)), i
        assert np.array_equal(got["emit"].view(np.uint64), S.ordered[RG.EMIT_K].view(np.uint64)), i
        assert st["terms"] == S.terms
        bounces += int((t.kind == RG.COLOR).sum())
    assert bounces >= 32  # more than one term per destination somewhere


@pytest.mark.parametrize("name", ["cornell+glow", "random_7_300"])
def test_overrides(name):
    """color / emit overrides: rgb_out is pt_bvh_trace on a BVH rebuilt with those materials, bit
    for bit, and the gradients are the helper's at the overridden values."""
    import ptamd
    o, d = RT.rays(name, N)
    g = RG.grad_rgb(N)
    sc = RT.make_scene(name)
    color, emit = RG.overrides(len(sc.mats))
    got, st = _bvh(name).trace_grad(o, d, g, 5, color=color, emit=emit)
    sc.mats = [dataclasses.replace(m, color=tuple(float(x) for x in color[i]), emit=tuple(float(x) for x in emit[i]))
               for i, m in enumerate(sc.mats)]
    rebuilt = ptamd.BVH.from_scene(sc)
    rebuilt.build()
    RT.assert_same(got["rgb"], rebuilt.trace(o, d, 5)[0], "override vs a rebuilt scene")
    t, S = RG.expected(name, N, 5, override=True)
    RG.assert_within(got["color"], got["emit"], S, f"{name} override")
    assert st["terms"] == S.terms
    RT.assert_same(got["rgb"], t.rgb, "override vs the helper")
    plain, _ = _bvh(name).trace_grad(o, d, g, 5)
    assert not np.array_equal(plain["color"], got["color"]) and not np.array_equal(plain["rgb"], got["rgb"])
    # one override at a time
    only_c, _ = _bvh(name).trace_grad(o, d, g, 5, color=color, want=("rgb",))
    sc2 = RT.make_scene(name)
    sc2.mats = [dataclasses.replace(m, color=tuple(float(x) for x in color[i])) for i, m in enumerate(sc2.mats)]
    RT.assert_same(only_c["rgb"], ptamd.BVH.from_scene(sc2).trace(o, d, 5)[0], "color override alone")
    assert set(only_c) == {"rgb"}


@pytest.mark.parametrize("name,variant", RT.TREES)
def test_caller_built_trees(name, variant):
    """Gradients are indexed by the caller's triangle, whatever leaves hold it."""
    import ptamd
    o, d, st, t, S = RG.tree_expected(name, variant)
    c = TC.case(name, variant)
    color, emit = RG.overrides(c.verts.shape[0])
    got, stats = TC.to_bvh(ptamd, c).trace_grad(o, d, RG.grad_rgb(256), 5, color=color, emit=emit)
    RG.assert_within(got["color"], got["emit"], S, f"{name} {variant}")
    RT.assert_same(got["rgb"], t.rgb, f"{name} {variant} rgb")
    assert stats["terms"] == S.terms
    assert (S.exact[RG.COLOR] != 0).any(axis=1).sum() >= 8
    if variant in ("duplicated", "dropped"):
        hit = (S.count[RG.EMIT_K] > 0)
        assert hit[c.tri] == (variant == "duplicated")  # the triangle in two leaves gets one sum; a dropped one none


def test_argument_handling():
    import ptamd
    from ptamd import _lib
    L = ptamd.lib()
    b = _bvh("cornell")
    ref = ptamd._SceneRef(b)
    T = len(b.triangles)
    o, d = RT.rays("cornell", 4)
    g = RG.grad_rgb(4)
    rgb = np.full((4, 3), -1.0, dtype=np.float32)
    gc, ge = np.full((T, 3), -1.0), np.full((T, 3), -1.0)
    st = _lib.pt_grad_stats()
    ok = _lib.pt_trace_params(5, 1, 1, None)

    def io(grad_rgb=g.ctypes.data, out=rgb.ctypes.data, color=gc.ctypes.data, emit=ge.ctypes.data):
        return _lib.pt_trace_grad_io(None, None, grad_rgb, out, color, emit)

    def host(scene=ref.s, org=o.ctypes.data, dirs=d.ctypes.data, n=4, prm=ok, x=None):
        x = io() if x is None else x
        return L.pt_bvh_trace_grad(C.byref(scene) if scene is not None else None, org, dirs, n,
                                   C.byref(prm) if prm is not None else None, C.byref(x) if x is not False else None,
                                   C.byref(st))

    def arg_error(rc):
        assert rc == _lib.PT_E_ARG
        assert L.pt_last_error()

    assert host() == 0 and st.terms > 0 and (ge != 0).any()
    arg_error(host(x=io(grad_rgb=None)))                # a gradient output without grad_rgb
    assert host(x=io(grad_rgb=None, color=None, emit=None)) == 0   # forward only
    assert host(x=io(out=None)) == 0                    # gradients only
    arg_error(host(x=False))
    arg_error(host(n=-1))
    arg_error(host(scene=None))
    arg_error(host(org=None))
    arg_error(host(prm=None))
    for depth, spp in ((-1, 1), (_lib.PT_MAX_DEPTH + 1, 1), (5, 0), (5, -3), (5, (1 << 20) + 1)):
        arg_error(host(prm=_lib.pt_trace_params(depth, spp, 1, None)))
    # n == 0 zeroes the gradient outputs
    gc[:], ge[:] = -1.0, -1.0
    assert host(org=None, dirs=None, n=0, x=io(grad_rgb=None, out=None)) == 0
    assert not gc.any() and not ge.any() and st.terms == 0
    # depth 0: all zeros
    gc[:], ge[:], rgb[:] = -1.0, -1.0, -1.0
    assert host(prm=_lib.pt_trace_params(0, 1, 1, None)) == 0
    assert not gc.any() and not ge.any() and not RW.bits(rgb).any() and st.terms == 0 and st.trace.rays == 0
    # a NULL context (no device needed for these returns)
    x = io()
    arg_error(L.pt_ctx_trace_grad(None, o.ctypes.data, d.ctypes.data, 4, C.byref(ok), C.byref(x), 0, C.byref(st)))
    with pytest.raises(ValueError):
        b.trace_grad(o, d, None, 5)                     # the wrapper refuses it before the library does
    with pytest.raises(ValueError):
        b.trace_grad(o, d, g, 5, color=np.zeros((T + 1, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        b.trace_grad(o, d, g, 5, want=("rgb", "albedo"))


def test_symbols_and_struct_sizes():
    import ptamd
    L = ptamd.lib()
    assert L.pt_abi_version() == 3
    for name in ("pt_bvh_trace_grad", "pt_ctx_trace_grad"):
        assert hasattr(L, name), name
        assert name in ptamd._lib.EXPORTED
    assert C.sizeof(ptamd._lib.pt_trace_grad_io) == 48
    assert C.sizeof(ptamd._lib.pt_grad_stats) == 64 + 24
