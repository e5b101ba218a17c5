"""Material gradients of the light-sampling estimator without a device: the formulas of
tests/_refneegrad.py against the estimator itself (its forward bits are `_refnee` / `_refmis`'s, its
analytic terms the complex-step derivative of its own float64 forward form), then
pt_bvh_trace_nee_grad (ptamd.BVH.trace_nee_grad) against the restatement within the derived
any-order summation tolerance, the expectation against trace_grad's, and the argument handling of
pt_bvh_trace_nee_grad / pt_ctx_trace_nee_grad."""
import ctypes as C
import functools

import numpy as np
import pytest

import _refgrad as RG
import _refmis as RM
import _refnee as RN
import _refneegrad as NG
import _reftrace as RT
import _refwalk as RW
import _treecases as TC

F32 = np.float32
N = NG.N
MIS = pytest.mark.parametrize("mis", [False, True], ids=["plain", "mis"])


@functools.lru_cache(maxsize=None)
def _bvh(name):
    import ptamd
    b = ptamd.BVH.from_scene(NG.make_scene(name))
    b.build()
    return b


def _complex_step(name, n, depth, mis):
    """The restatement on the first n paths of the scene's set: the float32 forward bits against
    `_refnee` / `_refmis`, then every analytic sum in float64 against the complex-step derivative
    (h = 1e-30) of the float64 forward form of sum(grad_rgb * rgb), one colour and one emission
    channel at a time, on the six triangles with the most terms and on every light triangle.
    Returns (checked values, visible-light terms, weighted-hit terms on the checked destinations)."""
    h = 1e-30
    W = NG.walked(name, n, 1, mis)
    g = RG.grad_rgb(n)
    if name == "tri3":
        ref = RM.radiance(RM.edge_paths(n, depth), depth)[0] if mis else None  # `_refnee` has no tri3 set
    else:
        ref = RM.radiance(RM.head(RM.paths(name), n), depth)[0] if mis else RN.radiance(RN.head(RN.paths(name), n), depth)[0]
    if ref is not None:
        RT.assert_same(NG.path_terms(W, depth, g).rgb, ref, "the restatement's forward form")
    t64 = NG.path_terms(W, depth, g, dtype=np.float64)
    T = W.mvals.shape[0]
    S = NG.summarize(t64, T)
    tris = list(np.argsort(-(S.count[0] + S.count[1]), kind="stable")[:6])
    tris += [int(j) for j in W.lights.tri if int(j) not in tris]
    vis = NG.case_counts(t64, NG.T_LIGHT, T)
    whit = NG.case_counts(t64, NG.T_END_WEIGHTED, T)
    if not mis:
        assert whit.sum() == 0  # the unweighted estimator has no such term: it drops those hits
    color, emit = W.mvals[:, 0:3].astype(np.complex128), W.mvals[:, 3:6].astype(np.complex128)
    g64 = g.astype(np.float64)
    checked = 0
    for tri in tris:
        for c in range(3):
            for kind, base in ((RG.COLOR, color), (RG.EMIT_K, emit)):
                want = S.exact[kind, tri, c]
                if S.count[kind, tri] == 0:
                    assert want == 0.0
                    continue
                pert = base.copy()
                pert[tri, c] += 1j * h
                args = (pert, emit) if kind == RG.COLOR else (color, pert)
                rgb = NG.path_terms(W, depth, g, 1, *args, dtype=np.complex128).rgb
                step = float((g64 * rgb.imag).sum() / h)
                assert abs(step - want) <= 1e-12 * abs(want), (name, tri, c, kind, step, want)
                checked += 1
    assert all(S.count[RG.EMIT_K, int(j)] > 0 for j in W.lights.tri)  # every light's d emit was checked
    return checked, int(vis[:, tris].sum()), int(whit[:, tris].sum())


@MIS
def test_formulas_match_the_estimator_itself(mis):
    """The restatement anchored on the estimator (`_complex_step`) on 64 paths of cornell+glow,
    depth 5: some checked destination receives a visible-light term.

    Those 64 paths hold no EMIT hit after a light draw (`_refmis.weighted_counts` counts 0 of them,
    and 1 among the first 256), so no destination there can receive a weighted-hit term. The
    weighted case is therefore checked, by the same procedure and bound, on a second input beside
    the first: tri3's first 64 edge rays at depth 5, where 40 paths end in a weighted hit."""
    checked, vis, _ = _complex_step("cornell+glow", 64, 5, mis)
    assert checked >= 30 and vis > 0, (checked, vis)
    checked, vis, whit = _complex_step("tri3", 64, 5, mis)
    assert checked >= 6 and vis > 0, (checked, vis)
    if mis:
        assert whit > 0, "no checked destination receives a weighted-hit term"


@MIS
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("name", NG.SCENES)
def test_host_form_matches_restatement(name, spp, mis):
    o, d = NG.rays(name, N)
    g = RG.grad_rgb(N)
    b = _bvh(name)
    lit = 0
    for depth in NG.DEPTHS:
        t, S = NG.expected(name, N, depth, spp, mis)
        got, st = b.trace_nee_grad(o, d, g, depth, samples=spp, mis=mis)
        what = f"{name} depth {depth} spp {spp} mis {mis}"
        RG.assert_within(got["color"], got["emit"], S, what)
        assert st["terms"] == S.terms > 0 and st["paths"] == N * spp
        rgb, st_f = b.trace_nee(o, d, depth, samples=spp, mis=mis)
        RT.assert_same(got["rgb"], rgb, what + ": rgb_out vs pt_bvh_trace_nee_opt")
        RT.assert_same(got["rgb"], NG.mean_rgb(t, spp), what + ": rgb_out vs the restatement")
        assert st["shadow_rays"] == st_f["shadow_rays"] == t.shadow and st["light_draws"] == st_f["light_draws"] == t.draws
        assert st["rays"] == st_f["rays"] == t.segments and st["lights"] == st_f["lights"]
        lit += int((t.case == NG.T_LIGHT).sum())
    assert lit > 0 and (S.exact[RG.COLOR] != 0).any() and (S.exact[RG.EMIT_K] != 0).any()


@MIS
def test_single_paths_sum_in_k_order(mis):
    """n = 1, spp = 1: the double sums in k order, bit for bit (32 rays of random_7_300, depth 8)."""
    name, depth = "random_7_300", 8
    W = NG.walked(name, 32, 1, mis)
    o, d = NG.rays(name, 32)
    seeds = RT.sample_seeds(32, 1, 1)[:, 0]
    g = RG.grad_rgb(32)
    b = _bvh(name)
    T = W.mvals.shape[0]
    lit = 0
    for i in range(32):
        Wi = NG.Walk(*(a[:, i:i + 1] for a in W[:9]), *W[9:])
        t = NG.path_terms(Wi, depth, g[i:i + 1])
        S = NG.summarize(t, T)
        got, st = b.trace_nee_grad(o[i:i + 1], d[i:i + 1], g[i:i + 1], depth, states=seeds[i:i + 1], mis=mis)
        assert np.array_equal(got["color"].view(np.uint64), S.ordered[RG.COLOR].view(np.uint64)), i
        assert np.array_equal(got["emit"].view(np.uint64), S.ordered[RG.EMIT_K].view(np.uint64)), i
        assert st["terms"] == S.terms
        lit += int((t.case == NG.T_LIGHT).sum())
    assert lit >= 8  # destinations with a light's term beside the suffix term


@MIS
def test_without_lights_it_is_trace_grad(mis):
    """A scene whose emitter is a DIFFUSE material with emission has no light table: no draw is
    made, the terms coincide with pt_bvh_trace_grad's by construction, and the single-path sums
    are bit-identical."""
    import ptamd
    b = _bvh("no_lights")
    assert ptamd.scene_lights(b)["tri"].size == 0
    o, d = NG.rays("no_lights", 32)
    g = RG.grad_rgb(32)
    terms = 0
    for i in range(32):
        got, st = b.trace_nee_grad(o[i:i + 1], d[i:i + 1], g[i:i + 1], 5, mis=mis)
        want, st_w = b.trace_grad(o[i:i + 1], d[i:i + 1], g[i:i + 1], 5)
        for k in ("color", "emit"):
            assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (i, k)
        assert st["terms"] == st_w["terms"] and st["light_draws"] == 0 and st["lights"] == 0 and st["rays"] == st_w["rays"]
        terms += st["terms"]
    assert terms > 64


@MIS
@pytest.mark.parametrize("name", ["cornell+glow", "random_7_300"])
def test_overrides(name, mis):
    """The gradients and rgb_out at overridden colours and emissions are the restatement's at those
    values; the scene and its light table are unchanged afterwards."""
    import ptamd
    o, d = NG.rays(name, N)
    g = RG.grad_rgb(N)
    b = _bvh(name)
    color, emit = RG.overrides(len(b.triangles))
    lights0 = ptamd.scene_lights(b)
    mats0 = bytes(b.materials())
    got, st = b.trace_nee_grad(o, d, g, 5, color=color, emit=emit, mis=mis)
    t, S = NG.expected(name, N, 5, 1, mis, override=True)
    RG.assert_within(got["color"], got["emit"], S, f"{name} override")
    assert st["terms"] == S.terms
    RT.assert_same(got["rgb"], t.rgb, "override vs the restatement")
    plain, _ = b.trace_nee_grad(o, d, g, 5, mis=mis)
    assert not np.array_equal(plain["color"], got["color"]) and not np.array_equal(plain["rgb"], got["rgb"])
    RT.assert_same(plain["rgb"], b.trace_nee(o, d, 5, mis=mis)[0], "no override after an override")
    lights1 = ptamd.scene_lights(b)
    assert bytes(b.materials()) == mats0 and lights1["area"] == lights0["area"]
    assert np.array_equal(lights1["tri"], lights0["tri"]) and np.array_equal(lights1["cdf"], lights0["cdf"])


@MIS
def test_zeroed_light_keeps_the_scenes_table(mis):
    """An override that zeroes a listed light's emission still draws from the scene's table: the
    walk, the counts and the terms are the restatement's with the table fixed."""
    name = "cornell+glow"
    b = _bvh(name)
    W = NG.walked(name, N, 1, mis)
    T = W.mvals.shape[0]
    emit = W.mvals[:, 3:6].copy()
    emit[W.lights.tri[0]] = 0.0
    o, d = NG.rays(name, N)
    g = RG.grad_rgb(N)
    t = NG.path_terms(W, 5, g, 1, None, emit)
    S = NG.summarize(t, T)
    got, st = b.trace_nee_grad(o, d, g, 5, emit=emit, mis=mis)
    RG.assert_within(got["color"], got["emit"], S, "zeroed light")
    RT.assert_same(got["rgb"], t.rgb, "zeroed light rgb")
    assert st["terms"] == S.terms and st["lights"] == W.lights.tri.size and st["shadow_rays"] == t.shadow > 0
    assert NG.case_counts(t, NG.T_LIGHT, T)[RG.EMIT_K, W.lights.tri[0]] > 0  # its d emit still gets the pairs


def test_same_expectation_as_trace_grad():
    """Cornell's camera rays at 16^2, 262,144 paths per estimator (64 batches of 16 samples a ray,
    seeds 1..64), depth 3, mis=True, dLoss/d rgb = 1: d emit summed over the light's triangles
    (three channels) and d color of the three triangles with the largest |gradient| (nine values)
    agree with trace_grad's within 4.5 standard errors of the difference (a two-sided tail of 7e-6
    per value), the standard errors taken from the 64 batch means; and the light-sampling standard
    error of d emit is the smaller one: the feature's point."""
    import ptamd
    sc = RT.make_scene("cornell")
    b = ptamd.BVH.from_scene(sc)
    b.build()
    o, d, _ = RT.camera_rays(sc, 1)
    n, spp, batches, depth = o.shape[0], 16, 64, 3
    assert n == 256 and n * spp * batches == 262144
    g = np.ones((n, 3), dtype=F32)
    lights = ptamd.scene_lights(b)["tri"]
    assert lights.size > 0
    nee = np.zeros((batches, 2, len(b.triangles), 3))
    ref = np.zeros_like(nee)
    for i in range(batches):
        a, _ = b.trace_nee_grad(o, d, g, depth, samples=spp, seed=1 + i, mis=True, want=("color", "emit"))
        r, _ = b.trace_grad(o, d, g, depth, samples=spp, seed=1 + i, want=("color", "emit"))
        nee[i, 0], nee[i, 1] = a["color"], a["emit"]
        ref[i, 0], ref[i, 1] = r["color"], r["emit"]

    def mean_se(x):
        return x.mean(axis=0), x.std(axis=0, ddof=1) / np.sqrt(batches)

    e_nee, se_e_nee = mean_se(nee[:, 1, lights].sum(axis=1))
    e_ref, se_e_ref = mean_se(ref[:, 1, lights].sum(axis=1))
    print("d emit of the light:", e_nee, "+-", se_e_nee, "| trace_grad", e_ref, "+-", se_e_ref)
    assert (e_ref != 0).all()
    assert (np.abs(e_nee - e_ref) <= 4.5 * np.sqrt(se_e_nee ** 2 + se_e_ref ** 2)).all()
    assert (se_e_nee < se_e_ref).all()
    top = np.argsort(-np.abs(ref[:, 0].mean(axis=0)).max(axis=1), kind="stable")[:3]
    c_nee, se_c_nee = mean_se(nee[:, 0, top])
    c_ref, se_c_ref = mean_se(ref[:, 0, top])
    print("d color of", top, ":", c_nee, "+-", se_c_nee, "| trace_grad", c_ref, "+-", se_c_ref)
    assert (c_ref != 0).all()
    assert (np.abs(c_nee - c_ref) <= 4.5 * np.sqrt(se_c_nee ** 2 + se_c_ref ** 2)).all()


@MIS
@pytest.mark.parametrize("name,variant", RN.TREES)
def test_caller_built_trees(name, variant, mis):
    """Gradients are indexed by the caller's triangle, whatever leaves hold it: the light that sits
    in two leaves gets one sum."""
    import ptamd
    o, d, t, S = NG.tree_expected(name, variant, mis)
    c = TC.case(name, variant)
    color, emit = RG.overrides(c.verts.shape[0])
    got, stats = TC.to_bvh(ptamd, c).trace_nee_grad(o, d, RG.grad_rgb(256), 5, color=color, emit=emit, mis=mis)
    RG.assert_within(got["color"], got["emit"], S, f"{name} {variant}")
    RT.assert_same(got["rgb"], t.rgb, f"{name} {variant} rgb")
    assert stats["terms"] == S.terms and stats["shadow_rays"] == t.shadow
    assert (S.exact[RG.COLOR] != 0).any(axis=1).sum() >= 8
    if variant in ("duplicated", "dropped"):
        assert (S.count[RG.EMIT_K][c.tri] > 0) == (variant == "duplicated")


def test_argument_handling():
    import ptamd
    from ptamd import _lib
    L = ptamd.lib()
    b = _bvh("cornell+glow")
    ref = ptamd._SceneRef(b)
    T = len(b.triangles)
    o, d = RT.rays("cornell", 4)
    g = RG.grad_rgb(4)
    rgb = np.full((4, 3), -1.0, dtype=np.float32)
    gc, ge = np.full((T, 3), -1.0), np.full((T, 3), -1.0)
    st = _lib.pt_nee_grad_stats()
    ok = _lib.pt_trace_params(5, 1, 1, None)

    def io(grad_rgb=g.ctypes.data, out=rgb.ctypes.data, color=gc.ctypes.data, emit=ge.ctypes.data):
        return _lib.pt_trace_grad_io(None, None, grad_rgb, out, color, emit)

    def host(scene=ref.s, org=o.ctypes.data, dirs=d.ctypes.data, n=4, prm=ok, x=None, opt=None):
        x = io() if x is None else x
        return L.pt_bvh_trace_nee_grad(C.byref(scene) if scene is not None else None, org, dirs, n,
                                       C.byref(prm) if prm is not None else None, C.byref(x) if x is not False else None,
                                       C.byref(st), C.byref(opt) if opt is not None else None)

    def arg_error(rc):
        assert rc == _lib.PT_E_ARG
        assert L.pt_last_error()

    assert host() == 0 and st.terms > 0 and (ge != 0).any() and st.nee.lights > 0
    assert host(opt=_lib.pt_nee_options(_lib.PT_NEE_MIS_BALANCE, (0, 0, 0))) == 0
    assert host(opt=_lib.pt_nee_options(_lib.PT_NEE_MIS_NONE, (0, 0, 0))) == 0
    arg_error(host(opt=_lib.pt_nee_options(2, (0, 0, 0))))       # an unknown mis mode
    arg_error(host(opt=_lib.pt_nee_options(-1, (0, 0, 0))))
    for r in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        arg_error(host(opt=_lib.pt_nee_options(_lib.PT_NEE_MIS_BALANCE, r)))  # a reserved word that is not 0
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
    assert not gc.any() and not ge.any() and not RW.bits(rgb).any() and st.terms == 0 and st.nee.trace.rays == 0
    # a NULL context, and bad options before it (no device needed for these returns)
    x = io()
    arg_error(L.pt_ctx_trace_nee_grad(None, o.ctypes.data, d.ctypes.data, 4, C.byref(ok), C.byref(x), 0, C.byref(st), None))
    bad = _lib.pt_nee_options(7, (0, 0, 0))
    arg_error(L.pt_ctx_trace_nee_grad(None, o.ctypes.data, d.ctypes.data, 4, C.byref(ok), C.byref(x), 0, C.byref(st),
                                      C.byref(bad)))
    with pytest.raises(ValueError):
        b.trace_nee_grad(o, d, None, 5)                 # the wrapper refuses it before the library does
    with pytest.raises(ValueError):
        b.trace_nee_grad(o, d, g, 5, color=np.zeros((T + 1, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        b.trace_nee_grad(o, d, g, 5, want=("rgb", "albedo"))


def test_symbols_and_struct_sizes():
    import ptamd
    L = ptamd.lib()
    assert L.pt_abi_version() == 3
    for name in ("pt_bvh_trace_nee_grad", "pt_ctx_trace_nee_grad"):
        assert hasattr(L, name), name
        assert name in ptamd._lib.EXPORTED
    assert C.sizeof(ptamd._lib.pt_nee_stats) == 88
    assert C.sizeof(ptamd._lib.pt_nee_grad_stats) == 88 + 24
    assert C.sizeof(ptamd._lib.pt_trace_grad_io) == 48 and C.sizeof(ptamd._lib.pt_nee_options) == 16
    assert hasattr(ptamd.BVH, "trace_nee_grad") and hasattr(ptamd.Renderer, "trace_nee_grad")
