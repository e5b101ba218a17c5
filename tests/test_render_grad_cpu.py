"""Material gradients of the rendered image along its own camera rays, host form
(pt_bvh_render_grad, pt_bvh_render_nee_grad) against tests/_refrendergrad.py: the camera ray bit
for bit, the forward image bit for bit, the gradients within the summed any-order tolerance."""
import ctypes as C

import numpy as np
import pytest

import _refgrad as RG
import _refrendergrad as RR
import _reftrace as RT
import _refwalk as RW
from conftest import load_golden

F32 = np.float32
RES = (8, 6)  # 48 pixels, W != H


def _host_rays(cam, res, s, seed):
    """The host form's camera ray of sample s of every pixel (pt_debug_host_camera_rays)."""
    import ptamd
    from ptamd import _lib
    n = res[0] * res[1]
    o, d, st = np.empty((n, 3), dtype=F32), np.empty((n, 3), dtype=F32), np.empty(n, dtype=np.uint32)
    prm = _lib.pt_params(1, 1, seed, 0, 1, 1, 0, 0)
    assert ptamd.lib().pt_debug_host_camera_rays(C.byref(cam.c), C.byref(prm), s, 0, n, o.ctypes.data, d.ctypes.data,
                                                 st.ctypes.data) == 0
    return o, d, st


@pytest.mark.parametrize("name", ["cornell", "random_7_300"])
def test_camera_ray_and_forward_bits(name):
    """The host camera ray is `_reftrace.camera_rays` for sample 0 and its generalised form for s in
    {1, 4}, bit for bit; the image of spp samples equals the in-order mean of BVH.trace /
    BVH.trace_nee on those rays and states."""
    sc, b, cam = RR.objects(name, RES)
    W, H = RES
    o0, d0, s0 = RT.camera_rays(sc, 3)
    for s in (0, 1, 4):
        o, d, st = RR.camera_rays(sc, 3, s)
        if s == 0:
            assert np.array_equal(RW.bits(o), RW.bits(o0)) and np.array_equal(RW.bits(d), RW.bits(d0)) and np.array_equal(st, s0)
        ho, hd, hs = _host_rays(cam, RES, s, 3)
        assert np.array_equal(RW.bits(ho), RW.bits(o)) and np.array_equal(RW.bits(hd), RW.bits(d)), (name, s)
        assert np.array_equal(hs, st), (name, s)
    spp, depth, seed = 5, 5, 3
    samples = [RR.camera_rays(sc, seed, k) for k in range(spp)]
    for mode in RR.MODES:
        kw = RR.mode_kw(mode)
        acc = np.zeros((W * H, 3), dtype=F32)
        rays = 0
        per_sample = []
        with np.errstate(all="ignore"):
            for os_, ds_, st in samples:
                if mode == "plain":
                    x, s1 = b.trace(os_, ds_, depth, states=st)
                else:
                    x, s1 = b.trace_nee(os_, ds_, depth, states=st, mis=kw.get("mis", False))
                per_sample.append(x)
                acc = acc + x
                rays += s1["rays"]
            want = (acc / F32(spp)).astype(F32)
        res, st = b.render_grad(cam, None, spp, depth, seed=seed, want=("rgb",), **kw)
        assert res["rgb"].shape == (H, W, 3) and RW.bits(res["rgb"]).any()
        RT.assert_same(res["rgb"].reshape(-1, 3), want, f"{name} {mode}: host render_grad rgb vs trace on the camera rays")
        assert st["rays"] == rays and st["paths"] == W * H * spp and st["terms"] == 0
        # single samples 1 and 4 on their own: the image of sample s alone cannot be asked for, but
        # spp = 2 holds sample 1 and spp = 5 sample 4 as their last addend
        res2, _ = b.render_grad(cam, None, 2, depth, seed=seed, want=("rgb",), **kw)
        with np.errstate(all="ignore"):
            want2 = ((per_sample[0] + per_sample[1]) / F32(2)).astype(F32)
        RT.assert_same(res2["rgb"].reshape(-1, 3), want2, f"{name} {mode}: samples 0 and 1")


def test_forward_equals_the_reference_image():
    """cornell at 16 x 16, 4 spp, depth 1, seed 1: the reference's own image (tests/golden; its seed
    convention is render's)."""
    sc, b, cam = RR.objects("cornell", (16, 16))
    res, _ = b.render_grad(cam, None, 4, 1, want=("rgb",))
    ref = load_golden("cornell_16_s4_d1")
    assert res["rgb"].shape == ref.shape
    assert np.array_equal(RW.bits(res["rgb"]), RW.bits(ref))


@pytest.mark.parametrize("mode", RR.MODES)
@pytest.mark.parametrize("depth", [1, 5, 8])
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("name", RR.SCENES)
def test_gradients(name, spp, depth, mode):
    _, b, cam = RR.objects(name, RES)
    W, H = RES
    E = RR.expected(name, RES, spp, depth, 7, mode)
    res, st = b.render_grad(cam, RR.grad_img(RES), spp, depth, seed=7, **RR.mode_kw(mode))
    what = f"{name} spp {spp} depth {depth} {mode}"
    RT.assert_same(res["rgb"].reshape(-1, 3), E.rgb.reshape(-1, 3), what)
    RG.assert_within(res["color"], res["emit"], E.S, what)
    RR.check_stats(st, E, W * H, spp, mode, what)
    assert np.any(res["emit"] != 0) and (depth == 1 or np.any(res["color"] != 0)), what
    # the host adds in (pixel, sample, k) order
    assert np.array_equal(res["color"], E.S.ordered[RG.COLOR]) and np.array_equal(res["emit"], E.S.ordered[RG.EMIT_K]), what


@pytest.mark.parametrize("mode", RR.MODES)
def test_single_path_adds_in_k_order(mode):
    _, b, cam = RR.objects("cornell+glow", (1, 1))
    E = RR.expected("cornell+glow", (1, 1), 1, 8, 1, mode)
    res, st = b.render_grad(cam, RR.grad_img((1, 1)), 1, 8, **RR.mode_kw(mode))
    assert E.S.terms > 1 and st["terms"] == E.S.terms
    assert np.array_equal(res["color"], E.S.ordered[RG.COLOR]) and np.array_equal(res["emit"], E.S.ordered[RG.EMIT_K])
    RT.assert_same(res["rgb"].reshape(-1, 3), E.rgb.reshape(-1, 3), mode)


@pytest.mark.parametrize("mode", RR.MODES)
@pytest.mark.parametrize("name", RR.SCENES)
def test_overrides(name, mode):
    _, b, cam = RR.objects(name, RES)
    T = len(b.triangles)
    color, emit = RG.overrides(T)
    E = RR.expected(name, RES, 3, 5, 1, mode, override=True)
    res, st = b.render_grad(cam, RR.grad_img(RES), 3, 5, color=color, emit=emit, **RR.mode_kw(mode))
    what = f"{name} {mode} overrides"
    RT.assert_same(res["rgb"].reshape(-1, 3), E.rgb.reshape(-1, 3), what)
    RG.assert_within(res["color"], res["emit"], E.S, what)
    RR.check_stats(st, E, RES[0] * RES[1], 3, mode, what)
    E0 = RR.expected(name, RES, 3, 5, 1, mode)
    assert not np.array_equal(RW.bits(E.rgb), RW.bits(E0.rgb))


@pytest.mark.parametrize("mis", [False, True])
def test_a_zeroed_light_keeps_the_scenes_table(mis):
    """An override that sets every light's emission to zero: the draws, the shadow segments and the
    light count are the scene's, and the lights still receive their d emit terms."""
    import ptamd
    _, b, cam = RR.objects("cornell+glow", RES)
    lights = ptamd.scene_lights(b)["tri"]
    emit = np.ascontiguousarray(RT.scene_arrays("cornell+glow")[4][:, 3:6], dtype=F32).copy()
    emit[lights] = 0.0
    kw = {"light_sampling": True, "mis": mis}
    base, st0 = b.render_grad(cam, RR.grad_img(RES), 3, 5, **kw)
    res, st = b.render_grad(cam, RR.grad_img(RES), 3, 5, emit=emit, **kw)
    for k in ("rays", "shadow_rays", "light_draws", "lights", "light_area", "terms"):
        assert st[k] == st0[k], k
    assert st["lights"] == len(lights) > 0 and st["shadow_rays"] > 0
    assert np.any(res["emit"][lights] != 0)
    assert not np.array_equal(RW.bits(res["rgb"]), RW.bits(base["rgb"]))


def test_symbols():
    import ptamd
    L = ptamd.lib()
    for s in ("pt_ctx_render_grad", "pt_ctx_render_nee_grad", "pt_bvh_render_grad", "pt_bvh_render_nee_grad"):
        assert hasattr(L, s), s
    with pytest.raises(ValueError):
        _, b, cam = RR.objects("cornell+glow", (1, 1))
        b.render_grad(cam, RR.grad_img((1, 1)), 1, 1, mis=True)


def test_argument_handling():
    import ptamd
    from ptamd import _lib
    L = ptamd.lib()
    _, b, cam = RR.objects("cornell+glow", RES)
    ref = ptamd._SceneRef(b)
    T = len(b.triangles)
    W, H = RES
    n = W * H
    g = RR.grad_img(RES)
    rgb = np.full((n, 3), -1.0, dtype=F32)
    gc, ge = np.full((T, 3), -1.0), np.full((T, 3), -1.0)
    st, nst = _lib.pt_grad_stats(), _lib.pt_nee_grad_stats()

    def prm(spp=2, depth=5, part_index=0, part_count=1, band_rows=1):
        return _lib.pt_params(spp, depth, 1, part_index, part_count, band_rows, 0, 0)

    def io(grad_rgb=g.ctypes.data, out=rgb.ctypes.data, color=gc.ctypes.data, emit=ge.ctypes.data):
        return _lib.pt_trace_grad_io(None, None, grad_rgb, out, color, emit)

    def plain(scene=ref.s, camera=cam.c, p=None, x=None):
        p = prm() if p is None else p
        x = io() if x is None else x
        return L.pt_bvh_render_grad(C.byref(scene) if scene is not None else None, C.byref(camera) if camera is not None else None,
                                    C.byref(p) if p is not False else None, C.byref(x) if x is not False else None, C.byref(st))

    def nee(scene=ref.s, camera=cam.c, p=None, x=None, opt=None):
        p = prm() if p is None else p
        x = io() if x is None else x
        return L.pt_bvh_render_nee_grad(C.byref(scene) if scene is not None else None,
                                        C.byref(camera) if camera is not None else None, C.byref(p) if p is not False else None,
                                        C.byref(x) if x is not False else None, C.byref(nst),
                                        C.byref(opt) if opt is not None else None)

    def arg_error(rc):
        assert rc == _lib.PT_E_ARG
        assert L.pt_last_error()

    assert plain() == 0 and st.terms > 0 and (ge != 0).any() and st.trace.paths == 2 * n
    assert nee() == 0 and nst.terms > 0 and nst.nee.lights > 0 and nst.nee.trace.paths == 2 * n
    assert nee(opt=_lib.pt_nee_options(_lib.PT_NEE_MIS_BALANCE, (0, 0, 0))) == 0
    arg_error(nee(opt=_lib.pt_nee_options(2, (0, 0, 0))))                          # an unknown mis mode
    for r in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        arg_error(nee(opt=_lib.pt_nee_options(_lib.PT_NEE_MIS_BALANCE, r)))        # a reserved word that is not 0
    for f in (plain, nee):
        arg_error(f(x=io(grad_rgb=None)))                                          # a gradient output without grad_rgb
        assert f(x=io(grad_rgb=None, color=None, emit=None)) == 0                  # forward only
        assert f(x=io(out=None)) == 0                                              # gradients only
        arg_error(f(x=False))
        arg_error(f(p=False))
        arg_error(f(scene=None))
        arg_error(f(camera=None))
        for spp, depth in ((0, 5), (-3, 5), (1, -1), (1, _lib.PT_MAX_DEPTH + 1)):
            arg_error(f(p=prm(spp=spp, depth=depth)))
        arg_error(f(p=prm(part_index=3, part_count=3)))
        # depth 0: every output +0
        gc[:], ge[:], rgb[:] = -1.0, -1.0, -1.0
        assert f(p=prm(depth=0)) == 0
        assert not gc.any() and not ge.any() and not RW.bits(rgb).any()
        # a part with no rows (H = 6 rows in bands of 4: parts 0 and 1 hold them all) zeroes the gradient outputs
        gc[:], ge[:] = -1.0, -1.0
        assert f(p=prm(part_index=2, part_count=3, band_rows=4), x=io(grad_rgb=None, out=None)) == 0
        assert not gc.any() and not ge.any()
    assert st.terms == 0 and st.trace.rays == 0 and nst.terms == 0
    # the device forms: a NULL context, and bad options before it (no device needed for these returns)
    x, p = io(), prm()
    arg_error(L.pt_ctx_render_grad(None, C.byref(cam.c), C.byref(p), C.byref(x), 0, C.byref(st)))
    arg_error(L.pt_ctx_render_nee_grad(None, C.byref(cam.c), C.byref(p), C.byref(x), 0, C.byref(nst), None))
    bad = _lib.pt_nee_options(7, (0, 0, 0))
    arg_error(L.pt_ctx_render_nee_grad(None, C.byref(cam.c), C.byref(p), C.byref(x), 0, C.byref(nst), C.byref(bad)))


def test_parts_sum_to_the_frame():
    _, b, cam = RR.objects("cornell+glow", RES)
    from ptamd import _lib
    import ptamd
    L = ptamd.lib()
    ref = ptamd._SceneRef(b)
    T = len(b.triangles)
    W, H = RES
    G = RR.grad_img(RES)
    E = RR.expected("cornell+glow", RES, 3, 5, 1, "nee+mis")
    tot_c, tot_e = np.zeros((T, 3)), np.zeros((T, 3))
    img = np.zeros((H, W, 3), dtype=F32)
    terms = 0
    for part in range(3):
        hs = [h for h in range(H) if (h // 2) % 3 == part]
        g = np.ascontiguousarray(G[hs])
        rgb = np.zeros((len(hs), W, 3), dtype=F32)
        gc, ge = np.zeros((T, 3)), np.zeros((T, 3))
        io = _lib.pt_trace_grad_io(None, None, g.ctypes.data, rgb.ctypes.data, gc.ctypes.data, ge.ctypes.data)
        p = _lib.pt_params(3, 5, 1, part, 3, 2, 0, 0)
        st = _lib.pt_nee_grad_stats()
        opt = _lib.pt_nee_options(_lib.PT_NEE_MIS_BALANCE, (0, 0, 0))
        assert L.pt_bvh_render_nee_grad(C.byref(ref.s), C.byref(cam.c), C.byref(p), C.byref(io), C.byref(st), C.byref(opt)) == 0
        img[hs] = rgb
        tot_c += gc
        tot_e += ge
        terms += st.terms
    RT.assert_same(img.reshape(-1, 3), E.rgb.reshape(-1, 3), "parts")
    assert terms == E.S.terms
    RG.assert_within(tot_c, tot_e, E.S, "parts")
