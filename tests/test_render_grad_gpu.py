"""Material gradients of the rendered image along its own camera rays on the GPU
(pt_grad_cam_kernel / pt_nee_grad_cam_kernel through pt_ctx_render_grad and pt_ctx_render_nee_grad)
against the host form and tests/_refrendergrad.py: the forward image bit for bit (also against
Renderer.render / render_nee), terms and rays equal, the gradients within the summed any-order
tolerance. Each case runs a frame of at most 561 pixels."""
import numpy as np
import pytest

import _edgescenes as ES
import _refgrad as RG
import _refrendergrad as RR
import _reftrace as RT
import _refwalk as RW

pytestmark = pytest.mark.gpu

F32 = np.float32
CAMERAS = [(1, 1), (7, 9), (8, 8), (5, 13), (33, 17)]  # 1, 63, 64, 65 and 561 pixels (an odd width)


@pytest.fixture(scope="module")
def renderers():
    """One context per (scene name, resolution), scene uploaded; closed at the end."""
    import ptamd
    made = {}

    def get(name, res=(8, 8)):
        key = (name, tuple(res))
        if key not in made:
            sc, bvh, cam = RR.objects(name, res)
            r = ptamd.Renderer(0)
            r.set_scene(bvh)
            made[key] = (r, sc, bvh, cam)
        return made[key]

    yield get
    for r, _, _, _ in made.values():
        r.close()


def _check(r, bvh, cam, name, res, spp, depth, mode, seed=7, what="", **kw):
    """Device against the host form and the restatement. Returns (device result, stats)."""
    W, H = res
    E = RR.expected(name, tuple(res), spp, depth, seed, mode)
    G = RR.grad_img(res)
    what = what or f"{name} {res} spp {spp} depth {depth} {mode}"
    host, st_h = bvh.render_grad(cam, G, spp, depth, seed=seed, **RR.mode_kw(mode))
    got, st = r.render_grad(cam, G, spp, depth, seed=seed, **RR.mode_kw(mode), **kw)
    assert got["rgb"].shape == (H, W, 3)
    RT.assert_same(got["rgb"].reshape(-1, 3), host["rgb"].reshape(-1, 3), what + ": rgb vs host")
    RT.assert_same(got["rgb"].reshape(-1, 3), E.rgb.reshape(-1, 3), what + ": rgb vs restatement")
    RG.assert_within(got["color"], got["emit"], E.S, what)
    RR.check_stats(st, E, W * H, spp, mode, what)
    assert st["terms"] == st_h["terms"] and st["rays"] == st_h["rays"]
    return got, st


@pytest.mark.parametrize("mode", RR.MODES)
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("res", CAMERAS)
@pytest.mark.parametrize("name", RR.SCENES)
def test_device_against_host(renderers, name, res, spp, mode):
    r, _, bvh, cam = renderers(name, res)
    got, st = _check(r, bvh, cam, name, res, spp, 5, mode)
    assert st["launches"] == 1
    if res != (1, 1):
        assert np.any(got["emit"] != 0) and np.any(got["color"] != 0)


@pytest.mark.parametrize("mode", RR.MODES)
def test_single_path_is_bit_exact(renderers, mode):
    """A 1 x 1 camera with spp 1: the device adds in k order too."""
    r, _, bvh, cam = renderers("cornell+glow", (1, 1))
    E = RR.expected("cornell+glow", (1, 1), 1, 8, 1, mode)
    got, st = r.render_grad(cam, RR.grad_img((1, 1)), 1, 8, **RR.mode_kw(mode))
    assert st["terms"] == E.S.terms > 1
    assert np.array_equal(got["color"], E.S.ordered[RG.COLOR]) and np.array_equal(got["emit"], E.S.ordered[RG.EMIT_K])


def _render(r, cam, spp, depth, seed, mode):
    if mode == "plain":
        return r.render(cam, spp, depth, seed=seed)[0]
    return r.render_nee(cam, spp, depth, seed=seed, mis=mode == "nee+mis")[0]


@pytest.mark.parametrize("mode", RR.MODES)
@pytest.mark.parametrize("name", RR.SCENES)
def test_forward_is_the_render(renderers, name, mode):
    r, _, _, cam = renderers(name, (33, 17))
    img = _render(r, cam, 3, 5, 9, mode)
    got, st = r.render_grad(cam, None, 3, 5, seed=9, want=("rgb",), **RR.mode_kw(mode))
    assert RW.bits(img).any() and st["terms"] == 0
    assert np.array_equal(RW.bits(got["rgb"]), RW.bits(img)), f"{name} {mode}"


@pytest.mark.parametrize("mode", RR.MODES)
def test_forward_is_the_render_with_a_far_camera(mode):
    """cornell seen from z = -2^61: the camera rays leave the fast number domain of the slab test."""
    import ptamd
    sc = ES.make("cornell/far_camera/61", (16, 12))
    bvh = ptamd.BVH.from_scene(sc)
    bvh.build()
    cam = ptamd.Camera.from_spec(sc.camera)
    r = ptamd.Renderer(0)
    try:
        r.set_scene(bvh)
        img = _render(r, cam, 2, 5, 1, mode)
        G = RR.grad_img((16, 12))
        got, st = r.render_grad(cam, G, 2, 5, **RR.mode_kw(mode))
        host, st_h = bvh.render_grad(cam, G, 2, 5, **RR.mode_kw(mode))
    finally:
        r.close()
    assert np.array_equal(RW.bits(got["rgb"]), RW.bits(img)), mode
    RT.assert_same(got["rgb"].reshape(-1, 3), host["rgb"].reshape(-1, 3), mode)
    assert st["terms"] == st_h["terms"] and st["rays"] == st_h["rays"]


def _loop(r, cam, W, H, G, spp, depth, seed, mode):
    """What the call replaces: per sample the AOV rays, the stepped states and trace_grad(samples=1)
    with grad_rgb = fl(G / spp), the float64 tables added (test_nee_gpu._camera_samples' loop)."""
    seeds = RT.sample_seeds(W * H, spp, seed)
    gs = RR.scaled(G, spp)
    color = emit = 0.0
    acc = np.zeros((W * H, 3), dtype=F32)
    for s in range(spp):
        a, _ = r.aov(cam, sample=s, seed=seed, channels=("ray",))
        o = np.ascontiguousarray(a["ray"][..., 0:3].reshape(-1, 3))
        d = np.ascontiguousarray(a["ray"][..., 3:6].reshape(-1, 3))
        st = RT.lcg_step(seeds[:, s], 2)
        if mode == "plain":
            res, _ = r.trace_grad(o, d, gs, depth, states=st)
        else:
            res, _ = r.trace_nee_grad(o, d, gs, depth, states=st, mis=mode == "nee+mis")
        color, emit = color + res["color"], emit + res["emit"]
        with np.errstate(all="ignore"):
            acc = acc + res["rgb"]
    with np.errstate(all="ignore"):
        return (acc / F32(spp)).astype(F32), color, emit


@pytest.mark.parametrize("mode", RR.MODES)
@pytest.mark.parametrize("name", RR.SCENES)
def test_device_against_the_loop(renderers, name, mode):
    res = (33, 17)
    W, H = res
    r, _, _, cam = renderers(name, res)
    G = RR.grad_img(res)
    E = RR.expected(name, res, 3, 5, 7, mode)
    got, _ = r.render_grad(cam, G, 3, 5, seed=7, **RR.mode_kw(mode))
    rgb, color, emit = _loop(r, cam, W, H, G, 3, 5, 7, mode)
    RT.assert_same(got["rgb"].reshape(-1, 3), rgb, f"{name} {mode}: the loop's rgb")
    RG.assert_within(color, emit, E.S, f"{name} {mode}: the loop")
    RG.assert_within(got["color"], got["emit"], E.S, f"{name} {mode}: the call")


@pytest.mark.parametrize("mode", RR.MODES)
def test_samples_cut_over_launches(renderers, monkeypatch, mode):
    name, res = "random_7_300", (33, 17)
    r, _, bvh, cam = renderers(name, res)
    one, st1 = _check(r, bvh, cam, name, res, 5, 5, mode)
    monkeypatch.setenv("PT_RENDER_GRAD_CHUNK", "2")
    cut, st = _check(r, bvh, cam, name, res, 5, 5, mode, what="three launches")
    only, st_g = r.render_grad(cam, RR.grad_img(res), 5, 5, seed=7, want=("color", "emit"), **RR.mode_kw(mode))
    monkeypatch.delenv("PT_RENDER_GRAD_CHUNK")
    assert st1["launches"] == 1 and st["launches"] == 3 and st_g["launches"] == 3
    assert np.array_equal(RW.bits(cut["rgb"]), RW.bits(one["rgb"]))
    assert "rgb" not in only and st_g["terms"] == st["terms"]
    RG.assert_within(only["color"], only["emit"], RR.expected(name, res, 5, 5, 7, mode).S, "gradient only, three launches")


FORMS = [(None, None, "lds_table", 1), ("PT_GRAD_LDS", "0", "lds_table", 0), ("PT_TRACE_LDS_REC", "0", "lds_records", 0),
         ("PT_QUERY_LDS_STACK", "0", "lds_stack", 0)]


@pytest.mark.parametrize("hook,value,flag,want", FORMS)
@pytest.mark.parametrize("mode", ["plain", "nee+mis"])
@pytest.mark.parametrize("name", RR.SCENES)
def test_kernel_forms(renderers, monkeypatch, name, mode, hook, value, flag, want):
    """The LDS and global forms of the table, the records and the stack: all within the tolerance,
    and the stats name the form that ran."""
    res = (5, 13)
    r, _, bvh, cam = renderers(name, res)
    if hook:
        monkeypatch.setenv(hook, value)
    _, st = _check(r, bvh, cam, name, res, 3, 5, mode, what=f"{name} {mode} {hook}={value}")
    if hook:
        monkeypatch.delenv(hook)
    if hook or name == "cornell+glow":  # 300 triangles beside the records may not leave room for the table
        assert st[flag] == want
    if flag != "lds_table" and name == "cornell+glow":
        assert st["lds_table"] == 1


@pytest.mark.parametrize("mode", RR.MODES)
def test_deep_paths(mode):
    """Depth 64 on random_3_40 with an 8 x 8 camera: global records, the re-unwinding form."""
    import ptamd
    name, res = "random_3_40", (8, 8)
    sc, bvh, cam = RR.objects(name, res)
    r = ptamd.Renderer(0)
    try:
        r.set_scene(bvh)
        G = RR.grad_img(res)
        got, st = r.render_grad(cam, G, 2, 64, seed=3, **RR.mode_kw(mode))
        host, st_h = bvh.render_grad(cam, G, 2, 64, seed=3, **RR.mode_kw(mode))
    finally:
        r.close()
    E = RR.expected(name, res, 2, 64, 3, mode)
    RT.assert_same(got["rgb"].reshape(-1, 3), host["rgb"].reshape(-1, 3), f"deep {mode}")
    RT.assert_same(got["rgb"].reshape(-1, 3), E.rgb.reshape(-1, 3), f"deep {mode} vs restatement")
    RG.assert_within(got["color"], got["emit"], E.S, f"deep {mode}")
    RR.check_stats(st, E, 64, 2, mode, f"deep {mode}")
    assert st["lds_records"] == 0 and E.S.count.max() > 8


@pytest.mark.parametrize("mode", RR.MODES)
def test_parts(renderers, mode):
    name, res = "cornell+glow", (33, 17)
    W, H = res
    r, _, _, cam = renderers(name, res)
    G = RR.grad_img(res)
    E = RR.expected(name, res, 3, 5, 7, mode)
    whole, st_w = r.render_grad(cam, G, 3, 5, seed=7, **RR.mode_kw(mode))
    img = np.zeros((H, W, 3), dtype=F32)
    color, emit, terms, rays = 0.0, 0.0, 0, 0
    for p in range(3):
        hs = [h for h in range(H) if (h // 2) % 3 == p]
        part, st = r.render_grad(cam, np.ascontiguousarray(G[hs]), 3, 5, seed=7, part_index=p, part_count=3, band_rows=2,
                                 **RR.mode_kw(mode))
        assert part["rgb"].shape == (len(hs), W, 3)
        img[hs] = part["rgb"]
        color, emit = color + part["color"], emit + part["emit"]
        terms, rays = terms + st["terms"], rays + st["rays"]
    assert np.array_equal(RW.bits(img), RW.bits(whole["rgb"]))
    assert terms == st_w["terms"] == E.S.terms and rays == st_w["rays"]
    RG.assert_within(color, emit, E.S, f"parts {mode}")
    RG.assert_within(whole["color"], whole["emit"], E.S, f"whole {mode}")


@pytest.mark.parametrize("mode", ["plain", "nee+mis"])
def test_device_tensors(renderers, mode):
    import torch
    name, res = "cornell+glow", (33, 17)
    W, H = res
    r, sc, bvh, cam = renderers(name, res)
    T = len(sc.mats)
    G = RR.grad_img(res)
    color, emit = RG.overrides(T)
    E = RR.expected(name, res, 3, 5, 7, mode, override=True)
    host, st_h = r.render_grad(cam, G, 3, 5, seed=7, color=color, emit=emit, **RR.mode_kw(mode))
    RG.assert_within(host["color"], host["emit"], E.S, "host pointers, override")
    RT.assert_same(host["rgb"].reshape(-1, 3), E.rgb.reshape(-1, 3), "host pointers, override")
    dev = torch.device("cuda", 0)
    ins = [torch.from_numpy(a.copy()).to(dev) for a in (G, color, emit)]
    res_d, st = r.render_grad(cam, ins[0], 3, 5, seed=7, color=ins[1], emit=ins[2], **RR.mode_kw(mode))
    assert res_d["color"].dtype == torch.float64 and res_d["emit"].dtype == torch.float64 and res_d["rgb"].dtype == torch.float32
    assert all(v.is_cuda for v in res_d.values()) and tuple(res_d["color"].shape) == (T, 3)
    assert tuple(res_d["rgb"].shape) == (H, W, 3)
    RG.assert_within(res_d["color"].cpu().numpy(), res_d["emit"].cpu().numpy(), E.S, "device tensors")
    RT.assert_same(res_d["rgb"].cpu().numpy().reshape(-1, 3), host["rgb"].reshape(-1, 3), "device tensors rgb")
    assert st["terms"] == st_h["terms"] == E.S.terms and st["launches"] == 1
    for t, a in zip(ins, (G, color, emit)):
        assert np.array_equal(RW.bits(t.cpu().numpy()), RW.bits(a))  # inputs untouched


@pytest.mark.parametrize("light_sampling,mis", [(False, False), (True, True)])
def test_autograd(renderers, light_sampling, mis):
    import torch
    from ptamd.autograd import render_radiance
    name, res = "cornell+glow", (33, 17)
    r, sc, _, cam = renderers(name, res)
    kw = dict(light_sampling=light_sampling, mis=mis)
    dev = torch.device("cuda", 0)
    _, _, _, _, mvals = RT.scene_arrays(name)
    color0, emit0 = mvals[:, 0:3].copy(), mvals[:, 3:6].copy()
    target = torch.from_numpy(r.render_grad(cam, None, 3, 5, want=("rgb",), **kw)[0]["rgb"]).to(dev)
    start = (emit0 * F32(1.5) + F32(0.05)).astype(F32)  # the perturbed start
    color = torch.from_numpy(color0).to(dev).requires_grad_(True)
    emit = torch.from_numpy(start).to(dev).requires_grad_(True)
    img = render_radiance(r, cam, color, emit, 5, 3, 1, **kw)
    assert tuple(img.shape) == (17, 33, 3)
    loss = ((img - target) ** 2).sum()
    loss.backward()
    want, _ = r.render_grad(cam, (2 * (img - target)).detach().contiguous(), 3, 5, color=color.detach(), emit=emit.detach(),
                            want=("color", "emit"), **kw)
    # two runs add the same float32 terms in double in different orders: the sums agree to ~1e-14
    # relative, so their float32 casts are equal unless a sum sits within that of a float32
    # rounding boundary (test_grad_gpu.test_autograd's rule)
    for grad, w in ((color.grad, want["color"]), (emit.grad, want["emit"])):
        assert grad.dtype == torch.float32 and (grad != 0).any()
        assert torch.equal(grad, w.to(torch.float32))
    assert float(loss.detach()) > 0
    with torch.no_grad():  # one SGD step on emit lowers the loss (the paths are fixed by the seed)
        step = emit - 1e-4 * emit.grad
    after = ((render_radiance(r, cam, color.detach(), step, 5, 3, 1, **kw) - target) ** 2).sum()
    assert float(after) < float(loss.detach())
    with pytest.raises(ValueError):
        render_radiance(r, cam, color, emit, 5, 3, 1, light_sampling=False, mis=True)


def test_side_effects(renderers):
    """A progressive sum survives a render_grad call, and the override does not leak into the scene
    or its light table (test_grad_gpu.test_side_effects' pattern)."""
    name, res = "cornell+glow", (8, 8)
    r, sc, _, cam = renderers(name, res)
    o, d = RT.rays(name, 65)
    color, emit = RG.overrides(len(sc.mats))
    before, _ = r.render(cam, 4, 4)
    nee_before, _ = r.trace_nee(o, d, 4)
    r.render_progressive(cam, 0, 2, 4)
    for mode in RR.MODES:
        r.render_grad(cam, RR.grad_img(res), 3, 4, color=color, emit=emit, **RR.mode_kw(mode))
    img, _ = r.render_progressive(cam, 2, 2, 4)
    assert np.array_equal(RW.bits(img), RW.bits(before))
    after, _ = r.render(cam, 4, 4)
    assert np.array_equal(RW.bits(after), RW.bits(before))
    RT.assert_same(r.trace_nee(o, d, 4)[0], nee_before, "trace_nee after an override")
    plain, _ = r.render_grad(cam, None, 4, 4, want=("rgb",))
    assert np.array_equal(RW.bits(plain["rgb"]), RW.bits(before))
