"""Material gradients of the light-sampling estimator on the GPU (pt_nee_grad.hip through
pt_ctx_trace_nee_grad) against the host form (pt_bvh_trace_nee_grad: forward bits and counts equal)
and against tests/_refneegrad.py within the derived any-order summation tolerance, and through torch
(device tensors, ptamd.autograd.trace_radiance with light_sampling). The shapes are the smallest at
which the kernel can still go wrong: 257 rays (two blocks, the second with one live lane), 1 and 3
samples, depth 1, 2, 5, 8 and 64."""
import numpy as np
import pytest

import _refgrad as RG
import _refnee as RN
import _refneegrad as NG
import _reftrace as RT
import _refwalk as RW
import _treecases as TC

pytestmark = pytest.mark.gpu

F32 = np.float32
N = NG.N
MIS = pytest.mark.parametrize("mis", [False, True], ids=["plain", "mis"])
COUNTS = ("terms", "rays", "paths", "shadow_rays", "light_draws", "lights", "runaway")


@pytest.fixture(scope="module")
def renderers():
    """One context per scene name, scene uploaded; closed at the end."""
    import ptamd
    made = {}

    def get(name):
        if name not in made:
            sc = NG.make_scene(name)
            bvh = ptamd.BVH.from_scene(sc)
            bvh.build()
            r = ptamd.Renderer(0)
            r.set_scene(bvh)
            made[name] = (r, sc, bvh)
        return made[name]

    yield get
    for r, _, _ in made.values():
        r.close()


def _check(r, bvh, name, depth, spp, mis, n=N, what="", walk_depth=0, **kw):
    """Device against the host form (rgb bits, every count) and the restatement's exact sums."""
    o, d = NG.rays(name, n)
    g = RG.grad_rgb(n)
    t, S = NG.expected(name, n, depth, spp, mis, walk_depth=walk_depth)
    got, st = r.trace_nee_grad(o, d, g, depth, samples=spp, mis=mis, **kw)
    host, st_h = bvh.trace_nee_grad(o, d, g, depth, samples=spp, mis=mis)
    what = what or f"{name} depth {depth} spp {spp} mis {mis}"
    print(what, "max |err| / tol", float(np.nanmax(np.abs(np.stack([got["color"], got["emit"]]) - S.exact) / np.maximum(S.tol, 1e-300))))
    RT.assert_same(got["rgb"], host["rgb"], what + " rgb vs the host form")
    RG.assert_within(got["color"], got["emit"], S, what)
    RG.assert_within(host["color"], host["emit"], S, what + " (host form)")
    assert {k: st[k] for k in COUNTS} == {k: st_h[k] for k in COUNTS}, (what, st, st_h)
    assert st["terms"] == S.terms and st["rays"] == t.segments and st["shadow_rays"] == t.shadow
    return got, st, t, S


@MIS
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("name", NG.SCENES)
def test_device_against_host_form(renderers, name, spp, mis):
    """Depth 1 (no record level), 2, 5 and 8, on two blocks with one live lane in the second."""
    r, _, bvh = renderers(name)
    lit = 0
    for depth in NG.DEPTHS:
        _, st, t, S = _check(r, bvh, name, depth, spp, mis)
        assert st["launches"] == 1
        if name != "random_7_300":  # small scenes: everything fits the block's LDS at these depths
            assert st["lds_table"] == 1 and st["lds_records"] == 1
        lit += int((t.case == NG.T_LIGHT).sum())
    assert lit > 0 and (S.exact[RG.COLOR] != 0).any() and (S.exact[RG.EMIT_K] != 0).any()
    if mis and name == "tri3":
        assert (t.case == NG.T_END_WEIGHTED).sum() > 0


@MIS
def test_scene_without_lights(renderers, mis):
    """No light table: no draw, no shadow segment, and the terms are trace_grad's."""
    r, _, bvh = renderers("no_lights")
    _, st, t, S = _check(r, bvh, "no_lights", 5, 3, mis)
    assert st["lights"] == 0 and st["light_draws"] == 0 and st["shadow_rays"] == 0 and (t.case == NG.T_LIGHT).sum() == 0
    assert (S.exact[RG.COLOR] != 0).any() and (S.exact[RG.EMIT_K] != 0).any()
    o, d = NG.rays("no_lights", N)
    _, st_g = r.trace_grad(o, d, RG.grad_rgb(N), 5, samples=3)
    assert st_g["terms"] == st["terms"] and st_g["rays"] == st["rays"]


@MIS
def test_depth_64_with_global_records(renderers, mis):
    name, n = "random_3_40", 64
    r, _, bvh = renderers(name)
    _, st, t, S = _check(r, bvh, name, 64, 1, mis, n=n, walk_depth=64)
    assert st["lds_records"] == 0 and S.count.max() > 8 and (t.case == NG.T_LIGHT).sum() > 0


FORMS = [(None, None, "lds_table", 1), ("PT_GRAD_LDS", "0", "lds_table", 0), ("PT_TRACE_LDS_REC", "0", "lds_records", 0),
         ("PT_QUERY_LDS_STACK", "0", "lds_stack", 0)]


@pytest.mark.parametrize("hook,value,flag,want", FORMS)
@pytest.mark.parametrize("name", ["cornell+glow", "random_7_300"])
def test_table_forms(renderers, monkeypatch, name, hook, value, flag, want):
    """The per-block LDS table and the global form, and the table beside global records / a global
    stack: all within the tolerance, and the stats say which ran."""
    r, _, bvh = renderers(name)
    if hook:
        monkeypatch.setenv(hook, value)
    _, st, _, _ = _check(r, bvh, name, 5, 3, True, what=f"{name} {hook}={value}")
    if hook:
        monkeypatch.delenv(hook)
    if hook or name == "cornell+glow":  # 300 triangles beside four-word records may not leave room for the table
        assert st[flag] == want
    if flag != "lds_table" and name == "cornell+glow":
        assert st["lds_table"] == 1


@MIS
def test_launches_cut_over_rays(renderers, monkeypatch, mis):
    r, _, bvh = renderers("random_7_300")
    monkeypatch.setenv("PT_TRACE_CHUNK", "64")
    _, st, _, _ = _check(r, bvh, "random_7_300", 5, 3, mis, what="five launches")
    monkeypatch.delenv("PT_TRACE_CHUNK")
    assert st["launches"] == 5


@MIS
def test_single_paths_are_bit_exact(renderers, mis):
    """n = 1, spp = 1: the device adds in k order too, bit for bit the host form's sums."""
    name, depth = "random_7_300", 8
    r, _, bvh = renderers(name)
    o, d = NG.rays(name, 16)
    seeds = RT.sample_seeds(16, 1, 1)[:, 0]
    g = RG.grad_rgb(16)
    terms = 0
    for i in range(16):
        got, st = r.trace_nee_grad(o[i:i + 1], d[i:i + 1], g[i:i + 1], depth, states=seeds[i:i + 1], mis=mis)
        host, st_h = bvh.trace_nee_grad(o[i:i + 1], d[i:i + 1], g[i:i + 1], depth, states=seeds[i:i + 1], mis=mis)
        assert np.array_equal(got["color"].view(np.uint64), host["color"].view(np.uint64)), i
        assert np.array_equal(got["emit"].view(np.uint64), host["emit"].view(np.uint64)), i
        RT.assert_same(got["rgb"], host["rgb"], f"ray {i}")
        assert st["terms"] == st_h["terms"] and st["shadow_rays"] == st_h["shadow_rays"]
        terms += st["terms"]
    assert terms > 32


@MIS
def test_device_tensors(renderers, mis):
    import torch
    name = "cornell+glow"
    r, sc, bvh = renderers(name)
    o, d = NG.rays(name, N)
    g = RG.grad_rgb(N)
    color, emit = RG.overrides(len(sc.mats))
    host, st_h = bvh.trace_nee_grad(o, d, g, 5, color=color, emit=emit, mis=mis)
    t, S = NG.expected(name, N, 5, 1, mis, override=True)
    RG.assert_within(host["color"], host["emit"], S, "host form, override")
    dev = torch.device("cuda", 0)
    ins = [torch.from_numpy(a.copy()).to(dev) for a in (o, d, g, color, emit)]
    res, st = r.trace_nee_grad(ins[0], ins[1], ins[2], 5, color=ins[3], emit=ins[4], mis=mis)
    assert res["color"].dtype == torch.float64 and res["emit"].dtype == torch.float64 and res["rgb"].dtype == torch.float32
    assert all(v.is_cuda for v in res.values()) and tuple(res["color"].shape) == (len(sc.mats), 3)
    RG.assert_within(res["color"].cpu().numpy(), res["emit"].cpu().numpy(), S, "device tensors")
    RT.assert_same(res["rgb"].cpu().numpy(), host["rgb"], "device tensors rgb")
    RT.assert_same(host["rgb"], t.rgb, "override rgb vs the restatement")
    assert st["terms"] == st_h["terms"] == S.terms and st["launches"] == 1
    for x, a in zip(ins, (o, d, g, color, emit)):
        assert np.array_equal(RW.bits(x.cpu().numpy()), RW.bits(a))  # inputs untouched
    # host pointers with the same override, and the override does not stay behind
    np_res, _ = r.trace_nee_grad(o, d, g, 5, color=color, emit=emit, mis=mis)
    RG.assert_within(np_res["color"], np_res["emit"], S, "host pointers, override")
    RT.assert_same(np_res["rgb"], host["rgb"], "host pointers rgb")
    RT.assert_same(r.trace_nee_grad(o, d, None, 5, want=("rgb",), mis=mis)[0]["rgb"], r.trace_nee(o, d, 5, mis=mis)[0],
                   "no override after an override")


@MIS
@pytest.mark.parametrize("name,variant", RN.TREES)
def test_caller_built_trees(name, variant, mis):
    import ptamd
    o, d, t, S = NG.tree_expected(name, variant, mis)
    c = TC.case(name, variant)
    color, emit = RG.overrides(c.verts.shape[0])
    r = ptamd.Renderer(0)
    try:
        r.set_scene(TC.to_bvh(ptamd, c))
        got, st = r.trace_nee_grad(o, d, RG.grad_rgb(256), 5, color=color, emit=emit, mis=mis)
    finally:
        r.close()
    RG.assert_within(got["color"], got["emit"], S, f"{name} {variant}")
    RT.assert_same(got["rgb"], t.rgb, f"{name} {variant} rgb")
    assert st["terms"] == S.terms and st["launches"] == 1 and st["shadow_rays"] == t.shadow
    if variant in ("duplicated", "dropped"):
        assert (S.count[RG.EMIT_K][c.tri] > 0) == (variant == "duplicated")  # two leaves, one sum


def test_autograd(renderers):
    import torch
    from ptamd.autograd import trace_radiance
    name, n, spp, depth = "cornell+glow", 64, 16, 5
    r, sc, _ = renderers(name)
    dev = torch.device("cuda", 0)
    o, d = (torch.from_numpy(a.copy()).to(dev) for a in NG.rays(name, n))
    _, _, _, _, mvals = NG.scene_arrays(name)
    color0, emit0 = mvals[:, 0:3].copy(), mvals[:, 3:6].copy()
    # the default call is today's function: trace()'s bits
    plain = trace_radiance(r, o, d, torch.from_numpy(color0).to(dev), torch.from_numpy(emit0).to(dev), depth, spp, 1)
    RT.assert_same(plain.cpu().numpy(), r.trace(o, d, depth, samples=spp)[0].cpu().numpy(), "the default call")
    # forward and backward of the light-sampling form
    target = r.trace_nee(o, d, depth, samples=spp, mis=True)[0].clone()
    color = torch.from_numpy(color0).to(dev).requires_grad_(True)
    emit = torch.from_numpy(emit0).to(dev).requires_grad_(True)
    rgb = trace_radiance(r, o, d, color, emit, depth, spp, 1, light_sampling=True, mis=True)
    RT.assert_same(rgb.detach().cpu().numpy(), target.cpu().numpy(), "forward vs Renderer.trace_nee")
    w = torch.from_numpy(RG.grad_rgb(n)).to(dev)
    (rgb * w).sum().backward()
    want, _ = r.trace_nee_grad(o, d, w, depth, samples=spp, color=color.detach(), emit=emit.detach(), want=("color", "emit"),
                               mis=True)
    _, S = NG.expected(name, n, depth, spp, True)
    for grad, k, kind in ((color.grad, "color", RG.COLOR), (emit.grad, "emit", RG.EMIT_K)):
        assert grad.dtype == torch.float32 and (grad != 0).any()
        # two runs add the same float32 terms in double in different orders: both lie within the
        # any-order bound of the exact sum, and the float32 cast adds half an ulp of the value
        a, b = grad.double().cpu().numpy(), want[k].cpu().numpy()
        assert (np.abs(a - b) <= 2 * S.tol[kind] + np.abs(b) * 2.0 ** -24).all(), k
    with pytest.raises(ValueError):
        trace_radiance(r, o, d, color, emit, depth, spp, 1, mis=True)  # the weights need light sampling
    # a 20-step Adam fit of one wall colour lowers the loss
    wall = int(np.argmax(S.count[RG.COLOR]))
    start = color0.copy()
    start[wall] = np.clip(start[wall] * F32(0.4) + F32(0.1), 0.05, 0.95)
    param = torch.from_numpy(start[wall].copy()).to(dev).requires_grad_(True)
    base = torch.from_numpy(start).to(dev)
    mask = torch.zeros_like(base)
    mask[wall] = 1.0
    emit_t = torch.from_numpy(emit0).to(dev)
    opt = torch.optim.Adam([param], lr=0.05)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        col = base * (1 - mask) + mask * param[None, :]
        out = trace_radiance(r, o, d, col.contiguous(), emit_t, depth, spp, 1, light_sampling=True, mis=True)
        loss = ((out - target) ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("Adam fit of triangle", wall, ":", losses[0], "->", losses[-1])
    assert losses[0] > 0 and losses[-1] < losses[0]


def test_side_effects(renderers):
    """A progressive sum survives the call, and Renderer.trace_nee and Renderer.trace_grad return
    their previous bits after it (the override does not leak, the record buffer is shared)."""
    import ptamd
    name = "random_3_40"
    r, sc, _ = renderers(name)
    cam = ptamd.Camera.from_spec(sc.camera)
    o, d = NG.rays(name, 65)
    g = RG.grad_rgb(65)
    color, emit = RG.overrides(len(sc.mats))
    nee0, _ = r.trace_nee(o, d, 4, samples=3, mis=True)
    grad0, _ = r.trace_grad(o, d, None, 8, want=("rgb",))
    before, _ = r.render(cam, 4, 4)
    r.render_progressive(cam, 0, 2, 4)
    r.trace_nee_grad(o, d, g, 8, samples=3, color=color, emit=emit, mis=True)
    img, _ = r.render_progressive(cam, 2, 2, 4)
    assert np.array_equal(RW.bits(img), RW.bits(before))
    nee1, _ = r.trace_nee(o, d, 4, samples=3, mis=True)
    grad1, _ = r.trace_grad(o, d, None, 8, want=("rgb",))
    RT.assert_same(nee1, nee0, "trace_nee after trace_nee_grad")
    RT.assert_same(grad1["rgb"], grad0["rgb"], "trace_grad after trace_nee_grad")
