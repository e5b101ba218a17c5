"""Material gradients of trace() on the GPU (pt_grad.hip through pt_ctx_trace_grad) against
tests/_refgrad.py within the derived any-order summation tolerance, against the host path, and
through torch (device tensors, ptamd.autograd.trace_radiance). Forward values: bits equal."""
import numpy as np
import pytest

import _refgrad as RG
import _reftrace as RT
import _refwalk as RW
import _treecases as TC

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = (1, 63, 64, 65, 257, 512)


@pytest.fixture(scope="module")
def renderers():
    """One context per scene name, scene uploaded; closed at the end."""
    import ptamd
    made = {}

    def get(name):
        if name not in made:
            sc = RT.make_scene(name)
            bvh = ptamd.BVH.from_scene(sc)
            r = ptamd.Renderer(0)
            r.set_scene(bvh)
            made[name] = (r, sc, bvh)
        return made[name]

    yield get
    for r, _, _ in made.values():
        r.close()


def _check(r, name, n, depth, spp=1, what="", **kw):
    o, d = RT.rays(name, n)
    t, S = RG.expected(name, n, depth, spp)
    got, st = r.trace_grad(o, d, RG.grad_rgb(n), depth, samples=spp, **kw)
    what = what or f"{name} n {n} depth {depth} spp {spp}"
    print(what, "max |err| / tol", float(np.nanmax(np.abs(np.stack([got["color"], got["emit"]]) - S.exact) / np.maximum(S.tol, 1e-300))))
    RG.assert_within(got["color"], got["emit"], S, what)
    RT.assert_same(got["rgb"], RG.mean_rgb(t, spp), what + " rgb")
    segs = int(RT.radiance(RG.paths_spp(name, n, spp, 1, max(depth, 5)), depth)[2].sum())
    assert st["terms"] == S.terms and st["rays"] == segs and st["paths"] == n * spp
    return got, st, S


def test_sizes_match_refgrad(renderers):
    r, _, _ = renderers("cornell+glow")
    for n in SIZES:
        _, st, S = _check(r, "cornell+glow", n, 5)
        assert st["launches"] == 1 and st["lds_table"] == 1
    assert (S.exact[RG.COLOR] != 0).any(axis=1).sum() >= 8


@pytest.mark.parametrize("spp", [2, 7])
def test_samples(renderers, spp):
    r, _, _ = renderers("cornell+glow")
    _check(r, "cornell+glow", 65, 5, spp)


@pytest.mark.parametrize("depth", [1, 2, 8])
def test_depths(renderers, depth):
    r, _, _ = renderers("random_7_300")
    _, st, S = _check(r, "random_7_300", 257, depth)
    assert st["lds_records"] == 1 and (S.exact[RG.EMIT_K] != 0).any()


FORMS = [(None, None, "lds_table", 1), ("PT_GRAD_LDS", "0", "lds_table", 0), ("PT_TRACE_LDS_REC", "0", "lds_records", 0),
         ("PT_QUERY_LDS_STACK", "0", "lds_stack", 0)]


@pytest.mark.parametrize("hook,value,flag,want", FORMS)
@pytest.mark.parametrize("name", ["cornell+glow", "random_7_300"])
def test_table_forms(renderers, monkeypatch, name, hook, value, flag, want):
    """The per-block LDS table and the global form, and the table beside global records / a global
    stack: all within the tolerance, and the stats say which ran."""
    r, _, _ = renderers(name)
    if hook:
        monkeypatch.setenv(hook, value)
    _, st, _ = _check(r, name, 257, 5, what=f"{name} {hook}={value}")
    if hook:
        monkeypatch.delenv(hook)
    assert st[flag] == want
    if flag != "lds_table":
        assert st["lds_table"] == 1


def test_depth_64_with_global_records(renderers):
    """Depth 64 (records in a global buffer, the re-unwinding form of the kernel) against the host
    path, each within the tolerance of the exact sum: within the sum of both tolerances."""
    name, n = "random_3_40", 64
    r, _, bvh = renderers(name)
    o, d = RT.rays(name, n)
    g = RG.grad_rgb(n)
    _, S = RG.expected(name, n, 64, walk_depth=64)
    got, st = r.trace_grad(o, d, g, 64)
    host, st_h = bvh.trace_grad(o, d, g, 64)
    assert st["lds_records"] == 0 and st["terms"] == st_h["terms"] == S.terms and st["rays"] == st_h["rays"]
    RT.assert_same(got["rgb"], host["rgb"], "depth 64 rgb")
    for k, kind in (("color", RG.COLOR), ("emit", RG.EMIT_K)):
        assert (np.abs(got[k] - host[k]) <= 2 * S.tol[kind]).all(), k
    assert S.count.max() > 8 and (S.exact[RG.EMIT_K] != 0).any()


def test_launches_cut_over_rays(renderers, monkeypatch):
    r, _, _ = renderers("random_7_300")
    monkeypatch.setenv("PT_TRACE_CHUNK", "64")
    _, st, _ = _check(r, "random_7_300", 257, 5, what="five launches")
    monkeypatch.delenv("PT_TRACE_CHUNK")
    assert st["launches"] == 5


def test_gpu_against_host_path(renderers):
    name, n = "random_7_300", 512
    r, _, bvh = renderers(name)
    o, d = RT.rays(name, n)
    g = RG.grad_rgb(n)
    _, S = RG.expected(name, n, 5, 3)
    got, st = r.trace_grad(o, d, g, 5, samples=3)
    host, st_h = bvh.trace_grad(o, d, g, 5, samples=3)
    RT.assert_same(got["rgb"], host["rgb"], "GPU vs host rgb")
    assert st["terms"] == st_h["terms"] == S.terms and st["rays"] == st_h["rays"]
    for k, kind in (("color", RG.COLOR), ("emit", RG.EMIT_K)):
        assert (np.abs(got[k] - host[k]) <= 2 * S.tol[kind]).all(), k
    assert (host["color"] != 0).any() and (host["emit"] != 0).any()


def test_device_tensors(renderers):
    import torch
    name, n = "cornell+glow", 257
    r, sc, _ = renderers(name)
    o, d = RT.rays(name, n)
    g = RG.grad_rgb(n)
    color, emit = RG.overrides(len(sc.mats))
    host, st_h = r.trace_grad(o, d, g, 5, color=color, emit=emit)
    _, S = RG.expected(name, n, 5, override=True)
    RG.assert_within(host["color"], host["emit"], S, "host pointers, override")
    dev = torch.device("cuda", 0)
    ins = [torch.from_numpy(a.copy()).to(dev) for a in (o, d, g, color, emit)]
    res, st = r.trace_grad(ins[0], ins[1], ins[2], 5, color=ins[3], emit=ins[4])
    assert res["color"].dtype == torch.float64 and res["emit"].dtype == torch.float64 and res["rgb"].dtype == torch.float32
    assert all(v.is_cuda for v in res.values()) and tuple(res["color"].shape) == (len(sc.mats), 3)
    RG.assert_within(res["color"].cpu().numpy(), res["emit"].cpu().numpy(), S, "device tensors")
    RT.assert_same(res["rgb"].cpu().numpy(), host["rgb"], "device tensors rgb")
    assert st["terms"] == st_h["terms"] == S.terms and st["launches"] == 1
    for t, a in zip(ins, (o, d, g, color, emit)):
        assert np.array_equal(RW.bits(t.cpu().numpy()), RW.bits(a))  # inputs untouched


@pytest.mark.parametrize("name,variant", RT.TREES)
def test_caller_built_trees(name, variant):
    import ptamd
    o, d, _, t, S = RG.tree_expected(name, variant)
    c = TC.case(name, variant)
    color, emit = RG.overrides(c.verts.shape[0])
    r = ptamd.Renderer(0)
    try:
        r.set_scene(TC.to_bvh(ptamd, c))
        got, st = r.trace_grad(o, d, RG.grad_rgb(256), 5, color=color, emit=emit)
    finally:
        r.close()
    RG.assert_within(got["color"], got["emit"], S, f"{name} {variant}")
    RT.assert_same(got["rgb"], t.rgb, f"{name} {variant} rgb")
    assert st["terms"] == S.terms and st["launches"] == 1


def test_single_paths_are_bit_exact(renderers):
    name, depth = "random_7_300", 8
    r, _, _ = renderers(name)
    P = RT.paths(name)
    o, d = RT.rays(name, 16)
    seeds = RT.sample_seeds(16, 1, 1)[:, 0]
    g = RG.grad_rgb(16)
    for i in range(16):
        Pi = RT.Paths(P.tri[:, i:i + 1], P.cos[:, i:i + 1], P.state[:, i:i + 1], P.init[i:i + 1], P.mtype, P.mvals)
        S = RG.summarize(RG.path_terms(Pi, depth, g[i:i + 1]), P.mvals.shape[0])
        got, st = r.trace_grad(o[i:i + 1], d[i:i + 1], g[i:i + 1], depth, states=seeds[i:i + 1])
        assert np.array_equal(got["color"].view(np.uint64), S.ordered[RG.COLOR].view(np.uint64)), i
        assert np.array_equal(got["emit"].view(np.uint64), S.ordered[RG.EMIT_K].view(np.uint64)), i
        assert st["terms"] == S.terms


def test_autograd(renderers):
    import torch
    from ptamd.autograd import trace_radiance
    name, n = "cornell+glow", 256
    r, sc, _ = renderers(name)
    dev = torch.device("cuda", 0)
    o, d = (torch.from_numpy(a.copy()).to(dev) for a in RT.rays(name, n))
    _, _, _, _, mvals = RT.scene_arrays(name)
    color0, emit0 = mvals[:, 0:3].copy(), mvals[:, 3:6].copy()
    target = r.trace(o, d, 5)[0]
    start = (emit0 * F32(1.5) + F32(0.05)).astype(F32)  # the perturbed start
    color = torch.from_numpy(color0).to(dev).requires_grad_(True)
    emit = torch.from_numpy(start).to(dev).requires_grad_(True)
    rgb = trace_radiance(r, o, d, color, emit, 5, 1, 1)
    loss = ((rgb - target) ** 2).sum()
    loss.backward()
    want, _ = r.trace_grad(o, d, (2 * (rgb - target)).detach().contiguous(), 5, color=color.detach(), emit=emit.detach(),
                           want=("color", "emit"))
    # two runs add the same float32 terms in double in different orders: the sums agree to ~1e-14
    # relative, so their float32 casts are equal unless a sum sits within that of a float32
    # rounding boundary (about 1e-7 per entry)
    for grad, w in ((color.grad, want["color"]), (emit.grad, want["emit"])):
        assert grad.dtype == torch.float32 and (grad != 0).any()
        assert torch.equal(grad, w.to(torch.float32))
    assert float(loss.detach()) > 0
    with torch.no_grad():  # one SGD step on emit lowers the loss (the paths are fixed by the seed)
        step = emit - 1e-4 * emit.grad
    after = ((trace_radiance(r, o, d, color.detach(), step, 5, 1, 1) - target) ** 2).sum()
    assert float(after) < float(loss.detach())


def test_side_effects(renderers):
    """A progressive sum survives a trace_grad call, and the override does not leak into the scene."""
    import ptamd
    name = "random_3_40"
    r, sc, _ = renderers(name)
    cam = ptamd.Camera.from_spec(sc.camera)
    o, d = RT.rays(name, 65)
    color, emit = RG.overrides(len(sc.mats))
    before, _ = r.render(cam, 4, 4)
    r.render_progressive(cam, 0, 2, 4)
    r.trace_grad(o, d, RG.grad_rgb(65), 4, samples=3, color=color, emit=emit)
    img, _ = r.render_progressive(cam, 2, 2, 4)
    assert np.array_equal(RW.bits(img), RW.bits(before))
    after, _ = r.render(cam, 4, 4)
    assert np.array_equal(RW.bits(after), RW.bits(before))
    plain, _ = r.trace_grad(o, d, None, 4, want=("rgb",))
    RT.assert_same(plain["rgb"], r.trace(o, d, 4)[0], "no override after an override")
