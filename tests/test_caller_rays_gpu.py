"""The host loop that trace, trace_nee and trace_grad share (cuts over rays, staging, seeding) and
the stream rule of the tensor paths, on the GPU: one call cut into launches against the same call
in one launch and against the host form, numpy arrays and device tensors alike; rays that torch
has queued but not written yet; render_nee's moments on a device image. Comparison rule: bits
equal, or both NaN; gradients within _refgrad's derived any-order tolerance."""
import functools

import numpy as np
import pytest

import _refgrad as RG
import _reftrace as RT
import _refwalk as RW

pytestmark = pytest.mark.gpu

NAME, N, SPP, DEPTH = "random_7_300", 257, 3, 5  # four launches of 64 rays and a one-ray tail
COUNTERS = ("rays", "paths", "shadow_rays", "light_draws", "terms")


@pytest.fixture(scope="module")
def scene():
    import ptamd
    sc = RT.make_scene(NAME)
    bvh = ptamd.BVH.from_scene(sc)
    r = ptamd.Renderer(0)
    r.set_scene(bvh)
    yield r, sc, bvh
    r.close()


def explicit_states():
    """Sample s of ray i starts at entry i * SPP + s: the states offset of a cut is not its ray offset."""
    return RT.explicit_states(N * SPP)


@functools.lru_cache(maxsize=None)
def grad_expected():
    """(Terms, Summary) of the N rays' SPP paths from `explicit_states`, with RG.grad_rgb(N)."""
    verts, nodes, idx, mtype, mvals = RT.scene_arrays(NAME)
    o, d = RT.rays(NAME, N)
    P = RT.walk_paths(nodes, idx, verts, mtype, mvals, np.repeat(o, SPP, axis=0), np.repeat(d, SPP, axis=0),
                      explicit_states(), DEPTH)
    t = RG.path_terms(P, DEPTH, RG.grad_rgb(N), SPP)
    return t, RG.summarize(t, mvals.shape[0])


def _to_numpy(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _call(target, entry, arrays, states, tensors=False):
    """`entry` of a Renderer or a BVH on copies of (o, d, grad_rgb) and the states: (rgb, gradients
    or None, stats, the copies as passed)."""
    ins = [a.copy() for a in arrays + (states,)]
    if tensors:
        import torch
        ins = [torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0") for a in ins]
    if entry == "trace_grad":
        res, st = target.trace_grad(ins[0], ins[1], ins[2], DEPTH, samples=SPP, states=ins[3])
        return _to_numpy(res["rgb"]), (_to_numpy(res["color"]), _to_numpy(res["emit"])), st, ins
    rgb, st = getattr(target, entry)(ins[0], ins[1], DEPTH, samples=SPP, states=ins[3])
    return _to_numpy(rgb), None, st, ins


@pytest.mark.parametrize("tensors", [False, True], ids=["numpy", "tensors"])
@pytest.mark.parametrize("entry", ["trace", "trace_nee", "trace_grad"])
def test_cut_staged_and_seeded(scene, monkeypatch, entry, tensors):
    """257 rays x 3 samples with explicit states in launches of 64 rays: the same bits and counters
    as one launch and as the host form, five launches, the inputs untouched."""
    r, _, bvh = scene
    o, d = RT.rays(NAME, N)
    arrays, states = (o, d, RG.grad_rgb(N)), explicit_states()
    one, g1, st1, _ = _call(r, entry, arrays, states, tensors)
    monkeypatch.setenv("PT_TRACE_CHUNK", "64")
    cut, g, st, ins = _call(r, entry, arrays, states, tensors)
    monkeypatch.delenv("PT_TRACE_CHUNK")
    host, _, st_h, _ = _call(bvh, entry, arrays, states)
    assert st1["launches"] == 1 and st["launches"] == 5
    RT.assert_same(cut, one, f"{entry}: five launches vs one")
    RT.assert_same(cut, host, f"{entry}: five launches vs the host form")
    assert RW.bits(cut).any()
    for k in COUNTERS:
        if k in st1:
            assert st[k] == st1[k] == st_h[k], (k, st, st1, st_h)
    assert st["paths"] == N * SPP and st["rays"] > 0
    for x, a in zip(ins, arrays + (states,)):
        assert np.array_equal(_to_numpy(x).view(np.uint32), a.view(np.uint32))  # inputs untouched
    if entry == "trace_grad":
        t, S = grad_expected()
        for what, (color, emit) in (("five launches", g), ("one launch", g1)):
            print(what, "max |err| / tol", float(np.nanmax(np.abs(np.stack([color, emit]) - S.exact) / np.maximum(S.tol, 1e-300))))
            RG.assert_within(color, emit, S, f"{entry} {what}")
        RT.assert_same(cut, RG.mean_rgb(t, SPP), "trace_grad rgb")
        assert st["terms"] == S.terms and (S.exact[RG.COLOR] != 0).any() and (S.exact[RG.EMIT_K] != 0).any()


def _in_flight(call, check):
    """`call` on rays that are results of torch operations queued behind about a hundred
    milliseconds of matrix products: when it is made they are not written yet."""
    import torch
    o, d = RT.rays(NAME, N)
    to, td = torch.from_numpy(o.copy()).to("cuda:0"), torch.from_numpy(d.copy()).to("cuda:0")
    a = torch.randn((6144, 6144), device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):  # the second round reuses the first one's freed blocks
        b = a
        for _ in range(12):
            b = torch.tanh(b @ a * 1e-2)
        zero = (b[0, 0] * 0).nan_to_num()  # 0, known only when the products are done
        o2, d2 = to + zero, td + zero
        got = call(o2, d2, zero)
        check(got)
        del o2, d2, got
    return to, td


def test_trace_rays_still_in_flight(scene):
    """The library's stream does not order itself after torch's, so the tensor path waits for
    torch's current stream first; without the wait the results differ from the numpy path's."""
    r, _, _ = scene
    o, d = RT.rays(NAME, N)
    want, _ = r.trace(o, d, DEPTH)
    to, td = _in_flight(lambda o2, d2, _: r.trace(o2, d2, DEPTH)[0],
                        lambda got: RT.assert_same(got.cpu().numpy(), want, "rays in flight"))
    with pytest.raises(ValueError):
        r.trace(to, td.cpu(), DEPTH)  # a tensor that is not on the context's device


def test_trace_grad_rays_still_in_flight(scene):
    import torch
    r, _, _ = scene
    o, d = RT.rays(NAME, N)
    g = RG.grad_rgb(N)
    want, _ = r.trace_grad(o, d, g, DEPTH)
    _, S = RG.expected(NAME, N, DEPTH)
    tg = torch.from_numpy(g.copy()).to("cuda:0")

    def check(got):
        RT.assert_same(got["rgb"].cpu().numpy(), want["rgb"], "rays in flight")
        RG.assert_within(got["color"].cpu().numpy(), got["emit"].cpu().numpy(), S, "rays in flight")

    to, td = _in_flight(lambda o2, d2, zero: r.trace_grad(o2, d2, tg + zero, DEPTH)[0], check)
    RG.assert_within(want["color"], want["emit"], S, "numpy path")
    with pytest.raises(ValueError):
        r.trace_grad(to, td, tg.cpu(), DEPTH)
    with pytest.raises(ValueError):
        r.trace_grad(to, td.cpu(), tg, DEPTH)


def test_intersect_rays_still_in_flight(scene):
    r, _, _ = scene
    o, d = RT.rays(NAME, N)
    (t, tri), _ = r.intersect(o, d)
    assert (tri >= 0).any()

    def check(got):
        bad = int((RW.bits(got[0].cpu().numpy()) != RW.bits(t)).sum() + (got[1].cpu().numpy() != tri).sum())
        assert bad == 0, f"rays in flight: {bad} of {2 * N} results differ from the numpy path's"

    to, td = _in_flight(lambda o2, d2, _: r.intersect(o2, d2)[0], check)
    with pytest.raises(ValueError):
        r.intersect(to, td.cpu())


@pytest.mark.parametrize("name", ["cornell", "random_7_300"])
def test_render_nee_moments_on_a_device_image(name):
    """render_nee(out=tensor, want=all three): the image and the moments equal the host arrays'
    (which test_nee_gpu compares with trace_nee on the camera rays) bit for bit."""
    import ptamd
    import torch
    sc = RT.make_scene(name, (16, 16))
    cam = ptamd.Camera.from_spec(sc.camera)
    W, H = sc.camera.res
    want = ("sum", "sumsq", "sem")
    r = ptamd.Renderer(0)
    try:
        r.set_scene(ptamd.BVH.from_scene(sc))
        img, mom, st_h = r.render_nee(cam, 5, 5, seed=9, want=want)
        out = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda:0")
        img_d, mom_d, st = r.render_nee(cam, 5, 5, seed=9, out=out, want=want)
    finally:
        r.close()
    assert img_d is out and sorted(mom_d) == sorted(want) and all(v.is_cuda for v in mom_d.values())
    assert np.array_equal(RW.bits(out.cpu().numpy()), RW.bits(img)) and RW.bits(img).any()
    for k in ("sum", "sumsq"):
        assert mom_d[k].dtype == torch.float64 and np.array_equal(mom_d[k].cpu().numpy().view(np.uint64), mom[k].view(np.uint64))
    assert mom_d["sem"].dtype == torch.float32 and np.array_equal(RW.bits(mom_d["sem"].cpu().numpy()), RW.bits(mom["sem"]))
    assert (mom["sem"] > 0).any() and st["rays"] == st_h["rays"] and st["shadow_rays"] == st_h["shadow_rays"] > 0
