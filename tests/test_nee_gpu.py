"""The light-sampling estimator on the GPU (pt_nee.hip through pt_ctx_trace_nee and
pt_ctx_render_nee), bit for bit against the host form and tests/_refnee.py (the definition of
include/pt_hip.h restated over the oracle's primitives). Comparison rule: bits equal, or both NaN."""
import numpy as np
import pytest

import _refnee as RN
import _reftrace as RT
import _refwalk as RW
import _treecases as TC
from _plans import _planned

pytestmark = pytest.mark.gpu

F32 = np.float32
NEE_KEYS = ("rays", "paths", "runaway", "shadow_rays", "light_draws", "lights", "light_area")


@pytest.fixture(scope="module")
def renderers():
    """One context per scene name (glow variants included), scene uploaded; closed at the end."""
    import ptamd
    made = {}

    def get(name, res=(16, 16)):
        key = (name, tuple(res))
        if key not in made:
            sc = RT.make_scene(name, res)
            bvh = ptamd.BVH.from_scene(sc)
            r = ptamd.Renderer(0)
            r.set_scene(bvh)
            made[key] = (r, sc, bvh)
        return made[key]

    yield get
    for r, _, _ in made.values():
        r.close()


def same_stats(a, b):
    assert {k: a[k] for k in NEE_KEYS} == {k: b[k] for k in NEE_KEYS}, (a, b)


@pytest.mark.parametrize("name", RN.SCENES)
def test_trace_nee_matches_host_and_restatement(renderers, name):
    r, _, bvh = renderers(name)
    o, d = RT.rays(name, 512)
    for explicit in (False, True):
        P = RN.paths(name, explicit=explicit)
        states = RT.explicit_states(512) if explicit else None
        for depth in RN.DEPTHS:
            want, segs, sh, dr = RN.radiance(P, depth)
            got, st = r.trace_nee(o, d, depth, states=states)
            RT.assert_same(got, want, f"{name} depth {depth} explicit {explicit}")
            assert st["launches"] == 1 and st["rays"] == int(segs.sum()) and st["shadow_rays"] == int(sh.sum())
            assert st["light_draws"] == int(dr.sum()) and st["paths"] == 512
            host, st_h = bvh.trace_nee(o, d, depth, states=states)
            RT.assert_same(got, host, f"{name} depth {depth}: GPU vs host")
            same_stats(st, st_h)
    # spp 7: the in-order sum, seeded and with explicit states laid out [ray][sample]
    host, st_h = bvh.trace_nee(o, d, 5, samples=7, seed=3)
    got, st = r.trace_nee(o, d, 5, samples=7, seed=3)
    RT.assert_same(got, host, f"{name} spp 7")
    same_stats(st, st_h)
    got2, st2 = r.trace_nee(o, d, 5, samples=7, states=RT.sample_seeds(512, 7, 3))
    RT.assert_same(got2, host, f"{name} spp 7, states")
    same_stats(st2, st_h)
    assert st["shadow_rays"] > 0
    if name == "cornell":
        assert st["lds_scene"] == 1 and st["lds_stack"] == 1


PLACEMENTS = [("PT_LDS_SCENE_BYTES", "0", dict(scene_budget=0)), ("PT_LDS_SCENE_BYTES", "65536", dict(scene_budget=65536)),
              ("PT_QUERY_LDS_STACK", "0", dict(stack=False)), ("PT_FORCE_EXACT_SLAB", "1", {})]


@pytest.mark.parametrize("hook,value,rule", PLACEMENTS)
@pytest.mark.parametrize("name", ["random_7_300", "random_3_40"])
def test_placement_variants(renderers, monkeypatch, name, hook, value, rule):
    """Scene and stack in LDS or not, and the exact slab form: the same bits, and the stats say
    which form ran, by the placement rule of the binary walk (tests/_plans.py; the scene and the
    stack are placed before any record row, so the rule's answer for them holds with none).
    (52 triangles fit the default LDS scene budget, 312 do not.)"""
    import ptamd
    r, sc, bvh = renderers(name)
    info = ptamd.scene_info(bvh)
    flags = ("lds_scene", "lds_stack")
    o, d = RT.rays(name, 512)
    want, segs, sh, _ = RN.radiance(RN.paths(name), 5)
    got0, st0 = r.trace_nee(o, d, 5)
    assert {k: st0[k] for k in flags} == {k: _planned(info, len(sc.tris), 5)[k] for k in flags}
    assert st0["lds_stack"] == 1 and st0["lds_scene"] == (1 if name == "random_3_40" else 0)
    monkeypatch.setenv(hook, value)
    got, st = r.trace_nee(o, d, 5)
    monkeypatch.delenv(hook)
    RT.assert_same(got, want, f"{name} {hook}={value}")
    RT.assert_same(got0, want, f"{name} default")
    assert st["rays"] == int(segs.sum()) and st["shadow_rays"] == int(sh.sum()) > 0
    forced = _planned(info, len(sc.tris), 5, **rule)
    assert {k: st[k] for k in flags} == {k: forced[k] for k in flags}, (st, forced)
    if hook == "PT_LDS_SCENE_BYTES" and value == "0":
        assert st["lds_scene"] == 0
    if hook == "PT_QUERY_LDS_STACK":
        assert st["lds_stack"] == 0


def test_launches_cut_over_rays(renderers, monkeypatch):
    name = "random_7_300"
    r, _, _ = renderers(name)
    o, d = RT.rays(name, 300)
    one, st1 = r.trace_nee(o, d, 5, samples=3, seed=5)
    monkeypatch.setenv("PT_TRACE_CHUNK", "64")
    cut, st = r.trace_nee(o, d, 5, samples=3, seed=5)
    monkeypatch.delenv("PT_TRACE_CHUNK")
    RT.assert_same(cut, one, "five launches vs one")
    assert st1["launches"] == 1 and st["launches"] == 5 > 1
    same_stats(st, st1)
    assert st["paths"] == 300 * 3 and st["shadow_rays"] > 0


def test_nonfinite_rays(renderers):
    r, _, bvh = renderers("random_7_300")
    o, d, want, segs, sh = RN.nonfinite_expected()
    got, st = r.trace_nee(o, d, 5)
    RT.assert_same(got, want, "non-finite rays")
    assert st["rays"] == segs and st["shadow_rays"] == sh
    same_stats(st, bvh.trace_nee(o, d, 5)[1])


@pytest.mark.parametrize("name,variant", [("cornell", "merged5"), ("mcornell", "duplicated")])
def test_caller_built_trees(name, variant):
    import ptamd
    o, d, want, segs, sh = RN.tree_expected(name, variant)
    bvh = TC.to_bvh(ptamd, TC.case(name, variant))
    r = ptamd.Renderer(0)
    try:
        r.set_scene(bvh)
        got, st = r.trace_nee(o, d, 5)
    finally:
        r.close()
    RT.assert_same(got, want, f"{name} {variant}")
    host, st_h = bvh.trace_nee(o, d, 5)
    RT.assert_same(got, host, f"{name} {variant}: GPU vs host")
    same_stats(st, st_h)
    assert st["rays"] == segs and st["shadow_rays"] == sh and st["launches"] == 1


def test_device_tensors(renderers):
    import torch
    name = "random_7_300"
    r, _, _ = renderers(name)
    o, d = RT.rays(name, 257)
    states = RT.explicit_states(512)[:257]
    host, st_h = r.trace_nee(o, d, 5, states=states)
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev)
    ts = torch.from_numpy(states.view(np.int32).copy()).to(dev)
    out = torch.full((257, 3), -1.0, dtype=torch.float32, device=dev)
    res, st = r.trace_nee(to, td, 5, states=ts, out=out)
    assert res is out and st["launches"] == 1
    same_stats(st, st_h)
    RT.assert_same(out.cpu().numpy(), host, "device tensors")
    assert np.array_equal(RW.bits(to.cpu().numpy()), RW.bits(o)) and np.array_equal(RW.bits(td.cpu().numpy()), RW.bits(d))
    assert np.array_equal(ts.cpu().numpy().view(np.uint32), states)
    res2, _ = r.trace_nee(to, td, 5, samples=2, seed=3)  # default seeding, output allocated
    assert res2.is_cuda and tuple(res2.shape) == (257, 3)
    RT.assert_same(res2.cpu().numpy(), r.trace_nee(o, d, 5, samples=2, seed=3)[0], "device default seeding")
    with pytest.raises(ValueError):
        r.trace_nee(to, td.cpu(), 5)  # a tensor that is not on the context's device


def test_rays_still_in_flight_on_torchs_stream(renderers):
    """The library's stream does not order itself after torch's, so the tensor path waits for
    torch's current stream first. Here the rays are the results of torch operations queued behind
    about a hundred milliseconds of matrix products: when trace_nee is called they are not written
    yet. Without the wait the results differ from the numpy path's."""
    import torch
    name = "random_7_300"
    r, _, _ = renderers(name)
    o, d = RT.rays(name, 257)
    want, _ = r.trace_nee(o, d, 5)
    to, td = torch.from_numpy(o.copy()).to("cuda:0"), torch.from_numpy(d.copy()).to("cuda:0")
    a = torch.randn((6144, 6144), device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):  # the second round reuses the first one's freed blocks
        b = a
        for _ in range(12):
            b = torch.tanh(b @ a * 1e-2)
        zero = (b[0, 0] * 0).nan_to_num()  # 0, known only when the products are done
        o2, d2 = to + zero, td + zero
        got, _ = r.trace_nee(o2, d2, 5)
        RT.assert_same(got.cpu().numpy(), want, "rays in flight")
        del o2, d2, got


def _camera_samples(r, cam, W, H, spp, seed):
    """Per sample s: the AOV rays of sample s and the states after the camera's two draws."""
    seeds = RT.sample_seeds(W * H, spp, seed)
    for s in range(spp):
        a, _ = r.aov(cam, sample=s, seed=seed, channels=("ray",))
        o, d = a["ray"][..., 0:3].reshape(-1, 3), a["ray"][..., 3:6].reshape(-1, 3)
        yield np.ascontiguousarray(o), np.ascontiguousarray(d), RT.lcg_step(seeds[:, s], 2)


@pytest.mark.parametrize("name", ["cornell", "random_7_300"])
def test_render_nee_is_trace_nee_on_the_camera_rays(renderers, name):
    import ptamd
    r, sc, _ = renderers(name)
    cam = ptamd.Camera.from_spec(sc.camera)
    W, H = sc.camera.res
    spp, depth, seed = 5, 5, 9
    acc = np.zeros((W * H, 3), dtype=F32)
    S = np.zeros((W * H, 3), dtype=np.float64)
    Q = np.zeros((W * H, 3), dtype=np.float64)
    rays = shadows = 0
    with np.errstate(all="ignore"):
        for o, d, st in _camera_samples(r, cam, W, H, spp, seed):
            x, s1 = r.trace_nee(o, d, depth, states=st)
            acc = acc + x
            S = S + x.astype(np.float64)
            Q = Q + x.astype(np.float64) * x.astype(np.float64)
            rays += s1["rays"]
            shadows += s1["shadow_rays"]
        want = (acc / F32(spp)).astype(F32)
        var = np.maximum(0.0, (Q - S * S / spp) / (spp - 1.0))
        sem = np.sqrt(var / spp).astype(F32)
    img, mom, st = r.render_nee(cam, spp, depth, seed=seed, want=("sum", "sumsq", "sem"))
    assert img.shape == (H, W, 3) and RW.bits(img).any()
    RT.assert_same(img.reshape(-1, 3), want, f"{name}: render_nee vs trace_nee on the AOV rays")
    assert np.array_equal(mom["sum"].reshape(-1, 3), S) and np.array_equal(mom["sumsq"].reshape(-1, 3), Q)
    assert np.array_equal(RW.bits(mom["sem"].reshape(-1, 3)), RW.bits(sem))
    assert st["rays"] == rays and st["shadow_rays"] == shadows > 0 and st["paths"] == W * H * spp
    # without moments the image is the same
    img2, none, _ = r.render_nee(cam, spp, depth, seed=seed)
    assert none == {} and np.array_equal(RW.bits(img2), RW.bits(img))
    # the parts of part_count = 3 concatenate to the whole frame
    rows = [r.render_nee(cam, spp, depth, seed=seed, part_index=p, part_count=3, band_rows=2, want=("sum",)) for p in range(3)]
    whole = np.zeros_like(img)
    whole_S = np.zeros((H, W, 3))
    for p, (part, pm, _) in enumerate(rows):
        hs = [h for h in range(H) if (h // 2) % 3 == p]
        assert part.shape[0] == len(hs)
        whole[hs] = part
        whole_S[hs] = pm["sum"]
    assert np.array_equal(RW.bits(whole), RW.bits(img)) and np.array_equal(whole_S, mom["sum"])


def test_samples_cut_over_launches(renderers, monkeypatch):
    import ptamd
    r, sc, _ = renderers("random_7_300")
    cam = ptamd.Camera.from_spec(sc.camera)
    one, m1, st1 = r.render_nee(cam, 5, 5, seed=2, want=("sum", "sumsq"))
    monkeypatch.setenv("PT_NEE_CHUNK", "2")
    cut, m, st = r.render_nee(cam, 5, 5, seed=2, want=("sum", "sumsq"))
    monkeypatch.delenv("PT_NEE_CHUNK")
    assert st1["launches"] == 1 and st["launches"] == 3
    assert np.array_equal(RW.bits(cut), RW.bits(one)) and np.array_equal(m["sum"], m1["sum"]) and np.array_equal(m["sumsq"], m1["sumsq"])
    same_stats(st, st1)


def test_running_sums(renderers):
    """trace_nee leaves a progressive sum valid; render_nee, as any render, ends it."""
    import ptamd
    r, sc, _ = renderers("random_3_40")
    cam = ptamd.Camera.from_spec(sc.camera)
    o, d = RT.rays("random_3_40", 65)
    r.render_progressive(cam, 0, 2, 4)
    r.trace_nee(o, d, 4, samples=3)
    img, _ = r.render_progressive(cam, 2, 2, 4)
    one_shot, _ = r.render(cam, 4, 4)
    assert np.array_equal(RW.bits(img), RW.bits(one_shot))
    r.render_progressive(cam, 0, 2, 4)
    r.render_nee(cam, 2, 4)
    with pytest.raises(ptamd.PTError):
        r.render_progressive(cam, 2, 2, 4)


def test_composition_with_the_denoiser(renderers):
    """render_nee(out=tensor, want=("sum", "sumsq")) -> moments_variance -> aov(device=True)
    guides -> denoise, all on the device, equals the same chain on numpy arrays bit for bit."""
    import ptamd
    import torch
    r, sc, _ = renderers("cornell", (32, 32))
    cam = ptamd.Camera.from_spec(sc.camera)
    spp, depth, seed = 4, 5, 3
    img, mom, _ = r.render_nee(cam, spp, depth, seed=seed, want=("sum", "sumsq"))
    aov, _ = r.aov(cam, sample=0, seed=seed)
    var = ptamd.moments_variance(mom["sum"], mom["sumsq"], spp)
    want, _ = ptamd.denoise(img, ptamd.denoise_guides(aov), var)
    out = torch.empty((32, 32, 3), dtype=torch.float32, device="cuda:0")
    img_d, mom_d, _ = r.render_nee(cam, spp, depth, seed=seed, out=out, want=("sum", "sumsq"))
    assert img_d is out and mom_d["sum"].is_cuda
    assert np.array_equal(RW.bits(out.cpu().numpy()), RW.bits(img))
    var_d = r.moments_variance(mom_d["sum"], mom_d["sumsq"], spp)
    aov_d, _ = r.aov(cam, sample=0, seed=seed, device=True)
    den, _, _ = r.denoise(out, ptamd.denoise_guides(aov_d), var_d)
    assert np.array_equal(RW.bits(den.cpu().numpy()), RW.bits(want)) and RW.bits(want).any()
