"""trace() on caller-supplied rays on the GPU (pt_paths.hip through pt_ctx_trace), bit for bit
against tests/_reftrace.py (trace() restated over the oracle's primitives), the oracle's renders
and the host path. Comparison rule: bits equal, or both NaN."""
import numpy as np
import pytest

import _oracle as O
import _reftrace as RT
import _refwalk as RW
import _treecases as TC
from _plans import _planned

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = (1, 63, 64, 65, 257, 512)


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


@pytest.mark.parametrize("seed", [1, 7])
@pytest.mark.parametrize("name,depth", [("cornell", 5), ("random_7_300", 4), ("sphere12", 5)])
def test_camera_ray_identity(renderers, name, depth, seed):
    """The AOV ray channel traced from the state after the camera's two draws is the render."""
    import ptamd
    r, sc, _ = renderers(name)
    cam = ptamd.Camera.from_spec(sc.camera)
    W, H = sc.camera.res
    a, _ = r.aov(cam, sample=0, seed=seed, channels=("ray",))
    o, d = a["ray"][..., 0:3].reshape(-1, 3), a["ray"][..., 3:6].reshape(-1, 3)
    states = RT.lcg_step(RT.sample_seeds(W * H, 1, seed)[:, 0], 2)
    rgb, st = r.trace(o, d, depth, states=states)
    img, st_r = r.render(cam, 1, depth, seed=seed)
    ref, rays = O.render(sc, 1, depth, seed)
    assert np.array_equal(RW.bits(rgb), RW.bits(img.reshape(-1, 3)))
    assert np.array_equal(RW.bits(rgb), RW.bits(ref.reshape(-1, 3)))
    assert st["rays"] == st_r["rays"] == rays and st["paths"] == W * H and st["launches"] == 1
    assert RW.bits(ref).any()


@pytest.mark.parametrize("name", RT.ALL)
def test_arbitrary_rays_match_restatement(renderers, name):
    r, _, bvh = renderers(name)
    P = RT.paths(name)
    o, d = RT.rays(name, 512)
    for depth in (2, 5):
        want, _, segs = RT.radiance(P, depth)
        for n in SIZES:
            got, st = r.trace(o[:n], d[:n], depth)
            RT.assert_same(got, want[:n], f"{name} depth {depth} n {n}")
            assert st["launches"] == 1 and st["rays"] == int(segs[:n].sum()) and st["paths"] == n
            RT.check_floor(name, got, RT.head(P, n), depth)
        host, st_h = bvh.trace(o, d, depth)
        RT.assert_same(got, host, f"{name} depth {depth}: GPU vs host")
        assert st_h["rays"] == st["rays"]
    if name == "cornell":
        assert st["lds_scene"] == 1 and st["lds_stack"] == 1 and st["lds_records"] == 1


PLACEMENTS = [("PT_LDS_SCENE_BYTES", "0", dict(scene_budget=0)),
              ("PT_LDS_SCENE_BYTES", "65536", dict(scene_budget=65536)),
              ("PT_QUERY_LDS_STACK", "0", dict(stack=False)),
              ("PT_FORCE_EXACT_SLAB", "1", {}),
              ("PT_TRACE_LDS_REC", "0", dict(rec=False))]


@pytest.mark.parametrize("hook,value,rule", PLACEMENTS)
@pytest.mark.parametrize("name", ["random_7_300", "random_3_40"])
def test_placement_variants(renderers, monkeypatch, name, hook, value, rule):
    """Scene, stack and records in LDS or not, and the exact slab form: the same bits, and the
    stats say which form ran. (52 triangles fit the default LDS scene budget, 312 do not.)"""
    import ptamd
    r, sc, bvh = renderers(name)
    info = ptamd.scene_info(bvh)
    o, d = RT.rays(name, 512)
    want, _, segs = RT.radiance(RT.paths(name), 5)
    got0, st0 = r.trace(o, d, 5)
    flags = ("lds_scene", "lds_stack", "lds_records")
    assert {k: st0[k] for k in flags} == _planned(info, len(sc.tris), 5)
    assert st0["lds_stack"] == 1 and st0["lds_records"] == 1 and st0["lds_scene"] == (1 if name == "random_3_40" else 0)
    monkeypatch.setenv(hook, value)
    got, st = r.trace(o, d, 5)
    monkeypatch.delenv(hook)
    RT.assert_same(got, got0, f"{name} {hook}={value} vs default")
    RT.assert_same(got, want, f"{name} {hook}={value}")
    assert st["rays"] == int(segs.sum())
    forced = _planned(info, len(sc.tris), 5, **rule)
    assert {k: st[k] for k in flags} == forced, (st, forced)
    if hook == "PT_LDS_SCENE_BYTES" and value == "0":
        assert st["lds_scene"] == 0
    if hook == "PT_QUERY_LDS_STACK":
        assert st["lds_stack"] == 0
    if hook == "PT_TRACE_LDS_REC":
        assert st["lds_records"] == 0


def test_depth_64_runs_with_global_records(renderers):
    name = "random_3_40+glow"
    r, _, _ = renderers(name)
    o, d = RT.rays(name, 65)
    P = RT.paths(name, n=65, depth=64)
    want, _, segs = RT.radiance(P, 64)
    assert segs.max() > 8  # paths longer than any other test's
    got, st = r.trace(o, d, 64)
    RT.assert_same(got, want, "depth 64")
    assert st["lds_records"] == 0 and st["rays"] == int(segs.sum()) and st["launches"] == 1
    RT.check_floor(name, got, P, 64)


@pytest.mark.parametrize("spp", [2, 7, 64])
def test_samples_sum_in_order(renderers, spp):
    name = "random_7_300"
    r, _, bvh = renderers(name)
    o, d = RT.rays(name, 65)
    want = RT.mean_of_samples(lambda st: r.trace(o, d, 5, states=st)[0], 65, spp, 3)
    got, st = r.trace(o, d, 5, samples=spp, seed=3)
    RT.assert_same(got, want, f"spp {spp}")
    assert st["paths"] == 65 * spp and st["launches"] == 1
    if spp <= 7:
        host, st_h = bvh.trace(o, d, 5, samples=spp, seed=3)
        RT.assert_same(got, host, f"spp {spp}: GPU vs host")
        assert st["rays"] == st_h["rays"]
    assert (RW.bits(got) != 0).any(axis=1).sum() >= 0.5 * 65


def test_launches_cut_over_rays(renderers, monkeypatch):
    name = "random_7_300"
    r, _, _ = renderers(name)
    o, d = RT.rays(name, 257)
    one, st1 = r.trace(o, d, 5, samples=3, seed=5)
    monkeypatch.setenv("PT_TRACE_CHUNK", "64")
    cut, st = r.trace(o, d, 5, samples=3, seed=5)
    monkeypatch.delenv("PT_TRACE_CHUNK")
    RT.assert_same(cut, one, "five launches vs one")
    assert st1["launches"] == 1 and st["launches"] == 5 and st["rays"] == st1["rays"] and st["paths"] == 257 * 3
    want = RT.mean_of_samples(lambda s: r.trace(o, d, 5, states=s)[0], 257, 3, 5)
    RT.assert_same(cut, want, "five launches vs single samples")


def test_nonfinite_rays(renderers):
    """inf and NaN in origins and directions, alone and spliced into a wave of ordinary rays (the
    wave then takes the exact slab form as a whole)."""
    name = "random_7_300"
    r, _, _ = renderers(name)
    o, d, want, segs = RT.nonfinite_expected()
    got, st = r.trace(o, d, 5)
    RT.assert_same(got, want, "non-finite rays")
    assert st["rays"] == int(segs.sum())
    o2, d2 = RT.rays(name, 100)
    st2 = RT.sample_seeds(116, 1, 1)[:, 0]  # ray i of the spliced call is seeded by its index there
    om, dm = np.concatenate([o2[:40], o, o2[40:]]), np.concatenate([d2[:40], d, d2[40:]])
    verts, nodes, idx, mtype, mvals = RT.scene_arrays(name)
    want_m, _, segs_m = RT.trace(nodes, idx, verts, mtype, mvals, om, dm, st2, 5)
    got, st = r.trace(om, dm, 5)
    RT.assert_same(got, want_m, "spliced")
    assert st["rays"] == int(segs_m.sum())
    assert (RW.bits(want_m) != 0).any(axis=1).sum() >= 0.3 * 116


def test_overflowing_direction_on_specular_gives_nan():
    """A dark scene (finish_path's skip is on): a NaN cosine still folds to NaN, as the reference's."""
    import ptamd
    o, d, want, segs = RT.overflow_expected()
    r = ptamd.Renderer(0)
    try:
        r.set_scene(ptamd.BVH.from_scene(RT.overflow_scene()))
        assert r.flags()["dark"]
        got, st = r.trace(o, d, 3)
    finally:
        r.close()
    RT.assert_same(got, want, "overflow")
    assert st["rays"] == segs


def test_device_tensors(renderers):
    import torch
    name = "random_7_300"
    r, _, _ = renderers(name)
    o, d = RT.rays(name, 257)
    states = RT.explicit_states(512)[:257]
    host, st_h = r.trace(o, d, 5, states=states)
    RT.assert_same(host, RT.radiance(RT.head(RT.paths(name, explicit=True), 257), 5)[0], "explicit states")
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev)
    ts = torch.from_numpy(states.view(np.int32).copy()).to(dev)
    out = torch.full((257, 3), -1.0, dtype=torch.float32, device=dev)
    res, st = r.trace(to, td, 5, states=ts, out=out)
    assert res is out and st["rays"] == st_h["rays"] and st["launches"] == 1
    RT.assert_same(out.cpu().numpy(), host, "device tensors")
    assert np.array_equal(RW.bits(to.cpu().numpy()), RW.bits(o)) and np.array_equal(RW.bits(td.cpu().numpy()), RW.bits(d))
    assert np.array_equal(ts.cpu().numpy().view(np.uint32), states)
    res2, _ = r.trace(to, td, 5, samples=2, seed=3)  # default seeding, output allocated
    assert res2.is_cuda and tuple(res2.shape) == (257, 3)
    RT.assert_same(res2.cpu().numpy(), r.trace(o, d, 5, samples=2, seed=3)[0], "device default seeding")


@pytest.mark.parametrize("name,variant", RT.TREES)
def test_caller_built_trees(name, variant):
    import ptamd
    o, d, want, segs = RT.tree_expected(name, variant)
    r = ptamd.Renderer(0)
    try:
        r.set_scene(TC.to_bvh(ptamd, TC.case(name, variant)))
        got, st = r.trace(o, d, 5)
    finally:
        r.close()
    RT.assert_same(got, want, f"{name} {variant}")
    assert st["rays"] == segs and st["launches"] == 1


def test_trace_leaves_progressive_sum(renderers):
    import ptamd
    r, sc, _ = renderers("random_3_40")
    cam = ptamd.Camera.from_spec(sc.camera)
    o, d = RT.rays("random_3_40", 65)
    r.render_progressive(cam, 0, 2, 4)
    r.trace(o, d, 4, samples=3)
    img, _ = r.render_progressive(cam, 2, 2, 4)
    one_shot, _ = r.render(cam, 4, 4)
    assert np.array_equal(RW.bits(img), RW.bits(one_shot))
