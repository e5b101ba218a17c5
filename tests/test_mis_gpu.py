"""The weighted light-sampling estimator (PT_NEE_MIS_BALANCE) on the GPU: the pt_nee_mis kernels
of pt_nee.hip through pt_ctx_trace_nee_opt and pt_ctx_render_nee_opt, bit for bit against the
host form pt_bvh_trace_nee_opt (which tests/test_mis_cpu.py holds to tests/_refmis.py, the
definition of include/pt_hip.h restated over the oracle's primitives). Comparison rule: bits
equal, or both NaN."""
import ctypes as C

import numpy as np
import pytest

import _refmis as RM
import _refnee as RN
import _reftrace as RT
import _refwalk as RW
import _treecases as TC
from _plans import _planned
from test_nee_gpu import NEE_KEYS, PLACEMENTS, _camera_samples

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 272  # not a multiple of the wave's 64 lanes


@pytest.fixture(scope="module")
def renderers():
    """One context per scene name (glow variants and tri3 included), scene uploaded; closed at the end."""
    import ptamd
    made = {}

    def get(name, res=(16, 16)):
        key = (name, tuple(res))
        if key not in made:
            sc = RM.tri3_scene() if name == "tri3" else RT.make_scene(name, res)
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
def test_trace_nee_mis_matches_host(renderers, name):
    r, _, bvh = renderers(name)
    o, d = RT.rays(name, N)
    shadows = changed = 0
    for explicit in (False, True):
        for spp in (1, 3):
            states = RT.explicit_states(N * spp).reshape(N, spp) if explicit else None
            for depth in RN.DEPTHS:
                got, st = r.trace_nee(o, d, depth, samples=spp, seed=3, states=states, mis=True)
                host, st_h = bvh.trace_nee(o, d, depth, samples=spp, seed=3, states=states, mis=True)
                RT.assert_same(got, host, f"{name} depth {depth} spp {spp} explicit {explicit}")
                same_stats(st, st_h)
                assert st["launches"] == 1 and st["paths"] == N * spp
                shadows += st["shadow_rays"]
                changed += int((~RT.same_bits(got, r.trace_nee(o, d, depth, samples=spp, seed=3, states=states)[0]).all(axis=1)).sum())
    assert shadows > 0 and changed > 0  # the weights were applied
    # one case against the restatement itself
    want, segs, sh, dr = RM.radiance(RM.paths(name), 5)
    got, st = r.trace_nee(*RT.rays(name, 512), 5, mis=True)
    RT.assert_same(got, want, f"{name}: GPU vs restatement")
    assert st["rays"] == int(segs.sum()) and st["shadow_rays"] == int(sh.sum()) and st["light_draws"] == int(dr.sum())
    if name == "cornell":
        assert st["lds_scene"] == 1 and st["lds_stack"] == 1


@pytest.mark.parametrize("depth", [2, 5])
def test_edge_rays(renderers, depth):
    """tri3's emitter touches its diffuse triangle: weights far from 0 and 1, and a bounded sample."""
    r, _, bvh = renderers("tri3")
    o, d = RM.edge_rays(512)
    got, st = r.trace_nee(o, d, depth, mis=True)
    host, st_h = bvh.trace_nee(o, d, depth, mis=True)
    RT.assert_same(got, host, f"edge rays depth {depth}")
    same_stats(st, st_h)
    assert st["shadow_rays"] > 0 and RW.bits(got).any()
    plain, st_p = r.trace_nee(o, d, depth)
    same_stats(st, st_p)  # the same draws and segments
    assert not RT.same_bits(got, plain).all()


@pytest.mark.parametrize("hook,value,rule", PLACEMENTS)
@pytest.mark.parametrize("name", ["random_7_300", "random_3_40"])
def test_placement_variants(renderers, monkeypatch, name, hook, value, rule):
    """Scene and stack in LDS or not, and the exact slab form: each picks another of the eight
    weighted kernels (or the other slab walk); the same bits, and the stats say which form ran."""
    import ptamd
    r, sc, bvh = renderers(name)
    info = ptamd.scene_info(bvh)
    flags = ("lds_scene", "lds_stack")
    o, d = RT.rays(name, N)
    want, st_h = bvh.trace_nee(o, d, 5, mis=True)
    got0, st0 = r.trace_nee(o, d, 5, mis=True)
    assert {k: st0[k] for k in flags} == {k: _planned(info, len(sc.tris), 5)[k] for k in flags}
    monkeypatch.setenv(hook, value)
    got, st = r.trace_nee(o, d, 5, mis=True)
    monkeypatch.delenv(hook)
    RT.assert_same(got, want, f"{name} {hook}={value}")
    RT.assert_same(got0, want, f"{name} default")
    same_stats(st, st_h)
    assert st["shadow_rays"] > 0
    forced = _planned(info, len(sc.tris), 5, **rule)
    assert {k: st[k] for k in flags} == {k: forced[k] for k in flags}, (st, forced)
    if hook == "PT_LDS_SCENE_BYTES" and value == "0":
        assert st["lds_scene"] == 0
    if hook == "PT_QUERY_LDS_STACK":
        assert st["lds_stack"] == 0


def test_launches_cut_over_rays(renderers, monkeypatch):
    name = "random_7_300"
    r, _, bvh = renderers(name)
    o, d = RT.rays(name, 300)
    one, st1 = r.trace_nee(o, d, 5, samples=3, seed=5, mis=True)
    monkeypatch.setenv("PT_TRACE_CHUNK", "64")
    cut, st = r.trace_nee(o, d, 5, samples=3, seed=5, mis=True)
    monkeypatch.delenv("PT_TRACE_CHUNK")
    RT.assert_same(cut, one, "five launches vs one")
    RT.assert_same(cut, bvh.trace_nee(o, d, 5, samples=3, seed=5, mis=True)[0], "cut launches vs host")
    assert st1["launches"] == 1 and st["launches"] == 5
    same_stats(st, st1)
    assert st["paths"] == 300 * 3 and st["shadow_rays"] > 0


def test_nonfinite_rays(renderers):
    r, _, bvh = renderers("random_7_300")
    o, d = RW.nonfinite_rays()
    got, st = r.trace_nee(o, d, 5, mis=True)
    host, st_h = bvh.trace_nee(o, d, 5, mis=True)
    RT.assert_same(got, host, "non-finite rays")
    same_stats(st, st_h)
    assert st["rays"] > 16


@pytest.mark.parametrize("name,variant", [("cornell", "merged5"), ("mcornell", "duplicated")])
def test_caller_built_trees(name, variant):
    import ptamd
    o, d = TC.rays()
    bvh = TC.to_bvh(ptamd, TC.case(name, variant))
    r = ptamd.Renderer(0)
    try:
        r.set_scene(bvh)
        got, st = r.trace_nee(o, d, 5, mis=True)
    finally:
        r.close()
    host, st_h = bvh.trace_nee(o, d, 5, mis=True)
    RT.assert_same(got, host, f"{name} {variant}: GPU vs host")
    same_stats(st, st_h)
    assert st["shadow_rays"] > 0 and st["launches"] == 1


def test_device_tensors(renderers):
    import torch
    name = "random_7_300"
    r, _, bvh = renderers(name)
    o, d = RT.rays(name, 257)
    states = RT.explicit_states(512)[:257]
    host, st_h = bvh.trace_nee(o, d, 5, states=states, mis=True)
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev)
    ts = torch.from_numpy(states.view(np.int32).copy()).to(dev)
    out = torch.full((257, 3), -1.0, dtype=torch.float32, device=dev)
    res, st = r.trace_nee(to, td, 5, states=ts, out=out, mis=True)
    assert res is out and st["launches"] == 1
    same_stats(st, st_h)
    RT.assert_same(out.cpu().numpy(), host, "device tensors")
    assert np.array_equal(RW.bits(to.cpu().numpy()), RW.bits(o)) and np.array_equal(RW.bits(td.cpu().numpy()), RW.bits(d))
    assert np.array_equal(ts.cpu().numpy().view(np.uint32), states)


@pytest.mark.parametrize("name", ["cornell", "random_7_300"])
def test_render_nee_mis_is_trace_nee_mis_on_the_camera_rays(renderers, monkeypatch, name):
    import ptamd
    r, sc, _ = renderers(name)
    cam = ptamd.Camera.from_spec(sc.camera)
    W, H = sc.camera.res
    spp, depth, seed = 3, 5, 9
    acc = np.zeros((W * H, 3), dtype=F32)
    S = np.zeros((W * H, 3), dtype=np.float64)
    Q = np.zeros((W * H, 3), dtype=np.float64)
    rays = shadows = 0
    with np.errstate(all="ignore"):
        for o, d, st in _camera_samples(r, cam, W, H, spp, seed):
            x, s1 = r.trace_nee(o, d, depth, states=st, mis=True)
            acc = acc + x
            S = S + x.astype(np.float64)
            Q = Q + x.astype(np.float64) * x.astype(np.float64)
            rays += s1["rays"]
            shadows += s1["shadow_rays"]
        want = (acc / F32(spp)).astype(F32)
        var = np.maximum(0.0, (Q - S * S / spp) / (spp - 1.0))
        sem = np.sqrt(var / spp).astype(F32)
    img, mom, st = r.render_nee(cam, spp, depth, seed=seed, want=("sum", "sumsq", "sem"), mis=True)
    assert img.shape == (H, W, 3) and RW.bits(img).any()
    RT.assert_same(img.reshape(-1, 3), want, f"{name}: render_nee vs trace_nee on the AOV rays")
    assert np.array_equal(mom["sum"].reshape(-1, 3), S) and np.array_equal(mom["sumsq"].reshape(-1, 3), Q)
    assert np.array_equal(RW.bits(mom["sem"].reshape(-1, 3)), RW.bits(sem))
    assert st["rays"] == rays and st["shadow_rays"] == shadows > 0 and st["paths"] == W * H * spp and st["launches"] == 1
    plain, _, st_p = r.render_nee(cam, spp, depth, seed=seed)
    same_stats(st, st_p)
    assert not np.array_equal(RW.bits(plain), RW.bits(img))
    # samples cut over launches: the same image, moments and counts
    monkeypatch.setenv("PT_NEE_CHUNK", "2")
    cut, m, st_c = r.render_nee(cam, spp, depth, seed=seed, want=("sum", "sumsq", "sem"), mis=True)
    monkeypatch.delenv("PT_NEE_CHUNK")
    assert st_c["launches"] == 2
    assert np.array_equal(RW.bits(cut), RW.bits(img))
    assert all(np.array_equal(m[k], mom[k]) for k in ("sum", "sumsq")) and np.array_equal(RW.bits(m["sem"]), RW.bits(mom["sem"]))
    same_stats(st_c, st)


def test_default_mode_through_the_new_entry_points(renderers):
    """NULL options and PT_NEE_MIS_NONE through pt_ctx_trace_nee_opt and pt_ctx_render_nee_opt:
    the existing entry points' bits and stats."""
    import ptamd
    from ptamd import _lib
    L = ptamd.lib()
    name = "random_7_300"
    r, sc, _ = renderers(name)
    o, d = RT.rays(name, N)
    want, st_w = r.trace_nee(o, d, 5, samples=3, seed=7)
    prm = _lib.pt_trace_params(5, 3, 7, None)
    none = _lib.pt_nee_options(_lib.PT_NEE_MIS_NONE, (0, 0, 0))
    cam = ptamd.Camera.from_spec(sc.camera)
    W, H = sc.camera.res
    img_w, _, ist_w = r.render_nee(cam, 3, 5, seed=7)
    rp = _lib.pt_params(3, 5, 7, 0, 1, 1, 0, 0)
    for opt in (None, C.byref(none)):
        rgb = np.full((N, 3), -1.0, dtype=F32)
        st = _lib.pt_nee_stats()
        ptamd.check(L.pt_ctx_trace_nee_opt(r.h, o.ctypes.data, d.ctypes.data, N, C.byref(prm), rgb.ctypes.data, 0, C.byref(st), opt))
        RT.assert_same(rgb, want, "pt_ctx_trace_nee_opt, unweighted")
        same_stats(st.as_dict(), st_w)
        img = np.full((H, W, 3), -1.0, dtype=F32)
        ist = _lib.pt_nee_stats()
        ptamd.check(L.pt_ctx_render_nee_opt(r.h, C.byref(cam.c), C.byref(rp), img.ctypes.data, None, 0, C.byref(ist), opt))
        assert np.array_equal(RW.bits(img), RW.bits(img_w))
        same_stats(ist.as_dict(), ist_w)
    bad = _lib.pt_nee_options(3, (0, 0, 0))
    assert L.pt_ctx_trace_nee_opt(r.h, o.ctypes.data, d.ctypes.data, N, C.byref(prm), rgb.ctypes.data, 0, None,
                                  C.byref(bad)) == _lib.PT_E_ARG
