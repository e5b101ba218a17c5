"""Light sampling at extreme scales, on exact ties and at the light table's edges
(tests/_edgelights.py) on the GPU: pt_nee.hip through Renderer.trace_nee and Renderer.render_nee,
both estimators, bit for bit against the host form BVH.trace_nee (which
tests/test_edge_lights_cpu.py holds to the restatements, with the floors that keep these
comparisons from passing on empty pictures) and, once per member, against the restatement
itself. The scenes' own data drives what no hook reaches: shadow segments,
whose unnormalised direction the scene scales, through the wave guards of the exact reciprocal,
the per-ray domain of the fast slab form and the absolute EPS of the triangle test; areas that
overflow or absorb one another in the light table; visibility decided by the rank of a tie; draws
of exactly 1.0f and on a cdf entry; and caller rays with large and small finite directions on
every caller-ray kernel. Comparison rule: bits equal, or both NaN."""
import numpy as np
import pytest

import _edgelights as EL
import _edgescenes as E
import _reftrace as RT
import _refwalk as RW
from _plans import _planned
from test_edge_scenes_gpu import _same, _tmax_for
from test_nee_gpu import NEE_KEYS, PLACEMENTS, _camera_samples

pytestmark = pytest.mark.gpu

F32 = np.float32
QRES = (16, 12)
MIS = [False, True]
MIS_IDS = ["plain", "mis"]


@pytest.fixture(scope="module")
def contexts():
    """One context per member (or base), scene uploaded; closed at the end of the module. None of
    these tests renders with the flat kernels, so the scene-specialised one is not compiled."""
    import ptamd
    if ptamd.lib().pt_device_count() <= 0:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    made = {}

    def get(member):
        if member not in made:
            sc = E.make(member, QRES)
            bvh = ptamd.BVH.from_scene(sc)
            r = ptamd.Renderer(0)
            with pytest.MonkeyPatch.context() as m:
                m.setenv("PT_RTC", "0")
                r.set_scene(bvh)
            made[member] = (r, sc, bvh)
        return made[member]

    yield get
    for r, _, _ in made.values():
        r.close()


def same_stats(a, b):
    assert {k: a[k] for k in NEE_KEYS} == {k: b[k] for k in NEE_KEYS}, (a, b)


@pytest.mark.parametrize("mis", MIS, ids=MIS_IDS)
@pytest.mark.parametrize("member", EL.LIGHT_MEMBERS)
def test_trace_nee_matches_host(contexts, member, mis):
    r, _, bvh = contexts(member)
    o, d = E.query_rays(member)
    n = o.shape[0]
    assert n % 64 != 0
    for depth in EL.DEPTHS:
        for samples in EL.SAMPLES:
            host, st_h = bvh.trace_nee(o, d, depth, samples=samples, seed=EL.SEED, mis=mis)
            got, st = r.trace_nee(o, d, depth, samples=samples, seed=EL.SEED, mis=mis)
            RT.assert_same(got, host, f"{member} depth {depth} samples {samples} mis {mis}")
            same_stats(st, st_h)
            assert st["launches"] == 1 and st["paths"] == n * samples
    # one depth against the restatement itself
    want, segs, sh, dr = EL.expected(member, mis, 5, 1)
    got, st = r.trace_nee(o, d, 5, seed=EL.SEED, mis=mis)
    RT.assert_same(got, want, f"{member} mis {mis}: GPU vs restatement")
    assert st["rays"] == segs and st["shadow_rays"] == sh and st["light_draws"] == dr
    assert st["lights"] == EL.lights(member).tri.size
    # the far and threshold rays alone: waves whose lanes are all outside the fast domain
    fo, fd = np.ascontiguousarray(o[E.N_NEAR:]), np.ascontiguousarray(d[E.N_NEAR:])
    host, st_h = bvh.trace_nee(fo, fd, 5, samples=3, seed=EL.SEED, mis=mis)
    got, st = r.trace_nee(fo, fd, 5, samples=3, seed=EL.SEED, mis=mis)
    RT.assert_same(got, host, f"{member} mis {mis} (far rays)")
    same_stats(st, st_h)


@pytest.mark.parametrize("mis", MIS, ids=MIS_IDS)
@pytest.mark.parametrize("hook,value,rule", PLACEMENTS)
@pytest.mark.parametrize("member", EL.PLACEMENT_MEMBERS)
def test_placement_variants(contexts, monkeypatch, member, hook, value, rule, mis):
    """Scene and stack in LDS or not, and the exact slab form: the host's bits, and the stats say
    which form ran, by the placement rule of the binary walk (tests/_plans.py)."""
    import ptamd
    r, sc, bvh = contexts(member)
    info = ptamd.scene_info(bvh)
    flags = ("lds_scene", "lds_stack")
    o, d = E.query_rays(member)
    want, st_h = bvh.trace_nee(o, d, 5, seed=EL.SEED, mis=mis)
    got0, st0 = r.trace_nee(o, d, 5, seed=EL.SEED, mis=mis)
    assert {k: st0[k] for k in flags} == {k: _planned(info, len(sc.tris), 5)[k] for k in flags}
    monkeypatch.setenv(hook, value)
    got, st = r.trace_nee(o, d, 5, seed=EL.SEED, mis=mis)
    monkeypatch.delenv(hook)
    RT.assert_same(got, want, f"{member} {hook}={value}")
    RT.assert_same(got0, want, f"{member} default")
    same_stats(st, st_h)
    same_stats(st0, st_h)
    forced = _planned(info, len(sc.tris), 5, **rule)
    assert {k: st[k] for k in flags} == {k: forced[k] for k in flags}, (st, forced)
    if hook == "PT_LDS_SCENE_BYTES" and value == "0":
        assert st["lds_scene"] == 0
    if hook == "PT_QUERY_LDS_STACK":
        assert st["lds_stack"] == 0


@pytest.mark.parametrize("mis", MIS, ids=MIS_IDS)
@pytest.mark.parametrize("kind", ["edge", "tie"])
@pytest.mark.parametrize("member", EL.STATE_MEMBERS_GPU)
def test_crafted_states(contexts, member, kind, mis):
    """First light draws of exactly 1.0f (xa == A: the last light; x2 + x3 > 1: the fold), of 0
    and 2^-32, and with xa on a cdf entry and one float below it."""
    r, _, bvh = contexts(member)
    o, d, states = EL.state_rays(member, kind)
    for depth in EL.DEPTHS:
        host, st_h = bvh.trace_nee(o, d, depth, states=states, mis=mis)
        got, st = r.trace_nee(o, d, depth, states=states, mis=mis)
        RT.assert_same(got, host, f"{member} {kind} depth {depth} mis {mis}")
        same_stats(st, st_h)
    assert st["shadow_rays"] > 0 and EL.lit_rays(got) > 0


@pytest.mark.parametrize("mis", MIS, ids=MIS_IDS)
@pytest.mark.parametrize("member", EL.RENDER_MEMBERS)
def test_render_nee_is_trace_nee_on_the_camera_rays(contexts, monkeypatch, member, mis):
    import ptamd
    r, sc, _ = contexts(member)
    cam = ptamd.Camera.from_spec(sc.camera)
    W, H = sc.camera.res
    spp, depth, seed = 3, 5, 9
    acc = np.zeros((W * H, 3), dtype=F32)
    S = np.zeros((W * H, 3), dtype=np.float64)
    Q = np.zeros((W * H, 3), dtype=np.float64)
    tot = dict.fromkeys(("rays", "shadow_rays", "light_draws"), 0)
    with np.errstate(all="ignore"):
        for o, d, st in _camera_samples(r, cam, W, H, spp, seed):
            x, s1 = r.trace_nee(o, d, depth, states=st, mis=mis)
            acc = acc + x
            S = S + x.astype(np.float64)
            Q = Q + x.astype(np.float64) * x.astype(np.float64)
            for k in tot:
                tot[k] += s1[k]
        want = (acc / F32(spp)).astype(F32)
        var = np.maximum(0.0, (Q - S * S / spp) / (spp - 1.0))
        sem = np.sqrt(var / spp).astype(F32)
    img, mom, st = r.render_nee(cam, spp, depth, seed=seed, want=("sum", "sumsq", "sem"), mis=mis)
    assert img.shape == (H, W, 3) and RW.bits(img).any()
    RT.assert_same(img.reshape(-1, 3), want, f"{member}: render_nee vs trace_nee on the AOV rays")
    assert np.array_equal(mom["sum"].reshape(-1, 3), S) and np.array_equal(mom["sumsq"].reshape(-1, 3), Q)
    assert np.array_equal(RW.bits(mom["sem"].reshape(-1, 3)), RW.bits(sem))
    assert {k: st[k] for k in tot} == tot and st["shadow_rays"] > 0
    assert st["paths"] == W * H * spp and st["launches"] == 1 and st["lights"] == s1["lights"]
    # samples cut over two launches: the same image, moments and counts
    monkeypatch.setenv("PT_NEE_CHUNK", "2")
    cut, m, st_c = r.render_nee(cam, spp, depth, seed=seed, want=("sum", "sumsq", "sem"), mis=mis)
    monkeypatch.delenv("PT_NEE_CHUNK")
    assert st_c["launches"] == 2
    assert np.array_equal(RW.bits(cut), RW.bits(img))
    assert all(np.array_equal(m[k], mom[k]) for k in ("sum", "sumsq")) and np.array_equal(RW.bits(m["sem"]), RW.bits(mom["sem"]))
    same_stats(st_c, st)


@pytest.mark.parametrize("exact_slab", [False, True], ids=["default", "exact_slab"])
@pytest.mark.parametrize("base", EL.LIGHT_BASES)
def test_big_directions_on_every_caller_ray_kernel(contexts, monkeypatch, base, exact_slab):
    """Directions times 2^e, e in ±61 .. ±126, whole or in one component (|1 / d| on both sides of
    2^60 and of 2^-100, |d| on both sides of 2^±126) through the query kernels (closest hit and
    any hit) against the restated walk, and through trace and both forms of trace_nee against the
    host forms; once more with the exact slab form forced."""
    r, _, bvh = contexts(base)
    o, d, _ = EL.big_dir_rays(base)
    t_ref, tri_ref = EL.big_dir_expected(base)
    n, hits = o.shape[0], int((tri_ref >= 0).sum())
    assert hits >= n // 4
    if exact_slab:
        monkeypatch.setenv("PT_FORCE_EXACT_SLAB", "1")
    (t, tri), st = r.intersect(o, d)
    _same(t, tri, t_ref, tri_ref, base)
    assert st["rays"] == n and st["hits"] == hits
    tmax = _tmax_for(t_ref, tri_ref)
    want = (t_ref < tmax).astype(np.int32)
    assert 0 < want.sum() < hits
    occ, st = r.intersect(o, d, any_hit=True, tmax=tmax)
    assert np.array_equal(occ, want), (base, np.flatnonzero(occ != want)[:8])
    assert st["hits"] == int(want.sum())
    occ, st = r.intersect(o, d, any_hit=True)
    assert np.array_equal(occ, (tri_ref >= 0).astype(np.int32)) and st["hits"] == hits
    host, st_h = bvh.trace(o, d, 5, seed=EL.SEED)
    got, st = r.trace(o, d, 5, seed=EL.SEED)
    RT.assert_same(got, host, f"{base}: trace")
    assert st["rays"] == st_h["rays"] and st["paths"] == n
    for mis in MIS:
        host, st_h = bvh.trace_nee(o, d, 5, seed=EL.SEED, mis=mis)
        got, st = r.trace_nee(o, d, 5, seed=EL.SEED, mis=mis)
        RT.assert_same(got, host, f"{base}: trace_nee mis {mis}")
        same_stats(st, st_h)
        assert st["shadow_rays"] > 0 and EL.lit_rays(got) > 0
