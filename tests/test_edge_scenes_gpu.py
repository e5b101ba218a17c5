"""Scenes at extreme coordinate scales and with exact ties (tests/_edgescenes.py) on the GPU: every
family member rendered on every kernel path that takes it, and ray queries, AOVs and caller rays
on a subset, bit for bit against the oracle and the restated walks. The scenes' own data flips
the gates that the other tests reach only through hooks: coords_small (a
coordinate >= 2^60), the per-ray domain tests (origins and 1 / d across 2^60 and 2^64), the
absolute EPS and miss thresholds of the triangle test (scaled scenes) and the rank of a tie
(doubled scenes). tests/test_edge_scenes_cpu.py holds the floors that keep these comparisons from
passing on an empty picture. Comparison rule: bits equal, or both NaN."""
import numpy as np
import pytest

import _edgescenes as E
import _oracle as O
import _reftrace as RT
import _refwalk as RW

pytestmark = pytest.mark.gpu

F32 = np.float32
RES, SPP, DEPTH = (26, 21), 3, 5
FLAT_RTC, FLAT_TABLE, FLAT_TABLE_FAST, WIDE, TREE = 3, 2, 5, 4, (0, 1)  # PT_PATH_* (include/pt_hip.h)


@pytest.fixture(scope="module")
def ptamd_mod():
    import ptamd
    if ptamd.lib().pt_device_count() <= 0:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    return ptamd


def _bits_equal_nan(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _render(ptamd, monkeypatch, bvh, cam, env):
    """One render on a context of its own under `env`: (image, stats, context flags)."""
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        r = ptamd.Renderer(0)
        try:
            r.set_scene(bvh)
            img, st = r.render(cam, SPP, DEPTH)
            return img, st, r.flags()
        finally:
            r.close()


def _paths_wanted(ptamd, member, bvh):
    """[(env, allowed kernel paths or None = decided from the scene kernel's flags)] for a member."""
    info = ptamd.scene_info(bvh)
    wide = info["wide_nodes"] > 0
    assert wide != E.one_leaf(member)
    off_flat = (WIDE,) if wide else TREE
    if 0 < info["flat_leaves"] <= 64:
        envs = [({"PT_RTC_WAIT": "1"}, (FLAT_RTC,)), ({"PT_RTC": "0"}, None),
                ({"PT_RTC": "0", "PT_FLAT_FAST": "0"}, (FLAT_TABLE,)), ({"PT_FLAT": "0"}, off_flat),
                ({"PT_FLAT": "0", "PT_WIDE": "0"}, TREE)]
        if E.parse(member)[1] == "far_camera":  # the scene kernel's sign-bit box mask (its domain: |o| < 2^60)
            envs.append(({"PT_RTC_WAIT": "1", "PT_RTC_DEFINES": "PT_FLAT_SIGN_MASK=1"}, (FLAT_RTC,)))
        return envs
    assert wide
    return [({}, (WIDE,)), ({"PT_FLAT": "0"}, (WIDE,)), ({"PT_WIDE": "1"}, (WIDE,)), ({"PT_FLAT": "0", "PT_WIDE": "0"}, TREE)]


@pytest.mark.parametrize("member", E.MEMBERS)
def test_render_bitexact_on_every_path(ptamd_mod, monkeypatch, member):
    sc = E.make(member, RES)
    ref, rays = O.render(sc, SPP, DEPTH)
    bvh = ptamd_mod.BVH.from_scene(sc)
    bvh.build()
    cam = ptamd_mod.Camera.from_spec(sc.camera)
    single = bool((bvh.nodes["tri_start"] == bvh.nodes["tri_end"])[bvh.nodes["left"] == -1].all())
    fast_ok = None
    seen = []
    for env, paths in _paths_wanted(ptamd_mod, member, bvh):
        img, st, flags = _render(ptamd_mod, monkeypatch, bvh, cam, env)
        if env == {"PT_RTC_WAIT": "1"}:
            assert flags["rtc"]
            # the offline table kernel with the scene's flags (pt_flat_fast.hip) takes the scenes
            # BVH::build makes with small coordinates, dark and with the pre-doubled albedo
            fast_ok = (not E.coords_big(member)) and single and flags["dark"] and flags["albedo_x2"]
        if paths is None:
            paths = (FLAT_TABLE_FAST,) if fast_ok else (FLAT_TABLE,)
            if E.coords_big(member) or not single:
                assert st["kernel_path"] == FLAT_TABLE, (member, env, st["kernel_path"])
        assert st["kernel_path"] in paths, (member, env, st["kernel_path"], paths)
        seen.append(st["kernel_path"])
        assert _bits_equal_nan(img, ref), (member, env, int((~RT.same_bits(img, ref)).reshape(-1, 3).any(axis=1).sum()))
        assert st["rays"] == rays, (member, env, st["rays"], rays)
    print(member, "kernel paths", seen, "lit", round(E.lit_share(ref), 3), "rays", rays)


@pytest.mark.parametrize("member", [m for m in E.MEMBERS if E.parse(m)[1] == "doubled" and E.parse(m)[0] in E.FLAT_BASES])
@pytest.mark.parametrize("env", [{"PT_BOX_PAIRS": "1"}, {"PT_BOX_PAIRS": "1", "PT_PAIR_QUEUE": "16"},
                                 {"PT_PAIR_QUEUE": "16"}, {"PT_PAIRS": "0"}])
def test_ties_in_pair_rounds_and_overflow_loops(ptamd_mod, monkeypatch, member, env):
    """Two triangles that tie bit for bit with different materials: the pair rounds' atomic min on
    (t, rank), the per-lane loops of a queue overflow and the loops without queues pick the
    lower rank, with and without box-level pairs."""
    sc = E.make(member, RES)
    ref, rays = O.render(sc, SPP, DEPTH)
    bvh = ptamd_mod.BVH.from_scene(sc)
    cam = ptamd_mod.Camera.from_spec(sc.camera)
    img, st, _ = _render(ptamd_mod, monkeypatch, bvh, cam, dict(env, PT_RTC_WAIT="1"))
    assert st["kernel_path"] == FLAT_RTC
    assert _bits_equal_nan(img, ref) and st["rays"] == rays, (member, env)


# ---------------------------------------------------------------- queries, AOVs and caller rays
QRES = (16, 12)


@pytest.fixture(scope="module")
def contexts(ptamd_mod):
    """One context per member, scene uploaded; closed at the end of the module."""
    made = {}

    def get(member):
        if member not in made:
            sc = E.make(member, QRES)
            bvh = ptamd_mod.BVH.from_scene(sc)
            r = ptamd_mod.Renderer(0)
            r.set_scene(bvh)
            made[member] = (r, sc, bvh)
        return made[member]

    yield get
    for r, _, _ in made.values():
        r.close()


def _same(t, tri, t_ref, tri_ref, what):
    bad = np.flatnonzero((RW.bits(t) != RW.bits(t_ref)) | (tri != tri_ref))
    assert bad.size == 0, f"{what}: {bad.size} rays differ, first {bad[:5]}: got {t[bad[:5]]} {tri[bad[:5]]}, " \
                          f"want {t_ref[bad[:5]]} {tri_ref[bad[:5]]}"


def _tmax_for(t_ref, tri_ref):
    """tests/test_query_gpu.py's per-ray bounds: half the hit distance, the distance itself, the
    next float up or 1e30 for a hit; 1 or 1e30 for a miss."""
    n = t_ref.shape[0]
    pick = np.random.default_rng(5).integers(4, size=n)
    hit_choices = np.stack([F32(0.5) * t_ref, t_ref, np.nextafter(t_ref, F32(np.inf)), np.full(n, 1e30, F32)])
    miss_choices = np.stack([np.full(n, 1.0, F32), np.full(n, 1e30, F32)])
    return np.where(tri_ref >= 0, hit_choices[pick, np.arange(n)], miss_choices[pick % 2, np.arange(n)]).astype(F32)


@pytest.mark.parametrize("member", E.QUERY_MEMBERS)
def test_intersect_bitexact(contexts, member):
    r, _, _ = contexts(member)
    o, d, t_ref, tri_ref = E.query_expected(member)
    n = o.shape[0]
    hits = int((tri_ref >= 0).sum())
    (t, tri), st = r.intersect(o, d)
    _same(t, tri, t_ref, tri_ref, member)
    assert st["rays"] == n and st["hits"] == hits and st["launches"] == 1
    tmax = _tmax_for(t_ref, tri_ref)
    want = (t_ref < tmax).astype(np.int32)
    if hits:
        assert 0 < want.sum() < hits
    occ, st = r.intersect(o, d, any_hit=True, tmax=tmax)
    assert occ.dtype == np.int32 and np.array_equal(occ, want), (member, np.flatnonzero(occ != want)[:8])
    assert st["rays"] == n and st["hits"] == int(want.sum())
    occ, st = r.intersect(o, d, any_hit=True)  # NULL tmax = 1e30f
    assert np.array_equal(occ, (tri_ref >= 0).astype(np.int32)) and st["hits"] == hits
    # the far rays alone: waves whose lanes are all outside the domain
    far = slice(E.N_NEAR, E.N_NEAR + E.N_FAR)
    (t, tri), _ = r.intersect(o[far], d[far])
    _same(t, tri, t_ref[far], tri_ref[far], member + " (far rays)")


@pytest.mark.parametrize("member", E.QUERY_MEMBERS)
def test_aov_triangle_and_depth(ptamd_mod, contexts, member):
    r, sc, _ = contexts(member)
    _, verts, _, _, nodes, idx = E.arrays(member, QRES)
    cam = ptamd_mod.Camera.from_spec(sc.camera)
    W, H = QRES
    o, d, _ = RT.camera_rays(sc, 1)
    t_ref, tri_ref = RW.ref_walk(nodes, idx, verts, o, d)
    a, st = r.aov(cam, sample=0, channels=("t", "tri", "ray"))
    assert np.array_equal(RW.bits(a["ray"][..., 0:3].reshape(-1, 3)), RW.bits(o))
    assert np.array_equal(RW.bits(a["ray"][..., 3:6].reshape(-1, 3)), RW.bits(d))
    _same(a["t"].reshape(-1), a["tri"].reshape(-1), t_ref, tri_ref, member)
    assert st["rays"] == W * H and st["hits"] == int((tri_ref >= 0).sum())
    print(member, "first-hit rate", round(float((tri_ref >= 0).mean()), 3))


@pytest.mark.parametrize("member", E.QUERY_MEMBERS)
def test_trace_caller_rays_bitexact(contexts, member):
    r, _, bvh = contexts(member)
    o, d = E.query_rays(member)
    n = o.shape[0]
    for depth, samples in ((5, 1), (8, 1), (5, 3), (8, 3)):
        want, st_h = bvh.trace(o, d, depth, samples=samples, seed=3)
        got, st = r.trace(o, d, depth, samples=samples, seed=3)
        RT.assert_same(got, want, f"{member} depth {depth} samples {samples}")
        assert st["launches"] == 1 and st["rays"] == st_h["rays"] and st["paths"] == n * samples
        assert st["rays"] >= n * samples  # every path traces its first segment
    if E.parse(member)[2][0] != "51":
        assert (RW.bits(want) != 0).any(axis=1).sum() > 0
