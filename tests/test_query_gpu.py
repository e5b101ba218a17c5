"""Ray queries and first-hit AOVs on the GPU (pt_query.hip through pt_ctx_intersect and
pt_ctx_render_aov), bit for bit against the oracle: tests/_refwalk.py restates BVH::intersect
(bvh.h:156-183) over the oracle's primitives, `_oracle.render` gives the depth-1 images."""
import numpy as np
import pytest

import _oracle as O
import _refwalk as RW

pytestmark = pytest.mark.gpu

SCENES = ["cornell", "random_3_40", "random_7_300", "sphere12"]
F32 = np.float32


@pytest.fixture(scope="module")
def renderers():
    """One context per scene name, scene uploaded; closed at the end of the module."""
    import ptamd
    made = {}

    def get(name, res=(16, 16)):
        key = (name, tuple(res))
        if key not in made:
            sc = RW.make_scene(name, res)
            r = ptamd.Renderer(0)
            r.set_scene(ptamd.BVH.from_scene(sc))
            made[key] = (r, sc)
        return made[key]

    yield get
    for r, _ in made.values():
        r.close()


def _same(t, tri, t_ref, tri_ref):
    bad = np.flatnonzero((RW.bits(t) != RW.bits(t_ref)) | (tri != tri_ref))
    assert bad.size == 0, f"{bad.size} rays differ, first {bad[:5]}: got {t[bad[:5]]} {tri[bad[:5]]}, " \
                          f"want {t_ref[bad[:5]]} {tri_ref[bad[:5]]}"


@pytest.mark.parametrize("name", SCENES)
def test_closest_hit_bitexact(renderers, name):
    import ptamd
    r, sc = renderers(name)
    if name == "sphere12":  # a scene that renders on the wide path still answers queries exactly
        assert ptamd.scene_info(ptamd.BVH.from_scene(sc))["wide_nodes"] > 0
    o, d, t_ref, tri_ref = RW.expected(name)
    full = o.shape[0]
    for n in (1, 63, 64, 65, 255, 256, 257, full):
        (t, tri), st = r.intersect(o[:n], d[:n])
        _same(t, tri, t_ref[:n], tri_ref[:n])
        assert st["rays"] == n and st["hits"] == int((tri_ref[:n] >= 0).sum()) and st["launches"] == 1
    if name == "cornell":
        assert st["lds_scene"] == 1 and st["lds_stack"] == 1


@pytest.mark.parametrize("name", ["cornell", "random_7_300"])
def test_closest_hit_nonfinite_rays(renderers, name):
    """inf and NaN in origins and directions: the exact slab form's answers, as the oracle's."""
    r, _ = renderers(name)
    o, d, t_ref, tri_ref = RW.expected_nonfinite(name)
    (t, tri), _ = r.intersect(o, d)
    _same(t, tri, t_ref, tri_ref)
    # mixed into a wave of ordinary rays (the wave then takes the exact form as a whole)
    o2, d2, t2, tri2 = RW.expected(name)
    om, dm = np.concatenate([o2[:40], o, o2[40:100]]), np.concatenate([d2[:40], d, d2[40:100]])
    (t, tri), _ = r.intersect(om, dm)
    _same(t, tri, np.concatenate([t2[:40], t_ref, t2[40:100]]), np.concatenate([tri2[:40], tri_ref, tri2[40:100]]))


PLACEMENTS = [("PT_LDS_SCENE_BYTES", "0", {"lds_scene": 0, "lds_stack": 1}),
              ("PT_LDS_SCENE_BYTES", "65536", {"lds_scene": 1, "lds_stack": 1}),
              ("PT_QUERY_LDS_STACK", "0", {"lds_stack": 0}),
              ("PT_FORCE_EXACT_SLAB", "1", {"lds_stack": 1})]


@pytest.mark.parametrize("hook,value,forced", PLACEMENTS)
@pytest.mark.parametrize("name", ["random_7_300", "random_3_40"])
def test_placement_variants(renderers, monkeypatch, name, hook, value, forced):
    """Scene and stack in LDS or not, and the exact slab form: the same bits. (52 triangles
    fit the default LDS scene budget, 312 do not: both defaults are covered.)"""
    r, _ = renderers(name)
    o, d, t_ref, tri_ref = RW.expected(name)
    (t0, tri0), st0 = r.intersect(o, d)
    assert st0["lds_stack"] == 1 and st0["lds_scene"] == (1 if name == "random_3_40" else 0)
    monkeypatch.setenv(hook, value)
    (t, tri), st = r.intersect(o, d)
    occ, st_any = r.intersect(o, d, any_hit=True)
    monkeypatch.delenv(hook)
    _same(t, tri, t0, tri0)
    _same(t, tri, t_ref, tri_ref)
    assert np.array_equal(occ, (tri_ref >= 0).astype(np.int32))
    for k, v in forced.items():
        assert st[k] == v and st_any[k] == v, (k, st, st_any)


@pytest.mark.parametrize("name", SCENES)
def test_any_hit(renderers, name):
    r, _ = renderers(name)
    o, d, t_ref, tri_ref = RW.expected(name)
    rng = np.random.default_rng(5)
    n = o.shape[0]
    pick = rng.integers(4, size=n)
    hit_choices = np.stack([F32(0.5) * t_ref, t_ref, np.nextafter(t_ref, F32(np.inf)), np.full(n, 1e30, F32)])
    miss_choices = np.stack([np.full(n, 1.0, F32), np.full(n, 1e30, F32)])
    tmax = np.where(tri_ref >= 0, hit_choices[pick, np.arange(n)], miss_choices[pick % 2, np.arange(n)]).astype(F32)
    want = (t_ref < tmax).astype(np.int32)
    assert 0 < want.sum() < (tri_ref >= 0).sum()
    occ, st = r.intersect(o, d, any_hit=True, tmax=tmax)
    assert occ.dtype == np.int32 and np.array_equal(occ, want)
    assert st["rays"] == n and st["hits"] == int(want.sum())
    occ, st = r.intersect(o, d, any_hit=True)  # NULL tmax = 1e30f
    assert np.array_equal(occ, (tri_ref >= 0).astype(np.int32))
    for m in (1, 65, 257):
        occ, _ = r.intersect(o[:m], d[:m], any_hit=True, tmax=tmax[:m])
        assert np.array_equal(occ, want[:m])


def test_device_pointers(renderers):
    import torch
    r, _ = renderers("random_7_300")
    o, d, t_ref, tri_ref = RW.expected("random_7_300")
    (t_h, tri_h), _ = r.intersect(o, d)
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev)
    out_t = torch.full((o.shape[0],), -1.0, dtype=torch.float32, device=dev)
    out_tri = torch.full((o.shape[0],), -7, dtype=torch.int32, device=dev)
    (rt, rtri), st = r.intersect(to, td, out=(out_t, out_tri))
    assert rt is out_t and rtri is out_tri and st["rays"] == o.shape[0]
    _same(out_t.cpu().numpy(), out_tri.cpu().numpy(), t_h, tri_h)
    _same(t_h, tri_h, t_ref, tri_ref)
    tmax = torch.from_numpy(np.where(tri_ref >= 0, t_ref, F32(1.0)).astype(F32)).to(dev)
    occ, _ = r.intersect(to, td, any_hit=True, tmax=tmax)
    assert occ.dtype == torch.int32 and not occ.cpu().numpy().any()  # t_ref < t_ref is false
    occ, _ = r.intersect(to, td, any_hit=True)
    assert np.array_equal(occ.cpu().numpy(), (tri_ref >= 0).astype(np.int32))
    assert np.array_equal(RW.bits(to.cpu().numpy()), RW.bits(o)) and np.array_equal(RW.bits(td.cpu().numpy()), RW.bits(d))


def _tiled(name, n, seed):
    """n rays drawn from the scene's 1024-ray set by seeded permutations laid end to end, with
    the known answers taken the same way (no new reference walks)."""
    o, d, t_ref, tri_ref = RW.expected(name)
    rng = np.random.default_rng(seed)
    m = o.shape[0]
    pick = np.concatenate([rng.permutation(m) for _ in range(-(-n // m))])[:n]
    return pick, np.take(o, pick, axis=0), np.take(d, pick, axis=0), np.take(t_ref, pick), np.take(tri_ref, pick)


def _tmax_for(t_ref, tri_ref):
    """test_any_hit's per-ray bounds for the base ray set."""
    n = t_ref.shape[0]
    pick = np.random.default_rng(5).integers(4, size=n)
    hit_choices = np.stack([F32(0.5) * t_ref, t_ref, np.nextafter(t_ref, F32(np.inf)), np.full(n, 1e30, F32)])
    miss_choices = np.stack([np.full(n, 1.0, F32), np.full(n, 1e30, F32)])
    return np.where(tri_ref >= 0, hit_choices[pick, np.arange(n)], miss_choices[pick % 2, np.arange(n)]).astype(F32)


def test_grid_stride_loop_runs_twice_on_device_pointers(renderers):
    """2^20 + 5 rays in one launch: more than the 8 blocks x 256 lanes per CU a launch can hold,
    so lanes take a second trip round the kernel's grid-stride loop; bits, ids and the hit
    counter against the tiled known answers."""
    import torch
    name = "random_3_40"
    r, _ = renderers(name)
    n = (1 << 20) + 5
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n > 8 * cus * 256
    _, o, d, t_ref, tri_ref = _tiled(name, n, 11)
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    (t, tri), st = r.intersect(to, td)
    assert st["rays"] == n and st["launches"] == 1 and st["hits"] == int((tri_ref >= 0).sum())
    _same(t.cpu().numpy(), tri.cpu().numpy(), t_ref, tri_ref)
    occ, st = r.intersect(to, td, any_hit=True)
    assert np.array_equal(occ.cpu().numpy(), (tri_ref >= 0).astype(np.int32)) and st["hits"] == int((tri_ref >= 0).sum())


def test_host_pointer_call_runs_two_chunks(renderers):
    """2^22 + 321 rays through host pointers: pt_ctx_intersect stages 2^22 at a time, so two
    launches; closest hit and any hit (per-ray tmax), the hit count summed over both, and the
    second chunk's 321 answers."""
    name = "cornell"
    r, _ = renderers(name)
    chunk = 1 << 22
    n = chunk + 321
    pick, o, d, t_ref, tri_ref = _tiled(name, n, 12)
    (t, tri), st = r.intersect(o, d)
    assert st["rays"] == n and st["launches"] == 2 and st["hits"] == int((tri_ref >= 0).sum())
    _same(t[chunk:], tri[chunk:], t_ref[chunk:], tri_ref[chunk:])
    _same(t, tri, t_ref, tri_ref)
    assert (tri_ref[chunk:] >= 0).any() and (tri_ref[chunk:] < 0).any()
    base = RW.expected(name)
    tmax = np.take(_tmax_for(base[2], base[3]), pick)
    want = (t_ref < tmax).astype(np.int32)
    occ, st = r.intersect(o, d, any_hit=True, tmax=tmax)
    assert st["launches"] == 2 and st["hits"] == int(want.sum()) and 0 < want[chunk:].sum() < 321
    assert np.array_equal(occ[chunk:], want[chunk:]) and np.array_equal(occ, want)


def _tri_normal(verts, tri, d):
    """Triangle::normal (triangle.h:45-49) in float32, linalg.h's operation order:
    edge1 x edge2, / length, then n . d < 0 ? n : -n."""
    v = verts[tri].astype(F32)
    e1, e2 = v[..., 3:6] - v[..., 0:3], v[..., 6:9] - v[..., 0:3]
    x1, y1, z1 = e1[..., 0], e1[..., 1], e1[..., 2]
    x2, y2, z2 = e2[..., 0], e2[..., 1], e2[..., 2]
    cx, cy, cz = y1 * z2 - z1 * y2, z1 * x2 - x1 * z2, x1 * y2 - y1 * x2
    ln = np.sqrt(cx * cx + cy * cy + cz * cz)
    n = np.stack([cx / ln, cy / ln, cz / ln], axis=-1)
    dot = n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1] + n[..., 2] * d[..., 2]
    return np.where((dot < 0)[..., None], n, -n).astype(F32)


@pytest.mark.parametrize("name,res", [("cornell", (32, 32)), ("random_3_40", (16, 16))])
def test_aov(renderers, name, res):
    import ptamd
    r, sc = renderers(name, res)
    cam = ptamd.Camera.from_spec(sc.camera)
    W, H = res
    a, st = r.aov(cam, sample=0)
    assert st["rays"] == W * H and st["hits"] == int((a["tri"] >= 0).sum())
    assert a["t"].shape == (H, W) and a["tri"].dtype == np.int32 and a["ray"].shape == (H, W, 6)
    # a depth-1 trace returns the first hit's emission (render.h:41-45)
    ref1, _ = O.render(sc, 1, 1)
    assert np.array_equal(RW.bits(a["emission"]), RW.bits(ref1))
    acc = a["emission"].copy()
    for s in (1, 2, 3):
        acc = acc + r.aov(cam, sample=s, channels=("emission",))[0]["emission"]
    ref4, _ = O.render(sc, 4, 1)
    assert np.array_equal(RW.bits(acc / F32(4)), RW.bits(ref4))
    # the ray channel, queried, gives the t and tri channels; and the oracle's walk agrees
    o, d = a["ray"][..., 0:3].reshape(-1, 3), a["ray"][..., 3:6].reshape(-1, 3)
    (t, tri), _ = r.intersect(o, d)
    _same(t, tri, a["t"].reshape(-1), a["tri"].reshape(-1))
    verts, nodes, idx = RW.oracle_bvh(name)
    _same(t, tri, *RW.ref_walk(nodes, idx, verts, o, d))
    hit = a["tri"] >= 0
    assert hit.any()
    assert np.array_equal(RW.bits(a["t"][~hit]), RW.bits(np.full((~hit).sum(), 1e30, F32)))
    _, _, mvals = O.pack_scene(sc)
    for ch, cols in (("albedo", slice(0, 3)), ("emission", slice(3, 6))):
        assert np.array_equal(RW.bits(a[ch][hit]), RW.bits(mvals[a["tri"][hit], cols]))
        assert not RW.bits(a[ch][~hit]).any()  # +0
    assert not RW.bits(a["normal"][~hit]).any()
    want_n = _tri_normal(verts, a["tri"][hit], a["ray"][..., 3:6][hit])
    assert np.array_equal(RW.bits(a["normal"][hit]), RW.bits(want_n))
    # three parts of bands of two rows reassemble the frame
    rows_of = [[h for h in range(H) if (h // 2) % 3 == p] for p in range(3)]
    for p in range(3):
        part, stp = r.aov(cam, sample=0, part_index=p, part_count=3, band_rows=2)
        assert stp["rays"] == len(rows_of[p]) * W
        for ch in a:
            assert part[ch].shape[0] == len(rows_of[p])
            assert np.array_equal(part[ch].view(np.uint32), a[ch][rows_of[p]].view(np.uint32)), (p, ch)


def test_queries_leave_progressive_sum(renderers):
    import ptamd
    r, sc = renderers("random_3_40", (16, 16))
    cam = ptamd.Camera.from_spec(sc.camera)
    o, d, t_ref, tri_ref = RW.expected("random_3_40")
    r.render_progressive(cam, 0, 2, 4)
    (t, tri), _ = r.intersect(o, d)
    _same(t, tri, t_ref, tri_ref)
    r.aov(cam, sample=1)
    img, _ = r.render_progressive(cam, 2, 2, 4)
    one_shot, _ = r.render(cam, 4, 4)
    assert np.array_equal(RW.bits(img), RW.bits(one_shot))
    ref, _ = O.render(sc, 4, 4)
    assert np.array_equal(RW.bits(img), RW.bits(ref))
