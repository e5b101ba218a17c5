"""Light sampling at extreme scales, on exact ties and at the light table's edges
(tests/_edgelights.py) on the host: pt_scene_lights against the restated table, BVH.trace_nee
(both estimators) against tests/_refnee.py and tests/_refmis.py bit for bit, crafted LCG states,
large and small finite directions through BVH.intersect, trace and trace_nee, and the floors that
keep these comparisons, and those of tests/test_edge_lights_gpu.py, from passing on empty
pictures. Comparison rule: bits equal, or both NaN."""
import functools

import numpy as np
import pytest

import _edgelights as EL
import _edgescenes as E
import _refmis as RM
import _refnee as RN
import _reftrace as RT
import _refwalk as RW

F32 = np.float32
RES = (16, 12)
MIS = [False, True]
MIS_IDS = ["plain", "mis"]


@functools.lru_cache(maxsize=None)
def _bvh(member):
    import ptamd
    b = ptamd.BVH.from_scene(E.make(member, RES))
    b.build()
    return b


def _bits1(x):
    return int(RW.bits(np.array([x], dtype=F32))[0])


def _same_stats(st, segs, sh, dr, lt, what):
    assert st["rays"] == segs and st["shadow_rays"] == sh and st["light_draws"] == dr, (what, st, segs, sh, dr)
    assert st["lights"] == lt.tri.size and _bits1(st["light_area"]) == _bits1(lt.area), (what, st)


# ---------------------------------------------------------------- the light table
@pytest.mark.parametrize("member", EL.LIGHT_MEMBERS)
def test_scene_lights_matches_restatement(member):
    """Count, triangle indices and the bits of cdf and A. kA = A / (float)M_PI is no output of
    pt_scene_lights; it is a function of A alone, and every light term of the walks below is a
    multiple of it. The host's tree is the oracle's, so the walks below compare like with like."""
    import ptamd
    want = EL.lights(member)
    got = ptamd.scene_lights(_bvh(member))
    assert got["tri"].dtype == np.int32 and got["cdf"].dtype == np.float32
    assert got["tri"].size == want.tri.size and np.array_equal(got["tri"], want.tri)
    assert np.array_equal(RW.bits(got["cdf"]), RW.bits(want.cdf))
    assert _bits1(got["area"]) == _bits1(want.area)
    assert _bits1(want.kA) == _bits1(F32(got["area"]) / F32(np.pi))
    assert np.isfinite(want.cdf).all() and (want.tri.size == 0 or want.area == want.cdf[-1])
    _, _, _, _, nodes, idx = E.arrays(member)
    b = _bvh(member)
    assert b.nodes.tobytes() == nodes.tobytes() and b.tri_idx.tobytes() == idx.tobytes()


def test_light_table_floors():
    """What the restated tables show (areas are 0.5 sqrt(dot(c, c)), so dot(c, c) overflows long
    before the coordinates do):
    * Cornell's two lights (A = 13650 at scale 1) are listed up to 2^25 and gone at 2^26;
      random_4_150 keeps 12 of its 24 at 2^26 (a partial table) and none at 2^33;
    * degenerate lists one light more than its base: the sliver (the point and the segment have
      area 0);
    * far_light lists one more light at every k (its area, 5000, does not depend on z);
    * far_light_big/62 (sides 2^52: dot(c, c) = 2^208 overflows) lists the base's lights only;
    * far_light_big/30 (area 2^39, ulp 2^16) is listed last, after the base's lights, so no two
      cdf entries are equal: the base's entries are the base's own bit for bit, and the base's
      whole area is absorbed in or rounded into the last one, A = F32(A_base + 2^39): exactly 2^39
      on Cornell (13650 < 2^15), 2^39 + 2^16 on random_4_150 (69418 > 2^15). A base light is drawn
      only by x1 < A_base / 2^39 < 2^-22."""
    for base, n0 in (("cornell", 2), ("random_4_150", 24)):
        lt0 = EL.lights(base)
        assert lt0.tri.size == n0
        size = lambda m: EL.lights(f"{base}/{m}").tri.size  # noqa: E731
        assert size("scaled/25") == n0 and size("scaled/-12") == n0
        assert size("degenerate") == n0 + 1
        assert EL.lights(f"{base}/degenerate").tri[-1] == len(E.arrays(base)[0].tris) + 2  # the sliver
        for k in (40, 63, 65, 100, 110, 120):
            lt = EL.lights(f"{base}/far_light/{k}")
            assert lt.tri.size == n0 + 1 and lt.area == F32(lt0.area + F32(5000))
        lt = EL.lights(f"{base}/far_light_big/62")
        assert np.array_equal(lt.tri, lt0.tri) and np.array_equal(RW.bits(lt.cdf), RW.bits(lt0.cdf))
        lt = EL.lights(f"{base}/far_light_big/30")
        assert lt.tri.size == n0 + 1 and np.array_equal(RW.bits(lt.cdf[:-1]), RW.bits(lt0.cdf))
        assert (np.diff(lt.cdf) > 0).all()
        assert lt.area == F32(lt0.area + F32(2.0 ** 39))
        assert lt.area == F32(2.0 ** 39 + (0 if base == "cornell" else 2.0 ** 16))
    assert EL.lights("cornell/scaled/26").tri.size == 0 and EL.lights("cornell/scaled/24").tri.size == 2
    assert 0 < EL.lights("random_4_150/scaled/26").tri.size < 24
    assert EL.lights("random_4_150/scaled/33").tri.size == 0
    # from 2^100 the builder's SAH costs overflow: one root leaf holds every triangle
    for base in EL.LIGHT_BASES:
        assert [E.arrays(f"{base}/far_light/{k}")[4].shape[0] == 1 for k in (65, 100, 110, 120)] == [False, True, True, True]


# ---------------------------------------------------------------- the host form on the query rays
@pytest.mark.parametrize("mis", MIS, ids=MIS_IDS)
@pytest.mark.parametrize("member", EL.LIGHT_MEMBERS)
def test_host_trace_nee_matches_restatement(member, mis):
    o, d = E.query_rays(member)
    lt = EL.lights(member)
    b = _bvh(member)
    for depth in EL.DEPTHS:
        for samples in EL.SAMPLES:
            want, segs, sh, dr = EL.expected(member, mis, depth, samples)
            got, st = b.trace_nee(o, d, depth, samples=samples, seed=EL.SEED, mis=mis)
            RT.assert_same(got, want, f"{member} depth {depth} samples {samples} mis {mis}")
            _same_stats(st, segs, sh, dr, lt, (member, depth, samples))
            assert st["paths"] == o.shape[0] * samples and st["runaway"] == 0
    # floors (depth 5, 3 samples), from the restatement's own counts
    if lt.tri.size:
        assert dr > 0, member
    else:
        assert dr == 0 and sh == 0
    if not EL.dim(member):
        assert sh > 0, member
        plain, _ = b.trace(o, d, 5, samples=1, seed=EL.SEED)
        one = EL.expected(member, mis, 5, 1)[0]
        assert (~RT.same_bits(one, plain).all(axis=1)).any(), member
        # the weights change a value (not asked of the doubled scenes: where a light's twin wins
        # the tie, no light is ever visible and both estimators add the same terms)
        if mis and E.parse(member)[1] != "doubled":
            assert (~RT.same_bits(one, EL.expected(member, False, 5, 1)[0]).all(axis=1)).any(), member
    assert EL.lit_rays(want) > 0, member


def test_family_floors():
    """doubled/base and doubled/alt differ (the rank of a tie decides which twin is seen); on
    Cornell the far light's term changes a ray between k = 40 and k = 65 (as r2 grows the term
    shrinks to a denormal, then to 0), and from k = 65 to k = 120 the number of lit rays stays."""
    for mis in MIS:
        for base in EL.LIGHT_BASES:
            a, b = (EL.expected(f"{base}/doubled/{f}", mis, 5, 1)[0] for f in ("base", "alt"))
            assert (~RT.same_bits(a, b).all(axis=1)).any()
    # the far_light members share their rays only where the member names are equally long
    assert len("cornell/far_light/40") == len("cornell/far_light/65")
    o, d = E.query_rays("cornell/far_light/40")
    st = EL.seeds(o.shape[0])[:, 0]
    for mis in MIS:
        P = {k: EL._walk(f"cornell/far_light/{k}", mis, o, d, st, 5) for k in (40, 65, 120)}
        v = {k: EL.radiance(P[k], 5)[0] for k in P}
        assert (~RT.same_bits(v[40], v[65]).all(axis=1)).any()
        assert EL.lit_rays(v[65]) == EL.lit_rays(v[120]) > 0


# ---------------------------------------------------------------- crafted states
def test_lcg_edges():
    """oracle_lcg's draws at the crafted states: 1.0f from 0xFFFFFF80 up, below 1 before, 0 at 0."""
    assert EL.one_edge() == 0xFFFFFF80
    st, cls, tgt = EL.edge_states(60)
    s, x = EL.draws(st, 3)
    own = x[np.arange(60), cls]
    assert (own[tgt >= 0xFFFFFF80] == F32(1)).all() and (own[tgt == 0xFFFFFF7F] < F32(1)).all()
    assert (own[tgt == 0] == 0).all() and (own[tgt == 1] == F32(2.0 ** -32)).all()
    assert {(int(c), int(t)) for c, t in zip(cls, tgt)} == {(c, t) for c in range(3) for t in
                                                           (0xFFFFFFFF, 0xFFFFFF80, 0xFFFFFF7F, 0, 1)}
    # the issue's examples
    assert np.array_equal(EL.draws([0x26f5b720, 0x93defb85, 0xa143553e], 3)[1].diagonal(), np.ones(3, F32))
    assert np.array_equal(EL.lcg_prev(RT.lcg_step(st, 3), 3), st)


def test_cdf_ties_exist():
    found = EL.cdf_tie_states(EL.lights("random_4_150"), EL.N_STATE_RAYS)
    assert found is not None
    st, j, side = found
    assert np.unique(j).size >= 12 and (side == 0).sum() >= EL.N_STATE_RAYS // 4 and (side == 1).any()
    # a tie passes cdf[j] over (the compare is strict); the float below picks j
    lt = EL.lights("random_4_150")
    xa, _, _ = EL.first_draw(lt, st)
    pick = np.minimum(np.searchsorted(lt.cdf, xa, side="right"), lt.tri.size - 1)
    assert np.array_equal(pick, j + (side == 0))


@pytest.mark.parametrize("mis", MIS, ids=MIS_IDS)
@pytest.mark.parametrize("kind", ["edge", "tie"])
@pytest.mark.parametrize("member", EL.STATE_MEMBERS_CPU)
def test_crafted_states(member, kind, mis):
    """Floors, from the restatement's records and oracle_lcg alone: among the paths that made
    their first light draw at the first vertex, every draw class has some; class 0 (x1 = 1.0f, so
    xa = A) has paths that pick the last light because no cdf_j > xa; classes 1 and 2 (x2 or
    x3 = 1.0f) have paths that fold (u, v); the tie states have paths on both sides of a cdf
    entry. The wave of a first vertex that draws walks a shadow segment somewhere."""
    o, d, states = EL.state_rays(member, kind)
    P = EL.state_paths(member, kind, mis)
    lt = EL.lights(member)
    b = _bvh(member)
    for depth in EL.DEPTHS:
        want, segs, sh, dr = EL.radiance(P, depth)
        got, st = b.trace_nee(o, d, depth, states=states, mis=mis)
        RT.assert_same(got, want, f"{member} {kind} depth {depth} mis {mis}")
        _same_stats(st, int(segs.sum()), int(sh.sum()), int(dr.sum()), lt, (member, kind, depth))
    drew = P.drew[0]
    assert drew.sum() >= EL.N_STATE_RAYS // 2 and P.shadow[0].any() and EL.lit_rays(want) > 0
    xa, last, folded = EL.first_draw(lt, states)
    if kind == "edge":
        _, cls, tgt = EL.edge_states(EL.N_STATE_RAYS)
        ones = tgt >= EL.one_edge()
        assert (drew & (cls == 0) & ones & last).any() and (RW.bits(xa[(cls == 0) & ones]) == _bits1(lt.area)).all()
        assert not last[(cls == 0) & ~ones].any()
        for c in (1, 2):
            assert (drew & (cls == c) & ones & folded).any() and (drew & (cls == c) & ~ones & ~folded).any()
    else:
        _, j, side = EL.cdf_tie_states(lt, EL.N_STATE_RAYS)
        assert (drew & (side == 0)).any() and (drew & (side == 1)).any() and not last[side == 1].any()


# ---------------------------------------------------------------- large and small finite directions
@pytest.mark.parametrize("base", EL.LIGHT_BASES)
def test_big_directions(base):
    """Directions times 2^e, e in ±61 .. ±126, whole or in one component: BVH.intersect against
    the restated walk, BVH.trace and both forms of BVH.trace_nee against their restatements at
    depth 5. Floor: at least a quarter of the rays hit (t scales by 2^-e: the negative exponents
    from -101 down push t past 1e30, and |a| of the triangle test under its absolute EPS)."""
    o, d, e = EL.big_dir_rays(base)
    with np.errstate(all="ignore"):
        inv = np.abs(F32(1) / d)
    for bound in (F32(2.0 ** 60), F32(2.0 ** -100)):
        assert (inv.max(axis=1) > bound).any() and (inv.min(axis=1) < bound).any()
    assert (np.abs(d) >= F32(2.0 ** 126)).any() and (np.abs(d)[d != 0] <= F32(2.0 ** -126)).any()
    t_ref, tri_ref = EL.big_dir_expected(base)
    hit = tri_ref >= 0
    print(base, "hits by exponent", {int(k): int(hit[e == k].sum()) for k in EL.BIG_EXPONENTS})
    assert hit.mean() >= 0.25 and hit[:64].mean() >= 0.5 and hit[e < 0].any()
    assert np.isfinite(t_ref[hit]).all() and (np.abs(t_ref[hit]) >= np.finfo(F32).tiny).all()
    b = _bvh(base)
    t, tri = b.intersect(o, d)
    bad = np.flatnonzero((RW.bits(t) != RW.bits(t_ref)) | (tri != tri_ref))
    assert bad.size == 0, (base, bad[:5], t[bad[:5]], t_ref[bad[:5]], tri[bad[:5]], tri_ref[bad[:5]])
    _, verts, mtype, mvals, nodes, idx = E.arrays(base)
    st0 = EL.seeds(EL.N_BIG)[:, 0]
    want, _, segs = RT.trace(nodes, idx, verts, mtype, mvals, o, d, st0, 5)
    got, st = b.trace(o, d, 5, seed=EL.SEED)
    RT.assert_same(got, want, f"{base}: trace")
    assert st["rays"] == int(segs.sum())
    for mis in MIS:
        want, segs, sh, dr = EL.radiance(EL.big_dir_paths(base, mis), 5)
        got, st = b.trace_nee(o, d, 5, seed=EL.SEED, mis=mis)
        RT.assert_same(got, want, f"{base}: trace_nee mis {mis}")
        _same_stats(st, int(segs.sum()), int(sh.sum()), int(dr.sum()), EL.lights(base), base)
        assert sh.sum() > 0 and EL.lit_rays(want) > 0
