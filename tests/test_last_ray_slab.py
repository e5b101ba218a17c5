"""The flat kernels' form of the last-ray rule: a path's last ray whose slab
test of the emitter box E itself fails (emit_slab_reject, pt_math.h) is not traced.

CPU: the predicate against a float32 restatement of the reference's AABB::intersect_inv for
boxes inside E, on random and adversarial inputs; its agreement with the sign rule
(emit_reject) wherever its guard holds; the generated scene-kernel source. GPU: float32 bits
and ray counts against the oracle on every flat kernel path under the slab rule, the sign-only
hook (PT_EMIT_REJECT=sign) and the rule off, and the early-end counts of the three."""
import ctypes as C
import re

import numpy as np
import pytest

import test_last_ray as LR
from test_last_ray import F32, INF, _bits, _bvh, _intersect_inv, _oracle, _rtc_source, _scene, gpu, pt  # noqa: F401

LIGHT = np.array([213, 548.7, 227, 343, 548.7, 332], dtype=F32)
EMPTY = np.array([np.inf] * 3 + [-np.inf] * 3, dtype=F32)


# ---------------------------------------------------------------- the predicate (CPU)
def _slab_reject(pt, box, o, inv):
    box, o, inv = (np.ascontiguousarray(a, dtype=F32) for a in (box, o, inv))
    n = o.shape[0]
    out = np.zeros(n, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert pt.lib().pt_debug_emit_slab_reject(p(box), p(o), p(inv), n, p(out)) == 0
    return out.astype(bool)


def _inv(d):
    with np.errstate(all="ignore"):
        return (F32(1) / d).astype(F32)


def _guard(o, inv):
    return (np.isfinite(inv) & (inv != 0)).all(axis=1) & np.isfinite(o).all(axis=1)


def _check(pt, elb, ert, lb, rt, o, d):
    """For every row: reject => intersect_inv fails for B; reject => the guard holds; and the sign
    rule under the guard => reject. Returns (rejected, rejected by the sign rule under the guard)."""
    assert np.all(elb <= lb) and np.all(lb <= rt) and np.all(rt <= ert)  # the inputs are boxes inside E
    inv = _inv(d)
    box = np.concatenate([elb, ert], axis=1)
    rej = _slab_reject(pt, box, o, inv)
    bad = np.flatnonzero(rej & _intersect_inv(lb, rt, o, inv))
    assert bad.size == 0, (bad[:5], elb[bad[:5]], ert[bad[:5]], lb[bad[:5]], rt[bad[:5]], o[bad[:5]], d[bad[:5]])
    g = _guard(o, inv)
    bad = np.flatnonzero(rej & ~g)
    assert bad.size == 0, (bad[:5], o[bad[:5]], d[bad[:5]])
    sign = LR._reject(pt, box, o, d) & g
    bad = np.flatnonzero(sign & ~rej)
    assert bad.size == 0, (bad[:5], elb[bad[:5]], ert[bad[:5]], o[bad[:5]], d[bad[:5]])
    return rej, sign


def _random_cases(n, seed):
    """E, a box B inside it (a share each of B = E, flat axes and point boxes), o around E (a share
    inside it) and a unit d."""
    g = np.random.default_rng(seed)
    elb = g.uniform(-100, 100, (n, 3)).astype(F32)
    ert = (elb + g.uniform(0, 100, (n, 3)).astype(F32)).astype(F32)
    flat = g.random((n, 3)) < 0.1  # flat axes of E (the Cornell light's y)
    ert = np.where(flat, elb, ert)
    lb = np.clip((elb + g.uniform(0, 1, (n, 3)).astype(F32) * (ert - elb)).astype(F32), elb, ert)
    rt = np.clip((lb + g.uniform(0, 1, (n, 3)).astype(F32) * (ert - lb)).astype(F32), lb, ert)
    kind = g.integers(0, 10, n)
    lb = np.where((kind == 0)[:, None], elb, lb)  # B = E
    rt = np.where((kind == 0)[:, None], ert, rt)
    rt = np.where((kind == 1)[:, None], lb, rt)  # a point box
    rt = np.where((kind == 2)[:, None] & (g.random((n, 3)) < 0.5), lb, rt)  # flat axes of B
    o = g.uniform(-250, 250, (n, 3)).astype(F32)
    inside = g.random(n) < 0.15
    o = np.where(inside[:, None], (elb + g.uniform(0, 1, (n, 3)).astype(F32) * (ert - elb)).astype(F32), o)
    d = g.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    return elb, ert, lb, rt, o, d


def test_slab_predicate_implies_miss_of_every_inner_box_random(pt):
    """400,000 seeded cases. Not vacuous: the rejected count is printed and non-zero, and it is
    above the sign rule's on the same rays."""
    rej, sign = _check(pt, *_random_cases(400_000, 20261019))
    print(f"random set: {rej.sum()} of {rej.size} rejected by the slab rule, {sign.sum()} by the sign rule")
    assert rej.sum() > 0 and rej.sum() > sign.sum() > 0


def _axis_cases():
    """One axis: (elb, ert, lb, rt, o, d). o on and one ulp to either side of each plane of E,
    inside E, far away, inf and NaN; d over +-0, subnormals (1 / d overflows), +-1, values whose
    reciprocal is subnormal, inf and NaN."""
    planes = [F32(x) for x in (0.0, 1.0, -1.0, 3.5, 2.0 ** 60, -(2.0 ** 60), 1e-40, -1e-40, 548.7)]
    ds = []
    for v in (F32(0), F32(1e-45), F32(1e-39), F32(2.0 ** -127), F32(1e-3), F32(0.5), F32(1), F32(2), F32(2.0 ** 127),
              F32(3e38), INF):
        ds += [v, -v]
    ds.append(F32(np.nan))
    rows = []
    for a in planes:
        for b in planes:
            if not a <= b:
                continue
            mid = F32((np.float64(a) + np.float64(b)) / 2)
            for lb, rt in ((a, b), (a, a), (b, b), (mid, mid), (a, mid), (mid, b)):
                os_ = {a, b, np.nextafter(a, -INF), np.nextafter(a, INF), np.nextafter(b, -INF), np.nextafter(b, INF),
                       F32(0), F32(2.0 ** 60), F32(-(2.0 ** 60)), mid, INF, -INF, F32(np.nan)}
                for o in os_:
                    for d in ds:
                        rows.append((a, b, lb, rt, o, d))
    return np.array(rows, dtype=F32)


def test_slab_predicate_adversarial_grid(pt):
    """The grid on each axis in turn with the other axes running through the same cases out of
    step, then 10^6 random triples of axis cases. Every row is checked (_check: a rejection only
    under the guard, so never with a NaN, an infinity or a zero of inv, or a non-finite o)."""
    A = _axis_cases()
    n = A.shape[0]
    assert n > 30_000
    total = 0
    for ax in range(3):
        cols = [np.roll(A, 7919 * ((k - ax) % 3), axis=0) for k in range(3)]
        stack = np.stack(cols, axis=1)  # (n, axis, field)
        f = [np.ascontiguousarray(stack[:, :, j]) for j in range(6)]
        total += _check(pt, *f)[0].sum()
    g = np.random.default_rng(7)
    pick = g.integers(0, n, (1_000_000, 3))
    stack = np.stack([A[pick[:, k]] for k in range(3)], axis=1)
    f = [np.ascontiguousarray(stack[:, :, j]) for j in range(6)]
    rej, _ = _check(pt, *f)
    total += rej.sum()
    print(f"adversarial grid: {total} rejections")
    assert total > 0
    # the guard, stated directly: any of these in one component and the answer is 0
    one = np.ones((1, 3), dtype=F32)
    box = np.array([[10, 10, 10, 20, 20, 20]], dtype=F32)
    assert _slab_reject(pt, box, one, -one).all()  # the base case is a rejection (E lies ahead, the ray points away)
    for bad in (np.nan, np.inf, -np.inf, 0.0, -0.0):
        for a in range(3):
            inv = -one.copy()
            inv[0, a] = bad
            assert not _slab_reject(pt, box, one, inv).any(), (bad, a)
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            o = one.copy()
            o[0, a] = bad
            assert not _slab_reject(pt, box, o, -one).any(), (bad, a)


def test_flat_and_empty_emitter_boxes(pt):
    """The Cornell light (flat in y) against rays from the floor and the walls, and the empty box,
    which rejects every ray, whatever it holds."""
    g = np.random.default_rng(3)
    n = 20000
    o = np.stack([g.uniform(0, 556, n), g.uniform(0, 548, n), g.uniform(0, 559, n)], axis=1).astype(F32)
    d = g.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    box = np.tile(LIGHT, (n, 1))
    rej, sign = _check(pt, box[:, :3], box[:, 3:], box[:, :3], box[:, 3:], o, d)
    # from below the light every downward ray is the sign rule's (half of them at least); the slab
    # rule adds the upward rays that pass beside the light: of the rays the sign rule leaves
    # (about 0.5 * 0.62 * 0.59 = 18 %: upward, not pointing away in x or z) well over a quarter
    print(f"Cornell light: slab rule {rej.mean():.4f}, sign rule {sign.mean():.4f}")
    assert sign.sum() > 0.5 * n and rej.sum() > sign.sum() + 0.05 * n and rej.sum() < n
    rows = np.array([[0, 0, 0], [np.nan] * 3, [np.inf, 0, -np.inf], [1, 2, 3]], dtype=F32)
    for inv in rows:
        assert _slab_reject(pt, np.tile(EMPTY, (4, 1)), rows, np.tile(inv, (4, 1))).all()


def test_generated_source_holds_the_slab_call_only_when_on(pt, monkeypatch):
    b = _bvh(pt, _scene("cornell"))
    src = _rtc_source(pt, b)
    m = re.search(r"emit_slab_reject\(v3\{([^}]*)\}, v3\{([^}]*)\}, o, inv\)", src)
    assert m and "static constexpr bool kSlab = !PT_EMIT_SIGN_ONLY;" in src
    lits = [float.fromhex(x.strip().rstrip("f")) for x in (m.group(1) + "," + m.group(2)).split(",")]
    assert np.array(lits, dtype=F32).tobytes() == LIGHT.tobytes()
    assert "#define PT_EMIT_SIGN_ONLY 1" not in src
    # everything of it sits inside the EmitRej block
    block = src[src.index("    struct EmitRej {"):src.index("    __device__ __forceinline__ static unsigned long long mask(")]
    assert "emit_slab_reject(" in block and "emit_slab_reject(" not in src.replace(block, "")
    # the sign-only hook: the same source with the define in front (pt_rtc_check compiled it)
    monkeypatch.setenv("PT_EMIT_REJECT", "sign")
    sign_src = _rtc_source(pt, b)
    assert sign_src.replace("#define PT_EMIT_SIGN_ONLY 1\n", "", 1) == src and sign_src != src
    monkeypatch.setenv("PT_EMIT_REJECT", "0")
    assert "emit_slab_reject(" not in _rtc_source(pt, b)
    monkeypatch.delenv("PT_EMIT_REJECT")
    # no emitter: the inf literals compile (pt_rtc_check compiled the source)
    src = _rtc_source(pt, _bvh(pt, _scene("no_emitter")))
    assert "emit_slab_reject(v3{__builtin_inff(), __builtin_inff(), __builtin_inff()}, v3{-__builtin_inff()," in src
    # not dark: no rule
    assert "emit_slab_reject(" not in _rtc_source(pt, _bvh(pt, _scene("diffuse_emits")))


# ---------------------------------------------------------------- renders (GPU)
FLAT_PATHS = {k: LR.PATHS[k] for k in ("rtc", "table_fast", "table")}
FORMS = {"slab": ({}, True), "sign": ({"PT_EMIT_REJECT": "sign"}, True), "off": ({}, False)}


def _run(gpu, monkeypatch, kind, path, form, depth, extra=None, **kw):
    env, want = FLAT_PATHS[path]
    fenv, rule = FORMS[form]
    return LR._run(gpu, monkeypatch, kind, {**env, **fenv, **(extra or {})}, want, rule, depth, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cornell", "mcornell_r0.8"])
@pytest.mark.parametrize("path", list(FLAT_PATHS))
def test_rule_forms_on_every_flat_path(gpu, monkeypatch, path, kind):
    """Slab rule, sign-only hook and rule off at depths 2, 3 and 5: bits, rays, kernel path, and
    early(sign-only) <= early(slab) <= last segments (LR._run checks the upper bound), strictly
    more under the slab rule on Cornell at depth 5."""
    for depth in (2, 3, 5):
        early = {form: _run(gpu, monkeypatch, kind, path, form, depth) for form in FORMS}
        print(f"{kind} {path} depth {depth}: early ends {early}")
        assert early["off"] == 0 and early["sign"] <= early["slab"], (kind, path, depth, early)
        if kind == "cornell" and depth == 5:
            assert early["sign"] < early["slab"], (path, early)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cornell", "mcornell_r0.8"])
def test_sign_only_hook_is_the_sign_rule_on_every_flat_path(gpu, monkeypatch, kind):
    """The scene kernel's hook runs emit_reject itself, the table kernels' the slab rule's
    `tmax < 0` term under its guard, which is the same condition for the rays a render makes
    (unit directions, finite inv): the same paths end early, and as many as on the tree walk,
    which has no other rule."""
    early = {path: _run(gpu, monkeypatch, kind, path, "sign", 5) for path in FLAT_PATHS}
    env, want = LR.PATHS["tree"]
    early["tree"] = LR._run(gpu, monkeypatch, kind, env, want, True, 5)
    assert len(set(early.values())) == 1, early


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(FLAT_PATHS))
def test_no_emitter_every_last_ray_ends_early_under_the_slab_rule(gpu, monkeypatch, path):
    for depth in (2, 5):
        early = _run(gpu, monkeypatch, "no_emitter", path, "slab", depth)
        ref, rays, shallower = _oracle("no_emitter", (36, 30), 5, depth)
        assert not _bits(ref).any()
        assert early == rays - shallower, (path, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["back_wall_emits", "two_lights"])
def test_origins_inside_a_large_emitter_box(gpu, monkeypatch, kind):
    """E spans the room (or most of it): most origins lie inside it, where neither rule rejects."""
    for path in ("rtc", "table"):
        e_slab = _run(gpu, monkeypatch, kind, path, "slab", 5)
        e_sign = _run(gpu, monkeypatch, kind, path, "sign", 5)
        assert e_sign <= e_slab, (kind, path, e_sign, e_slab)


@pytest.mark.gpu
def test_merged_leaves_larger_box(gpu, monkeypatch):
    """_trees.merged(5): the emitter's leaf box is larger than the light (generic table kernel and
    the scene kernel)."""
    for path in ("table", "rtc"):
        e_slab = _run(gpu, monkeypatch, "cornell", path, "slab", 5, merged=5)
        e_sign = _run(gpu, monkeypatch, "cornell", path, "sign", 5, merged=5)
        assert e_sign <= e_slab, (path, e_sign, e_slab)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(FLAT_PATHS))
def test_one_wave_of_mixed_lanes_across_refills(gpu, monkeypatch, path):
    """One 64 x 1 frame at 70 spp, depth 3: rejected lanes, surviving lanes and fresh camera lanes
    meet in one wave, so the carried inv crosses refills."""
    for form in FORMS:
        _run(gpu, monkeypatch, "cornell", path, form, 3, res=(64, 1), spp=70)


@pytest.mark.gpu
@pytest.mark.parametrize("hook", [{"PT_PAIR_QUEUE": "16"}, {"PT_PAIRS": "0"}, {"PT_FORCE_EXACT_SLAB": "2"}])
def test_carried_inv_feeds_the_lane_loops_and_the_exact_walk(gpu, monkeypatch, hook):
    for path in FLAT_PATHS:
        for kind in ("cornell", "mcornell_r0.8"):
            _run(gpu, monkeypatch, kind, path, "slab", 5, extra=hook)


@pytest.mark.gpu
def test_camera_inv_in_the_start_branch_form(gpu, monkeypatch):
    """The scene kernel's other form of the camera ray's inv (PT_CAM_INV=1: computed in the branch
    that starts the path, as the generic table kernel does) renders the same bits."""
    extra = {"PT_RTC_DEFINES": "PT_COUNT_EARLY=1,PT_CAM_INV=1"}
    _run(gpu, monkeypatch, "cornell", "rtc", "slab", 5, extra=extra)
    _run(gpu, monkeypatch, "cornell", "rtc", "slab", 3, extra=extra, res=(64, 1), spp=70)
