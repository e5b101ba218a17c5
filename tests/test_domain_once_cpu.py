"""One domain verdict per ray (PT_DOMAIN_ONCE), without a device.

The flat body no longer tests a ray's inv = 1 / d where it is used: the range predicate of the
reciprocal (rcp3_exact_v, pt_math.h) is the verdict "inv is finite, non-zero and not NaN", and the
slab rule and the top-of-iteration test read it. Here: the implication in float32 numpy, the
verdict's two forms restated in numpy and through the host build (pt_debug_domain_once,
device -1), on crafted components in each slot beside two ordinary ones, and the unit form's
precondition (no NaN, |component| <= 1) on the actual hemisphere_dir for 2^16 LCG states, the
ones that make a zero component among them."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _edgelights as EL

F32 = np.float32
TINY, HUGE = F32(2.0) ** F32(-126), F32(2.0) ** F32(126)
BOX = np.array([213, 548.7, 227, 343, 548.7, 332], dtype=F32)  # the Cornell light's leaf box
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def bind(ptamd):
    """The two hooks' argument types (ctypes would pass the 64-bit count as an int otherwise)."""
    L = ptamd.lib()
    L.pt_debug_domain_once.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                       C.c_void_p]
    L.pt_debug_hemisphere_dir.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    return ptamd


@pytest.fixture(scope="module")
def pt():
    import ptamd
    return bind(ptamd)


def _bits(x):
    return F32(x).view(np.uint32)


def _specials():
    """+-0, subnormals, 2^-127, 2^-126, the float below 2^-126, 1.0, the float above 1.0, NaN, inf
    (both signs of each), and the neighbours of the two-sided form's upper bound."""
    sub_min, sub_max = np.uint32(1).view(F32), np.nextafter(TINY, F32(0))
    pos = [F32(0), sub_min, F32(2.0) ** F32(-127), sub_max, TINY, F32(1), np.nextafter(F32(1), F32(2)),
           F32(np.nan), F32(np.inf), HUGE, np.nextafter(HUGE, F32(np.inf)), F32(2.0) ** F32(127)]
    assert _bits(sub_max) == 0x007FFFFF and _bits(TINY) == 0x00800000
    return np.array(pos + [-x for x in pos], dtype=F32)


@pytest.fixture(scope="module")
def crafted():
    """(d (n, 3), o (n, 3)): every special in each slot beside two ordinary components, against
    origins inside, beside and far from the box, one of them not finite."""
    ordinary = [(F32(0.6), F32(-0.64)), (F32(-0.28), F32(0.96)), (F32(2.0) ** F32(-20), F32(1))]
    rows = []
    for s, (a, b), slot in itertools.product(_specials(), ordinary, range(3)):
        v = [a, b]
        v.insert(slot, s)
        rows.append(v)
    rows += [[F32(0.48), F32(0.6), F32(-0.64)], [F32(1), F32(1), F32(1)], [TINY, TINY, -TINY]]  # nothing special
    d = np.array(rows, dtype=F32)
    os_ = np.array([[278, 273, 300], [100, 600, 100], [278, 548.7, 280], [1e30, 0, 0], [np.inf, 0, 0], [0, np.nan, 0]],
                   dtype=F32)
    d = np.repeat(d, len(os_), axis=0)
    o = np.tile(os_, (len(rows), 1))
    for a in (d, o):
        a.setflags(write=False)
    return d, o


def _inv(d):
    with np.errstate(all="ignore"):
        return (F32(1) / d).astype(F32)


def _verdict_np(d, unit):
    """rcp3_exact_v's predicate: the minimum as v_min3_f32 takes it (a NaN operand is skipped) and,
    in the two-sided form, the left-to-right float32 sum of the magnitudes."""
    a = np.abs(d)
    with np.errstate(all="ignore"):
        ok = np.fmin(np.fmin(a[:, 0], a[:, 1]), a[:, 2]) >= TINY
        if not unit:
            s = ((a[:, 0] + a[:, 1]).astype(F32) + a[:, 2]).astype(F32)
            ok &= s <= HUGE
    return ok


def _unit_pre(d):
    """What the unit form assumes of its input: hemisphere_dir's sample (test_hemisphere_... below)."""
    with np.errstate(all="ignore"):
        return (np.abs(d) <= F32(1) + F32(2.0) ** F32(-22)).all(axis=1)  # false for NaN


def _probe(pt, o, d, unit, device=-1):
    o, d = np.ascontiguousarray(o, dtype=F32), np.ascontiguousarray(d, dtype=F32)
    n = d.shape[0]
    out, inv = np.zeros((n, 6), dtype=np.uint8), np.zeros((n, 3), dtype=F32)
    assert pt.lib().pt_debug_domain_once(device, P(BOX), P(o), P(d), n, int(unit), P(out), P(inv)) == 0, \
        pt.lib().pt_last_error()
    return out.astype(bool), inv


def test_implication_float32(crafted):
    """min |d_i| >= 2^-126 and |d_i| <= 1 + 2^-22 => every 1 / d_i is finite and non-zero; the
    crafted set holds rows on both sides, and the boundary values themselves."""
    d, _ = crafted
    with np.errstate(all="ignore"):
        pre = (np.abs(d) >= TINY).all(axis=1) & (np.abs(d) <= F32(1) + F32(2.0) ** F32(-22)).all(axis=1)
    inv = _inv(d)
    good = np.isfinite(inv).all(axis=1) & (inv != 0).all(axis=1)
    assert pre.sum() > 50 and (~pre).sum() > 50
    assert good[pre].all()
    # the interval's ends map onto each other: [2^-126, 1] -> [1, 2^126]
    assert _inv(np.array([TINY, F32(1)], dtype=F32)).tolist() == [float(HUGE), 1.0]


@pytest.mark.parametrize("unit", [False, True])
def test_verdict_never_fast_where_inv_is_not_finite(crafted, unit):
    """The numpy restatement: the two-sided form on every crafted row (NaN and inf included); the
    unit form on the rows that meet its precondition."""
    d, _ = crafted
    v = _verdict_np(d, unit)
    if unit:
        v &= _unit_pre(d)
    inv = _inv(d)
    fin, nz = np.isfinite(inv).all(axis=1), (inv != 0).all(axis=1)
    assert v.sum() > 20 and (~fin).sum() > 100
    assert not (v & ~fin).any() and not (v & ~nz).any()
    if not unit:  # the form that takes any float must refuse every NaN, infinite or out-of-range component
        with np.errstate(all="ignore"):
            out = ~((np.abs(d) >= TINY) & (np.abs(d) <= HUGE)).all(axis=1)
        assert not (v & out).any()


@pytest.mark.parametrize("unit", [False, True])
def test_host_build_agrees(pt, crafted, unit):
    """The code itself on the host: the verdict equals the restatement, implies the three
    predicates it replaces, the reciprocal keeps its bits, and the guard-free slab rule is the
    guarded one (on the host every ray is its own wave, so on every row)."""
    d, o = crafted
    if unit:
        keep = _unit_pre(d)
        d, o = d[keep], o[keep]
    r, inv = _probe(pt, o, d, unit)
    assert np.array_equal(r[:, 3], _verdict_np(d, unit))
    want = _inv(d)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(inv), nan) and np.array_equal(inv[~nan].view(np.uint32), want[~nan].view(np.uint32))
    fast = r[:, 3]
    assert fast.any() and (~fast).any()
    assert r[fast][:, :3].all()  # rcp3_exact's own predicate, finite_nonzero3(inv), all_finite(inv)
    assert np.array_equal(r[:, 1], (np.isfinite(want) & (want != 0)).all(axis=1))
    assert np.array_equal(r[:, 2], np.isfinite(want).all(axis=1))
    assert np.array_equal(r[:, 4], r[:, 5]) and r[:, 4].any() and (~r[:, 4]).any()


def test_hemisphere_dir_meets_the_unit_precondition(pt):
    """hemisphere_dir on 2^16 LCG states about five normals: no NaN, |component| <= 1, and the
    states whose second draw is 0 (sin phi = 0) or whose first is 0 or 1 give an exactly zero
    component, i.e. rays outside the domain that the verdict must refuse."""
    edge = np.concatenate([EL.lcg_prev(np.array([0, 1, 0xFFFFFFFF, EL.one_edge()], dtype=np.uint32), 2),
                           EL.lcg_prev(np.array([0, 0xFFFFFFFF, EL.one_edge()], dtype=np.uint32), 1)])
    n = 1 << 16
    st = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)).astype(np.uint32)
    st[:edge.size] = edge
    nrm = np.array([[0, 1, 0], [0, 0, -1], [1, 0, 0], [0.6, 0, 0.8], [-0.48, 0.6, 0.64]], dtype=F32)[np.arange(n) % 5]
    nrm = np.ascontiguousarray(nrm)
    d = np.zeros((n, 3), dtype=F32)
    assert pt.lib().pt_debug_hemisphere_dir(P(st), P(nrm), n, P(d)) == 0
    assert not np.isnan(d).any() and (np.abs(d) <= F32(1)).all()
    zero = (d == 0).any(axis=1)
    assert zero[:edge.size].any(), d[:edge.size]
    r, inv = _probe(pt, np.tile(np.array([[278, 273, 300]], dtype=F32), (n, 1)), d, True)
    fast = r[:, 3]
    assert not (fast & zero).any() and fast.sum() > n - 64
    assert r[fast][:, :3].all() and np.array_equal(r[:, 4], r[:, 5])
    assert np.array_equal(fast, (np.abs(d) >= TINY).all(axis=1))
