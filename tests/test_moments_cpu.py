"""The host side of the per-pixel sample moments (include/pt_hip.h): the new symbols, and
pt_moments_unconverged against a numpy restatement of its criterion. No device needed."""
import ctypes as C

import numpy as np
import pytest

import ptamd
from ptamd import _lib

F64 = np.float64
NEW = ("pt_ctx_render_moments", "pt_moments_unconverged", "pt_ctx_unconverged", "pt_ctx_render_converge")


def np_unconverged(S, Q, n, rel, abs_):
    """The contract's inequality in float64, every operation a numpy operation of its own:
    a = n*Q; b = S*S; l = a - b; t = rel*|S| + abs*n; r = (n-1)*(t*t); converged = l <= r.
    Returns the per-pixel mask (1 = unconverged) over (..., 3) arrays."""
    S, Q = np.asarray(S, dtype=F64), np.asarray(Q, dtype=F64)
    if n < 2:
        return np.ones(S.shape[:-1], dtype=np.uint8)
    dn, rel, abs_ = F64(n), F64(np.float32(rel)), F64(np.float32(abs_))
    with np.errstate(all="ignore"):
        a = dn * Q
        b = S * S
        l = a - b
        t = rel * np.abs(S) + abs_ * dn
        r = (dn - F64(1)) * (t * t)
        conv = l <= r
    return (~conv.all(axis=-1)).astype(np.uint8)


def integer_moments(rng, npix, n, hi=9):
    """S and Q of n integer-valued samples per pixel and channel: exact in double, n*Q >= S*S."""
    r = rng.integers(0, hi + 1, size=(n, npix, 3)).astype(F64)
    return r.sum(axis=0), (r * r).sum(axis=0)


def test_symbols_and_abi():
    L = ptamd.lib()
    assert L.pt_abi_version() == 3
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTED
    assert C.sizeof(_lib.pt_moments) == 24 and C.sizeof(_lib.pt_converge) == 32
    assert C.sizeof(_lib.pt_converge_stats) == 48


@pytest.mark.parametrize("n", [2, 3, 17, 1000])
def test_host_count_matches_numpy(n):
    rng = np.random.default_rng(n)
    S, Q = integer_moments(rng, 301, n)
    S[:7] = 0.0  # pixels whose samples are all +0: converged at any tolerance
    Q[:7] = 0.0
    seen = set()
    for rel, abs_ in [(0.5, 0.0), (0.1, 0.0), (0.0, 1.5), (0.02, 0.25), (1e-6, 0.0), (0.0, 1e-3), (10.0, 10.0)]:
        want = np_unconverged(S, Q, n, rel, abs_)
        cnt, mask = ptamd.moments_unconverged(S, Q, n, rel, abs_, mask=True)
        assert np.array_equal(mask, want), (n, rel, abs_)
        assert cnt == int(want.sum()) == ptamd.moments_unconverged(S, Q, n, rel, abs_)
        assert not mask[:7].any()
        seen.add(0 < cnt < 301)
    assert seen == {True, False}  # some tolerances split the pixels, some do not


@pytest.mark.parametrize("n", [-3, 0, 1])
def test_fewer_than_two_samples(n):
    S, Q = integer_moments(np.random.default_rng(5), 40, 1)
    cnt, mask = ptamd.moments_unconverged(S, Q, n, 10.0, 10.0, mask=True)
    assert cnt == 40 and mask.all()
    assert ptamd.moments_unconverged(np.zeros((0, 3)), np.zeros((0, 3)), 4, 0.1) == 0


def test_non_finite_entries_are_unconverged():
    n = 8
    S, Q = integer_moments(np.random.default_rng(9), 64, n)
    rel, abs_ = 100.0, 100.0  # every finite pixel converges
    assert ptamd.moments_unconverged(S, Q, n, rel, abs_) == 0
    bad = {3: (np.nan, None), 10: (None, np.nan), 20: (np.inf, None), 30: (None, np.inf), 40: (-np.inf, np.inf),
           50: (np.inf, np.inf)}
    for q, (s, qq) in bad.items():
        if s is not None:
            S[q, q % 3] = s
        if qq is not None:
            Q[q, (q + 1) % 3] = qq
    cnt, mask = ptamd.moments_unconverged(S, Q, n, rel, abs_, mask=True)
    want = np_unconverged(S, Q, n, rel, abs_)
    assert np.array_equal(mask, want) and cnt == int(want.sum())
    assert set(np.flatnonzero(mask).tolist()) <= set(bad)
    assert mask[3] and mask[10]  # a NaN compares false
    assert mask[30] and mask[40] and mask[50]  # Q = inf: the left side is +inf
    assert not mask[20]  # S = inf alone: -inf <= +inf (the inequality, not a promise about such input)


def test_exact_boundary_counts_as_converged():
    """Samples {1, 3}: S = 4, Q = 10, n*Q - S*S = 4; t = 2 makes (n-1)*t*t = 4 as well."""
    S = np.full((1, 3), 4.0)
    Q = np.full((1, 3), 10.0)
    assert ptamd.moments_unconverged(S, Q, 2, 0.5, 0.0) == 0    # t = 0.5 * 4
    assert ptamd.moments_unconverged(S, Q, 2, 0.0, 1.0) == 0    # t = 1 * 2
    assert ptamd.moments_unconverged(S, Q, 2, 0.25, 0.5) == 0   # t = 1 + 1
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert ptamd.moments_unconverged(S, Q, 2, below, 0.0) == 1
    assert ptamd.moments_unconverged(S, Q, 2, 0.0, float(np.nextafter(np.float32(1), np.float32(0)))) == 1
    Q[0, 2] = np.nextafter(10.0, 11.0)  # one channel just past the boundary
    assert ptamd.moments_unconverged(S, Q, 2, 0.5, 0.0) == 1


def test_argument_errors():
    L = ptamd.lib()
    S, Q = integer_moments(np.random.default_rng(1), 4, 3)
    cnt = C.c_int64(-7)

    def call(rel, abs_, count=cnt, s=S, q=Q, npix=4):
        return L.pt_moments_unconverged(s.ctypes.data if s is not None else None, q.ctypes.data if q is not None else None,
                                        npix, 3, C.c_float(rel), C.c_float(abs_),
                                        C.byref(count) if count is not None else None, None)

    assert call(0.1, 0.0) == 0 and cnt.value >= 0
    for rel, abs_ in [(0.0, 0.0), (-0.1, 1.0), (1.0, -0.1), (float("nan"), 1.0), (1.0, float("nan"))]:
        assert call(rel, abs_) == _lib.PT_E_ARG, (rel, abs_)
        assert b"rel" in L.pt_last_error()
    assert call(0.1, 0.0, count=None) == _lib.PT_E_ARG
    assert call(0.1, 0.0, s=None) == _lib.PT_E_ARG
    assert call(0.1, 0.0, npix=-1) == _lib.PT_E_ARG
    with pytest.raises(ptamd.PTError):
        ptamd.moments_unconverged(S, Q, 3, 0.0, 0.0)
    with pytest.raises(ValueError):
        ptamd.moments_unconverged(S, Q[:2], 3, 0.1)
