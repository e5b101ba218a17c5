"""The domain facts the device's acosf_fast rests on when it calls the reciprocal and square-root
sequences without their range guards (pt_math.h), recomputed in numpy over the sampler's whole
grid: float32 arithmetic, every operation rounded on its own (no FMA), as the device code is built.

The sampler's argument is x = fl(2u - 1) for u = (float)state / 2^32, which lies on the grid
k 2^-24 of [-1, 1] (tests/test_math.py checks that over all 2^32 states). The grid points the fast
stream answers itself are those with 2^-26 < |x| < 1: every k with 0 < |k| < 2^24."""
import numpy as np

F32 = np.float32
Q1, Q2, Q3, Q4 = F32(-2.4033949375e+00), F32(2.0209457874e+00), F32(-6.8828397989e-01), F32(7.7038154006e-02)
RCP_LO, RCP_HI = F32(2.0) ** -126, F32(2.0) ** 126      # rcp_exact's proven range
SQRT_LO, SQRT_HI = F32(2.0) ** -100, F32(2.0) ** 100    # sqrt_exact's proven range


def _operands(k: np.ndarray):
    """(q, zs, s + df, zs - df df) of acosf_fast for x = k 2^-24, as float32 arrays."""
    x = k.astype(F32) * F32(2.0 ** -24)
    ax = np.abs(x)
    small = ax < F32(0.5)
    z = np.where(small, x * x, (F32(1.0) - ax) * F32(0.5)).astype(F32)
    q = F32(1.0) + z * (Q1 + z * (Q2 + z * (Q3 + z * Q4)))
    zs = np.where(small, F32(0.25), z).astype(F32)
    s = np.sqrt(zs)  # correctly rounded in float32
    df = (s.view(np.uint32) & np.uint32(0xFFFFF000)).view(F32)
    assert q.dtype == zs.dtype == s.dtype == df.dtype == F32
    return small, q, zs, s + df, zs - df * df


def test_acosf_inner_operands_stay_in_the_proven_ranges():
    lo = {"q": np.inf, "zs": np.inf, "sd": np.inf}
    hi = {"q": -np.inf, "zs": -np.inf, "sd": -np.inf}
    n = 0
    step = 1 << 22
    for start in range(1, 1 << 24, step):  # k and -k: the operands depend on |x| alone
        k = np.arange(start, min(start + step, 1 << 24), dtype=np.int64)
        for sign in (1, -1):
            small, q, zs, sd, num = _operands(sign * k)
            n += k.size
            for name, v in (("q", q), ("zs", zs), ("sd", sd)):
                lo[name] = min(lo[name], float(v.min()))
                hi[name] = max(hi[name], float(v.max()))
            assert not num[small].any()  # |x| < 0.5: c = 0 / (s + df), as before
    assert n == (1 << 25) - 2
    print({k: (lo[k], hi[k]) for k in lo})
    # the ranges the grid reaches (0.5150069 is the float32 0x3f03d77e, 0.51500689983...)
    assert float(F32(0.5150069)) <= lo["q"] and hi["q"] <= 1.0
    assert 2.0 ** -25 <= lo["zs"] and hi["zs"] <= 0.25
    assert 3.45e-4 <= lo["sd"] and hi["sd"] <= 1.0
    # and they lie inside the ranges on which the unguarded sequences are exact
    assert RCP_LO <= lo["q"] and hi["q"] <= RCP_HI
    assert SQRT_LO <= lo["zs"] and hi["zs"] <= SQRT_HI
    assert RCP_LO <= lo["sd"] and hi["sd"] <= RCP_HI


def test_edge_inputs_are_the_rest_of_the_grid():
    """What the wave-uniform fallback answers: |x| >= 1 and |x| <= 2^-26. On the grid that is
    x = -1, 0 and 1 only, so a wave takes it about once in 2^18 samples."""
    k = np.array([-(1 << 24), -1, 0, 1, 1 << 24], dtype=np.int64)
    ax = (k.astype(F32) * F32(2.0 ** -24)).view(np.uint32) & np.uint32(0x7FFFFFFF)
    edge = (ax >= np.uint32(0x3F800000)) | (ax <= np.uint32(0x32800000))
    assert edge.tolist() == [True, False, True, False, True]


def test_lcg_step_by_24_bit_multiplies_is_the_same_integer():
    """mad_u32_u24(s, a, c) + (mul_u32_u24(s >> 24, a) << 24) == a s + c mod 2^32 for a = 1664525
    < 2^24: the restatement of Lcg::next01's step that was measured and not adopted (v_mul_lo_u32
    costs one main-port slot). On 2^20 random states and the 2^16 states around
    each multiple of 2^24, where the two halves of s meet."""
    a, c, m32, m24 = np.uint64(1664525), np.uint64(1013904223), np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFF)
    rnd = np.random.default_rng(24).integers(0, 1 << 32, 1 << 20, dtype=np.uint64)
    near = (np.arange(256, dtype=np.int64)[:, None] * (1 << 24) + np.arange(-(1 << 15), 1 << 15, dtype=np.int64)[None, :])
    s = np.concatenate([rnd, (near.reshape(-1) % (1 << 32)).astype(np.uint64)])
    assert s.size == (1 << 20) + 256 * (1 << 16)
    mad = ((s & m24) * a + c) & m32            # v_mad_u32_u24: 24-bit operands, low 32 bits of the sum
    mul = (((s >> np.uint64(24)) & m24) * a) & m32  # v_mul_u32_u24
    got = (mad + ((mul << np.uint64(24)) & m32)) & m32
    assert np.array_equal(got, (a * s + c) & m32)
