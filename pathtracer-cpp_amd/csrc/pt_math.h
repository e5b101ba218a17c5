// pt_math.h — bit-exact arithmetic of the reference trace loop, for gfx950 and host.
//
// Everything here must produce the same bits as the reference compiled with
// g++ -O3 for x86-64 (no FMA): the translation units that include this header
// are built with -ffp-contract=off and IEEE division/sqrt (see Makefile).
//
// Reference semantics reproduced (file:line into the reference tree):
//   LCG                       rng.h:14-20   state' = 1664525*state + 1013904223 mod 2^32,
//                                           rand01 = (float)state / 2^32 (can be 1.0f)
//   std::min/std::max         aabb.h:24-25  (b<a)?b:a / (a<b)?b:a, and min_element /
//                                           max_element scan order for the 3-way forms,
//                                           so NaN behaves as in the reference
//   |a| < EPS                 triangle.h:31 EPS = 1e-6 is a double; for float |a| the
//                                           compare is exactly |a| < 0x1.0c6f7cp-20f
//   acosf                     glibc 2.35 e_acosf.c (fdlibm), float arithmetic
//   sincosf                   glibc 2.35 s_sincosf.c (double polynomial)
// Both libm restatements equal the host glibc on every input of the path's
// domain (tests/test_math.py); on the GPU they are checked against the oracle.
#pragma once

#if !defined(__HIPCC_RTC__)
#include <stdint.h>
#endif

#if defined(__HIPCC__)
#define PT_HD __host__ __device__ __forceinline__
#else
#define PT_HD inline
#endif

namespace pt {

// ------------------------------------------------------------------ bits
PT_HD uint32_t f2u(float f) { return __builtin_bit_cast(uint32_t, f); }
PT_HD float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }

// ------------------------------------------------------------------ vec3
struct v3 {
    float x, y, z;
};
PT_HD v3 mk(float x, float y, float z) { return v3{x, y, z}; }
PT_HD v3 add(v3 a, v3 b) { return v3{a.x + b.x, a.y + b.y, a.z + b.z}; }
PT_HD v3 sub(v3 a, v3 b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
PT_HD v3 mul(v3 a, v3 b) { return v3{a.x * b.x, a.y * b.y, a.z * b.z}; }
PT_HD v3 scale(v3 a, float s) { return v3{a.x * s, a.y * s, a.z * s}; }
PT_HD v3 neg(v3 a) { return v3{-a.x, -a.y, -a.z}; }
PT_HD float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PT_HD v3 cross(v3 a, v3 b) {
    return v3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// ------------------------------------------------------------------ exact rcp / sqrt
// Correctly rounded 1/a and sqrt(x) in fewer instructions than the IEEE division and
// square-root expansions (12 and 15 VALU ops on gfx950). The fast sequences are exact
// on a range of inputs, established by sweeping EVERY float of that range on the GPU
// (pt_debug_sweep; tests/test_gpu_parity.py::test_fast_exact_math_sweep re-checks all
// 2^32 inputs of the guarded functions on each GPU run); outside it the IEEE operation
// runs (a branch no lane of a wave normally takes).
//   rcp:  v_rcp_f32, then one Newton step with FMA; exact for |a| in [2^-126, 2^126]
//   sqrt: v_sqrt_f32, then the +-1 ulp residual fix-up; exact for x in [2^-100, 2^100]
// On the host (oracle, CPU builds) they are the IEEE operations themselves.
//
// The fallback is chosen once per wave, not per lane (PT_WAVE_GUARD): every lane runs the
// fast sequence, and when ANY active lane's input is out of range the whole wave runs the
// IEEE operation too and keeps that. The two agree on every lane in range, so each lane
// gets the bits the per-lane guard gave it, and the common case is straight-line code: one
// or two compares and a scalar branch instead of a divergent if/else per call, and the
// sequences of neighbouring calls share a basic block, where their v_rcp latencies overlap.
#ifndef PT_WAVE_GUARD
#define PT_WAVE_GUARD 1  // 0: a per-lane branch around every fast sequence (A/B hook)
#endif
#ifndef PT_ACOS_WAVE
#define PT_ACOS_WAVE 1  // 0: acosf_fast with guarded inner operations and a per-lane early-out (A/B hook)
#endif
#ifndef PT_SINCOS_BITS
#define PT_SINCOS_BITS 1  // 0: sincosf_fast with the |y| < 2^-12 selects and compared signs (A/B hook)
#endif

// Whether `p` holds in some active lane of the wave (the one caller on the host).
PT_HD bool wave_any(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_ballot_w64(p) != 0;
#else
    return p;
#endif
}

#if defined(__HIP_DEVICE_COMPILE__)
// The fast sequences themselves, for callers that know the range.
__device__ __forceinline__ float rcp_newton(float a) {  // == 1.0f / a for |a| in [2^-126, 2^126]
    const float r = __builtin_amdgcn_rcpf(a);
    const float e = __builtin_fmaf(-a, r, 1.0f);
    return __builtin_fmaf(e, r, r);
}
__device__ __forceinline__ float sqrt_fixup(float x) {  // == sqrtf(x) for x in [2^-100, 2^100]
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sd = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) - 1u);
    const float su = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) + 1u);
    const float rd = __builtin_fmaf(-sd, s, x), ru = __builtin_fmaf(-su, s, x);
    float r = rd <= 0.0f ? sd : s;
    r = ru > 0.0f ? su : r;
    return r;
}
#endif

PT_HD float rcp_exact(float a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float m = __builtin_fabsf(a);
    const bool out = !(m >= 0x1p-126f && m <= 0x1p126f);
#if PT_WAVE_GUARD
    float f = rcp_newton(a);
    if (__builtin_expect(wave_any(out), 0)) f = 1.0f / a;
    return f;
#else
    if (__builtin_expect(out, 0)) return 1.0f / a;
    return rcp_newton(a);
#endif
#else
    return 1.0f / a;
#endif
}

PT_HD float sqrt_exact(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const bool out = !(x >= 0x1p-100f && x <= 0x1p100f);
#if PT_WAVE_GUARD
    float r = sqrt_fixup(x);
    if (__builtin_expect(wave_any(out), 0)) r = __builtin_sqrtf(x);
    return r;
#else
    if (__builtin_expect(out, 0)) return __builtin_sqrtf(x);
    return sqrt_fixup(x);
#endif
#else
    return __builtin_sqrtf(x);
#endif
}

// inv = 1 / d per component (bvh.h:157): rcp_exact three times with ONE range predicate, so the
// three v_rcp_f32 and their Newton steps interleave in one block. `live`: the lanes whose result
// is used; the others' components (a stale or never-set d) neither start the fallback nor get
// a defined result. kUnit: every live d is a unit vector made by hemisphere_dir, |component| <= 1,
// so the upper bound cannot fail and only the lower one is tested; callers' rays, and directions
// that went through a division (the camera's and the specular sampler's normalize, whose length
// can underflow to 0 and give an infinite component), take the two-sided test.
// A NaN component beside two in range passes the predicate (v_min3 / v_max3 skip NaN): both
// sides then give a NaN, possibly of different payload; inv only ever feeds comparisons.
template <bool kUnit = false>
PT_HD v3 rcp3_exact(v3 d, bool live = true) {
#if defined(__HIP_DEVICE_COMPILE__) && PT_WAVE_GUARD
    const float ax = __builtin_fabsf(d.x), ay = __builtin_fabsf(d.y), az = __builtin_fabsf(d.z);
    bool out = !(__builtin_fminf(__builtin_fminf(ax, ay), az) >= 0x1p-126f);
    if (!kUnit) out = out || !(__builtin_fmaxf(__builtin_fmaxf(ax, ay), az) <= 0x1p126f);
    v3 r{rcp_newton(d.x), rcp_newton(d.y), rcp_newton(d.z)};
    if (__builtin_expect(wave_any(live && out), 0)) r = v3{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    return r;
#else
    (void)live;
    return v3{rcp_exact(d.x), rcp_exact(d.y), rcp_exact(d.z)};
#endif
}

// rcp3_exact that also hands its range predicate to the caller (PT_DOMAIN_ONCE):
// `fell` is whether the wave ran the fallback, i.e. some lane active here failed the predicate (on
// the host, where a lane is its own wave: whether this d failed it). The result has rcp3_exact's
// bits. What !fell proves about every lane active at the call, per component i:
//     inv_i = RN(1 / d_i) is finite and non-zero, and not NaN.
// Proof, kUnit (d is hemisphere_dir's sample, the caller's condition).
//   * d has no NaN and |d_i| <= 1: its components are sin / cos values of finite angles (the angles
//     come from the LCG alone, the normal only picks the sign) and products of two of them;
//     |sin|, |cos| <= 1 as floats (correctly rounded, 1 is a float) and RN(a b) <= 1 for
//     |a|, |b| <= 1 by the monotonicity of rounding.
//   * Without a NaN v_min3_f32 is the true minimum, so min |d_i| >= 2^-126 puts every |d_i| in
//     [2^-126, 1], 1 / |d_i| in [1, 2^126], and RN of it (2^126 and 1 are floats) in the same
//     interval: finite, non-zero, normal.
// Proof, !kUnit (a camera ray, the specular sample: any float may arrive).
//   * The predicate here is s = (|d_x| + |d_y|) + |d_z| <= 2^126 beside the minimum: an addition
//     hands a NaN operand on and v_min3 / v_max3 do not, so a NaN component, which passes
//     rcp3_exact's own two-sided test beside two components in range, fails this one; so does an
//     infinite one. With neither, |d_i| <= s by monotonicity (the other terms are >= 0), and the
//     minimum is the true one: every |d_i| in [2^-126, 2^126], so RN(1 / |d_i|) too.
//   * The sum is stricter than max |d_i| <= 2^126 (by less than two binades); a lane in between
//     takes the IEEE divisions, which give the same bits (rcp_newton is exact on its range).
template <bool kUnit>
PT_HD v3 rcp3_exact_v(v3 d, bool& fell) {
    const float ax = __builtin_fabsf(d.x), ay = __builtin_fabsf(d.y), az = __builtin_fabsf(d.z);
    bool out = !(__builtin_fminf(__builtin_fminf(ax, ay), az) >= 0x1p-126f);
    if (!kUnit) out = out || !((ax + ay) + az <= 0x1p126f);
#if defined(__HIP_DEVICE_COMPILE__) && PT_WAVE_GUARD
    v3 r{rcp_newton(d.x), rcp_newton(d.y), rcp_newton(d.z)};
    fell = wave_any(out);
    if (__builtin_expect(fell, 0)) r = v3{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    return r;
#else
    fell = out;
    return v3{rcp_exact(d.x), rcp_exact(d.y), rcp_exact(d.z)};
#endif
}

// vec3::normalize = *this / length(): three correctly rounded divisions.
PT_HD v3 normalize(v3 a) {
    float len = sqrt_exact(dot(a, a));
    return v3{a.x / len, a.y / len, a.z / len};
}

// a / b given y = RN(1/b) (rcp_exact): q0 = RN(a y), the exact remainder r = a - b q0
// (one FMA), then RN(q0 + r y). Markstein's theorem (P. Markstein, IBM J. Res. Dev. 34(1),
// 1990; Muller et al., Handbook of Floating-Point Arithmetic, §4.7): with y within half an
// ulp of 1/b and q0 within one ulp of a/b, that is the correctly rounded quotient, barring
// underflow / overflow of q0, r and the result — here ruled out by |a|, |b| in
// [2^-60, 2^60] (callers check) — and a = 0 (RN(q0 + r y) would lose the sign of -0).
// Checked on the GPU against IEEE division over 2^32 such pairs (pt_debug_sweep 4).
PT_HD float div_by_rcp(float a, float b, float y) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float q0 = a * y;
    return __builtin_fmaf(__builtin_fmaf(-b, q0, a), y, q0);
#else
    (void)y;
    return a / b;
#endif
}

// vec3::normalize (linalg.h:149-151) with the three divisions by one reciprocal: exact
// when |len| and every nonzero |component| lie in [2^-60, 2^60] and no component is 0
// (div_by_rcp); otherwise the IEEE divisions. Same bits as normalize in every case.
// The wave-uniform form evaluates one predicate: |a|^2 in [2^-100, 2^100] (sqrt_exact's range)
// puts len in [2^-50, 2^50] and every |component| <= len (1 + 2^-22) below 2^60, so the smallest
// |component| >= 2^-60 is all that is left to test; a NaN component makes |a|^2 NaN. One
// reciprocal then feeds the three quotients, and the wave's slow path is the IEEE square root and
// divisions.
PT_HD v3 normalize_fast(v3 a) {
#if defined(__HIP_DEVICE_COMPILE__) && PT_WAVE_GUARD
    const float l2 = dot(a, a);
    const float mn = __builtin_fminf(__builtin_fminf(__builtin_fabsf(a.x), __builtin_fabsf(a.y)), __builtin_fabsf(a.z));
    const bool out = !(l2 >= 0x1p-100f && l2 <= 0x1p100f && mn >= 0x1p-60f);
    const float lf = sqrt_fixup(l2), y = rcp_newton(lf);
    v3 r{div_by_rcp(a.x, lf, y), div_by_rcp(a.y, lf, y), div_by_rcp(a.z, lf, y)};
    if (__builtin_expect(wave_any(out), 0)) {
        const float len = __builtin_sqrtf(l2);
        r = v3{a.x / len, a.y / len, a.z / len};
    }
    return r;
#else
    const float len = sqrt_exact(dot(a, a));
    const float m = __builtin_fminf(__builtin_fminf(__builtin_fabsf(a.x), __builtin_fabsf(a.y)), __builtin_fabsf(a.z));
    const float mx = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(a.x), __builtin_fabsf(a.y)), __builtin_fabsf(a.z));
    if (__builtin_expect(m >= 0x1p-60f && mx <= 0x1p60f && len >= 0x1p-60f && len <= 0x1p60f, 1)) {
        const float y = rcp_exact(len);
        return v3{div_by_rcp(a.x, len, y), div_by_rcp(a.y, len, y), div_by_rcp(a.z, len, y)};
    }
    return v3{a.x / len, a.y / len, a.z / len};
#endif
}

PT_HD float std_max(float a, float b) { return (a < b) ? b : a; }
PT_HD float std_min(float a, float b) { return (b < a) ? b : a; }
PT_HD float std_min3(float a, float b, float c) {
    float r = a;
    r = (b < r) ? b : r;
    r = (c < r) ? c : r;
    return r;
}
PT_HD float std_max3(float a, float b, float c) {
    float r = a;
    r = (r < b) ? b : r;
    r = (r < c) ? c : r;
    return r;
}

// ------------------------------------------------------------------ LCG
struct Lcg {
    uint32_t s;
    PT_HD float next01() {
        // one v_mul_lo_u32: 4.6 cycles per wave-instruction, the cost of any other main-port form
        // (tools/valu_ubench.hip), so a restatement by 24-bit multiplies has nothing to gain
        s = 1664525u * s + 1013904223u;
        return (float)s * 0x1p-32f;  // == (float)s / 2^32 exactly
    }
};

// ------------------------------------------------------------------ AABB slab (aabb.h:20-29)
PT_HD bool slab_hit(v3 lb, v3 rt, v3 o, v3 inv) {
    float t1x = (lb.x - o.x) * inv.x, t1y = (lb.y - o.y) * inv.y, t1z = (lb.z - o.z) * inv.z;
    float t2x = (rt.x - o.x) * inv.x, t2y = (rt.y - o.y) * inv.y, t2z = (rt.z - o.z) * inv.z;
    float tmax = std_min3(std_max(t1x, t2x), std_max(t1y, t2y), std_max(t1z, t2z));
    float tmin = std_max3(std_min(t1x, t2x), std_min(t1y, t2y), std_min(t1z, t2z));
    return !(tmax < 0) && (tmin <= tmax);
}

// Same result as slab_hit whenever inv has no infinite component. Then no slab value
// can be NaN (box and origin are finite, 0 * finite = 0), and without NaN the
// reference's compare-select min/max equal IEEE min/max up to the sign of a zero,
// which neither `tmax < 0` nor `tmin <= tmax` can observe. Lowers to v_min3/v_max3.
PT_HD bool slab_hit_finite(v3 lb, v3 rt, v3 o, v3 inv) {
    float t1x = (lb.x - o.x) * inv.x, t1y = (lb.y - o.y) * inv.y, t1z = (lb.z - o.z) * inv.z;
    float t2x = (rt.x - o.x) * inv.x, t2y = (rt.y - o.y) * inv.y, t2z = (rt.z - o.z) * inv.z;
    float tmax = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(t1x, t2x), __builtin_fmaxf(t1y, t2y)),
                                 __builtin_fmaxf(t1z, t2z));
    float tmin = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(t1x, t2x), __builtin_fminf(t1y, t2y)),
                                 __builtin_fminf(t1z, t2z));
    // !(tmax < 0) && tmin <= tmax  <=>  max(tmin, 0) <= tmax  (no NaN here)
    return __builtin_fmaxf(tmin, 0.0f) <= tmax;
}

PT_HD bool all_finite(v3 a) {
    return __builtin_fabsf(a.x) < __builtin_inff() && __builtin_fabsf(a.y) < __builtin_inff() &&
           __builtin_fabsf(a.z) < __builtin_inff();
}

// Whether ray (o, d) provably fails slab_hit (aabb.h:20-29, inv = 1 / d) for EVERY box
// [lb, rt] inside E = [elb, ert] (elb <= lb <= rt <= ert per axis, no NaN in the boxes):
// on some axis a the origin lies outside E and the direction points away from it,
//     o.a < elb.a and -2 < d.a < 0,   or   o.a > ert.a and 0 < d.a < 2.
// The render kernels use it with E = the union of the leaf boxes that hold an EMIT
// triangle: a rejected ray tests no emitter triangle.
// Proof for the first case (the second mirrors it: both differences are negative, inv.a > 0).
//   * The differences are non-zero: lb.a >= elb.a > o.a and rt.a >= lb.a, so lb.a - o.a
//     and rt.a - o.a are positive reals, and a float subtraction of unequal operands never
//     rounds to zero (denormals are kept); it may round to +inf, which is positive too.
//   * The products do not underflow: inv.a = 1 / d.a is negative with |inv.a| > 1/2
//     (-inf when d.a is a small subnormal). A non-zero x times such a factor has magnitude
//     above 2^-150, which rounds to 2^-149 or more, never to -0 (the only reason for the
//     bound on |d.a|: -0 would pass `tmax < 0`). So t1.a and t2.a are strictly negative
//     (or -inf), neither is NaN, and M_a = max(t1.a, t2.a) < 0.
//   * tmax = std_min3(M_x, M_y, M_z) is a left fold with `<` (std::min of an initializer
//     list). a = x: r starts at M_x < 0 and a later NaN never replaces it (`NaN < r` is
//     false), so tmax <= M_x < 0. a = y: r is M_x; if it is NaN (0 * inf) then `M_y < r` and
//     `M_z < r` are false and tmax is NaN, else r becomes min(M_x, M_y) <= M_y < 0 and stays
//     negative. a = z: r after two steps is NaN (then tmax is NaN) or a number, and the last
//     step gives min(r, M_z) <= M_z < 0. So tmax < 0, which fails `!(tmax < 0)`, or tmax is
//     NaN, which fails `tmin <= tmax`.
//   * NaN in o or d: every comparison below is false, the ray is not rejected. d.a = +-0
//     satisfies neither d.a < 0 nor d.a > 0.
//   * E empty (elb = +inf, ert = -inf: no box to hit): every ray with a non-zero component
//     of magnitude below 2 is rejected, vacuously right.
// The rule never claims a hit; a ray that is not rejected is traced as before.
// Bitwise & and | on purpose: 15 compares and mask operations in a straight line. The
// short-circuit forms compiled to a dozen divergent branches in the kernels' shade section.
PT_HD int emit_reject_axis(float lo, float hi, float o, float d) {
    return (int)(__builtin_fabsf(d) < 2.0f) & (((int)(o < lo) & (int)(d < 0.0f)) | ((int)(o > hi) & (int)(d > 0.0f)));
}
PT_HD bool emit_reject(v3 elb, v3 ert, v3 o, v3 d) {
    return (emit_reject_axis(elb.x, ert.x, o.x, d.x) | emit_reject_axis(elb.y, ert.y, o.y, d.y) |
            emit_reject_axis(elb.z, ert.z, o.z, d.z)) != 0;
}

// Whether ray (o, inv = 1 / d) provably fails slab_hit (aabb.h:20-29) for EVERY box [lb, rt]
// inside E = [elb, ert] (elb <= lb <= rt <= ert per axis, no NaN in the boxes; scene_emit_box
// turns the rule off otherwise): E itself fails the reference's slab test. The flat kernels
// use it in place of emit_reject: it rejects every ray emit_reject rejects
// whenever the guard below holds (tests/test_last_ray_slab.py), and the rays that miss E
// while facing it.
// Guard: every component of inv is finite and non-zero and o is finite. Otherwise the answer
// is "not rejected" and the ray is traced as before (no fallback to the sign rule).
// Proof, for one box B = [lb, rt] inside a non-empty E, under the guard.
//   * No NaN: x - o.a for a plane x is a number (finite, or +-inf when x is infinite or the
//     difference overflows; never inf - inf, o.a is finite), and a number times a finite
//     non-zero inv.a is a number (0 * inf needs a zero or an infinite factor: the only zero
//     is x - o.a = 0, whose other factor is finite).
//   * Monotone: float subtraction and multiplication round monotonically, so f(x) =
//     (x - o.a) * inv.a is non-decreasing in x for inv.a > 0 and non-increasing for inv.a < 0
//     (overflow to +-inf and underflow to +-0 keep the order; -0 and +0 compare equal). With
//     elb.a <= lb.a <= rt.a <= ert.a that gives, for either sign of inv.a,
//         min(t1, t2)_B >= min(t1, t2)_E   and   max(t1, t2)_B <= max(t1, t2)_E.
//   * The folds: without NaN the reference's std::max(a, b) = (a < b) ? b : a, std::min and
//     the left folds of std::min({..}) / std::max({..}) return a value equal (==) to the
//     IEEE maximum / minimum of their operands; they can differ only in the sign of a zero.
//     Minimum and maximum are monotone in every operand, so tmin_B >= tmin_E and
//     tmax_B <= tmax_E as numbers, where the E values are the IEEE ones computed here.
//   * E fails: tmax_E < 0 gives tmax_B <= tmax_E < 0, so B fails `!(tmax < 0)`; tmin_E > tmax_E
//     gives tmin_B >= tmin_E > tmax_E >= tmax_B, so B fails `tmin <= tmax`. Both comparisons are
//     strict and between numbers, so the sign of a zero cannot change either.
//   * A failed box is not entered: BVH::intersect tests none of B's triangles, and an
//     ancestor's box failing only removes more tests.
// NaN in o or inv fails the guard; the claim is a conjunction of comparisons that are false
// for NaN, never the negation of a hit test.
// A flat axis of E (elb.a == ert.a, the Cornell light in y) has t1 == t2: with the box as
// literals the compiler folds that axis' min and max away.
// Bitwise & and | as in emit_reject: straight-line compares, no branches per lane.
PT_HD bool finite_nonzero(float x) { return ((int)(__builtin_fabsf(x) < __builtin_inff()) & (int)(x != 0.0f)) != 0; }
PT_HD bool finite_nonzero3(v3 a) {
    return ((int)finite_nonzero(a.x) & (int)finite_nonzero(a.y) & (int)finite_nonzero(a.z)) != 0;
}
// behind_only: the `tmax < 0` term alone, E lies behind the ray on some axis. Under the guard
// that is emit_reject's condition without its bound on |d|: max(t1, t2) < 0 on axis a means
// both differences are non-zero with the sign opposite to inv.a's, i.e. o.a < elb.a with
// d.a < 0 or o.a > ert.a with d.a > 0, and emit_reject's proof gives the converse for |d.a| < 2.
// The table kernels' sign-only hook runs this (a select on a flag, no second predicate in the
// kernel); the hipRTC scene kernel's runs emit_reject itself.
// inv_ok: the inv half of the guard, made by the caller (emit_slab_reject_nonempty tests inv itself).
PT_HD bool emit_slab_reject_core(v3 elb, v3 ert, v3 o, v3 inv, bool behind_only, bool inv_ok) {
    const int guard = (int)inv_ok & (int)(__builtin_fabsf(o.x) < __builtin_inff()) & (int)(__builtin_fabsf(o.y) < __builtin_inff()) &
                      (int)(__builtin_fabsf(o.z) < __builtin_inff());
    const float t1x = (elb.x - o.x) * inv.x, t1y = (elb.y - o.y) * inv.y, t1z = (elb.z - o.z) * inv.z;
    const float t2x = (ert.x - o.x) * inv.x, t2y = (ert.y - o.y) * inv.y, t2z = (ert.z - o.z) * inv.z;
    const float tmax = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(t1x, t2x), __builtin_fmaxf(t1y, t2y)),
                                       __builtin_fmaxf(t1z, t2z));
    const float tmin = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(t1x, t2x), __builtin_fminf(t1y, t2y)),
                                       __builtin_fminf(t1z, t2z));
    return (guard & ((int)(tmax < 0.0f) | ((int)!behind_only & (int)(tmin > tmax)))) != 0;
}
PT_HD bool emit_slab_reject_nonempty(v3 elb, v3 ert, v3 o, v3 inv, bool behind_only = false) {
    return emit_slab_reject_core(elb, ert, o, inv, behind_only, finite_nonzero3(inv));
}
// E empty (scene_emit_box's encoding of "no emitter leaf": elb = +inf, ert = -inf): there is no
// box to hit, every last ray is rejected, whatever o and inv hold (the slab arithmetic on the
// inverted infinite box would pass it). With the box as literals the test folds at compile
// time; the kernels that take the box as an argument decide it from a flag, wave-uniformly.
PT_HD bool emit_box_empty(v3 elb, v3 ert) {
    return ((int)(elb.x > ert.x) | (int)(elb.y > ert.y) | (int)(elb.z > ert.z)) != 0;
}
PT_HD bool emit_slab_reject(v3 elb, v3 ert, v3 o, v3 inv) {
    return emit_box_empty(elb, ert) ? true : emit_slab_reject_nonempty(elb, ert, o, inv);
}
// emit_slab_reject_given (PT_DOMAIN_ONCE): the caller hands in the inv half of the guard, inv_ok.
// A lane that holds rcp3_exact_v's verdict !fell passes `true`: every component of inv is finite
// and non-zero (the proof is there), so no test of inv is issued; the lanes of a wave that fell
// back pass finite_nonzero3(inv), which makes this the guarded form itself. The o half stays as it
// is: o = (o' + d t) + 1e-4 n rounds three times and
// can overflow for scene coordinates near the top of the float range, which no baked bound rules
// out without a margin; and a form through v_max3_f32 would let a NaN component pass beside two
// finite ones, so the three tests are already the short exact form.
PT_HD bool emit_slab_reject_given(v3 elb, v3 ert, v3 o, v3 inv, bool inv_ok) {
    return emit_box_empty(elb, ert) ? true : emit_slab_reject_core(elb, ert, o, inv, false, inv_ok);
}

// ------------------------------------------------------------------ Möller–Trumbore (triangle.h:25-44)
// e1 = v2 - v1 and e2 = v3 - v1 are precomputed on the host with the same float ops.
PT_HD bool tri_hit(v3 v1, v3 e1, v3 e2, v3 o, v3 d, float& t) {
    v3 h = cross(d, e2);
    float a = dot(e1, h);
    // (double)|a| < 1e-6  <=>  |a| <= 1e-6f (0x1.0c6f7ap-20)  <=>  |a| < 0x1.0c6f7cp-20f
    if (__builtin_fabsf(a) < 0x1.0c6f7cp-20f) return false;
    float f = rcp_exact(a);
    v3 s = sub(o, v1);
    float u = f * dot(s, h);
    if (u < 0.0f || u > 1.0f) return false;
    v3 q = cross(s, e1);
    float v = f * dot(d, q);
    if (v < 0.0f || u + v > 1.0f) return false;
    t = f * dot(e2, q);
    return t > 0.0f;
}

// tri_hit with the same operations and the same result, for lanes that all run the whole
// test (the flat path's pair rounds: 64 different (ray, triangle) pairs, so no early exit
// is ever taken by a whole wave): no branches, and 1/a without the range guard. Requires
// |a| <= 2^126: a = e1 . (d x e2) with |d| ~ 1, so |a| < 2^124 whenever every vertex
// coordinate is below 2^60 in magnitude (the host checks before enabling it); |a| below
// the EPS threshold only clears `ok`. NaN behaves as in tri_hit: every rejection is a
// comparison that is false for NaN, so a NaN u or v passes through to `t > 0`.
PT_HD bool tri_hit_nb(v3 v1, v3 e1, v3 e2, v3 o, v3 d, float& t) {
    v3 h = cross(d, e2);
    float a = dot(e1, h);
    const bool ok = !(__builtin_fabsf(a) < 0x1.0c6f7cp-20f);
#if defined(__HIP_DEVICE_COMPILE__)
    const float r = __builtin_amdgcn_rcpf(a);
    const float f = __builtin_fmaf(__builtin_fmaf(-a, r, 1.0f), r, r);  // rcp_exact's fast branch
#else
    const float f = 1.0f / a;
#endif
    v3 s = sub(o, v1);
    float u = f * dot(s, h);
    v3 q = cross(s, e1);
    float v = f * dot(d, q);
    t = f * dot(e2, q);
    return ok && !(u < 0.0f || u > 1.0f) && !(v < 0.0f || u + v > 1.0f) && t > 0.0f;
}

// ------------------------------------------------------------------ acosf (fdlibm)
// The restatement: glibc's float acosf (fdlibm e_acosf.c) as g++ compiles it for the
// reference (IEEE division and sqrt, no FMA).
PT_HD float acosf_ref(float x) {
    const float pi = 3.1415925026e+00f, pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f;
    const float p0 = 1.6666667163e-01f, p1 = -3.2556581497e-01f, p2 = 2.0121252537e-01f,
                p3 = -4.0055535734e-02f, p4 = 7.9153501429e-04f, p5 = 3.4793309169e-05f;
    const float q1 = -2.4033949375e+00f, q2 = 2.0209457874e+00f, q3 = -6.8828397989e-01f,
                q4 = 7.7038154006e-02f;
    const uint32_t ux = f2u(x), ax = ux & 0x7fffffffu;
    if (ax >= 0x3f800000u) {
        if (ax == 0x3f800000u) return (ux >> 31) ? pi + 2.0f * pio2_lo : 0.0f;
        return (x - x) / (x - x);
    }
    if (ax < 0x3f000000u) {  // |x| < 0.5
        if (ax <= 0x32800000u) return pio2_hi + pio2_lo;
        float z = x * x;
        float p = z * (p0 + z * (p1 + z * (p2 + z * (p3 + z * (p4 + z * p5)))));
        float q = 1.0f + z * (q1 + z * (q2 + z * (q3 + z * q4)));
        float r = p / q;
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if (ux >> 31) {  // x <= -0.5
        float z = (1.0f + x) * 0.5f;
        float p = z * (p0 + z * (p1 + z * (p2 + z * (p3 + z * (p4 + z * p5)))));
        float q = 1.0f + z * (q1 + z * (q2 + z * (q3 + z * q4)));
        float s = __builtin_sqrtf(z);
        float r = p / q;
        float w = r * s - pio2_lo;
        return pi - 2.0f * (s + w);
    }
    // x >= 0.5
    float z = (1.0f - x) * 0.5f;
    float s = __builtin_sqrtf(z);
    float df = u2f(f2u(s) & 0xfffff000u);
    float c = (z - df * df) / (s + df);
    float p = z * (p0 + z * (p1 + z * (p2 + z * (p3 + z * (p4 + z * p5)))));
    float q = 1.0f + z * (q1 + z * (q2 + z * (q3 + z * q4)));
    float r = p / q;
    float w = r * s + c;
    return 2.0f * (df + w);
}

// Device form: the three cases of acosf_ref as one instruction stream (every lane runs
// the polynomial, both divisions and the sqrt once; the case picks the result), each
// division as the exact reciprocal + one Markstein correction (div_by_rcp) and the exact sqrt. Not
// claimed for every (p, q) — but acosf_fast(x) == acosf_ref(x) for EVERY float x in
// [-1, 1], the whole domain the path reaches (argument 2u - 1, material.h:9), by
// exhaustive GPU sweep (pt_debug_sweep 2, tests/test_gpu_parity.py). Cases split over a
// wave otherwise cost the sum of the three branches.
PT_HD float acosf_fast(float x) {
    const float pi = 3.1415925026e+00f, pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f;
    const float p0 = 1.6666667163e-01f, p1 = -3.2556581497e-01f, p2 = 2.0121252537e-01f,
                p3 = -4.0055535734e-02f, p4 = 7.9153501429e-04f, p5 = 3.4793309169e-05f;
    const float q1 = -2.4033949375e+00f, q2 = 2.0209457874e+00f, q3 = -6.8828397989e-01f,
                q4 = 7.7038154006e-02f;
    const uint32_t ux = f2u(x), ax = ux & 0x7fffffffu;
    const bool edge = ax >= 0x3f800000u || ax <= 0x32800000u;  // |x| >= 1, tiny
#if !(defined(__HIP_DEVICE_COMPILE__) && PT_ACOS_WAVE)
    if (__builtin_expect(edge, 0)) return acosf_ref(x);
#endif
    const bool small = ax < 0x3f000000u;
    // 1 + x for x <= -0.5 and 1 - x for x >= 0.5 are both 1 - |x|
    const float z = small ? x * x : (1.0f - u2f(ax)) * 0.5f;
    const float p = z * (p0 + z * (p1 + z * (p2 + z * (p3 + z * (p4 + z * p5)))));
    const float q = 1.0f + z * (q1 + z * (q2 + z * (q3 + z * q4)));
    const float zs = small ? 0.25f : z;  // |x| < 0.5 uses neither s nor c
#if defined(__HIP_DEVICE_COMPILE__) && PT_ACOS_WAVE
    // No inner guards: for every x with 2^-26 < |x| < 1 the operands stay far inside the fast
    // sequences' ranges, q in [0.515, 1], zs in [2^-25, 0.25], s + df in [3.4e-4, 1]
    // (tests/test_exact_guards_cpu.py recomputes them over the sampler's whole grid; the
    // exhaustive sweep checks the result on every float). The edge inputs run the same stream
    // (any value, no trap) and, once per wave that holds one, take fdlibm's constants.
    const float r = div_by_rcp(p, q, rcp_newton(q));
    const float s = sqrt_fixup(zs);
#else
    const float r = div_by_rcp(p, q, rcp_exact(q));
    const float s = sqrt_exact(zs);
#endif
    const float df = u2f(f2u(s) & 0xfffff000u);
    const float sd = s + df;
#if defined(__HIP_DEVICE_COMPILE__) && PT_ACOS_WAVE
    const float c = div_by_rcp(zs - df * df, sd, rcp_newton(sd));
#else
    const float c = div_by_rcp(zs - df * df, sd, rcp_exact(sd));
#endif
    const float v_small = pio2_hi - (x - (pio2_lo - x * r));
    const float v_neg = pi - 2.0f * (s + (r * s - pio2_lo));
    const float v_pos = 2.0f * (df + (r * s + c));
    float v = small ? v_small : ((ux >> 31) ? v_neg : v_pos);
#if defined(__HIP_DEVICE_COMPILE__) && PT_ACOS_WAVE
    if (__builtin_expect(wave_any(edge), 0)) {
        if (ax > 0x3f800000u) v = (x - x) / (x - x);
        else if (ax == 0x3f800000u) v = (ux >> 31) ? pi + 2.0f * pio2_lo : 0.0f;
        else if (ax <= 0x32800000u) v = pio2_hi + pio2_lo;
    }
#endif
    return v;
}

// ------------------------------------------------------------------ sincosf (double kernel)
// The restatement: glibc's sincosf (the double-precision polynomial kernel, no FMA as
// g++ compiles it for x86-64). Valid for |y| < 120 (top12 < 0x42F); the path only
// evaluates |y| <= 2*pi.
PT_HD void sincosf_ref(float y, float& sin_out, float& cos_out) {
    const uint32_t t12 = (f2u(y) >> 20) & 0x7ffu;
    double x = (double)y;
    int n = 0;
    double csign = 1.0;
    if (t12 < 0x3f4u) {  // |y| < pi/4
        if (t12 < 0x398u) {  // |y| < 2^-12
            sin_out = y;
            cos_out = 1.0f;
            return;
        }
    } else {
        double r = x * 0x1.45F306DC9C883p+23;  // 2/pi * 2^24
        n = ((int32_t)r + 0x800000) >> 24;
        x = -(double)n * 0x1.921FB54442D18p0 + x;  // x - n * pi/2
        if ((n & 3) == 1 || (n & 3) == 2) x = -x;  // sign[n & 3] = {1,-1,-1,1}
        // sincos_poly is called with (x * s, x * x): x2 uses the unsigned x, same value.
        if (n & 2) csign = -1.0;
    }
    const double c0 = csign * 0x1p0, c1 = csign * -0x1.ffffffd0c621cp-2,
                 c2 = csign * 0x1.55553e1068f19p-5, c3 = csign * -0x1.6c087e89a359dp-10,
                 c4 = csign * 0x1.99343027bf8c3p-16;
    const double s1c = -0x1.555545995a603p-3, s2c = 0x1.1107605230bc4p-7, s3c = -0x1.994eb3774cf24p-13;
    double x2 = x * x;
    double x4 = x2 * x2, x3 = x2 * x;
    double cc2 = x2 * c4 + c3, ss1 = x2 * s3c + s2c;
    double cc1 = x2 * c1 + c0, x5 = x3 * x2, x6 = x4 * x2;
    double s = x3 * s1c + x, c = x4 * c2 + cc1;
    float sv = (float)(x5 * ss1 + s), cv = (float)(x6 * cc2 + c);
    if (n & 1) {
        sin_out = cv;
        cos_out = sv;
    } else {
        sin_out = sv;
        cos_out = cv;
    }
}

// Device form: one instruction stream for every y — the range reduction runs
// for |y| < pi/4 too, where it yields n = 0 and x unchanged, i.e. the unreduced case —
// with the double polynomial and the reduction FMA-contracted (glibc's own
// __sincosf_fma variant does the same on FMA hosts), and the cosine's sign applied to
// the result (rounding is symmetric, so the polynomial of the negated coefficients is
// the negated polynomial; the cosine term is never 0 here). sincosf_fast ==
// sincosf_ref for EVERY float in [-2, 7] (theta in [-pi/2, pi/2], phi in [0, 2*pi]),
// by exhaustive GPU sweep (pt_debug_sweep 3).
PT_HD void sincosf_fast(float y, float& sin_out, float& cos_out) {
    const double y0 = (double)y;
    const double rr = y0 * 0x1.45F306DC9C883p+23;  // 2/pi * 2^24
    const int n = ((int32_t)rr + 0x800000) >> 24;
    double x = __builtin_fma(-(double)n, 0x1.921FB54442D18p0, y0);
#if PT_SINCOS_BITS
    // The sine polynomial is odd in x and the cosine's even, and rounding is symmetric: the
    // reduction's sign flip ((n & 3) == 1 or 2: bit 1 of n + 1) goes to the sine's sign bit at the
    // end instead of a compare and a 64-bit select here.
    const uint32_t sin_sign = (uint32_t)(__builtin_bit_cast(uint64_t, x) >> 32) ^ (((uint32_t)n + 1u) << 30);
#else
    if ((n & 3) == 1 || (n & 3) == 2) x = -x;
#endif
    const double c0 = 0x1p0, c1 = -0x1.ffffffd0c621cp-2, c2 = 0x1.55553e1068f19p-5, c3 = -0x1.6c087e89a359dp-10,
                 c4 = 0x1.99343027bf8c3p-16;
    const double s1c = -0x1.555545995a603p-3, s2c = 0x1.1107605230bc4p-7, s3c = -0x1.994eb3774cf24p-13;
    const double x2 = x * x;
    const double x4 = x2 * x2, x3 = x2 * x;
    const double cc2 = __builtin_fma(x2, c4, c3), ss1 = __builtin_fma(x2, s3c, s2c);
    const double cc1 = __builtin_fma(x2, c1, c0), x5 = x3 * x2, x6 = x4 * x2;
    const double s = __builtin_fma(x3, s1c, x), c = __builtin_fma(x4, c2, cc1);
#if PT_SINCOS_BITS
    // The signs by bit field insert: the sine takes the reduced x's sign and the flip (so -0
    // stays -0, which the sum x3 s1c + x loses), the cosine, positive on |x| <= pi/4, bit 1 of n.
    // No test for |y| < 2^-12, where glibc returns (y, 1): there n = 0 and the polynomials give
    // y - y^3/6 and 1 - y^2/2, less than half an ulp from y and from 1 (y^2/6 < 2^-26.5 relative,
    // y^2/2 < 2^-25), subnormal y included; the exhaustive sweep covers all of them.
    const float sv = __builtin_copysignf((float)__builtin_fma(x5, ss1, s), u2f(sin_sign));  // v_bfi_b32
    const float cv = __builtin_copysignf((float)__builtin_fma(x6, cc2, c), u2f((uint32_t)n << 30));
    const bool swap = (n & 1) != 0;
    sin_out = swap ? cv : sv;
    cos_out = swap ? sv : cv;
#else
    const float sv = (float)__builtin_fma(x5, ss1, s);
    float cv = (float)__builtin_fma(x6, cc2, c);
    if (n & 2) cv = -cv;
    const bool swap = (n & 1) != 0, tiny = ((f2u(y) >> 20) & 0x7ffu) < 0x398u;  // |y| < 2^-12: (y, 1)
    sin_out = tiny ? y : (swap ? cv : sv);
    cos_out = tiny ? 1.0f : (swap ? sv : cv);
#endif
}

// What the path calls: the fast forms on the device, the restatements on the host.
#if defined(__HIP_DEVICE_COMPILE__)
constexpr bool kFastLibm = true;
#else
constexpr bool kFastLibm = false;
#endif
PT_HD float acosf_path(float x) { return kFastLibm ? acosf_fast(x) : acosf_ref(x); }
PT_HD void sincosf_path(float y, float& s, float& c) {
    if (kFastLibm) sincosf_fast(y, s, c);
    else sincosf_ref(y, s, c);
}

// ------------------------------------------------------------------ BRDF (material.h:6-25)
// hemisphere_sample: u first, then v (separate declarators are sequenced).
PT_HD v3 hemisphere_dir(Lcg& g, v3 n) {
    float u = g.next01();
    float v = g.next01();
#ifdef PT_EXP_CHEAP_LIBM  // timing experiment only (wrong images): hardware approximations
    float theta = (float)((double)acosf(2.0f * u - 1.0f) - 1.57079632679489661923);
    float phi = (float)(6.28318530717958647692 * (double)v);
    float st = __sinf(theta), ct = __cosf(theta), sp = __sinf(phi), cp = __cosf(phi);
#else
    float theta = (float)((double)acosf_path(2.0f * u - 1.0f) - 1.57079632679489661923);  // - M_PI_2
    float phi = (float)(6.28318530717958647692 * (double)v);                                // 2 * M_PI * v
    float st, ct, sp, cp;
    sincosf_path(theta, st, ct);
    sincosf_path(phi, sp, cp);
#endif
    v3 smp = v3{ct * cp, ct * sp, st};
    return dot(smp, n) < 0.0f ? neg(smp) : smp;
}

// hemisphere_sample's theta part by table: theta = acosf(x) - M_PI_2 for x = 2u - 1, and
// its sine and cosine, depend on x alone, and x = fl(2u - 1) for every u the LCG yields
// (rand01 = (float)state / 2^32) lies on the grid k 2^-24 of [-1, 1] (all 2^32 states
// checked: tests/test_math.py), so (sin theta, cos theta) for all 2^25 + 1 grid values fit
// one table, built on the device by the same exact functions (pt_theta_table_kernel).
// Index of x in it: x 2^24 + 2^24 (both steps exact).
PT_HD int theta_index(float x) { return (int)(x * 0x1p24f) + (1 << 24); }
constexpr int kThetaEntries = (1 << 25) + 1;

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
// hemisphere_dir with (sin theta, cos theta) from the table: u, then v, as the reference
// draws them; phi's sincosf is computed. Same bits as hemisphere_dir.
__device__ __forceinline__ v3 hemisphere_dir_tab(Lcg& g, v3 n, const float2* __restrict__ tab) {
    float u = g.next01();
    float v = g.next01();
    const float2 sct = tab[theta_index(2.0f * u - 1.0f)];  // (sin theta, cos theta)
    float phi = (float)(6.28318530717958647692 * (double)v);  // 2 * M_PI * v
    float sp, cp;
    sincosf_path(phi, sp, cp);
    v3 smp = v3{sct.y * cp, sct.y * sp, sct.x};
    return dot(smp, n) < 0.0f ? neg(smp) : smp;
}
#endif

// specular_sample: vec3(rand01(), rand01(), rand01()) is evaluated right to left by
// g++, so the first draw is z. Returns false if the rejection loop hit `max_iter`.
PT_HD bool specular_dir(Lcg& g, v3 d, v3 n, float rough, int max_iter, v3& out) {
    v3 refl = sub(d, scale(n, 2.0f * dot(d, n)));
    v3 ret;
    int it = 0;
    do {
        float jz = g.next01();
        float jy = g.next01();
        float jx = g.next01();
        v3 j = v3{(jx - 0.5f) * rough, (jy - 0.5f) * rough, (jz - 0.5f) * rough};
        ret = add(refl, j);
        if (++it >= max_iter) {
            out = normalize(ret);
            return false;
        }
    } while (dot(ret, n) < 0.0f);
    out = normalize(ret);
    return true;
}

}  // namespace pt
