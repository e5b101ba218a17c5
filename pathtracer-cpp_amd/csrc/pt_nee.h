// pt_nee.h — the arithmetic of the light-sampling estimator (include/pt_hip.h: the header text is
// the definition), stated once for the host form (pt_bvh_trace_nee, pt_host.cpp) and the kernels
// (pt_nee.hip). Both are built with -ffp-contract=off and correctly rounded division, so every
// operation below is rounded on its own and the two return the same bits.
//
// A light is a row of the scene's light table (LightTable, pt_internal.h): its running area sum,
// the caller's triangle index and five vectors {v1, e1, e2, unit normal, emit_color}. The table is
// made on the host (scene_light_table); the kernels read a copy of it.
#pragma once

#include "pt_math.h"

namespace pt {

// The first light j with cdf[j] > xa, the last one when there is none (rand01 can return 1.0f, and
// xa = x1 * A can then equal A). cdf is non-decreasing: a running sum of positive terms. count >= 1.
PT_HD int nee_pick(const float* cdf, int count, float xa) {
    int lo = 0, hi = count - 1;  // the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > xa) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The point of the light (u, v) = (x2, x3) selects, folded into the triangle: y = v1 + u e1 + v e2.
PT_HD v3 nee_point(v3 v1, v3 e1, v3 e2, float x2, float x3) {
    float u = x2, v = x3;
    if (u + v > 1.0f) {
        u = 1.0f - u;
        v = 1.0f - v;
    }
    return add(add(v1, scale(e1, u)), scale(e2, v));
}

// The connection from the shifted hit point o (normal n, faced) to the point y of a light with
// unit normal nl: w = y - o (the shadow segment's direction, unnormalised), and whether the two
// cosines and the squared distance allow a contribution; g = ((cx / r2) (cy / r2)) kA then.
PT_HD bool nee_connect(v3 y, v3 o, v3 n, v3 nl, float kA, v3& w, float& g) {
    w = sub(y, o);
    const float cx = dot(n, w);
    const float cy = __builtin_fabsf(dot(nl, w));
    const float r2 = dot(w, w);
    g = 0.0f;
    if (!(cx > 0.0f && cy > 0.0f && r2 > 0.0f)) return false;
    g = ((cx / r2) * (cy / r2)) * kA;
    return true;
}

// ---- the balance-heuristic weights (PT_NEE_MIS_BALANCE). hA = A / 2 pi is an exact scaling of kA.
// Both are written as 1 / (1 + ratio of the densities), so an operand that overflows or underflows
// gives a weight of 0 or 1 and never inf / inf (the header text gives the ranges).
PT_HD float nee_half_area(float kA) { return 0.5f * kA; }

// nee_connect with the light's weight folded into g: g = (((cx / r2) a) kA) wl, a = cy / r2,
// s = sqrtf(r2), wl = 1 / (1 + (a hA) / s). Same w and same return value as nee_connect.
PT_HD bool nee_connect_mis(v3 y, v3 o, v3 n, v3 nl, float kA, v3& w, float& g) {
    w = sub(y, o);
    const float cx = dot(n, w);
    const float cy = __builtin_fabsf(dot(nl, w));
    const float r2 = dot(w, w);
    g = 0.0f;
    if (!(cx > 0.0f && cy > 0.0f && r2 > 0.0f)) return false;
    const float a = cy / r2;
    const float s = __builtin_sqrtf(r2);
    const float wl = 1.0f / (1.0f + (a * nee_half_area(kA)) / s);
    g = (((cx / r2) * a) * kA) * wl;
    return true;
}

// The weight of an EMIT hit at distance t along the unit direction d on a listed triangle of unit
// normal nh (not faced): a = |nh . d| / t, wb = 1 / (1 + t / (a hA)). t > 0 on a hit.
PT_HD float nee_brdf_weight(v3 nh, v3 d, float t, float kA) {
    const float a = __builtin_fabsf(dot(nh, d)) / t;
    return 1.0f / (1.0f + t / (a * nee_half_area(kA)));
}

// L += (T o emit) wb (the weighted EMIT hit).
PT_HD v3 nee_add_emit_weighted(v3 L, v3 T, v3 emit, float wb) { return add(L, scale(mul(T, emit), wb)); }

// What a visible light adds: ((T o color) o emit) g.
PT_HD v3 nee_direct(v3 T, v3 color, v3 emit, float g) { return scale(mul(mul(T, color), emit), g); }

// L += T o emit (an emitter reached by the BRDF sample, or a bounce material's own emission).
PT_HD v3 nee_add_emit(v3 L, v3 T, v3 emit) { return add(L, mul(T, emit)); }

// The throughput after a bounce with cosine c = n . new_d: T = ((2 T) o color) c.
PT_HD v3 nee_throughput(v3 T, v3 color, float c) { return scale(mul(scale(T, 2.0f), color), c); }

// ---- the estimator's material gradients (pt_hip.h: "material gradients of the light-sampling
// estimator"). Two forms carry every term: (a o b) g, and nee_throughput's ((2 a) o b) c, which is
// also the throughput pass Tw_{k+1} and the colour term ((2 Tw_k) o R_{k+1}) c_k.
// (a o b) g: D_k = (color o emit_j) g, d emit_j += (Tw o color) g, d color += (Tw o emit_j) g.
PT_HD v3 nee_pair(v3 a, v3 b, float g) { return scale(mul(a, b), g); }

// R_k from R_{k+1}: (emit + D) + ((2 R) o color) c with a visible light (lit), emit + ... without.
PT_HD v3 nee_suffix(v3 emit, v3 color, float c, v3 R, bool lit, v3 emit_j, float g) {
    const v3 e = lit ? add(emit, nee_pair(color, emit_j, g)) : emit;
    return add(e, nee_throughput(R, color, c));
}

// The terminal of a path: none (a miss or a dropped hit), a hit with m = 1, a weighted hit.
enum { kNeeEndNone = 0, kNeeEndPlain = 1, kNeeEndWeighted = 2 };
// R_K, and what the terminal adds to d emit of its triangle (kind != kNeeEndNone).
PT_HD v3 nee_end_value(int kind, v3 emit, float m) {
    return kind == kNeeEndNone ? v3{0.0f, 0.0f, 0.0f} : kind == kNeeEndPlain ? emit : scale(emit, m);
}
PT_HD v3 nee_end_term(int kind, v3 Tw, float m) { return kind == kNeeEndWeighted ? scale(Tw, m) : Tw; }

}  // namespace pt
