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

// What a visible light adds: ((T o color) o emit) g.
PT_HD v3 nee_direct(v3 T, v3 color, v3 emit, float g) { return scale(mul(mul(T, color), emit), g); }

// L += T o emit (an emitter reached by the BRDF sample, or a bounce material's own emission).
PT_HD v3 nee_add_emit(v3 L, v3 T, v3 emit) { return add(L, mul(T, emit)); }

// The throughput after a bounce with cosine c = n . new_d: T = ((2 T) o color) c.
PT_HD v3 nee_throughput(v3 T, v3 color, float c) { return scale(mul(scale(T, 2.0f), color), c); }

}  // namespace pt
