// pt_moments.h — the convergence criterion of the sample moments (include/pt_hip.h), stated once
// for the host form (pt_moments_unconverged, pt_host.cpp), the device reduction
// (pt_unconverged_kernel, pt_kernel.hip) and the active-list compaction (pt_adaptive.hip). Both are built with -ffp-contract=off, so every
// operation below is rounded on its own and the two counts are equal.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PT_MOM_FN static inline __host__ __device__
#else
#define PT_MOM_FN static inline
#endif

namespace pt {

// n >= 2 samples of one channel with sum S and sum of squares Q: n*Q - S*S <= (n-1) * t*t,
// t = rel*|S| + abs*n, in the contract's order. A NaN on either side compares false.
PT_MOM_FN bool moments_channel_converged(double S, double Q, double n, double rel, double abs_tol) {
    const double a = n * Q;
    const double b = S * S;
    const double l = a - b;
    const double t = rel * fabs(S) + abs_tol * n;
    const double r = (n - 1.0) * (t * t);
    return l <= r;
}

// A pixel (three channels at S[0..2], Q[0..2]) is unconverged unless every channel is converged.
PT_MOM_FN bool moments_pixel_unconverged(const double* S, const double* Q, int n, double rel, double abs_tol) {
    if (n < 2) return true;
    const double dn = (double)n;
    return !(moments_channel_converged(S[0], Q[0], dn, rel, abs_tol) &&
             moments_channel_converged(S[1], Q[1], dn, rel, abs_tol) &&
             moments_channel_converged(S[2], Q[2], dn, rel, abs_tol));
}

#if defined(__HIPCC__)
// A pixel's running sums as slab_walk's accumulator (pt_trace.h; device code) in a moments
// render (pt_accumulate_moments_kernel, pt_adaptive_accumulate_kernel): the image's float32 sum (SumF32's) and, per channel beside it, S = sum of (double)r and Q = sum of
// (double)r * (double)r (include/pt_hip.h: pt_moments; the product of two floats is exact in
// double, every addition is rounded on its own). A +0 record (a slot the parallel walk pads
// with) changes none of them.
struct MomentSums {
    float &x, &y, &z;
    double sx, sy, sz, qx, qy, qz;
    __device__ __forceinline__ void add(const float3 v) {
        x += v.x;
        y += v.y;
        z += v.z;
        const double dx = (double)v.x, dy = (double)v.y, dz = (double)v.z;
        sx += dx;
        sy += dy;
        sz += dz;
        qx += dx * dx;
        qy += dy * dy;
        qz += dz * dz;
    }
};
#endif

}  // namespace pt
