// pt_moments.h — the convergence criterion of the sample moments (include/pt_hip.h), stated once
// for the host form (pt_moments_unconverged, pt_host.cpp) and the device reduction
// (pt_unconverged_kernel, pt_kernel.hip). Both are built with -ffp-contract=off, so every
// operation below is rounded on its own and the two counts are equal.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
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

}  // namespace pt
