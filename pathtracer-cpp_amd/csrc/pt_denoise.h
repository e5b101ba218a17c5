// pt_denoise.h — the arithmetic of the a-trous denoiser (include/pt_hip.h: the header text is the
// definition), stated once for the host form (pt_image_denoise, pt_host.cpp) and the kernels
// (pt_denoise.hip). Both are built with -ffp-contract=off and correctly rounded division and
// square root, so every operation below is rounded on its own and the two return the same bits.
//
// A pixel is read as four 16-byte records, made once per call by the pack step:
//   nt  {n.xyz, tau = sigma_z * t}        guides, the same for every pass
//   xc  {X.xyz, class (0, 1 or 2)}        guides, the same for every pass
//   col {c.rgb, l(c)}                     ping-pong: a pass writes the luminance of its result
//   var {v.rgb, 0}                        ping-pong, only with a variance
// so a tap costs four 16-byte loads. `Src` is where they come from: global memory, an LDS tile,
// or the host's arrays.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PT_DN_FN static inline __host__ __device__ __attribute__((always_inline))
#define PT_DN_MEMBER inline __host__ __device__ __attribute__((always_inline))
#else
#define PT_DN_FN static inline
#define PT_DN_MEMBER inline
#endif

namespace pt {

struct alignas(16) DnRec {
    float x, y, z, w;
};

constexpr int kDnMaxPasses = 8;
constexpr int kDnMaxPowLog2 = 10;

// pt_denoise_params with its defaults filled in and checked.
struct DnParams {
    int passes, npow;
    float sigma_l, sigma_z, eps;
};

PT_DN_FN float dn_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return ((ax * bx) + (ay * by)) + (az * bz);
}

PT_DN_FN float dn_lum(float r, float g, float b) { return ((0.25f * r) + (0.5f * g)) + (0.25f * b); }

// Class of a pixel: 0 miss, 2 emitter, 1 any other hit.
PT_DN_FN float dn_class(int32_t tri, float er, float eg, float eb) {
    if (tri < 0) return 0.0f;
    return (er != 0.0f || eg != 0.0f || eb != 0.0f) ? 2.0f : 1.0f;
}

// The variance of the mean of one channel from its moments.
PT_DN_FN float dn_variance(double S, double Q, int n) {
    if (n < 2) return __builtin_inff();
    const double dn = (double)n;
    const double m = (S * S) / dn;
    double d = (Q - m) / (dn - 1.0);
    d = d > 0.0 ? d : 0.0;
    return (float)(d / dn);
}

// den_p: the 3x3 prefiltered variance around (x, y) as a luminance tolerance.
template <class Src>
PT_DN_FN float dn_den(const Src& src, int W, int H, int x, int y, float sigma_l, float eps) {
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, wacc = 0.0f;
    for (int j = -1; j <= 1; j++) {
        const int yy = y + j;
        if (yy < 0 || yy >= H) continue;
        const float gj = j == 0 ? 0.5f : 0.25f;
        for (int k = -1; k <= 1; k++) {
            const int xx = x + k;
            if (xx < 0 || xx >= W) continue;
            const float g = gj * (k == 0 ? 0.5f : 0.25f);
            const DnRec v = src.var(xx, yy);
            ar += g * v.x;
            ag += g * v.y;
            ab += g * v.z;
            wacc += g;
        }
    }
    const float sig = ((0.25f * sqrtf(ar / wacc)) + (0.5f * sqrtf(ag / wacc))) + (0.25f * sqrtf(ab / wacc));
    return (sigma_l * sig) + eps;
}

// One pass at stride s for pixel (x, y): the new colour record and, with kVar, variance record.
template <bool kVar, class Src>
PT_DN_FN void dn_pixel(const Src& src, int W, int H, int x, int y, int s, const DnParams& P, DnRec& c_out,
                       DnRec& v_out) {
    const DnRec np = src.nt(x, y);
    const DnRec xp = src.xc(x, y);
    const DnRec cp = src.col(x, y);
    const float tau = np.w, cls = xp.w, lp = cp.w;
    float den = 0.0f;
    if (kVar) den = dn_den(src, W, H, x, y, P.sigma_l, P.eps);
    float A0 = 0.0f, A1 = 0.0f, A2 = 0.0f, B0 = 0.0f, B1 = 0.0f, B2 = 0.0f, wsum = 0.0f;
    for (int j = -2; j <= 2; j++) {
        const int yy = y + j * s;
        if (yy < 0 || yy >= H) continue;
        const float hj = j == 0 ? 0.375f : (j == -1 || j == 1) ? 0.25f : 0.0625f;
        for (int k = -2; k <= 2; k++) {
            const int xx = x + k * s;
            if (xx < 0 || xx >= W) continue;
            const float hh = hj * (k == 0 ? 0.375f : (k == -1 || k == 1) ? 0.25f : 0.0625f);
            float w = 1.0f;
            DnRec cq = cp;
            if (j != 0 || k != 0) {
                const DnRec xq = src.xc(xx, yy);
                if (xq.w != cls) continue;
                cq = src.col(xx, yy);
                float wg = 1.0f;
                if (cls != 0.0f) {
                    const DnRec nq = src.nt(xx, yy);
                    float dn = dn_dot(np.x, np.y, np.z, nq.x, nq.y, nq.z);
                    dn = dn > 0.0f ? dn : 0.0f;
                    for (int i = 0; i < P.npow; i++) dn = dn * dn;
                    const float dl = fabsf(dn_dot(np.x, np.y, np.z, xq.x - xp.x, xq.y - xp.y, xq.z - xp.z));
                    const float wz = (dl < tau) ? (tau - dl) / tau : 0.0f;
                    wg = dn * wz;
                }
                float wl = 1.0f;
                if (kVar) {
                    const float xl = fabsf(lp - cq.w) / den;
                    wl = 1.0f / (1.0f + xl * xl);
                }
                w = wg * wl;
                if (!(w > 0.0f)) continue;
            }
            const float kq = hh * w;
            A0 += kq * cq.x;
            A1 += kq * cq.y;
            A2 += kq * cq.z;
            if (kVar) {
                const DnRec vq = src.var(xx, yy);
                const float k2 = kq * kq;
                B0 += k2 * vq.x;
                B1 += k2 * vq.y;
                B2 += k2 * vq.z;
            }
            wsum += kq;
        }
    }
    c_out.x = A0 / wsum;
    c_out.y = A1 / wsum;
    c_out.z = A2 / wsum;
    c_out.w = dn_lum(c_out.x, c_out.y, c_out.z);
    if (kVar) {
        const float w2 = wsum * wsum;
        v_out.x = B0 / w2;
        v_out.y = B1 / w2;
        v_out.z = B2 / w2;
        v_out.w = 0.0f;
    }
}

// Records in global memory or on the host: planes of W*H records.
struct DnPlanes {
    const DnRec *nt_, *xc_, *col_, *var_;
    int W;
    PT_DN_MEMBER DnRec nt(int x, int y) const { return nt_[(size_t)y * W + x]; }
    PT_DN_MEMBER DnRec xc(int x, int y) const { return xc_[(size_t)y * W + x]; }
    PT_DN_MEMBER DnRec col(int x, int y) const { return col_[(size_t)y * W + x]; }
    PT_DN_MEMBER DnRec var(int x, int y) const { return var_[(size_t)y * W + x]; }
};

// The pack step for pixel i (var == nullptr: no variance record).
PT_DN_FN void dn_pack(size_t i, const float* color, const float* var, const float* normal, const float* t,
                      const int32_t* tri, const float* emission, const float* position, float sigma_z, DnRec* nt,
                      DnRec* xc, DnRec* col, DnRec* vr) {
    const size_t a = 3 * i;
    nt[i] = DnRec{normal[a], normal[a + 1], normal[a + 2], sigma_z * t[i]};
    xc[i] = DnRec{position[a], position[a + 1], position[a + 2],
                  dn_class(tri[i], emission[a], emission[a + 1], emission[a + 2])};
    col[i] = DnRec{color[a], color[a + 1], color[a + 2], dn_lum(color[a], color[a + 1], color[a + 2])};
    if (var) vr[i] = DnRec{var[a], var[a + 1], var[a + 2], 0.0f};
}

}  // namespace pt
