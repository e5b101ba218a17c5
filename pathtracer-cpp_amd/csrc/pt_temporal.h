// pt_temporal.h — the arithmetic of the temporal reprojection (include/pt_hip.h: the header text is
// the definition), stated once for the host form (pt_image_temporal, pt_host.cpp) and the kernel
// (pt_temporal.hip). Both are built with -ffp-contract=off and correctly rounded division, so
// every operation below is rounded on its own and the two return the same bits.
//
// A pixel reads its own current-frame planes (the caller's arrays as they are, no pack step: each
// is read once) and up to four pixels of the previous history; it writes its pixel of the next.
#pragma once

#include <math.h>
#include <stdint.h>

#include "pt_denoise.h"

namespace pt {

// A camera as proj() reads it: what can be formed once per call is formed on the host
// (tp_camera), so the kernel receives it as arguments and no lane repeats it.
struct TpCam {
    float px, py, pz;
    float r00, r01, r02, r10, r11, r12, r20, r21, r22;  // rows right, up, -forward
    float half_vx, half_vy;                             // 0.5f * v_res
    float neg_dist;                                     // 0.0f - distance
    float cell;
};

// pt_temporal_params with its defaults filled in and checked.
struct TpParams {
    int max_history;
    float sigma_z, normal_min;
    int sample;  // 1: PT_TEMPORAL_VAR_SAMPLE, 0: PT_TEMPORAL_VAR_TEMPORAL
};

// The current frame's planes.
struct TpFrame {
    const float* color;
    const float* var;  // sample mode only
    const float* normal;
    const float* t;
    const int32_t* tri;
    const float* emission;
    const float* position;
};

// A history's planes (pt_temporal_history).
struct TpHist {
    float* color;
    float* m2;
    float* var;
    int32_t* hist;
    float* normal;
    float* position;
    int32_t* cls;
};

template <class Cam>
PT_DN_FN TpCam tp_camera(const Cam& c) {
    return TpCam{c.pos[0],       c.pos[1],       c.pos[2],       c.transform[0],        c.transform[1],
                 c.transform[2], c.transform[3], c.transform[4], c.transform[5],        c.transform[6],
                 c.transform[7], c.transform[8], 0.5f * c.v_res[0], 0.5f * c.v_res[1], 0.0f - c.distance,
                 c.cell_size};
}

// proj(cam, X): the continuous pixel coordinates of X, false when X is not in front of the camera.
PT_DN_FN bool tp_proj(const TpCam& c, float X, float Y, float Z, float& fx, float& fy) {
    const float dx = X - c.px, dy = Y - c.py, dz = Z - c.pz;
    const float cx = dn_dot(dx, dy, dz, c.r00, c.r01, c.r02);
    const float cy = dn_dot(dx, dy, dz, c.r10, c.r11, c.r12);
    const float cz = dn_dot(dx, dy, dz, c.r20, c.r21, c.r22);
    if (!(cz < 0.0f)) return false;
    const float k = c.neg_dist / cz;
    fx = ((cx * k) + c.half_vx) / c.cell;
    fy = ((cy * k) + c.half_vy) / c.cell;
    return true;
}

PT_DN_FN int32_t tp_class(int32_t tri, float er, float eg, float eb) {
    if (tri < 0) return 0;
    return (er != 0.0f || eg != 0.0f || eb != 0.0f) ? 2 : 1;
}

// Pixel (x, y) of one call: writes its pixel of `next`, returns whether it reused its history.
// has_prev false: the first frame (prev is not read). A tap's normal, position, cls and hist are
// read first and its colour planes only when it counts.
template <bool kSample>
PT_DN_FN bool tp_pixel(int W, int H, int x, int y, const TpCam& cur, const TpCam& old, const TpFrame& F,
                       const TpHist& prev, bool has_prev, const TpHist& next, const TpParams& P) {
    const size_t i = (size_t)y * W + x, a = 3 * i;
    const float c0 = F.color[a], c1 = F.color[a + 1], c2 = F.color[a + 2];
    const float n0 = F.normal[a], n1 = F.normal[a + 1], n2 = F.normal[a + 2];
    const float X0 = F.position[a], X1 = F.position[a + 1], X2 = F.position[a + 2];
    const int32_t cls = tp_class(F.tri[i], F.emission[a], F.emission[a + 1], F.emission[a + 2]);
    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
    if (kSample) {
        v0 = F.var[a];
        v1 = F.var[a + 1];
        v2 = F.var[a + 2];
    }
    float A0 = 0.0f, A1 = 0.0f, A2 = 0.0f, M0 = 0.0f, M1 = 0.0f, M2 = 0.0f, V0 = 0.0f, V1 = 0.0f, V2 = 0.0f;
    float wsum = 0.0f;
    int32_t nmin = INT32_MAX;
    float fxc, fyc, fxp, fyp;
    if (has_prev && cls != 0 && tp_proj(cur, X0, X1, X2, fxc, fyc) && tp_proj(old, X0, X1, X2, fxp, fyp)) {
        const float gx = (float)x + (fxp - fxc), gy = (float)y + (fyp - fyc);
        if (gx > -1.0f && gx < (float)W && gy > -1.0f && gy < (float)H) {
            const float tau = P.sigma_z * F.t[i];
            const int xb = (int)floorf(gx), yb = (int)floorf(gy);
            const float ax = gx - (float)xb, ay = gy - (float)yb;
            // Tap s = 2 j + k. Three steps, so that the loads of the four taps are in flight together
            // and not one tap's after the other's: weights and addresses; the guides of every tap that
            // can count; the colour planes of those that do, then the sums in tap order.
            float bw[4];
            size_t tq[4];
            int32_t th[4] = {0, 0, 0, 0};
            bool ok[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int s = 0; s < 4; s++) {
                const int yy = yb + (s >> 1), xx = xb + (s & 1);
                bw[s] = ((s & 1) == 0 ? 1.0f - ax : ax) * ((s >> 1) == 0 ? 1.0f - ay : ay);
                ok[s] = yy >= 0 && yy < H && xx >= 0 && xx < W && bw[s] > 0.0f;
                tq[s] = ok[s] ? (size_t)yy * W + xx : i;  // a tap that cannot count is not read
            }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int s = 0; s < 4; s++) {
                if (!ok[s]) continue;
                const size_t q = tq[s], b = 3 * q;
                th[s] = prev.hist[q];
                const int32_t cq = prev.cls[q];
                const float dn = dn_dot(n0, n1, n2, prev.normal[b], prev.normal[b + 1], prev.normal[b + 2]);
                const float dl = fabsf(dn_dot(n0, n1, n2, prev.position[b] - X0, prev.position[b + 1] - X1,
                                              prev.position[b + 2] - X2));
                ok[s] = th[s] >= 1 && cq == cls && dn > P.normal_min && dl < tau;
            }
            float pc[4][3] = {}, pm[4][3] = {}, pv[4][3] = {};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int s = 0; s < 4; s++) {
                if (!ok[s]) continue;
                const size_t b = 3 * tq[s];
                for (int ch = 0; ch < 3; ch++) {
                    pc[s][ch] = prev.color[b + ch];
                    pm[s][ch] = prev.m2[b + ch];
                    if (kSample) pv[s][ch] = prev.var[b + ch];
                }
            }
            const float inf = __builtin_inff();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int s = 0; s < 4; s++) {
                if (!ok[s]) continue;
                if (!(fabsf(pc[s][0]) < inf && fabsf(pc[s][1]) < inf && fabsf(pc[s][2]) < inf)) continue;
                wsum += bw[s];
                A0 += bw[s] * pc[s][0];
                A1 += bw[s] * pc[s][1];
                A2 += bw[s] * pc[s][2];
                M0 += bw[s] * pm[s][0];
                M1 += bw[s] * pm[s][1];
                M2 += bw[s] * pm[s][2];
                if (kSample) {
                    V0 += bw[s] * pv[s][0];
                    V1 += bw[s] * pv[s][1];
                    V2 += bw[s] * pv[s][2];
                }
                nmin = th[s] < nmin ? th[s] : nmin;
            }
        }
    }
    const bool reuse = wsum > 0.0f;
    float o0 = c0, o1 = c1, o2 = c2;
    float m0 = c0 * c0, m1 = c1 * c1, m2 = c2 * c2;
    float w0, w1, w2;
    int32_t N = 1;
    if (reuse) {
        N = (nmin < P.max_history - 1 ? nmin : P.max_history - 1) + 1;
        const float alpha = 1.0f / (float)N, bb = 1.0f - alpha;
        o0 = (bb * (A0 / wsum)) + (alpha * c0);
        o1 = (bb * (A1 / wsum)) + (alpha * c1);
        o2 = (bb * (A2 / wsum)) + (alpha * c2);
        m0 = (bb * (M0 / wsum)) + (alpha * m0);
        m1 = (bb * (M1 / wsum)) + (alpha * m1);
        m2 = (bb * (M2 / wsum)) + (alpha * m2);
        if (kSample) {
            const float b2 = bb * bb, a2 = alpha * alpha;
            w0 = (b2 * (V0 / wsum)) + (a2 * v0);
            w1 = (b2 * (V1 / wsum)) + (a2 * v1);
            w2 = (b2 * (V2 / wsum)) + (a2 * v2);
        } else {
            float d0 = m0 - (o0 * o0), d1 = m1 - (o1 * o1), d2 = m2 - (o2 * o2);
            d0 = d0 > 0.0f ? d0 : 0.0f;
            d1 = d1 > 0.0f ? d1 : 0.0f;
            d2 = d2 > 0.0f ? d2 : 0.0f;
            w0 = d0 * alpha;
            w1 = d1 * alpha;
            w2 = d2 * alpha;
        }
    } else if (kSample) {
        w0 = v0;
        w1 = v1;
        w2 = v2;
    } else {
        w0 = w1 = w2 = __builtin_inff();
    }
    next.color[a] = o0;
    next.color[a + 1] = o1;
    next.color[a + 2] = o2;
    next.m2[a] = m0;
    next.m2[a + 1] = m1;
    next.m2[a + 2] = m2;
    next.var[a] = w0;
    next.var[a + 1] = w1;
    next.var[a + 2] = w2;
    next.hist[i] = N;
    next.normal[a] = n0;
    next.normal[a + 1] = n1;
    next.normal[a + 2] = n2;
    next.position[a] = X0;
    next.position[a + 1] = X1;
    next.position[a + 2] = X2;
    next.cls[i] = cls;
    return reuse;
}

}  // namespace pt
