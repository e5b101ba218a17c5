// pt_kernel.hip — the gfx950 kernels of libpt_hip.so and its device context.
//
//   pt_trace_kernel<kLds, kFlat>  generic megakernel (device code in pt_trace.h)
//   pt_trace_flat_rtc             the flat-path megakernel specialised per scene through
//                                 hipRTC (leaf-box planes as constants; shared planes and
//                                 boxes fold), compiled in the background from
//                                 pt_ctx_set_scene on (rtc_job, pt_rtc.hip)
//   pt_accumulate_kernel          in-order per-pixel accumulation + /spp
//   pt_accumulate_moments_kernel  the same with the per-pixel double sums S and Q (pt_moments)
//   pt_moments_sem_kernel         their standard error of the mean
//   pt_unconverged_kernel         the convergence count of the moments (ballot + one atomic per block)
//   pt_math_kernel                device copies of the math primitives (test hook)
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <atomic>

#include "pt_grad.h"
#include "pt_hip_debug.h"
#include "pt_launch.h"
#include "pt_moments.h"
#include "pt_nee_grad.h"
#include "pt_rtc.h"
#include "pt_trace.h"

namespace pt {

#ifndef PT_WIDE8_WAVES
#define PT_WIDE8_WAVES 6  // waves per SIMD the 8-wide walk is register-allocated for (80 VGPRs, no scratch)
#endif
#ifndef PT_WIDE4_WAVES
#define PT_WIDE4_WAVES 6
#endif
static_assert(kNodeU4<8, kWideF16> == kWideNodeU4(8, kWideF16) && kNodeU4<4, kWideF16> == kWideNodeU4(4, kWideF16) &&
                  kNodeU4<8, kWideF32> == kWideNodeU4(8, kWideF32) && kNodeU4<4, kWideF32> == kWideNodeU4(4, kWideF32) &&
                  kNodeU4<8, kWideByte> == kWideNodeU4(8, kWideByte),
              "wide node size: host and device agree");
// kLdsScene: generic tree kernels — scene arrays in LDS; wide kernels — the distinct
// materials (umats) in LDS.
// kPF: the wide tree's child planes (kWideByte, kWideF16 binary16 integers, kWideF32 floats).
// Float planes (kWideF32, PT_WIDE_PLANES=f32) are register-allocated for 5 waves: at 6 they
// spill 18 VGPRs and run at half speed (config 4: 10.3 against 18.4 Grays/s, profiles/r06_planes).
// kStack = false: the flat kernel's PerLaneRays form (test hook PT_RAY_STACK=0).
template <bool kLdsScene, bool kFlat, int kWide = 0, int kPF = kWideByte, bool kStack = true>
__global__ __launch_bounds__(kBlock, kPF == kWideF32 ? 5 : kWide == 8 ? PT_WIDE8_WAVES : kWide == 4 ? PT_WIDE4_WAVES : PT_WAVES)
void pt_trace_kernel(TraceArgs A) {
    if constexpr (kWide > 0)
        trace_body_wide<kWide, kPF, kLdsScene>(A);
    else if constexpr (kFlat && kStack)
        trace_body_flat<TableBoxMask>(A);
    else if constexpr (kFlat)
        trace_body_flat<PerLaneRays<TableBoxMask>>(A);
    else
        trace_body<kLdsScene>(A);
}

using TraceKernel = void (*)(TraceArgs);
// The wide-walk instantiation for a tree's width and plane format.
template <int kW, int kPF>
static TraceKernel wide_kernel_t(bool lds_mats) {
    return lds_mats ? pt_trace_kernel<true, false, kW, kPF> : pt_trace_kernel<false, false, kW, kPF>;
}
static TraceKernel wide_kernel(int width, int fmt, bool lds_mats) {
    if (width == 8)
        return fmt == kWideF32   ? wide_kernel_t<8, kWideF32>(lds_mats)
               : fmt == kWideF16 ? wide_kernel_t<8, kWideF16>(lds_mats)
                                 : wide_kernel_t<8, kWideByte>(lds_mats);
    return fmt == kWideF32   ? wide_kernel_t<4, kWideF32>(lds_mats)
           : fmt == kWideF16 ? wide_kernel_t<4, kWideF16>(lds_mats)
                             : wide_kernel_t<4, kWideByte>(lds_mats);
}

// Running per-pixel sum in sample order (image.h:27-31 via render.h:84), then /spp
// (image.h:37-40) on the last batch; output interleaved RGB rows of this part. The order of the
// sum is slab_walk<true>'s (pt_trace.h): dense records, or a flagged slab's flagged ones.
__global__ __launch_bounds__(kBlock) void pt_accumulate_kernel(const float* __restrict__ radiance,
                                                               float* __restrict__ accum, float* __restrict__ out,
                                                               int npix, int s_count, int first, int last,
                                                               int keep, float spp, const uint32_t* __restrict__ flags,
                                                               int flags_pm) {
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= npix) return;
    float x = first ? 0.0f : accum[q];
    float y = first ? 0.0f : accum[npix + q];
    float z = first ? 0.0f : accum[2 * (size_t)npix + q];
    SumF32 a{x, y, z};
    slab_walk<true>(radiance, flags, flags_pm, s_count, (uint32_t)q, (uint32_t)npix, a);
    if (last) {
        out[3 * (size_t)q] = x / spp;
        out[3 * (size_t)q + 1] = y / spp;
        out[3 * (size_t)q + 2] = z / spp;
    }
    if (!last || keep) {  // keep: the running sum stays for a progressive continuation
        accum[q] = x;
        accum[npix + q] = y;
        accum[2 * (size_t)npix + q] = z;
    }
}

// pt_accumulate_kernel for a moments render (pt_ctx_render_moments): the same walk, the same
// image, and the context's six doubles per pixel continued in `mom`: S at [3 q + c], Q at
// [3 npix + 3 q + c] (the layout of `out`). The float32 sum always stays.
__global__ __launch_bounds__(kBlock) void pt_accumulate_moments_kernel(const float* __restrict__ radiance,
                                                                       float* __restrict__ accum,
                                                                       float* __restrict__ out, double* __restrict__ mom,
                                                                       int npix, int s_count, int first, int last,
                                                                       float spp, const uint32_t* __restrict__ flags,
                                                                       int flags_pm) {
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= npix) return;
    float x = first ? 0.0f : accum[q];
    float y = first ? 0.0f : accum[npix + q];
    float z = first ? 0.0f : accum[2 * (size_t)npix + q];
    double* S = mom + 3 * (size_t)q;
    double* Q = S + 3 * (size_t)npix;
    MomentSums a{x, y, z, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!first) {
        a.sx = S[0];
        a.sy = S[1];
        a.sz = S[2];
        a.qx = Q[0];
        a.qy = Q[1];
        a.qz = Q[2];
    }
    slab_walk<true>(radiance, flags, flags_pm, s_count, (uint32_t)q, (uint32_t)npix, a);
    if (last) {
        out[3 * (size_t)q] = x / spp;
        out[3 * (size_t)q + 1] = y / spp;
        out[3 * (size_t)q + 2] = z / spp;
    }
    accum[q] = x;
    accum[npix + q] = y;
    accum[2 * (size_t)npix + q] = z;
    S[0] = a.sx;
    S[1] = a.sy;
    S[2] = a.sz;
    Q[0] = a.qx;
    Q[1] = a.qy;
    Q[2] = a.qz;
}

// The standard error of the mean of n samples from the moments (one thread per pixel and channel):
// sqrt(max(0, (Q - S*S/n) / (n-1)) / n) in double, rounded to float; +inf for n < 2. A NaN stays.
__global__ __launch_bounds__(kBlock) void pt_moments_sem_kernel(const double* __restrict__ mom, size_t nval, int n,
                                                                float* __restrict__ sem) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nval) return;
    if (n < 2) {
        sem[i] = __builtin_inff();
        return;
    }
    const double S = mom[i], Q = mom[nval + i], dn = (double)n;
    double var = (Q - S * S / dn) / (dn - 1.0);
    if (var < 0.0) var = 0.0;
    sem[i] = (float)sqrt(var / dn);
}

// The unconverged pixels of the moments (the criterion: pt_moments.h), one pixel per lane: a wave
// counts by ballot and popcount, a block adds its waves' counts with one atomic. mask (optional):
// one byte per pixel, 1 = unconverged.
__global__ __launch_bounds__(kBlock) void pt_unconverged_kernel(const double* __restrict__ mom, int npix, int n,
                                                                double rel, double abs_tol,
                                                                unsigned long long* __restrict__ count,
                                                                uint8_t* __restrict__ mask) {
    __shared__ unsigned int wave_count[kBlock / kWave];
    const int q = blockIdx.x * kBlock + threadIdx.x;
    bool un = false;
    if (q < npix) {
        const double* S = mom + 3 * (size_t)q;
        un = moments_pixel_unconverged(S, S + 3 * (size_t)npix, n, rel, abs_tol);
        if (mask) mask[q] = un ? 1 : 0;
    }
    const unsigned long long b = __ballot(un);
    if ((threadIdx.x & (kWave - 1)) == 0) wave_count[threadIdx.x / kWave] = (unsigned int)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int t = 0;
#pragma unroll
        for (int w = 0; w < kBlock / kWave; w++) t += wave_count[w];
        if (t) atomicAdd(count, (unsigned long long)t);
    }
}

// gamma_correct + save_png quantisation (image.h:41-55) on the device. The 8-bit value of
// x >= 0 is the number of thresholds thr[0..254] <= x (pt_rgb8_thresholds: for each value
// the least float reaching it under the host's powf), so no powf runs here and the bytes
// are pt_image_to_rgb8's (tests: every float of [0, 2] on the host, every threshold and
// its neighbours on the device). NaN -> 255 (clamp(NaN) = 1, linalg.h:233-235); x < 0 by
// neg_mode: powf of a negative base is NaN for a non-integer exponent (255), negative for
// an odd integer one (0), |x|^e for an even one. Row r of the part is written to row
// (flip ? rows - 1 - r : r); flip = top row first, as the PNG (image.h:51).
__global__ __launch_bounds__(kBlock) void pt_rgb8_kernel(const float* __restrict__ lin, uint8_t* __restrict__ out,
                                                         const float* __restrict__ thr, int rows, int W, int flip,
                                                         int neg_mode) {
    __shared__ float t[256];
    t[threadIdx.x] = thr[threadIdx.x];  // thr[255] = +inf
    __syncthreads();
    const int r = blockIdx.y;
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= 3 * W) return;
    float x = lin[(size_t)r * 3 * W + c];
    int v;
    if (x != x) {
        v = 255;
    } else if (x < 0.0f && neg_mode != 2) {
        v = neg_mode == 0 ? 255 : 0;
    } else {
        x = __builtin_fabsf(x);
        v = 0;
#pragma unroll
        for (int step = 128; step > 0; step >>= 1)
            if (t[v + step - 1] <= x) v += step;
    }
    out[(size_t)(flip ? rows - 1 - r : r) * 3 * W + c] = (uint8_t)v;
}

// The theta table of hemisphere_dir_tab (pt_math.h): for grid point idx, x = (idx - 2^24)
// 2^-24 (exact), theta = acosf(x) - M_PI_2 as material.h:9 forms it, and its sine and cosine,
// by the same exact device functions hemisphere_dir uses.
__global__ __launch_bounds__(kBlock) void pt_theta_table_kernel(float2* __restrict__ tab) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= kThetaEntries) return;
    const float x = (float)(i - (1 << 24)) * 0x1p-24f;
    const float theta = (float)((double)acosf_path(x) - 1.57079632679489661923);
    float st, ct;
    sincosf_path(theta, st, ct);
    tab[i] = make_float2(st, ct);
}

// Device copies of the math primitives, for the GPU math known-answer tests.
__global__ void pt_math_kernel(int which, const float* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (which == 0) {
        out[i] = acosf_ref(in[i]);
    } else if (which == 1) {
        float sv, cv;
        sincosf_ref(in[i], sv, cv);
        out[2 * i] = sv;
        out[2 * i + 1] = cv;
    } else if (which == 2) {
        // BRDF from an LCG state: in = {state_bits, type, rough, dx, dy, dz, nx, ny, nz} per item
        const float* a = in + 9 * (size_t)i;
        Lcg g{__float_as_uint(a[0])};
        const int type = __float_as_int(a[1]);
        const v3 dd{a[3], a[4], a[5]}, nn{a[6], a[7], a[8]};
        v3 r;
        if (type == PT_MAT_SPECULAR) specular_dir(g, dd, nn, a[2], kMaxSpecularIters, r);
        else r = hemisphere_dir(g, nn);
        out[4 * i] = r.x;
        out[4 * i + 1] = r.y;
        out[4 * i + 2] = r.z;
        out[4 * i + 3] = __uint_as_float(g.s);
    }
}

// pt_debug_domain_once (test hook): the three predicates the flat body asked of a ray, the one
// verdict it asks with PT_DOMAIN_ONCE, and the slab rule with and without the inv half of its
// guard, as shade_inv calls them. One function for the host and the device form.
template <bool kUnit>
PT_HD void domain_once_probe(v3 elb, v3 ert, v3 o, v3 d, uint8_t* r, float* inv3) {
    const float ax = __builtin_fabsf(d.x), ay = __builtin_fabsf(d.y), az = __builtin_fabsf(d.z);
    bool in = __builtin_fminf(__builtin_fminf(ax, ay), az) >= 0x1p-126f;  // rcp3_exact's predicate
    if (!kUnit) in = in && __builtin_fmaxf(__builtin_fmaxf(ax, ay), az) <= 0x1p126f;
    bool fell;
    const v3 inv = rcp3_exact_v<kUnit>(d, fell);
    const bool inv_ok = fell ? finite_nonzero3(inv) : true;
    r[0] = in;
    r[1] = finite_nonzero3(inv);
    r[2] = all_finite(inv);
    r[3] = !fell;
    r[4] = emit_slab_reject(elb, ert, o, inv);
    r[5] = emit_slab_reject_given(elb, ert, o, inv, inv_ok);
    inv3[0] = inv.x;
    inv3[1] = inv.y;
    inv3[2] = inv.z;
}
// One block; every lane of a wave runs the same number of rounds (a lane past the end repeats the
// last ray and stores nothing), so the wave's vote inside rcp3_exact_v sees whole waves.
__global__ void pt_domain_once_kernel(const float* box6, const float* org, const float* dir, int n, int unit,
                                      uint8_t* out, float* inv3) {
    const v3 elb{box6[0], box6[1], box6[2]}, ert{box6[3], box6[4], box6[5]};
    for (int base = 0; base < n; base += (int)blockDim.x) {
        const int i = base + (int)threadIdx.x, j = i < n ? i : n - 1;
        const v3 o{org[3 * j], org[3 * j + 1], org[3 * j + 2]}, d{dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]};
        uint8_t r[6];
        float v[3];
        if (unit) domain_once_probe<true>(elb, ert, o, d, r, v);
        else domain_once_probe<false>(elb, ert, o, d, r, v);
        if (i < n) {
            for (int c = 0; c < 6; c++) out[6 * i + c] = r[c];
            for (int c = 0; c < 3; c++) inv3[3 * i + c] = v[c];
        }
    }
}

// Exhaustive sweep of a fast exact sequence against the IEEE operation (test hook).
__global__ void pt_sweep_kernel(int which, uint32_t lo, unsigned long long n, unsigned long long* bad,
                                uint32_t* first) {
    unsigned long long nb = 0;
    uint32_t fb = 0xffffffffu;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t bits = lo + (uint32_t)i;
        const float x = __uint_as_float(bits);
        if (x != x) continue;
        bool same;
        if (which == 0) {
            same = __float_as_uint(rcp_exact(x)) == __float_as_uint(1.0f / x);
        } else if (which == 1) {
            same = __float_as_uint(sqrt_exact(x)) == __float_as_uint(__builtin_sqrtf(x));
        } else if (which == 4) {
            // div_by_rcp vs IEEE division: dividend x (the swept bits, taken when in
            // [2^-60, 2^60]); divisor a hashed normal float in [1, 2^11) (camera-length
            // range) or, for odd i, in [2^-60, 2^60]
            const float ax = __builtin_fabsf(x);
            if (!(ax >= 0x1p-60f && ax <= 0x1p60f)) continue;
            const uint32_t hsh = pt_mix32(bits * 0x9e3779b9u + 0x7f4a7c15u);
            const uint32_t e = (bits & 1u) ? 67u + (hsh >> 23) % 121u : 127u + (hsh >> 23) % 11u;
            const float b = __uint_as_float((e << 23) | (hsh & 0x7fffffu));
            same = __float_as_uint(div_by_rcp(x, b, rcp_exact(b))) == __float_as_uint(x / b);
        } else if (which == 2) {
            same = __float_as_uint(acosf_fast(x)) == __float_as_uint(acosf_ref(x));
        } else if (which == 5) {
            // rcp3_exact's two predicates on three equal components: the unit form (lower bound only)
            // wherever a unit vector's component can lie, |x| <= 2, the two-sided form elsewhere
            const v3 r = __builtin_fabsf(x) <= 2.0f ? rcp3_exact<true>(v3{x, x, x}) : rcp3_exact<false>(v3{x, x, x});
            const uint32_t q = __float_as_uint(1.0f / x);
            same = __float_as_uint(r.x) == q && __float_as_uint(r.y) == q && __float_as_uint(r.z) == q;
        } else if (which >= 6 && which <= 9) {
            // The wave-uniform fallback with a wave's lanes on both sides of the range: component 0 is
            // x, components 1 and 2 are hashed normal floats (6, 9: of rcp_exact's whole range; 7, 8: of
            // [2^-40, 2^40], where normalize_fast's fast path holds), and in 6 and 7 one input in 16
            // (four lanes of every wave) has them forced to +-0, a subnormal, 2^127, +-inf or a value in
            // (2^126, 2^128). 6: rcp3_exact, 7 and 8: normalize_fast, against the IEEE operations.
            // 8 and 9 are 7 and 6 without the forced lanes, so that the waves of in-range x keep the
            // fast results of three different components; in 9 one input in 16 has a NaN as component
            // 1, which passes rcp3_exact's predicate beside two components in range: the result must
            // be a NaN there (any payload) and the other two components exact.
            const uint32_t h1 = pt_mix32(bits * 0x9e3779b9u + 0x7f4a7c15u), h2 = pt_mix32(h1 ^ 0x85ebca6bu);
            auto pick = [&](uint32_t h, uint32_t k) {
                const uint32_t sign = h & 0x80000000u, mant = h & 0x7fffffu;
                if (which <= 7 && (bits & 15u) == 11u) {
                    switch (k & 7u) {
                        case 0: return __uint_as_float(sign);                              // +-0
                        case 1: return __uint_as_float(sign | mant | 1u);                  // subnormal
                        case 2: return 0x1p127f;
                        case 3: return __uint_as_float(sign | 0x7f800000u);                // +-inf
                        case 4: return __uint_as_float(sign | 0x7e800000u | mant | 1u);    // (2^126, 2^127)
                        case 5: return __uint_as_float(sign | 0x7f000000u | mant);         // [2^127, 2^128)
                        case 6: return __uint_as_float(sign | 1u);                         // smallest subnormal
                        default: return __uint_as_float(0x80000000u);                      // -0
                    }
                }
                const uint32_t e = (which == 6 || which == 9) ? 1u + (h >> 23) % 252u : 87u + (h >> 23) % 81u;
                return __uint_as_float(sign | (e << 23) | mant);
            };
            v3 a{x, pick(h1, h1 >> 8), pick(h2, (h1 >> 8) + 3u)};
            if (which == 9 && (bits & 15u) == 11u) a.y = __uint_as_float((h1 & 0x80000000u) | 0x7fc00000u | (h1 & 0x3fffffu));
            v3 r, q;
            if (which == 6 || which == 9) {
                r = rcp3_exact<false>(a);
                q = v3{1.0f / a.x, 1.0f / a.y, 1.0f / a.z};
            } else {
                r = normalize_fast(a);
                const float len = __builtin_sqrtf(dot(a, a));
                q = v3{a.x / len, a.y / len, a.z / len};
            }
            same = __float_as_uint(r.x) == __float_as_uint(q.x) &&
                   (__float_as_uint(r.y) == __float_as_uint(q.y) || (which == 9 && r.y != r.y && q.y != q.y)) &&
                   __float_as_uint(r.z) == __float_as_uint(q.z);
        } else {
            float s1, c1, s0, c0;
            sincosf_fast(x, s1, c1);
            sincosf_ref(x, s0, c0);
            same = __float_as_uint(s1) == __float_as_uint(s0) && __float_as_uint(c1) == __float_as_uint(c0);
        }
        if (!same) {
            nb++;
            fb = min(fb, bits);
        }
    }
    if (nb) {
        atomicAdd(bad, nb);
        atomicMin(first, fb);
    }
}

}  // namespace pt

using namespace pt;

struct pt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // The stream and work counter are made on a thread of their own (pt_ctx_create): a new
    // stream takes ~5 ms (a hardware queue), which then overlaps the caller's scene packing.
    // ctx_ready() joins it (once) before anything uses them.
    std::thread init;
    std::once_flag init_once;
    std::string init_error;  // set by the init thread when a creation failed
    bool counted = false;    // counted in g_dev_contexts (pt_ctx_create succeeded)
    int num_cus = 0;
    size_t lds_usable = 0;  // LDS per CU the blocks of one launch can count on (kLdsUsable on gfx950)
    // scene
    float4* d_nodes = nullptr;
    float4* d_tris = nullptr;
    float4* d_mats = nullptr;
    float4* d_leaves = nullptr;
    float4* d_wide = nullptr;
    float4* d_wtris = nullptr;
    float4* d_nrm = nullptr;    // wide path: {n.xyz, material id} per rank position
    float4* d_umats = nullptr;  // wide path: distinct materials
    int32_t* d_rank_tri = nullptr;  // rank position -> the caller's triangle index (ray queries, AOVs)
    std::vector<f4> flat_host;  // leaf boxes for the kernel-argument table
    FlatLeaves flat_tab;        // that table (build_flat_table): distinct boxes and their leaves
    int flat_boxes_padded = 0;  // its boxes, rounded up to a multiple of 4 (0: not a flat scene)
    PackedScene meta;
    bool have_scene = false;
    bool has_specular = false;  // the scene holds a SPECULAR material
    bool albedo_x2 = false;     // the scene kernel unwinds with pre-doubled albedo (albedo_x2_ok)
    bool dark = false;          // every bounce material is dark (scene_dark): finish_path's skip
    EmitBox emit;               // the last-ray rule and its emitter box (scene_emit_box)
    uint64_t last_early = 0;    // paths the rule ended in the last render (PT_COUNT_EARLY kernels; ctr[4])
    void* flat_fast = nullptr;  // the flat table kernel with the scene's flags (pt_flat_fast.hip), or none
    int flat_boxes = 0;         // box-level pairs in the hipRTC kernel: distinct boxes (its LDS table), else 0
    bool rtc_requested = false; // a hipRTC scene kernel was requested for the scene
    // buffers
    float* d_radiance = nullptr;
    size_t radiance_floats = 0;
    uint32_t* d_flags = nullptr;  // flagged slabs (TraceArgs::flags): one bit per record, per slab
    size_t flags_words = 0;
    float* d_accum = nullptr;
    size_t accum_floats = 0;
    float* d_out = nullptr;
    size_t out_floats = 0;
    unsigned long long* d_ctr = nullptr;
    unsigned long long* d_stamps = nullptr;  // PT_STAMPS builds only
    int* d_xstack = nullptr;                 // wide path: exact binary-walk stacks
    size_t xstack_ints = 0;
    uint8_t* d_rgb8 = nullptr;               // 8-bit output staging (pt_ctx_render_rgb8)
    size_t rgb8_bytes = 0;
    float* d_thr = nullptr;                  // quantisation thresholds, 256 floats
    // ray queries and AOVs (pt_ctx_intersect, pt_ctx_render_aov)
    int* d_qstack = nullptr;                 // traversal stacks, when they do not go to LDS
    size_t qstack_ints = 0;
    float* d_qbuf = nullptr;                 // staging of a host-pointer call's rays / channels and results
    size_t qbuf_floats = 0;
    unsigned long long* d_qhits = nullptr;   // hit counter of a call
    // trace() on caller-supplied rays (pt_ctx_trace): buffers of its own, so a progressive sum stays valid
    float* d_tslab = nullptr;                // dense radiance slab of one launch, [sample][ray][rgb]
    size_t tslab_floats = 0;
    float* d_trec = nullptr;                 // path records, when they do not go to LDS
    size_t trec_words = 0;
    float* d_tbuf = nullptr;                 // staging of a host-pointer call's rays and results
    size_t tbuf_floats = 0;
    float* d_tstates = nullptr;              // staging of a host-pointer call's LCG states (uint32)
    size_t tstates_words = 0;
    unsigned long long* d_tctr = nullptr;    // counters of a call (6 x u64): work head, rays, gradient terms, runaway,
                                             // shadow segments, light draws (trace_counters)
    // light sampling (pt_ctx_trace_nee, pt_ctx_render_nee; pt_nee.hip): the scene's light table, made on the
    // host when the scene is set and uploaded by the first call that samples lights; pt_ctx_trace's staging
    LightTable lights;
    bool lights_uploaded = false;
    uint8_t* d_lights = nullptr;             // [geom 5 x float4][cdf][tri][listed per caller triangle]
    size_t lights_bytes = 0;
    // material gradients (pt_ctx_trace_grad): pt_ctx_trace's buffers, and
    double* d_gtab = nullptr;                // the gradient table, 6 doubles per caller triangle, then the split outputs
    size_t gtab_doubles = 0;
    float4* d_gmats = nullptr;               // the per-call materials (override gathered), 2 per packed triangle; then
                                             // (pt_ctx_trace_nee_grad) the per-call emission of every light
    size_t gmats_f4 = 0;
    float* d_gbuf = nullptr;                 // staging of a host-pointer call's override rows and grad_rgb
    size_t gbuf_floats = 0;
    // sample moments (pt_ctx_render_moments): S and Q, 6 doubles per pixel (48 x npix bytes), made on
    // first use and released with the slabs; the unconverged count; staging of a host-pointer sem
    double* d_mom = nullptr;
    size_t mom_doubles = 0;
    unsigned long long* d_mcount = nullptr;
    float* d_sem = nullptr;
    size_t sem_floats = 0;
    // per-pixel rounds of pt_ctx_render_adaptive (pt_adaptive.hip): buffers of its own
    int32_t* d_alist[2] = {nullptr, nullptr};  // the active list and the next one (part-local pixel indices)
    size_t alist_ints[2] = {0, 0};
    int32_t* d_aspp = nullptr;               // n_p per pixel
    size_t aspp_ints = 0;
    float* d_aslab = nullptr;                // dense radiance slab of one launch, [sample][listed pixel][rgb]
    size_t aslab_floats = 0;
    float* d_arec = nullptr;                 // path records, when they do not go to LDS
    size_t arec_words = 0;
    unsigned long long* d_actr = nullptr;    // work head, ray and runaway counters (4 x u64), then the list's count
    // the denoiser's scratch (pt_denoise.hip through ctx_scratch)
    void* d_dn[kDnScratchSlots] = {};
    size_t dn_bytes[kDnScratchSlots] = {};
    TemporalState temporal;                  // pt_ctx_render_temporal's history (pt_temporal.hip)
    // progressive rendering: d_accum holds the running sum of prog_spp samples; prog_moments: the
    // sum is a moments sum (d_mom continues with it, over prog_npix pixels)
    bool prog_valid = false;
    bool prog_moments = false;
    int prog_spp = 0;
    int prog_npix = 0;
    pt_camera prog_cam{};
    pt_params prog_prm{};
    hipFunction_t rtc_flat = nullptr;        // scene-specialised flat kernel (hipRTC), if built
    std::string rtc_status;                  // why there is no rtc_flat ("" when there is)
    std::string rtc_src;                     // its source while the compile is pending
    RtcBaked rtc_baked;                      // what that source (pending or loaded) holds as constants
    RtcFuture rtc_job;                       // its pending compile (valid() until taken)
    int64_t last_plan[24] = {};              // pt_debug_ctx_plan: the launch plan of the last render (order: pt_hip_debug.h)
};

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return set_error(PT_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// The context's stream and work counter, once pt_ctx_create's init thread has made them:
// PT_OK, or that thread's error (reported on the calling thread).
int ctx_ready(pt_ctx* c) {
    std::call_once(c->init_once, [c] {
        if (c->init.joinable()) c->init.join();
    });
    if (!c->init_error.empty()) return set_error(PT_E_HIP, "%s", c->init_error.c_str());
    return PT_OK;
}

// Live contexts per device: the radiance-slab budget is shared among them (several
// contexts on one device — pt_render_*_devices with a device listed twice, or long-lived
// Renderer objects — must not each size their slab from the same free memory).
std::mutex g_dev_mu;
std::map<int, int> g_dev_contexts;

size_t batch_bytes_budget(int device, bool compile_pending) {
    const char* e = hook_env("PT_BATCH_BYTES");  // test hook: the budget itself (0 too: one sample per launch)
    if (e && *e) return (size_t)strtoull(e, nullptr, 0);
    // Radiance slabs (both, when two alternate): 48 GiB, ~2047 spp of a 1024^2 frame per
    // launch (the 2^31-item bound), so a frame pays fewer launch drains (~0.37 ms each on the
    // headline, DESIGN.md §6: 15 -> 5 launches, whole job +0.3 % at 10 launches, profiles/r06_batch);
    // 16 GiB while the scene kernel still compiles (a cold first frame: shorter launches
    // switch to it sooner and the first allocation is smaller). At most half the free HBM,
    // divided among the device's live contexts.
    int sharers = 1;
    {
        std::lock_guard<std::mutex> lock(g_dev_mu);
        sharers = std::max(1, g_dev_contexts[device]);
    }
    size_t budget = ((size_t)(compile_pending ? 16 : 48) << 30) / sharers, free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b / 2 / sharers < budget) budget = free_b / 2 / sharers;
    return std::max<size_t>(budget, (size_t)64 << 20);
}

std::atomic<int64_t> g_ctx_created{0}, g_scene_uploads{0};  // pt_debug_counter

// Renders of at least this many paths wait for a pending compile (~0.4 s) rather than
// run the generic flat kernel (bit-identical, ~40 % slower); smaller ones (config 1, the
// first frames of a progressive render) start at once with the generic kernel.
constexpr double kRtcWaitPaths = 256.0 * 1024 * 1024;

// The fused accumulation's last batch as a fraction of a batch (render_range: tail); 0 = the
// remainder as it falls.
constexpr int kTailDiv = 0;

}  // namespace

int64_t pt::kernel_counter(int which) { return which == 0 ? g_ctx_created.load() : g_scene_uploads.load(); }

// The context's radiance slabs and their flags (the largest buffers: up to half the free HBM)
// back to the device; the next render allocates them again. The scene, accumulation and
// output buffers stay (pt_multi.hip: cached multi-device contexts after each render). The
// moments buffer goes too, and a running moments sum ends with it.
int pt::ctx_release_slabs(pt_ctx* c) {
    if (!c) return PT_OK;
    if (int rc = ctx_ready(c)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (c->stream) HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->d_radiance) (void)hipFree(c->d_radiance);
    if (c->d_flags) (void)hipFree(c->d_flags);
    c->d_radiance = nullptr;
    c->radiance_floats = 0;
    c->d_flags = nullptr;
    c->flags_words = 0;
    if (c->d_mom) (void)hipFree(c->d_mom);
    c->d_mom = nullptr;
    c->mom_doubles = 0;
    if (c->prog_moments) c->prog_valid = false;
    return PT_OK;
}


namespace {

// Take the context's pending compile if it is done, or (wait) once it is.
void rtc_resolve(pt_ctx* c, bool wait) {
    if (!c->rtc_job.valid()) return;
    if (!wait && c->rtc_job.wait_for(std::chrono::seconds(0)) != std::future_status::ready) return;
    c->rtc_flat = rtc_load(c->device, c->rtc_src, *c->rtc_job.get(), c->rtc_status);
    if (!c->rtc_flat && c->rtc_status == "evicted") {  // the disk entry did not load: compile it
        c->rtc_job = rtc_job(c->rtc_src);
        c->rtc_status = "compiling";
        if (wait) rtc_resolve(c, true);
        return;
    }
    c->rtc_job = RtcFuture();
    c->rtc_src.clear();
}

}  // namespace

// One theta table per device (256 MB), built on first use and kept for the process.
static std::mutex g_theta_mu;
static std::map<int, float2*> g_theta_tabs;

// Freed when the device's last context is destroyed (pt_ctx_destroy). The count is checked
// again under both locks (device count, then table; nothing takes them in the other order):
// a context created on the device meanwhile keeps the table (it could otherwise
// have fetched the pointer and launched kernels reading it after the free).
static void theta_table_release(int device) {
    std::lock_guard<std::mutex> dev_lock(g_dev_mu);
    std::lock_guard<std::mutex> lock(g_theta_mu);
    if (g_dev_contexts[device] != 0) return;
    auto it = g_theta_tabs.find(device);
    if (it == g_theta_tabs.end()) return;
    (void)hipFree(it->second);
    g_theta_tabs.erase(it);
}

[[maybe_unused]] static int theta_table(pt_ctx* c, const float2** out) {
    std::lock_guard<std::mutex> lock(g_theta_mu);
    auto it = g_theta_tabs.find(c->device);
    if (it != g_theta_tabs.end()) {
        *out = it->second;
        return PT_OK;
    }
    float2* t = nullptr;
    HIP_TRY(hipMalloc((void**)&t, sizeof(float2) * (size_t)kThetaEntries));
    hipLaunchKernelGGL(pt_theta_table_kernel, dim3((kThetaEntries + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, t);
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipFree(t);
        return set_error(PT_E_HIP, "theta table: %s", hipGetErrorString(e));
    }
    g_theta_tabs[c->device] = t;
    *out = t;
    return PT_OK;
}

// ---------------------------------------------------------------- renders
// render_range: validate, plan (plan_render: no allocation, no launch), buffers
// (render_buffers), launch-invariant arguments (fill_trace_args), one launch_batch per batch,
// finish_render.
namespace {

// What a render decides once, before it allocates or launches anything.
struct RenderPlan {
    PartShape shape;
    int s_lo = 0, spp = 0;  // samples [s_lo, spp) are added; the image is the running sum / spp (render.h:97)
    // batching (plan_batch)
    int batch = 0, per_item = 1, tail = 0;
    bool fused = false, flagged = false;
    bool moments = false;  // a moments render: every slab summed by pt_accumulate_moments_kernel (never fused)
    int flags_pm = 0;
    size_t slab_floats = 0, slab_words = 0;  // one radiance slab and its flag bits
    // kernel family and its LDS
    bool flat = false, wide = false, pairs = false, wide_single = false, lds_scene = false;
    int rec = 1, stack = 1, exact_rows = 1;
    int pair_queue = 0, wide_rows = 0, wide_queue = 0, wide_top = 0;
    size_t box_tab_bytes = 0, lds_bytes = 0;
    TraceKernel kern = nullptr;
    bool use_rtc = false;     // launches run the hipRTC scene kernel (may turn true between launches)
    bool may_switch = false;  // a compile still running may switch this render to it
    int rtc_switch_at = -1;   // PT_RTC_SWITCH_AT (test hook): wait for the compile before launch k
    int theta_lanes = 0;                // theta_choice's answer, asked once per render
    const float2* theta_tab = nullptr;
    int blocks_per_cu = 1;
};

// PT_FORCE_EXACT_SLAB (test hook): 1 never take the IEEE slab form, 2 only in odd waves of a block.
int force_exact_slab() {
    const char* fe = hook_env("PT_FORCE_EXACT_SLAB");
    return (fe && (*fe == '1' || *fe == '2')) ? *fe - '0' : 0;
}

// Batch size: a radiance slab of 3 * batch * npix floats within the budget, work items of one
// launch below 2^31, and whether launches sum the previous slab (fused accumulation).
void plan_batch(const pt_ctx* c, const pt_params* prm, RenderPlan& P) {
    const int npix = P.shape.npix, spp = P.spp, s_lo = P.s_lo;
    int batch = prm->batch_spp > 0 ? prm->batch_spp : 0;
    const bool compile_pending = c->rtc_job.valid();
    bool halved = false;  // an automatic batch already sized for two alternating slabs
    if (batch <= 0) {
        const size_t per_sample = 3 * sizeof(float) * (size_t)std::max(npix, 1);
        const size_t whole = std::max<size_t>(1, batch_bytes_budget(c->device, compile_pending) / per_sample);
        // more than one launch: two slabs share the budget (fused accumulation, below),
        // halved before the 2^31-item bound so that bound, not the halving, sets the size
        halved = (size_t)std::max(spp - s_lo, 1) > whole;
        batch = (int)std::min<size_t>(halved ? (whole + 1) / 2 : whole, (size_t)INT32_MAX);
    }
    batch = std::max(1, std::min(batch, std::max(spp - s_lo, 1)));
    int per_item = prm->samples_per_item > 0 ? std::min(prm->samples_per_item, batch) : 1;  // one sample per work item (2: -0.4 %, 4: -1.5 % on the headline)
    // work items of one launch stay below 2^31 (32-bit item arithmetic in the kernel)
    batch = (int)std::min<long long>(batch, std::max<long long>(per_item, ((1ll << 31) - 1) / std::max(npix, 1) * per_item));
    if (P.flat && per_item != 1) {  // the flat kernel's work items are single samples (claim_item)
        per_item = 1;
        batch = (int)std::min<long long>(batch, std::max<long long>(1, ((1ll << 31) - 1) / std::max(npix, 1)));
    }
    // Fused accumulation (fused_accumulate_chunk, pt_trace.h): with more than one launch,
    // launch b also sums batch b-1's slab into the running sum, so only the last batch
    // needs pt_accumulate_kernel between trace launches. Two slabs alternate; an automatic
    // batch is halved so both fit the budget of one. PT_FUSED_ACC=0 (test hook): the
    // separate pass after every launch.
    // A moments render (P.moments) takes that separate pass too: the double sums live in it.
    bool fused = (spp - s_lo) > batch && !hook_off("PT_FUSED_ACC") && !P.moments;
    if (fused && prm->batch_spp <= 0 && !halved) batch = std::max(1, (batch + 1) / 2);
    // an explicit batch keeps its size: fusion (two slabs) only when both fit the budget (read
    // here, before render_buffers grows the sum, staging and stack buffers: the free HBM it
    // sees is larger by those than when this was decided after them)
    if (fused && prm->batch_spp > 0 && 2 * 3 * sizeof(float) * (size_t)batch * npix > batch_bytes_budget(c->device, compile_pending))
        fused = false;
    P.batch = batch;
    P.per_item = per_item;
    P.fused = fused;
    P.slab_floats = 3 * (size_t)batch * npix;
    // Tail batch (fused): the last batch is summed by pt_accumulate_kernel after the last
    // launch, on the stream's critical path, so it is made small: the samples left after the
    // full batches end in (left - tail, tail) with tail = batch / PT_TAIL_DIV (tuning hook,
    // 0 = off: the last batch is the remainder).
    const int tail_div = std::max(0, hook_int("PT_TAIL_DIV", kTailDiv));
    P.tail = fused && tail_div > 0 ? std::max(1, batch / tail_div) : 0;
    // Flagged slabs (TraceArgs::flags) in dark scenes: a path that ends at +0 (98 % of them in
    // every BASELINE scene, §3.9) stores nothing, the others store their record and set its
    // bit, and the accumulation reads the bits and only the flagged records. The sums are the
    // dense slab's (an unflagged record is +0; adding +0 changes no running sum). Each slab's
    // bits are cleared before the launch that fills it. PT_FLAGS=0 (test hook): dense slabs.
    P.flagged = c->dark && !hook_off("PT_FLAGS");
    // Bit layout (TraceArgs::flags_pm): pixel-major words (one load per 32 samples of a pixel)
    // for frames of several launches, whose slabs the trace kernels sum (fused accumulation):
    // headline whole job +0.7 %, config 5 +0.6 %; sample-major (round 5) for one-launch frames
    // (an 8-GPU share), whose trace kernel measured 1 % slower with the other layout
    // (profiles/r06_flags). A moments render of several launches sums every slab in the separate
    // pass and takes the pixel-major words too: that pass 10.7 -> 3.2 ms per 8192-spp Cornell frame,
    // the trace kernels the same (profiles/moments). PT_FLAGS_PM=0 / 1 (test hook) forces one.
    const char* pm_env = hook_env("PT_FLAGS_PM");
    const bool several = fused || (P.moments && (spp - s_lo) > batch);
    P.flags_pm = (pm_env && *pm_env) ? (*pm_env == '1' ? 1 : 0) : (several ? 1 : 0);
    P.slab_words = P.flags_pm ? ((size_t)batch + 31) / 32 * npix : ((size_t)batch * npix + 31) / 32;
}

// Samples of the launch that starts at sample s0.
int batch_at(const RenderPlan& P, int s0) {
    const int left = P.spp - s0;
    if (P.tail <= 0 || left <= P.tail) return std::min(P.batch, left);
    return left <= P.batch + P.tail ? left - P.tail : P.batch;
}

// Dynamic LDS of a flat-kernel block whose waves hold pair queues of `queue` 16-bit entries: the
// layout the kernels form their bases from (pt_flatlds.h) — triangles and materials (Cornell:
// 2.5 KB), the prefetched camera rays, the winners, the hipRTC kernel's box table, then the
// queues and the path records.
size_t flat_lds_bytes(const pt_ctx* c, const RenderPlan& P, int queue) {
    return flat_lds_layout(3u * (unsigned)c->meta.num_tris, 2u * (unsigned)c->meta.num_tris, (unsigned)P.box_tab_bytes,
                           (unsigned)queue, (unsigned)P.rec).bytes;
}

// Flat path: (lane, leaf) pair queues of 512 16-bit entries per wave; PT_PAIRS=0
// disables them (per-lane loops), PT_PAIR_QUEUE=n shrinks them (overflow fallback).
void plan_flat(const pt_ctx* c, RenderPlan& P) {
    P.pairs = !hook_off("PT_PAIRS");
    // the hipRTC kernel's box table (box-level pairs), after the prefetched camera rays
    P.box_tab_bytes = (size_t)rtc_baked(c->meta.num_tris, c->has_specular, c->flat_boxes).box_tab_bytes;
    int queue = P.pairs ? 512 : 0;
    const char* pq = hook_env("PT_PAIR_QUEUE");
    if (P.pairs && pq && *pq) {
        queue = std::max(1, std::min(queue, atoi(pq)));
    } else if (P.pairs && c->lds_usable > 0) {
        // Shorter queues where that lets one more block per CU fit the LDS (up to the 8 the
        // registers allow): modified Cornell's 34 triangles put its block 160 B over the
        // 8-block share with 512 entries, config 5's depth-8 records fit 6 blocks, not 7.
        // A wave-iteration rarely holds more pairs than the shorter queue (overflow: the
        // per-lane loop, same bits).
        auto blocks = [&](int q) { return std::min(8, lds_blocks(c->lds_usable, flat_lds_bytes(c, P, q))); };
        const int want = blocks(kPairQueueMin);
        while (queue > kPairQueueMin && blocks(queue) < want) queue -= 32;
    }
    P.pair_queue = (queue + 3) & ~3;  // keeps the records after the queues 8-B aligned (pt_flatlds.h)
    P.lds_scene = true;
    P.lds_bytes = flat_lds_bytes(c, P, P.pair_queue);
}

// Dynamic LDS of a wide-walk block that holds the first `top` nodes of the tree.
size_t wide_lds_bytes(const pt_ctx* c, const RenderPlan& P, int top) {
    return (size_t)top * 16 * kWideNodeU4(c->meta.wide_width, c->meta.wide_fmt) + sizeof(int) * (size_t)kBlock * P.wide_rows +
           (P.wide_single ? 4 : 8) * (size_t)P.wide_queue * (kBlock / kWave) +
           (sizeof(float) + (P.lds_scene ? sizeof(uint8_t) : sizeof(int))) * (size_t)kBlock * P.rec +
           sizeof(unsigned long long) * kBlock + (P.lds_scene ? sizeof(float4) * 2 * (size_t)c->meta.num_umats : 0);
}

// Wide walk: LDS holds the top levels of the tree, one stack row per wide level above
// the last (a node of the last level has no inner children to push) and a
// triangle queue of 128 entries (8 B) per wave. The exact binary walk (rays with a
// zero direction component) of the wide and flat kernels keeps its stack (tree depth
// rows) in HBM.
int plan_wide(const pt_ctx* c, RenderPlan& P) {
    if (c->meta.num_tris >= (1 << 26))  // queue entries hold the triangle index in 32 bits, count in 26
        return set_error(PT_E_ARG, "wide path: %d triangles exceed 2^26", c->meta.num_tris);
    P.wide_rows = std::max(1, c->meta.wide_depth - 1);
    P.wide_queue = 160;  // 128: -0.35 % on config 4 (profiles/r03y_lds); PT_WIDE_QUEUE_LEN (tuning hook) sets another length
    // (an empty PT_WIDE_QUEUE_LEN reads as 0 and clamps to 64, unlike hook_int's hooks)
    if (const char* wl = hook_env("PT_WIDE_QUEUE_LEN")) P.wide_queue = std::max(64, std::min(1024, atoi(wl)));
    P.wide_top = c->meta.wide_top;  // may shrink (shrink_wide_top), to keep the occupancy
    P.wide_single = c->meta.wide_single && !hook_off("PT_WIDE_SINGLE");  // test hook: 0 = the general leaf-range decode
    // the distinct materials go to LDS when there are few (PT_UMAT_LDS_MAX: test hook)
    P.lds_scene = c->meta.num_umats <= std::min(hook_int("PT_UMAT_LDS_MAX", kMaxLdsMaterials), kMaxLdsRowsByte);
    P.lds_bytes = wide_lds_bytes(c, P, P.wide_top);
    return PT_OK;
}

// The LDS copy of the top nodes takes only what the blocks the kernel's registers
// allow per CU leave free: as many of the packed top nodes (an index prefix) as fit
// without losing a block (a lost block cost 8 %, profiles/r03y_lds).
int shrink_wide_top(const pt_ctx* c, RenderPlan& P) {
    int full = 0, with = 0, rc;
    if ((rc = occupancy((const void*)P.kern, wide_lds_bytes(c, P, 0), c->lds_usable, &full, "render"))) return rc;
    while (P.wide_top > 0) {
        if ((rc = occupancy((const void*)P.kern, wide_lds_bytes(c, P, P.wide_top), c->lds_usable, &with, "render"))) return rc;
        if (with >= full) break;
        P.wide_top--;
    }
    P.lds_bytes = wide_lds_bytes(c, P, P.wide_top);
    return PT_OK;
}

// Generic tree kernels: child-pair stack rows and two record rows per lane in LDS, and the scene
// beside them while it fits PT_LDS_SCENE_BYTES' budget and the whole block 64 KiB (no granule
// rounding: not the binary walk's place_walk rule).
void plan_tree(const pt_ctx* c, RenderPlan& P) {
    const size_t work = sizeof(int) * (size_t)kBlock * (P.stack + 2 * P.rec);
    const size_t scene = sizeof(float4) * ((size_t)2 * c->meta.num_nodes + (size_t)(3 + 2) * c->meta.num_tris);
    P.lds_scene = scene <= lds_scene_budget() && scene + work <= 64 * 1024;
    P.lds_bytes = work + (P.lds_scene ? scene : 0);
}

int theta_choice(pt_ctx* c, int* lanes, const float2** tab);  // below

// Everything a render decides before it allocates or launches: batch, kernel family, LDS
// layout, kernel and blocks per CU.
int plan_render(pt_ctx* c, const PartShape& shape, const pt_params* prm, int s_lo, int spp, bool moments, RenderPlan& P) {
    P.shape = shape;
    P.moments = moments;
    P.s_lo = s_lo;
    P.spp = spp;
    P.rec = std::max(1, prm->depth - 1);
    P.stack = std::max(1, c->meta.tree_depth);  // tree kernels: child-pair stack rows in LDS
    P.exact_rows = std::max(1, c->meta.tree_depth);
    // Wide tree for scenes past the flat list (the 99k-triangle mesh); PT_WIDE=0 disables
    // it, PT_WIDE=1 also uses it where the flat list would apply (tests).
    const char* wenv = hook_env("PT_WIDE");
    const bool flat_ok = flat_eligible(c->meta) && !hook_off("PT_FLAT");
    P.wide = c->meta.num_wide > 0 && !(wenv && *wenv == '0') && (!flat_ok || (wenv && *wenv == '1'));
    P.flat = flat_ok && !P.wide;
    plan_batch(c, prm, P);
    int rc;
    if (P.flat) plan_flat(c, P);
    else if (P.wide) {
        if ((rc = plan_wide(c, P))) return rc;
    } else plan_tree(c, P);
    if (P.lds_bytes > 160 * 1024)
        return set_error(PT_E_ARG, "BVH depth (%d) x path depth needs %zu B of LDS", P.wide ? P.wide_rows : P.stack, P.lds_bytes);
    // The hipRTC kernel: a render does not wait for its compile. Launches run the generic
    // flat kernel (the same algorithm with the box table in kernel arguments: same bits)
    // until the compile is done and switch between launches (launch_batch). PT_RTC_SWITCH=0
    // (tuning hook): renders of >= 2^28 paths wait for the compile first (round 2's rule).
    const bool rtc_switch = !hook_off("PT_RTC_SWITCH");
    P.rtc_switch_at = hook_int("PT_RTC_SWITCH_AT", -1);
    if (P.flat && c->rtc_job.valid()) rtc_resolve(c, !rtc_switch && (double)shape.npix * (spp - s_lo) >= kRtcWaitPaths);
    // The scene kernel holds what pt_ctx_set_scene fixed as constants (RtcBaked). Test hooks read at
    // the render, or a theta table that could not be allocated, can leave this plan with other
    // values: that kernel is then never launched. The render starts on the table kernel, as it does
    // while a compile is pending, and a compile of the source with the plan's values is requested.
    if ((rc = theta_choice(c, &P.theta_lanes, &P.theta_tab))) return rc;
    if (P.flat && c->rtc_requested) {
        RtcBaked want = rtc_baked(c->meta.num_tris, c->has_specular, c->flat_boxes);
        want.theta_lanes = P.theta_lanes;
        want.pairs = P.pairs;
        if (!c->rtc_baked.runs(want)) {
            c->rtc_flat = nullptr;
            c->rtc_baked = want;
            c->rtc_src = rtc_flat_source(c->flat_host, c->meta.num_leaves, c->has_specular, c->meta.coords_small, c->albedo_x2,
                                         c->dark, c->emit, want);
            c->rtc_job = rtc_job(c->rtc_src);
            c->rtc_status = "compiling";
        }
    }
    P.kern = P.flat        ? (c->flat_fast                    ? (TraceKernel)c->flat_fast
                              : ray_stack_on(c->has_specular) ? pt_trace_kernel<true, true>
                                                              : pt_trace_kernel<true, true, 0, kWideByte, false>)
             : P.wide      ? wide_kernel(c->meta.wide_width, c->meta.wide_fmt, P.lds_scene)
             : P.lds_scene ? pt_trace_kernel<true, false>
                           : pt_trace_kernel<false, false>;
    P.use_rtc = P.flat && c->rtc_flat != nullptr;
    if (P.wide && P.wide_top > 0 && (rc = shrink_wide_top(c, P))) return rc;
    // never more blocks than the measured per-CU LDS holds (the flat kernel at 8 waves: 8 blocks of <= 20,160 B)
    if ((rc = P.use_rtc ? plan_grid_module(c->rtc_flat, P.lds_bytes, c->lds_usable, c->num_cus, 0, &P.blocks_per_cu, nullptr, "render")
                        : plan_grid((const void*)P.kern, P.lds_bytes, c->lds_usable, c->num_cus, 0, &P.blocks_per_cu, nullptr, "render")))
        return rc;
    P.may_switch = P.flat && !P.use_rtc && c->rtc_job.valid();
    return PT_OK;
}

// The running sum, the output staging, the radiance slabs with their flag bits, the exact
// walk's stacks, and a moments render's double sums.
int render_buffers(pt_ctx* c, const RenderPlan& P, bool out_is_device) {
    const size_t npix = (size_t)P.shape.npix;
    int rc;
    if ((rc = ensure(&c->d_accum, &c->accum_floats, 3 * npix))) return rc;
    if (P.moments && (rc = ensure(&c->d_mom, &c->mom_doubles, 6 * npix))) return rc;
    if (!out_is_device && (rc = ensure(&c->d_out, &c->out_floats, 3 * npix))) return rc;
    if (P.wide || P.flat) {
        // a compile still running may switch this render to the hipRTC kernel, whose
        // occupancy is not known yet: stacks for the most blocks a CU holds (8 of 256)
        const size_t need = (size_t)(P.may_switch ? std::max(P.blocks_per_cu, 8) : P.blocks_per_cu) * c->num_cus * kBlock * P.exact_rows;
        if ((rc = ensure(&c->d_xstack, &c->xstack_ints, need))) return rc;
    }
    if ((rc = ensure(&c->d_radiance, &c->radiance_floats, (P.fused ? 2 : 1) * P.slab_floats))) return rc;
    if (P.flagged && (rc = ensure(&c->d_flags, &c->flags_words, (P.fused ? 2 : 1) * P.slab_words))) return rc;
    return PT_OK;
}

// The theta table (hemisphere_dir_tab, 256 MB per device, built once) only for scenes with a
// SPECULAR material, where few lanes of a wave sample the hemisphere at a time: *lanes =
// PT_THETA_LANES (tuning hook) or 32 there, else 0. Without the table (*tab = nullptr) every
// wave computes: the computed hemisphere_dir gives the same bits (the forced all-table build,
// PT_THETA_TAB == 1, has no such fallback and fails).
int theta_choice(pt_ctx* c, int* lanes, const float2** tab) {
    *lanes = 0;
    *tab = nullptr;
#if PT_THETA_TAB
    *lanes = theta_lanes_wanted(c->has_specular);
    if (PT_THETA_TAB == 1 || *lanes > 0) {
        if (int rc = theta_table(c, tab)) {
            if (PT_THETA_TAB == 1) return rc;
            *lanes = 0;
            *tab = nullptr;
        }
    }
#else
    (void)c;
#endif
    return PT_OK;
}

// Distinct leaf boxes (bitwise), each with the mask of its leaves, for the generic flat kernels'
// argument table; padding boxes set no bit. A property of the scene (pt_ctx_set_scene).
void build_flat_table(pt_ctx* c) {
    memset(&c->flat_tab, 0, sizeof(c->flat_tab));
    c->flat_boxes_padded = 0;
    if (!flat_eligible(c->meta)) return;
    int nb = 0;
    for (int k = 0; k < c->meta.num_leaves; k++) {
        const f4* L = &c->flat_host[2 * k];
        const float b6[6] = {L[0].x, L[0].y, L[0].z, L[0].w, L[1].x, L[1].y};
        int u = 0;
        while (u < nb && memcmp(c->flat_tab.box[u], b6, sizeof(b6)) != 0) u++;
        if (u == nb) {
            memcpy(c->flat_tab.box[nb], b6, sizeof(b6));
            c->flat_tab.bits[nb++] = 0;
        }
        c->flat_tab.bits[u] |= 1ull << k;
    }
    c->flat_boxes_padded = (nb + 3) & ~3;
    for (int u = nb; u < c->flat_boxes_padded; u++) memcpy(c->flat_tab.box[u], c->flat_tab.box[0], sizeof(c->flat_tab.box[0]));
}

// The fields of TraceArgs that no launch of the render changes.
int fill_trace_args(pt_ctx* c, const RenderPlan& P, const pt_camera* cam, const pt_params* prm, TraceArgs& A) {
    memset(&A, 0, sizeof(A));
    A.nodes = c->d_nodes;
    A.tris = c->d_tris;
    A.mats = c->d_mats;
    A.leaves = c->d_leaves;
    A.wide = reinterpret_cast<const uint4*>(c->d_wide);
    A.wtris = c->d_wtris;
    A.nrm = c->d_nrm;
    A.umats = c->d_umats;
    A.num_umat4 = P.wide ? 2 * c->meta.num_umats : 0;
    if (P.flat) {
        A.num_leaves = c->meta.num_leaves;
        A.num_boxes_padded = c->flat_boxes_padded;
        A.flat = c->flat_tab;
    }
    A.radiance = c->d_radiance;
    A.theta_lanes = P.theta_lanes;
    A.theta_tab = P.theta_tab;
    A.work = c->d_ctr;
    A.ctr = c->d_ctr;
    A.dark = c->dark ? 1 : 0;
    A.emit_on = emit_mode(c->emit);
    A.emit_lo_x = c->emit.lo[0], A.emit_lo_y = c->emit.lo[1], A.emit_lo_z = c->emit.lo[2];
    A.emit_hi_x = c->emit.hi[0], A.emit_hi_y = c->emit.hi[1], A.emit_hi_z = c->emit.hi[2];
    fill_camera(A, cam, P.shape, prm);
    A.depth = prm->depth;
    A.per_item = P.per_item;
    A.stack_size = P.stack;
    A.rec_size = P.rec;
    A.num_node4 = 2 * c->meta.num_nodes;
    A.num_tri4 = 3 * c->meta.num_tris;
    A.num_mat4 = 2 * c->meta.num_tris;
    A.force_exact_slab = force_exact_slab();
    // 99k mesh (r02e build): 16 -8 %, 20 -3.5 %, 24 -1.4 %, 28 best, 32 -0.7 %
    A.wide_thresh = std::max(1, std::min(64, hook_int("PT_WIDE_THRESH", 28)));
    A.pair_queue = P.pair_queue;
    A.wide_rows = P.wide_rows;
    A.exact_stack = c->d_xstack;
    A.exact_rows = P.exact_rows;
    A.wide_queue = P.wide_queue;
    A.wide_top = P.wide_top;
    A.wide_nodes = P.wide ? (uint32_t)c->meta.num_wide : 0u;
    A.wide_span_x = c->meta.wide_span[0];
    A.wide_span_y = c->meta.wide_span[1];
    A.wide_span_z = c->meta.wide_span[2];
    A.wide_single = P.wide_single ? 1 : 0;
    A.wide_compact = P.wide && c->meta.wide_compact ? 1 : 0;  // the record format (host), not a choice
    A.tri_fast = P.wide && c->meta.coords_small && !hook_off("PT_WIDE_NB") ? 1 : 0;  // test hook: 0 = tri_hit in the wide drains
    const char* wq = hook_env("PT_WIDE_QUEUE_CAP");  // test hook: a smaller queue forces drains and the fallback
    if (P.wide && wq && *wq) A.wide_queue = std::max(1, std::min(A.wide_queue, atoi(wq)));
    // camera rays generated once this many lanes want one: 32, 40 in scenes with a
    // SPECULAR material (config 3: +0.6 %, Cornell flat at 32-40; profiles/r04_knobs)
    A.regen_thresh = std::max(1, std::min(64, hook_int("PT_REGEN_THRESH", c->has_specular ? 40 : 32)));
    A.ray_reserve = ray_reserve();
    A.flags_pm = P.flags_pm;
    A.acc_chunks = 0;
    return PT_OK;
}

// The three events of every launch (start, trace done, reduce done), destroyed with the render.
struct RenderEvents {
    std::vector<hipEvent_t> ev;
    ~RenderEvents() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};

// What the launches of a render leave for its end: the last launch's figures (pt_debug_ctx_plan)
// and each launch's samples (progress).
struct LaunchLog {
    std::vector<int> samples;
    int grid = 0, chunk = 0, acc_every = 0;
    uint32_t static_items = 0;
};

// Launch b: samples [s0, s0 + sc) traced into slab b & 1, the previous slab summed on the way
// (fused) or this one summed by pt_accumulate_kernel after it.
int launch_batch(pt_ctx* c, RenderPlan& P, TraceArgs& A, int b, int s0, int sc, int prev_s0, int prev_sc, float* dst, int keep,
                 RenderEvents& E, LaunchLog& log) {
    const int npix = P.shape.npix;
    auto flags_at = [&](int k) -> uint32_t* {  // batch k's bits (the slab it writes)
        return P.flagged ? c->d_flags + (P.fused ? (size_t)(k & 1) * P.slab_words : 0) : nullptr;
    };
    A.s_begin = s0;
    A.s_count = sc;
    float* slab = c->d_radiance + (P.fused ? (size_t)(b & 1) * P.slab_floats : 0);
    A.radiance = slab;
    A.flags = flags_at(b);
    // cleared after the launch that last read these bits (stream order)
    const size_t words_b = P.flags_pm ? ((size_t)sc + 31) / 32 * npix : ((size_t)sc * npix + 31) / 32;
    if (A.flags && hipMemsetAsync(A.flags, 0, words_b * sizeof(uint32_t), c->stream) != hipSuccess)
        return set_error(PT_E_HIP, "hipMemsetAsync of the slab flags failed");
    A.total_items = (unsigned long long)((sc + P.per_item - 1) / P.per_item) * (unsigned long long)npix;
    if (A.total_items >= (1ull << 31))
        return set_error(PT_E_ARG, "batch of %d samples x %d pixels exceeds 2^31 work items", sc, npix);
    if (P.flat && !P.use_rtc && c->rtc_job.valid() && b >= 1) {
        // switch to the hipRTC kernel once its compile is done. While it is pending no
        // launch is queued ahead: launch b is enqueued when b-1's trace kernel has finished,
        // so the switch comes at the first launch boundary after the compile instead of one
        // launch later (round 6: cold headline end to end 0.627 -> 0.618-0.621 s, the device
        // idle only for the host's enqueue between two launches; profiles/r06_cold)
        (void)hipEventSynchronize(E.ev[3 * (size_t)(b - 1) + 1]);
        rtc_resolve(c, b == P.rtc_switch_at);  // test hook: the switch forced at launch b
        if (c->rtc_flat) {
            int rb = 0;
            if (int rc = plan_grid_module(c->rtc_flat, P.lds_bytes, c->lds_usable, c->num_cus, 0, &rb, nullptr, "render")) return rc;
            P.blocks_per_cu = std::min(rb, 8);
            P.use_rtc = true;
        }
    }
    const unsigned long long want_blocks = (A.total_items + kBlock - 1) / kBlock;
    const int grid = (int)std::min<unsigned long long>(want_blocks, (unsigned long long)P.blocks_per_cu * c->num_cus);
    const PoolSizing pool = pool_sizing(A.total_items, grid, P.flat ? 512 : 128);
    A.chunk = pool.chunk;
    A.static_items = pool.static_items;
    A.static_base = pool.static_base;
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    for (hipEvent_t& ek : e) {
        if (hipEventCreate(&ek) != hipSuccess) {
            for (hipEvent_t made : e)
                if (made) (void)hipEventDestroy(made);
            return set_error(PT_E_HIP, "hipEventCreate failed");
        }
    }
    E.ev.insert(E.ev.end(), e, e + 3);
    (void)hipMemsetAsync(c->d_ctr, 0, sizeof(unsigned long long), c->stream);  // work head only
    if (P.fused && prev_s0 >= 0) {  // this launch also sums the previous batch's slab
        A.acc_src = c->d_radiance + (size_t)((b - 1) & 1) * P.slab_floats;
        A.acc_flags = flags_at(b - 1);
        A.acc_sum = c->d_accum;
        A.acc_count = prev_sc;
        A.acc_first = prev_s0 == 0 ? 1 : 0;
        A.acc_chunks = (npix + kWave - 1) / kWave;
        // a chunk every acc_every-th refill of a wave: about half of them are done
        // spread over the launch's first half, the rest by waves out of trace work
        const unsigned long long refills =
            std::max<unsigned long long>(1, (A.total_items - A.static_base) / (unsigned long long)A.chunk);
        const unsigned long long div = (unsigned long long)std::max(1, hook_int("PT_ACC_DIV", 2));  // tuning hook: chunks spread over 1/div of the refills
        A.acc_every = (int)std::max<unsigned long long>(1, refills / (div * (unsigned long long)A.acc_chunks));
        (void)hipMemsetAsync(c->d_ctr + 2, 0, sizeof(unsigned long long), c->stream);  // chunk head
    } else {
        A.acc_chunks = 0;
        A.acc_flags = nullptr;
    }
    (void)hipEventRecord(e[0], c->stream);
    if (P.use_rtc) {
        size_t arg_bytes = sizeof(A);
        void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &A, HIP_LAUNCH_PARAM_BUFFER_SIZE, &arg_bytes,
                       HIP_LAUNCH_PARAM_END};
        const hipError_t le = hipModuleLaunchKernel(c->rtc_flat, grid, 1, 1, kBlock, 1, 1, (unsigned)P.lds_bytes,
                                                    c->stream, nullptr, cfg);
        if (le != hipSuccess) return set_error(PT_E_HIP, "hipModuleLaunchKernel failed: %s", hipGetErrorString(le));
    } else {
        hipLaunchKernelGGL(P.kern, dim3(grid), dim3(kBlock), P.lds_bytes, c->stream, A);
    }
    (void)hipEventRecord(e[1], c->stream);
    if (P.moments)
        hipLaunchKernelGGL(pt_accumulate_moments_kernel, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream,
                           slab, c->d_accum, dst, c->d_mom, npix, sc, s0 == 0 ? 1 : 0, s0 + sc >= P.spp ? 1 : 0,
                           (float)P.spp, A.flags, P.flags_pm);
    else if (!P.fused || s0 + sc >= P.spp)  // fused: only the last batch (the others are summed by the next launch)
        hipLaunchKernelGGL(pt_accumulate_kernel, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, slab,
                           c->d_accum, dst, npix, sc, s0 == 0 ? 1 : 0, s0 + sc >= P.spp ? 1 : 0, keep, (float)P.spp, A.flags,
                           P.flags_pm);
    (void)hipEventRecord(e[2], c->stream);
    log.samples.push_back(sc);
    log.grid = grid;
    log.chunk = A.chunk;
    log.static_items = A.static_items;
    log.acc_every = A.acc_chunks ? A.acc_every : 0;
    return PT_OK;
}

#ifdef PT_STAMPS
// PT_STAMPS builds: the kernel's section stamps of the render, on stderr.
void report_stamps(const pt_ctx* c, bool wide, const unsigned long long* h_ctr) {
    unsigned long long hs[kStampSections];
    if (hipMemcpy(hs, c->d_stamps, sizeof(hs), hipMemcpyDeviceToHost) == hipSuccess) {
        if (wide) {
            const double tot = (double)(hs[0] + hs[1] + hs[2] + hs[3] + hs[4]);
            fprintf(stderr,
                    "[stamps] wide: waves %llu  cycles/wave %.3g  start %.1f%%  steps %.1f%%  drains %.1f%%  "
                    "shade %.1f%%  fold %.1f%%  | steps/wave %.0f, traversing lanes/step %.1f, in-loop drains/wave %.0f\n",
                    hs[6], tot / (double)(hs[6] ? hs[6] : 1), 100 * hs[0] / tot, 100 * hs[1] / tot, 100 * hs[2] / tot,
                    100 * hs[3] / tot, 100 * hs[4] / tot, (double)hs[7] / (hs[6] ? hs[6] : 1),
                    (double)hs[8] / (hs[7] ? hs[7] : 1), (double)hs[9] / (hs[6] ? hs[6] : 1));
            const double oi = (double)(hs[10] ? hs[10] : 1), ray = (double)(h_ctr[1] ? h_ctr[1] : 1);
            fprintf(stderr,
                    "[stamps] wide per outer iteration: steps %.2f, shading lanes %.1f, new paths %.1f, path ends %.1f, "
                    "drain rounds %.2f (end-of-iteration %.2f), drained entries %.1f | per ray: steps %.3f, "
                    "lane-steps %.3f, triangle entries %.3f, outer iterations %.4f\n",
                    (double)hs[7] / oi, (double)hs[11] / oi, (double)hs[12] / oi, (double)hs[16] / oi,
                    (double)hs[13] / oi, (double)hs[15] / oi, (double)hs[14] / oi, (double)hs[7] / ray * (double)hs[6] / (double)(hs[6] ? hs[6] : 1),
                    (double)hs[8] / ray, (double)hs[14] / ray, (double)hs[10] / ray);
            // launch timeline (one launch per render for this line to read as one): 100 MHz ticks
            const double w = (double)(hs[6] ? hs[6] : 1);
            const unsigned long long t0 = ~hs[17], ex0 = ~hs[19];
            fprintf(stderr,
                    "[stamps] wide timeline: span %.3f ms, first exhaustion at %.3f ms, last wave end %.3f ms after it, "
                    "last exhaustion %.3f ms after it | mean wave life %.3f ms, mean end - own exhaustion %.3f ms\n",
                    (hs[18] - t0) * 1e-5, (ex0 - t0) * 1e-5, (hs[18] - ex0) * 1e-5, (hs[22] - ex0) * 1e-5,
                    hs[20] / w * 1e-5, hs[21] / w * 1e-5);
        }
        const double tot = (double)(hs[0] + hs[5] + hs[3] + hs[4]);
        if (!wide) fprintf(stderr,
                "[stamps] waves %llu  cycles/wave %.3g  start %.1f%%  intersect %.1f%% (box mask %.1f%%, "
                "pair phase %.1f%%)  shade %.1f%%  fold %.1f%%\n",
                hs[6], tot / (double)(hs[6] ? hs[6] : 1), 100 * hs[0] / tot, 100 * hs[5] / tot,
                100 * hs[1] / tot, 100 * hs[2] / tot, 100 * hs[3] / tot, 100 * hs[4] / tot);
        const double it = (double)(hs[7] ? hs[7] : 1);
        if (!wide)
            fprintf(stderr, "[stamps] per flat wave-iteration: pairs %.1f, pair rounds %.2f, max pairs of a lane %.2f, "
                    "rays credited %.2f (%llu wave-iterations)\n",
                hs[8] / it, hs[9] / it, hs[10] / it, (double)h_ctr[1] / it, hs[7]);
        if (!wide)
            fprintf(stderr, "[stamps] camera-ray generator: %.4f runs per wave-iteration, %.2f lanes per run (%llu runs)\n",
                    hs[11] / it, (double)hs[12] / (double)(hs[11] ? hs[11] : 1), hs[11]);
    }
}
#endif

int kernel_path_of(const pt_ctx* c, const RenderPlan& P) {
    return P.use_rtc                ? PT_PATH_FLAT_RTC
           : P.flat && c->flat_fast ? PT_PATH_FLAT_TABLE_FAST
           : P.flat                 ? PT_PATH_FLAT_TABLE
           : P.wide                 ? PT_PATH_WIDE
           : P.lds_scene            ? PT_PATH_TREE_LDS
                                    : PT_PATH_TREE_GLOBAL;
}

// What a call that counted runaway specular rejection loops returns.
int runaway_result(unsigned long long loops) {
    if (loops != 0)
        return set_error(PT_E_RUNAWAY, "%llu specular rejection loops hit the %d-iteration bound", loops, kMaxSpecularIters);
    return PT_OK;
}

// Progress reports, the image and the counters back, the stats and pt_debug_ctx_plan's record.
int finish_render(pt_ctx* c, const RenderPlan& P, const TraceArgs& A, const pt_params* prm, const RenderEvents& E,
                  const LaunchLog& log, float* out, const float* dst, bool out_is_device,
                  std::chrono::steady_clock::time_point t_start, pt_stats* stats) {
    const int npix = P.shape.npix, launches = (int)log.samples.size();
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return set_error(PT_E_HIP, "kernel launch failed: %s", hipGetErrorString(le));
    if (prm->progress && npix > 0) {
        // progress as each launch's samples are summed (the reference prints per row or
        // per tile, render.h:87, 136); the launches are already queued, so waiting here
        // costs the device nothing
        // A launch that failed ends the reports there: render_range returns its error
        // below, and no line claims rows that were not rendered.
        const int64_t total = (int64_t)(P.spp - P.s_lo) * npix;
        int64_t done = 0;
        for (int b = 0; b < launches; b++) {
            const hipError_t pe = hipEventSynchronize(E.ev[3 * (size_t)b + 2]);
            if (pe != hipSuccess) return set_error(PT_E_HIP, "render failed: %s", hipGetErrorString(pe));
            done += (int64_t)log.samples[(size_t)b] * npix;
            prm->progress(prm->progress_user, done, total);
        }
        if (launches == 0) prm->progress(prm->progress_user, total, total);
    }
    unsigned long long h_ctr[5] = {0, 0, 0, 0, 0};
    hipError_t e = hipMemcpyAsync(h_ctr, c->d_ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && !out_is_device && out)  // a moments render may want no image
        e = hipMemcpyAsync(out, dst, 3 * (size_t)npix * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_error(PT_E_HIP, "render failed: %s", hipGetErrorString(e));
#ifdef PT_STAMPS
    report_stamps(c, P.wide, h_ctr);
#endif
    double kms = 0, rms = 0;
    for (size_t i = 0; i + 2 < E.ev.size(); i += 3) {
        float a = 0, b = 0;
        (void)hipEventElapsedTime(&a, E.ev[i], E.ev[i + 1]);
        (void)hipEventElapsedTime(&b, E.ev[i + 1], E.ev[i + 2]);
        kms += a;
        rms += b;
    }
    const int kernel_path = kernel_path_of(c, P);
    // pt_debug_ctx_plan (pt_hip_debug.h gives the order)
    const int64_t plan[24] = {kernel_path, P.flat, P.wide, P.pairs, A.pair_queue, (int64_t)P.lds_bytes, P.lds_scene,
                              A.wide_rows, A.wide_queue, A.wide_top, launches ? P.blocks_per_cu : 0,
                              P.batch, P.per_item, P.fused, P.tail, P.flagged ? P.flags_pm : -1, launches, A.regen_thresh,
                              A.theta_lanes, log.grid, log.chunk, (int64_t)log.static_items, log.acc_every, c->num_cus};
    memcpy(c->last_plan, plan, sizeof(plan));
    c->last_early = h_ctr[4];
    if (stats) {
        stats->rays = h_ctr[1];
        stats->paths = (uint64_t)(P.spp - P.s_lo) * (uint64_t)npix;
        stats->runaway = h_ctr[3];
        stats->kernel_ms = kms;
        stats->reduce_ms = rms;
        stats->trace_launches = launches;
        stats->rows = P.shape.rows;
        stats->kernel_path = kernel_path;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return runaway_result(h_ctr[3]);
}

// Samples [s_lo, s_hi) of this part added to the running sum (a new sum when s_lo == 0),
// the image = sum / s_hi written to `out`; keep: the sum stays in d_accum (progressive).
// moments: the double sums S and Q in d_mom are started or continued with it, `out` is optional
// (NULL: the image stays in the staging buffer d_out) and the sum always stays.
int render_range(pt_ctx* c, const pt_camera* cam, const pt_params* prm, int s_lo, int s_hi, int keep, float* out,
                 int out_is_device, pt_stats* stats, bool moments = false) {
    const auto t_start = std::chrono::steady_clock::now();
    if (!c || !cam || !prm || (!out && !moments)) return set_error(PT_E_ARG, "pt_ctx_render: NULL argument");
    if (s_lo < 0 || s_hi < s_lo) return set_error(PT_E_ARG, "bad sample range [%d, %d)", s_lo, s_hi);
    if (!c->have_scene) return set_error(PT_E_ARG, "pt_ctx_render: no scene set");
    int rc;
    if ((rc = ctx_ready(c))) return rc;
    PartShape shape;
    if ((rc = part_shape(cam, prm, PT_MAX_DEPTH, &shape))) return rc;
    HIP_TRY(hipSetDevice(c->device));

    RenderPlan P;
    if ((rc = plan_render(c, shape, prm, s_lo, s_hi, moments, P))) return rc;
    const bool to_device = out_is_device && out;
    if ((rc = render_buffers(c, P, to_device))) return rc;
    float* dst = to_device ? out : c->d_out;
    TraceArgs A;
    if ((rc = fill_trace_args(c, P, cam, prm, A))) return rc;

    HIP_TRY(hipMemsetAsync(c->d_ctr, 0, 5 * sizeof(unsigned long long), c->stream));
#ifdef PT_STAMPS
    if (!c->d_stamps) HIP_TRY(hipMalloc((void**)&c->d_stamps, kStampSections * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->d_stamps, 0, kStampSections * sizeof(unsigned long long), c->stream));
    A.stamps = c->d_stamps;
#endif
    const int npix = shape.npix, spp = s_hi;
    if (s_lo == spp && npix > 0) {
        // No samples: the reference divides the zero image by 0 (render.h:97).
        if (moments)
            hipLaunchKernelGGL(pt_accumulate_moments_kernel, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream,
                               c->d_radiance, c->d_accum, dst, c->d_mom, npix, 0, s_lo == 0 ? 1 : 0, 1, (float)spp, nullptr, 0);
        else
            hipLaunchKernelGGL(pt_accumulate_kernel, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream,
                               c->d_radiance, c->d_accum, dst, npix, 0, s_lo == 0 ? 1 : 0, 1, keep, (float)spp, nullptr, 0);
    }
    RenderEvents events;
    LaunchLog log;
    int prev_s0 = -1, prev_sc = 0;
    for (int s0 = s_lo, b = 0, sc = 0; s0 < spp && npix > 0; s0 += sc, b++) {
        sc = batch_at(P, s0);
        if ((rc = launch_batch(c, P, A, b, s0, sc, prev_s0, prev_sc, dst, keep, events, log))) return rc;
        prev_s0 = s0;
        prev_sc = sc;
    }
    return finish_render(c, P, A, prm, events, log, out, dst, to_device, t_start, stats);
}

// Whether samples from s_first on continue the context's running sum of that kind (moments or
// plain progressive): the same camera, depth, seed and partition.
bool continues_sum(const pt_ctx* c, bool moments, const pt_camera* cam, const pt_params* prm, int s_first) {
    return c->prog_valid && c->prog_moments == moments && c->prog_spp == s_first &&
           memcmp(&c->prog_cam, cam, sizeof(pt_camera)) == 0 && c->prog_prm.depth == prm->depth &&
           c->prog_prm.seed == prm->seed && c->prog_prm.part_index == prm->part_index &&
           c->prog_prm.part_count == prm->part_count && c->prog_prm.band_rows == prm->band_rows;
}

void keep_sum(pt_ctx* c, bool moments, const pt_camera* cam, const pt_params* prm, int spp, int npix) {
    c->prog_valid = true;
    c->prog_moments = moments;
    c->prog_spp = spp;
    c->prog_npix = npix;
    c->prog_cam = *cam;
    c->prog_prm = *prm;
}

bool tolerances_ok(float rel, float abs_tol) { return rel >= 0.0f && abs_tol >= 0.0f && !(rel == 0.0f && abs_tol == 0.0f); }

// Samples [s_first, s_first + s_count) added to the context's moments sum (the checks and the
// bookkeeping of pt_ctx_render_moments without its export). A runaway render still leaves a
// valid sum: its code is returned after the bookkeeping.
int moments_range(pt_ctx* c, const pt_camera* cam, const pt_params* prm, int32_t s_first, int32_t s_count, float* out,
                  int out_is_device, pt_stats* stats) {
    if (!c || !cam || !prm) return set_error(PT_E_ARG, "pt_ctx_render_moments: NULL argument");
    if (s_first < 0 || s_count < 0 || (long long)s_first + s_count > 0x7fffffffll)
        return set_error(PT_E_ARG, "pt_ctx_render_moments: bad sample range");
    if (s_first > 0 && !continues_sum(c, true, cam, prm, s_first))
        return set_error(PT_E_ARG,
                         "moments render: samples from %d do not continue this context's running moments sum "
                         "(%d samples, a progressive sum, or another camera / parameters)",
                         s_first, c->prog_valid && c->prog_moments ? c->prog_spp : 0);
    c->prog_valid = false;
    PartShape shape;
    if (int rc = part_shape(cam, prm, PT_MAX_DEPTH, &shape)) return rc;
    const int rc = render_range(c, cam, prm, s_first, s_first + s_count, 1, out, out_is_device, stats, true);
    if (rc && rc != PT_E_RUNAWAY) return rc;
    keep_sum(c, true, cam, prm, s_first + s_count, shape.npix);
    return rc;
}

// The context's moments over npix pixels to the caller's arrays (device or host pointers): S and Q
// are copies of d_mom's halves, sem is computed from them with n = spp, or with each pixel's own n
// (d_spp, after per-pixel rounds). Synchronous.
int moments_export(pt_ctx* c, const pt_moments* mom, int is_device, int npix, int spp, const int32_t* d_spp = nullptr) {
    const size_t nval = 3 * (size_t)npix;
    if (!mom || nval == 0) return PT_OK;
    const hipMemcpyKind kind = is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (mom->sum) HIP_TRY(hipMemcpyAsync(mom->sum, c->d_mom, nval * sizeof(double), kind, c->stream));
    if (mom->sumsq) HIP_TRY(hipMemcpyAsync(mom->sumsq, c->d_mom + nval, nval * sizeof(double), kind, c->stream));
    if (mom->sem) {
        if (!is_device)
            if (int rc = ensure(&c->d_sem, &c->sem_floats, nval)) return rc;
        float* dst = is_device ? mom->sem : c->d_sem;
        if (d_spp) {
            if (int rc = adaptive_sem(c->stream, c->d_mom, nval, d_spp, dst)) return rc;
        } else {
            hipLaunchKernelGGL(pt_moments_sem_kernel, dim3((unsigned)((nval + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                               c->stream, c->d_mom, nval, spp, dst);
            HIP_TRY(hipGetLastError());
        }
        if (!is_device) HIP_TRY(hipMemcpyAsync(mom->sem, dst, nval * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

// The unconverged pixels of the context's moments sum (pt_unconverged_kernel); ms (optional): the
// kernel's duration is added.
int unconverged_count(pt_ctx* c, float rel, float abs_tol, int64_t* count, uint8_t* mask, int mask_is_device, double* ms) {
    const int npix = c->prog_npix;
    *count = 0;
    if (npix <= 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->d_mcount) HIP_TRY(hipMalloc((void**)&c->d_mcount, sizeof(unsigned long long)));
    uint8_t* d_mask = mask;
    if (mask && !mask_is_device) {
        if (int rc = ensure(&c->d_rgb8, &c->rgb8_bytes, (size_t)npix)) return rc;  // the 8-bit staging buffer
        d_mask = c->d_rgb8;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ms && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) {
        if (e0) (void)hipEventDestroy(e0);
        return set_error(PT_E_HIP, "hipEventCreate failed");
    }
    unsigned long long h = 0;
    hipError_t e = hipMemsetAsync(c->d_mcount, 0, sizeof(unsigned long long), c->stream);
    if (ms) (void)hipEventRecord(e0, c->stream);
    hipLaunchKernelGGL(pt_unconverged_kernel, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->d_mom, npix,
                       c->prog_spp, (double)rel, (double)abs_tol, c->d_mcount, d_mask);
    if (ms) (void)hipEventRecord(e1, c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&h, c->d_mcount, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && mask && !mask_is_device)
        e = hipMemcpyAsync(mask, d_mask, (size_t)npix, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (ms) {
        float t = 0;
        if (e == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess) *ms += t;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    if (e != hipSuccess) return set_error(PT_E_HIP, "convergence count failed: %s", hipGetErrorString(e));
    *count = (int64_t)h;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pt_ctx_create(int device, pt_ctx** out) {
    if (!out) return set_error(PT_E_ARG, "pt_ctx_create: out is NULL");
    *out = nullptr;
    // PT_TIME_CTX=1 (test hook): each phase's wall time on stderr (cold-start accounting)
    const bool timed = hook_env("PT_TIME_CTX") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto phase = [&](const char* what) {
        if (!timed) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[pt_ctx_create] %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
        t_last = t;
    };
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return set_error(PT_E_HIP, "no HIP device available");
    if (device < 0 || device >= n) return set_error(PT_E_ARG, "device %d out of range (have %d)", device, n);
    HIP_TRY(hipSetDevice(device));
    phase("device count + set");
    pt_ctx* c = new pt_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        delete c;
        return set_error(PT_E_HIP, "hipGetDeviceProperties failed");
    }
    phase("device properties");
    c->num_cus = prop.multiProcessorCount;
    // the measured per-CU LDS bound (kLdsUsable) is a gfx950 figure; another device uses
    // what it reports for itself
    c->lds_usable = strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? kLdsUsable
                    : prop.sharedMemPerMultiprocessor > 0   ? (size_t)prop.sharedMemPerMultiprocessor
                                                            : (size_t)65536;
    auto make = [c] {
        if (hipSetDevice(c->device) != hipSuccess) c->init_error = "hipSetDevice failed";
        else if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
            c->init_error = "stream creation failed";
        else if (hipMalloc((void**)&c->d_ctr, 5 * sizeof(unsigned long long)) != hipSuccess)
            c->init_error = "counter allocation failed";
    };
    // PT_CTX_SYNC=1 (test hook): made here, as before round 6
    const char* cs = hook_env("PT_CTX_SYNC");
    if (!(cs && *cs == '1')) {
        try {
            c->init = std::thread(make);
        } catch (const std::system_error&) {
        }
    }
    if (!c->init.joinable()) make();
    if (!c->init_error.empty()) {
        const std::string err = c->init_error;
        pt_ctx_destroy(c);
        return set_error(PT_E_HIP, "%s", err.c_str());
    }
    phase("stream + counter (started)");
    {
        std::lock_guard<std::mutex> lock(g_dev_mu);
        g_dev_contexts[device]++;
    }
    c->counted = true;
    g_ctx_created++;
    *out = c;
    return PT_OK;
}

void pt_ctx_destroy(pt_ctx* c) {
    if (!c) return;
    (void)ctx_ready(c);  // the init thread is done with the context
    bool last = false;
    if (c->counted) {  // a fully created context (pt_ctx_create counts only those)
        std::lock_guard<std::mutex> lock(g_dev_mu);
        last = --g_dev_contexts[c->device] == 0;
    }
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (last) theta_table_release(c->device);  // no context left on the device to read it (re-checked there)
    for (void* p : {(void*)c->d_nodes, (void*)c->d_tris, (void*)c->d_mats, (void*)c->d_leaves, (void*)c->d_wide, (void*)c->d_wtris, (void*)c->d_nrm, (void*)c->d_umats, (void*)c->d_radiance, (void*)c->d_flags,
                    (void*)c->d_accum, (void*)c->d_out, (void*)c->d_ctr, (void*)c->d_stamps, (void*)c->d_rgb8, (void*)c->d_thr, (void*)c->d_xstack,
                    (void*)c->d_rank_tri, (void*)c->d_qstack, (void*)c->d_qbuf, (void*)c->d_qhits,
                    (void*)c->d_tslab, (void*)c->d_trec, (void*)c->d_tbuf, (void*)c->d_tstates, (void*)c->d_tctr,
                    (void*)c->d_lights,
                    (void*)c->d_gtab, (void*)c->d_gmats, (void*)c->d_gbuf, (void*)c->d_mom, (void*)c->d_mcount, (void*)c->d_sem,
                    (void*)c->d_alist[0], (void*)c->d_alist[1], (void*)c->d_aspp, (void*)c->d_aslab, (void*)c->d_arec, (void*)c->d_actr})
        if (p) (void)hipFree(p);
    for (void* p : c->d_dn)
        if (p) (void)hipFree(p);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int pt_ctx_set_scene(pt_ctx* c, const pt_scene* scene) {
    if (!c) return set_error(PT_E_ARG, "context is NULL");
    g_scene_uploads++;
    PackedScene ps;
    int rc = pack_scene(scene, ps);
    if (rc) return rc;
    // the scene's flags (the radiance bound and the dark-path gate read the materials and
    // normals, which are dropped after the upload)
    const bool specular = scene_has_specular(ps);
    const bool albedo_x2 = albedo_x2_ok(ps);
    const bool dark = scene_dark(ps);
    const EmitBox emit = scene_emit_box(ps, dark);
    // The scene-specialised kernel's compile starts before the upload (and before the
    // context's stream is waited for): renders pick it up (render_range: rtc_resolve).
    const bool want_rtc = flat_eligible(ps) && !hook_off("PT_RTC");
    std::string src;
    RtcFuture job;
    RtcBaked baked;
    if (want_rtc) {
        baked = rtc_baked(ps.num_tris, specular, flat_box_pairs(ps.leaves, ps.num_leaves));
        src = rtc_flat_source(ps.leaves, ps.num_leaves, specular, ps.coords_small, albedo_x2, dark, emit, baked);
        job = rtc_job(src);
    }
    if ((rc = ctx_ready(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    for (float4** p : {&c->d_nodes, &c->d_tris, &c->d_mats, &c->d_leaves, &c->d_wide, &c->d_wtris, &c->d_nrm, &c->d_umats}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    if (c->d_rank_tri) (void)hipFree(c->d_rank_tri);
    c->d_rank_tri = nullptr;
    c->have_scene = false;
    c->prog_valid = false;
    c->temporal.valid = false;
    c->lights_uploaded = false, scene_light_table(scene, c->lights);  // the light table of pt_ctx_*_nee
    HIP_TRY(hipMalloc((void**)&c->d_nodes, ps.nodes.size() * sizeof(float4)));
    HIP_TRY(hipMalloc((void**)&c->d_tris, ps.tris.size() * sizeof(float4)));
    HIP_TRY(hipMalloc((void**)&c->d_mats, ps.mats.size() * sizeof(float4)));
    HIP_TRY(hipMemcpyAsync(c->d_nodes, ps.nodes.data(), ps.nodes.size() * sizeof(float4), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_tris, ps.tris.data(), ps.tris.size() * sizeof(float4), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_mats, ps.mats.data(), ps.mats.size() * sizeof(float4), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMalloc((void**)&c->d_rank_tri, ps.rank_tri.size() * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(c->d_rank_tri, ps.rank_tri.data(), ps.rank_tri.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, c->stream));
    if (!ps.leaves.empty()) {
        HIP_TRY(hipMalloc((void**)&c->d_leaves, ps.leaves.size() * sizeof(float4)));
        HIP_TRY(hipMemcpyAsync(c->d_leaves, ps.leaves.data(), ps.leaves.size() * sizeof(float4),
                               hipMemcpyHostToDevice, c->stream));
    }
    if (!ps.wide.empty()) {
        HIP_TRY(hipMalloc((void**)&c->d_wide, ps.wide.size() * sizeof(float4)));
        HIP_TRY(hipMemcpyAsync(c->d_wide, ps.wide.data(), ps.wide.size() * sizeof(float4), hipMemcpyHostToDevice,
                               c->stream));
        HIP_TRY(hipMalloc((void**)&c->d_wtris, ps.wtris.size() * sizeof(float4)));
        HIP_TRY(hipMemcpyAsync(c->d_wtris, ps.wtris.data(), ps.wtris.size() * sizeof(float4), hipMemcpyHostToDevice,
                               c->stream));
        HIP_TRY(hipMalloc((void**)&c->d_nrm, ps.nrm.size() * sizeof(float4)));
        HIP_TRY(hipMemcpyAsync(c->d_nrm, ps.nrm.data(), ps.nrm.size() * sizeof(float4), hipMemcpyHostToDevice,
                               c->stream));
        HIP_TRY(hipMalloc((void**)&c->d_umats, ps.umats.size() * sizeof(float4)));
        HIP_TRY(hipMemcpyAsync(c->d_umats, ps.umats.data(), ps.umats.size() * sizeof(float4), hipMemcpyHostToDevice,
                               c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    ps.wide.clear();
    ps.wtris.clear();
    ps.nrm.clear();
    ps.umats.clear();
    ps.nodes.clear();
    ps.tris.clear();
    ps.mats.clear();
    ps.rank_tri.clear();
    c->has_specular = specular;
    c->dark = dark;
    c->emit = emit;
    c->albedo_x2 = false;
    // the table kernel a flat scene runs until its hipRTC kernel is ready: with the scene's
    // flags when it has the usual ones (PT_FLAT_FAST=0, test hook: the fully generic one)
    c->flat_fast = nullptr;
    if (flat_eligible(ps) && !hook_off("PT_FLAT_FAST") && leaves_single(ps.leaves, ps.num_leaves) && ps.coords_small &&
        c->dark && albedo_x2)
        c->flat_fast = flat_fast_kernel(specular, ps.num_leaves <= 32);
    c->flat_boxes = 0;
    c->rtc_requested = false;
    c->flat_host = ps.leaves;
    ps.leaves.clear();
    c->meta = ps;
    build_flat_table(c);
    c->rtc_flat = nullptr;
    c->rtc_job = RtcFuture();
    c->rtc_src.clear();
    c->rtc_status = "not a flat scene";
    if (want_rtc) {
        c->rtc_src = std::move(src);
        c->rtc_baked = baked;
        c->albedo_x2 = albedo_x2;
        c->rtc_requested = true;
        c->flat_boxes = flat_box_pairs(c->flat_host, ps.num_leaves);
        c->rtc_job = job;
        c->rtc_status = "compiling";
        // PT_RTC_WAIT=1 (test hook) waits for it here
        const char* w = hook_env("PT_RTC_WAIT");
        if ((w && *w == '1') || !rtc_async_ready()) rtc_resolve(c, true);
    }
    c->have_scene = true;
    return PT_OK;
}

// A one-shot render that exits while the compile runs: with Python's faulthandler enabled,
// 4 of 132 such processes ended in SIGSEGV after interpreter finalisation, none of 80 without a
// background compile (scripts/exit_race.sh, round 5); waiting before finalisation avoids it.
int pt_rtc_wait(void) { return rtc_wait_all(); }

int pt_ctx_prepare(pt_ctx* c) {
    if (!c) return set_error(PT_E_ARG, "context is NULL");
    if (int rc = ctx_ready(c)) return rc;
    if (c->rtc_job.valid()) {
        HIP_TRY(hipSetDevice(c->device));
        rtc_resolve(c, true);
    }
    return PT_OK;
}

int pt_ctx_render(pt_ctx* c, const pt_camera* cam, const pt_params* prm, float* out, int out_is_device,
                  pt_stats* stats) {
    if (c) c->prog_valid = false;  // d_accum is reused
    return render_range(c, cam, prm, 0, prm && prm->spp > 0 ? prm->spp : 0, 0, out, out_is_device, stats);
}

int pt_ctx_render_progressive(pt_ctx* c, const pt_camera* cam, const pt_params* prm, int32_t s_first,
                              int32_t s_count, float* out, int out_is_device, pt_stats* stats) {
    if (!c || !cam || !prm) return set_error(PT_E_ARG, "pt_ctx_render_progressive: NULL argument");
    if (s_first < 0 || s_count < 0 || (long long)s_first + s_count > 0x7fffffffll)
        return set_error(PT_E_ARG, "pt_ctx_render_progressive: bad sample range");
    if (s_first > 0 && !continues_sum(c, false, cam, prm, s_first))
        return set_error(PT_E_ARG,
                         "progressive render: samples from %d do not continue this context's running sum "
                         "(%d samples, a moments sum, or another camera / parameters)",
                         s_first, c->prog_valid && !c->prog_moments ? c->prog_spp : 0);
    c->prog_valid = false;
    const int rc = render_range(c, cam, prm, s_first, s_first + s_count, 1, out, out_is_device, stats);
    if (rc) return rc;
    keep_sum(c, false, cam, prm, s_first + s_count, 0);
    return PT_OK;
}

int pt_ctx_render_moments(pt_ctx* c, const pt_camera* cam, const pt_params* prm, int32_t s_first, int32_t s_count,
                          float* out, const pt_moments* mom, int out_is_device, pt_stats* stats) {
    const int rc = moments_range(c, cam, prm, s_first, s_count, out, out_is_device, stats);
    if (rc && rc != PT_E_RUNAWAY) return rc;
    if (int xrc = moments_export(c, mom, out_is_device, c->prog_npix, c->prog_spp)) return xrc;
    return rc;
}

int pt_ctx_unconverged(pt_ctx* c, float rel, float abs_tol, int64_t* count, uint8_t* mask, int mask_is_device) {
    if (!c || !count) return set_error(PT_E_ARG, "pt_ctx_unconverged: NULL argument");
    if (!tolerances_ok(rel, abs_tol))
        return set_error(PT_E_ARG, "pt_ctx_unconverged: rel and abs must be >= 0 and not both 0");
    if (!c->prog_valid || !c->prog_moments)
        return set_error(PT_E_ARG, "pt_ctx_unconverged: the context has no running moments sum");
    return unconverged_count(c, rel, abs_tol, count, mask, mask_is_device, nullptr);
}

int pt_ctx_render_converge(pt_ctx* c, const pt_camera* cam, const pt_params* prm, const pt_converge* cv, float* out,
                           const pt_moments* mom, int out_is_device, pt_converge_stats* cs) {
    const auto t_start = std::chrono::steady_clock::now();
    if (!c || !cam || !prm || !cv) return set_error(PT_E_ARG, "pt_ctx_render_converge: NULL argument");
    if (!tolerances_ok(cv->rel, cv->abs))
        return set_error(PT_E_ARG, "pt_ctx_render_converge: rel and abs must be >= 0 and not both 0");
    if (cv->min_spp < 2 || cv->max_spp < cv->min_spp || cv->step < 0 || cv->max_unconverged < 0)
        return set_error(PT_E_ARG, "pt_ctx_render_converge: needs 2 <= min_spp <= max_spp, step >= 0, max_unconverged >= 0");
    pt_converge_stats S{};
    int runaway = PT_OK;
    // rounds on a device image write it in place; a host image is copied once, after the last
    for (int32_t done = 0, n = cv->min_spp;;) {
        pt_stats st{};
        const int rc = moments_range(c, cam, prm, done, n - done, out_is_device ? out : nullptr, out_is_device, &st);
        if (rc && rc != PT_E_RUNAWAY) return rc;
        if (rc) runaway = rc;
        S.rays += st.rays;
        S.kernel_ms += st.kernel_ms;
        S.reduce_ms += st.reduce_ms;
        if (int urc = unconverged_count(c, cv->rel, cv->abs, &S.unconverged, nullptr, 0, &S.reduce_ms)) return urc;
        S.rounds++;
        S.spp = done = n;
        if (S.unconverged <= cv->max_unconverged || n >= cv->max_spp) break;
        const int64_t next = cv->step > 0 ? (int64_t)n + cv->step : 2 * (int64_t)n;
        n = (int32_t)std::min<int64_t>(next, cv->max_spp);
    }
    if (out && !out_is_device && c->prog_npix > 0) {
        HIP_TRY(hipMemcpyAsync(out, c->d_out, 3 * (size_t)c->prog_npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (int xrc = moments_export(c, mom, out_is_device, c->prog_npix, c->prog_spp)) return xrc;
    S.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (cs) *cs = S;
    if (runaway)
        return set_error(PT_E_RUNAWAY, "specular rejection loops hit the %d-iteration bound during the rounds", kMaxSpecularIters);
    return PT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- ray queries and first-hit AOVs
// Entry points of the kernels in pt_query.hip. They use buffers of their own (d_qstack, d_qbuf,
// d_qhits) and never d_accum, so a progressive sum stays valid across them.
namespace {

constexpr int64_t kQueryChunk = 1ll << 28;      // rays per launch: 3 * i stays below 2^31 in the kernel
constexpr int64_t kQueryHostChunk = 1ll << 22;  // rays staged at a time for a host-pointer call

QueryScene query_scene(const pt_ctx* c) {
    return QueryScene{reinterpret_cast<const f4*>(c->d_nodes), reinterpret_cast<const f4*>(c->d_tris),
                      reinterpret_cast<const f4*>(c->d_mats), c->d_rank_tri, c->meta.num_nodes, c->meta.num_tris,
                      c->meta.tree_depth};
}

int query_force_exact() {
    return force_exact_slab() ? 1 : 0;
}

// The plan's global stack (if any) and the zeroed hit counter.
int query_buffers(pt_ctx* c, const WalkPlan& plan) {
    if (plan.stack_ints > 0)
        if (int rc = ensure(&c->d_qstack, &c->qstack_ints, plan.stack_ints)) return rc;
    if (!c->d_qhits) HIP_TRY(hipMalloc((void**)&c->d_qhits, sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->d_qhits, 0, sizeof(unsigned long long), c->stream));
    return PT_OK;
}

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    int create() {
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        return PT_OK;
    }
    ~EventPair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

int query_finish(pt_ctx* c, const WalkPlan& plan, uint64_t rays, double kernel_ms, int launches,
                 std::chrono::steady_clock::time_point t_start, pt_query_stats* stats) {
    unsigned long long hits = 0;
    HIP_TRY(hipMemcpyAsync(&hits, c->d_qhits, sizeof(hits), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats) {
        stats->rays = rays;
        stats->hits = hits;
        stats->kernel_ms = kernel_ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        stats->launches = launches;
        stats->lds_scene = plan.lds_scene;
        stats->lds_stack = plan.lds_stack;
    }
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_ctx_intersect(pt_ctx* c, const float* origins, const float* dirs, int64_t n, int mode, const float* tmax,
                     float* t_out, int32_t* out, int is_device, pt_query_stats* stats) {
    const auto t_start = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return set_error(PT_E_ARG, "pt_ctx_intersect: context is NULL");
    if (mode != PT_QUERY_CLOSEST && mode != PT_QUERY_ANY) return set_error(PT_E_ARG, "pt_ctx_intersect: unknown mode %d", mode);
    if (n < 0) return set_error(PT_E_ARG, "pt_ctx_intersect: n = %lld is negative", (long long)n);
    if (!c->have_scene) return set_error(PT_E_ARG, "pt_ctx_intersect: no scene set");
    if (n == 0) return PT_OK;
    const bool any = mode == PT_QUERY_ANY;
    if (!origins || !dirs || !out || (!any && !t_out)) return set_error(PT_E_ARG, "pt_ctx_intersect: NULL argument");
    if (int rc0 = ctx_ready(c)) return rc0;
    HIP_TRY(hipSetDevice(c->device));
    const QueryScene sc = query_scene(c);
    const int64_t chunk = std::min(n, is_device ? kQueryChunk : kQueryHostChunk);
    WalkPlan plan;
    int rc;
    if ((rc = query_plan(any ? 1 : 0, sc, c->lds_usable, c->num_cus, chunk, plan))) return rc;
    if ((rc = query_buffers(c, plan))) return rc;
    // host pointers: one staging buffer [origins 3][dirs 3][tmax 1][t 1][out 1] x chunk
    float *s_org = nullptr, *s_dir = nullptr, *s_tmax = nullptr, *s_t = nullptr;
    int32_t* s_out = nullptr;
    if (!is_device) {
        if ((rc = ensure(&c->d_qbuf, &c->qbuf_floats, 9 * (size_t)chunk))) return rc;
        s_org = c->d_qbuf;
        s_dir = s_org + 3 * chunk;
        s_tmax = s_dir + 3 * chunk;
        s_t = s_tmax + chunk;
        s_out = reinterpret_cast<int32_t*>(s_t + chunk);
    }
    EventPair ev;
    if ((rc = ev.create())) return rc;
    double kernel_ms = 0;
    int launches = 0;
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int32_t m = (int32_t)std::min(chunk, n - i0);
        const float *k_org = origins + 3 * i0, *k_dir = dirs + 3 * i0, *k_tmax = tmax ? tmax + i0 : nullptr;
        float* k_t = t_out ? t_out + i0 : nullptr;
        int32_t* k_out = out + i0;
        if (!is_device) {
            HIP_TRY(hipMemcpyAsync(s_org, k_org, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(s_dir, k_dir, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            if (any && tmax)
                HIP_TRY(hipMemcpyAsync(s_tmax, k_tmax, sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            k_org = s_org;
            k_dir = s_dir;
            k_tmax = (any && tmax) ? s_tmax : nullptr;
            k_t = s_t;
            k_out = s_out;
        }
        HIP_TRY(hipEventRecord(ev.a, c->stream));
        if ((rc = query_launch(c->stream, sc, plan, any, k_org, k_dir, any ? k_tmax : nullptr, m, k_t, k_out, c->d_qstack,
                               c->d_qhits, query_force_exact())))
            return rc;
        HIP_TRY(hipEventRecord(ev.b, c->stream));
        launches++;
        if (!is_device) {
            if (!any)
                HIP_TRY(hipMemcpyAsync(t_out + i0, s_t, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(out + i0, s_out, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        kernel_ms += ms;
    }
    return query_finish(c, plan, (uint64_t)n, kernel_ms, launches, t_start, stats);
}

int pt_ctx_render_aov(pt_ctx* c, const pt_camera* cam, const pt_params* prm, int32_t sample, const pt_aov* out,
                      int out_is_device, pt_query_stats* stats) {
    const auto t_start = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c || !cam || !prm || !out) return set_error(PT_E_ARG, "pt_ctx_render_aov: NULL argument");
    if (sample < 0) return set_error(PT_E_ARG, "pt_ctx_render_aov: sample %d is negative", sample);
    if (!c->have_scene) return set_error(PT_E_ARG, "pt_ctx_render_aov: no scene set");
    PartShape shape;
    int rc;
    if ((rc = part_shape(cam, prm, -1, &shape))) return rc;  // first hits only: depth is not used
    const long long npix = shape.npix;
    if (npix == 0) return PT_OK;
    if ((rc = ctx_ready(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const QueryScene sc = query_scene(c);
    WalkPlan plan;
    if ((rc = query_plan(2, sc, c->lds_usable, c->num_cus, npix, plan))) return rc;
    if ((rc = query_buffers(c, plan))) return rc;
    // host pointers: the requested channels staged one after the other in d_qbuf
    float* const host[6] = {out->t, reinterpret_cast<float*>(out->tri), out->normal, out->albedo, out->emission, out->ray};
    const int width[6] = {1, 1, 3, 3, 3, 6};
    float* dev[6];
    if (out_is_device) {
        for (int k = 0; k < 6; k++) dev[k] = host[k];
    } else {
        size_t total = 0;
        for (int k = 0; k < 6; k++) total += host[k] ? (size_t)width[k] * npix : 0;
        if ((rc = ensure(&c->d_qbuf, &c->qbuf_floats, total))) return rc;
        size_t at = 0;
        for (int k = 0; k < 6; k++) {
            dev[k] = host[k] ? c->d_qbuf + at : nullptr;
            at += host[k] ? (size_t)width[k] * npix : 0;
        }
    }
    const pt_aov d_out{dev[0], reinterpret_cast<int32_t*>(dev[1]), dev[2], dev[3], dev[4], dev[5]};
    EventPair ev;
    if ((rc = ev.create())) return rc;
    HIP_TRY(hipEventRecord(ev.a, c->stream));
    if ((rc = aov_launch(c->stream, sc, plan, cam, prm, shape, sample, &d_out, c->d_qstack, c->d_qhits, query_force_exact())))
        return rc;
    HIP_TRY(hipEventRecord(ev.b, c->stream));
    if (!out_is_device)
        for (int k = 0; k < 6; k++)
            if (host[k])
                HIP_TRY(hipMemcpyAsync(host[k], dev[k], sizeof(float) * (size_t)width[k] * npix, hipMemcpyDeviceToHost,
                                       c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    return query_finish(c, plan, (uint64_t)npix, ms, 1, t_start, stats);
}

}  // extern "C"

// ---------------------------------------------------------------- trace() along caller-supplied rays
// pt_ctx_trace, pt_ctx_trace_nee and pt_ctx_trace_grad are one host loop (caller_rays_*) around
// three kernels: the kernel fills a dense slab [sample][ray][rgb] of one launch,
// pt_accumulate_kernel adds a ray's samples in order and divides. Launches are cut over rays only.
// The buffers are their own (d_tslab, d_trec, d_tbuf, d_tstates, d_tctr), never d_accum, so a
// progressive sum stays valid across them.
namespace {

// Three events around a launch and the pass that sums its slab: kernel = [0, 1), reduce = [1, 2).
struct LaunchTimer {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~LaunchTimer() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int create() {
        for (hipEvent_t& x : e) HIP_TRY(hipEventCreate(&x));
        return PT_OK;
    }
    int mark(int i, hipStream_t stream) {
        HIP_TRY(hipEventRecord(e[i], stream));
        return PT_OK;
    }
    // once the stream is synchronised: the two durations added to the caller's sums
    int add(double* kernel_ms, double* reduce_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e[0], e[1]));
        *kernel_ms += ms;
        HIP_TRY(hipEventElapsedTime(&ms, e[1], e[2]));
        *reduce_ms += ms;
        return PT_OK;
    }
};

// A call's counters, zeroed: work head, rays, gradient terms (pt_grad.hip), runaway, shadow
// segments and light draws (pt_nee.hip). A launch zeroes only the work head again.
constexpr int kTraceCounters = 6;
int trace_counters(pt_ctx* c) {
    if (!c->d_tctr) HIP_TRY(hipMalloc((void**)&c->d_tctr, kTraceCounters * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->d_tctr, 0, kTraceCounters * sizeof(unsigned long long), c->stream));
    return PT_OK;
}

// The fields of a PathsLaunch that no launch of a call changes (the rays, m, ray_base and, where
// launches are cut over samples, spp are the launch's own). d_qstack must have its size by now.
int paths_launch_base(pt_ctx* c, int32_t spp, int32_t depth, uint32_t seed, float* slab, unsigned long long* ctr,
                      float* grec, int dark, PathsLaunch& l) {
    l = PathsLaunch{};
    l.spp = spp;
    l.depth = depth;
    l.seed = seed;
    l.slab = slab;
    l.ctr = ctr;
    l.gstack = c->d_qstack;
    l.grec = grec;
    l.dark = dark;
    l.force_exact = query_force_exact();
    const float2* tab = nullptr;
    if (int rc = theta_choice(c, &l.theta_lanes, &tab)) return rc;
    l.theta_tab = tab;
    return PT_OK;
}

int zero_output(pt_ctx* c, void* p, size_t bytes, int is_device) {
    if (!p || bytes == 0) return PT_OK;
    if (is_device) HIP_TRY(hipMemsetAsync(p, 0, bytes, c->stream));
    else memset(p, 0, bytes);
    return PT_OK;
}

// plan: nullptr when nothing was launched; records: the kernel keeps path records.
void fill_trace_stats(pt_trace_stats* ts, const WalkPlan* plan, bool records, const unsigned long long* ctr, uint64_t paths,
                      double kernel_ms, double reduce_ms, int launches, std::chrono::steady_clock::time_point t_start) {
    if (!ts) return;
    ts->rays = ctr[1];
    ts->paths = paths;
    ts->runaway = ctr[3];
    ts->kernel_ms = kernel_ms;
    ts->reduce_ms = reduce_ms;
    ts->launches = launches;
    if (plan) {
        ts->lds_scene = plan->lds_scene;
        ts->lds_stack = plan->lds_stack;
        if (records) ts->lds_records = plan->lds_rec;
    }
    ts->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
}

// One call along the caller's rays: what the entry point asks for, what caller_rays_begin derives
// and what the launches leave behind.
struct CallerRays {
    const char* who;  // the entry point's name, for its messages
    const float *origins, *dirs;
    int64_t n;
    const pt_trace_params* prm;
    float* rgb_out;  // nullptr (pt_ctx_trace_grad without "rgb"): nothing is summed or copied
    int is_device;
    int dark;      // PathsLaunch::dark
    bool records;  // the kernel keeps path records
    std::chrono::steady_clock::time_point t_start;
    // caller_rays_begin
    int64_t m_max = 0;  // rays per launch; 0: no ray is traced
    WalkPlan plan{};
    PathsLaunch l{};
    float *s_org = nullptr, *s_dir = nullptr, *s_out = nullptr;  // a host-pointer call's staging
    // caller_rays_loop, caller_rays_end
    unsigned long long ctr[kTraceCounters] = {};
    double kernel_ms = 0, reduce_ms = 0;
    int launches = 0;
};

// What every entry point checks first, in this order. null_extra: the name of an argument of its
// own that is NULL (it comes after params), or nullptr.
int caller_rays_check(const char* who, const pt_ctx* c, const pt_trace_params* prm, const char* null_extra, int64_t n) {
    if (!c) return set_error(PT_E_ARG, "%s: context is NULL", who);
    if (!prm) return set_error(PT_E_ARG, "%s: params is NULL", who);
    if (null_extra) return set_error(PT_E_ARG, "%s: %s is NULL", who, null_extra);
    if (n < 0) return set_error(PT_E_ARG, "%s: n = %lld is negative", who, (long long)n);
    if (int rc = trace_params_check(who, prm)) return rc;
    if (!c->have_scene) return set_error(PT_E_ARG, "%s: no scene set", who);
    return PT_OK;
}

// The last check (a NULL array), then the context's stream and device.
int caller_rays_ready(const char* who, pt_ctx* c, bool null_array) {
    if (null_array) return set_error(PT_E_ARG, "%s: NULL argument", who);
    if (int rc = ctx_ready(c)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return PT_OK;
}

// Without a ray to trace (n or depth 0) the answer, rgb +0 (render.h:37), and m_max = 0. Else the
// rays per launch, the plan (plan_for(items, WalkPlan&) for m_max x spp items), the buffers, the
// zeroed counters and the launch's fixed fields.
template <class Plan>
int caller_rays_begin(pt_ctx* c, CallerRays& R, Plan&& plan_for) {
    const int64_t n = R.n, spp = R.prm->spp;
    int rc;
    if (n == 0 || R.prm->depth == 0) {
        if ((rc = zero_output(c, R.rgb_out, 3 * sizeof(float) * (size_t)n, R.is_device))) return rc;
        if (R.is_device) HIP_TRY(hipStreamSynchronize(c->stream));
        return PT_OK;
    }
    // rays per launch: m * spp < 2^31 records inside the slab budget, a host-pointer call's staging
    // (PT_TRACE_CHUNK, test hook: rays per launch)
    int64_t m_max = std::min<int64_t>(n, ((1ll << 31) - 1) / spp);
    m_max = std::min<int64_t>(m_max, (int64_t)(batch_bytes_budget(c->device, false) / (3 * sizeof(float) * (size_t)spp)));
    if (!R.is_device) m_max = std::min(m_max, kQueryHostChunk);
    if (const char* tc = hook_env("PT_TRACE_CHUNK"))
        if (*tc) m_max = std::min<int64_t>(m_max, strtoll(tc, nullptr, 10));
    R.m_max = m_max = std::max<int64_t>(m_max, 1);
    if ((rc = plan_for(m_max * spp, R.plan))) return rc;
    if (R.plan.stack_ints > 0 && (rc = ensure(&c->d_qstack, &c->qstack_ints, R.plan.stack_ints))) return rc;
    if (R.plan.rec_words > 0 && (rc = ensure(&c->d_trec, &c->trec_words, 2 * R.plan.rec_words))) return rc;
    if ((rc = ensure(&c->d_tslab, &c->tslab_floats, 3 * (size_t)(m_max * spp)))) return rc;
    if ((rc = trace_counters(c))) return rc;
    // host pointers: staging [origins 3][dirs 3][rgb 3] x m_max, and the states
    if (!R.is_device) {
        if ((rc = ensure(&c->d_tbuf, &c->tbuf_floats, 9 * (size_t)m_max))) return rc;
        R.s_org = c->d_tbuf;
        R.s_dir = R.s_org + 3 * m_max;
        R.s_out = R.s_dir + 3 * m_max;
        if (R.prm->states && (rc = ensure(&c->d_tstates, &c->tstates_words, (size_t)(m_max * spp)))) return rc;
    }
    return paths_launch_base(c, (int32_t)spp, R.prm->depth, R.prm->seed, c->d_tslab, c->d_tctr,
                             R.plan.rec_words > 0 ? c->d_trec : nullptr, R.dark, R.l);
}

// The launches, m_max rays each: stage (host pointers; then stage(i0, m), the entry point's own
// staging), zero the work head, launch(PathsLaunch), the in-order sum, copy back, synchronise.
template <class Launch, class Stage>
int caller_rays_loop(pt_ctx* c, CallerRays& R, Launch&& launch, Stage&& stage) {
    if (R.m_max == 0) return PT_OK;
    const int64_t n = R.n, spp = R.prm->spp, m_max = R.m_max;
    const uint32_t* states = R.prm->states;
    PathsLaunch& l = R.l;
    LaunchTimer timer;
    int rc;
    if ((rc = timer.create())) return rc;
    for (int64_t i0 = 0; i0 < n; i0 += m_max) {
        const int32_t m = (int32_t)std::min(m_max, n - i0);
        l.m = m;
        l.ray_base = (uint32_t)i0;
        l.org = R.origins + 3 * i0;
        l.dir = R.dirs + 3 * i0;
        l.states = states ? states + i0 * spp : nullptr;
        float* k_out = R.rgb_out ? R.rgb_out + 3 * i0 : nullptr;
        if (!R.is_device) {
            HIP_TRY(hipMemcpyAsync(R.s_org, l.org, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(R.s_dir, l.dir, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            if (states) {
                HIP_TRY(hipMemcpyAsync(c->d_tstates, l.states, sizeof(uint32_t) * (size_t)(m * spp), hipMemcpyHostToDevice,
                                       c->stream));
                l.states = reinterpret_cast<const uint32_t*>(c->d_tstates);
            }
            l.org = R.s_org;
            l.dir = R.s_dir;
            k_out = R.rgb_out ? R.s_out : nullptr;
        }
        if ((rc = stage(i0, m))) return rc;
        HIP_TRY(hipMemsetAsync(c->d_tctr, 0, sizeof(unsigned long long), c->stream));  // work head only
        if ((rc = timer.mark(0, c->stream))) return rc;
        if ((rc = launch(l))) return rc;
        if ((rc = timer.mark(1, c->stream))) return rc;
        if (k_out) {  // the ray's samples in order from +0, then / spp (image.h:27-31, 37-40)
            hipLaunchKernelGGL(pt_accumulate_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->d_tslab,
                               (float*)nullptr, k_out, (int)m, (int)spp, 1, 1, 0, (float)spp, (const uint32_t*)nullptr, 0);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = timer.mark(2, c->stream))) return rc;
        R.launches++;
        if (!R.is_device && R.rgb_out)
            HIP_TRY(hipMemcpyAsync(R.rgb_out + 3 * i0, R.s_out, 3 * sizeof(float) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = timer.add(&R.kernel_ms, &R.reduce_ms))) return rc;
    }
    return PT_OK;
}

// The counters back (synchronises; also what the entry point queued after the launches).
int caller_rays_end(pt_ctx* c, CallerRays& R) {
    if (R.m_max == 0) return PT_OK;
    HIP_TRY(hipMemcpyAsync(R.ctr, c->d_tctr, sizeof(R.ctr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PT_OK;
}

// The call's pt_trace_stats (ts may be NULL), and what the call returns: PT_OK or PT_E_RUNAWAY.
int caller_rays_stats(const CallerRays& R, pt_trace_stats* ts) {
    fill_trace_stats(ts, R.m_max ? &R.plan : nullptr, R.records, R.ctr, (uint64_t)R.n * (uint64_t)R.prm->spp, R.kernel_ms,
                     R.reduce_ms, R.launches, R.t_start);
    return runaway_result(R.ctr[3]);
}

// An entry point without steps of its own between those four.
template <class Plan, class Launch>
int caller_rays(pt_ctx* c, CallerRays& R, pt_trace_stats* ts, Plan&& plan_for, Launch&& launch) {
    int rc;
    if ((rc = caller_rays_begin(c, R, plan_for))) return rc;
    if ((rc = caller_rays_loop(c, R, launch, [](int64_t, int32_t) { return PT_OK; }))) return rc;
    if ((rc = caller_rays_end(c, R))) return rc;
    return caller_rays_stats(R, ts);
}

// ---- light sampling (pt_nee.hip)
// The context's light table on its device: uploaded by the first call after pt_ctx_set_scene.
int nee_lights(pt_ctx* c, NeeLights* out) {
    const LightTable& lt = c->lights;
    const size_t nl = lt.tri.size();
    *out = NeeLights{nullptr, nullptr, nullptr, nullptr, 0, 0.0f, 0.0f};
    if (nl == 0) return PT_OK;
    const size_t geom_b = nl * kNeeLightF4 * sizeof(f4), word_b = nl * sizeof(float);
    if (!c->lights_uploaded) {
        if (int rc = ensure(&c->d_lights, &c->lights_bytes, geom_b + 2 * word_b + lt.listed.size())) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_lights, lt.geom.data(), geom_b, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_lights + geom_b, lt.cdf.data(), word_b, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_lights + geom_b + word_b, lt.tri.data(), word_b, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_lights + geom_b + 2 * word_b, lt.listed.data(), lt.listed.size(), hipMemcpyHostToDevice,
                               c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->lights_uploaded = true;
    }
    out->geom = reinterpret_cast<const f4*>(c->d_lights);
    out->cdf = reinterpret_cast<const float*>(c->d_lights + geom_b);
    out->tri = reinterpret_cast<const int32_t*>(c->d_lights + geom_b + word_b);
    out->listed = c->d_lights + geom_b + 2 * word_b;
    out->count = (int32_t)nl;
    out->area = lt.area;
    out->kA = lt.kA;
    return PT_OK;
}

void nee_light_stats(pt_nee_stats* stats, const pt_ctx* c, const unsigned long long* ctr) {
    stats->shadow_rays = ctr[4];
    stats->light_draws = ctr[5];
    stats->lights = (int32_t)c->lights.tri.size();
    stats->light_area = c->lights.area;
}

}  // namespace

extern "C" {

// trace() (render.h:36-61) along the caller's rays: pt_paths_kernel under the shared loop.
int pt_ctx_trace(pt_ctx* c, const float* origins, const float* dirs, int64_t n, const pt_trace_params* prm,
                 float* rgb_out, int is_device, pt_trace_stats* stats) {
    const auto t_start = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    static const char who[] = "pt_ctx_trace";
    if (int rc = caller_rays_check(who, c, prm, nullptr, n)) return rc;
    if (n == 0) return PT_OK;
    if (int rc = caller_rays_ready(who, c, !origins || !dirs || !rgb_out)) return rc;
    const QueryScene sc = query_scene(c);
    CallerRays R{who, origins, dirs, n, prm, rgb_out, is_device, c->dark ? 1 : 0, true, t_start};
    return caller_rays(
        c, R, stats,
        [&](int64_t items, WalkPlan& plan) { return paths_plan(sc, c->lds_usable, c->num_cus, prm->depth, items, plan); },
        [&](const PathsLaunch& l) { return paths_launch(c->stream, sc, R.plan, l); });
}

// The light-sampling estimator along the caller's rays: pt_nee_kernel under the shared loop (no
// path records; the stats add its own counters). opt (NULL: the unweighted estimator) picks the
// kernel; nothing else of the call depends on it.
int pt_ctx_trace_nee_opt(pt_ctx* c, const float* origins, const float* dirs, int64_t n, const pt_trace_params* prm,
                         float* rgb_out, int is_device, pt_nee_stats* stats, const pt_nee_options* opt) {
    const auto t_start = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    static const char who[] = "pt_ctx_trace_nee";
    int mis;
    if (int rc = nee_options_check(who, opt, &mis)) return rc;
    if (int rc = caller_rays_check(who, c, prm, nullptr, n)) return rc;
    if (n == 0) return PT_OK;
    if (int rc = caller_rays_ready(who, c, !origins || !dirs || !rgb_out)) return rc;
    const QueryScene sc = query_scene(c);
    NeeLights lights;
    CallerRays R{who, origins, dirs, n, prm, rgb_out, is_device, 0, false, t_start};
    const int rc = caller_rays(
        c, R, stats ? &stats->trace : nullptr,
        [&](int64_t items, WalkPlan& plan) {
            if (int lrc = nee_lights(c, &lights)) return lrc;
            return nee_plan(false, mis, sc, c->lds_usable, c->num_cus, items, plan);
        },
        [&](const PathsLaunch& l) { return nee_launch(c->stream, sc, R.plan, l, lights, mis, 0, nullptr, nullptr, nullptr); });
    if (stats && (rc == PT_OK || rc == PT_E_RUNAWAY)) nee_light_stats(stats, c, R.ctr);
    return rc;
}

int pt_ctx_trace_nee(pt_ctx* c, const float* origins, const float* dirs, int64_t n, const pt_trace_params* prm,
                     float* rgb_out, int is_device, pt_nee_stats* stats) {
    return pt_ctx_trace_nee_opt(c, origins, dirs, n, prm, rgb_out, is_device, stats, nullptr);
}

// The estimator along the part's own camera rays: pt_nee_cam_kernel fills a dense slab
// [sample][pixel][rgb] of one launch, and the render's accumulation passes sum a pixel's samples
// in order (pt_accumulate_kernel; with moments pt_accumulate_moments_kernel). Launches are cut over
// samples: c samples with npix * c < 2^31 records inside the slab budget (PT_NEE_CHUNK, test hook:
// samples per launch). The sums use the render's buffers, so a running sum ends here.
int pt_ctx_render_nee_opt(pt_ctx* c, const pt_camera* cam, const pt_params* prm, float* img_out, const pt_moments* mom,
                          int is_device, pt_nee_stats* stats, const pt_nee_options* opt) {
    const auto t_start = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    int mis;
    if (int orc = nee_options_check("pt_ctx_render_nee", opt, &mis)) return orc;
    if (!c || !cam || !prm || !img_out) return set_error(PT_E_ARG, "pt_ctx_render_nee: NULL argument");
    if (prm->spp < 1) return set_error(PT_E_ARG, "pt_ctx_render_nee: spp %d", prm->spp);
    if (!c->have_scene) return set_error(PT_E_ARG, "pt_ctx_render_nee: no scene set");
    PartShape shape;
    int rc;
    if ((rc = part_shape(cam, prm, PT_MAX_DEPTH, &shape))) return rc;
    c->prog_valid = false;
    const int npix = shape.npix, spp = prm->spp;
    if (npix == 0) return PT_OK;
    if ((rc = ctx_ready(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const bool moments = mom && (mom->sum || mom->sumsq || mom->sem);
    const size_t nval = 3 * (size_t)npix;
    if ((rc = ensure(&c->d_accum, &c->accum_floats, nval))) return rc;
    if (moments && (rc = ensure(&c->d_mom, &c->mom_doubles, 2 * nval))) return rc;
    if (!is_device && (rc = ensure(&c->d_out, &c->out_floats, nval))) return rc;
    float* dst = is_device ? img_out : c->d_out;
    // samples per launch
    int64_t c_max = std::min<int64_t>(spp, ((1ll << 31) - 1) / npix);
    c_max = std::min<int64_t>(c_max, (int64_t)(std::min<size_t>(batch_bytes_budget(c->device, false), (size_t)4 << 30) /
                                               (sizeof(float) * nval)));
    if (const char* nc = hook_env("PT_NEE_CHUNK"))
        if (*nc) c_max = std::min<int64_t>(c_max, strtoll(nc, nullptr, 10));
    c_max = std::max<int64_t>(c_max, 1);
    const QueryScene sc = query_scene(c);
    NeeLights lights;
    WalkPlan plan;
    PathsLaunch l;
    unsigned long long h_ctr[kTraceCounters] = {};
    double kernel_ms = 0, reduce_ms = 0;
    int launches = 0;
    LaunchTimer timer;
    if ((rc = timer.create())) return rc;
    const auto accumulate = [&](int count, int first, int last) {
        if (moments)
            hipLaunchKernelGGL(pt_accumulate_moments_kernel, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream,
                               c->d_tslab, c->d_accum, dst, c->d_mom, npix, count, first, last, (float)spp,
                               (const uint32_t*)nullptr, 0);
        else
            hipLaunchKernelGGL(pt_accumulate_kernel, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->d_tslab,
                               c->d_accum, dst, npix, count, first, last, 0, (float)spp, (const uint32_t*)nullptr, 0);
    };
    if (prm->depth == 0) {  // no segment is walked: every sample is +0
        if ((rc = ensure(&c->d_tslab, &c->tslab_floats, 1))) return rc;
        // spp zero records would give the same sums: S = Q = +0, the image +0 / spp
        accumulate(0, 1, 1);
        HIP_TRY(hipGetLastError());
    } else {
        if ((rc = nee_lights(c, &lights))) return rc;
        if ((rc = nee_plan(true, mis, sc, c->lds_usable, c->num_cus, (int64_t)npix * c_max, plan))) return rc;
        if ((rc = ensure(&c->d_tslab, &c->tslab_floats, nval * (size_t)c_max))) return rc;
        if (plan.stack_ints > 0 && (rc = ensure(&c->d_qstack, &c->qstack_ints, plan.stack_ints))) return rc;
        if ((rc = trace_counters(c))) return rc;
        if ((rc = paths_launch_base(c, 0, prm->depth, prm->seed, c->d_tslab, c->d_tctr, nullptr, 0, l))) return rc;
        l.m = npix;
        for (int s0 = 0; s0 < spp; s0 += (int)c_max) {
            const int sc_n = (int)std::min<int64_t>(c_max, spp - s0);
            l.spp = sc_n;
            HIP_TRY(hipMemsetAsync(c->d_tctr, 0, sizeof(unsigned long long), c->stream));  // work head only
            if ((rc = timer.mark(0, c->stream))) return rc;
            if ((rc = nee_launch(c->stream, sc, plan, l, lights, mis, s0, cam, prm, &shape))) return rc;
            if ((rc = timer.mark(1, c->stream))) return rc;
            accumulate(sc_n, s0 == 0 ? 1 : 0, s0 + sc_n == spp ? 1 : 0);
            HIP_TRY(hipGetLastError());
            if ((rc = timer.mark(2, c->stream))) return rc;
            launches++;
            HIP_TRY(hipStreamSynchronize(c->stream));
            if ((rc = timer.add(&kernel_ms, &reduce_ms))) return rc;
        }
        HIP_TRY(hipMemcpyAsync(h_ctr, c->d_tctr, sizeof(h_ctr), hipMemcpyDeviceToHost, c->stream));
    }
    // the image and the moments (n = spp) to the caller
    if (!is_device) HIP_TRY(hipMemcpyAsync(img_out, dst, sizeof(float) * nval, hipMemcpyDeviceToHost, c->stream));
    if ((rc = moments_export(c, moments ? mom : nullptr, is_device, npix, spp))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats) {
        fill_trace_stats(&stats->trace, prm->depth > 0 ? &plan : nullptr, false, h_ctr, (uint64_t)npix * (uint64_t)spp, kernel_ms,
                         reduce_ms, launches, t_start);
        nee_light_stats(stats, c, h_ctr);
    }
    return runaway_result(h_ctr[3]);
}

int pt_ctx_render_nee(pt_ctx* c, const pt_camera* cam, const pt_params* prm, float* img_out, const pt_moments* mom,
                      int is_device, pt_nee_stats* stats) {
    return pt_ctx_render_nee_opt(c, cam, prm, img_out, mom, is_device, stats, nullptr);
}

// Material gradients of trace() along the caller's rays (pt_grad.hip):
// pt_grad_kernel under the shared loop, with grad_rgb staged beside the rays. Before the launches
// the gradient table is zeroed and, with an override, the per-call materials are gathered; after
// them the table is split into the caller's two arrays.
int pt_ctx_trace_grad(pt_ctx* c, const float* origins, const float* dirs, int64_t n, const pt_trace_params* prm,
                      const pt_trace_grad_io* io, int is_device, pt_grad_stats* stats) {
    const auto t_start = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    static const char who[] = "pt_ctx_trace_grad";
    if (int rc = caller_rays_check(who, c, prm, io ? nullptr : "io", n)) return rc;
    const bool want_grad = io->grad_color || io->grad_emit;
    if (want_grad && !io->grad_rgb && n > 0)
        return set_error(PT_E_ARG, "pt_ctx_trace_grad: grad_rgb is NULL but a gradient is asked for");
    if (int rc = caller_rays_ready(who, c, n > 0 && (!origins || !dirs))) return rc;
    const int32_t T = c->meta.num_tris;  // the caller's triangles (one tri_idx position each)
    const size_t g_bytes = 3 * sizeof(double) * (size_t)T;
    const QueryScene sc = query_scene(c);
    pt_trace_stats* ts = stats ? &stats->trace : nullptr;
    GradPlan plan;
    CallerRays R{who, origins, dirs, n, prm, io->rgb_out, is_device, 0, true, t_start};
    int rc;
    if (n == 0 || prm->depth == 0)  // no ray is traced: the gradients are +0 as well (caller_rays_begin waits for them)
        if ((rc = zero_output(c, io->grad_color, g_bytes, is_device)) || (rc = zero_output(c, io->grad_emit, g_bytes, is_device)))
            return rc;
    if ((rc = caller_rays_begin(c, R, [&](int64_t items, WalkPlan& walk) {
            const int prc = grad_plan(sc, T, c->lds_usable, c->num_cus, prm->depth, items, plan);
            walk = plan.walk;
            return prc;
        })))
        return rc;
    if (R.m_max == 0) return caller_rays_stats(R, ts);
    if ((rc = ensure(&c->d_gtab, &c->gtab_doubles, 12 * (size_t)T))) return rc;  // table, then the split outputs
    // host pointers: [color 3T][emit 3T][grad_rgb 3 m_max] beside the loop's staging
    float* s_grgb = nullptr;
    const float *d_color = io->color, *d_emit = io->emit;
    if (!is_device) {
        if ((rc = ensure(&c->d_gbuf, &c->gbuf_floats, 6 * (size_t)T + 3 * (size_t)R.m_max))) return rc;
        s_grgb = c->d_gbuf + 6 * (size_t)T;
    }
    EventPair evg, evs;
    if ((rc = evg.create()) || (rc = evs.create())) return rc;
    HIP_TRY(hipEventRecord(evg.a, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_gtab, 0, 6 * sizeof(double) * (size_t)T, c->stream));
    const f4* mats = sc.mats;
    if (io->color || io->emit) {
        if ((rc = ensure(&c->d_gmats, &c->gmats_f4, 2 * (size_t)T))) return rc;
        if (!is_device) {
            if (io->color) {
                HIP_TRY(hipMemcpyAsync(c->d_gbuf, io->color, 3 * sizeof(float) * (size_t)T, hipMemcpyHostToDevice, c->stream));
                d_color = c->d_gbuf;
            }
            if (io->emit) {
                HIP_TRY(hipMemcpyAsync(c->d_gbuf + 3 * (size_t)T, io->emit, 3 * sizeof(float) * (size_t)T,
                                       hipMemcpyHostToDevice, c->stream));
                d_emit = c->d_gbuf + 3 * (size_t)T;
            }
        }
        if ((rc = grad_gather_mats(c->stream, sc, d_color, d_emit, reinterpret_cast<f4*>(c->d_gmats)))) return rc;
        mats = reinterpret_cast<const f4*>(c->d_gmats);
    }
    HIP_TRY(hipEventRecord(evg.b, c->stream));
    GradLaunch gl{};
    gl.mats = mats;
    gl.table = c->d_gtab;
    gl.table_rows = T;
    gl.want_rgb = io->rgb_out ? 1 : 0;
    gl.want_color = io->grad_color ? 1 : 0;
    gl.want_emit = io->grad_emit ? 1 : 0;
    rc = caller_rays_loop(
        c, R,
        [&](const PathsLaunch& l) {
            gl.p = l;
            return grad_launch(c->stream, sc, plan, gl);
        },
        [&](int64_t i0, int32_t m) -> int {
            gl.grad_rgb = want_grad ? io->grad_rgb + 3 * i0 : nullptr;
            if (want_grad && !is_device) {
                HIP_TRY(hipMemcpyAsync(s_grgb, gl.grad_rgb, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
                gl.grad_rgb = s_grgb;
            }
            return PT_OK;
        });
    if (rc) return rc;
    // the table's rows into the caller's two arrays
    HIP_TRY(hipEventRecord(evs.a, c->stream));
    if (want_grad) {
        double* o_color = io->grad_color ? (is_device ? io->grad_color : c->d_gtab + 6 * (size_t)T) : nullptr;
        double* o_emit = io->grad_emit ? (is_device ? io->grad_emit : c->d_gtab + 9 * (size_t)T) : nullptr;
        if ((rc = grad_split_table(c->stream, c->d_gtab, T, o_color, o_emit))) return rc;
        if (!is_device) {
            if (o_color) HIP_TRY(hipMemcpyAsync(io->grad_color, o_color, g_bytes, hipMemcpyDeviceToHost, c->stream));
            if (o_emit) HIP_TRY(hipMemcpyAsync(io->grad_emit, o_emit, g_bytes, hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIP_TRY(hipEventRecord(evs.b, c->stream));
    if ((rc = caller_rays_end(c, R))) return rc;
    if (stats) {
        float gather_ms = 0, split_ms = 0;
        HIP_TRY(hipEventElapsedTime(&gather_ms, evg.a, evg.b));
        HIP_TRY(hipEventElapsedTime(&split_ms, evs.a, evs.b));
        stats->terms = R.ctr[2];
        stats->grad_ms = (double)gather_ms + (double)split_ms;
        stats->lds_table = plan.lds_tab;
    }
    return caller_rays_stats(R, ts);
}

// Material gradients of the light-sampling estimator along the caller's rays (pt_nee_grad.hip,
// DESIGN.md §3.26): pt_nee_grad_kernel under the shared loop, staged as pt_ctx_trace_grad stages
// its call. Before the launches the table is zeroed, the per-call materials are gathered (with an
// override) and so is every light's emission (always: the kernel never reads the light table's
// own copy); after them the table is split into the caller's two arrays.
int pt_ctx_trace_nee_grad(pt_ctx* c, const float* origins, const float* dirs, int64_t n, const pt_trace_params* prm,
                          const pt_trace_grad_io* io, int is_device, pt_nee_grad_stats* stats, const pt_nee_options* opt) {
    const auto t_start = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    static const char who[] = "pt_ctx_trace_nee_grad";
    int mis;
    if (int rc = nee_options_check(who, opt, &mis)) return rc;
    if (int rc = caller_rays_check(who, c, prm, io ? nullptr : "io", n)) return rc;
    const bool want_grad = io->grad_color || io->grad_emit;
    if (want_grad && !io->grad_rgb && n > 0)
        return set_error(PT_E_ARG, "pt_ctx_trace_nee_grad: grad_rgb is NULL but a gradient is asked for");
    if (int rc = caller_rays_ready(who, c, n > 0 && (!origins || !dirs))) return rc;
    const int32_t T = c->meta.num_tris;  // the caller's triangles (one tri_idx position each)
    const size_t g_bytes = 3 * sizeof(double) * (size_t)T;
    const QueryScene sc = query_scene(c);
    pt_trace_stats* ts = stats ? &stats->nee.trace : nullptr;
    NeeGradPlan plan;
    NeeLights lights;
    CallerRays R{who, origins, dirs, n, prm, io->rgb_out, is_device, 0, true, t_start};
    int rc;
    if (n == 0 || prm->depth == 0)  // no ray is traced: the gradients are +0 as well (caller_rays_begin waits for them)
        if ((rc = zero_output(c, io->grad_color, g_bytes, is_device)) || (rc = zero_output(c, io->grad_emit, g_bytes, is_device)))
            return rc;
    if ((rc = caller_rays_begin(c, R, [&](int64_t items, WalkPlan& walk) {
            if (int lrc = nee_lights(c, &lights)) return lrc;
            const int prc = nee_grad_plan(sc, T, c->lds_usable, c->num_cus, prm->depth, items, plan);
            walk = plan.walk;
            return prc;
        })))
        return rc;
    if (R.m_max == 0) {
        if (stats) nee_light_stats(&stats->nee, c, R.ctr);
        return caller_rays_stats(R, ts);
    }
    if ((rc = ensure(&c->d_gtab, &c->gtab_doubles, 12 * (size_t)T))) return rc;  // table, then the split outputs
    // the per-call materials, then every light's emission
    if ((rc = ensure(&c->d_gmats, &c->gmats_f4, 2 * (size_t)T + (size_t)lights.count))) return rc;
    f4* const lemit = reinterpret_cast<f4*>(c->d_gmats) + 2 * (size_t)T;
    // host pointers: [color 3T][emit 3T][grad_rgb 3 m_max] beside the loop's staging
    float* s_grgb = nullptr;
    const float *d_color = io->color, *d_emit = io->emit;
    if (!is_device) {
        if ((rc = ensure(&c->d_gbuf, &c->gbuf_floats, 6 * (size_t)T + 3 * (size_t)R.m_max))) return rc;
        s_grgb = c->d_gbuf + 6 * (size_t)T;
        if (io->color) {
            HIP_TRY(hipMemcpyAsync(c->d_gbuf, io->color, 3 * sizeof(float) * (size_t)T, hipMemcpyHostToDevice, c->stream));
            d_color = c->d_gbuf;
        }
        if (io->emit) {
            HIP_TRY(hipMemcpyAsync(c->d_gbuf + 3 * (size_t)T, io->emit, 3 * sizeof(float) * (size_t)T, hipMemcpyHostToDevice,
                                   c->stream));
            d_emit = c->d_gbuf + 3 * (size_t)T;
        }
    }
    EventPair evg, evs;
    if ((rc = evg.create()) || (rc = evs.create())) return rc;
    HIP_TRY(hipEventRecord(evg.a, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_gtab, 0, 6 * sizeof(double) * (size_t)T, c->stream));
    const f4* mats = sc.mats;
    if (io->color || io->emit) {
        if ((rc = grad_gather_mats(c->stream, sc, d_color, d_emit, reinterpret_cast<f4*>(c->d_gmats)))) return rc;
        mats = reinterpret_cast<const f4*>(c->d_gmats);
    }
    if ((rc = nee_grad_gather_lights(c->stream, lights, d_emit, lemit))) return rc;
    HIP_TRY(hipEventRecord(evg.b, c->stream));
    NeeGradLaunch gl{};
    gl.mats = mats;
    gl.lemit = lemit;
    gl.table = c->d_gtab;
    gl.table_rows = T;
    gl.want_rgb = io->rgb_out ? 1 : 0;
    gl.want_color = io->grad_color ? 1 : 0;
    gl.want_emit = io->grad_emit ? 1 : 0;
    gl.mis = mis;
    rc = caller_rays_loop(
        c, R,
        [&](const PathsLaunch& l) {
            gl.p = l;
            return nee_grad_launch(c->stream, sc, plan, gl, lights);
        },
        [&](int64_t i0, int32_t m) -> int {
            gl.grad_rgb = want_grad ? io->grad_rgb + 3 * i0 : nullptr;
            if (want_grad && !is_device) {
                HIP_TRY(hipMemcpyAsync(s_grgb, gl.grad_rgb, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
                gl.grad_rgb = s_grgb;
            }
            return PT_OK;
        });
    if (rc) return rc;
    // the table's rows into the caller's two arrays
    HIP_TRY(hipEventRecord(evs.a, c->stream));
    if (want_grad) {
        double* o_color = io->grad_color ? (is_device ? io->grad_color : c->d_gtab + 6 * (size_t)T) : nullptr;
        double* o_emit = io->grad_emit ? (is_device ? io->grad_emit : c->d_gtab + 9 * (size_t)T) : nullptr;
        if ((rc = grad_split_table(c->stream, c->d_gtab, T, o_color, o_emit))) return rc;
        if (!is_device) {
            if (o_color) HIP_TRY(hipMemcpyAsync(io->grad_color, o_color, g_bytes, hipMemcpyDeviceToHost, c->stream));
            if (o_emit) HIP_TRY(hipMemcpyAsync(io->grad_emit, o_emit, g_bytes, hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIP_TRY(hipEventRecord(evs.b, c->stream));
    if ((rc = caller_rays_end(c, R))) return rc;
    if (stats) {
        float gather_ms = 0, split_ms = 0;
        HIP_TRY(hipEventElapsedTime(&gather_ms, evg.a, evg.b));
        HIP_TRY(hipEventElapsedTime(&split_ms, evs.a, evs.b));
        stats->terms = R.ctr[2];
        stats->grad_ms = (double)gather_ms + (double)split_ms;
        stats->lds_table = plan.lds_tab;
        nee_light_stats(&stats->nee, c, R.ctr);
    }
    return caller_rays_stats(R, ts);
}
}  // extern "C"

// ---------------------------------------------------------------- render gradients
// Material gradients of the rendered image along the part's own camera rays: the two gradient
// kernels fed from camera_ray (pt_grad_cam_kernel, pt_nee_grad_cam_kernel). Launches are cut over
// samples as in pt_ctx_render_nee_opt (PT_RENDER_GRAD_CHUNK, test hook: samples per launch); the
// table is zeroed once, accumulates across the launches and is split once at the end. The radiance
// slab and the in-order sum pass exist only with io->rgb_out. The buffers are the caller-ray
// gradients' own (d_tslab, d_trec, d_tbuf, d_tctr, d_gtab, d_gmats, d_gbuf), never d_accum, so a
// progressive sum stays valid.
namespace {

int render_grad_call(const char* who, pt_ctx* c, const pt_camera* cam, const pt_params* prm, const pt_trace_grad_io* io,
                     int is_device, bool nee, int mis, pt_trace_stats* ts, pt_nee_stats* ns, uint64_t* terms_out,
                     double* grad_ms_out, int32_t* lds_table_out) {
    const auto t_start = std::chrono::steady_clock::now();
    if (!c || !cam || !prm || !io) return set_error(PT_E_ARG, "%s: NULL argument", who);
    if (prm->spp < 1) return set_error(PT_E_ARG, "%s: spp %d", who, prm->spp);
    if (prm->depth < 0) return set_error(PT_E_ARG, "%s: depth %d", who, prm->depth);
    if (!c->have_scene) return set_error(PT_E_ARG, "%s: no scene set", who);
    PartShape shape;
    int rc;
    if ((rc = part_shape(cam, prm, PT_MAX_DEPTH, &shape))) return rc;
    const int npix = shape.npix, spp = prm->spp;
    const bool want_grad = io->grad_color || io->grad_emit;
    if (want_grad && !io->grad_rgb && npix > 0)
        return set_error(PT_E_ARG, "%s: grad_rgb is NULL but a gradient is asked for", who);
    if ((rc = ctx_ready(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int32_t T = c->meta.num_tris;  // the caller's triangles (one tri_idx position each)
    const size_t g_bytes = 3 * sizeof(double) * (size_t)T;
    const size_t nval = 3 * (size_t)npix;
    unsigned long long h_ctr[kTraceCounters] = {};
    if (npix == 0 || prm->depth == 0) {  // no ray is traced: every output is +0 (+0 / spp)
        if ((rc = zero_output(c, io->grad_color, g_bytes, is_device)) || (rc = zero_output(c, io->grad_emit, g_bytes, is_device)) ||
            (rc = zero_output(c, io->rgb_out, sizeof(float) * nval, is_device)))
            return rc;
        if (is_device) HIP_TRY(hipStreamSynchronize(c->stream));
        fill_trace_stats(ts, nullptr, true, h_ctr, (uint64_t)npix * (uint64_t)spp, 0, 0, 0, t_start);
        if (ns) nee_light_stats(ns, c, h_ctr);
        return PT_OK;
    }
    const bool want_rgb = io->rgb_out != nullptr;
    // samples per launch: npix * c < 2^31 items, and with a slab its budget
    int64_t c_max = std::min<int64_t>(spp, ((1ll << 31) - 1) / npix);
    if (want_rgb)
        c_max = std::min<int64_t>(c_max, (int64_t)(std::min<size_t>(batch_bytes_budget(c->device, false), (size_t)4 << 30) /
                                                   (sizeof(float) * nval)));
    if (const char* gc = hook_env("PT_RENDER_GRAD_CHUNK"))
        if (*gc) c_max = std::min<int64_t>(c_max, strtoll(gc, nullptr, 10));
    c_max = std::max<int64_t>(c_max, 1);
    const QueryScene sc = query_scene(c);
    GradPlan gplan;
    NeeGradPlan nplan;
    NeeLights lights{};
    const int64_t items = (int64_t)npix * c_max;
    if (nee) {
        if ((rc = nee_lights(c, &lights))) return rc;
        if ((rc = nee_grad_plan(sc, T, c->lds_usable, c->num_cus, prm->depth, items, nplan, true))) return rc;
    } else {
        if ((rc = grad_plan(sc, T, c->lds_usable, c->num_cus, prm->depth, items, gplan, true))) return rc;
    }
    const WalkPlan& walk = nee ? nplan.walk : gplan.walk;
    if (walk.stack_ints > 0 && (rc = ensure(&c->d_qstack, &c->qstack_ints, walk.stack_ints))) return rc;
    if (walk.rec_words > 0 && (rc = ensure(&c->d_trec, &c->trec_words, 2 * walk.rec_words))) return rc;
    if (want_rgb && (rc = ensure(&c->d_tslab, &c->tslab_floats, nval * (size_t)c_max))) return rc;
    // the running sum of the in-order pass, then (host pointers) the image's staging
    if (want_rgb && (rc = ensure(&c->d_tbuf, &c->tbuf_floats, 2 * nval))) return rc;
    if ((rc = trace_counters(c))) return rc;
    if ((rc = ensure(&c->d_gtab, &c->gtab_doubles, 12 * (size_t)T))) return rc;  // table, then the split outputs
    // the per-call materials, then (light sampling) every light's emission
    if ((rc = ensure(&c->d_gmats, &c->gmats_f4, 2 * (size_t)T + (size_t)lights.count))) return rc;
    f4* const lemit = reinterpret_cast<f4*>(c->d_gmats) + 2 * (size_t)T;
    // host pointers: [color 3T][emit 3T][grad_rgb 3 npix]
    const float *d_color = io->color, *d_emit = io->emit, *d_grgb = want_grad ? io->grad_rgb : nullptr;
    if (!is_device) {
        if ((rc = ensure(&c->d_gbuf, &c->gbuf_floats, 6 * (size_t)T + nval))) return rc;
        if (io->color) {
            HIP_TRY(hipMemcpyAsync(c->d_gbuf, io->color, 3 * sizeof(float) * (size_t)T, hipMemcpyHostToDevice, c->stream));
            d_color = c->d_gbuf;
        }
        if (io->emit) {
            HIP_TRY(hipMemcpyAsync(c->d_gbuf + 3 * (size_t)T, io->emit, 3 * sizeof(float) * (size_t)T, hipMemcpyHostToDevice,
                                   c->stream));
            d_emit = c->d_gbuf + 3 * (size_t)T;
        }
        if (want_grad) {
            HIP_TRY(hipMemcpyAsync(c->d_gbuf + 6 * (size_t)T, io->grad_rgb, sizeof(float) * nval, hipMemcpyHostToDevice, c->stream));
            d_grgb = c->d_gbuf + 6 * (size_t)T;
        }
    }
    EventPair evg, evs;
    if ((rc = evg.create()) || (rc = evs.create())) return rc;
    HIP_TRY(hipEventRecord(evg.a, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_gtab, 0, 6 * sizeof(double) * (size_t)T, c->stream));
    const f4* mats = sc.mats;
    if (io->color || io->emit) {
        if ((rc = grad_gather_mats(c->stream, sc, d_color, d_emit, reinterpret_cast<f4*>(c->d_gmats)))) return rc;
        mats = reinterpret_cast<const f4*>(c->d_gmats);
    }
    if (nee && (rc = nee_grad_gather_lights(c->stream, lights, d_emit, lemit))) return rc;
    HIP_TRY(hipEventRecord(evg.b, c->stream));
    PathsLaunch l;
    if ((rc = paths_launch_base(c, 0, prm->depth, prm->seed, want_rgb ? c->d_tslab : nullptr, c->d_tctr,
                                walk.rec_words > 0 ? c->d_trec : nullptr, 0, l)))
        return rc;
    l.m = npix;
    GradLaunch gl{};
    NeeGradLaunch ngl{};
    gl.mats = ngl.mats = mats;
    ngl.lemit = lemit;
    gl.grad_rgb = ngl.grad_rgb = d_grgb;
    gl.table = ngl.table = c->d_gtab;
    gl.table_rows = ngl.table_rows = T;
    gl.want_rgb = ngl.want_rgb = want_rgb ? 1 : 0;
    gl.want_color = ngl.want_color = io->grad_color ? 1 : 0;
    gl.want_emit = ngl.want_emit = io->grad_emit ? 1 : 0;
    ngl.mis = mis;
    gl.cam = ngl.cam = cam;
    gl.prm = ngl.prm = prm;
    gl.shape = ngl.shape = &shape;
    gl.spp_total = ngl.spp_total = spp;
    float* const accum = c->d_tbuf;
    float* const dst = want_rgb ? (is_device ? io->rgb_out : c->d_tbuf + nval) : nullptr;
    double kernel_ms = 0, reduce_ms = 0;
    int launches = 0;
    LaunchTimer timer;
    if ((rc = timer.create())) return rc;
    for (int s0 = 0; s0 < spp; s0 += (int)c_max) {
        const int sc_n = (int)std::min<int64_t>(c_max, spp - s0);
        l.spp = sc_n;
        gl.p = ngl.p = l;
        gl.s_begin = ngl.s_begin = s0;
        HIP_TRY(hipMemsetAsync(c->d_tctr, 0, sizeof(unsigned long long), c->stream));  // work head only
        if ((rc = timer.mark(0, c->stream))) return rc;
        if ((rc = nee ? nee_grad_launch(c->stream, sc, nplan, ngl, lights) : grad_launch(c->stream, sc, gplan, gl))) return rc;
        if ((rc = timer.mark(1, c->stream))) return rc;
        if (want_rgb) {  // the pixel's samples in order from +0, then / spp on the last launch (image.h:27-31, 37-40)
            hipLaunchKernelGGL(pt_accumulate_kernel, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->d_tslab,
                               accum, dst, npix, sc_n, s0 == 0 ? 1 : 0, s0 + sc_n == spp ? 1 : 0, 0, (float)spp,
                               (const uint32_t*)nullptr, 0);
            HIP_TRY(hipGetLastError());
        }
        if ((rc = timer.mark(2, c->stream))) return rc;
        launches++;
        HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = timer.add(&kernel_ms, &reduce_ms))) return rc;
    }
    // the table's rows into the caller's two arrays
    HIP_TRY(hipEventRecord(evs.a, c->stream));
    if (want_grad) {
        double* o_color = io->grad_color ? (is_device ? io->grad_color : c->d_gtab + 6 * (size_t)T) : nullptr;
        double* o_emit = io->grad_emit ? (is_device ? io->grad_emit : c->d_gtab + 9 * (size_t)T) : nullptr;
        if ((rc = grad_split_table(c->stream, c->d_gtab, T, o_color, o_emit))) return rc;
        if (!is_device) {
            if (o_color) HIP_TRY(hipMemcpyAsync(io->grad_color, o_color, g_bytes, hipMemcpyDeviceToHost, c->stream));
            if (o_emit) HIP_TRY(hipMemcpyAsync(io->grad_emit, o_emit, g_bytes, hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIP_TRY(hipEventRecord(evs.b, c->stream));
    if (want_rgb && !is_device) HIP_TRY(hipMemcpyAsync(io->rgb_out, dst, sizeof(float) * nval, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_ctr, c->d_tctr, sizeof(h_ctr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float gather_ms = 0, split_ms = 0;
    HIP_TRY(hipEventElapsedTime(&gather_ms, evg.a, evg.b));
    HIP_TRY(hipEventElapsedTime(&split_ms, evs.a, evs.b));
    if (terms_out) *terms_out = h_ctr[2];
    if (grad_ms_out) *grad_ms_out = (double)gather_ms + (double)split_ms;
    if (lds_table_out) *lds_table_out = nee ? nplan.lds_tab : gplan.lds_tab;
    fill_trace_stats(ts, &walk, true, h_ctr, (uint64_t)npix * (uint64_t)spp, kernel_ms, reduce_ms, launches, t_start);
    if (ns) nee_light_stats(ns, c, h_ctr);
    return runaway_result(h_ctr[3]);
}

}  // namespace

extern "C" {

int pt_ctx_render_grad(pt_ctx* c, const pt_camera* cam, const pt_params* prm, const pt_trace_grad_io* io, int is_device,
                       pt_grad_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return render_grad_call("pt_ctx_render_grad", c, cam, prm, io, is_device, false, PT_NEE_MIS_NONE,
                            stats ? &stats->trace : nullptr, nullptr, stats ? &stats->terms : nullptr,
                            stats ? &stats->grad_ms : nullptr, stats ? &stats->lds_table : nullptr);
}

int pt_ctx_render_nee_grad(pt_ctx* c, const pt_camera* cam, const pt_params* prm, const pt_trace_grad_io* io, int is_device,
                           pt_nee_grad_stats* stats, const pt_nee_options* opt) {
    if (stats) memset(stats, 0, sizeof(*stats));
    int mis;
    if (int orc = nee_options_check("pt_ctx_render_nee_grad", opt, &mis)) return orc;
    return render_grad_call("pt_ctx_render_nee_grad", c, cam, prm, io, is_device, true, mis,
                            stats ? &stats->nee.trace : nullptr, stats ? &stats->nee : nullptr, stats ? &stats->terms : nullptr,
                            stats ? &stats->grad_ms : nullptr, stats ? &stats->lds_table : nullptr);
}

}  // extern "C"

// ---------------------------------------------------------------- adaptive sampling
// pt_ctx_render_converge whose later rounds go only to the pixels that still miss the criterion:
// dense rounds through moments_range, then per-pixel rounds through the kernels of pt_adaptive.hip
// (the binary walk of pt_ctx_trace fed with the render's camera rays of a compacted pixel list).
namespace {

// The active fraction below which a per-pixel round pays (pt_adaptive::sparse_below = 0), by the
// kernel family of the dense rounds: 0.8 of the rate of the binary walk over the rate of the
// render's own kernel, both measured inside this call at 1024^2, depth 5 (scripts/adaptive_bench.py,
// profiles/adaptive): flat 10.4 / 53.7 Gray/s = 0.194 on Cornell (0.242 with
// emission on every surface: the lower one counts), wide 1.36 / 13.1 = 0.104 on the 99k mesh. A
// scene whose render already runs the binary walk was not measured: §3.13's ratio of about 1.
float default_sparse_below(int kernel_path) {
    switch (kernel_path) {
        case PT_PATH_FLAT_RTC:
        case PT_PATH_FLAT_TABLE:
        case PT_PATH_FLAT_TABLE_FAST: return 0.155f;
        case PT_PATH_WIDE: return 0.083f;
        default: return 0.8f;
    }
}

// The per-pixel rounds from boundary n on (the switch included): the pixels that miss the criterion
// at n are listed, the others frozen; rounds over the list until it holds at most max_unconverged
// pixels or n reaches max_spp. dst: the device image (rows*W*3). S: rounds, samples, rays, times
// and launches are added; unconverged and max_spp are set.
int adaptive_rounds(pt_ctx* c, const pt_camera* cam, const pt_params* prm, const pt_converge* cv, int32_t n, float* dst,
                    pt_adaptive_stats& S, int* runaway) {
    PartShape shape;
    int rc;
    if ((rc = part_shape(cam, prm, PT_MAX_DEPTH, &shape))) return rc;
    const int32_t npix = shape.npix;
    c->prog_valid = false;  // the running sum is no longer one of a uniform sample count
    for (int k = 0; k < 2; k++)
        if ((rc = ensure(&c->d_alist[k], &c->alist_ints[k], (size_t)npix))) return rc;
    if ((rc = ensure(&c->d_aspp, &c->aspp_ints, (size_t)npix))) return rc;
    if (!c->d_actr) HIP_TRY(hipMalloc((void**)&c->d_actr, 5 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->d_actr, 0, 5 * sizeof(unsigned long long), c->stream));
    unsigned long long* d_count = c->d_actr + 4;
    LaunchTimer timer;
    if ((rc = timer.create())) return rc;
    // the unconverged pixels of `prev` (m of them; nullptr: the part) after n samples -> d_alist[to]; 8 bytes read back
    auto compact = [&](const int32_t* prev, int32_t m, int32_t n_at, int to, int64_t* left) -> int {
        unsigned long long h = 0;
        if (int trc = timer.mark(0, c->stream)) return trc;
        if (int crc = adaptive_compact(c->stream, prev, m, c->d_mom, npix, n_at, cv->rel, cv->abs, c->d_alist[to], d_count,
                                       c->d_aspp))
            return crc;
        if (int trc = timer.mark(1, c->stream)) return trc;
        HIP_TRY(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, timer.e[0], timer.e[1]));
        S.reduce_ms += ms;
        *left = (int64_t)h;
        return PT_OK;
    };
    int cur = 0;
    int64_t m = 0;
    if ((rc = compact(nullptr, npix, n, cur, &m))) return rc;
    S.samples = (int64_t)(npix - m) * n;

    const QueryScene sc = query_scene(c);
    PathsLaunch l;  // slab, stack and records: each round's own, below
    if ((rc = paths_launch_base(c, 0, prm->depth, prm->seed, nullptr, c->d_actr, nullptr, c->dark ? 1 : 0, l))) return rc;
    // items (listed pixels x samples) per launch: the slab budget and the 2^31-item bound;
    // PT_ADAPTIVE_CHUNK (test hook): the items themselves
    int64_t items_max = std::min<int64_t>((1ll << 31) - 1, (int64_t)(batch_bytes_budget(c->device, false) / (3 * sizeof(float))));
    if (const char* ac = hook_env("PT_ADAPTIVE_CHUNK"))
        if (*ac) items_max = std::min<int64_t>(items_max, strtoll(ac, nullptr, 10));
    items_max = std::max<int64_t>(items_max, 1);

    while (m > cv->max_unconverged && n < cv->max_spp) {
        const int32_t n_next = (int32_t)std::min<int64_t>(cv->step > 0 ? (int64_t)n + cv->step : 2 * (int64_t)n, cv->max_spp);
        // a round is cut over samples first, then over listed pixels
        const int64_t m_l = std::min<int64_t>(m, items_max);
        const int64_t c_l = std::min<int64_t>(n_next - n, std::max<int64_t>(1, items_max / m_l));
        WalkPlan plan;
        if ((rc = adaptive_plan(sc, c->lds_usable, c->num_cus, prm->depth, m_l * c_l, plan))) return rc;
        if (plan.stack_ints > 0 && (rc = ensure(&c->d_qstack, &c->qstack_ints, plan.stack_ints))) return rc;
        if (plan.rec_words > 0 && (rc = ensure(&c->d_arec, &c->arec_words, 2 * plan.rec_words))) return rc;
        if ((rc = ensure(&c->d_aslab, &c->aslab_floats, 3 * (size_t)(m_l * c_l)))) return rc;
        l.slab = c->d_aslab;
        l.gstack = c->d_qstack;
        l.grec = plan.rec_words > 0 ? c->d_arec : nullptr;
        for (int64_t a0 = 0; a0 < m; a0 += m_l) {
            const int32_t* list = c->d_alist[cur] + a0;
            l.m = (int32_t)std::min<int64_t>(m_l, m - a0);
            for (int64_t s0 = n; s0 < n_next; s0 += c_l) {
                l.spp = (int32_t)std::min<int64_t>(c_l, n_next - s0);
                HIP_TRY(hipMemsetAsync(c->d_actr, 0, sizeof(unsigned long long), c->stream));  // work head only
                if ((rc = timer.mark(0, c->stream))) return rc;
                if ((rc = adaptive_launch(c->stream, sc, plan, l, list, (int32_t)s0, cam, prm, shape))) return rc;
                if ((rc = timer.mark(1, c->stream))) return rc;
                if ((rc = adaptive_accumulate(c->stream, c->d_aslab, list, l.m, l.spp, c->d_accum, c->d_mom, dst, npix,
                                              s0 + l.spp == n_next ? n_next : 0)))
                    return rc;
                if ((rc = timer.mark(2, c->stream))) return rc;
                HIP_TRY(hipStreamSynchronize(c->stream));
                double kernel_ms = 0;
                if ((rc = timer.add(&kernel_ms, &S.reduce_ms))) return rc;
                S.kernel_ms += kernel_ms;
                S.sparse_kernel_ms += kernel_ms;
                S.sparse_launches++;
            }
        }
        int64_t left = 0;
        if ((rc = compact(c->d_alist[cur], (int32_t)m, n_next, 1 - cur, &left))) return rc;
        S.samples += (m - left) * n_next;
        cur = 1 - cur;
        m = left;
        n = n_next;
        S.rounds++;
    }
    // the pixels still listed keep the last boundary
    if ((rc = adaptive_fill_spp(c->stream, c->d_alist[cur], (int32_t)m, n, c->d_aspp))) return rc;
    S.samples += m * n;
    S.unconverged = m;
    S.max_spp = n;
    unsigned long long h_ctr[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h_ctr, c->d_actr, sizeof(h_ctr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    S.sparse_rays = h_ctr[1];
    S.rays += h_ctr[1];
    if (h_ctr[3] != 0) *runaway = PT_E_RUNAWAY;
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_ctx_render_adaptive(pt_ctx* c, const pt_camera* cam, const pt_params* prm, const pt_adaptive* ad, float* out,
                           const pt_moments* mom, int32_t* spp_out, int out_is_device, pt_adaptive_stats* as) {
    const auto t_start = std::chrono::steady_clock::now();
    if (!c || !cam || !prm || !ad) return set_error(PT_E_ARG, "pt_ctx_render_adaptive: NULL argument");
    const pt_converge* cv = &ad->conv;
    if (!tolerances_ok(cv->rel, cv->abs))
        return set_error(PT_E_ARG, "pt_ctx_render_adaptive: rel and abs must be >= 0 and not both 0");
    if (cv->min_spp < 2 || cv->max_spp < cv->min_spp || cv->step < 0 || cv->max_unconverged < 0)
        return set_error(PT_E_ARG, "pt_ctx_render_adaptive: needs 2 <= min_spp <= max_spp, step >= 0, max_unconverged >= 0");
    if (ad->sparse_below != ad->sparse_below) return set_error(PT_E_ARG, "pt_ctx_render_adaptive: sparse_below is NaN");
    pt_adaptive_stats S{};
    int runaway = PT_OK;
    float below = ad->sparse_below;
    bool sparse = false;
    int32_t n = cv->min_spp;
    // dense rounds, as pt_ctx_render_converge's: on a device image they write it in place
    for (int32_t done = 0;;) {
        pt_stats st{};
        const int rc = moments_range(c, cam, prm, done, n - done, out_is_device ? out : nullptr, out_is_device, &st);
        if (rc && rc != PT_E_RUNAWAY) return rc;
        if (rc) runaway = rc;
        S.rays += st.rays;
        S.kernel_ms += st.kernel_ms;
        S.reduce_ms += st.reduce_ms;
        if (int urc = unconverged_count(c, cv->rel, cv->abs, &S.unconverged, nullptr, 0, &S.reduce_ms)) return urc;
        S.rounds++;
        S.dense_rounds++;
        S.max_spp = done = n;
        if (below == 0.0f) below = default_sparse_below(st.kernel_path);
        if (S.unconverged <= cv->max_unconverged || n >= cv->max_spp) break;
        if (below > 0.0f && (double)S.unconverged <= (double)below * (double)c->prog_npix) {
            sparse = true;
            break;
        }
        n = (int32_t)std::min<int64_t>(cv->step > 0 ? (int64_t)n + cv->step : 2 * (int64_t)n, cv->max_spp);
    }
    const int npix = c->prog_npix;
    S.samples = (int64_t)npix * n;
    if (sparse) {
        float* dst = out_is_device && out ? out : c->d_out;
        if (int rc = adaptive_rounds(c, cam, prm, cv, n, dst, S, &runaway)) return rc;
    }
    if (out && !out_is_device && npix > 0)
        HIP_TRY(hipMemcpyAsync(out, c->d_out, 3 * (size_t)npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (spp_out && npix > 0) {
        if (!sparse) {  // every pixel received the last boundary's samples
            if (int rc = ensure(&c->d_aspp, &c->aspp_ints, (size_t)npix)) return rc;
            if (int rc = adaptive_fill_spp(c->stream, nullptr, npix, n, c->d_aspp)) return rc;
        }
        HIP_TRY(hipMemcpyAsync(spp_out, c->d_aspp, (size_t)npix * sizeof(int32_t),
                               out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int xrc = moments_export(c, mom, out_is_device, npix, c->prog_spp, sparse ? c->d_aspp : nullptr)) return xrc;
    S.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (as) *as = S;
    if (runaway)
        return set_error(PT_E_RUNAWAY, "specular rejection loops hit the %d-iteration bound during the rounds", kMaxSpecularIters);
    return PT_OK;
}

}  // extern "C"

int pt::ctx_scratch(pt_ctx* c, int slot, size_t bytes, void** out) {
    if (!c || slot < 0 || slot >= kDnScratchSlots) return set_error(PT_E_ARG, "ctx_scratch: bad argument");
    if (int rc = ctx_ready(c)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_bytes(&c->d_dn[slot], &c->dn_bytes[slot], bytes, 1)) return rc;
    *out = c->d_dn[slot];
    return PT_OK;
}

void* pt::ctx_stream(pt_ctx* c) { return c && ctx_ready(c) == PT_OK ? (void*)c->stream : nullptr; }

pt::TemporalState* pt::ctx_temporal_state(pt_ctx* c) { return &c->temporal; }

// Quantise a device image of `rows` x W pixels into d_dst (synchronous).
int pt::rgb8_device(pt_ctx* c, const float* d_lin, int rows, int W, float gamma, int flip, uint8_t* d_dst) {
    if (int rc0 = ctx_ready(c)) return rc0;
    float thr[256];
    int32_t neg_mode = 0;
    const int rc = pt_rgb8_thresholds(gamma, thr, &neg_mode);
    if (rc) return rc;
    thr[255] = __builtin_inff();
    if (rows > 65535) return set_error(PT_E_ARG, "pt_rgb8: %d rows exceed the quantiser grid", rows);
    if (!c->d_thr) HIP_TRY(hipMalloc((void**)&c->d_thr, 256 * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(c->d_thr, thr, sizeof(thr), hipMemcpyHostToDevice, c->stream));
    if (rows > 0 && W > 0)
        hipLaunchKernelGGL(pt_rgb8_kernel, dim3((3 * W + kBlock - 1) / kBlock, rows), dim3(kBlock), 0, c->stream,
                           d_lin, d_dst, c->d_thr, rows, W, flip, neg_mode);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));  // thr lives on this stack frame
    return PT_OK;
}

extern "C" {

int pt_ctx_render_rgb8(pt_ctx* c, const pt_camera* cam, const pt_params* prm, float gamma, int flip, uint8_t* out,
                       int out_is_device, pt_stats* stats) {
    if (!c || !cam || !prm || !out) return set_error(PT_E_ARG, "pt_ctx_render_rgb8: NULL argument");
    PartShape shape;
    int rc;
    if ((rc = part_shape(cam, prm, -1, &shape))) return rc;  // depth: checked by render_range, in its order
    const int rows = shape.rows, W = shape.W;
    const size_t n = (size_t)shape.npix * 3;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure(&c->d_out, &c->out_floats, n))) return rc;
    c->prog_valid = false;
    if ((rc = render_range(c, cam, prm, 0, prm->spp > 0 ? prm->spp : 0, 0, c->d_out, 1, stats))) return rc;
    uint8_t* dst = out;
    if (!out_is_device) {
        if ((rc = ensure(&c->d_rgb8, &c->rgb8_bytes, n))) return rc;
        dst = c->d_rgb8;
    }
    if ((rc = rgb8_device(c, c->d_out, rows, W, gamma, flip, dst))) return rc;
    if (!out_is_device && n) HIP_TRY(hipMemcpy(out, dst, n, hipMemcpyDeviceToHost));
    return PT_OK;
}

// Test hook: the device quantiser on a host image (top row first, as pt_image_to_rgb8).
int pt_debug_rgb8(int device, const float* lin, int32_t W, int32_t H, float gamma, uint8_t* rgb8) {
    if (!lin || !rgb8 || W <= 0 || H <= 0) return set_error(PT_E_ARG, "pt_debug_rgb8: bad argument");
    pt_ctx* c = nullptr;
    int rc = pt_ctx_create(device, &c);
    if (rc) return rc;
    const size_t n = (size_t)W * H * 3;
    float* d_lin = nullptr;
    uint8_t* d_o = nullptr;
    hipError_t e = hipMalloc((void**)&d_lin, n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&d_o, n);
    if (e == hipSuccess) e = hipMemcpy(d_lin, lin, n * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = set_error(PT_E_HIP, "pt_debug_rgb8: %s", hipGetErrorString(e));
    if (!rc) rc = rgb8_device(c, d_lin, H, W, gamma, 1, d_o);
    if (!rc && hipMemcpy(rgb8, d_o, n, hipMemcpyDeviceToHost) != hipSuccess)
        rc = set_error(PT_E_HIP, "pt_debug_rgb8: copy failed");
    if (d_lin) (void)hipFree(d_lin);
    if (d_o) (void)hipFree(d_o);
    pt_ctx_destroy(c);
    return rc;
}

int pt_render_f32(const pt_scene* scene, const pt_camera* cam, const pt_params* params, float* out_rgb,
                  pt_stats* stats) {
    if (!params) return set_error(PT_E_ARG, "params is NULL");
    if (scene && scene->num_tris <= 0) return set_error(PT_E_EMPTY, "No triangles in scene.");
    pt_ctx* c = nullptr;
    int rc = pt_ctx_create(0, &c);
    if (rc) return rc;
    rc = pt_ctx_set_scene(c, scene);
    if (!rc) {
        pt_params p = *params;
        p.part_index = 0;
        p.part_count = 1;
        if (p.band_rows <= 0) p.band_rows = 1;
        rc = pt_ctx_render(c, cam, &p, out_rgb, 0, stats);
    }
    pt_ctx_destroy(c);
    return rc;
}

// Test hook: how the context renders its scene (pt_hip_debug.h).
int pt_debug_ctx_flags(const pt_ctx* c, int32_t out[5]) {
    if (!c || !out) return set_error(PT_E_ARG, "pt_debug_ctx_flags: NULL argument");
    out[0] = c->albedo_x2 ? 1 : 0;
    out[1] = c->has_specular ? 1 : 0;
    out[2] = c->rtc_requested ? 1 : 0;
    out[3] = c->meta.num_wide;
    out[4] = c->dark ? 1 : 0;
    return PT_OK;
}

// Test hook: the last-ray rule of the context's scene and its count in the last render (pt_hip_debug.h).
int pt_debug_ctx_emit_reject(const pt_ctx* c, int32_t* on, float box[6], uint64_t* early) {
    if (!c) return set_error(PT_E_ARG, "pt_debug_ctx_emit_reject: NULL argument");
    if (on) *on = c->emit.on ? 1 : 0;
    if (box)
        for (int a = 0; a < 3; a++) box[a] = c->emit.lo[a], box[3 + a] = c->emit.hi[a];
    if (early) *early = c->last_early;
    return PT_OK;
}

// Test hook (no device needed): the last-ray rule's emitter box of a scene (scene_emit_box).
int pt_debug_emit_box(const pt_scene* scene, float out[6]) {
    if (!out) return set_error(PT_E_ARG, "pt_debug_emit_box: NULL argument");
    PackedScene ps;
    const int rc = pack_scene(scene, ps);
    if (rc) return rc;
    const EmitBox e = scene_emit_box(ps, scene_dark(ps));
    for (int a = 0; a < 3; a++) out[a] = e.lo[a], out[3 + a] = e.hi[a];
    return e.on ? 1 : 0;
}

// Test hook (no device needed): emit_reject (pt_math.h) on n rays against n boxes.
int pt_debug_emit_reject(const float* box6, const float* org, const float* dir, int64_t n, uint8_t* out) {
    if (!box6 || !org || !dir || !out || n < 0) return set_error(PT_E_ARG, "pt_debug_emit_reject: bad argument");
    for (int64_t i = 0; i < n; i++) {
        const float *b = box6 + 6 * i, *o = org + 3 * i, *d = dir + 3 * i;
        out[i] = emit_reject(v3{b[0], b[1], b[2]}, v3{b[3], b[4], b[5]}, v3{o[0], o[1], o[2]}, v3{d[0], d[1], d[2]}) ? 1 : 0;
    }
    return PT_OK;
}

// Test hook (no device needed): emit_slab_reject (pt_math.h) on n rays against n boxes.
int pt_debug_emit_slab_reject(const float* box6, const float* org, const float* inv, int64_t n, uint8_t* out) {
    if (!box6 || !org || !inv || !out || n < 0) return set_error(PT_E_ARG, "pt_debug_emit_slab_reject: bad argument");
    for (int64_t i = 0; i < n; i++) {
        const float *b = box6 + 6 * i, *o = org + 3 * i, *v = inv + 3 * i;
        out[i] = emit_slab_reject(v3{b[0], b[1], b[2]}, v3{b[3], b[4], b[5]}, v3{o[0], o[1], o[2]}, v3{v[0], v[1], v[2]}) ? 1 : 0;
    }
    return PT_OK;
}

// Test hook: the one-verdict-per-ray policy's device functions (domain_once_probe) on n rays
// against one box, on the host (device < 0) or in one block on a device.
int pt_debug_domain_once(int device, const float* box6, const float* org, const float* dir, int64_t n, int unit,
                         uint8_t* out, float* inv3) {
    if (!box6 || !org || !dir || !out || !inv3 || n < 1 || n > (1 << 20))
        return set_error(PT_E_ARG, "pt_debug_domain_once: bad argument");
    if (device < 0) {
        const v3 elb{box6[0], box6[1], box6[2]}, ert{box6[3], box6[4], box6[5]};
        for (int64_t i = 0; i < n; i++) {
            const v3 o{org[3 * i], org[3 * i + 1], org[3 * i + 2]}, d{dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]};
            if (unit) domain_once_probe<true>(elb, ert, o, d, out + 6 * i, inv3 + 3 * i);
            else domain_once_probe<false>(elb, ert, o, d, out + 6 * i, inv3 + 3 * i);
        }
        return PT_OK;
    }
    HIP_TRY(hipSetDevice(device));
    const size_t fb = (size_t)n * 3 * sizeof(float);
    float* dbuf = nullptr;  // box6 | org | dir | inv3, then the flags
    uint8_t* dout = nullptr;
    HIP_TRY(hipMalloc((void**)&dbuf, 6 * sizeof(float) + 3 * fb));
    if (hipMalloc((void**)&dout, (size_t)n * 6) != hipSuccess) {
        (void)hipFree(dbuf);
        return set_error(PT_E_HIP, "hipMalloc failed");
    }
    float *dorg = dbuf + 6, *ddir = dorg + 3 * n, *dinv = ddir + 3 * n;
    hipError_t e = hipMemcpy(dbuf, box6, 6 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dorg, org, fb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ddir, dir, fb, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pt_domain_once_kernel, dim3(1), dim3(256), 0, 0, dbuf, dorg, ddir, (int)n, unit, dout, dinv);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * 6, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(inv3, dinv, fb, hipMemcpyDeviceToHost);
    (void)hipFree(dbuf);
    (void)hipFree(dout);
    if (e != hipSuccess) return set_error(PT_E_HIP, "pt_debug_domain_once: %s", hipGetErrorString(e));
    return PT_OK;
}

// Test hook (no device needed): hemisphere_dir's host form.
int pt_debug_hemisphere_dir(const uint32_t* lcg, const float* nrm, int64_t n, float* dir3) {
    if (!lcg || !nrm || !dir3 || n < 0) return set_error(PT_E_ARG, "pt_debug_hemisphere_dir: bad argument");
    for (int64_t i = 0; i < n; i++) {
        Lcg g{lcg[i]};
        const v3 r = hemisphere_dir(g, v3{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]});
        dir3[3 * i] = r.x;
        dir3[3 * i + 1] = r.y;
        dir3[3 * i + 2] = r.z;
    }
    return PT_OK;
}

// Test hook (no device needed): the loop control of the shared camera-ray stock (pt_raystack.h).
int pt_debug_ray_stack(int32_t which, int32_t count, int32_t n, int32_t reserve, int32_t flag) {
    switch (which) {
        case 0: return ray_stack_generate(count, n, reserve, flag != 0) ? 1 : 0;
        case 1: return ray_stack_filled(count, n);
        case 2: return ray_stack_dry(count, n) ? 1 : 0;
        case 3: return ray_stack_slot(count, n);
        case 4: return ray_stack_taken(count, n);
        case 5: return ray_stack_done(flag != 0, count, n != 0) ? 1 : 0;
    }
    return set_error(PT_E_ARG, "pt_debug_ray_stack: which = %d", which);
}

// Test hook (no device needed): the flat block's LDS layout (pt_flatlds.h), as plan_flat sizes it.
int pt_debug_flat_lds(int32_t num_tris, int32_t box_tab_bytes, int32_t pair_queue, int32_t rec_size, uint32_t out[10]) {
    if (!out || num_tris < 0 || box_tab_bytes < 0 || pair_queue < 0 || rec_size < 0)
        return set_error(PT_E_ARG, "pt_debug_flat_lds: bad argument");
    const FlatLds l = flat_lds_layout(3u * (unsigned)num_tris, 2u * (unsigned)num_tris, (unsigned)box_tab_bytes,
                                      (unsigned)pair_queue, (unsigned)rec_size);
    const uint32_t v[10] = {l.tris, l.mats, l.next_ray, l.best, l.next_at, l.boxtab, l.queues, l.rec_tri, l.rec_cos, l.bytes};
    memcpy(out, v, sizeof(v));
    return PT_OK;
}

// Test hook: the launch plan of the context's last render (pt_hip_debug.h).
int pt_debug_ctx_plan(const pt_ctx* c, int64_t out[24]) {
    if (!c || !out) return set_error(PT_E_ARG, "pt_debug_ctx_plan: NULL argument");
    memcpy(out, c->last_plan, sizeof(c->last_plan));
    return PT_OK;
}

// Test hook (no device needed): the dark-path gate (scene_dark) on a scene.
int pt_debug_scene_dark(const pt_scene* scene) {
    PackedScene ps;
    const int rc = pack_scene(scene, ps);
    if (rc) return rc;
    return scene_dark(ps) ? 1 : 0;
}

// GPU copies of the math primitives (test hook): which = 0 acosf, 1 sincosf, 2 BRDF.
int pt_debug_math(int device, int which, const float* in, int n, float* out) {
    if (!in || !out || n <= 0 || which < 0 || which > 2) return set_error(PT_E_ARG, "pt_debug_math: bad argument");
    HIP_TRY(hipSetDevice(device));
    const size_t in_n = (size_t)n * (which == 2 ? 9 : 1), out_n = (size_t)n * (which == 0 ? 1 : which == 1 ? 2 : 4);
    float *di = nullptr, *dout = nullptr;
    HIP_TRY(hipMalloc((void**)&di, in_n * sizeof(float)));
    if (hipMalloc((void**)&dout, out_n * sizeof(float)) != hipSuccess) {
        (void)hipFree(di);
        return set_error(PT_E_HIP, "hipMalloc failed");
    }
    hipError_t e = hipMemcpy(di, in, in_n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pt_math_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, which, di, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout, out_n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(di);
    (void)hipFree(dout);
    if (e != hipSuccess) return set_error(PT_E_HIP, "pt_debug_math: %s", hipGetErrorString(e));
    return PT_OK;
}

int pt_debug_sweep(int device, int which, uint32_t lo_bits, uint32_t hi_bits, uint64_t* mismatches,
                   uint32_t* first_bad) {
    if (!mismatches || !first_bad || which < 0 || which > 9 || hi_bits < lo_bits)
        return set_error(PT_E_ARG, "pt_debug_sweep: bad argument");
    HIP_TRY(hipSetDevice(device));
    unsigned long long* d_bad = nullptr;
    uint32_t* d_first = nullptr;
    HIP_TRY(hipMalloc((void**)&d_bad, sizeof(unsigned long long)));
    if (hipMalloc((void**)&d_first, sizeof(uint32_t)) != hipSuccess) {
        (void)hipFree(d_bad);
        return set_error(PT_E_HIP, "hipMalloc failed");
    }
    hipError_t e = hipMemset(d_bad, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d_first, 0xff, sizeof(uint32_t));
    if (e == hipSuccess) {
        const unsigned long long n = (unsigned long long)(hi_bits - lo_bits) + 1ull;
        hipLaunchKernelGGL(pt_sweep_kernel, dim3(8192), dim3(256), 0, 0, which, lo_bits, n, d_bad, d_first);
        e = hipGetLastError();
    }
    unsigned long long hb = 0;
    uint32_t hf = 0;
    if (e == hipSuccess) e = hipMemcpy(&hb, d_bad, sizeof(hb), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&hf, d_first, sizeof(hf), hipMemcpyDeviceToHost);
    (void)hipFree(d_bad);
    (void)hipFree(d_first);
    if (e != hipSuccess) return set_error(PT_E_HIP, "pt_debug_sweep: %s", hipGetErrorString(e));
    *mismatches = hb;
    *first_bad = hf;
    return PT_OK;
}

}  // extern "C"
