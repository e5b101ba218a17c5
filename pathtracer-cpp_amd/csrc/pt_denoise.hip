// pt_denoise.hip — the a-trous denoiser on the device (gfx950). The arithmetic is
// pt_denoise.h's, shared with the host form (pt_image_denoise, pt_host.cpp); here are the kernels
// and the pt_ctx_* entry points.
//
//   pt_dn_pack_kernel          guides, colour and variance -> 16-byte records (pt_denoise.h)
//   pt_dn_pass_kernel          one pass, direct form: one pixel per lane, lanes along x, every tap
//                              a coalesced 1 KiB wave load served by L1 / L2
//   pt_dn_pass_lds_kernel      the pass at stride 1, tiled form: a 32 x 16 tile and its halo of 2
//                              pixels staged in LDS, two pixels per lane
//   pt_dn_variance_kernel      the variance of the mean from the moments
//   pt_dn_position_kernel      o + d * t of the AOV's rays (pt_ctx_render_denoised)
//
// The filter needs no scene and touches none of the context's render state: its buffers are the
// context's scratch slots (ctx_scratch, pt_internal.h).
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>

#include "pt_denoise.h"
#include "pt_internal.h"

namespace pt {

namespace {

constexpr int kDnBlock = 256;
// direct form: a block covers 64 x 4 pixels, one wave per row
constexpr int kDnDirW = 64, kDnDirH = 4;
// tiled form: a block covers 32 x 16 pixels, a lane the pixels (tx, ty) and (tx, ty + 8)
constexpr int kDnTileW = 32, kDnTileH = 16;

// The tiled form exists at stride 1 only, where it is the default: measured on MI355X at 1024^2
// with a variance, 0.087 ms against 0.109 ms direct. At stride 2 (a 40 x 24 tile of records for
// 32 x 16 pixels, 61 KB of LDS) it was not faster, 0.110 ms against 0.107 ms, and was removed
// (profiles/denoise/forms_strides_1_2).
constexpr bool kDnLdsDefault = true;

__global__ __launch_bounds__(kDnBlock) void pt_dn_pack_kernel(size_t npix, const float* __restrict__ color,
                                                             const float* __restrict__ var,
                                                             const float* __restrict__ normal,
                                                             const float* __restrict__ t,
                                                             const int32_t* __restrict__ tri,
                                                             const float* __restrict__ emission,
                                                             const float* __restrict__ position, float sigma_z,
                                                             DnRec* __restrict__ nt, DnRec* __restrict__ xc,
                                                             DnRec* __restrict__ col, DnRec* __restrict__ vr) {
    const size_t i = (size_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (i < npix) dn_pack(i, color, var, normal, t, tri, emission, position, sigma_z, nt, xc, col, vr);
}

// Where a pass writes pixel i: the next ping-pong records, or (the last pass) the caller's images.
struct DnDst {
    DnRec* col;
    DnRec* var;
    float* out3;
    float* var3;
};

template <bool kVar>
__device__ __forceinline__ void dn_store(const DnDst& D, size_t i, const DnRec& c, const DnRec& v) {
    if (D.out3) {
        D.out3[3 * i] = c.x;
        D.out3[3 * i + 1] = c.y;
        D.out3[3 * i + 2] = c.z;
        if (kVar && D.var3) {
            D.var3[3 * i] = v.x;
            D.var3[3 * i + 1] = v.y;
            D.var3[3 * i + 2] = v.z;
        }
    } else {
        D.col[i] = c;
        if (kVar) D.var[i] = v;
    }
}

template <bool kVar>
__global__ __launch_bounds__(kDnBlock) void pt_dn_pass_kernel(DnPlanes src, int W, int H, int s, int tiles_x, DnParams P,
                                                             DnDst D) {
    const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
    const int x = bx * kDnDirW + (int)(threadIdx.x % kDnDirW);
    const int y = by * kDnDirH + (int)(threadIdx.x / kDnDirW);
    if (x >= W || y >= H) return;
    DnRec c, v;
    dn_pixel<kVar>(src, W, H, x, y, s, P, c, v);
    dn_store<kVar>(D, (size_t)y * W + x, c, v);
}

// The records of a tile and its halo in LDS: four planes of TW x TH records, rows of TW.
struct DnTile {
    const DnRec *nt_, *xc_, *col_, *var_;
    int x0, y0, TW;
    __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * TW + (x - x0); }
    __device__ __forceinline__ DnRec nt(int x, int y) const { return nt_[at(x, y)]; }
    __device__ __forceinline__ DnRec xc(int x, int y) const { return xc_[at(x, y)]; }
    __device__ __forceinline__ DnRec col(int x, int y) const { return col_[at(x, y)]; }
    __device__ __forceinline__ DnRec var(int x, int y) const { return var_[at(x, y)]; }
};

// the tile with its halo of 2 pixels (stride 1)
constexpr int kDnHalo = 2, kDnLdsW = kDnTileW + 2 * kDnHalo, kDnLdsH = kDnTileH + 2 * kDnHalo;
constexpr size_t dn_tile_bytes(bool var) { return (size_t)kDnLdsW * kDnLdsH * sizeof(DnRec) * (var ? 4 : 3); }

// Lanes of a row read consecutive 16-byte records, so every ds_read_b128 lane group covers 16
// distinct 16-byte slots of the 256-byte bank row whatever the row pitch: no bank conflicts.
template <bool kVar>
__global__ __launch_bounds__(kDnBlock) void pt_dn_pass_lds_kernel(DnPlanes src, int W, int H, int tiles_x, DnParams P,
                                                                 DnDst D) {
    extern __shared__ DnRec dn_lds[];
    constexpr int TW = kDnLdsW, TH = kDnLdsH, R = kDnHalo, N = TW * TH;
    const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
    const int x0 = bx * kDnTileW - R, y0 = by * kDnTileH - R;
    DnRec* l_nt = dn_lds;
    DnRec* l_xc = dn_lds + N;
    DnRec* l_col = dn_lds + 2 * N;
    DnRec* l_var = dn_lds + 3 * N;  // only with kVar (the launch sizes the LDS)
    for (int i = (int)threadIdx.x; i < N; i += kDnBlock) {
        const int gx = x0 + i % TW, gy = y0 + i / TW;
        const DnRec zero{0.0f, 0.0f, 0.0f, 0.0f};
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;  // a slot outside the image is never read
        l_nt[i] = in ? src.nt(gx, gy) : zero;
        l_xc[i] = in ? src.xc(gx, gy) : zero;
        l_col[i] = in ? src.col(gx, gy) : zero;
        if (kVar) l_var[i] = in ? src.var(gx, gy) : zero;
    }
    __syncthreads();
    const DnTile tile{l_nt, l_xc, l_col, l_var, x0, y0, TW};
    const int x = bx * kDnTileW + (int)(threadIdx.x % kDnTileW);
    if (x >= W) return;
#pragma unroll 1
    for (int r = 0; r < 2; r++) {
        const int y = by * kDnTileH + (int)(threadIdx.x / kDnTileW) + r * (kDnTileH / 2);
        if (y >= H) break;
        DnRec c, v;
        dn_pixel<kVar>(tile, W, H, x, y, 1, P, c, v);
        dn_store<kVar>(D, (size_t)y * W + x, c, v);
    }
}

__global__ __launch_bounds__(kDnBlock) void pt_dn_variance_kernel(const double* __restrict__ sum,
                                                                 const double* __restrict__ sumsq, size_t nval, int n,
                                                                 const int32_t* __restrict__ spp,
                                                                 float* __restrict__ var) {
    const size_t i = (size_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (i < nval) var[i] = dn_variance(sum[i], sumsq[i], spp ? spp[i / 3] : n);
}

// position = o + d * t per component of the AOV's rays (6 floats per pixel: o.xyz, d.xyz).
__global__ __launch_bounds__(kDnBlock) void pt_dn_position_kernel(const float* __restrict__ ray,
                                                                 const float* __restrict__ t, size_t npix,
                                                                 float* __restrict__ pos) {
    const size_t i = (size_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= npix) return;
    const float ti = t[i];
    for (int k = 0; k < 3; k++) {
        const float m = ray[6 * i + 3 + k] * ti;
        pos[3 * i + k] = ray[6 * i + k] + m;
    }
}

#define DN_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return set_error(PT_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct DnEvents {
    hipEvent_t e[kDnMaxPasses + 2] = {};
    int n = 0;
    int make(int count) {
        for (; n < count; n++) DN_HIP(hipEventCreate(&e[n]));
        return PT_OK;
    }
    ~DnEvents() {
        for (int i = 0; i < n; i++) (void)hipEventDestroy(e[i]);
    }
};

unsigned dn_blocks(size_t n) { return (unsigned)((n + kDnBlock - 1) / kDnBlock); }

// PT_DENOISE_LDS (test hook): 0 every pass direct, 1 stride 1 tiled; unset: the default.
bool dn_use_lds(int pass) {
    if (pass != 0) return false;
    if (const char* e = hook_env("PT_DENOISE_LDS"))
        if (*e) return atoi(e) != 0;
    return kDnLdsDefault;
}

template <bool kVar>
void dn_launch_pass(hipStream_t st, bool lds, int pass, const DnPlanes& src, int W, int H, const DnParams& P,
                    const DnDst& D) {
    if (lds) {
        const int tiles_x = (W + kDnTileW - 1) / kDnTileW, tiles_y = (H + kDnTileH - 1) / kDnTileH;
        const dim3 grid((unsigned)((size_t)tiles_x * tiles_y));
        hipLaunchKernelGGL(pt_dn_pass_lds_kernel<kVar>, grid, dim3(kDnBlock), dn_tile_bytes(kVar), st, src, W, H, tiles_x,
                           P, D);
    } else {
        const int tiles_x = (W + kDnDirW - 1) / kDnDirW, tiles_y = (H + kDnDirH - 1) / kDnDirH;
        hipLaunchKernelGGL(pt_dn_pass_kernel<kVar>, dim3((unsigned)((size_t)tiles_x * tiles_y)), dim3(kDnBlock), 0, st, src,
                           W, H, 1 << pass, tiles_x, P, D);
    }
}
static_assert(dn_tile_bytes(true) <= 65536, "the tiled form's LDS stays within the default dynamic limit");

}  // namespace

int dn_position_launch(void* stream, const float* ray, const float* t, size_t npix, float* pos) {
    hipLaunchKernelGGL(pt_dn_position_kernel, dim3(dn_blocks(npix)), dim3(kDnBlock), 0, (hipStream_t)stream, ray, t, npix,
                       pos);
    DN_HIP(hipGetLastError());
    return PT_OK;
}

}  // namespace pt

using namespace pt;

extern "C" {

int pt_ctx_moments_variance(pt_ctx* c, const double* sum, const double* sumsq, int64_t npix, int32_t n,
                            const int32_t* spp, float* var_out, int is_device) {
    if (!c) return set_error(PT_E_ARG, "pt_ctx_moments_variance: NULL context");
    if (npix < 0 || npix > (1ll << 30) || (npix > 0 && (!sum || !sumsq || !var_out)))
        return set_error(PT_E_ARG, "pt_ctx_moments_variance: bad arrays");
    if (npix == 0) return PT_OK;
    const size_t nval = 3 * (size_t)npix;
    void* p = nullptr;
    // a host-pointer call stages S, Q, var and spp in slot 1; a device-pointer call only selects the device
    if (int rc = ctx_scratch(c, 1, is_device ? 0 : nval * (2 * sizeof(double) + sizeof(float)) + (size_t)npix * sizeof(int32_t), &p))
        return rc;
    hipStream_t st = (hipStream_t)ctx_stream(c);
    const double *dS = sum, *dQ = sumsq;
    const int32_t* dn = spp;
    float* dv = var_out;
    if (!is_device) {
        double* b = (double*)p;
        float* v = (float*)(b + 2 * nval);
        int32_t* sp = (int32_t*)(v + nval);
        DN_HIP(hipMemcpyAsync(b, sum, nval * sizeof(double), hipMemcpyHostToDevice, st));
        DN_HIP(hipMemcpyAsync(b + nval, sumsq, nval * sizeof(double), hipMemcpyHostToDevice, st));
        if (spp) DN_HIP(hipMemcpyAsync(sp, spp, (size_t)npix * sizeof(int32_t), hipMemcpyHostToDevice, st));
        dS = b;
        dQ = b + nval;
        dn = spp ? sp : nullptr;
        dv = v;
    }
    hipLaunchKernelGGL(pt_dn_variance_kernel, dim3(dn_blocks(nval)), dim3(kDnBlock), 0, st, dS, dQ, nval, (int)n, dn, dv);
    DN_HIP(hipGetLastError());
    if (!is_device) DN_HIP(hipMemcpyAsync(var_out, dv, nval * sizeof(float), hipMemcpyDeviceToHost, st));
    DN_HIP(hipStreamSynchronize(st));
    return PT_OK;
}

int pt_ctx_denoise(pt_ctx* c, int32_t W, int32_t H, const float* color, const float* var, const pt_denoise_guides* g,
                   const pt_denoise_params* prm, float* out, float* var_out, int is_device, pt_denoise_stats* stats) {
    const auto t_start = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return set_error(PT_E_ARG, "pt_ctx_denoise: NULL context");
    DnParams P;
    if (int rc = denoise_check("pt_ctx_denoise", W, H, color, var, g, prm, out, var_out, &P)) return rc;
    const size_t npix = (size_t)W * H;
    const bool has_var = var != nullptr;
    void* p0 = nullptr;
    if (int rc = ctx_scratch(c, 0, npix * sizeof(DnRec) * (has_var ? 6 : 4), &p0)) return rc;
    hipStream_t st = (hipStream_t)ctx_stream(c);
    DnRec* nt = (DnRec*)p0;
    DnRec* xc = nt + npix;
    DnRec* col[2] = {xc + npix, xc + 2 * npix};
    DnRec* vr[2] = {has_var ? xc + 3 * npix : nullptr, has_var ? xc + 4 * npix : nullptr};

    const float *d_color = color, *d_var = var;
    pt_denoise_guides dg = *g;
    float *d_out = out, *d_var_out = var_out;
    if (!is_device) {
        // staged one after the other in slot 1: colour, var, normal, t, tri, emission, position; then out, var_out
        const size_t floats = npix * (size_t)(3 + (has_var ? 3 : 0) + 3 + 1 + 1 + 3 + 3 + 3 + (var_out ? 3 : 0));
        void* p1 = nullptr;
        if (int rc = ctx_scratch(c, 1, floats * sizeof(float), &p1)) return rc;
        float* at = (float*)p1;
        auto up = [&](const void* src, size_t width) -> float* {
            float* dst = at;
            at += width * npix;
            return hipMemcpyAsync(dst, src, width * npix * sizeof(float), hipMemcpyHostToDevice, st) == hipSuccess ? dst
                                                                                                                  : nullptr;
        };
        d_color = up(color, 3);
        if (has_var) d_var = up(var, 3);
        dg.normal = up(g->normal, 3);
        dg.t = up(g->t, 1);
        dg.tri = (const int32_t*)up(g->tri, 1);
        dg.emission = up(g->emission, 3);
        dg.position = up(g->position, 3);
        if (!d_color || (has_var && !d_var) || !dg.normal || !dg.t || !dg.tri || !dg.emission || !dg.position)
            return set_error(PT_E_HIP, "pt_ctx_denoise: upload failed");
        d_out = at;
        at += 3 * npix;
        d_var_out = var_out ? at : nullptr;
    }

    DnEvents ev;
    if (int rc = ev.make(P.passes + 2)) return rc;
    DN_HIP(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(pt_dn_pack_kernel, dim3(dn_blocks(npix)), dim3(kDnBlock), 0, st, npix, d_color, d_var, dg.normal, dg.t,
                       dg.tri, dg.emission, dg.position, P.sigma_z, nt, xc, col[0], vr[0]);
    DN_HIP(hipGetLastError());
    DN_HIP(hipEventRecord(ev.e[1], st));
    int form[kDnMaxPasses] = {};
    for (int pass = 0; pass < P.passes; pass++) {
        const int from = pass & 1;
        const bool last = pass == P.passes - 1;
        const bool lds = dn_use_lds(pass);
        const DnPlanes src{nt, xc, col[from], vr[from], W};
        const DnDst D{col[1 - from], vr[1 - from], last ? d_out : nullptr, last ? d_var_out : nullptr};
        if (has_var)
            dn_launch_pass<true>(st, lds, pass, src, W, H, P, D);
        else
            dn_launch_pass<false>(st, lds, pass, src, W, H, P, D);
        DN_HIP(hipGetLastError());
        DN_HIP(hipEventRecord(ev.e[2 + pass], st));
        form[pass] = lds ? PT_DENOISE_LDS : PT_DENOISE_DIRECT;
    }
    if (!is_device) {
        DN_HIP(hipMemcpyAsync(out, d_out, 3 * npix * sizeof(float), hipMemcpyDeviceToHost, st));
        if (var_out) DN_HIP(hipMemcpyAsync(var_out, d_var_out, 3 * npix * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    DN_HIP(hipStreamSynchronize(st));
    if (stats) {
        float ms = 0;
        DN_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        stats->pack_ms = ms;
        stats->kernel_ms = ms;
        for (int pass = 0; pass < P.passes; pass++) {
            DN_HIP(hipEventElapsedTime(&ms, ev.e[1 + pass], ev.e[2 + pass]));
            stats->pass_ms[pass] = ms;
            stats->kernel_ms += ms;
            stats->form[pass] = form[pass];
        }
        stats->passes = P.passes;
        stats->launches = P.passes + 1;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return PT_OK;
}

int pt_ctx_render_denoised(pt_ctx* c, const pt_camera* cam, const pt_params* prm, const pt_adaptive* ad,
                           const pt_denoise_params* dprm, float* out, float* noisy_out, int32_t* spp_out,
                           int out_is_device, pt_adaptive_stats* render_stats, pt_denoised_stats* stats) {
    const auto t_start = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c || !cam || !prm || !ad || !out) return set_error(PT_E_ARG, "pt_ctx_render_denoised: NULL argument");
    if (prm->part_count > 1)
        return set_error(PT_E_ARG, "pt_ctx_render_denoised: part_count %d: the filter needs the whole image on one device",
                         prm->part_count);
    const int32_t W = cam->res[0], H = cam->res[1];
    if (W <= 0 || H <= 0 || (int64_t)W * H > (1ll << 30))
        return set_error(PT_E_ARG, "pt_ctx_render_denoised: image of %d x %d pixels", W, H);
    {  // the filter's own argument errors before anything is rendered
        DnParams P;
        const float dummy = 0.0f;
        const pt_denoise_guides gd{&dummy, &dummy, reinterpret_cast<const int32_t*>(&dummy), &dummy, &dummy};
        if (int rc = denoise_check("pt_ctx_render_denoised", W, H, &dummy, &dummy, &gd, dprm, &dummy, nullptr, &P)) return rc;
    }
    const size_t n = (size_t)W * H;
    // slot 2: S, Q (doubles); noisy, normal, t, emission, ray, position, var, out (floats); tri, spp (int32)
    void* p2 = nullptr;
    if (int rc = ctx_scratch(c, 2, n * (6 * sizeof(double) + 25 * sizeof(float) + 2 * sizeof(int32_t)), &p2)) return rc;
    hipStream_t st = (hipStream_t)ctx_stream(c);
    double* dS = (double*)p2;
    double* dQ = dS + 3 * n;
    float* d_noisy = (float*)(dQ + 3 * n);
    float* d_normal = d_noisy + 3 * n;
    float* d_t = d_normal + 3 * n;
    float* d_emit = d_t + n;
    float* d_ray = d_emit + 3 * n;
    float* d_pos = d_ray + 6 * n;
    float* d_var = d_pos + 3 * n;
    float* d_den = d_var + 3 * n;
    int32_t* d_tri = (int32_t*)(d_den + 3 * n);
    int32_t* d_spp = d_tri + n;

    int runaway = PT_OK;
    const pt_moments mom{dS, dQ, nullptr};
    if (int rc = pt_ctx_render_adaptive(c, cam, prm, ad, d_noisy, &mom, d_spp, 1, render_stats)) {
        if (rc != PT_E_RUNAWAY) return rc;
        runaway = rc;
    }
    const pt_aov aov{d_t, d_tri, d_normal, nullptr, d_emit, d_ray};
    pt_query_stats qs;
    if (int rc = pt_ctx_render_aov(c, cam, prm, 0, &aov, 1, &qs)) return rc;
    DnEvents ev;
    if (int rc = ev.make(2)) return rc;
    DN_HIP(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(pt_dn_position_kernel, dim3(dn_blocks(n)), dim3(kDnBlock), 0, st, d_ray, d_t, n, d_pos);
    DN_HIP(hipGetLastError());
    if (int rc = pt_ctx_moments_variance(c, dS, dQ, (int64_t)n, 0, d_spp, d_var, 1)) return rc;
    DN_HIP(hipEventRecord(ev.e[1], st));
    const pt_denoise_guides g{d_normal, d_t, d_tri, d_emit, d_pos};
    float* dst = out_is_device ? out : d_den;
    pt_denoise_stats ds;
    if (int rc = pt_ctx_denoise(c, W, H, d_noisy, d_var, &g, dprm, dst, nullptr, 1, &ds)) return rc;
    const hipMemcpyKind kind = out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (!out_is_device) DN_HIP(hipMemcpyAsync(out, d_den, 3 * n * sizeof(float), kind, st));
    if (noisy_out) DN_HIP(hipMemcpyAsync(noisy_out, d_noisy, 3 * n * sizeof(float), kind, st));
    if (spp_out) DN_HIP(hipMemcpyAsync(spp_out, d_spp, n * sizeof(int32_t), kind, st));
    DN_HIP(hipStreamSynchronize(st));
    if (stats) {
        float ms = 0;
        DN_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        stats->variance_ms = ms;
        stats->aov_ms = qs.kernel_ms;
        stats->denoise = ds;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    if (runaway) return set_error(PT_E_RUNAWAY, "pt_ctx_render_denoised: specular rejection loops hit their bound during the render");
    return PT_OK;
}

}  // extern "C"
