// pt_temporal.hip — the temporal reprojection on the device (gfx950). The
// arithmetic is pt_temporal.h's, shared with the host form (pt_image_temporal, pt_host.cpp); here
// are the kernel and the pt_ctx_* entry points.
//
//   pt_tp_kernel      one pixel per lane, a block 64 x 4 pixels with a wave per row (the direct
//                     denoise pass's shape): the current frame's planes load coalesced, and the
//                     four taps of neighbouring lanes fall in neighbouring pixels of the previous
//                     history for any camera move, so the gather is served by L1 / L2 without LDS.
//                     Both cameras arrive as kernel arguments with their per-call terms formed on
//                     the host (TpCam). A wave counts its reusing pixels by ballot and adds them
//                     with one atomic.
//
// pt_ctx_temporal needs no scene and touches none of the context's render state: its buffers are
// the context's scratch slots 3..6 (ctx_scratch, pt_internal.h).
#include <hip/hip_runtime.h>

#include <string.h>

#include <chrono>

#include "pt_internal.h"
#include "pt_temporal.h"

namespace pt {

namespace {

constexpr int kTpBlock = 256, kTpWave = 64;
constexpr int kTpW = 64, kTpH = 4;  // a block's pixels, one wave per row

template <bool kSample>
__global__ __launch_bounds__(kTpBlock) void pt_tp_kernel(int W, int H, int tiles_x, TpCam cur, TpCam old, TpFrame F,
                                                        TpHist prev, int has_prev, TpHist next, TpParams P,
                                                        unsigned long long* __restrict__ reused) {
    const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
    const int x = bx * kTpW + (int)(threadIdx.x % kTpW);
    const int y = by * kTpH + (int)(threadIdx.x / kTpW);
    bool reuse = false;
    if (x < W && y < H) reuse = tp_pixel<kSample>(W, H, x, y, cur, old, F, prev, has_prev != 0, next, P);
    const unsigned long long b = __ballot(reuse);
    if ((threadIdx.x & (kTpWave - 1)) == 0 && b) atomicAdd(reused, (unsigned long long)__popcll(b));
}

#define TP_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return set_error(PT_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct TpEvents {
    hipEvent_t e[2] = {};
    int n = 0;
    int make() {
        for (; n < 2; n++) TP_HIP(hipEventCreate(&e[n]));
        return PT_OK;
    }
    ~TpEvents() {
        for (int i = 0; i < n; i++) (void)hipEventDestroy(e[i]);
    }
};

constexpr size_t kTpHead = 256;  // slot 3 starts with the reuse counter; a host-pointer call's staging follows
// words of 4 bytes per pixel: a history's seven planes, and the current frame's inputs with a variance
constexpr size_t kTpHistWords = 3 + 3 + 3 + 1 + 3 + 3 + 1, kTpFrameWords = 3 + 3 + 3 + 1 + 1 + 3 + 3;

// A history's planes laid one after the other in a buffer of kTpHistWords * npix words.
TpHist tp_carve(void* base, size_t npix) {
    float* f = (float*)base;
    TpHist h;
    h.color = f;
    h.m2 = f + 3 * npix;
    h.var = f + 6 * npix;
    h.normal = f + 9 * npix;
    h.position = f + 12 * npix;
    h.hist = (int32_t*)(f + 15 * npix);
    h.cls = (int32_t*)(f + 16 * npix);
    return h;
}

}  // namespace

}  // namespace pt

using namespace pt;

extern "C" {

int pt_ctx_temporal(pt_ctx* c, int32_t W, int32_t H, const pt_camera* cam_cur, const pt_camera* cam_prev,
                    const float* color, const float* var, const pt_denoise_guides* g, const pt_temporal_history* prev,
                    const pt_temporal_history* next, const pt_temporal_params* prm, int is_device,
                    pt_temporal_stats* stats) {
    const auto t_start = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return set_error(PT_E_ARG, "pt_ctx_temporal: NULL context");
    TpParams P;
    if (int rc = temporal_check("pt_ctx_temporal", W, H, cam_cur, cam_prev, color, var, g, prev, next, prm, &P)) return rc;
    const size_t npix = (size_t)W * H;
    const size_t staging = is_device ? 0 : npix * sizeof(float) * (kTpFrameWords + 2 * kTpHistWords);
    void* p3 = nullptr;
    if (int rc = ctx_scratch(c, 3, kTpHead + staging, &p3)) return rc;
    hipStream_t st = (hipStream_t)ctx_stream(c);
    unsigned long long* d_count = (unsigned long long*)p3;

    TpFrame F{color, P.sample ? var : nullptr, g->normal, g->t, g->tri, g->emission, g->position};
    TpHist nx{next->color, next->m2, next->var, next->hist, next->normal, next->position, next->cls};
    TpHist pv{};
    if (prev) pv = TpHist{prev->color, prev->m2, prev->var, prev->hist, prev->normal, prev->position, prev->cls};
    if (!is_device) {
        float* at = (float*)((char*)p3 + kTpHead);
        bool ok = true;
        auto up = [&](const void* src, size_t width) -> float* {
            float* dst = at;
            at += width * npix;
            if (src && hipMemcpyAsync(dst, src, width * npix * sizeof(float), hipMemcpyHostToDevice, st) != hipSuccess) ok = false;
            return dst;
        };
        F.color = up(color, 3);
        F.var = up(P.sample ? var : nullptr, 3);
        if (!P.sample) F.var = nullptr;
        F.normal = up(g->normal, 3);
        F.t = up(g->t, 1);
        F.tri = (const int32_t*)up(g->tri, 1);
        F.emission = up(g->emission, 3);
        F.position = up(g->position, 3);
        TpHist dp = tp_carve(at, npix);
        at += kTpHistWords * npix;
        nx = tp_carve(at, npix);
        if (prev) {
            const hipMemcpyKind k = hipMemcpyHostToDevice;
            ok = ok && hipMemcpyAsync(dp.color, prev->color, 12 * npix, k, st) == hipSuccess &&
                 hipMemcpyAsync(dp.m2, prev->m2, 12 * npix, k, st) == hipSuccess &&
                 (!P.sample || hipMemcpyAsync(dp.var, prev->var, 12 * npix, k, st) == hipSuccess) &&
                 hipMemcpyAsync(dp.hist, prev->hist, 4 * npix, k, st) == hipSuccess &&
                 hipMemcpyAsync(dp.normal, prev->normal, 12 * npix, k, st) == hipSuccess &&
                 hipMemcpyAsync(dp.position, prev->position, 12 * npix, k, st) == hipSuccess &&
                 hipMemcpyAsync(dp.cls, prev->cls, 4 * npix, k, st) == hipSuccess;
            pv = dp;
        }
        if (!ok) return set_error(PT_E_HIP, "pt_ctx_temporal: upload failed");
    }

    TpEvents ev;
    if (int rc = ev.make()) return rc;
    TP_HIP(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
    const TpCam cur = tp_camera(*cam_cur), old = tp_camera(prev ? *cam_prev : *cam_cur);
    const int tiles_x = (W + kTpW - 1) / kTpW, tiles_y = (H + kTpH - 1) / kTpH;
    const dim3 grid((unsigned)((size_t)tiles_x * tiles_y));
    TP_HIP(hipEventRecord(ev.e[0], st));
    if (P.sample)
        hipLaunchKernelGGL(pt_tp_kernel<true>, grid, dim3(kTpBlock), 0, st, W, H, tiles_x, cur, old, F, pv, prev ? 1 : 0, nx, P,
                           d_count);
    else
        hipLaunchKernelGGL(pt_tp_kernel<false>, grid, dim3(kTpBlock), 0, st, W, H, tiles_x, cur, old, F, pv, prev ? 1 : 0, nx, P,
                           d_count);
    TP_HIP(hipGetLastError());
    TP_HIP(hipEventRecord(ev.e[1], st));
    unsigned long long count = 0;
    TP_HIP(hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, st));
    if (!is_device) {
        const hipMemcpyKind k = hipMemcpyDeviceToHost;
        TP_HIP(hipMemcpyAsync(next->color, nx.color, 12 * npix, k, st));
        TP_HIP(hipMemcpyAsync(next->m2, nx.m2, 12 * npix, k, st));
        TP_HIP(hipMemcpyAsync(next->var, nx.var, 12 * npix, k, st));
        TP_HIP(hipMemcpyAsync(next->hist, nx.hist, 4 * npix, k, st));
        TP_HIP(hipMemcpyAsync(next->normal, nx.normal, 12 * npix, k, st));
        TP_HIP(hipMemcpyAsync(next->position, nx.position, 12 * npix, k, st));
        TP_HIP(hipMemcpyAsync(next->cls, nx.cls, 4 * npix, k, st));
    }
    TP_HIP(hipStreamSynchronize(st));
    if (stats) {
        float ms = 0;
        TP_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        stats->kernel_ms = ms;
        stats->reused = (int64_t)count;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return PT_OK;
}

// The frame's steps; pt_ctx_render_temporal wraps them so that every error return drops the history.
static int render_temporal_frame(pt_ctx* c, const pt_camera* cam, const pt_params* prm, const pt_temporal_params* tprm,
                                 const pt_denoise_params* dprm, int reset, float* out, float* accumulated_out,
                                 int out_is_device, pt_render_temporal_stats* stats, TemporalState* T) {
    const auto t_start = std::chrono::steady_clock::now();
    if (prm->part_count > 1)
        return set_error(PT_E_ARG, "pt_ctx_render_temporal: part_count %d: the history needs the whole image on one device",
                         prm->part_count);
    const int32_t W = cam->res[0], H = cam->res[1];
    if (W <= 0 || H <= 0 || (int64_t)W * H > (1ll << 30))
        return set_error(PT_E_ARG, "pt_ctx_render_temporal: image of %d x %d pixels", W, H);
    if (prm->spp < 1) return set_error(PT_E_ARG, "pt_ctx_render_temporal: spp %d", prm->spp);
    const int mode = prm->spp >= 2 ? PT_TEMPORAL_VAR_SAMPLE : PT_TEMPORAL_VAR_TEMPORAL;
    pt_temporal_params tp = tprm ? *tprm : pt_temporal_params{0, 0.0f, 0.0f, 0};
    if (tp.variance_mode != 0 && tp.variance_mode != mode)
        return set_error(PT_E_ARG, "pt_ctx_render_temporal: variance_mode %d with spp %d", tp.variance_mode, prm->spp);
    tp.variance_mode = mode;
    {  // the accumulation's and the filter's own argument errors before anything is rendered
        const float dummy = 0.0f;
        float sink = 0.0f;
        int32_t isink = 0;
        const pt_denoise_guides gd{&dummy, &dummy, reinterpret_cast<const int32_t*>(&dummy), &dummy, &dummy};
        const pt_temporal_history hd{&sink, &sink, &sink, &isink, &sink, &sink, &isink};
        TpParams P;
        DnParams D;
        if (int rc = temporal_check("pt_ctx_render_temporal", W, H, cam, nullptr, &dummy, &dummy, &gd, nullptr, &hd, &tp, &P)) return rc;
        if (int rc = denoise_check("pt_ctx_render_temporal", W, H, &dummy, &dummy, &gd, dprm, &dummy, nullptr, &D)) return rc;
    }
    if (reset || T->cam.res[0] != W || T->cam.res[1] != H) T->valid = false;
    const size_t n = (size_t)W * H;
    // slot 6: S, Q (doubles); colour, normal, t, emission, ray, position, var, out (floats); tri (int32)
    void *p6 = nullptr, *ph[2] = {nullptr, nullptr};
    if (int rc = ctx_scratch(c, 6, n * (6 * sizeof(double) + 25 * sizeof(float) + sizeof(int32_t)), &p6)) return rc;
    for (int k = 0; k < 2; k++)
        if (int rc = ctx_scratch(c, 4 + k, n * kTpHistWords * sizeof(float), &ph[k])) return rc;
    hipStream_t st = (hipStream_t)ctx_stream(c);
    double* dS = (double*)p6;
    double* dQ = dS + 3 * n;
    float* d_color = (float*)(dQ + 3 * n);
    float* d_normal = d_color + 3 * n;
    float* d_t = d_normal + 3 * n;
    float* d_emit = d_t + n;
    float* d_ray = d_emit + 3 * n;
    float* d_pos = d_ray + 6 * n;
    float* d_var = d_pos + 3 * n;
    float* d_den = d_var + 3 * n;
    int32_t* d_tri = (int32_t*)(d_den + 3 * n);

    int runaway = PT_OK;
    const pt_moments mom{dS, dQ, nullptr};
    pt_stats rs;
    if (int rc = pt_ctx_render_moments(c, cam, prm, 0, prm->spp, d_color, &mom, 1, &rs)) {
        if (rc != PT_E_RUNAWAY) return rc;
        runaway = rc;
    }
    const pt_aov aov{d_t, d_tri, d_normal, nullptr, d_emit, d_ray};
    pt_query_stats qs;
    if (int rc = pt_ctx_render_aov(c, cam, prm, 0, &aov, 1, &qs)) return rc;
    TpEvents ev;
    if (int rc = ev.make()) return rc;
    TP_HIP(hipEventRecord(ev.e[0], st));
    if (int rc = dn_position_launch(st, d_ray, d_t, n, d_pos)) return rc;
    if (mode == PT_TEMPORAL_VAR_SAMPLE)
        if (int rc = pt_ctx_moments_variance(c, dS, dQ, (int64_t)n, prm->spp, nullptr, d_var, 1)) return rc;
    TP_HIP(hipEventRecord(ev.e[1], st));
    const pt_denoise_guides g{d_normal, d_t, d_tri, d_emit, d_pos};
    const bool had = T->valid;
    const TpHist hp = tp_carve(ph[T->slot], n), hn = tp_carve(ph[1 - T->slot], n);
    const pt_temporal_history prev{hp.color, hp.m2, hp.var, hp.hist, hp.normal, hp.position, hp.cls};
    const pt_temporal_history next{hn.color, hn.m2, hn.var, hn.hist, hn.normal, hn.position, hn.cls};
    pt_temporal_stats ts;
    if (int rc = pt_ctx_temporal(c, W, H, cam, had ? &T->cam : nullptr, d_color, mode == PT_TEMPORAL_VAR_SAMPLE ? d_var : nullptr,
                                 &g, had ? &prev : nullptr, &next, &tp, 1, &ts))
        return rc;
    float* dst = out_is_device ? out : d_den;
    pt_denoise_stats ds;
    if (int rc = pt_ctx_denoise(c, W, H, hn.color, hn.var, &g, dprm, dst, nullptr, 1, &ds)) return rc;
    const hipMemcpyKind kind = out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (!out_is_device) TP_HIP(hipMemcpyAsync(out, d_den, 3 * n * sizeof(float), kind, st));
    if (accumulated_out) TP_HIP(hipMemcpyAsync(accumulated_out, hn.color, 3 * n * sizeof(float), kind, st));
    TP_HIP(hipStreamSynchronize(st));
    T->slot = 1 - T->slot;
    T->cam = *cam;
    T->valid = true;
    if (stats) {
        float ms = 0;
        TP_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        stats->variance_ms = ms;
        stats->aov_ms = qs.kernel_ms;
        stats->render_ms = rs.total_ms;
        stats->rays = rs.rays;
        stats->had_history = had ? 1 : 0;
        stats->variance_mode = mode;
        stats->temporal = ts;
        stats->denoise = ds;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    if (runaway) return set_error(PT_E_RUNAWAY, "pt_ctx_render_temporal: specular rejection loops hit their bound during the render");
    return PT_OK;
}

int pt_ctx_render_temporal(pt_ctx* c, const pt_camera* cam, const pt_params* prm, const pt_temporal_params* tprm,
                           const pt_denoise_params* dprm, int reset, float* out, float* accumulated_out, int out_is_device,
                           pt_render_temporal_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c || !cam || !prm || !out) return set_error(PT_E_ARG, "pt_ctx_render_temporal: NULL argument");
    TemporalState* T = ctx_temporal_state(c);
    const int rc = render_temporal_frame(c, cam, prm, tprm, dprm, reset, out, accumulated_out, out_is_device, stats, T);
    if (rc) T->valid = false;
    return rc;
}

}  // extern "C"
