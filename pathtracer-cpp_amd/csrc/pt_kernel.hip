// pt_kernel.hip — the gfx950 kernels of libpt_hip.so and its device context.
//
//   pt_trace_kernel<kLds, kFlat>  generic megakernel (device code in pt_trace.h)
//   pt_trace_flat_rtc             the flat-path megakernel specialised per scene through
//                                 hipRTC (leaf-box planes as constants; shared planes and
//                                 boxes fold), compiled in the background from
//                                 pt_ctx_set_scene on (rtc_job)
//   pt_accumulate_kernel          in-order per-pixel accumulation + /spp
//   pt_math_kernel                device copies of the math primitives (test hook)
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <errno.h>
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
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <atomic>
#include <fstream>
#include <fcntl.h>
#include <link.h>
#include <signal.h>
#include <spawn.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

extern char** environ;

#include "pt_hip_debug.h"
#include "pt_internal.h"
#include "pt_sha256.h"
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
template <bool kLdsScene, bool kFlat, int kWide = 0, int kPF = kWideByte>
__global__ __launch_bounds__(kBlock, kPF == kWideF32 ? 5 : kWide == 8 ? PT_WIDE8_WAVES : kWide == 4 ? PT_WIDE4_WAVES : PT_WAVES)
void pt_trace_kernel(TraceArgs A) {
    if constexpr (kWide > 0)
        trace_body_wide<kWide, kPF, kLdsScene>(A);
    else if constexpr (kFlat)
        trace_body_flat<TableBoxMask>(A);
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
// (image.h:37-40) on the last batch; output interleaved RGB rows of this part.
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
    if (flags) {
        // a flagged slab (TraceArgs::flags): only the records of paths that did not end dark
        slab_sum<true>(radiance, flags, flags_pm, s_count, (uint32_t)q, (uint32_t)npix, x, y, z);
    } else {
        // 8 samples' loads in flight per step, added in sample order: a part of few pixels
        // (one rank's rows at 8 GPUs: 131k threads) is latency-bound with one sample per step
        int sl = 0;
        for (; sl + 8 <= s_count; sl += 8) {
            float3 v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = slab_at(radiance, (size_t)(sl + j), (uint32_t)q, (uint32_t)npix);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                x += v[j].x;
                y += v[j].y;
                z += v[j].z;
            }
        }
        for (; sl < s_count; sl++) {
            const float3 v = slab_at(radiance, (size_t)sl, (uint32_t)q, (uint32_t)npix);
            x += v.x;
            y += v.y;
            z += v.z;
        }
    }
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

// A hipRTC compile's result: the code object, or why there is none.
struct RtcCode {
    std::vector<char> code;
    std::string status;
    std::string disk_key;  // set when the code object was read from the on-disk cache
};
typedef std::shared_future<std::shared_ptr<const RtcCode>> RtcFuture;

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
    PackedScene meta;
    bool have_scene = false;
    bool has_specular = false;  // the scene holds a SPECULAR material
    bool albedo_x2 = false;     // the scene kernel unwinds with pre-doubled albedo (albedo_x2_ok)
    bool dark = false;          // every bounce material is dark (scene_dark): finish_path's skip
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
    unsigned long long* d_tctr = nullptr;    // work head, ray and runaway counters of a call (4 x u64)
    // progressive rendering: d_accum holds the running sum of prog_spp samples
    bool prog_valid = false;
    int prog_spp = 0;
    pt_camera prog_cam{};
    pt_params prog_prm{};
    hipFunction_t rtc_flat = nullptr;        // scene-specialised flat kernel (hipRTC), if built
    std::string rtc_status;                  // why there is no rtc_flat ("" when there is)
    std::string rtc_src;                     // its source while the compile is pending
    RtcFuture rtc_job;                       // its pending compile (valid() until taken)
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

int ensure(float** p, size_t* cap, size_t n) {
    if (*cap >= n && *p) return PT_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(float)));
    *cap = n;
    return PT_OK;
}

// Magic numbers of FastDiv for divisor d >= 1 (Granlund & Montgomery 1994, Fig. 4.1):
// l = ceil(log2 d), m = floor(2^32 (2^l - d) / d) + 1, q = (t + ((n - t) >> 1)) >> (l - 1).
FastDiv make_fastdiv(uint32_t d) {
    uint32_t l = 0;
    while (l < 32 && (1ull << l) < d) l++;
    FastDiv f;
    f.d = d;
    f.m = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    f.sh1 = l > 0 ? 1u : 0u;
    f.sh2 = l > 0 ? l - 1 : 0u;
    return f;
}

size_t lds_scene_budget() {
    const char* e = hook_env("PT_LDS_SCENE_BYTES");
    if (e && *e) return (size_t)strtoull(e, nullptr, 0);
    return 32 * 1024;
}

// Live contexts per device: the radiance-slab budget is shared among them (several
// contexts on one device — pt_render_*_devices with a device listed twice, or long-lived
// Renderer objects — must not each size their slab from the same free memory).
std::mutex g_dev_mu;
std::map<int, int> g_dev_contexts;

size_t batch_bytes_budget(int device, bool compile_pending) {
    const char* e = hook_env("PT_BATCH_BYTES");
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

// ---------------------------------------------------------------- hipRTC specialisation
// Sources of pt_trace.h, pt_math.h and pt_hip.h, embedded at build time (build/pt_rtc_blob.cpp).
extern "C" const char* pt_rtc_src_trace;
extern "C" const char* pt_rtc_src_math;
extern "C" const char* pt_rtc_src_hip;

std::string hexf(float v) {
    char b[64];
    snprintf(b, sizeof(b), "%af", (double)v);
    return b;
}

// Box-level pairs (PT_BOX_PAIRS, the hipRTC flat kernel): when every leaf holds one triangle
// (leaf k = triangle rank k) and no distinct leaf box bounds more than two leaves, the box
// mask carries one bit per DISTINCT box (Cornell: 20 for 32 leaves) and a pair (lane, box)
// tests the box's one or two triangles. Returns the number of distinct boxes in that case
// (the LDS table the kernel reads: one uint16 (rank0 | rank1 << 8, 0xff = none) per box),
// else 0. Box u is numbered by its first leaf, as in flat_mask_source.
// Off unless PT_BOX_PAIRS=1 (test hook): measured 2.2% slower on Cornell, 1.6% on modified
// Cornell r=0.3 and Cornell depth 8 (profiles/r05_ab/box_pairs) — the pair rounds' second
// triangle test and its divergence cost more than the 12 fewer mask bits save.
int flat_box_pairs(const std::vector<f4>& leaves, int n, std::vector<uint16_t>* tab = nullptr) {
    const char* e = hook_env("PT_BOX_PAIRS");
    if (!e || *e != '1') return 0;
    std::map<std::vector<uint32_t>, int> box_id;
    std::vector<std::vector<int>> box_leaves;
    for (int k = 0; k < n; k++) {
        const f4 a = leaves[2 * k], b = leaves[2 * k + 1];
        if (__builtin_bit_cast(int, b.z) != k || __builtin_bit_cast(int, b.w) != k) return 0;  // not one triangle per leaf
        const std::vector<uint32_t> key = {f2u(a.x), f2u(a.y), f2u(a.z), f2u(a.w), f2u(b.x), f2u(b.y)};
        auto it = box_id.find(key);
        if (it == box_id.end()) {
            it = box_id.emplace(key, (int)box_leaves.size()).first;
            box_leaves.emplace_back();
        }
        box_leaves[it->second].push_back(k);
    }
    for (const auto& l : box_leaves)
        if (l.size() > 2 || l.back() > 254) return 0;
    if (tab) {
        tab->clear();
        for (const auto& l : box_leaves) tab->push_back((uint16_t)(l[0] | ((l.size() > 1 ? l[1] : 0xff) << 8)));
    }
    return (int)box_leaves.size();
}

// Whether leaf k of the flat list holds exactly triangle rank k (every BVH::build tree).
bool leaves_single(const std::vector<f4>& leaves, int n) {
    for (int k = 0; k < n; k++)
        if (__builtin_bit_cast(int, leaves[2 * k + 1].z) != k || __builtin_bit_cast(int, leaves[2 * k + 1].w) != k)
            return false;
    return true;
}

// The flat path's leaf-box test for one scene as straight-line code: each distinct box
// plane (c - o) * inv is computed once, boxes shared by several leaves are tested once,
// and a flat axis (lb == rt) needs no min/max. Same IEEE operations as slab_hit_finite.
std::string flat_mask_source(const std::vector<f4>& leaves, int n, bool specular, bool tri_fast, bool albedo_x2,
                             bool dark) {
    std::vector<std::map<uint32_t, int>> planes(3);
    auto plane = [&](int ax, float c) {
        auto it = planes[ax].find(f2u(c));
        if (it != planes[ax].end()) return it->second;
        const int id = (int)planes[ax].size();
        planes[ax][f2u(c)] = id;
        return id;
    };
    std::string body;
    std::map<std::vector<uint32_t>, int> box_id;
    std::vector<unsigned long long> box_bits;
    struct BoxExpr {
        std::string lo[3], hi[3];
    };
    std::vector<BoxExpr> boxes;
    for (int k = 0; k < n; k++) {
        const f4 a = leaves[2 * k], b = leaves[2 * k + 1];
        const float lb[3] = {a.x, a.y, a.z}, rt[3] = {a.w, b.x, b.y};
        std::vector<uint32_t> key = {f2u(lb[0]), f2u(lb[1]), f2u(lb[2]), f2u(rt[0]), f2u(rt[1]), f2u(rt[2])};
        auto it = box_id.find(key);
        if (it != box_id.end()) {
            box_bits[it->second] |= 1ull << k;
            continue;
        }
        const int id = (int)box_bits.size();
        box_id[key] = id;
        box_bits.push_back(1ull << k);
        BoxExpr e;
        const char ax_name[3] = {'x', 'y', 'z'};
        for (int ax = 0; ax < 3; ax++) {
            const std::string p1 = std::string("t") + ax_name[ax] + std::to_string(plane(ax, lb[ax]));
            const std::string p2 = std::string("t") + ax_name[ax] + std::to_string(plane(ax, rt[ax]));
            if (p1 == p2) {
                e.lo[ax] = e.hi[ax] = p1;
            } else {
                e.lo[ax] = "__builtin_fminf(" + p1 + ", " + p2 + ")";
                e.hi[ax] = "__builtin_fmaxf(" + p1 + ", " + p2 + ")";
            }
        }
        boxes.push_back(e);
    }
    // tmin = max(lo_x, lo_y, lo_z, 0): the clamp to 0 is applied to one axis term and that
    // clamped term is computed once for every box that shares it (PT_SHARED_CLAMP; the same
    // maximum: max is associative and commutative on non-NaN values, and which zero a tie
    // returns does not change the comparison), instead of one max(., 0) per box.
    std::map<std::string, int> lo_uses;
    for (const BoxExpr& e : boxes)
        for (int ax = 0; ax < 3; ax++) lo_uses[e.lo[ax]]++;
    std::map<std::string, std::string> clamp_name;
    std::string clamps, tests, tests_plain, tests_sign;
    for (size_t id = 0; id < boxes.size(); id++) {
        const BoxExpr& e = boxes[id];
        int cax = 0;
        for (int ax = 1; ax < 3; ax++)
            if (lo_uses[e.lo[ax]] > lo_uses[e.lo[cax]]) cax = ax;
        auto cn = clamp_name.find(e.lo[cax]);
        if (cn == clamp_name.end()) {
            const std::string nm = "c" + std::to_string(clamp_name.size());
            clamps += "        const float " + nm + " = __builtin_fmaxf(" + e.lo[cax] + ", 0.0f);\n";
            cn = clamp_name.emplace(e.lo[cax], nm).first;
        }
        const int a1 = cax == 0 ? 1 : 0, a2 = cax == 2 ? 1 : 2;
        const std::string tmax = "__builtin_fminf(__builtin_fminf(" + e.hi[0] + ", " + e.hi[1] + "), " + e.hi[2] + ")";
        tests += "        const bool b" + std::to_string(id) + " = __builtin_fmaxf(__builtin_fmaxf(" + e.lo[a1] + ", " +
                 e.lo[a2] + "), " + cn->second + ") <= " + tmax + ";\n";
        tests_plain += "        const bool b" + std::to_string(id) + " = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(" +
                       e.lo[0] + ", " + e.lo[1] + "), " + e.lo[2] + "), 0.0f) <= " + tmax + ";\n";
        // sign-bit form (PT_SIGN_MASK): tmax + 0 turns a -0 exit value (origin on a plane,
        // 1 / d < 0) into +0, which the comparison above treats as equal to 0
        tests_sign += "        const uint32_t f" + std::to_string(id) + " = box_fail_bits(__builtin_fmaxf(__builtin_fmaxf(" +
                      e.lo[0] + ", " + e.lo[1] + "), " + e.lo[2] + "), " + tmax + " + 0.0f);\n";
    }
    tests = "#if KSIGN\n" + tests_sign + "#elif PT_SHARED_CLAMP\n" + clamps + tests + "#else\n" + tests_plain + "#endif\n";
    const char ax_name[3] = {'x', 'y', 'z'};
    // Plane values two at a time (v_pk_add_f32 + v_pk_mul_f32: the same two IEEE
    // operations per value, half the instructions); PT_PK_PLANES=0 emits scalar code.
    body += "#if PT_PK_PLANES\n";
    for (int ax = 0; ax < 3; ax++) {
        const std::string comp(1, ax_name[ax]);
        std::vector<std::pair<uint32_t, int>> ps(planes[ax].begin(), planes[ax].end());
        if (ps.empty()) continue;
        body += "        const f2v o" + comp + "2 = {o." + comp + ", o." + comp + "}, i" + comp + "2 = {inv." + comp +
                ", inv." + comp + "};\n";
        for (size_t i = 0; i < ps.size(); i += 2) {
            const auto& a = ps[i];
            const auto& b = ps[i + 1 < ps.size() ? i + 1 : i];
            const std::string pv = "p" + comp + std::to_string(i);
            body += "        const f2v " + pv + " = (f2v{" + hexf(u2f(a.first)) + ", " + hexf(u2f(b.first)) + "} - o" +
                    comp + "2) * i" + comp + "2;\n";
            body += "        const float t" + comp + std::to_string(a.second) + " = " + pv + ".x;\n";
            if (i + 1 < ps.size()) body += "        const float t" + comp + std::to_string(b.second) + " = " + pv + ".y;\n";
        }
    }
    body += "#else\n";
    for (int ax = 0; ax < 3; ax++)
        for (const auto& kv : planes[ax]) {
            const std::string comp(1, ax_name[ax]);
            body += "        const float t" + comp + std::to_string(kv.second) + " = (" + hexf(u2f(kv.first)) +
                    " - o." + comp + ") * inv." + comp + ";\n";
        }
    body += "#endif\n";
    // Leaf bits shifted in from the top leaf down, m = 2m + b: one add-with-carry per
    // leaf with the box test's lane mask as the carry, no constants held in registers.
    // PT_MULTI_LEAF_OR: a box holding several leaves (the two triangles of a quad) sets all
    // their bits with one select + or after the chain, whose steps for those leaves are
    // plain doublings (v_add_u32, which dual-issues) instead of one carry add (main VALU
    // port only) per leaf.
    std::vector<int> leaf_box(n, -1);
    for (size_t i = 0; i < box_bits.size(); i++)
        for (int k = 0; k < n; k++)
            if (box_bits[i] >> k & 1) leaf_box[k] = (int)i;
    auto multi = [&](int k) { return __builtin_popcountll(box_bits[leaf_box[k]]) > 1; };
    std::string acc = "        uint32_t lo = 0, hi = 0;\n#if KSIGN\n";
    for (int k = n - 1; k >= 0; k--) {  // fail bits shifted in, then inverted
        const char* w = k >= 32 ? "hi" : "lo";
        acc += std::string("        ") + w + " = shl1_add_sign(" + w + ", f" + std::to_string(leaf_box[k]) + ");\n";
    }
    acc += "        lo = ~lo" + std::string(n < 32 ? " & " + std::to_string((1u << n) - 1u) + "u" : "") + ";\n";
    if (n > 32) acc += "        hi = ~hi" + std::string(n < 64 ? " & " + std::to_string((uint32_t)((1ull << (n - 32)) - 1u)) + "u" : "") + ";\n";
    acc += "#else\n";
    for (int k = n - 1; k >= 0; k--) {
        const char* w = k >= 32 ? "hi" : "lo";
        const std::string bit = std::string("#if PT_ADDC_MASK\n        ") + w + " = shl1_add_bit(" + w +
                                ", __builtin_amdgcn_ballot_w64(b" + std::to_string(leaf_box[k]) + "));\n#else\n        " + w +
                                " = " + w + " + " + w + " + (b" + std::to_string(leaf_box[k]) + " ? 1u : 0u);\n#endif\n";
        if (multi(k))
            acc += std::string("#if PT_MULTI_LEAF_OR\n        ") + w + " = dbl_u32(" + w + ");\n#else\n" + bit + "#endif\n";
        else
            acc += bit;
    }
    acc += "#if PT_MULTI_LEAF_OR\n";
    for (size_t i = 0; i < box_bits.size(); i++) {
        const unsigned long long m = box_bits[i];
        if (__builtin_popcountll(m) < 2) continue;
        const std::string bal = "__builtin_amdgcn_ballot_w64(b" + std::to_string(i) + ")";
        if ((uint32_t)m)
            acc += "        lo = or_if_bit(lo, " + std::to_string((uint32_t)m) + "u, " + bal + ");\n";
        if ((uint32_t)(m >> 32))
            acc += "        hi = or_if_bit(hi, " + std::to_string((uint32_t)(m >> 32)) + "u, " + bal + ");\n";
    }
    acc += "#endif\n";
    acc += "#endif\n";  // KSIGN
    // box-level pairs: one bit per distinct box, box u at bit u
    std::vector<uint16_t> box_tab;
    const int nbox = flat_box_pairs(leaves, n, &box_tab);
    if (nbox > 0) {
        std::string chain = "        lo = 0;\n        hi = 0;\n";
        for (int u = nbox - 1; u >= 0; u--) {
            const char* w = u >= 32 ? "hi" : "lo";
            chain += std::string("        ") + w + " = shl1_add_bit(" + w + ", __builtin_amdgcn_ballot_w64(b" +
                     std::to_string(u) + "));\n";
        }
        acc = "#if KBOX\n        uint32_t lo, hi;\n" + chain + "#else\n" + acc + "#endif\n";
    }
    acc += "        const unsigned long long m = ((unsigned long long)hi << 32) | lo;\n";
    const bool single = leaves_single(leaves, n);  // leaf k holds exactly triangle rank k
    // the sign-bit box bits need finite plane values: scene coordinates below 2^60 (tri_fast's
    // condition) with the kernel's ray bound (bounded_ray)
    const bool sign = tri_fast;
    std::string tabs = "{";
    for (size_t u = 0; u < box_tab.size(); u++) tabs += (u ? ", " : "") + std::to_string(box_tab[u]) + "u";
    tabs += box_tab.empty() ? "0u}" : "}";
    return std::string("#ifndef PT_FLAT_SIGN_MASK\n#define PT_FLAT_SIGN_MASK 0\n#endif\n#define KSIGN (PT_FLAT_SIGN_MASK && ") +
           (sign ? "1" : "0") + ")\n" + "#define KBOX " + (nbox > 0 ? "(!KSIGN)" : "0") + "\n" +
           "namespace pt {\nstruct SceneBoxMask {\n    static constexpr bool kSignMask = KSIGN;\n"
           "    static constexpr bool kBoxPairs = KBOX;\n    static constexpr int kBoxes = " + std::to_string(nbox) +
           ";\n    static constexpr uint16_t kBoxTab[" + std::to_string(std::max<size_t>(1, box_tab.size())) + "] = " + tabs +
           ";\n    static constexpr bool kMask32 = " +
           (n <= 32 ? "true" : "false") + ";\n    static constexpr bool kSingleTri = " + (single ? "true" : "false") +
           ";\n    static constexpr bool kSpecular = " + (specular ? "true" : "false") +
           ";\n    static constexpr bool kTriFast = " + (tri_fast ? "true" : "false") +
           ";\n    static constexpr bool kAlbedoX2 = " + (albedo_x2 ? "true" : "false") +
           ";\n    static constexpr bool kDarkKnown = true;\n    static constexpr bool kDark = " + (dark ? "true" : "false") +
           ";\n    __device__ __forceinline__ static unsigned long long "
           "mask(const TraceArgs&, v3 o, v3 inv) {\n" +
           body + tests + acc + "        return m;\n    }\n};\n}  // namespace pt\n";
}

struct RtcCache {
    std::mutex mu;
    std::map<std::string, RtcFuture> code;                        // source -> compile job
    std::map<std::pair<int, std::string>, hipFunction_t> funcs;   // (device, source) -> loaded kernel
    std::set<std::string> refused;  // disk keys whose code object the runtime refused: never read again
};
RtcCache& rtc_cache() {
    static RtcCache* c = new RtcCache();  // never destroyed: modules live for the process
    return *c;
}

// Waves per SIMD the scene kernel is register-allocated for: 8 (<= 64 VGPRs; with the
// AMDGPU pressure trackers below it needs 62-63 and no scratch, and 8 blocks of <= 20 KB
// fit the LDS): +2.4 % on Cornell, +2.2 % on config 3 against 7 (profiles/r04_sched).
int rtc_waves() {
    const char* e = hook_env("PT_RTC_WAVES");
    const int w = (e && *e) ? atoi(e) : 8;
    return (w >= 1 && w <= 8) ? w : 8;
}

// specular: the scene holds a SPECULAR material (else the sampler is compiled out).
// PT_RTC_DEFINES="NAME=VALUE,..." adds macros to the generated source (A/B experiments).
std::string rtc_defines() {
    const char* e = hook_env("PT_RTC_DEFINES");
    std::string out;
    if (!e) return out;
    std::stringstream ss(e);
    std::string item;
    while (std::getline(ss, item, ',')) {
        const size_t eq = item.find('=');
        if (!item.empty()) out += "#define " + (eq == std::string::npos ? item : item.substr(0, eq) + " " + item.substr(eq + 1)) + "\n";
    }
    return out;
}

// PT_RTC_FLAGS="-flag -flag ..." (or comma-separated) adds compiler options (A/B experiments; named in the
// generated source, so the per-process code cache keys on them).
std::vector<std::string> rtc_extra_flags() {
    std::vector<std::string> out;
    const char* e = hook_env("PT_RTC_FLAGS");
    if (!e) return out;
    std::string flags(e);
    std::replace(flags.begin(), flags.end(), ',', ' ');  // "-mllvm,-opt" in env lists that split on spaces
    std::stringstream ss(flags);
    std::string f;
    while (ss >> f) out.push_back(f);
    return out;
}

std::string rtc_flat_source(const std::vector<f4>& leaves, int n, bool specular, bool tri_fast, bool albedo_x2,
                            bool dark) {
    std::string fl = "// extra flags:";
    for (const std::string& f : rtc_extra_flags()) fl += " " + f;
    // camera fields from the kernel's argument registers at 8 waves: +0.5-1.0 % on configs
    // 2, 3, 5 against the kernarg-segment form the offline kernels keep (profiles/r04_switches).
    // threadIdx.x re-read at each use (fresh_tid) only in scenes with the specular sampler:
    // without it the kernel has VGPRs to spare at 8 waves and plain threadIdx.x is +0.5-1.2 %
    // (configs 2, 5); with it plain threadIdx.x costs SGPR spill lanes, -0.3 % (config 3)
    return fl + "\n" + rtc_defines() + "#define PT_WAVES " + std::to_string(rtc_waves()) +
           "\n#define PT_FLAT_ONLY 1\n#ifndef PT_CAM_KERNARG\n#define PT_CAM_KERNARG 0\n#endif\n"
           "#ifndef PT_FRESH_TID\n#define PT_FRESH_TID " + (specular ? "1" : "0") + "\n#endif\n"
           "typedef __hip_internal::int32_t int32_t; typedef __hip_internal::uint32_t uint32_t;\n"
           "typedef __hip_internal::int64_t int64_t; typedef __hip_internal::uint64_t uint64_t;\n"
           "typedef __hip_internal::uint8_t uint8_t; typedef __hip_internal::uint16_t uint16_t;\n"
           "#if !defined(__HIP_DEVICE_COMPILE__)\n#error expected a device compilation (pt_math.h fast paths)\n#endif\n"
           "#include \"pt_trace.h\"\n" +
           flat_mask_source(leaves, n, specular, tri_fast, albedo_x2, dark) +
           "extern \"C\" __global__ __launch_bounds__(256, PT_WAVES) void pt_trace_flat_rtc(pt::TraceArgs A) {\n"
           "    pt::trace_body_flat<pt::SceneBoxMask>(A);\n}\n";
}

// The hipRTC options of the scene kernel. The numerics flags of the offline build
// (Makefile): bit parity depends on them.
// -fno-slp-vectorize: the SLP vectorizer packs the path's scalar f32 math into
// v_pk_* pairs at the price of register shuffles (~20 v_mov per triangle test):
// 44.0 -> 49.0 Grays/s without it (bit-identical either way).
// -disable-machine-licm: as for the offline kernels (Makefile), loop-invariant values are
// not hoisted into registers live across the megakernel loop (60.1 vs 59.4 Grays/s).
// -amdgpu-use-amdgpu-trackers: the scheduler tracks register pressure with the AMDGPU
// trackers; the kernel then needs 62 VGPRs instead of 67 (at 7 waves) and fits 8 waves
// without scratch (LLVM's own trackers: 64 VGPRs and 12 B of scratch at 8). Scheduling
// only: the arithmetic and its bits are unchanged.
std::vector<std::string> rtc_flags() {
    std::vector<std::string> flags = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                                      "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
                                      "-fno-gpu-flush-denormals-to-zero", "-fno-slp-vectorize",
                                      "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-use-amdgpu-trackers"};
#ifdef PT_STAMPS
    flags.push_back("-DPT_STAMPS");
#endif
    for (const std::string& f : rtc_extra_flags()) flags.push_back(f);
    return flags;
}

// ---- on-disk code-object cache: a later process starts on the scene kernel at once
// instead of compiling it again (~0.4 s) while its first launches run the generic kernel.
// Directory: $PT_RTC_CACHE_DIR, else $XDG_CACHE_HOME/pathtracer-amd/rtc, else
// ~/.cache/pathtracer-amd/rtc; PT_RTC_CACHE=0 turns it off. Entry <key>.co, key = sha256 of
// the generated source, the embedded device headers, the compile options, the hipRTC
// version, the HIP runtime version and this format's tag; the file holds a header (magic,
// key, payload size, the payload's sha256) verified on every load, and an entry that fails
// any check is ignored, recompiled and rewritten. Only entries owned by the current user and
// writable by nobody else are read (the directory is created 0700), and an entry whose code
// object the runtime refuses to load is deleted and compiled again (rtc_resolve). Writes go
// to a temporary file renamed into place.
std::atomic<int64_t> g_rtc_disk_hits{0}, g_rtc_disk_rejects{0}, g_rtc_compiles{0};
std::atomic<int64_t> g_rtc_last_compile_us{0}, g_rtc_server_compiles{0};  // pt_debug_rtc_cache 4, 5
std::atomic<int64_t> g_ctx_created{0}, g_scene_uploads{0};  // pt_debug_counter
constexpr char kRtcMagic[8] = {'P', 'T', 'R', 'T', 'C', '0', '0', '1'};

std::string rtc_cache_dir() {
    const char* off = getenv("PT_RTC_CACHE");
    if (off && *off == '0') return "";
    const char* d = getenv("PT_RTC_CACHE_DIR");
    if (d && *d) return d;
    const char* x = getenv("XDG_CACHE_HOME");
    if (x && *x) return std::string(x) + "/pathtracer-amd/rtc";
    const char* h = getenv("HOME");
    if (h && *h) return std::string(h) + "/.cache/pathtracer-amd/rtc";
    return "";
}

// The file of the loaded library that defines `addr` ("" if none).
std::string lib_of(const void* addr) {
    Dl_info di;
    return dladdr(addr, &di) && di.dli_fname ? std::string(di.dli_fname) : std::string();
}

// The libraries a compile in this process uses: amd_comgr if something loaded it already
// (PyTorch's wheel ships its own, and hipRTC then uses that one), then hipRTC; with
// `runtime`, also the HIP runtime library.
std::vector<std::string> rtc_compiler_libs(bool runtime) {
    std::vector<std::string> libs;
    if (void* h = dlopen("libamd_comgr.so.3", RTLD_NOW | RTLD_NOLOAD)) {
        struct link_map* lm = nullptr;
        if (dlinfo(h, RTLD_DI_LINKMAP, &lm) == 0 && lm && lm->l_name && *lm->l_name) libs.push_back(lm->l_name);
        dlclose(h);
    }
    const std::string rtc = lib_of(reinterpret_cast<const void*>(&hiprtcCompileProgram));
    if (!rtc.empty()) libs.push_back(rtc);
    if (runtime) {
        const std::string hip = lib_of(reinterpret_cast<const void*>(&hipModuleLoadData));
        if (!hip.empty()) libs.push_back(hip);
    }
    return libs;
}

std::string rtc_key(const std::string& src) {
    Sha256 k;
    k.update("pathtracer-amd hipRTC code object v1");
    k.update(src.c_str(), src.size() + 1);
    for (const char* h : {pt_rtc_src_trace, pt_rtc_src_math, pt_rtc_src_hip}) k.update(h, strlen(h) + 1);
    for (const std::string& f : rtc_flags()) k.update(f.c_str(), f.size() + 1);
    int maj = 0, mnr = 0;
    (void)hiprtcVersion(&maj, &mnr);
    k.update(std::to_string(maj) + "." + std::to_string(mnr));
    // the headers this library was built with, and the identity (path, size, modification
    // time) of the libraries that compile and load the code object in this process: hipRTC,
    // amd_comgr when it is loaded, and the HIP runtime whose loader runs it (no HIP call:
    // pt_rtc_check keys compiles on hosts without a device). An upgraded runtime is a new key;
    // a code object a runtime still refuses is evicted and compiled again (rtc_load).
    k.update(std::to_string(HIP_VERSION) + " " + HIP_VERSION_GITHASH);
    for (const std::string& lib : rtc_compiler_libs(true)) {
        struct stat st;
        const bool ok = stat(lib.c_str(), &st) == 0;
        k.update(lib + " " + (ok ? std::to_string((long long)st.st_size) + " " + std::to_string((long long)st.st_mtime) : "?"));
    }
    return k.hex();
}

// The cache directory is used only if it belongs to this user and nobody else can write to
// it (an existing directory keeps its mode: mkdir's 0700 applies only to new ones).
bool rtc_dir_private(const std::string& dir) {
    struct stat st;
    return stat(dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode) && st.st_uid == geteuid() &&
           !(st.st_mode & (S_IWGRP | S_IWOTH));
}

bool rtc_disk_load(const std::string& key, std::vector<char>& code) {
    const std::string dir = rtc_cache_dir();
    if (dir.empty()) return false;
    if (!rtc_dir_private(dir)) {
        g_rtc_disk_rejects++;
        return false;
    }
    // the checks bind to the file actually read: no symlink is followed, and the owner, mode
    // and type come from the open descriptor
    const std::string path = dir + "/" + key + ".co";
    const int fd = open(path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
    if (fd < 0) {
        if (errno == ELOOP) g_rtc_disk_rejects++;
        return false;
    }
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_uid != geteuid() || (st.st_mode & (S_IWGRP | S_IWOTH)) || !S_ISREG(st.st_mode)) {
        close(fd);
        g_rtc_disk_rejects++;  // another user's (or a shared-writable) entry is never run
        return false;
    }
    auto rd = [fd](void* p, size_t n) {
        char* c = static_cast<char*>(p);
        while (n > 0) {
            const ssize_t r = read(fd, c, n);
            if (r <= 0) return false;
            c += r;
            n -= (size_t)r;
        }
        return true;
    };
    char magic[8], kh[64];
    uint64_t size = 0;
    uint8_t sum[32], got[32];
    bool ok = rd(magic, 8) && memcmp(magic, kRtcMagic, 8) == 0 && rd(kh, 64) && memcmp(kh, key.data(), 64) == 0 &&
              rd(&size, 8) && size > 0 && size < ((uint64_t)1 << 30) && (uint64_t)st.st_size == 112 + size &&
              rd(sum, 32);
    if (ok) {
        code.resize(size);
        ok = rd(code.data(), size);
    }
    close(fd);
    if (ok) {
        Sha256 p;
        p.update(code.data(), code.size());
        p.digest(got);
        ok = memcmp(got, sum, 32) == 0;
    }
    if (!ok) {
        code.clear();
        g_rtc_disk_rejects++;
        return false;
    }
    g_rtc_disk_hits++;
    return true;
}

void rtc_disk_store(const std::string& key, const std::vector<char>& code) {
    const std::string dir = rtc_cache_dir();
    if (dir.empty() || code.empty()) return;
    for (size_t i = 1; i <= dir.size(); i++)  // mkdir -p
        if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0700);
    if (!rtc_dir_private(dir)) return;
    std::ostringstream tn;
    tn << dir << "/" << key << ".co.tmp." << getpid() << "." << std::this_thread::get_id();
    const std::string tmp = tn.str();
    {
        const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0600);  // owner-only entry
        if (fd < 0) return;
        close(fd);
        std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
        if (!f) return;
        uint8_t sum[32];
        Sha256 p;
        p.update(code.data(), code.size());
        p.digest(sum);
        const uint64_t size = code.size();
        f.write(kRtcMagic, 8);
        f.write(key.data(), 64);
        f.write(reinterpret_cast<const char*>(&size), 8);
        f.write(reinterpret_cast<const char*>(sum), 32);
        f.write(code.data(), (std::streamsize)code.size());
        if (!f) {
            f.close();
            (void)unlink(tmp.c_str());
            return;
        }
    }
    if (rename(tmp.c_str(), (dir + "/" + key + ".co").c_str()) != 0) (void)unlink(tmp.c_str());
}

// ---- compile server (tools/pt_rtc_server.cc): the compiles run in a child process that
// loads the same hipRTC / amd_comgr libraries as this one. In this process a compile on a
// background thread runs inside amd_comgr, whose lazily constructed statics register their
// destructors with atexit during the compile — after any handler that waits for it — so a
// process exiting with a compile in flight destroyed them under it (SIGSEGV in the compile
// thread, a call through a destroyed object from amd_comgr_do_action; reproduced without a
// GPU, tests/test_rtc_exit.py). With the server, exit only closes a socket.
// One server per process, started on the first compile, one request at a time; it exits at
// end of input. PT_RTC_SERVER=0 (test hook), a missing server binary or a failed exchange:
// the compile runs in this process (the round-5 form).
struct RtcServer {
    std::mutex mu;
    pid_t pid = -1;
    int fd = -1;
    bool broken = false;  // could not start or failed: compile in this process from then on
};
RtcServer& rtc_server() {
    static RtcServer* s = new RtcServer();  // never destroyed (used by threads at exit)
    return *s;
}

// bin/pt_rtc_server next to this library's lib/ directory ("" if absent)
std::string rtc_server_path() {
    if (const char* e = hook_env("PT_RTC_SERVER"))
        if (*e == '0') return "";
    std::string p = lib_of(reinterpret_cast<const void*>(&rtc_server_path));
    const size_t k = p.rfind('/');
    if (k == std::string::npos) return "";
    p = p.substr(0, k) + "/../bin/pt_rtc_server";
    return access(p.c_str(), X_OK) == 0 ? p : "";
}

bool rtc_server_start(RtcServer& s) {
    const std::string path = rtc_server_path();
    if (path.empty()) return false;
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0, sv) != 0) return false;
    std::vector<std::string> args{path};
    for (const std::string& lib : rtc_compiler_libs(false)) args.insert(args.end(), {"--lib", lib});
    std::vector<char*> argv;
    for (std::string& a : args) argv.push_back(&a[0]);
    argv.push_back(nullptr);
    posix_spawn_file_actions_t fa;
    posix_spawnattr_t at;
    posix_spawn_file_actions_init(&fa);
    posix_spawn_file_actions_adddup2(&fa, sv[1], 0);
    posix_spawn_file_actions_adddup2(&fa, sv[1], 1);
    posix_spawn_file_actions_addclosefrom_np(&fa, 3);  // no GPU or other descriptors of ours in the child
    posix_spawnattr_init(&at);
    sigset_t none, dflt;
    sigemptyset(&none);
    sigemptyset(&dflt);
    sigaddset(&dflt, SIGPIPE);
    posix_spawnattr_setsigmask(&at, &none);
    posix_spawnattr_setsigdefault(&at, &dflt);
    posix_spawnattr_setflags(&at, POSIX_SPAWN_SETSIGMASK | POSIX_SPAWN_SETSIGDEF);
    pid_t pid = -1;
    const int rc = posix_spawn(&pid, path.c_str(), &fa, &at, argv.data(), environ);
    posix_spawn_file_actions_destroy(&fa);
    posix_spawnattr_destroy(&at);
    close(sv[1]);
    if (rc != 0) {
        close(sv[0]);
        return false;
    }
    s.pid = pid;
    s.fd = sv[0];
    return true;
}

void rtc_server_stop(RtcServer& s) {
    if (s.fd >= 0) close(s.fd);
    if (s.pid > 0) {
        kill(s.pid, SIGKILL);
        (void)waitpid(s.pid, nullptr, 0);
    }
    s.fd = -1;
    s.pid = -1;
    s.broken = true;
}

// One compile through the server; false if the exchange failed (then the caller compiles here).
bool rtc_server_compile(const std::string& src, RtcCode& out) {
    RtcServer& s = rtc_server();
    std::lock_guard<std::mutex> lock(s.mu);
    if (s.broken) return false;
    if (s.fd < 0 && !rtc_server_start(s)) {
        s.broken = true;
        return false;
    }
    const int fd = s.fd;
    auto put = [fd](const void* p, size_t n) {
        const char* c = static_cast<const char*>(p);
        while (n > 0) {
            const ssize_t r = send(fd, c, n, MSG_NOSIGNAL);
            if (r <= 0) return false;
            c += r;
            n -= (size_t)r;
        }
        return true;
    };
    auto get = [fd](void* p, size_t n) {
        char* c = static_cast<char*>(p);
        while (n > 0) {
            const ssize_t r = recv(fd, c, n, 0);
            if (r <= 0) return false;
            c += r;
            n -= (size_t)r;
        }
        return true;
    };
    auto put_str = [&put](const char* str, size_t n) {
        const uint64_t len = n;
        return put(&len, 8) && put(str, n);
    };
    const char* hdrs[] = {pt_rtc_src_trace, pt_rtc_src_math, pt_rtc_src_hip};
    const char* names[] = {"pt_trace.h", "pt_math.h", "pt_hip.h"};
    const std::vector<std::string> flags = rtc_flags();
    const uint32_t head[3] = {0x51525450u /* "PTRQ" */, 3u, (uint32_t)flags.size()};
    bool ok = put(head, 12) && put_str(src.data(), src.size());
    for (int i = 0; ok && i < 3; i++) ok = put_str(names[i], strlen(names[i])) && put_str(hdrs[i], strlen(hdrs[i]));
    for (size_t i = 0; ok && i < flags.size(); i++) ok = put_str(flags[i].data(), flags[i].size());
    uint32_t resp[2] = {0, 0};
    uint64_t n = 0;
    ok = ok && get(resp, 8) && resp[0] == 0x53525450u /* "PTRS" */ && get(&n, 8) && n < ((uint64_t)1 << 30);
    std::vector<char> bytes;
    if (ok) {
        bytes.resize(n);
        ok = n == 0 || get(bytes.data(), n);
    }
    if (!ok) {
        rtc_server_stop(s);
        return false;
    }
    if (resp[1] == 1) {
        out.code = std::move(bytes);
    } else {
        out.status = "hipRTC compile failed: " + std::string(bytes.begin(), bytes.begin() + std::min<size_t>(bytes.size(), 400));
    }
    return true;
}

// Compile `src` to a code object (or an error status), stored in the disk cache under
// `key`. Runs on a background thread: through the compile server when there is one.
std::shared_ptr<const RtcCode> rtc_compile(const std::string& src, const std::string& key) {
    auto out = std::make_shared<RtcCode>();
    g_rtc_compiles++;
    const auto t0 = std::chrono::steady_clock::now();
    auto done = [&t0]() {
        g_rtc_last_compile_us =
            std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    };
    if (rtc_server_compile(src, *out)) {
        done();
        g_rtc_server_compiles++;
        if (!out->code.empty()) rtc_disk_store(key, out->code);
        return out;
    }
    const char* hdrs[] = {pt_rtc_src_trace, pt_rtc_src_math, pt_rtc_src_hip};
    const char* names[] = {"pt_trace.h", "pt_math.h", "pt_hip.h"};
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "pt_trace_flat_rtc.hip", 3, hdrs, names) != HIPRTC_SUCCESS) {
        out->status = "hiprtcCreateProgram failed";
        return out;
    }
    const std::vector<std::string> flags = rtc_flags();
    std::vector<const char*> opts;
    for (const std::string& f : flags) opts.push_back(f.c_str());
    if (hiprtcCompileProgram(prog, (int)opts.size(), opts.data()) != HIPRTC_SUCCESS) {
        size_t ls = 0;
        hiprtcGetProgramLogSize(prog, &ls);
        std::string log(ls, '\0');
        if (ls) hiprtcGetProgramLog(prog, &log[0]);
        out->status = "hipRTC compile failed: " + log.substr(0, 400);
    } else {
        size_t cs = 0;
        hiprtcGetCodeSize(prog, &cs);
        out->code.resize(cs);
        hiprtcGetCode(prog, out->code.data());
        done();
        rtc_disk_store(key, out->code);
    }
    hiprtcDestroyProgram(&prog);
    return out;
}

// Wait for every background compile started so far (deferred jobs are not run); returns how
// many were still running.
int rtc_wait_all() {
    std::vector<RtcFuture> jobs;
    {
        RtcCache& c = rtc_cache();
        std::lock_guard<std::mutex> lock(c.mu);
        for (auto& kv : c.code) jobs.push_back(kv.second);
    }
    int running = 0;
    for (RtcFuture& f : jobs) {
        if (!f.valid()) continue;
        const std::future_status st = f.wait_for(std::chrono::seconds(0));
        if (st == std::future_status::deferred) continue;
        if (st != std::future_status::ready) running++;
        f.wait();
    }
    return running;
}

// Background compiles: with the compile server the exit handler below only waits for its
// answer (so the code object reaches the disk cache for the next process). Without a server
// the compile runs in this process, and the compiler library is loaded first so that at least
// its load-time statics outlive the handler (exit() runs handlers in reverse registration
// order); the statics it constructs during a compile are not covered (see RtcServer), which is
// why the server is the default. No compiler library: compiles run synchronously.
bool rtc_async_ready() {
    static const bool ok = [] {
        if (rtc_server_path().empty()) {
            void* h = dlopen("libamd_comgr.so.3", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("libamd_comgr.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) return false;
        }
        std::atexit([] { (void)rtc_wait_all(); });
        return true;
    }();
    return ok;
}

// The compile job for `src`: the process's own result if it has one, else a verified
// entry of the disk cache (read here, so the first launch already finds the kernel ready),
// else a compile started on first request (on a background thread when possible); shared
// by every context and device that asks for the same source.
RtcFuture rtc_job(const std::string& src) {
    RtcCache& cache = rtc_cache();
    const bool async = rtc_async_ready();
    std::lock_guard<std::mutex> lock(cache.mu);
    auto it = cache.code.find(src);
    if (it != cache.code.end()) return it->second;
    const std::string key = rtc_key(src);
    RtcFuture f;
    auto disk = std::make_shared<RtcCode>();
    // an entry the runtime refused once is never read again (rtc_load): the retry compiles
    if (!cache.refused.count(key) && rtc_disk_load(key, disk->code)) {
        disk->disk_key = key;
        std::promise<std::shared_ptr<const RtcCode>> p;
        p.set_value(disk);
        f = p.get_future().share();
    } else {
        f = async ? std::async(std::launch::async, rtc_compile, src, key).share()
                  : std::async(std::launch::deferred, rtc_compile, src, key).share();
    }
    cache.code.emplace(src, f);
    return f;
}

// Whether a scene takes the flat path: at most kMaxFlatLeaves leaves, and
// triangle ranks that fit the path records' 16 bits. pt_ctx_set_scene starts the hipRTC
// compile, render_range picks the flat kernels and pt_rtc_check compiles by this one rule.
bool flat_eligible(const PackedScene& m) {
    return m.num_leaves > 0 && m.num_leaves <= kMaxFlatLeaves && m.num_tris < 65536;
}

// Material types sit in the first float4 of each position's pair (pt_internal.h).
bool scene_has_specular(const PackedScene& ps) {
    for (size_t i = 0; i < ps.mats.size(); i += 2)
        if (__builtin_bit_cast(int, ps.mats[i].x) == PT_MAT_SPECULAR) return true;
    return false;
}

// Whether finish_path may skip the unwinding of a path whose end value is +0:
// a level of render.h:60, e + (L a) c, is then +0 + (+-0) = +0 for every bounce of the path.
// That needs, per non-emitting triangle (the only ones a path bounces off):
//   * emission bits +0 and a finite albedo a (material.h:27-38), so (L a) is +-0;
//   * a finite cos theta c = n . new_d (render.h:56-59): the shading normal finite with
//     |n|^2 in [0.999, 1.001] (normalize(cross(e1, e2)), triangle.h:45-49: a sliver whose cross
//     product rounds to 0 or underflows gives a NaN / inaccurate normal), and for SPECULAR
//     materials |roughness| <= 1.15, so that specular_sample's ret = refl + j (material.h:15-25)
//     never vanishes: |j| <= |r| sqrt(3) / 2 (1 + u) <= 0.9960 while |refl| >= 0.998 (|d| = 1
//     within a few ulps for every ray the kernel traces, |n|^2 >= 0.999), so normalize(ret)
//     divides by a length >= 0.0019 and the new direction is finite. At |r| >= 2 / sqrt(3) a
//     draw can cancel refl exactly and the reference's cos theta is NaN, so its path value is
//     NaN where a skipped unwinding would store +0 (VERDICT r5 finding 1).
// Diffuse directions are always finite (hemisphere_sample: |components| <= 1). PT_DARK=0 (test
// hook) turns the skip off.
bool scene_dark(const PackedScene& ps) {
    const char* e = hook_env("PT_DARK");
    if (e && *e == '0') return false;
    for (size_t i = 0; i + 1 < ps.mats.size(); i += 2) {
        const int type = __builtin_bit_cast(int, ps.mats[i].x);
        if (type == PT_MAT_EMIT) continue;
        const f4 a = ps.mats[i], b = ps.mats[i + 1];
        if (!std::isfinite(a.y) || !std::isfinite(a.z) || !std::isfinite(a.w)) return false;
        if (f2u(b.x) | f2u(b.y) | f2u(b.z)) return false;
        if (type == PT_MAT_SPECULAR && !(std::fabs(b.w) <= 1.15f)) return false;
        const f4 t = ps.tris[3 * (i / 2) + 2];  // {e2.z, n.xyz} at the same rank position
        const double n2 = (double)t.y * t.y + (double)t.z * t.z + (double)t.w * t.w;
        if (!(n2 >= 0.999 && n2 <= 1.001)) return false;
    }
    return true;
}

// Whether the flat kernel may unwind with pre-doubled albedo (finish_path<., true>: L * 2a
// instead of (2L) * a, the same bits while 2L cannot overflow). Requires every material
// finite with |2 * albedo| finite, and the radiance bound B_{j+1} = e + (2 a B_j) c over
// PT_MAX_DEPTH levels (a, e: the largest |albedo| and |emission| components, c: |cos| <= 1
// with a margin for rounding) below 2^125. PT_ALBEDO_X2=0 (test hook) turns it off.
bool albedo_x2_ok(const PackedScene& ps) {
    const char* e = hook_env("PT_ALBEDO_X2");
    if (e && *e == '0') return false;
    double a_max = 0.0, e_max = 0.0;
    for (size_t i = 0; i + 1 < ps.mats.size(); i += 2) {
        const float v[6] = {ps.mats[i].y, ps.mats[i].z, ps.mats[i].w, ps.mats[i + 1].x, ps.mats[i + 1].y, ps.mats[i + 1].z};
        for (int j = 0; j < 6; j++)
            if (!std::isfinite(v[j])) return false;
        for (int j = 0; j < 3; j++) a_max = std::max(a_max, (double)std::fabs(v[j]));
        for (int j = 3; j < 6; j++) e_max = std::max(e_max, (double)std::fabs(v[j]));
    }
    if (!(2.0 * a_max < 0x1p127)) return false;
    const double c_max = 1.0 + 0x1p-10;
    double b = 0.0;
    for (int lvl = 0; lvl < PT_MAX_DEPTH; lvl++) {
        b = e_max + (2.0 * a_max * b) * c_max;
        if (!(b < 0x1p125)) return false;
    }
    return true;
}

// Load a finished compile of `src` on `device` (once per device and source).
hipFunction_t rtc_load(int device, const std::string& src, const RtcCode& code, std::string& status) {
    if (code.code.empty()) {
        status = code.status;
        return nullptr;
    }
    RtcCache& cache = rtc_cache();
    std::lock_guard<std::mutex> lock(cache.mu);
    auto fit = cache.funcs.find({device, src});
    if (fit != cache.funcs.end()) return fit->second;
    hipModule_t mod;
    hipFunction_t fn;
    if (hipModuleLoadData(&mod, code.code.data()) != hipSuccess ||
        hipModuleGetFunction(&fn, mod, "pt_trace_flat_rtc") != hipSuccess) {
        status = "hipModuleLoadData/GetFunction failed";
        if (!code.disk_key.empty()) {  // a cached entry this runtime refuses: evicted, compiled again
            const std::string dir = rtc_cache_dir();
            if (!dir.empty()) (void)unlink((dir + "/" + code.disk_key + ".co").c_str());
            g_rtc_disk_rejects++;
            cache.code.erase(src);
            // marked even if the unlink failed (a read-only cache): the next job for this
            // source compiles instead of reading the entry again, so the retry happens once
            cache.refused.insert(code.disk_key);
            status = "evicted";
        }
        return nullptr;
    }
    cache.funcs[{device, src}] = fn;
    status.clear();
    return fn;
}

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
// output buffers stay (pt_multi.hip: cached multi-device contexts after each render).
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
        else if (hipMalloc((void**)&c->d_ctr, 4 * sizeof(unsigned long long)) != hipSuccess)
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
                    (void*)c->d_tslab, (void*)c->d_trec, (void*)c->d_tbuf, (void*)c->d_tstates, (void*)c->d_tctr})
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
    // The scene-specialised kernel's compile starts before the upload (and before the
    // context's stream is waited for): renders pick it up (render_range: rtc_resolve).
    const char* rtc_env = hook_env("PT_RTC");
    const bool want_rtc = flat_eligible(ps) && !(rtc_env && *rtc_env == '0');
    std::string src;
    RtcFuture job;
    if (want_rtc) {
        src = rtc_flat_source(ps.leaves, ps.num_leaves, specular, ps.coords_small, albedo_x2, dark);
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
    c->albedo_x2 = false;
    // the table kernel a flat scene runs until its hipRTC kernel is ready: with the scene's
    // flags when it has the usual ones (PT_FLAT_FAST=0, test hook: the fully generic one)
    c->flat_fast = nullptr;
    const char* ff = hook_env("PT_FLAT_FAST");
    if (flat_eligible(ps) && !(ff && *ff == '0') && leaves_single(ps.leaves, ps.num_leaves) && ps.coords_small &&
        c->dark && albedo_x2)
        c->flat_fast = flat_fast_kernel(specular, ps.num_leaves <= 32);
    c->flat_boxes = 0;
    c->rtc_requested = false;
    c->flat_host = ps.leaves;
    ps.leaves.clear();
    c->meta = ps;
    c->rtc_flat = nullptr;
    c->rtc_job = RtcFuture();
    c->rtc_src.clear();
    c->rtc_status = "not a flat scene";
    if (want_rtc) {
        c->rtc_src = std::move(src);
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

// Samples [s_lo, s_hi) of this part added to the running sum (a new sum when s_lo == 0),
// the image = sum / s_hi written to `out`; keep: the sum stays in d_accum (progressive).
static int render_range(pt_ctx* c, const pt_camera* cam, const pt_params* prm, int s_lo, int s_hi, int keep,
                        float* out, int out_is_device, pt_stats* stats) {
    const auto t_start = std::chrono::steady_clock::now();
    if (!c || !cam || !prm || !out) return set_error(PT_E_ARG, "pt_ctx_render: NULL argument");
    if (s_lo < 0 || s_hi < s_lo) return set_error(PT_E_ARG, "bad sample range [%d, %d)", s_lo, s_hi);
    if (!c->have_scene) return set_error(PT_E_ARG, "pt_ctx_render: no scene set");
    if (int rc0 = ctx_ready(c)) return rc0;
    const int W = cam->res[0], H = cam->res[1];
    if (W <= 0 || H <= 0) return set_error(PT_E_ARG, "camera resolution must be positive");
    const int parts = prm->part_count > 0 ? prm->part_count : 1;
    const int band = prm->band_rows > 0 ? prm->band_rows : 1;
    if (prm->part_index < 0 || prm->part_index >= parts) return set_error(PT_E_ARG, "part_index out of range");
    if (prm->depth > PT_MAX_DEPTH) return set_error(PT_E_ARG, "depth %d exceeds PT_MAX_DEPTH", prm->depth);
    const int rows = pt_part_rows(H, prm->part_index, parts, band);
    const long long npix_ll = (long long)rows * W;
    if (npix_ll > (1ll << 30)) return set_error(PT_E_ARG, "too many pixels for one part");
    const int npix = (int)npix_ll;
    const int spp = s_hi;  // the image is the running sum / spp (render.h:97)
    HIP_TRY(hipSetDevice(c->device));

    // batch size: radiance slab of 3 * batch * npix floats within the budget
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

    int rc;
    if ((rc = ensure(&c->d_accum, &c->accum_floats, 3 * (size_t)npix))) return rc;
    float* dst = out;
    if (!out_is_device) {
        if ((rc = ensure(&c->d_out, &c->out_floats, 3 * (size_t)npix))) return rc;
        dst = c->d_out;
    }

    const int rec = std::max(1, prm->depth - 1);
    // Wide tree for scenes past the flat list (the 99k-triangle mesh); PT_WIDE=0 disables
    // it, PT_WIDE=1 also uses it where the flat list would apply (tests).
    const char* fenv = hook_env("PT_FLAT");
    const char* wenv = hook_env("PT_WIDE");
    const bool flat_ok = flat_eligible(c->meta) && !(fenv && *fenv == '0');
    const bool wide = c->meta.num_wide > 0 && !(wenv && *wenv == '0') && (!flat_ok || (wenv && *wenv == '1'));
    const bool flat = flat_ok && !wide;
    if (flat && per_item != 1) {  // the flat kernel's work items are single samples (claim_item)
        per_item = 1;
        batch = (int)std::min<long long>(batch, std::max<long long>(1, ((1ll << 31) - 1) / std::max(npix, 1)));
    }
    // Flat path: (lane, leaf) pair queues of 512 16-bit entries per wave; PT_PAIRS=0
    // disables them (per-lane loops), PT_PAIR_QUEUE=n shrinks them (overflow fallback).
    const char* penv = hook_env("PT_PAIRS");
    const bool pairs = flat && !(penv && *penv == '0');
    // the hipRTC kernel's box table (box-level pairs), after the prefetched camera rays
    const size_t box_tab_bytes = flat ? (sizeof(uint16_t) * (size_t)c->flat_boxes + 3) & ~(size_t)3 : 0;
    int pair_queue = pairs ? 512 : 0;
    const char* pq = hook_env("PT_PAIR_QUEUE");
    if (pairs && pq && *pq) {
        pair_queue = std::max(1, std::min(pair_queue, atoi(pq)));
    } else if (pairs && c->lds_usable > 0) {
        // Shorter queues where that lets one more block per CU fit the LDS (up to the 8 the
        // registers allow): modified Cornell's 34 triangles put its block 160 B over the
        // 8-block share with 512 entries, config 5's depth-8 records fit 6 blocks, not 7.
        // A wave-iteration rarely holds more pairs than the shorter queue (overflow: the
        // per-lane loop, same bits).
        const size_t fixed = sizeof(float4) * (size_t)(3 + 2) * c->meta.num_tris +
                             (sizeof(uint16_t) + sizeof(float)) * (size_t)kBlock * rec + sizeof(unsigned long long) * kBlock +
                             (sizeof(float4) + sizeof(uint32_t)) * kBlock + box_tab_bytes;
        auto blocks = [&](int q) {
            const size_t b = fixed + sizeof(uint16_t) * (size_t)q * (kBlock / kWave);
            return std::min<int>(8, (int)(c->lds_usable / ((b + kLdsGranule - 1) / kLdsGranule * kLdsGranule)));
        };
        const int want = blocks(kPairQueueMin);
        while (pair_queue > kPairQueueMin && blocks(pair_queue) < want) pair_queue -= 32;
    }
    pair_queue = (pair_queue + 3) & ~3;  // keeps the records after the queues 8-B aligned
    const int stack = std::max(1, c->meta.tree_depth);  // tree kernels: child-pair stack rows in LDS
    // Wide walk: LDS holds the top levels of the tree, one stack row per wide level above
    // the last (a node of the last level has no inner children to push) and a
    // triangle queue of 128 entries (8 B) per wave. The exact binary walk (rays with a
    // zero direction component) of the wide and flat kernels keeps its stack (tree depth
    // rows) in HBM.
    const int wide_rows = wide ? std::max(1, c->meta.wide_depth - 1) : 0;
    int wide_queue = 160;  // 128: -0.35 % on config 4 (profiles/r03y_lds); PT_WIDE_QUEUE_LEN (tuning hook) sets another length
    if (const char* wl = hook_env("PT_WIDE_QUEUE_LEN")) wide_queue = std::max(64, std::min(1024, atoi(wl)));
    int wide_top = wide ? c->meta.wide_top : 0;  // may shrink below, to keep the occupancy
    if (wide && c->meta.num_tris >= (1 << 26))  // queue entries hold the triangle index in 32 bits, count in 26
        return set_error(PT_E_ARG, "wide path: %d triangles exceed 2^26", c->meta.num_tris);
    const int node4 = 2 * c->meta.num_nodes, tri4 = 3 * c->meta.num_tris, mat4 = 2 * c->meta.num_tris;
    size_t lds_bytes = 0;
    bool lds_scene = false;
    const char* ws = hook_env("PT_WIDE_SINGLE");  // test hook: 0 = the general leaf-range decode
    const bool wide_single = wide && c->meta.wide_single && !(ws && *ws == '0');
    if (wide) {
        // the distinct materials go to LDS when there are few (PT_UMAT_LDS_MAX: test hook)
        const char* um = hook_env("PT_UMAT_LDS_MAX");
        lds_scene = c->meta.num_umats <= std::min((um && *um) ? atoi(um) : kMaxLdsMaterials, kMaxLdsRowsByte);
        lds_bytes = (size_t)wide_top * 16 * kWideNodeU4(c->meta.wide_width, c->meta.wide_fmt) + sizeof(int) * (size_t)kBlock * wide_rows +
                    (wide_single ? 4 : 8) * (size_t)wide_queue * (kBlock / kWave) +
                    (sizeof(float) + (lds_scene ? sizeof(uint8_t) : sizeof(int))) * (size_t)kBlock * rec +
                    sizeof(unsigned long long) * kBlock + (lds_scene ? sizeof(float4) * 2 * (size_t)c->meta.num_umats : 0);
    } else if (flat) {
        lds_scene = true;  // triangles + materials (Cornell: 2.5 KB)
        lds_bytes = sizeof(float4) * ((size_t)tri4 + mat4) + sizeof(uint16_t) * (size_t)pair_queue * (kBlock / kWave) +
                    (sizeof(uint16_t) + sizeof(float)) * (size_t)kBlock * rec + sizeof(unsigned long long) * kBlock +
                    (sizeof(float4) + sizeof(uint32_t)) * kBlock + box_tab_bytes;
    } else {
        const size_t work = sizeof(int) * (size_t)kBlock * (stack + 2 * rec);
        const size_t scene = sizeof(float4) * ((size_t)node4 + tri4 + mat4);
        lds_scene = scene <= lds_scene_budget() && scene + work <= 64 * 1024;
        lds_bytes = work + (lds_scene ? scene : 0);
    }
    if (lds_bytes > 160 * 1024)
        return set_error(PT_E_ARG, "BVH depth (%d) x path depth needs %zu B of LDS", wide ? wide_rows : stack, lds_bytes);
    // The hipRTC kernel: a render does not wait for its compile. Launches run the generic
    // flat kernel (the same algorithm with the box table in kernel arguments: same bits)
    // until the compile is done and switch between launches (below). PT_RTC_SWITCH=0
    // (tuning hook): renders of >= 2^28 paths wait for the compile first (round 2's rule).
    const char* rsw = hook_env("PT_RTC_SWITCH");
    const bool rtc_switch = !(rsw && *rsw == '0');
    const char* rsa = hook_env("PT_RTC_SWITCH_AT");  // test hook: wait for the compile before launch k
    const int rtc_switch_at = (rsa && *rsa) ? atoi(rsa) : -1;
    if (flat && c->rtc_job.valid()) rtc_resolve(c, !rtc_switch && (double)npix * (spp - s_lo) >= kRtcWaitPaths);
    auto kern = flat        ? (c->flat_fast ? (TraceKernel)c->flat_fast : pt_trace_kernel<true, true>)
                : wide      ? wide_kernel(c->meta.wide_width, c->meta.wide_fmt, lds_scene)
                : lds_scene ? pt_trace_kernel<true, false>
                            : pt_trace_kernel<false, false>;
    bool use_rtc = flat && c->rtc_flat != nullptr;
    if (wide && wide_top > 0) {
        // The LDS copy of the top nodes takes only what the blocks the kernel's registers
        // allow per CU leave free: as many of the packed top nodes (an index prefix) as fit
        // without losing a block (a lost block cost 8 %, profiles/r03y_lds).
        // The occupancy query is optimistic about LDS: blocks of 27,072 B were reported to
        // fit 6 per CU and ran 5 (-8 %), blocks of 26,816 B ran 6 (profiles/r03z_lds). The
        // count is also checked against that measured bound (kLdsUsable, 256-B granule).
        const size_t node_bytes = 16 * (size_t)kWideNodeU4(c->meta.wide_width, c->meta.wide_fmt);
        const size_t rest = lds_bytes - (size_t)wide_top * node_bytes;
        const size_t usable = c->lds_usable;
        auto lds_blocks = [usable](size_t bytes) { return (int)(usable / ((bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule)); };
        int full = 0, with = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&full, kern, kBlock, rest));
        full = std::min(full, lds_blocks(rest));
        while (wide_top > 0) {
            const size_t b = rest + (size_t)wide_top * node_bytes;
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&with, kern, kBlock, b));
            if (std::min(with, lds_blocks(b)) >= full) break;
            wide_top--;
        }
        lds_bytes = rest + (size_t)wide_top * node_bytes;
    }
    int blocks_per_cu = 0;
    if (use_rtc)
        HIP_TRY(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, c->rtc_flat, kBlock, lds_bytes));
    else
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kern, kBlock, lds_bytes));
    // the occupancy query can be optimistic about LDS (above): never more blocks than the
    // measured per-CU LDS holds (the flat kernel at 8 waves: 8 blocks of <= 20,160 B)
    if (lds_bytes > 0 && c->lds_usable > 0)
        blocks_per_cu = std::min<int>(blocks_per_cu,
                                      (int)(c->lds_usable / ((lds_bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule)));
    blocks_per_cu = std::max(1, blocks_per_cu);
    const int exact_rows = std::max(1, c->meta.tree_depth);
    if (wide || flat) {
        // a compile still running may switch this render to the hipRTC kernel, whose
        // occupancy is not known yet: stacks for the most blocks a CU holds (8 of 256)
        const bool may_switch = flat && !use_rtc && c->rtc_job.valid();
        const size_t need = (size_t)(may_switch ? std::max(blocks_per_cu, 8) : blocks_per_cu) * c->num_cus * kBlock * exact_rows;
        if (need > c->xstack_ints) {
            if (c->d_xstack) (void)hipFree(c->d_xstack);
            c->d_xstack = nullptr;
            c->xstack_ints = 0;
            HIP_TRY(hipMalloc((void**)&c->d_xstack, need * sizeof(int)));
            c->xstack_ints = need;
        }
    }

    TraceArgs A;
    memset(&A, 0, sizeof(A));
    A.nodes = c->d_nodes;
    A.tris = c->d_tris;
    A.mats = c->d_mats;
    A.leaves = c->d_leaves;
    A.wide = reinterpret_cast<const uint4*>(c->d_wide);
    A.wtris = c->d_wtris;
    A.nrm = c->d_nrm;
    A.umats = c->d_umats;
    A.num_umat4 = wide ? 2 * c->meta.num_umats : 0;
    A.num_leaves = flat ? c->meta.num_leaves : 0;
    {
        // distinct boxes (bitwise), each with the mask of its leaves; padding boxes set no bit
        int nb = 0;
        for (int k = 0; k < A.num_leaves; k++) {
            const f4* L = &c->flat_host[2 * k];
            const float b6[6] = {L[0].x, L[0].y, L[0].z, L[0].w, L[1].x, L[1].y};
            int u = 0;
            while (u < nb && memcmp(A.flat.box[u], b6, sizeof(b6)) != 0) u++;
            if (u == nb) {
                memcpy(A.flat.box[nb], b6, sizeof(b6));
                A.flat.bits[nb++] = 0;
            }
            A.flat.bits[u] |= 1ull << k;
        }
        A.num_boxes_padded = (nb + 3) & ~3;
        for (int u = nb; u < A.num_boxes_padded; u++) {
            memcpy(A.flat.box[u], A.flat.box[0], sizeof(A.flat.box[0]));
            A.flat.bits[u] = 0;
        }
    }
    A.radiance = c->d_radiance;
#if PT_THETA_TAB
    {
        // the table (256 MB per device, built once) only for scenes with a SPECULAR
        // material, where few lanes of a wave sample the hemisphere at a time
        const char* tl = hook_env("PT_THETA_LANES");
        A.theta_lanes = (tl && *tl) ? atoi(tl) : (c->has_specular ? 32 : 0);
        if (PT_THETA_TAB == 1 || A.theta_lanes > 0) {
            const float2* tab = nullptr;
            if ((rc = theta_table(c, &tab))) {
                // the computed hemisphere_dir gives the same bits: without the table every
                // wave computes (the forced all-table build has no such fallback)
                if (PT_THETA_TAB == 1) return rc;
                A.theta_lanes = 0;
                tab = nullptr;
            }
            A.theta_tab = tab;
        }
    }
#endif
    A.work = c->d_ctr;
    A.ctr = c->d_ctr;
    A.dark = c->dark ? 1 : 0;
    A.pos_x = cam->pos[0];
    A.pos_y = cam->pos[1];
    A.pos_z = cam->pos[2];
    const float* T = cam->transform;  // rows right, up, -forward; columns feed get_ray's dots
    A.col0_x = T[0]; A.col0_y = T[3]; A.col0_z = T[6];
    A.col1_x = T[1]; A.col1_y = T[4]; A.col1_z = T[7];
    A.col2_x = T[2]; A.col2_y = T[5]; A.col2_z = T[8];
    A.half_vres_x = cam->v_res[0] / 2.0f;
    A.half_vres_y = cam->v_res[1] / 2.0f;
    A.cell = cam->cell_size;
    A.cz_col0 = -cam->distance * A.col0_z;  // the float products camera_ray's z terms use
    A.cz_col1 = -cam->distance * A.col1_z;
    A.cz_col2 = -cam->distance * A.col2_z;
    A.W = W;
    A.npix = npix;
    A.part_index = prm->part_index;
    A.part_count = parts;
    A.band_rows = band;
    A.depth = prm->depth;
    A.seed = prm->seed;
    A.per_item = per_item;
    A.div_npix = make_fastdiv((uint32_t)std::max(npix, 1));
    A.div_w = make_fastdiv((uint32_t)W);
    A.div_band = make_fastdiv((uint32_t)band);
    A.stack_size = stack;
    A.rec_size = rec;
    A.num_node4 = node4;
    A.num_tri4 = tri4;
    A.num_mat4 = mat4;
    {
        const char* fe = hook_env("PT_FORCE_EXACT_SLAB");
        A.force_exact_slab = (fe && (*fe == '1' || *fe == '2')) ? *fe - '0' : 0;
        const char* th = hook_env("PT_WIDE_THRESH");
        // 99k mesh (r02e build): 16 -8 %, 20 -3.5 %, 24 -1.4 %, 28 best, 32 -0.7 %
        A.wide_thresh = (th && *th) ? std::max(1, std::min(64, atoi(th))) : 28;
        A.pair_queue = pair_queue;
        A.wide_rows = wide_rows;
        A.exact_stack = c->d_xstack;
        A.exact_rows = exact_rows;
        A.wide_queue = wide ? wide_queue : 0;
        A.wide_top = wide_top;
        A.wide_nodes = wide ? (uint32_t)c->meta.num_wide : 0u;
        A.wide_span_x = c->meta.wide_span[0];
        A.wide_span_y = c->meta.wide_span[1];
        A.wide_span_z = c->meta.wide_span[2];
        A.wide_single = wide_single ? 1 : 0;
        A.wide_compact = wide && c->meta.wide_compact ? 1 : 0;  // the record format (host), not a choice
        const char* nb = hook_env("PT_WIDE_NB");  // test hook: 0 = tri_hit in the wide drains
        A.tri_fast = wide && c->meta.coords_small && !(nb && *nb == '0') ? 1 : 0;
        const char* wq = hook_env("PT_WIDE_QUEUE_CAP");  // test hook: a smaller queue forces drains and the fallback
        if (wide && wq && *wq) A.wide_queue = std::max(1, std::min(A.wide_queue, atoi(wq)));
        // camera rays generated once this many lanes want one: 32, 40 in scenes with a
        // SPECULAR material (config 3: +0.6 %, Cornell flat at 32-40; profiles/r04_knobs)
        const char* rt = hook_env("PT_REGEN_THRESH");
        A.regen_thresh = (rt && *rt) ? std::max(1, std::min(64, atoi(rt))) : (c->has_specular ? 40 : 32);
    }

    // Fused accumulation (fused_accumulate_chunk, pt_trace.h): with more than one launch,
    // launch b also sums batch b-1's slab into the running sum, so only the last batch
    // needs pt_accumulate_kernel between trace launches. Two slabs alternate; an automatic
    // batch is halved so both fit the budget of one. PT_FUSED_ACC=0 (test hook): the
    // separate pass after every launch.
    const char* fa = hook_env("PT_FUSED_ACC");
    bool fused = (spp - s_lo) > batch && !(fa && *fa == '0');
    if (fused && prm->batch_spp <= 0 && !halved) batch = std::max(1, (batch + 1) / 2);
    // an explicit batch keeps its size: fusion (two slabs) only when both fit the budget
    if (fused && prm->batch_spp > 0 && 2 * 3 * sizeof(float) * (size_t)batch * npix > batch_bytes_budget(c->device, compile_pending))
        fused = false;
    const size_t slab_floats = 3 * (size_t)batch * npix;
    // Tail batch (fused): the last batch is summed by pt_accumulate_kernel after the last
    // launch, on the stream's critical path, so it is made small: the samples left after the
    // full batches end in (left - tail, tail) with tail = batch / PT_TAIL_DIV (tuning hook,
    // 0 = off: the last batch is the remainder).
    const char* td = hook_env("PT_TAIL_DIV");
    const int tail_div = (td && *td) ? std::max(0, atoi(td)) : kTailDiv;
    const int tail = fused && tail_div > 0 ? std::max(1, batch / tail_div) : 0;
    auto batch_at = [&](int s0) {
        const int left = spp - s0;
        if (tail <= 0 || left <= tail) return std::min(batch, left);
        return left <= batch + tail ? left - tail : batch;
    };
    if ((rc = ensure(&c->d_radiance, &c->radiance_floats, (fused ? 2 : 1) * slab_floats))) return rc;
    // Flagged slabs (TraceArgs::flags) in dark scenes: a path that ends at +0 (98 % of them in
    // every BASELINE scene, §3.9) stores nothing, the others store their record and set its
    // bit, and the accumulation reads the bits and only the flagged records. The sums are the
    // dense slab's (an unflagged record is +0; adding +0 changes no running sum). Each slab's
    // bits are cleared before the launch that fills it. PT_FLAGS=0 (test hook): dense slabs.
    const char* fl_env = hook_env("PT_FLAGS");
    const bool flagged = c->dark && !(fl_env && *fl_env == '0');
    // Bit layout (TraceArgs::flags_pm): pixel-major words (one load per 32 samples of a pixel)
    // for frames of several launches, whose slabs the trace kernels sum (fused accumulation):
    // headline whole job +0.7 %, config 5 +0.6 %; sample-major (round 5) for one-launch frames
    // (an 8-GPU share), whose trace kernel measured 1 % slower with the other layout
    // (profiles/r06_flags). PT_FLAGS_PM=0 / 1 (test hook) forces one.
    const char* pm_env = hook_env("PT_FLAGS_PM");
    const int flags_pm = (pm_env && *pm_env) ? (*pm_env == '1' ? 1 : 0) : (fused ? 1 : 0);
    const size_t slab_words = flags_pm ? ((size_t)batch + 31) / 32 * npix : ((size_t)batch * npix + 31) / 32;
    if (flagged) {
        const size_t words = (fused ? 2 : 1) * slab_words;
        if (c->flags_words < words || !c->d_flags) {
            if (c->d_flags) (void)hipFree(c->d_flags);
            c->d_flags = nullptr;
            c->flags_words = 0;
            HIP_TRY(hipMalloc((void**)&c->d_flags, std::max<size_t>(words, 1) * sizeof(uint32_t)));
            c->flags_words = words;
        }
    }
    auto flags_at = [&](int b) -> uint32_t* {  // batch b's bits (the slab it writes)
        return flagged ? c->d_flags + (fused ? (size_t)(b & 1) * slab_words : 0) : nullptr;
    };
    A.acc_chunks = 0;

    HIP_TRY(hipMemsetAsync(c->d_ctr, 0, 4 * sizeof(unsigned long long), c->stream));
#ifdef PT_STAMPS
    if (!c->d_stamps) HIP_TRY(hipMalloc((void**)&c->d_stamps, kStampSections * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->d_stamps, 0, kStampSections * sizeof(unsigned long long), c->stream));
    A.stamps = c->d_stamps;
#endif
    std::vector<hipEvent_t> ev;
    auto cleanup = [&]() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    };
    int launches = 0;
    const int acc_grid = (npix + kBlock - 1) / kBlock;
    if (s_lo == spp || npix == 0) {
        if (npix > 0) {
            // No samples: the reference divides the zero image by 0 (render.h:97).
            hipLaunchKernelGGL(pt_accumulate_kernel, dim3(acc_grid), dim3(kBlock), 0, c->stream, c->d_radiance,
                               c->d_accum, dst, npix, 0, s_lo == 0 ? 1 : 0, 1, keep, (float)spp, nullptr, 0);
        }
    }
    int prev_s0 = -1, prev_sc = 0;
    std::vector<int> launch_sc;  // samples of each launch (progress)
    for (int s0 = s_lo, b = 0, sc = 0; s0 < spp && npix > 0; s0 += sc, b++) {
        sc = batch_at(s0);
        launch_sc.push_back(sc);
        A.s_begin = s0;
        A.s_count = sc;
        float* slab = c->d_radiance + (fused ? (size_t)(b & 1) * slab_floats : 0);
        A.radiance = slab;
        A.flags = flags_at(b);
        // cleared after the launch that last read these bits (stream order)
        A.flags_pm = flags_pm;
        const size_t words_b = flags_pm ? ((size_t)sc + 31) / 32 * npix : ((size_t)sc * npix + 31) / 32;
        if (A.flags && hipMemsetAsync(A.flags, 0, words_b * sizeof(uint32_t), c->stream) != hipSuccess) {
            cleanup();
            return set_error(PT_E_HIP, "hipMemsetAsync of the slab flags failed");
        }
        const unsigned long long blocks_of_samples = (unsigned long long)((sc + per_item - 1) / per_item);
        A.total_items = blocks_of_samples * (unsigned long long)npix;
        if (A.total_items >= (1ull << 31)) {
            cleanup();
            return set_error(PT_E_ARG, "batch of %d samples x %d pixels exceeds 2^31 work items", sc, npix);
        }
        if (flat && !use_rtc && c->rtc_job.valid() && b >= 1) {
            // switch to the hipRTC kernel once its compile is done. While it is pending no
            // launch is queued ahead: launch b is enqueued when b-1's trace kernel has finished,
            // so the switch comes at the first launch boundary after the compile instead of one
            // launch later (round 6: cold headline end to end 0.627 -> 0.618-0.621 s, the device
            // idle only for the host's enqueue between two launches; profiles/r06_cold)
            (void)hipEventSynchronize(ev[3 * (size_t)(b - 1) + 1]);
            rtc_resolve(c, b == rtc_switch_at);  // test hook: the switch forced at launch b
            if (c->rtc_flat) {
                int rb = 0;
                if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&rb, c->rtc_flat, kBlock, lds_bytes) != hipSuccess) {
                    cleanup();
                    return set_error(PT_E_HIP, "hipModuleOccupancyMaxActiveBlocksPerMultiprocessor failed");
                }
                if (lds_bytes > 0 && c->lds_usable > 0)
                    rb = std::min<int>(rb, (int)(c->lds_usable / ((lds_bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule)));
                blocks_per_cu = std::min(std::max(1, rb), 8);
                use_rtc = true;
            }
        }
        const unsigned long long want_blocks = (A.total_items + kBlock - 1) / kBlock;
        const int grid = (int)std::min<unsigned long long>(want_blocks, (unsigned long long)blocks_per_cu * c->num_cus);
        // Refill size: kChunk, or less when the launch holds too few items for every wave
        // to get ~128 refills, so that the launch's drain (waves finishing their last pool)
        // stays short: config 4's 8-GPU share (131k pixels x 1000 spp, 166-item refills)
        // 1.047 / 1.044 of ideal at ~4 refills, 1.036 / 1.031 at 64, then with the scaled step
        // bar 1.026-1.028 at 64 and 1.023-1.024 at 128; whole frames unchanged (their refills
        // stay at kChunk; profiles/r06_pool). At least 64: one refill must cover a whole wave's
        // claims (claim_work). Smaller refills only at the end of a launch (a second counter)
        // measured slower: the waves then contend on it (profiles/r06_drain/pool_tail_rejected.json).
        unsigned long long max_chunk = kChunk, refills = 128;
        if (const char* pc = hook_env("PT_POOL_CHUNK"))  // tuning hook: the refill size's upper bound
            if (*pc) max_chunk = std::max<unsigned long long>(kWave, std::min<unsigned long long>(kChunk, strtoull(pc, nullptr, 10)));
        if (const char* pr = hook_env("PT_POOL_REFILLS"))  // tuning hook: refills per wave the size aims at
            if (*pr) refills = std::max<unsigned long long>(1, std::min<unsigned long long>(1024, strtoull(pr, nullptr, 10)));
        // ... but never below the size that keeps the refill atomics (one counter, all waves)
        // near the rate of full-size refills on the wide walk: a flat kernel's lane finishes a
        // sample in ~26 us at full speed, so 64-item refills would be ~300 M atomics per second
        // on one address (a 40-spp headline frame measured 4x slower, tests/test_bench_gpu.py);
        // 512 items there, 128 on the wide walk (~70 us per sample: ~35 M/s at 166 items).
        const unsigned long long floor_chunk = std::min<unsigned long long>(max_chunk, flat ? 512 : 128);
        A.chunk = (int)std::max<unsigned long long>(
            kWave, std::min<unsigned long long>(
                       max_chunk, std::max<unsigned long long>(
                                      floor_chunk, A.total_items / ((unsigned long long)grid * (kBlock / kWave) * refills))));
        // Static start: each wave's first pool needs no atomic. Large launches: one refill's
        // worth (the claims then stay in order, so the waves of a CU trace neighbouring
        // items); small ones (an even share under 4 kChunk items): the whole even share,
        // the remainder (< one item per wave) claimed in refills. Config 1's kernel: 0.39
        // (mode 0) -> 0.30 (mode 1) -> 0.19 ms (mode 2); configs 2 and 4 unchanged (+0.1 %).
        // Tuning hooks: PT_STATIC_MODE 0 off, 1 one refill always, 2 (default) as above;
        // PT_STATIC_FRAC the small-launch share (0.9: 0.21 ms, 0.75: 0.24 ms).
        {
            const unsigned long long waves = (unsigned long long)grid * (kBlock / kWave);
            const unsigned long long share = A.total_items / waves;
            const char* sm = hook_env("PT_STATIC_MODE");
            const char* sf = hook_env("PT_STATIC_FRAC");
            const int mode = (sm && *sm) ? atoi(sm) : 2;
            const double frac = (sf && *sf) ? std::max(0.0, std::min(1.0, atof(sf))) : 1.0;
            unsigned long long st = std::min<unsigned long long>((unsigned long long)A.chunk, share);
            if (mode == 2 && share < 4ull * kChunk) st = std::max(st, (unsigned long long)((double)share * frac));
            if (mode == 0) st = 0;
            A.static_items = (uint32_t)st;
            A.static_base = waves * st;  // <= total_items < 2^31
        }
        hipEvent_t e0, e1, e2;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess ||
            hipEventCreate(&e2) != hipSuccess) {
            cleanup();
            return set_error(PT_E_HIP, "hipEventCreate failed");
        }
        ev.push_back(e0);
        ev.push_back(e1);
        ev.push_back(e2);
        (void)hipMemsetAsync(c->d_ctr, 0, sizeof(unsigned long long), c->stream);  // work head only
        if (fused && prev_s0 >= 0) {  // this launch also sums the previous batch's slab
            A.acc_src = c->d_radiance + (size_t)((b - 1) & 1) * slab_floats;
            A.acc_flags = flags_at(b - 1);
            A.acc_sum = c->d_accum;
            A.acc_count = prev_sc;
            A.acc_first = prev_s0 == 0 ? 1 : 0;
            A.acc_chunks = (npix + kWave - 1) / kWave;
            // a chunk every acc_every-th refill of a wave: about half of them are done
            // spread over the launch's first half, the rest by waves out of trace work
            const unsigned long long refills =
                std::max<unsigned long long>(1, (A.total_items - A.static_base) / (unsigned long long)A.chunk);
            const char* ad = hook_env("PT_ACC_DIV");  // tuning hook: chunks spread over 1/div of the refills
            const unsigned long long div = (ad && *ad) ? std::max(1, atoi(ad)) : 2;
            A.acc_every = (int)std::max<unsigned long long>(1, refills / (div * (unsigned long long)A.acc_chunks));
            (void)hipMemsetAsync(c->d_ctr + 2, 0, sizeof(unsigned long long), c->stream);  // chunk head
        } else {
            A.acc_chunks = 0;
            A.acc_flags = nullptr;
        }
        (void)hipEventRecord(e0, c->stream);
        if (use_rtc) {
            size_t arg_bytes = sizeof(A);
            void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &A, HIP_LAUNCH_PARAM_BUFFER_SIZE, &arg_bytes,
                           HIP_LAUNCH_PARAM_END};
            const hipError_t le2 = hipModuleLaunchKernel(c->rtc_flat, grid, 1, 1, kBlock, 1, 1, (unsigned)lds_bytes,
                                                         c->stream, nullptr, cfg);
            if (le2 != hipSuccess) {
                cleanup();
                return set_error(PT_E_HIP, "hipModuleLaunchKernel failed: %s", hipGetErrorString(le2));
            }
        } else {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds_bytes, c->stream, A);
        }
        (void)hipEventRecord(e1, c->stream);
        if (!fused || s0 + sc >= spp)  // fused: only the last batch (the others are summed by the next launch)
            hipLaunchKernelGGL(pt_accumulate_kernel, dim3(acc_grid), dim3(kBlock), 0, c->stream, slab, c->d_accum, dst,
                               npix, sc, s0 == 0 ? 1 : 0, s0 + sc >= spp ? 1 : 0, keep, (float)spp, A.flags,
                               flags_pm);
        (void)hipEventRecord(e2, c->stream);
        prev_s0 = s0;
        prev_sc = sc;
        launches++;
    }
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
        cleanup();
        return set_error(PT_E_HIP, "kernel launch failed: %s", hipGetErrorString(le));
    }
    if (prm->progress && npix > 0) {
        // progress as each launch's samples are summed (the reference prints per row or
        // per tile, render.h:87, 136); the launches are already queued, so waiting here
        // costs the device nothing
        // A launch that failed ends the reports there: render_range returns its error
        // below, and no line claims rows that were not rendered.
        const int64_t total = (int64_t)(spp - s_lo) * npix;
        int64_t done = 0;
        hipError_t pe = hipSuccess;
        for (int b = 0; b < launches; b++) {
            if ((pe = hipEventSynchronize(ev[3 * (size_t)b + 2])) != hipSuccess) break;
            done += (int64_t)launch_sc[(size_t)b] * npix;
            prm->progress(prm->progress_user, done, total);
        }
        if (pe != hipSuccess) {
            cleanup();
            return set_error(PT_E_HIP, "render failed: %s", hipGetErrorString(pe));
        }
        if (launches == 0) prm->progress(prm->progress_user, total, total);
    }
    unsigned long long h_ctr[4] = {0, 0, 0, 0};
    hipError_t e = hipMemcpyAsync(h_ctr, c->d_ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && !out_is_device)
        e = hipMemcpyAsync(out, dst, 3 * (size_t)npix * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        cleanup();
        return set_error(PT_E_HIP, "render failed: %s", hipGetErrorString(e));
    }
#ifdef PT_STAMPS
    {
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
                fprintf(stderr, "[stamps] per flat wave-iteration: pairs %.1f, pair rounds %.2f, max pairs of a lane %.2f\n",
                    hs[8] / it, hs[9] / it, hs[10] / it);
        }
    }
#endif
    double kms = 0, rms = 0;
    for (size_t i = 0; i + 2 < ev.size(); i += 3) {
        float a = 0, b = 0;
        (void)hipEventElapsedTime(&a, ev[i], ev[i + 1]);
        (void)hipEventElapsedTime(&b, ev[i + 1], ev[i + 2]);
        kms += a;
        rms += b;
    }
    cleanup();
    if (stats) {
        stats->rays = h_ctr[1];
        stats->paths = (uint64_t)(spp - s_lo) * (uint64_t)npix;
        stats->runaway = h_ctr[3];
        stats->kernel_ms = kms;
        stats->reduce_ms = rms;
        stats->trace_launches = launches;
        stats->rows = rows;
        stats->kernel_path = use_rtc     ? PT_PATH_FLAT_RTC
                             : flat && c->flat_fast ? PT_PATH_FLAT_TABLE_FAST
                             : flat      ? PT_PATH_FLAT_TABLE
                             : wide      ? PT_PATH_WIDE
                             : lds_scene ? PT_PATH_TREE_LDS : PT_PATH_TREE_GLOBAL;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    if (h_ctr[3] != 0)
        return set_error(PT_E_RUNAWAY, "%llu specular rejection loops hit the %d-iteration bound", h_ctr[3],
                         kMaxSpecularIters);
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
    if (s_first > 0) {
        const bool same = c->prog_valid && c->prog_spp == s_first && memcmp(&c->prog_cam, cam, sizeof(pt_camera)) == 0 &&
                          c->prog_prm.depth == prm->depth && c->prog_prm.seed == prm->seed &&
                          c->prog_prm.part_index == prm->part_index && c->prog_prm.part_count == prm->part_count &&
                          c->prog_prm.band_rows == prm->band_rows;
        if (!same)
            return set_error(PT_E_ARG,
                             "progressive render: samples from %d do not continue this context's running sum "
                             "(%d samples, or another camera / parameters)",
                             s_first, c->prog_valid ? c->prog_spp : 0);
    }
    c->prog_valid = false;
    const int rc = render_range(c, cam, prm, s_first, s_first + s_count, 1, out, out_is_device, stats);
    if (rc) return rc;
    c->prog_valid = true;
    c->prog_spp = s_first + s_count;
    c->prog_cam = *cam;
    c->prog_prm = *prm;
    return PT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- ray queries and first-hit AOVs
// Entry points of the kernels in pt_query.hip. They use buffers of their own (d_qstack, d_qbuf,
// d_qhits) and never d_accum, so a progressive sum stays valid across them.
namespace pt {
FastDiv fastdiv_for(uint32_t d) { return make_fastdiv(d); }  // for pt_query.hip's TraceArgs
}

namespace {

constexpr int64_t kQueryChunk = 1ll << 28;      // rays per launch: 3 * i stays below 2^31 in the kernel
constexpr int64_t kQueryHostChunk = 1ll << 22;  // rays staged at a time for a host-pointer call

QueryScene query_scene(const pt_ctx* c) {
    return QueryScene{reinterpret_cast<const f4*>(c->d_nodes), reinterpret_cast<const f4*>(c->d_tris),
                      reinterpret_cast<const f4*>(c->d_mats), c->d_rank_tri, c->meta.num_nodes, c->meta.num_tris,
                      c->meta.tree_depth};
}

int query_force_exact() {
    const char* fe = hook_env("PT_FORCE_EXACT_SLAB");
    return (fe && (*fe == '1' || *fe == '2')) ? 1 : 0;
}

// The plan's global stack (if any) and the zeroed hit counter.
int query_buffers(pt_ctx* c, const QueryPlan& plan) {
    if (plan.stack_ints > c->qstack_ints) {
        if (c->d_qstack) (void)hipFree(c->d_qstack);
        c->d_qstack = nullptr;
        c->qstack_ints = 0;
        HIP_TRY(hipMalloc((void**)&c->d_qstack, plan.stack_ints * sizeof(int)));
        c->qstack_ints = plan.stack_ints;
    }
    if (!c->d_qhits) HIP_TRY(hipMalloc((void**)&c->d_qhits, sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->d_qhits, 0, sizeof(unsigned long long), c->stream));
    return PT_OK;
}

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

int query_finish(pt_ctx* c, const QueryPlan& plan, uint64_t rays, double kernel_ms, int launches,
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
    QueryPlan plan;
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
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
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
    const int W = cam->res[0], H = cam->res[1];
    if (W <= 0 || H <= 0) return set_error(PT_E_ARG, "camera resolution must be positive");
    const int parts = prm->part_count > 0 ? prm->part_count : 1;
    const int band = prm->band_rows > 0 ? prm->band_rows : 1;
    if (prm->part_index < 0 || prm->part_index >= parts) return set_error(PT_E_ARG, "part_index out of range");
    const int rows = pt_part_rows(H, prm->part_index, parts, band);
    const long long npix = (long long)rows * W;
    if (npix > (1ll << 30)) return set_error(PT_E_ARG, "too many pixels for one part");
    if (npix == 0) return PT_OK;
    if (int rc0 = ctx_ready(c)) return rc0;
    HIP_TRY(hipSetDevice(c->device));
    const QueryScene sc = query_scene(c);
    QueryPlan plan;
    int rc;
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
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipEventRecord(ev.a, c->stream));
    if ((rc = aov_launch(c->stream, sc, plan, cam, prm, rows, sample, &d_out, c->d_qstack, c->d_qhits, query_force_exact())))
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

// trace() (render.h:36-61) along the caller's rays: pt_paths_kernel fills a dense slab
// [sample][ray][rgb] of one launch, pt_accumulate_kernel adds a ray's samples in order and
// divides. Launches are cut over rays only: m rays with m * spp < 2^31 records inside the slab
// budget (PT_TRACE_CHUNK, test hook: rays per launch).
int pt_ctx_trace(pt_ctx* c, const float* origins, const float* dirs, int64_t n, const pt_trace_params* prm,
                 float* rgb_out, int is_device, pt_trace_stats* stats) {
    const auto t_start = std::chrono::steady_clock::now();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return set_error(PT_E_ARG, "pt_ctx_trace: context is NULL");
    if (!prm) return set_error(PT_E_ARG, "pt_ctx_trace: params is NULL");
    if (n < 0) return set_error(PT_E_ARG, "pt_ctx_trace: n = %lld is negative", (long long)n);
    if (prm->depth < 0 || prm->depth > PT_MAX_DEPTH)
        return set_error(PT_E_ARG, "pt_ctx_trace: depth %d outside 0..%d", prm->depth, PT_MAX_DEPTH);
    if (prm->spp < 1 || prm->spp > kTraceMaxSpp)
        return set_error(PT_E_ARG, "pt_ctx_trace: spp %d outside 1..%d", prm->spp, kTraceMaxSpp);
    if (!c->have_scene) return set_error(PT_E_ARG, "pt_ctx_trace: no scene set");
    if (n == 0) return PT_OK;
    if (!origins || !dirs || !rgb_out) return set_error(PT_E_ARG, "pt_ctx_trace: NULL argument");
    if (int rc0 = ctx_ready(c)) return rc0;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t spp = prm->spp;
    auto finish = [&](const PathsPlan* plan, const unsigned long long* ctr, double kms, double rms, int launches) {
        if (!stats) return;
        stats->rays = ctr[1];
        stats->paths = (uint64_t)n * (uint64_t)spp;
        stats->runaway = ctr[3];
        stats->kernel_ms = kms;
        stats->reduce_ms = rms;
        stats->launches = launches;
        if (plan) {
            stats->lds_scene = plan->lds_scene;
            stats->lds_stack = plan->lds_stack;
            stats->lds_records = plan->lds_rec;
        }
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    };
    if (prm->depth == 0) {  // trace() returns 0 (render.h:37): no ray is traced
        if (is_device) {
            HIP_TRY(hipMemsetAsync(rgb_out, 0, 3 * sizeof(float) * (size_t)n, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        } else {
            memset(rgb_out, 0, 3 * sizeof(float) * (size_t)n);
        }
        const unsigned long long zero[4] = {0, 0, 0, 0};
        finish(nullptr, zero, 0, 0, 0);
        return PT_OK;
    }
    // rays per launch
    int64_t m_max = std::min<int64_t>(n, ((1ll << 31) - 1) / spp);
    m_max = std::min<int64_t>(m_max, (int64_t)(batch_bytes_budget(c->device, false) / (3 * sizeof(float) * (size_t)spp)));
    if (!is_device) m_max = std::min(m_max, kQueryHostChunk);
    if (const char* tc = hook_env("PT_TRACE_CHUNK"))
        if (*tc) m_max = std::min<int64_t>(m_max, strtoll(tc, nullptr, 10));
    m_max = std::max<int64_t>(m_max, 1);
    const QueryScene sc = query_scene(c);
    PathsPlan plan;
    int rc;
    if ((rc = paths_plan(sc, c->lds_usable, c->num_cus, prm->depth, m_max * spp, plan))) return rc;
    if (plan.stack_ints > c->qstack_ints) {
        if (c->d_qstack) (void)hipFree(c->d_qstack);
        c->d_qstack = nullptr;
        c->qstack_ints = 0;
        HIP_TRY(hipMalloc((void**)&c->d_qstack, plan.stack_ints * sizeof(int)));
        c->qstack_ints = plan.stack_ints;
    }
    if (plan.rec_words > 0 && (rc = ensure(&c->d_trec, &c->trec_words, 2 * plan.rec_words))) return rc;
    if ((rc = ensure(&c->d_tslab, &c->tslab_floats, 3 * (size_t)(m_max * spp)))) return rc;
    if (!c->d_tctr) HIP_TRY(hipMalloc((void**)&c->d_tctr, 4 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->d_tctr, 0, 4 * sizeof(unsigned long long), c->stream));
    // host pointers: staging [origins 3][dirs 3][rgb 3] x m_max, and the states
    float *s_org = nullptr, *s_dir = nullptr, *s_out = nullptr;
    if (!is_device) {
        if ((rc = ensure(&c->d_tbuf, &c->tbuf_floats, 9 * (size_t)m_max))) return rc;
        s_org = c->d_tbuf;
        s_dir = s_org + 3 * m_max;
        s_out = s_dir + 3 * m_max;
        if (prm->states && (rc = ensure(&c->d_tstates, &c->tstates_words, (size_t)(m_max * spp)))) return rc;
    }
    PathsLaunch l{};
    l.spp = (int32_t)spp;
    l.depth = prm->depth;
    l.seed = prm->seed;
    l.slab = c->d_tslab;
    l.ctr = c->d_tctr;
    l.gstack = c->d_qstack;
    l.grec = plan.rec_words > 0 ? c->d_trec : nullptr;
    l.dark = c->dark ? 1 : 0;
    l.force_exact = query_force_exact();
#if PT_THETA_TAB
    {
        // as pt_ctx_render: the theta table only for scenes with a SPECULAR material
        const char* tl = hook_env("PT_THETA_LANES");
        l.theta_lanes = (tl && *tl) ? atoi(tl) : (c->has_specular ? 32 : 0);
        if (PT_THETA_TAB == 1 || l.theta_lanes > 0) {
            const float2* tab = nullptr;
            if ((rc = theta_table(c, &tab))) {
                if (PT_THETA_TAB == 1) return rc;
                tab = nullptr;  // the computed hemisphere_dir gives the same bits
            }
            l.theta_tab = tab;
        }
    }
#endif
    EventPair ev, ev2;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipEventCreate(&ev2.a));
    double kernel_ms = 0, reduce_ms = 0;
    int launches = 0;
    for (int64_t i0 = 0; i0 < n; i0 += m_max) {
        const int32_t m = (int32_t)std::min(m_max, n - i0);
        l.m = m;
        l.ray_base = (uint32_t)i0;
        l.org = origins + 3 * i0;
        l.dir = dirs + 3 * i0;
        l.states = prm->states ? prm->states + i0 * spp : nullptr;
        float* k_out = rgb_out + 3 * i0;
        if (!is_device) {
            HIP_TRY(hipMemcpyAsync(s_org, l.org, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpyAsync(s_dir, l.dir, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            if (prm->states) {
                HIP_TRY(hipMemcpyAsync(c->d_tstates, l.states, sizeof(uint32_t) * (size_t)(m * spp), hipMemcpyHostToDevice,
                                       c->stream));
                l.states = reinterpret_cast<const uint32_t*>(c->d_tstates);
            }
            l.org = s_org;
            l.dir = s_dir;
            k_out = s_out;
        }
        HIP_TRY(hipMemsetAsync(c->d_tctr, 0, sizeof(unsigned long long), c->stream));  // work head only
        HIP_TRY(hipEventRecord(ev.a, c->stream));
        if ((rc = paths_launch(c->stream, sc, plan, l))) return rc;
        HIP_TRY(hipEventRecord(ev.b, c->stream));
        // the ray's samples in order from +0, then / spp (image.h:27-31, 37-40)
        hipLaunchKernelGGL(pt_accumulate_kernel, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->d_tslab,
                           (float*)nullptr, k_out, (int)m, (int)spp, 1, 1, 0, (float)spp, (const uint32_t*)nullptr, 0);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev2.a, c->stream));
        launches++;
        if (!is_device)
            HIP_TRY(hipMemcpyAsync(rgb_out + 3 * i0, s_out, 3 * sizeof(float) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        kernel_ms += ms;
        HIP_TRY(hipEventElapsedTime(&ms, ev.b, ev2.a));
        reduce_ms += ms;
    }
    unsigned long long h_ctr[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h_ctr, c->d_tctr, sizeof(h_ctr), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    finish(&plan, h_ctr, kernel_ms, reduce_ms, launches);
    if (h_ctr[3] != 0)
        return set_error(PT_E_RUNAWAY, "%llu specular rejection loops hit the %d-iteration bound", h_ctr[3],
                         kMaxSpecularIters);
    return PT_OK;
}

}  // extern "C"

void* pt::ctx_stream(pt_ctx* c) { return c && ctx_ready(c) == PT_OK ? (void*)c->stream : nullptr; }

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
    const int W = cam->res[0], H = cam->res[1];
    if (W <= 0 || H <= 0) return set_error(PT_E_ARG, "camera resolution must be positive");
    const int parts = prm->part_count > 0 ? prm->part_count : 1, band = prm->band_rows > 0 ? prm->band_rows : 1;
    if (prm->part_index < 0 || prm->part_index >= parts) return set_error(PT_E_ARG, "part_index out of range");
    const int rows = pt_part_rows(H, prm->part_index, parts, band);
    const size_t n = (size_t)rows * W * 3;
    int rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure(&c->d_out, &c->out_floats, n))) return rc;
    c->prog_valid = false;
    if ((rc = render_range(c, cam, prm, 0, prm->spp > 0 ? prm->spp : 0, 0, c->d_out, 1, stats))) return rc;
    uint8_t* dst = out;
    if (!out_is_device) {
        if (c->rgb8_bytes < n || !c->d_rgb8) {
            if (c->d_rgb8) (void)hipFree(c->d_rgb8);
            c->d_rgb8 = nullptr;
            c->rgb8_bytes = 0;
            HIP_TRY(hipMalloc((void**)&c->d_rgb8, std::max<size_t>(n, 1)));
            c->rgb8_bytes = n;
        }
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

// Test hook: generate and compile the scene-specialised flat kernel without a device.
int pt_rtc_check(const pt_scene* scene, char* src_out, size_t cap) {
    PackedScene ps;
    const int rc = pack_scene(scene, ps);
    if (rc) return rc;
    if (!flat_eligible(ps))
        return set_error(PT_E_ARG, "scene has no flat leaf list (%d leaves, %d triangles)", ps.num_leaves, ps.num_tris);
    const std::string src =
        rtc_flat_source(ps.leaves, ps.num_leaves, scene_has_specular(ps), ps.coords_small, albedo_x2_ok(ps), scene_dark(ps));
    if (src_out && cap) {
        const size_t n = std::min(cap - 1, src.size());
        memcpy(src_out, src.data(), n);
        src_out[n] = 0;
    }
    const std::shared_ptr<const RtcCode> code = rtc_job(src).get();
    if (code->code.empty()) return set_error(PT_E_HIP, "%s", code->status.c_str());
    return (int)code->code.size();
}

// Test hook (no device needed): start the scene kernel's compile as pt_ctx_set_scene does (in
// the background) and return at once: 1 if a compile is running, 0 if the job was already
// done (a disk-cache hit or an earlier compile).
int pt_debug_rtc_start(const pt_scene* scene) {
    PackedScene ps;
    const int rc = pack_scene(scene, ps);
    if (rc) return rc;
    if (!flat_eligible(ps))
        return set_error(PT_E_ARG, "scene has no flat leaf list (%d leaves, %d triangles)", ps.num_leaves, ps.num_tris);
    const RtcFuture f = rtc_job(
        rtc_flat_source(ps.leaves, ps.num_leaves, scene_has_specular(ps), ps.coords_small, albedo_x2_ok(ps), scene_dark(ps)));
    return f.wait_for(std::chrono::seconds(0)) == std::future_status::ready ? 0 : 1;
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

// Test hook (no device needed): the dark-path gate (scene_dark) on a scene.
int pt_debug_scene_dark(const pt_scene* scene) {
    PackedScene ps;
    const int rc = pack_scene(scene, ps);
    if (rc) return rc;
    return scene_dark(ps) ? 1 : 0;
}

// Test hook (no device needed): the hipRTC code-object caches. op 0 forgets this process's
// compiles and loaded scene kernels (later requests go to the disk cache or compile again;
// contexts keep the kernels they hold), 1 / 2 / 3 return the disk-cache hits, the rejected
// (corrupt or mismatched) entries and the compiles so far.
int64_t pt_debug_rtc_cache(int32_t op) {
    if (op == 0) {
        RtcCache& c = rtc_cache();
        std::lock_guard<std::mutex> lock(c.mu);
        for (auto& kv : c.code) kv.second.wait();
        c.code.clear();
        c.funcs.clear();  // the modules stay loaded (a context may still launch them)
        return 0;
    }
    if (op == 1) return g_rtc_disk_hits.load();
    if (op == 2) return g_rtc_disk_rejects.load();
    if (op == 3) return g_rtc_compiles.load();
    if (op == 4) return g_rtc_last_compile_us.load();
    if (op == 5) return g_rtc_server_compiles.load();
    return set_error(PT_E_ARG, "pt_debug_rtc_cache: bad op %d", op);
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
    if (!mismatches || !first_bad || which < 0 || which > 4 || hi_bits < lo_bits)
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
