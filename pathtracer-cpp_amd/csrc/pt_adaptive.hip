// pt_adaptive.hip — the per-pixel rounds of pt_ctx_render_adaptive (gfx950). The
// host loop is beside pt_ctx_render_converge in pt_kernel.hip; here are its kernels and their
// launches.
//
//   pt_active_list_kernel           the pixels of a list (or of the whole part) that miss the
//                                   criterion of pt_moments.h, compacted into a new list; the
//                                   others leave with their sample count written to spp
//   pt_adaptive_kernel<...>         paths_body (pt_paths.h) fed with camera_ray of the listed pixels
//   pt_adaptive_accumulate_kernel   a launch's records added to the listed pixels' running sums
//   pt_spp_fill_kernel              spp of the listed pixels (or of every pixel) set to n
//   pt_moments_sem_pp_kernel        pt_moments_sem_kernel with each pixel's own n
//
// A work item of the trace kernel is (listed pixel, sample), numbered sample-major as in
// pt_paths.hip: item j of a launch over m listed pixels -> sample s_begin + j / m of pixel
// list[j % m], and its radiance is record j of the launch's dense slab [sample][listed pixel][rgb].
// A pixel's samples are the render's own (camera_ray seeds with pt_sample_seed at the global pixel
// index) and they are added in sample order, so a pixel that received n samples holds the bits of
// pt_ctx_render at spp = n whatever the order of the list and however a round is cut into launches.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>

#include "pt_moments.h"
#include "pt_paths.h"

namespace pt {

// One lane per entry of `prev` (nullptr: the part's pixels 0..m-1 themselves). A wave votes by
// ballot, reserves its slots with one atomic and places its unconverged pixels by their rank among
// the voters, so the list's order is that of the waves' reservations (unspecified). A pixel that
// meets the criterion leaves: spp[q] = n. `list` holds m entries and is not `prev`.
__global__ __launch_bounds__(kBlock) void pt_active_list_kernel(const int32_t* __restrict__ prev, int m,
                                                                const double* __restrict__ mom, int npix, int n,
                                                                double rel, double abs_tol, int32_t* __restrict__ list,
                                                                unsigned long long* __restrict__ count,
                                                                int32_t* __restrict__ spp) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int q = 0;
    bool un = false;
    if (i < m) {
        q = prev ? prev[i] : i;
        const double* S = mom + 3 * (size_t)q;
        un = moments_pixel_unconverged(S, S + 3 * (size_t)npix, n, rel, abs_tol);
        if (!un) spp[q] = n;
    }
    const unsigned long long b = __ballot(un);
    if (b == 0ull) return;  // wave-uniform
    unsigned long long base = 0;
    if ((threadIdx.x & (kWave - 1)) == 0) base = atomicAdd(count, (unsigned long long)__popcll(b));
    const uint32_t first = __builtin_amdgcn_readfirstlane((uint32_t)base);  // count <= m <= 2^30
    if (un) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        list[first + rank] = q;  // first + rank < the final count <= m
    }
}

__global__ __launch_bounds__(kBlock) void pt_spp_fill_kernel(const int32_t* __restrict__ list, int m, int n,
                                                             int32_t* __restrict__ spp) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < m) spp[list ? list[i] : i] = n;
}

// The loop (paths_body, pt_paths.h) over the camera rays of the listed pixels.
template <bool kLdsScene, bool kLdsStack, bool kLdsRec>
__global__ __launch_bounds__(kBlock) void pt_adaptive_kernel(TraceArgs A, PathArgs P) {
    paths_body<ListRays, kLdsScene, kLdsStack, kLdsRec>(A, P);
}

// One lane per listed pixel: its float32 sum (accum, planes of npix) and its six doubles (mom, the
// layout of pt_accumulate_moments_kernel) continued with the launch's c records of that pixel in
// sample order (the dense slab_walk with MomentSums: the order is stated there). n_new > 0 (the
// launch holds the round's last samples of these pixels): out[q] = sum / n_new.
__global__ __launch_bounds__(kBlock) void pt_adaptive_accumulate_kernel(const float* __restrict__ slab,
                                                                        const int32_t* __restrict__ list, int m, int c,
                                                                        float* __restrict__ accum,
                                                                        double* __restrict__ mom,
                                                                        float* __restrict__ out, int npix, int n_new) {
    const int a = blockIdx.x * kBlock + threadIdx.x;
    if (a >= m) return;
    const int q = list[a];
    float x = accum[q];
    float y = accum[npix + q];
    float z = accum[2 * (size_t)npix + q];
    double* S = mom + 3 * (size_t)q;
    double* Q = S + 3 * (size_t)npix;
    MomentSums s{x, y, z, S[0], S[1], S[2], Q[0], Q[1], Q[2]};
    slab_walk<true>(slab, nullptr, 0, c, (uint32_t)a, (uint32_t)m, s);
    if (n_new > 0) {
        const float spp = (float)n_new;
        out[3 * (size_t)q] = x / spp;
        out[3 * (size_t)q + 1] = y / spp;
        out[3 * (size_t)q + 2] = z / spp;
    }
    accum[q] = x;
    accum[npix + q] = y;
    accum[2 * (size_t)npix + q] = z;
    S[0] = s.sx;
    S[1] = s.sy;
    S[2] = s.sz;
    Q[0] = s.qx;
    Q[1] = s.qy;
    Q[2] = s.qz;
}

// pt_moments_sem_kernel (pt_kernel.hip) with n = the pixel's own sample count (one thread per
// pixel and channel).
__global__ __launch_bounds__(kBlock) void pt_moments_sem_pp_kernel(const double* __restrict__ mom, size_t nval,
                                                                   const int32_t* __restrict__ spp,
                                                                   float* __restrict__ sem) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nval) return;
    const int n = spp[i / 3];
    if (n < 2) {
        sem[i] = __builtin_inff();
        return;
    }
    const double S = mom[i], Q = mom[nval + i], dn = (double)n;
    double var = (Q - S * S / dn) / (dn - 1.0);
    if (var < 0.0) var = 0.0;
    sem[i] = (float)sqrt(var / dn);
}

namespace {

using PathsKernel = void (*)(TraceArgs, PathArgs);

template <bool kLdsScene, bool kLdsStack>
PathsKernel adaptive_kernel_t(bool lds_rec) {
    return lds_rec ? pt_adaptive_kernel<kLdsScene, kLdsStack, true> : pt_adaptive_kernel<kLdsScene, kLdsStack, false>;
}
PathsKernel adaptive_kernel(bool lds_scene, bool lds_stack, bool lds_rec) {
    return lds_scene ? (lds_stack ? adaptive_kernel_t<true, true>(lds_rec) : adaptive_kernel_t<true, false>(lds_rec))
                     : (lds_stack ? adaptive_kernel_t<false, true>(lds_rec) : adaptive_kernel_t<false, false>(lds_rec));
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PT_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    return PT_OK;
}

unsigned blocks_for(int32_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

// Placement and grid as paths_plan (pt_paths.hip), for the kernel of this file.
int adaptive_plan(const QueryScene& sc, size_t lds_usable, int num_cus, int depth, int64_t items, WalkPlan& plan) {
    place_walk_hooked(sc.num_nodes, sc.num_tris, sc.tree_depth, 5, std::max(0, depth - 1), lds_usable, true, plan);
    return walk_grid((const void*)adaptive_kernel(plan.lds_scene, plan.lds_stack, plan.lds_rec), lds_usable, num_cus, items,
                     plan, "adaptive render");
}

int adaptive_launch(void* stream, const QueryScene& sc, const WalkPlan& plan, const PathsLaunch& l, const int32_t* list,
                    int32_t s_begin, const pt_camera* cam, const pt_params* prm, const PartShape& shape) {
    const unsigned long long total = (unsigned long long)l.m * (unsigned long long)l.spp;
    if (l.m <= 0 || l.spp <= 0 || l.depth <= 0 || total >= (1ull << 31) || l.m > shape.npix || s_begin < 0)
        return set_error(PT_E_ARG, "adaptive launch of %d pixels x %d samples from %d, depth %d", l.m, l.spp, s_begin,
                         l.depth);
    const int grid = (int)std::min<unsigned long long>((unsigned long long)plan.grid, (total + kBlock - 1) / kBlock);
    TraceArgs A;
    PathArgs P;
    paths_args(sc, plan, l, grid, A, P);
    // the fields camera_ray and part_row read, as the AOV path (pt_query.hip) fills them; the
    // items stay numbered over the launch's m listed pixels
    fill_camera(A, cam, shape, prm);
    A.npix = l.m;
    A.div_npix = make_fastdiv((uint32_t)l.m);
    A.s_begin = s_begin;
    P.list = list;
    hipLaunchKernelGGL(adaptive_kernel(plan.lds_scene, plan.lds_stack, plan.lds_rec), dim3(grid), dim3(kBlock),
                       plan.lds_bytes, (hipStream_t)stream, A, P);
    return launched("adaptive trace");
}

int adaptive_compact(void* stream, const int32_t* prev, int32_t m, const double* mom, int32_t npix, int32_t n, float rel,
                     float abs_tol, int32_t* list, unsigned long long* count, int32_t* spp) {
    if (m <= 0 || m > npix || prev == list) return set_error(PT_E_ARG, "adaptive list of %d of %d pixels", m, npix);
    if (hipMemsetAsync(count, 0, sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess)
        return set_error(PT_E_HIP, "adaptive list: counter reset failed");
    hipLaunchKernelGGL(pt_active_list_kernel, dim3(blocks_for(m)), dim3(kBlock), 0, (hipStream_t)stream, prev, (int)m, mom,
                       (int)npix, (int)n, (double)rel, (double)abs_tol, list, count, spp);
    return launched("adaptive list");
}

int adaptive_fill_spp(void* stream, const int32_t* list, int32_t m, int32_t n, int32_t* spp) {
    if (m <= 0) return PT_OK;
    hipLaunchKernelGGL(pt_spp_fill_kernel, dim3(blocks_for(m)), dim3(kBlock), 0, (hipStream_t)stream, list, (int)m, (int)n,
                       spp);
    return launched("adaptive spp");
}

int adaptive_accumulate(void* stream, const float* slab, const int32_t* list, int32_t m, int32_t c, float* accum,
                        double* mom, float* out, int32_t npix, int32_t n_new) {
    if (m <= 0 || m > npix || c <= 0) return set_error(PT_E_ARG, "adaptive sum of %d of %d pixels x %d samples", m, npix, c);
    hipLaunchKernelGGL(pt_adaptive_accumulate_kernel, dim3(blocks_for(m)), dim3(kBlock), 0, (hipStream_t)stream, slab, list,
                       (int)m, (int)c, accum, mom, out, (int)npix, (int)n_new);
    return launched("adaptive sum");
}

int adaptive_sem(void* stream, const double* mom, size_t nval, const int32_t* spp, float* sem) {
    if (nval == 0) return PT_OK;
    hipLaunchKernelGGL(pt_moments_sem_pp_kernel, dim3((unsigned)((nval + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, mom, nval, spp, sem);
    return launched("adaptive sem");
}

}  // namespace pt
