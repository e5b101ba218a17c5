// pt_grad.hip — material gradients of trace() (render.h:36-61) along a caller's rays, over the
// binary child-pair walk (gfx950). DESIGN.md §3.14; the contract is in include/pt_hip.h.
//
//   pt_grad_kernel<kLdsScene, kLdsStack, kLdsRec, kLdsTab>  pt_paths_kernel's loop (one path per
//       lane: intersect_tree and shade of pt_trace.h, claim_item refills, the slab-form gate on
//       every segment); a path that ends is unwound with L_{k+1} kept per level, stores its
//       radiance record, and then runs the throughput pass T_{k+1} = ((2 T_k) color) c, adding
//       T_k to d emit and ((2 T_k) L_{k+1}) c to d color of bounce k's triangle
//   pt_grad_cam_kernel<...> the same loop fed from the part's own camera rays (PartRays, pt_paths.h):
//       the render gradients of DESIGN.md §3.29, grad_rgb indexed by the part-local pixel
//   pt_grad_gather_kernel   the per-call material array from the scene's and the override rows
//   pt_grad_split_kernel    the table's rows into the caller's grad_color / grad_emit
//
// A path's geometry depends on the normal, the incoming direction and the roughness only, so the
// walk and the samplers are the forward pass's, untouched, and the radiance is a polynomial in
// color and emit_color: no reparameterisation, no bias.
//
// The unwinding always runs (finish_path's dark-path skip is an optimisation proven equal, so the
// forward bits are pt_ctx_trace's with or without it; with it gone the NaN-cosine rule has
// nothing left to guard), and a dark path still carries T_k != 0 into d emit.
//
// Gradient table: 6 doubles per caller triangle {d color rgb, d emit rgb}, rows by
// rank_tri[packed row], so a triangle that sits in several leaves gets one sum. kLdsTab: each
// block adds into a zeroed table of its own in LDS (ds_add_f64) and adds its non-zero entries to
// the global table once, at block end (global_atomic_add_f64); otherwise lanes add to the global
// table directly. Terms that are +-0 are not added (x + (+-0) = x for every x the table can hold:
// it starts at +0 and +0 + (-0) = +0), but they are counted.
//
// LDS: pt_paths_kernel's layout, then [table: 6 x rows doubles (kLdsTab)] at G.tab_off.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "pt_grad.h"
#include "pt_paths.h"

namespace pt {

static_assert(kSpecularIterBound == kMaxSpecularIters, "host and device bound of the specular rejection loop");

namespace grad {

struct GradArgs {
    const float* __restrict__ grad_rgb;   // m x 3, or nullptr: forward only
    double* table;                        // [rows][6], global
    const int* __restrict__ rank_tri;     // packed row -> the caller's triangle
    int table_rows;
    uint32_t tab_off;                     // kLdsTab: byte offset of the block's table in LDS
    float spp_f;                          // (float)spp of the call (a render's launches are cut over samples)
    int want_rgb, want_color, want_emit;
};

}  // namespace grad

using grad::GradArgs;

// `tab` is the block's LDS table or the global one (the kernel's kLdsTab, known at compile time):
// the hardware add of that address space, ds_add_f64 or global_atomic_add_f64.
__device__ __forceinline__ void grad_add(double* __restrict__ tab, int at, float v) {
    if (v == 0.0f) return;  // +-0: leaves every sum as it is
    unsafeAtomicAdd(tab + at, (double)v);
}

__device__ __forceinline__ void grad_add3(double* __restrict__ tab, int row, int part, v3 t) {
    const int at = 6 * row + 3 * part;
    grad_add(tab, at, t.x);
    grad_add(tab, at + 1, t.y);
    grad_add(tab, at + 2, t.z);
}

__device__ __forceinline__ v3 fold_level(float4 m0, float4 m1, float c, v3 L) {  // render.h:60
    return v3{m1.x + ((2.0f * L.x) * m0.y) * c, m1.y + ((2.0f * L.y) * m0.z) * c, m1.z + ((2.0f * L.z) * m0.w) * c};
}
__device__ __forceinline__ v3 color_term(v3 T, v3 below, float c) {
    return v3{((2.0f * T.x) * below.x) * c, ((2.0f * T.y) * below.y) * c, ((2.0f * T.z) * below.z) * c};
}
__device__ __forceinline__ v3 next_throughput(v3 T, float4 m0, float c) {
    return v3{((2.0f * T.x) * m0.y) * c, ((2.0f * T.y) * m0.z) * c, ((2.0f * T.z) * m0.w) * c};
}

// The end of a path of k bounces whose terminal value is L on packed triangle `hit` (-1: a miss).
// Returns the terms it counted.
__device__ __forceinline__ uint32_t grad_finish(const TraceArgs& A, const GradArgs& G, const float4* __restrict__ mats,
                                                const int* __restrict__ rec_tri, const float* __restrict__ rec_cos,
                                                double* __restrict__ tab, int tid, int k, v3 L, int hit, uint32_t at,
                                                uint32_t ray) {
    const bool grads = G.grad_rgb != nullptr;
    v3 T{0.0f, 0.0f, 0.0f};
    if (grads)
        T = v3{G.grad_rgb[3 * (size_t)ray] / G.spp_f, G.grad_rgb[3 * (size_t)ray + 1] / G.spp_f,
               G.grad_rgb[3 * (size_t)ray + 2] / G.spp_f};
    uint32_t terms = 0;
    if (kernarg_args()->rec_size <= 4) {  // uniform: depth <= 5, every level in registers
        int tj[4];
        float cj[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            tj[j] = 0;
            cj[j] = 0.0f;
            if (j < k) {
                tj[j] = rec_tri[j * kBlock + tid];
                cj[j] = rec_cos[j * kBlock + tid];
            }
        }
        float4 m0[4];
        v3 below[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (j < k) m0[j] = mats[2 * tj[j]];
#pragma unroll
        for (int j = 3; j >= 0; j--)
            if (j < k) {
                below[j] = L;
                L = fold_level(m0[j], mats[2 * tj[j] + 1], cj[j], L);
            }
        if (G.want_rgb) *reinterpret_cast<float3*>(A.radiance + 3 * (size_t)at) = make_float3(L.x, L.y, L.z);
        if (grads) {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (j < k) {
                    const int row = G.rank_tri[tj[j]];
                    if (G.want_emit) {
                        grad_add3(tab, row, 1, T);
                        terms++;
                    }
                    if (G.want_color) {
                        grad_add3(tab, row, 0, color_term(T, below[j], cj[j]));
                        terms++;
                    }
                    T = next_throughput(T, m0[j], cj[j]);
                }
        }
    } else {
        // deeper paths: L_{j+1} is unwound again from the records for every level j (no per-level
        // storage: the records hold two words a level, L three)
        const v3 L_end = L;
        for (int j = k - 1; j >= 0; j--) {
            const int t = rec_tri[j * kBlock + tid];
            L = fold_level(mats[2 * t], mats[2 * t + 1], rec_cos[j * kBlock + tid], L);
        }
        if (G.want_rgb) *reinterpret_cast<float3*>(A.radiance + 3 * (size_t)at) = make_float3(L.x, L.y, L.z);
        if (grads) {
            for (int j = 0; j < k; j++) {
                const int t = rec_tri[j * kBlock + tid];
                const float c = rec_cos[j * kBlock + tid];
                const int row = G.rank_tri[t];
                if (G.want_emit) {
                    grad_add3(tab, row, 1, T);
                    terms++;
                }
                if (G.want_color) {
                    v3 below = L_end;
                    for (int i = k - 1; i > j; i--) {
                        const int ti = rec_tri[i * kBlock + tid];
                        below = fold_level(mats[2 * ti], mats[2 * ti + 1], rec_cos[i * kBlock + tid], below);
                    }
                    grad_add3(tab, row, 0, color_term(T, below, c));
                    terms++;
                }
                T = next_throughput(T, mats[2 * t], c);
            }
        }
    }
    if (grads && G.want_emit && hit >= 0) {  // the terminal: an emitter, or a hit on the last allowed segment
        grad_add3(tab, G.rank_tri[hit], 1, T);
        terms++;
    }
    return terms;
}

template <class Rays, bool kLdsScene, bool kLdsStack, bool kLdsRec, bool kLdsTab>
__device__ __forceinline__ void grad_body(const TraceArgs& A, const PathArgs& P, const GradArgs& G) {
    extern __shared__ float4 lds4[];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const float4* __restrict__ nodes = A.nodes;
    const float4* __restrict__ tris = A.tris;
    const float4* __restrict__ mats = A.mats;
    const int scene4 = kLdsScene ? A.num_node4 + A.num_tri4 + A.num_mat4 : 0;
    double* tab = G.table;
    if (kLdsTab) {
        tab = reinterpret_cast<double*>(reinterpret_cast<char*>(lds4) + G.tab_off);
        for (int i = tid; i < 6 * G.table_rows; i += kBlock) tab[i] = 0.0;
    }
    if (kLdsScene) {
        float4* s_nodes = lds4;
        float4* s_tris = lds4 + A.num_node4;
        float4* s_mats = s_tris + A.num_tri4;
        for (int i = tid; i < A.num_node4; i += kBlock) s_nodes[i] = A.nodes[i];
        for (int i = tid; i < A.num_tri4; i += kBlock) s_tris[i] = A.tris[i];
        for (int i = tid; i < A.num_mat4; i += kBlock) s_mats[i] = A.mats[i];
        nodes = s_nodes;
        tris = s_tris;
        mats = s_mats;
    }
    if (kLdsScene || kLdsTab) __syncthreads();
    int* const lds_stk = reinterpret_cast<int*>(lds4 + scene4);
    int* const lds_rec = lds_stk + (kLdsStack ? P.rows * kBlock : 0);
    int* __restrict__ stk = kLdsStack ? lds_stk : P.gstack + (size_t)blockIdx.x * P.rows * kBlock;
    int* __restrict__ rec_tri = kLdsRec ? lds_rec : P.grec_tri + (size_t)blockIdx.x * A.rec_size * kBlock;
    float* __restrict__ rec_cos = kLdsRec ? reinterpret_cast<float*>(lds_rec + A.rec_size * kBlock)
                                          : P.grec_cos + (size_t)blockIdx.x * A.rec_size * kBlock;

    bool alive = true;    // the pool may still hold items for this lane
    bool active = false;  // the lane has a path in flight (item `item`)
    uint32_t item = 0;
    Lcg g{0};
    v3 o{0, 0, 0}, d{0, 0, 1};
    int k = 0;
    unsigned long long n_rays = 0;  // this wave's segments (wave-uniform)
    uint32_t n_terms = 0;           // this lane's terms
    Pool pool = pool_start(A);

    while (true) {
        const bool need = alive && !active;
        if (__any(need)) {
            claim_item(A, lane, need, pool, alive, item);
            if (need && alive) {  // item < total_items = m * spp
                const uint32_t sm = fdiv(item, A.div_npix), i = item - sm * P.m;
                Rays::load(A, P, i, sm, g, o, d);
                k = 0;
                active = true;
            }
        }
        if (!__any(active)) break;

        // ---- BVH::intersect (bvh.h:156-183)
        float t = 0.0f;
        int hit = -1;
        n_rays += (unsigned long long)__popcll(__ballot(active));
        const v3 inv = rcp3_exact(d, active);  // bvh.h:157
        const bool fast = !P.force_exact && __all(!active || query_ray_bounded(o, inv));
        if (active)
            hit = fast ? intersect_tree<true>(nodes, tris, stk, tid, o, d, inv, t)
                       : intersect_tree<false>(nodes, tris, stk, tid, o, d, inv, t);
        bool end = false;
        v3 L{0.0f, 0.0f, 0.0f};
        if (active) end = shade(A, mats, tris, rec_tri, rec_cos, tid, hit, t, g, o, d, k, L);
        if (end) {
            const uint32_t sm = fdiv(item, A.div_npix);
            n_terms += grad_finish(A, G, mats, rec_tri, rec_cos, tab, tid, k, L, hit, item, item - sm * P.m);
            active = false;
        }
    }
    count_rays_wave(A, lane, n_rays);
    {  // the terms: wave reduction, one atomic per wave
        unsigned long long r = n_terms;
        for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off);
        if (lane == 0 && r) atomicAdd(A.ctr + 2, r);
    }
    if (kLdsTab) {
        __syncthreads();
        for (int i = tid; i < 6 * G.table_rows; i += kBlock) {
            const double v = tab[i];
            if (!(v == 0.0)) unsafeAtomicAdd(G.table + i, v);  // a NaN goes through
        }
    }
}

template <bool kLdsScene, bool kLdsStack, bool kLdsRec, bool kLdsTab>
__global__ __launch_bounds__(kBlock) void pt_grad_kernel(TraceArgs A, PathArgs P, GradArgs G) {
    grad_body<BufferRays, kLdsScene, kLdsStack, kLdsRec, kLdsTab>(A, P, G);
}

// The part's own camera rays: item (pixel i, sample A.s_begin + sm), grad_rgb by the part-local pixel.
template <bool kLdsScene, bool kLdsStack, bool kLdsRec, bool kLdsTab>
__global__ __launch_bounds__(kBlock) void pt_grad_cam_kernel(TraceArgs A, PathArgs P, GradArgs G) {
    grad_body<PartRays, kLdsScene, kLdsStack, kLdsRec, kLdsTab>(A, P, G);
}

// out = the scene's materials with color / emit replaced by the caller-ordered override rows
__global__ __launch_bounds__(kBlock) void pt_grad_gather_kernel(const float4* __restrict__ mats,
                                                                const int* __restrict__ rank_tri,
                                                                const float* __restrict__ color,
                                                                const float* __restrict__ emit, float4* __restrict__ out,
                                                                int rows) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= rows) return;
    float4 m0 = mats[2 * r], m1 = mats[2 * r + 1];
    const size_t t = (size_t)rank_tri[r];
    if (color) {
        m0.y = color[3 * t];
        m0.z = color[3 * t + 1];
        m0.w = color[3 * t + 2];
    }
    if (emit) {
        m1.x = emit[3 * t];
        m1.y = emit[3 * t + 1];
        m1.z = emit[3 * t + 2];
    }
    out[2 * r] = m0;
    out[2 * r + 1] = m1;
}

__global__ __launch_bounds__(kBlock) void pt_grad_split_kernel(const double* __restrict__ table, int rows,
                                                               double* __restrict__ grad_color,
                                                               double* __restrict__ grad_emit) {
    const int i = blockIdx.x * kBlock + threadIdx.x;  // (row, channel)
    if (i >= 3 * rows) return;
    const int t = i / 3, c = i - 3 * t;
    if (grad_color) grad_color[i] = table[6 * t + c];
    if (grad_emit) grad_emit[i] = table[6 * t + 3 + c];
}

namespace {

using GradKernel = void (*)(TraceArgs, PathArgs, GradArgs);

template <bool kLdsScene, bool kLdsStack>
GradKernel grad_kernel_t(bool lds_rec, bool lds_tab) {
    return lds_rec ? (lds_tab ? pt_grad_kernel<kLdsScene, kLdsStack, true, true> : pt_grad_kernel<kLdsScene, kLdsStack, true, false>)
                   : (lds_tab ? pt_grad_kernel<kLdsScene, kLdsStack, false, true>
                              : pt_grad_kernel<kLdsScene, kLdsStack, false, false>);
}
template <bool kLdsScene, bool kLdsStack>
GradKernel grad_cam_kernel_t(bool lds_rec, bool lds_tab) {
    return lds_rec ? (lds_tab ? pt_grad_cam_kernel<kLdsScene, kLdsStack, true, true>
                              : pt_grad_cam_kernel<kLdsScene, kLdsStack, true, false>)
                   : (lds_tab ? pt_grad_cam_kernel<kLdsScene, kLdsStack, false, true>
                              : pt_grad_cam_kernel<kLdsScene, kLdsStack, false, false>);
}
GradKernel grad_kernel(const GradPlan& p) {
    const bool r = p.walk.lds_rec, t = p.lds_tab;
    if (p.camera)
        return p.walk.lds_scene
                   ? (p.walk.lds_stack ? grad_cam_kernel_t<true, true>(r, t) : grad_cam_kernel_t<true, false>(r, t))
                   : (p.walk.lds_stack ? grad_cam_kernel_t<false, true>(r, t) : grad_cam_kernel_t<false, false>(r, t));
    return p.walk.lds_scene ? (p.walk.lds_stack ? grad_kernel_t<true, true>(r, t) : grad_kernel_t<true, false>(r, t))
                            : (p.walk.lds_stack ? grad_kernel_t<false, true>(r, t) : grad_kernel_t<false, false>(r, t));
}

}  // namespace

// pt_ctx_trace's placement (paths_plan: stack rows, the scene with materials, depth - 1 record
// rows), then the table while it fits the same cap beside them.
void grad_place(const QueryScene& sc, int table_rows, size_t lds_usable, int depth, GradPlan& plan) {
    place_walk_hooked(sc.num_nodes, sc.num_tris, sc.tree_depth, 5, std::max(0, depth - 1), lds_usable, true, plan.walk);
    const size_t cap = std::min<size_t>(64 * 1024, lds_usable / 2);
    const size_t off = (plan.walk.lds_bytes + 15) / 16 * 16;
    const size_t tab_b = 6 * sizeof(double) * (size_t)table_rows;
    plan.lds_tab = !hook_off("PT_GRAD_LDS") && table_rows > 0 && lds_round(off + tab_b) <= cap;
    plan.tab_off = plan.lds_tab ? off : 0;
    if (plan.lds_tab) plan.walk.lds_bytes = off + tab_b;
}

int grad_plan(const QueryScene& sc, int table_rows, size_t lds_usable, int num_cus, int depth, int64_t items,
              GradPlan& plan, bool camera) {
    grad_place(sc, table_rows, lds_usable, depth, plan);
    plan.camera = camera ? 1 : 0;
    return walk_grid((const void*)grad_kernel(plan), lds_usable, num_cus, items, plan.walk,
                     camera ? "render_grad" : "trace_grad");
}

int grad_launch(void* stream, const QueryScene& sc, const GradPlan& plan, const GradLaunch& gl) {
    const PathsLaunch& l = gl.p;
    const WalkPlan& wp = plan.walk;
    const unsigned long long total = (unsigned long long)l.m * (unsigned long long)l.spp;
    if (l.m <= 0 || l.spp <= 0 || l.depth <= 0 || total >= (1ull << 31))
        return set_error(PT_E_ARG, "trace_grad launch of %d rays x %d samples, depth %d", l.m, l.spp, l.depth);
    if (gl.table_rows <= 0 || !gl.table || !gl.mats) return set_error(PT_E_ARG, "trace_grad launch without a table");
    if ((plan.camera != 0) != (gl.cam != nullptr) ||
        (gl.cam && (!gl.prm || !gl.shape || l.m != gl.shape->npix || gl.s_begin < 0 || gl.spp_total < l.spp)))
        return set_error(PT_E_ARG, "render_grad launch of %d pixels x %d samples from %d", l.m, l.spp, gl.s_begin);
    const int grid = (int)std::min<unsigned long long>((unsigned long long)wp.grid, (total + kBlock - 1) / kBlock);
    // every field shade and claim_item read, as paths_launch (pt_paths.hip) fills them
    TraceArgs A;
    memset(&A, 0, sizeof(A));
    A.nodes = reinterpret_cast<const float4*>(sc.nodes);
    A.tris = reinterpret_cast<const float4*>(sc.tris);
    A.mats = reinterpret_cast<const float4*>(gl.mats);
    A.radiance = l.slab;
    A.ctr = l.ctr;
    A.work = l.ctr;
    A.total_items = total;
    A.npix = l.m;
    A.depth = l.depth;
    A.seed = l.seed;
    A.s_count = l.spp;
    A.per_item = 1;
    A.stack_size = wp.rows;
    A.rec_size = wp.rec;
    A.num_node4 = 2 * sc.num_nodes;
    A.num_tri4 = 3 * sc.num_tris;
    A.num_mat4 = 2 * sc.num_tris;
    A.force_exact_slab = l.force_exact;
    A.div_npix = make_fastdiv((uint32_t)l.m);
    A.theta_tab = reinterpret_cast<const float2*>(l.theta_tab);
    A.theta_lanes = l.theta_tab ? l.theta_lanes : 0;  // no table: the computed form in every wave
    A.dark = 0;         // the unwinding always runs here
    A.flags = nullptr;  // dense slab
    const PoolSizing pool = pool_sizing(total, grid, 128);
    A.chunk = pool.chunk;
    A.static_items = pool.static_items;
    A.static_base = pool.static_base;
    A.acc_chunks = 0;  // no fused accumulation: ctr[2] counts the terms
    if (gl.cam) {
        // the fields camera_ray and part_row read, as nee_launch fills them: the items stay numbered
        // over the part's m = npix pixels
        fill_camera(A, gl.cam, *gl.shape, gl.prm);
        A.npix = l.m;
        A.div_npix = make_fastdiv((uint32_t)l.m);
        A.s_begin = gl.s_begin;
    }

    PathArgs P{};
    P.org = l.org;
    P.dir = l.dir;
    P.states = l.states;
    P.gstack = l.gstack;
    P.grec_tri = reinterpret_cast<int*>(l.grec);
    P.grec_cos = l.grec ? l.grec + wp.rec_words : nullptr;
    P.m = (uint32_t)l.m;
    P.spp = (uint32_t)l.spp;
    P.ray_base = l.ray_base;
    P.rows = wp.rows;
    P.force_exact = l.force_exact;

    GradArgs G{};
    G.grad_rgb = gl.grad_rgb;
    G.table = gl.table;
    G.rank_tri = sc.rank_tri;
    G.table_rows = gl.table_rows;
    G.tab_off = (uint32_t)plan.tab_off;
    G.spp_f = (float)(gl.cam ? gl.spp_total : l.spp);
    G.want_rgb = gl.want_rgb;
    G.want_color = gl.want_color;
    G.want_emit = gl.want_emit;
    hipLaunchKernelGGL(grad_kernel(plan), dim3(grid), dim3(kBlock), wp.lds_bytes, (hipStream_t)stream, A, P, G);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PT_E_HIP, "trace_grad launch failed: %s", hipGetErrorString(e));
    return PT_OK;
}

int grad_gather_mats(void* stream, const QueryScene& sc, const float* color, const float* emit, f4* out) {
    hipLaunchKernelGGL(pt_grad_gather_kernel, dim3((sc.num_tris + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(sc.mats), sc.rank_tri, color, emit, reinterpret_cast<float4*>(out),
                       sc.num_tris);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PT_E_HIP, "trace_grad gather failed: %s", hipGetErrorString(e));
    return PT_OK;
}

int grad_split_table(void* stream, const double* table, int32_t table_rows, double* grad_color, double* grad_emit) {
    hipLaunchKernelGGL(pt_grad_split_kernel, dim3((3 * table_rows + kBlock - 1) / kBlock), dim3(kBlock), 0,
                       (hipStream_t)stream, table, table_rows, grad_color, grad_emit);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PT_E_HIP, "trace_grad split failed: %s", hipGetErrorString(e));
    return PT_OK;
}

}  // namespace pt
