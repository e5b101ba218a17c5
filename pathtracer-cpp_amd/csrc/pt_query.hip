// pt_query.hip — batched ray queries and first-hit AOVs over the binary child-pair walk (gfx950).
//
//   pt_query_kernel<kAny, kLdsScene, kLdsStack>  BVH::intersect (bvh.h:156-183) for a caller's
//                                                buffer of rays: closest hit, or occlusion
//   pt_aov_kernel<kLdsScene, kLdsStack>          the first hit of one sample of every pixel:
//                                                camera_ray + the same walk + material / normal
//
// One ray (pixel) per lane, blocks of kBlock lanes, grid-stride. The closest-hit walk is
// intersect_tree (pt_trace.h), whose triangle-test order is the reference's; its result is a
// rank position, mapped to the caller's triangle index through rank_tri (pt_internal.h).
//
// Stack: rows stk[sp * kBlock + tid], `rows` = max(1, tree depth) of them. The child-pair walk
// pushes at most once per level it descends (the deferred left sibling) and a pop resumes at a
// sibling's level with that entry gone, so sp never exceeds the depth of the node in hand: the
// row count is a property of the tree alone. Whatever the caller passes as a ray (inf, NaN, a
// zero direction) only decides which box tests pass, never how deep the stack gets.
//
// Any hit: occluded iff the reference's t < tmax. The reference's walk is not pruned by t (its
// slab test has no far bound), so the set of triangles it tests does not depend on the order
// or on hits found so far, and its t is the minimum over the tested triangles that hit. Hence
// t < tmax iff some tested triangle hits with t_ < tmax, and the walk may stop at the first
// such triangle. Boxes are not culled by tmax.
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "pt_launch.h"
#include "pt_raygate.h"
#include "pt_trace.h"

namespace pt {

// intersect_tree's walk, stopping at the first triangle hit with t < tmax (see above).
template <bool kFiniteInv, typename NodePtr, typename TriPtr>
__device__ __forceinline__ bool occluded_tree(NodePtr nodes, TriPtr tris, int* __restrict__ stk, int tid, v3 o, v3 d,
                                              v3 inv, float tmax) {
    int sp = 0;
    const NodeBox root = load_node(nodes, 0);
    int ca = root.a, cb = root.b;
    bool go = box_hit<kFiniteInv>(root.lb, root.rt, o, inv);
    while (go) {
        if (ca >= 0) {
            const NodeBox L = load_node(nodes, ca);
            const NodeBox R = load_node(nodes, ca + 1);
            const bool hl = box_hit<kFiniteInv>(L.lb, L.rt, o, inv);
            const bool hr = box_hit<kFiniteInv>(R.lb, R.rt, o, inv);
            if (hr) {
                if (hl) {
                    stk[sp * kBlock + tid] = ca;
                    sp++;
                }
                ca = R.a;
                cb = R.b;
                continue;
            }
            if (hl) {
                ca = L.a;
                cb = L.b;
                continue;
            }
        } else {
            for (int i = -ca - 1; i <= cb; i++) {
                const float4 t0 = tris[3 * i], t1 = tris[3 * i + 1], t2 = tris[3 * i + 2];
                float tt;
                if (tri_hit(v3{t0.x, t0.y, t0.z}, v3{t0.w, t1.x, t1.y}, v3{t1.z, t1.w, t2.x}, o, d, tt) && tt < tmax)
                    return true;
            }
        }
        if (sp == 0) break;
        sp--;
        const float4 q = nodes[2 * stk[sp * kBlock + tid] + 1];
        ca = __float_as_int(q.z);
        cb = __float_as_int(q.w);
    }
    return false;
}

struct QueryArgs {
    const float4* __restrict__ nodes;
    const float4* __restrict__ tris;
    const float4* __restrict__ mats;
    const int32_t* __restrict__ rank_tri;
    const float* __restrict__ org;   // n x 3
    const float* __restrict__ dir;   // n x 3
    const float* __restrict__ tmax;  // kAny: n floats, or nullptr = 1e30f
    float* __restrict__ t_out;
    int32_t* __restrict__ out;
    int* __restrict__ gstack;        // !kLdsStack: [grid][rows][kBlock]
    unsigned long long* __restrict__ hits;
    int n;
    int num_node4, num_tri4;
    int rows;
    int force_exact;                 // PT_FORCE_EXACT_SLAB: never the IEEE min/max slab form
};

// LDS: [nodes, tris (kLdsScene)] [stack: rows x kBlock int (kLdsStack)]
template <bool kLdsScene, bool kLdsStack>
__device__ __forceinline__ int* query_stage(const QueryArgs& Q, const float4*& nodes, const float4*& tris) {
    extern __shared__ float4 lds4[];
    const int tid = threadIdx.x;
    nodes = Q.nodes;
    tris = Q.tris;
    if (kLdsScene) {
        float4* s_nodes = lds4;
        float4* s_tris = lds4 + Q.num_node4;
        for (int i = tid; i < Q.num_node4; i += kBlock) s_nodes[i] = Q.nodes[i];
        for (int i = tid; i < Q.num_tri4; i += kBlock) s_tris[i] = Q.tris[i];
        __syncthreads();
        nodes = s_nodes;
        tris = s_tris;
    }
    return kLdsStack ? reinterpret_cast<int*>(lds4 + (kLdsScene ? Q.num_node4 + Q.num_tri4 : 0))
                     : Q.gstack + (size_t)blockIdx.x * Q.rows * kBlock;
}

// The walk of one lane's ray; `fast` is wave-uniform. Returns the rank position (closest) or
// 0 / 1 (any hit); a lane without a ray returns -1 / 0.
template <bool kAny>
__device__ __forceinline__ int query_walk(const float4* nodes, const float4* tris, int* stk, int tid, bool have,
                                          bool fast, v3 o, v3 d, v3 inv, float tmax, float& t) {
    t = 1e30f;
    if (!have) return kAny ? 0 : -1;
    if (kAny)
        return fast ? occluded_tree<true>(nodes, tris, stk, tid, o, d, inv, tmax)
                    : occluded_tree<false>(nodes, tris, stk, tid, o, d, inv, tmax);
    return fast ? intersect_tree<true>(nodes, tris, stk, tid, o, d, inv, t)
                : intersect_tree<false>(nodes, tris, stk, tid, o, d, inv, t);
}

__device__ __forceinline__ void count_hits_wave(unsigned long long* hits, unsigned long long n) {
    if ((threadIdx.x & (kWave - 1)) == 0 && n) atomicAdd(hits, n);
}

template <bool kAny, bool kLdsScene, bool kLdsStack>
__global__ __launch_bounds__(kBlock) void pt_query_kernel(QueryArgs Q) {
    const int tid = threadIdx.x;
    const float4 *nodes, *tris;
    int* stk = query_stage<kLdsScene, kLdsStack>(Q, nodes, tris);
    unsigned long long n_hits = 0;  // this wave's (wave-uniform)
    // base < n <= 2^28 and the stride is below 2^25: no 32-bit overflow (host: kQueryChunk)
    for (int base = blockIdx.x * kBlock; base < Q.n; base += gridDim.x * kBlock) {
        const int i = base + tid;
        const bool have = i < Q.n;
        v3 o{0, 0, 0}, d{0, 0, 1};
        float tmax = 1e30f;
        if (have) {
            o = v3{Q.org[3 * i], Q.org[3 * i + 1], Q.org[3 * i + 2]};
            d = v3{Q.dir[3 * i], Q.dir[3 * i + 1], Q.dir[3 * i + 2]};
            if (kAny && Q.tmax) tmax = Q.tmax[i];
        }
        const v3 inv = rcp3_exact(d, have);  // bvh.h:157
        const bool fast = !Q.force_exact && __all(!have || query_ray_bounded(o, inv));
        float t;
        const int r = query_walk<kAny>(nodes, tris, stk, tid, have, fast, o, d, inv, tmax, t);
        n_hits += (unsigned long long)__popcll(__ballot(kAny ? r != 0 : r >= 0));
        if (have) {
            if (kAny) {
                Q.out[i] = r;
            } else {
                Q.t_out[i] = t;
                Q.out[i] = r >= 0 ? Q.rank_tri[r] : -1;
            }
        }
    }
    count_hits_wave(Q.hits, n_hits);
}

struct AovOut {
    float* __restrict__ t;
    int32_t* __restrict__ tri;
    float* __restrict__ normal;
    float* __restrict__ albedo;
    float* __restrict__ emission;
    float* __restrict__ ray;
};

__device__ __forceinline__ void store3(float* __restrict__ p, size_t q, v3 v) {
    p[3 * q] = v.x;
    p[3 * q + 1] = v.y;
    p[3 * q + 2] = v.z;
}

// A: the camera, partition and FastDiv fields camera_ray reads, FIRST among the arguments
// (camera_ray reads them from the kernarg segment at offset 0, kernarg_args); A.npix pixels.
template <bool kLdsScene, bool kLdsStack>
__global__ __launch_bounds__(kBlock) void pt_aov_kernel(TraceArgs A, QueryArgs Q, AovOut out, int sample) {
    const int tid = threadIdx.x;
    const float4 *nodes, *tris;
    int* stk = query_stage<kLdsScene, kLdsStack>(Q, nodes, tris);
    unsigned long long n_hits = 0;
    for (int base = blockIdx.x * kBlock; base < A.npix; base += gridDim.x * kBlock) {  // npix <= 2^30
        const int q = base + tid;
        const bool have = q < A.npix;
        v3 o{0, 0, 0}, d{0, 0, 1};
        if (have) {
            Lcg g{0};
            camera_ray(A, q, sample, g, o, d);
        }
        const v3 inv = rcp3_exact(d, have);
        const bool fast = !Q.force_exact && __all(!have || query_ray_bounded(o, inv));
        float t;
        const int r = query_walk<false>(nodes, tris, stk, tid, have, fast, o, d, inv, 1e30f, t);
        n_hits += (unsigned long long)__popcll(__ballot(r >= 0));
        if (have) {  // no early `continue`: every lane reaches the next iteration's wave-wide vote together
            if (out.t) out.t[q] = t;
            if (out.tri) out.tri[q] = r >= 0 ? Q.rank_tri[r] : -1;
            if (out.ray) {
                store3(out.ray, 2 * (size_t)q, o);
                store3(out.ray, 2 * (size_t)q + 1, d);
            }
            v3 n{0, 0, 0}, alb{0, 0, 0}, emi{0, 0, 0};
            if (r >= 0) {
                // the packed normal normalize(cross(e1, e2)), faced as Triangle::normal (triangle.h:48)
                const float4 t2 = tris[3 * r + 2];
                n = v3{t2.y, t2.z, t2.w};
                if (!(dot(n, d) < 0.0f)) n = neg(n);
                const float4 m0 = Q.mats[2 * r], m1 = Q.mats[2 * r + 1];
                alb = v3{m0.y, m0.z, m0.w};
                emi = v3{m1.x, m1.y, m1.z};
            }
            if (out.normal) store3(out.normal, (size_t)q, n);
            if (out.albedo) store3(out.albedo, (size_t)q, alb);
            if (out.emission) store3(out.emission, (size_t)q, emi);
        }
    }
    count_hits_wave(Q.hits, n_hits);
}

namespace {

using QueryKernel = void (*)(QueryArgs);
using AovKernel = void (*)(TraceArgs, QueryArgs, AovOut, int);

template <bool kAny>
QueryKernel query_kernel_t(bool lds_scene, bool lds_stack) {
    return lds_scene ? (lds_stack ? pt_query_kernel<kAny, true, true> : pt_query_kernel<kAny, true, false>)
                     : (lds_stack ? pt_query_kernel<kAny, false, true> : pt_query_kernel<kAny, false, false>);
}
AovKernel aov_kernel(bool lds_scene, bool lds_stack) {
    return lds_scene ? (lds_stack ? pt_aov_kernel<true, true> : pt_aov_kernel<true, false>)
                     : (lds_stack ? pt_aov_kernel<false, true> : pt_aov_kernel<false, false>);
}
const void* plan_kernel(int which, bool lds_scene, bool lds_stack) {
    return which == 2   ? (const void*)aov_kernel(lds_scene, lds_stack)
           : which == 1 ? (const void*)query_kernel_t<true>(lds_scene, lds_stack)
                        : (const void*)query_kernel_t<false>(lds_scene, lds_stack);
}

QueryArgs query_args(const QueryScene& sc, const WalkPlan& plan, int* gstack, unsigned long long* hits,
                     int force_exact) {
    QueryArgs Q{};
    Q.nodes = reinterpret_cast<const float4*>(sc.nodes);
    Q.tris = reinterpret_cast<const float4*>(sc.tris);
    Q.mats = reinterpret_cast<const float4*>(sc.mats);
    Q.rank_tri = sc.rank_tri;
    Q.gstack = gstack;
    Q.hits = hits;
    Q.num_node4 = 2 * sc.num_nodes;
    Q.num_tri4 = 3 * sc.num_tris;
    Q.rows = plan.rows;
    Q.force_exact = force_exact;
    return Q;
}

}  // namespace

// Placement and grid by the binary walk's shared rules (pt_launch.h: place_walk, plan_grid): the
// stack rows, then nodes and triangles (3 float4 each, no materials), no records.
int query_plan(int which, const QueryScene& sc, size_t lds_usable, int num_cus, int64_t count, WalkPlan& plan) {
    place_walk_hooked(sc.num_nodes, sc.num_tris, sc.tree_depth, 3, 0, lds_usable, false, plan);
    return walk_grid(plan_kernel(which, plan.lds_scene, plan.lds_stack), lds_usable, num_cus, count, plan, "query");
}

int query_launch(void* stream, const QueryScene& sc, const WalkPlan& plan, int any, const float* org, const float* dir,
                 const float* tmax, int32_t n, float* t_out, int32_t* out, int* gstack, unsigned long long* hits,
                 int force_exact) {
    QueryArgs Q = query_args(sc, plan, gstack, hits, force_exact);
    Q.org = org;
    Q.dir = dir;
    Q.tmax = tmax;
    Q.t_out = t_out;
    Q.out = out;
    Q.n = n;
    const int grid = (int)std::min<int64_t>(plan.grid, ((int64_t)n + kBlock - 1) / kBlock);
    QueryKernel k = any ? query_kernel_t<true>(plan.lds_scene, plan.lds_stack)
                        : query_kernel_t<false>(plan.lds_scene, plan.lds_stack);
    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), plan.lds_bytes, (hipStream_t)stream, Q);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PT_E_HIP, "query launch failed: %s", hipGetErrorString(e));
    return PT_OK;
}

int aov_launch(void* stream, const QueryScene& sc, const WalkPlan& plan, const pt_camera* cam, const pt_params* prm,
               const PartShape& shape, int32_t sample, const pt_aov* out, int* gstack, unsigned long long* hits,
               int force_exact) {
    const QueryArgs Q = query_args(sc, plan, gstack, hits, force_exact);
    TraceArgs A;
    memset(&A, 0, sizeof(A));
    fill_camera(A, cam, shape, prm);  // the fields camera_ray and part_row read
    const AovOut O{out->t, out->tri, out->normal, out->albedo, out->emission, out->ray};
    const int grid = (int)std::min<int64_t>(plan.grid, ((int64_t)A.npix + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(aov_kernel(plan.lds_scene, plan.lds_stack), dim3(grid), dim3(kBlock), plan.lds_bytes,
                       (hipStream_t)stream, A, Q, O, sample);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PT_E_HIP, "aov launch failed: %s", hipGetErrorString(e));
    return PT_OK;
}

}  // namespace pt
