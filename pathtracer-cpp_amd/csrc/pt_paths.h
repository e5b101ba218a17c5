// pt_paths.h — the one-path-per-lane loop over the binary child-pair walk, stated once for its two
// ray sources (device code; the description of the loop, its slab-form gate, dark paths and LDS
// layout is at the top of pt_paths.hip):
//
//   BufferRays  item -> a ray of the caller's buffer (pt_paths_kernel, pt_paths.hip)
//   ListRays    item -> camera_ray of a listed pixel of the part (pt_adaptive_kernel, pt_adaptive.hip)
//   PartRays    item -> camera_ray of a pixel of the part (the light-sampling render, pt_nee.hip, and
//               the render gradients, pt_grad.hip and pt_nee_grad.hip)
//
// and the host's filling of the loop's arguments (paths_args, pt_paths.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "pt_launch.h"
#include "pt_raygate.h"
#include "pt_trace.h"

namespace pt {

struct PathArgs {
    const float* __restrict__ org;        // m x 3 (BufferRays)
    const float* __restrict__ dir;        // m x 3 (BufferRays)
    const uint32_t* __restrict__ states;  // m x spp LCG states [ray][sample], or nullptr (BufferRays)
    const int32_t* __restrict__ list;     // m part-local pixel indices (ListRays)
    int* __restrict__ gstack;             // !kLdsStack: [grid][rows][kBlock]
    int* __restrict__ grec_tri;           // !kLdsRec: [grid][rec][kBlock]
    float* __restrict__ grec_cos;
    uint32_t m;                           // rays (listed pixels) of this launch
    uint32_t spp;
    uint32_t ray_base;                    // index in the call of this launch's first ray (default seeding)
    int rows;                             // stack rows
    int force_exact;                      // PT_FORCE_EXACT_SLAB: never the IEEE min/max slab form
};

// Sample sm of ray i of the launch: the caller's ray and its LCG state, given or by the default seeding.
struct BufferRays {
    __device__ __forceinline__ static void load(const TraceArgs& A, const PathArgs& P, uint32_t i, uint32_t sm, Lcg& g,
                                                v3& o, v3& d) {
        o = v3{P.org[3 * (size_t)i], P.org[3 * (size_t)i + 1], P.org[3 * (size_t)i + 2]};
        d = v3{P.dir[3 * (size_t)i], P.dir[3 * (size_t)i + 1], P.dir[3 * (size_t)i + 2]};
        g.s = P.states ? P.states[(size_t)i * P.spp + sm] : pt_sample_seed(P.ray_base + i, sm, A.seed);
    }
};

// Sample A.s_begin + sm of listed pixel i: the render's camera ray of part-local pixel list[i]
// (camera_ray seeds at the global pixel index; A holds the camera and partition fields, while
// A.npix and A.div_npix are the launch's m, as for BufferRays).
struct ListRays {
    __device__ __forceinline__ static void load(const TraceArgs& A, const PathArgs& P, uint32_t i, uint32_t sm, Lcg& g,
                                                v3& o, v3& d) {
        camera_ray(A, (int)P.list[i], A.s_begin + (int)sm, g, o, d);
    }
};

// Sample A.s_begin + sm of pixel i of the part: the render's camera ray (camera_ray seeds at the
// global pixel index and makes Camera::get_ray's two draws; A holds the camera and partition fields).
struct PartRays {
    __device__ __forceinline__ static void load(const TraceArgs& A, const PathArgs&, uint32_t i, uint32_t sm, Lcg& g, v3& o,
                                                v3& d) {
        camera_ray(A, (int)i, A.s_begin + (int)sm, g, o, d);
    }
};

template <class Rays, bool kLdsScene, bool kLdsStack, bool kLdsRec>
__device__ __forceinline__ void paths_body(const TraceArgs& A, const PathArgs& P) {
    extern __shared__ float4 lds4[];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const float4* __restrict__ nodes = A.nodes;
    const float4* __restrict__ tris = A.tris;
    const float4* __restrict__ mats = A.mats;
    const int scene4 = kLdsScene ? A.num_node4 + A.num_tri4 + A.num_mat4 : 0;
    if (kLdsScene) {
        float4* s_nodes = lds4;
        float4* s_tris = lds4 + A.num_node4;
        float4* s_mats = s_tris + A.num_tri4;
        for (int i = tid; i < A.num_node4; i += kBlock) s_nodes[i] = A.nodes[i];
        for (int i = tid; i < A.num_tri4; i += kBlock) s_tris[i] = A.tris[i];
        for (int i = tid; i < A.num_mat4; i += kBlock) s_mats[i] = A.mats[i];
        __syncthreads();
        nodes = s_nodes;
        tris = s_tris;
        mats = s_mats;
    }
    int* const lds_stk = reinterpret_cast<int*>(lds4 + scene4);
    int* const lds_rec = lds_stk + (kLdsStack ? P.rows * kBlock : 0);
    int* __restrict__ stk = kLdsStack ? lds_stk : P.gstack + (size_t)blockIdx.x * P.rows * kBlock;
    int* __restrict__ rec_tri = kLdsRec ? lds_rec : P.grec_tri + (size_t)blockIdx.x * A.rec_size * kBlock;
    float* __restrict__ rec_cos = kLdsRec ? reinterpret_cast<float*>(lds_rec + A.rec_size * kBlock)
                                          : P.grec_cos + (size_t)blockIdx.x * A.rec_size * kBlock;

    bool alive = true;     // the pool may still hold items for this lane
    bool active = false;   // the lane has a path in flight (item `item`)
    bool nan_cos = false;  // its path recorded a non-finite cosine
    uint32_t item = 0;
    Lcg g{0};
    v3 o{0, 0, 0}, d{0, 0, 1};
    int k = 0;
    unsigned long long n_rays = 0;  // this wave's segments (wave-uniform)
    Pool pool = pool_start(A);

    while (true) {
        const bool need = alive && !active;
        if (__any(need)) {
            claim_item(A, lane, need, pool, alive, item);
            if (need && alive) {  // item < total_items = m * spp
                const uint32_t sm = fdiv(item, A.div_npix), i = item - sm * P.m;
                Rays::load(A, P, i, sm, g, o, d);
                k = 0;
                nan_cos = false;
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
        if (active) {
            end = shade(A, mats, tris, rec_tri, rec_cos, tid, hit, t, g, o, d, k, L);
            // the recorded cosine n . d' is finite exactly when the new direction is (|n| = 1)
            if (!end) nan_cos = nan_cos || !all_finite(d);
        }
        if (__any(end && nan_cos)) {
            if (end) finish_path<int, false, true, false>(A, mats, rec_tri, rec_cos, tid, k, L, item);
        } else if (end) {
            finish_path<int>(A, mats, rec_tri, rec_cos, tid, k, L, item);
        }
        if (end) active = false;
    }
    count_rays_wave(A, lane, n_rays);
}

// Every field of TraceArgs and PathArgs the loop reads with BufferRays, for one launch over l.m
// rays x l.spp samples on `grid` blocks (the pool by pool_sizing, as a render's tree walk).
void paths_args(const QueryScene& sc, const WalkPlan& plan, const PathsLaunch& l, int grid, TraceArgs& A, PathArgs& P);

}  // namespace pt
