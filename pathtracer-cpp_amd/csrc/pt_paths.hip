// pt_paths.hip — trace() (render.h:36-61) for a caller's buffer of rays, over the binary
// child-pair walk (gfx950).
//
//   pt_paths_kernel<kLdsScene, kLdsStack, kLdsRec>  one path per lane: intersect_tree, shade and
//                                                   finish_path of pt_trace.h, fed from a ray
//                                                   buffer instead of camera_ray
//
// A work item is (ray, sample); the items of a launch over m rays are numbered sample-major
// (item j -> sample j / m, ray j % m), so consecutive lanes load consecutive rays and item j's
// radiance is record j of the launch's dense slab [sample][ray][rgb], as finish_path writes it.
// Paths run from 1 to `depth` segments: one loop iteration is one segment of every lane, and a
// lane whose path ended takes its next item at the top of the next iteration (claim_item: the
// idle lanes counted by ballot, one counter atomic per wave per refill), so a wave never waits
// for its longest path with idle lanes. The per-ray sum over samples is a separate pass
// (pt_accumulate_kernel, one lane per ray, samples ascending, then / spp): the samples of one ray
// finish in any order in any wave, and float addition in sample order is the contract.
//
// shade and finish_path read kernarg_args(): the FIRST kernel argument as TraceArgs (depth,
// rec_size, dark, flags, theta_tab, theta_lanes). paths_launch fills those as pt_ctx_render does.
//
// Slab-form gate: the IEEE min/max slab form needs every lane's origin and inverse direction
// finite and bounded (query_ray_bounded). A caller's origin can be NaN or inf, and after such a
// ray so can a bounce origin (hp = o + d t), so the gate is evaluated on every segment.
//
// Dark paths: finish_path skips the unwinding of a path that ends at +0 in a scene whose bounce
// materials are dark, because every level is then +0 + (+-0) c = +0 — for a FINITE cosine c. A
// caller's direction near FLT_MAX can hit a small triangle at a finite point and overflow
// 2 (d . n) in the SPECULAR sampler: the new direction and its cosine are NaN, and the reference
// returns NaN. A wave with such a path among its ending lanes unwinds them all.
//
// LDS: [nodes, tris, mats (kLdsScene)] [stack: rows x kBlock int (kLdsStack)]
//      [records: rec x kBlock int, rec x kBlock float (kLdsRec)], every part a multiple of 16 B.
// Otherwise the stack rows are P.gstack[block][row][lane] and the records
// P.grec_tri / P.grec_cos [block][row][lane] (the per-block layout shade's indexing expects).
#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "pt_internal.h"
#include "pt_raygate.h"
#include "pt_trace.h"

namespace pt {

static_assert(kSpecularIterBound == kMaxSpecularIters, "host and device bound of the specular rejection loop");

FastDiv fastdiv_for(uint32_t d);  // make_fastdiv (pt_kernel.hip)

struct PathArgs {
    const float* __restrict__ org;        // m x 3
    const float* __restrict__ dir;        // m x 3
    const uint32_t* __restrict__ states;  // m x spp LCG states [ray][sample], or nullptr
    int* __restrict__ gstack;             // !kLdsStack: [grid][rows][kBlock]
    int* __restrict__ grec_tri;           // !kLdsRec: [grid][rec][kBlock]
    float* __restrict__ grec_cos;
    uint32_t m;                           // rays of this launch
    uint32_t spp;
    uint32_t ray_base;                    // index in the call of this launch's first ray (default seeding)
    int rows;                             // stack rows
    int force_exact;                      // PT_FORCE_EXACT_SLAB: never the IEEE min/max slab form
};

template <bool kLdsScene, bool kLdsStack, bool kLdsRec>
__global__ __launch_bounds__(kBlock) void pt_paths_kernel(TraceArgs A, PathArgs P) {
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
                o = v3{P.org[3 * (size_t)i], P.org[3 * (size_t)i + 1], P.org[3 * (size_t)i + 2]};
                d = v3{P.dir[3 * (size_t)i], P.dir[3 * (size_t)i + 1], P.dir[3 * (size_t)i + 2]};
                g.s = P.states ? P.states[(size_t)i * P.spp + sm] : pt_sample_seed(P.ray_base + i, sm, A.seed);
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
        const v3 inv{rcp_exact(d.x), rcp_exact(d.y), rcp_exact(d.z)};  // bvh.h:157
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

namespace {

using PathsKernel = void (*)(TraceArgs, PathArgs);

template <bool kLdsScene, bool kLdsStack>
PathsKernel paths_kernel_t(bool lds_rec) {
    return lds_rec ? pt_paths_kernel<kLdsScene, kLdsStack, true> : pt_paths_kernel<kLdsScene, kLdsStack, false>;
}
PathsKernel paths_kernel(bool lds_scene, bool lds_stack, bool lds_rec) {
    return lds_scene ? (lds_stack ? paths_kernel_t<true, true>(lds_rec) : paths_kernel_t<true, false>(lds_rec))
                     : (lds_stack ? paths_kernel_t<false, true>(lds_rec) : paths_kernel_t<false, false>(lds_rec));
}

size_t lds_round(size_t b) { return (b + kLdsGranule - 1) / kLdsGranule * kLdsGranule; }

}  // namespace

// Placement, by query_plan's rules (pt_query.hip) and hooks: the stack rows go to LDS when they
// leave two blocks per CU and stay inside 64 KiB; nodes, triangles and (here) materials when
// they fit PT_LDS_SCENE_BYTES' budget and the same bounds beside the stack; then the path
// records, depth - 1 rows of kBlock x 8 B, when they still fit beside both (PT_TRACE_LDS_REC=0,
// test hook, forces the global buffer). Whatever does not fit is read and written through L1/L2,
// so every depth up to PT_MAX_DEPTH runs.
int paths_plan(const QueryScene& sc, size_t lds_usable, int num_cus, int depth, int64_t items, PathsPlan& plan) {
    const size_t cap = std::min<size_t>(64 * 1024, lds_usable / 2);
    plan.rows = std::max(1, sc.tree_depth);
    plan.rec = std::max(0, depth - 1);
    const size_t stack_b = sizeof(int) * (size_t)kBlock * plan.rows;
    const char* ls = hook_env("PT_QUERY_LDS_STACK");
    plan.lds_stack = !(ls && *ls == '0') && lds_round(stack_b) <= cap;
    const size_t scene_b = sizeof(float4) * (2 * (size_t)sc.num_nodes + 5 * (size_t)sc.num_tris);
    const char* le = hook_env("PT_LDS_SCENE_BYTES");
    const size_t budget = (le && *le) ? (size_t)strtoull(le, nullptr, 0) : 32 * 1024;  // lds_scene_budget (pt_kernel.hip)
    size_t used = plan.lds_stack ? stack_b : 0;
    plan.lds_scene = scene_b <= budget && lds_round(scene_b + used) <= cap;
    used += plan.lds_scene ? scene_b : 0;
    const size_t rec_b = 2 * sizeof(int) * (size_t)kBlock * plan.rec;
    const char* lr = hook_env("PT_TRACE_LDS_REC");
    plan.lds_rec = !(lr && *lr == '0') && lds_round(used + rec_b) <= cap;
    used += plan.lds_rec ? rec_b : 0;
    plan.lds_bytes = used;
    int per_cu = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, (const void*)paths_kernel(plan.lds_scene, plan.lds_stack, plan.lds_rec), kBlock, plan.lds_bytes);
    if (e != hipSuccess) return set_error(PT_E_HIP, "trace occupancy failed: %s", hipGetErrorString(e));
    // the occupancy query can be optimistic about LDS (kLdsUsable, pt_internal.h)
    if (plan.lds_bytes > 0 && lds_usable > 0) per_cu = std::min<int>(per_cu, (int)(lds_usable / lds_round(plan.lds_bytes)));
    per_cu = std::max(1, per_cu);
    const int64_t blocks = (items + kBlock - 1) / kBlock;
    plan.grid = (int)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)per_cu * std::max(1, num_cus)));
    plan.stack_ints = plan.lds_stack ? 0 : (size_t)plan.grid * plan.rows * kBlock;
    plan.rec_words = plan.lds_rec ? 0 : (size_t)plan.grid * plan.rec * kBlock;
    return PT_OK;
}

int paths_launch(void* stream, const QueryScene& sc, const PathsPlan& plan, const PathsLaunch& l) {
    const unsigned long long total = (unsigned long long)l.m * (unsigned long long)l.spp;
    if (l.m <= 0 || l.spp <= 0 || l.depth <= 0 || total >= (1ull << 31))
        return set_error(PT_E_ARG, "trace launch of %d rays x %d samples, depth %d", l.m, l.spp, l.depth);
    const int grid = (int)std::min<unsigned long long>((unsigned long long)plan.grid, (total + kBlock - 1) / kBlock);
    // every field shade, finish_path and claim_item read, as pt_ctx_render fills them
    TraceArgs A;
    memset(&A, 0, sizeof(A));
    A.nodes = reinterpret_cast<const float4*>(sc.nodes);
    A.tris = reinterpret_cast<const float4*>(sc.tris);
    A.mats = reinterpret_cast<const float4*>(sc.mats);
    A.radiance = l.slab;
    A.ctr = l.ctr;
    A.work = l.ctr;
    A.total_items = total;
    A.npix = l.m;
    A.depth = l.depth;
    A.seed = l.seed;
    A.s_count = l.spp;
    A.per_item = 1;
    A.stack_size = plan.rows;
    A.rec_size = plan.rec;
    A.num_node4 = 2 * sc.num_nodes;
    A.num_tri4 = 3 * sc.num_tris;
    A.num_mat4 = 2 * sc.num_tris;
    A.force_exact_slab = l.force_exact;
    A.div_npix = fastdiv_for((uint32_t)l.m);
    A.theta_tab = reinterpret_cast<const float2*>(l.theta_tab);
    A.theta_lanes = l.theta_tab ? l.theta_lanes : 0;  // no table: the computed form in every wave
    A.dark = l.dark;
    A.flags = nullptr;  // dense slab: every path stores its record
    // Refills (pt_ctx_render's rules for the tree walk): about 128 per wave, 128 to kChunk items
    // each; every wave starts with a static range, the whole even share in a small launch.
    const unsigned long long waves = (unsigned long long)grid * (kBlock / kWave);
    A.chunk = (int)std::max<unsigned long long>(kWave, std::min<unsigned long long>(kChunk, std::max<unsigned long long>(128, total / (waves * 128))));
    const unsigned long long share = total / waves;
    unsigned long long st = std::min<unsigned long long>((unsigned long long)A.chunk, share);
    if (share < 4ull * kChunk) st = share;
    A.static_items = (uint32_t)st;
    A.static_base = waves * st;  // <= total < 2^31
    A.acc_chunks = 0;            // no fused accumulation: the sum is a pass of its own

    PathArgs P{};
    P.org = l.org;
    P.dir = l.dir;
    P.states = l.states;
    P.gstack = l.gstack;
    P.grec_tri = reinterpret_cast<int*>(l.grec);
    P.grec_cos = l.grec ? l.grec + plan.rec_words : nullptr;
    P.m = (uint32_t)l.m;
    P.spp = (uint32_t)l.spp;
    P.ray_base = l.ray_base;
    P.rows = plan.rows;
    P.force_exact = l.force_exact;
    hipLaunchKernelGGL(paths_kernel(plan.lds_scene, plan.lds_stack, plan.lds_rec), dim3(grid), dim3(kBlock), plan.lds_bytes,
                       (hipStream_t)stream, A, P);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PT_E_HIP, "trace launch failed: %s", hipGetErrorString(e));
    return PT_OK;
}

}  // namespace pt
