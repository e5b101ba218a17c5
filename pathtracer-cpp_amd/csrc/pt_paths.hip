// pt_paths.hip — trace() (render.h:36-61) for a caller's buffer of rays, over the binary
// child-pair walk (gfx950).
//
//   pt_paths_kernel<kLdsScene, kLdsStack, kLdsRec>  one path per lane: intersect_tree, shade and
//                                                   finish_path of pt_trace.h, fed from a ray
//                                                   buffer instead of camera_ray (the loop itself:
//                                                   paths_body, pt_paths.h, shared with the
//                                                   per-pixel rounds of pt_adaptive.hip)
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
// rec_size, dark, flags, theta_tab, theta_lanes). paths_launch fills those as a render does (the pool by pool_sizing, pt_launch.h).
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

#include "pt_paths.h"

namespace pt {

static_assert(kSpecularIterBound == kMaxSpecularIters, "host and device bound of the specular rejection loop");

// The loop (paths_body, pt_paths.h) over the caller's ray buffer.
template <bool kLdsScene, bool kLdsStack, bool kLdsRec>
__global__ __launch_bounds__(kBlock) void pt_paths_kernel(TraceArgs A, PathArgs P) {
    paths_body<BufferRays, kLdsScene, kLdsStack, kLdsRec>(A, P);
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

}  // namespace

// Placement and grid by the binary walk's shared rules (pt_launch.h: place_walk, plan_grid): the
// stack rows, then nodes, triangles and (here) materials, 5 float4 per triangle, then the path
// records, depth - 1 rows. Whatever does not fit is read and written through L1/L2, so every
// depth up to PT_MAX_DEPTH runs.
int paths_plan(const QueryScene& sc, size_t lds_usable, int num_cus, int depth, int64_t items, WalkPlan& plan) {
    place_walk_hooked(sc.num_nodes, sc.num_tris, sc.tree_depth, 5, std::max(0, depth - 1), lds_usable, true, plan);
    return walk_grid((const void*)paths_kernel(plan.lds_scene, plan.lds_stack, plan.lds_rec), lds_usable, num_cus, items,
                     plan, "trace");
}

void paths_args(const QueryScene& sc, const WalkPlan& plan, const PathsLaunch& l, int grid, TraceArgs& A, PathArgs& P) {
    const unsigned long long total = (unsigned long long)l.m * (unsigned long long)l.spp;
    // every field shade, finish_path and claim_item read, as fill_trace_args (pt_kernel.hip) fills them
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
    A.div_npix = make_fastdiv((uint32_t)l.m);
    A.theta_tab = reinterpret_cast<const float2*>(l.theta_tab);
    A.theta_lanes = l.theta_tab ? l.theta_lanes : 0;  // no table: the computed form in every wave
    A.dark = l.dark;
    A.flags = nullptr;  // dense slab: every path stores its record
    // the work pool by a render's rule for the tree walk (refills of 128 to kChunk items)
    const PoolSizing pool = pool_sizing(total, grid, 128);
    A.chunk = pool.chunk;
    A.static_items = pool.static_items;
    A.static_base = pool.static_base;
    A.acc_chunks = 0;            // no fused accumulation: the sum is a pass of its own

    P = PathArgs{};
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
}

int paths_launch(void* stream, const QueryScene& sc, const WalkPlan& plan, const PathsLaunch& l) {
    const unsigned long long total = (unsigned long long)l.m * (unsigned long long)l.spp;
    if (l.m <= 0 || l.spp <= 0 || l.depth <= 0 || total >= (1ull << 31))
        return set_error(PT_E_ARG, "trace launch of %d rays x %d samples, depth %d", l.m, l.spp, l.depth);
    const int grid = (int)std::min<unsigned long long>((unsigned long long)plan.grid, (total + kBlock - 1) / kBlock);
    TraceArgs A;
    PathArgs P;
    paths_args(sc, plan, l, grid, A, P);
    hipLaunchKernelGGL(paths_kernel(plan.lds_scene, plan.lds_stack, plan.lds_rec), dim3(grid), dim3(kBlock), plan.lds_bytes,
                       (hipStream_t)stream, A, P);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PT_E_HIP, "trace launch failed: %s", hipGetErrorString(e));
    return PT_OK;
}

}  // namespace pt
