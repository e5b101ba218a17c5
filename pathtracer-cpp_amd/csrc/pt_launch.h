// pt_launch.h — the host's launch rules, each stated once (pt_launch.hip): hook parsing, LDS
// rounding and the occupancy clamp, device buffers that grow, a part's shape and the camera /
// partition fields of TraceArgs, the work pool of a launch, the scene predicates, and where the
// binary walk keeps its stack, scene and records. Host only; used by pt_kernel.hip (renders),
// pt_query.hip (ray queries and AOVs), pt_paths.hip (trace() on caller-supplied rays) and pt_rtc.hip.
#pragma once

#include <stdlib.h>

#include "pt_internal.h"

namespace pt {

struct TraceArgs;

// ---- hooks (hook_env: honoured only under PT_TEST_HOOKS=1). Call sites keep their own clamps.
// Off when the value starts with '0'.
inline bool hook_off(const char* name) {
    const char* e = hook_env(name);
    return e && *e == '0';
}
// A non-empty value, else dflt. (An EMPTY value is ignored here. PT_WIDE_QUEUE_LEN reads an empty
// value as 0, and PT_POOL_CHUNK / PT_POOL_REFILLS are decimal only: parsed where they are used.
// So are the hooks for which every number means something other than "unset", 0 included:
// PT_BATCH_BYTES, PT_PAIR_QUEUE, PT_WIDE_QUEUE_CAP, and PT_FLAGS_PM, which reads one character.)
inline int hook_int(const char* name, int dflt) {
    const char* e = hook_env(name);
    return (e && *e) ? atoi(e) : dflt;
}
// Whether the flat kernels share the wave's stock of prefetched camera rays among its lanes
//  or keep each ray to the lane that generated it: shared in scenes without a
// SPECULAR material (headline +1.1 %, 4096^2 depth 8 +1.9 %), per lane in scenes with one (modified
// Cornell r = 0.3: -0.7 % shared; profiles/ray_stack). PT_RAY_STACK=0 / 1 (test hook, A/B) forces
// either. Read when a scene is set (the scene kernel's source) and when a render is planned.
inline bool ray_stack_on(bool specular) { return hook_int("PT_RAY_STACK", specular ? 0 : 1) != 0; }
// PT_RAY_RESERVE (tuning hook): the shared stock refills once it holds fewer rays than the lanes
// without a path plus this; 0..64, 0 measured best (profiles/ray_stack). A constant of the scene
// kernel's source, TraceArgs::ray_reserve for the offline kernels.
inline int ray_reserve() {
    const int r = hook_int("PT_RAY_RESERVE", 0);
    return r < 0 ? 0 : r > 64 ? 64 : r;
}
// Byte counts: any base strtoull takes (0x..., 0...).
inline size_t hook_size(const char* name, size_t dflt) {
    const char* e = hook_env(name);
    return (e && *e) ? (size_t)strtoull(e, nullptr, 0) : dflt;
}
// PT_LDS_SCENE_BYTES: the most scene bytes a tree-walk kernel stages in LDS.
size_t lds_scene_budget();

// ---- LDS per CU. A block's LDS is rounded to kLdsGranule, and the occupancy query is optimistic
// about it: blocks of 27,072 B were reported to fit 6 per CU and ran 5 (-8 %), blocks of 26,816 B
// ran 6 (profiles/r03z_lds). So every block count is also checked against the measured bound
// (`usable`: pt_ctx::lds_usable, kLdsUsable on gfx950).
inline size_t lds_round(size_t bytes) { return (bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule; }
inline int lds_blocks(size_t usable, size_t bytes) { return (int)(usable / lds_round(bytes)); }  // bytes > 0

// Blocks of kBlock lanes with lds_bytes of dynamic LDS that run per CU: the occupancy query,
// clamped by lds_blocks (0: such a block does not fit; the top-of-tree shrink needs to see that).
// The clamp is skipped when lds_bytes or lds_usable is 0. (The shrink loop once clamped without
// that guard; pt_ctx_create never leaves lds_usable at 0, so the two forms agree.) `kernel`: a
// __global__ function's address. `what` names the caller in the error.
int occupancy(const void* kernel, size_t lds_bytes, size_t lds_usable, int* blocks, const char* what);
// occupancy, at least 1 (*per_cu), and with `grid` the launch's blocks for `count` lanes: at most
// per_cu * num_cus, at least 1 (grid may be NULL: a render sizes each launch's grid itself). The
// _module form takes a hipFunction_t (the hipRTC scene kernel).
int plan_grid(const void* kernel, size_t lds_bytes, size_t lds_usable, int num_cus, int64_t count, int* per_cu,
              int* grid, const char* what);
int plan_grid_module(void* function, size_t lds_bytes, size_t lds_usable, int num_cus, int64_t count, int* per_cu,
                     int* grid, const char* what);

// ---- device buffers that only grow: *p holds at least n elements afterwards (*cap: its
// capacity in elements; at least one element is allocated).
int ensure_bytes(void** p, size_t* cap, size_t n, size_t elem_bytes);
template <class T>
int ensure(T** p, size_t* cap, size_t n) {
    return ensure_bytes(reinterpret_cast<void**>(p), cap, n, sizeof(T));
}

// ---- a part of an image (pt_part_rows): validated shape of the rows a call renders.
struct PartShape {
    int W, H;         // camera resolution
    int parts, band;  // part_count and band_rows with their defaults (1)
    int rows, npix;   // this part's rows, rows * W (at most 2^30)
};
// Checked in this order: resolution, part_index, prm->depth against max_depth (a render passes
// PT_MAX_DEPTH; < 0: the caller traces no paths, depth is not looked at), the pixel count.
int part_shape(const pt_camera* cam, const pt_params* prm, int max_depth, PartShape* out);
// The fields camera_ray and part_row read: camera, partition, npix, W, seed and the three FastDivs.
void fill_camera(TraceArgs& A, const pt_camera* cam, const PartShape& shape, const pt_params* prm);

// ---- the work pool of one launch (TraceArgs::chunk, static_items, static_base).
struct PoolSizing {
    int chunk;
    uint32_t static_items;
    unsigned long long static_base;
};
// floor_items: the smallest refill while the launch is large enough (512 on the flat kernels,
// 128 on the wide and binary walks). Tuning hooks: PT_POOL_CHUNK, PT_POOL_REFILLS,
// PT_STATIC_MODE, PT_STATIC_FRAC.
PoolSizing pool_sizing(unsigned long long total_items, int grid, int floor_items);

// ---- scene predicates (on the packed scene, before its upload)
// Whether a scene takes the flat path: the hipRTC compile, the choice of the flat
// kernels and pt_rtc_check go by this one rule.
bool flat_eligible(const PackedScene& m);
bool scene_has_specular(const PackedScene& ps);  // a SPECULAR material: the sampler is compiled in
bool scene_dark(const PackedScene& ps);          // finish_path may skip paths that end at +0 (§3.9)
bool albedo_x2_ok(const PackedScene& ps);        // the flat kernel may unwind with pre-doubled albedo
// The last-ray rule (§3.15): on in a dark scene (`dark`: scene_dark), with the union of the leaf
// boxes that hold an EMIT triangle. Test hook PT_EMIT_REJECT=0 turns it off.
EmitBox scene_emit_box(const PackedScene& ps, bool dark);
// TraceArgs::emit_on for a box: 0 off, else which form the flat kernels run (kEmitSlab,
// kEmitSignOnly, kEmitSlabEmpty in pt_trace.h); the tree and wide kernels read it as on / off.
int emit_mode(const EmitBox& e);

// ---- the binary walk of pt_query.hip and pt_paths.hip.
// Where a launch keeps the scene, the walk's stack and the path records, and its grid.
struct WalkPlan {
    int lds_scene, lds_stack, lds_rec;  // 1: in LDS; 0: read through L1/L2 / rows in a global buffer
    int rows;                           // stack rows per lane = max(1, tree depth)
    int rec;                            // path records per lane (depth - 1; 0 for queries)
    int grid;                           // blocks of kBlock lanes
    size_t lds_bytes;                   // dynamic LDS per block
    size_t stack_ints;                  // ints the global stack buffer must hold (0 with the stack in LDS)
    size_t rec_words;                   // 32-bit words EACH of the two global record arrays must hold
};
// Placement (no HIP call; fills lds_*, rows, rec, lds_bytes): stack rows (kBlock x 4 B each), then
// the scene (2 float4 per node and tri_f4 per triangle: 3 for queries, 5 with materials), then
// rec_rows record rows (kBlock x 8 B each); each goes to LDS while it fits
// cap = min(64 KiB, lds_usable / 2) in 256-B granules beside what is already there — two blocks
// per CU, inside what a launch gets without an opt-in — and the scene also only within
// scene_budget. Whatever does not fit is read and written through L1/L2.
void place_walk(int num_nodes, int num_tris, int tree_depth, int tri_f4, int rec_rows, size_t lds_usable,
                size_t scene_budget, bool allow_stack, bool allow_rec, WalkPlan& out);
// place_walk under the hooks: PT_LDS_SCENE_BYTES (the budget), PT_QUERY_LDS_STACK=0 and, where
// `records`, PT_TRACE_LDS_REC=0 (test hooks) force the global buffers.
void place_walk_hooked(int num_nodes, int num_tris, int tree_depth, int tri_f4, int rec_rows, size_t lds_usable,
                       bool records, WalkPlan& out);
// plan_grid for `items` lanes, and the global buffers of what place_walk left out of LDS.
int walk_grid(const void* kernel, size_t lds_usable, int num_cus, int64_t items, WalkPlan& plan, const char* what);

}  // namespace pt
