// pt_internal.h — what the translation units of libpt_hip.so share without HIP: errors and
// hooks, the packed scene (pt_host.cpp builds it, pt_kernel.hip uploads it), a few constants both
// sides must agree on, and the boundaries between pt_kernel.hip (pt_ctx and its entry points) and
// pt_multi.hip, pt_query.hip, pt_paths.hip, pt_flat_fast.hip. The launch rules those share are in
// pt_launch.h, the hipRTC scene kernel in pt_rtc.h; DESIGN.md §3 has the map of the host code.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "pt_hip.h"

namespace pt {

// Record the error message of the calling thread and return `code`.
int set_error(int code, const char* fmt, ...);

// Test / tuning hooks (PT_FLAT, PT_WIDE, PT_PAIRS, PT_BATCH_BYTES, ...): the value of
// environment variable `name`, or nullptr. Hooks are honoured only when PT_TEST_HOOKS=1
// was set when the library first looked (once per process), so a stray variable in a
// user's environment never changes which kernel or queue size the product runs.
const char* hook_env(const char* name);

struct f4 {
    float x, y, z, w;
};

// Magic numbers of the kernels' division by a launch constant (FastDiv, pt_trace.h; pt_launch.hip).
struct FastDiv;
FastDiv make_fastdiv(uint32_t d);
// pt_launch.h: where the binary walk keeps its data (WalkPlan) and a part's validated shape.
struct WalkPlan;
struct PartShape;

// Device layout of a scene (see DESIGN.md "Data layout in HBM"):
//   nodes: 2 x f4 per node   {lb.xyz, rt.x}, {rt.y, rt.z, a, b}, renumbered so that the two
//          children of every interior node are adjacent (left = a, right = a + 1; the
//          reference builder already emits them so, bvh.h:142-152). Root = node 0.
//          interior: a = left (>= 1), b = 0; leaf: a = -(tri_start+1), b = tri_end
//          (bit-cast ints). Traversal order depends only on the tree, not on numbering.
//   tris : 3 x f4 per tri_idx POSITION i (triangle tri_idx[i]):
//          {v1.xyz, e1.x}, {e1.yz, e2.xy}, {e2.z, n.xyz}   e1 = v2-v1, e2 = v3-v1,
//          n = normalize(cross(e1, e2)) (triangle.h:28-29, 46-47), computed on the host
//   mats : 2 x f4 per position {type, color.rgb}, {emit.rgb, roughness}
//   Triangle positions are renumbered into the reference's visit RANK: the order in
//   which BVH::intersect would test them if every box passed (right subtree first,
//   bvh.h:177-178; ascending tri_idx position inside a leaf). The first strict minimum
//   in rank order is then the reference's winner for any traversal order.
//   leaves: 2 x f4 per leaf in rank order {lb.xyz, rt.x}, {rt.y, rt.z, first, last}
//          (first/last = rank positions, bit-cast ints) — the flat leaf list.
//   wide: the binary tree collapsed into nodes of `wide_width` (4 or 8) children with
//          quantised child boxes, built only when the flat-leaf argument holds
//          (partition + containment). Nodes in BFS order (root 0; the first levels
//          form an index prefix, staged in LDS by the kernel); the inner children of a
//          node are consecutive nodes from child_base, slots [0, ni); its leaf children
//          follow in slots [ni, ni + nl), their triangles consecutive in `wtris` from
//          leaf_base. Per node kWideNodeU4[W] uint4:
//            [0] O.x O.y O.z (float), meta = (ex+128) | (ey+128) << 8 | (ez+128) << 16
//                | ni << 24 | nl << 28
//            [1] child_base, leaf_base, end[0..3], end[4..7] (bytes: cumulative end
//                offset of leaf k's triangles from leaf_base)
//            [2..] per axis a (x, y, z), `wide_fmt` kWideF16 (default): binary16 integers
//                lo.a[W] hi.a[W] in 0..2047, so a ray reads its entry run at lo or hi
//                and its exit run at the other (the sign of its 1 / d); otherwise bytes
//                lo.a[W] hi.a[W] hi.a[W] lo.a[W] in 0..255, one (entry, exit) run.
//                8-wide: 128 B per node, one cache line, in either format.
//          Child box on axis a: [O + lo * 2^e, O + hi * 2^e] (reals), containing the
//          reference's child box; the kernel's test is conservative,
//          exactness comes from the exact leaf box checked on every triangle hit.
//          `wide_fmt` kWideF32 (round 6): no quantisation — the child
//          planes are the reference's own float boxes. Per node 1 + 3 W / 2 uint4:
//            [0] child_base | ni << 24 | nl << 28, leaf_base, end[0..3], end[4..7]
//            [1..] per axis a: lo.a[W] hi.a[W] (float; an empty slot lo = +inf, hi = -inf)
//          8-wide: 208 B per node; 4-wide: 112 B.
//   wtris: 4 x f4 per triangle in wide-leaf order: {v1.xyz, e1.x}, {e1.yz, e2.xy},
//          {e2.z, rank (bits), leaf lb.xy}, {leaf lb.z, leaf rt.xyz}; or, when every
//          leaf holds one triangle (`wide_compact`), 3 x f4: {v1.xyz, rank (bits)},
//          {v2.xyz, v3.x}, {v3.yz, 0, 0} (edges and the leaf box formed by the kernel).
//   nrm  : (wide path) 1 x f4 per rank position {n.xyz, material id (bits)}: the shading
//          normal and the row of the triangle's material in `umats`
//   umats: (wide path) 2 x f4 per DISTINCT material, same layout as `mats` (the wide
//          kernel keeps them in LDS when there are at most kMaxLdsMaterials)
// Child-plane formats of the wide tree.
constexpr int kWideByte = 0, kWideF16 = 1, kWideF32 = 2;
constexpr int kWideNodeU4(int W, int fmt) { return fmt == kWideF32 ? 1 + 3 * W / 2 : W == 8 ? 8 : 5; }
constexpr int kMaxLdsMaterials = 64;
// With the table in LDS the path records hold a material row in ONE byte (trace_body_wide):
// the LDS form is only ever chosen for at most kMaxLdsRowsByte rows, whatever the tuning hook.
constexpr int kMaxLdsRowsByte = 256;
static_assert(kMaxLdsMaterials <= kMaxLdsRowsByte, "LDS material rows must fit the 8-bit path records");
// LDS per CU the blocks of one kernel can count on, and the granule a block's LDS is
// rounded to: 6 blocks of 26,816 B run together, 6 of 27,072 B do not (measured on the wide
// kernel on gfx950 / MI355X, profiles/r03z_lds), although 160 KiB would hold them. Applied
// only on that architecture, and never above the device's reported LDS per CU
// (pt_ctx::lds_usable, set in pt_ctx_create; lds_blocks, pt_launch.h).
constexpr size_t kLdsUsable = 161280;
constexpr size_t kLdsGranule = 256;
// trace() on caller-supplied rays (pt_bvh_trace, pt_ctx_trace): the bound on material.h:20-23's
// rejection loop (kMaxSpecularIters of the kernels) and the most samples per ray, so that one
// ray's records always fit a launch (pt_ctx_trace cuts launches over rays only).
constexpr int kSpecularIterBound = 1 << 16;
constexpr int kTraceMaxSpp = 1 << 20;
// The depth and spp ranges every entry point that traces caller-supplied rays checks (`who`: its name).
inline int trace_params_check(const char* who, const pt_trace_params* prm) {
    if (prm->depth < 0 || prm->depth > PT_MAX_DEPTH)
        return set_error(PT_E_ARG, "%s: depth %d outside 0..%d", who, prm->depth, PT_MAX_DEPTH);
    if (prm->spp < 1 || prm->spp > kTraceMaxSpp)
        return set_error(PT_E_ARG, "%s: spp %d outside 1..%d", who, prm->spp, kTraceMaxSpp);
    return PT_OK;
}
constexpr int kPairQueueMin = 256;  // shortest flat pair queue (entries per wave) the launch picks for occupancy

struct PackedScene {
    std::vector<f4> nodes, tris, mats, leaves, wide, wtris, nrm, umats;
    std::vector<int32_t> rank_tri;  // rank position -> index into the caller's triangles (tri_idx of that
                                    // position): what BVH::intersect returns for a hit there (bvh.h:173)
    int32_t num_umats = 0;
    int32_t num_leaves = 0;
    int32_t num_wide = 0, wide_width = 0;
    int32_t wide_depth = 0;  // wide levels; the walk holds at most wide_depth - 1 pending stack entries
                             // (one per level above the current node; the last level has no inner nodes)
    int32_t wide_top = 0;    // nodes of the first wide levels that fit the LDS top-of-tree budget
    int32_t wide_fmt = kWideByte;  // child planes: bytes 0..255, binary16 integers 0..2047, or floats
    float wide_span[3] = {0, 0, 0};  // kWideF32: max |plane| per axis (the per-ray margin's bound)
    bool wide_single = false;  // every wide leaf holds exactly one triangle (BVH::build's output)
    bool wide_compact = false;  // wtris holds the 3-f4 records of single-triangle leaves
    int32_t num_nodes = 0, num_tris = 0;
    int32_t stack_size = 0;  // max LIFO occupancy of BVH::intersect over this tree
    int32_t tree_depth = 0;  // max root-to-leaf edge count (child-pair traversal stack bound)
    bool coords_small = false;  // every vertex coordinate below 2^60 in magnitude (tri_hit_nb's precondition)
};

// The last-ray rule's emitter box (scene_emit_box in pt_launch.h): the union
// of the tree's leaf boxes that hold an EMIT triangle; lo = +inf, hi = -inf when there is none.
struct EmitBox {
    bool on = false;  // the rule applies (a dark scene; PT_EMIT_REJECT=0 turns it off)
    bool sign_only = false;  // test hook PT_EMIT_REJECT=sign: the flat kernels keep the sign rule alone
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
};

// Validate the node graph and pack it. Returns PT_OK or an error code.
int pack_scene(const pt_scene* s, PackedScene& out);

// A context's HIP stream (hipStream_t) and device gamma/quantisation (pt_kernel.hip):
// `rows` x W linear pixels at d_lin -> bytes at d_dst (flip: last row first); synchronous.
void* ctx_stream(pt_ctx* c);
int rgb8_device(pt_ctx* c, const float* d_lin, int rows, int W, float gamma, int flip, uint8_t* d_dst);
// The flat path's table kernel with a scene's flags baked in (pt_flat_fast.hip): every leaf one
// triangle, coordinates below 2^60, a dark scene with pre-doubled albedo; `specular`: the scene
// holds a SPECULAR material, `mask32`: at most 32 leaves. A __global__ function's address.
void* flat_fast_kernel(bool specular, bool mask32);
// Free a context's radiance slabs and flag words (allocated again by its next render).
int ctx_release_slabs(pt_ctx* c);
// pt_debug_counter's context counters (pt_kernel.hip): 0 contexts created, 1 scene uploads.
int64_t kernel_counter(int which);

// ---- ray queries and first-hit AOVs (pt_query.hip; the entry points are in pt_kernel.hip) ----
// A scene as the query kernels read it: device arrays in the layout above.
struct QueryScene {
    const f4* nodes;
    const f4* tris;
    const f4* mats;
    const int32_t* rank_tri;
    int32_t num_nodes, num_tris, tree_depth;
};
// which: 0 closest hit, 1 any hit, 2 AOV. `count`: rays or pixels of the largest launch.
int query_plan(int which, const QueryScene& sc, size_t lds_usable, int num_cus, int64_t count, WalkPlan& plan);
// One launch over n rays (device pointers) on `stream` (a hipStream_t); no synchronisation.
// `hits` (device): incremented by the number of rays that hit / are occluded.
int query_launch(void* stream, const QueryScene& sc, const WalkPlan& plan, int any, const float* org, const float* dir,
                 const float* tmax, int32_t n, float* t_out, int32_t* out, int* gstack, unsigned long long* hits,
                 int force_exact);
// One launch over the pixels of a part (shape: part_shape of cam and prm, pt_launch.h); `out` holds device pointers, NULL = channel skipped.
int aov_launch(void* stream, const QueryScene& sc, const WalkPlan& plan, const pt_camera* cam, const pt_params* prm,
               const PartShape& shape, int32_t sample, const pt_aov* out, int* gstack, unsigned long long* hits,
               int force_exact);

// ---- trace() on caller-supplied rays (pt_paths.hip; the entry point is in pt_kernel.hip) ----
// `items`: rays x samples of the largest launch; depth >= 1.
int paths_plan(const QueryScene& sc, size_t lds_usable, int num_cus, int depth, int64_t items, WalkPlan& plan);
// One launch over m rays x spp samples (device pointers; m * spp < 2^31); no synchronisation.
struct PathsLaunch {
    const float* org;         // m x 3
    const float* dir;         // m x 3
    const uint32_t* states;   // m x spp, or nullptr: pt_sample_seed(ray_base + i, s, seed)
    int32_t m, spp, depth;
    uint32_t seed, ray_base;
    float* slab;              // m * spp records of 3 floats, [sample][ray][rgb]
    unsigned long long* ctr;  // zeroed 4 x u64 (work head at [0]); ray count added at [1], runaway at [3]
    int* gstack;              // plan.stack_ints ints
    float* grec;              // 2 * plan.rec_words words: material rows, then cosines
    const void* theta_tab;    // the device's theta table (float2), or nullptr
    int theta_lanes, dark, force_exact;
};
int paths_launch(void* stream, const QueryScene& sc, const WalkPlan& plan, const PathsLaunch& l);

// ---- light sampling (pt_nee.h, pt_nee.hip; the host form is in pt_host.cpp, the entry points in pt_kernel.hip) ----
// The light table of a scene (include/pt_hip.h: the definition), made on the host by
// scene_light_table (pt_host.cpp) from the caller's arrays of a validated scene.
constexpr int kNeeLightF4 = 5;  // float4 per light in the geometry rows
struct LightTable {
    std::vector<int32_t> tri;     // the caller's triangle index of each light
    std::vector<float> cdf;       // running float32 sum of the areas; A = cdf.back()
    std::vector<f4> geom;         // kNeeLightF4 rows per light: v1, e1, e2, unit normal, emit_color (w = 0)
    std::vector<uint8_t> listed;  // per caller triangle: 1 when it is a light
    float area = 0.0f, kA = 0.0f; // A and A / (float)M_PI; both 0 without lights
};
void scene_light_table(const pt_scene* s, LightTable& out);
// The options of the *_nee_opt entry points (pt_host.cpp): *mis = PT_NEE_MIS_NONE for NULL, else
// opt->mis; PT_E_ARG for an unknown mode or a reserved word that is not 0.
int nee_options_check(const char* who, const pt_nee_options* opt, int* mis);
// The table on a device (pt_kernel.hip uploads it on the first light-sampling call after a scene is set).
struct NeeLights {
    const float* cdf;
    const int32_t* tri;
    const f4* geom;
    const uint8_t* listed;
    int32_t count;
    float area, kA;
};
// paths_plan for the light-sampling kernels (no path records); camera: the part's camera rays;
// mis: PT_NEE_MIS_* (the weighted estimator has kernels of its own, and so an occupancy of its own).
int nee_plan(bool camera, int mis, const QueryScene& sc, size_t lds_usable, int num_cus, int64_t items, WalkPlan& plan);
// One launch over l.m rays (or, with cam, the first l.m pixels of the part) x l.spp samples from
// sample s_begin; l.ctr: 6 zeroed u64, [4] shadow segments and [5] light draws added. l.grec is not read.
int nee_launch(void* stream, const QueryScene& sc, const WalkPlan& plan, const PathsLaunch& l, const NeeLights& lights,
               int mis, int32_t s_begin, const pt_camera* cam, const pt_params* prm, const PartShape* shape);

// ---- per-pixel rounds of pt_ctx_render_adaptive (pt_adaptive.hip; the host loop is in pt_kernel.hip) ----
// All on `stream` (a hipStream_t), device pointers, no synchronisation. Lists hold part-local pixel indices.
// paths_plan for the kernel fed from a list; `items`: listed pixels x samples of the largest launch.
int adaptive_plan(const QueryScene& sc, size_t lds_usable, int num_cus, int depth, int64_t items, WalkPlan& plan);
// Samples [s_begin, s_begin + l.spp) of the l.m pixels of `list`, traced as a render traces them
// (camera_ray; cam, prm and shape as the render's): record j of l.slab is sample s_begin + j / l.m
// of pixel list[j % l.m]. l.org, l.dir, l.states and l.ray_base are not read.
int adaptive_launch(void* stream, const QueryScene& sc, const WalkPlan& plan, const PathsLaunch& l, const int32_t* list,
                    int32_t s_begin, const pt_camera* cam, const pt_params* prm, const PartShape& shape);
// The m pixels of `prev` (nullptr: pixels 0..m-1) that miss the criterion (pt_moments.h) after n
// samples -> `list` (another buffer of m entries, order unspecified), their number -> *count
// (zeroed here); spp[q] = n for those that meet it. mom: the context's S and Q over npix pixels.
int adaptive_compact(void* stream, const int32_t* prev, int32_t m, const double* mom, int32_t npix, int32_t n, float rel,
                     float abs_tol, int32_t* list, unsigned long long* count, int32_t* spp);
// spp[list[i]] = n for i < m (list nullptr: spp[i] = n).
int adaptive_fill_spp(void* stream, const int32_t* list, int32_t m, int32_t n, int32_t* spp);
// A launch's slab (c samples of the m listed pixels) added in sample order to the pixels' float32
// sums (accum, planes of npix) and double sums (mom); n_new > 0: out[q] = sum / n_new as well.
int adaptive_accumulate(void* stream, const float* slab, const int32_t* list, int32_t m, int32_t c, float* accum,
                        double* mom, float* out, int32_t npix, int32_t n_new);
// The standard error of the mean of nval = 3 npix values, each with its pixel's n = spp[pixel].
int adaptive_sem(void* stream, const double* mom, size_t nval, const int32_t* spp, float* sem);

// ---- the a-trous denoiser (pt_denoise.h, pt_denoise.hip; the host form is in pt_host.cpp) ----
struct DnParams;
// The arguments every form checks, and pt_denoise_params with its defaults filled in (pt_host.cpp).
int denoise_check(const char* who, int32_t W, int32_t H, const float* color, const float* var,
                  const pt_denoise_guides* g, const pt_denoise_params* prm, const float* out, const float* var_out,
                  DnParams* P);
// The denoiser's scratch on the context's device, kept by the context and freed with it
// (pt_kernel.hip): buffer `slot` (0 records and ping-pong, 1 a host-pointer call's staging,
// 2 pt_ctx_render_denoised's images and guides) grown to `bytes`. Waits for the context's stream
// to exist and selects its device.
// Slots 3..6 are the temporal reprojection's (pt_temporal.hip): 3 its counter and a host-pointer
// call's staging, 4 and 5 the context's two histories, 6 pt_ctx_render_temporal's frame.
constexpr int kDnScratchSlots = 7;
int ctx_scratch(pt_ctx* c, int slot, size_t bytes, void** out);
// position = o + d * t per component of an AOV's rays (6 floats per pixel) on `stream`; no synchronisation.
int dn_position_launch(void* stream, const float* ray, const float* t, size_t npix, float* pos);

// ---- temporal reprojection (pt_temporal.h, pt_temporal.hip; the host form is in pt_host.cpp) ----
struct TpParams;
// The arguments every form checks, and pt_temporal_params with its defaults filled in (pt_host.cpp).
int temporal_check(const char* who, int32_t W, int32_t H, const pt_camera* cam_cur, const pt_camera* cam_prev,
                   const float* color, const float* var, const pt_denoise_guides* g, const pt_temporal_history* prev,
                   const pt_temporal_history* next, const pt_temporal_params* prm, TpParams* P);
// What a context keeps between two pt_ctx_render_temporal calls (pt_kernel.hip owns it and ends it
// in pt_ctx_set_scene): the history in scratch slot 4 + `slot` was written for camera `cam`.
struct TemporalState {
    bool valid = false;
    int slot = 0;
    pt_camera cam{};
};
TemporalState* ctx_temporal_state(pt_ctx* c);

}  // namespace pt
