// pt_launch.hip — the host's launch rules (pt_launch.h). No kernel is defined here: the file is
// compiled as HIP only because TraceArgs and the block constants live in pt_trace.h.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "pt_launch.h"
#include "pt_trace.h"

namespace pt {

size_t lds_scene_budget() { return hook_size("PT_LDS_SCENE_BYTES", 32 * 1024); }

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

namespace {

int clamped(hipError_t e, int n, size_t lds_bytes, size_t lds_usable, int* blocks, const char* what) {
    if (e != hipSuccess) return set_error(PT_E_HIP, "%s occupancy failed: %s", what, hipGetErrorString(e));
    if (lds_bytes > 0 && lds_usable > 0) n = std::min(n, lds_blocks(lds_usable, lds_bytes));
    *blocks = n;
    return PT_OK;
}

}  // namespace

int occupancy(const void* kernel, size_t lds_bytes, size_t lds_usable, int* blocks, const char* what) {
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kBlock, lds_bytes);
    return clamped(e, n, lds_bytes, lds_usable, blocks, what);
}

namespace {

void grid_from(int blocks, int num_cus, int64_t count, int* per_cu, int* grid) {
    blocks = std::max(1, blocks);
    *per_cu = blocks;
    if (grid)
        *grid = (int)std::max<int64_t>(1, std::min<int64_t>((count + kBlock - 1) / kBlock, (int64_t)blocks * std::max(1, num_cus)));
}

}  // namespace

int plan_grid(const void* kernel, size_t lds_bytes, size_t lds_usable, int num_cus, int64_t count, int* per_cu,
              int* grid, const char* what) {
    int blocks = 0;
    if (int rc = occupancy(kernel, lds_bytes, lds_usable, &blocks, what)) return rc;
    grid_from(blocks, num_cus, count, per_cu, grid);
    return PT_OK;
}

int plan_grid_module(void* function, size_t lds_bytes, size_t lds_usable, int num_cus, int64_t count, int* per_cu,
                     int* grid, const char* what) {
    int n = 0, blocks = 0;
    const hipError_t e = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&n, (hipFunction_t)function, kBlock, lds_bytes);
    if (int rc = clamped(e, n, lds_bytes, lds_usable, &blocks, what)) return rc;
    grid_from(blocks, num_cus, count, per_cu, grid);
    return PT_OK;
}

int ensure_bytes(void** p, size_t* cap, size_t n, size_t elem_bytes) {
    if (*cap >= n && *p) return PT_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const hipError_t e = hipMalloc(p, std::max<size_t>(n, 1) * elem_bytes);
    if (e != hipSuccess) return set_error(PT_E_HIP, "hipMalloc of %zu bytes failed: %s", n * elem_bytes, hipGetErrorString(e));
    *cap = n;
    return PT_OK;
}

int part_shape(const pt_camera* cam, const pt_params* prm, int max_depth, PartShape* out) {
    PartShape s;
    s.W = cam->res[0];
    s.H = cam->res[1];
    if (s.W <= 0 || s.H <= 0) return set_error(PT_E_ARG, "camera resolution must be positive");
    s.parts = prm->part_count > 0 ? prm->part_count : 1;
    s.band = prm->band_rows > 0 ? prm->band_rows : 1;
    if (prm->part_index < 0 || prm->part_index >= s.parts) return set_error(PT_E_ARG, "part_index out of range");
    if (max_depth >= 0 && prm->depth > max_depth) return set_error(PT_E_ARG, "depth %d exceeds PT_MAX_DEPTH", prm->depth);
    s.rows = pt_part_rows(s.H, prm->part_index, s.parts, s.band);
    const long long npix = (long long)s.rows * s.W;
    if (npix > (1ll << 30)) return set_error(PT_E_ARG, "too many pixels for one part");
    s.npix = (int)npix;
    *out = s;
    return PT_OK;
}

void fill_camera(TraceArgs& A, const pt_camera* cam, const PartShape& shape, const pt_params* prm) {
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
    A.W = shape.W;
    A.npix = shape.npix;
    A.part_index = prm->part_index;
    A.part_count = shape.parts;
    A.band_rows = shape.band;
    A.seed = prm->seed;
    A.div_npix = make_fastdiv((uint32_t)std::max(shape.npix, 1));
    A.div_w = make_fastdiv((uint32_t)shape.W);
    A.div_band = make_fastdiv((uint32_t)shape.band);
}

PoolSizing pool_sizing(unsigned long long total_items, int grid, int floor_items) {
    // Refill size: kChunk, or less when the launch holds too few items for every wave
    // to get ~128 refills, so that the launch's drain (waves finishing their last pool)
    // stays short: config 4's 8-GPU share (131k pixels x 1000 spp, 166-item refills)
    // 1.047 / 1.044 of ideal at ~4 refills, 1.036 / 1.031 at 64, then with the scaled step
    // bar 1.026-1.028 at 64 and 1.023-1.024 at 128; whole frames unchanged (their refills
    // stay at kChunk; profiles/r06_pool). At least 64: one refill must cover a whole wave's
    // claims (claim_work). Smaller refills only at the end of a launch (a second counter)
    // measured slower: the waves then contend on it (profiles/r06_drain/pool_tail_rejected.json).
    // (PT_POOL_CHUNK and PT_POOL_REFILLS are decimal only, unlike hook_size's byte counts.)
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
    const unsigned long long waves = (unsigned long long)grid * (kBlock / kWave);
    const unsigned long long floor_chunk = std::min<unsigned long long>(max_chunk, (unsigned long long)floor_items);
    PoolSizing p;
    p.chunk = (int)std::max<unsigned long long>(
        kWave, std::min<unsigned long long>(max_chunk, std::max<unsigned long long>(floor_chunk, total_items / (waves * refills))));
    // Static start: each wave's first pool needs no atomic. Large launches: one refill's
    // worth (the claims then stay in order, so the waves of a CU trace neighbouring
    // items); small ones (an even share under 4 kChunk items): the whole even share,
    // the remainder (< one item per wave) claimed in refills. Config 1's kernel: 0.39
    // (mode 0) -> 0.30 (mode 1) -> 0.19 ms (mode 2); configs 2 and 4 unchanged (+0.1 %).
    // Tuning hooks: PT_STATIC_MODE 0 off, 1 one refill always, 2 (default) as above;
    // PT_STATIC_FRAC the small-launch share (0.9: 0.21 ms, 0.75: 0.24 ms).
    const unsigned long long share = total_items / waves;
    const char* sf = hook_env("PT_STATIC_FRAC");
    const int mode = hook_int("PT_STATIC_MODE", 2);
    const double frac = (sf && *sf) ? std::max(0.0, std::min(1.0, atof(sf))) : 1.0;
    unsigned long long st = std::min<unsigned long long>((unsigned long long)p.chunk, share);
    if (mode == 2 && share < 4ull * kChunk) st = std::max(st, (unsigned long long)((double)share * frac));
    if (mode == 0) st = 0;
    p.static_items = (uint32_t)st;
    p.static_base = waves * st;  // <= total_items < 2^31
    return p;
}

void place_walk(int num_nodes, int num_tris, int tree_depth, int tri_f4, int rec_rows, size_t lds_usable,
                size_t scene_budget, bool allow_stack, bool allow_rec, WalkPlan& out) {
    const size_t cap = std::min<size_t>(64 * 1024, lds_usable / 2);
    out.rows = std::max(1, tree_depth);
    out.rec = rec_rows;
    const size_t stack_b = sizeof(int) * (size_t)kBlock * out.rows;
    out.lds_stack = allow_stack && lds_round(stack_b) <= cap;
    size_t used = out.lds_stack ? stack_b : 0;
    const size_t scene_b = sizeof(float4) * (2 * (size_t)num_nodes + (size_t)tri_f4 * (size_t)num_tris);
    out.lds_scene = scene_b <= scene_budget && lds_round(scene_b + used) <= cap;
    used += out.lds_scene ? scene_b : 0;
    const size_t rec_b = 2 * sizeof(int) * (size_t)kBlock * out.rec;
    out.lds_rec = allow_rec && lds_round(used + rec_b) <= cap;
    used += out.lds_rec ? rec_b : 0;
    out.lds_bytes = used;
}

void place_walk_hooked(int num_nodes, int num_tris, int tree_depth, int tri_f4, int rec_rows, size_t lds_usable,
                       bool records, WalkPlan& out) {
    place_walk(num_nodes, num_tris, tree_depth, tri_f4, rec_rows, lds_usable, lds_scene_budget(),
               !hook_off("PT_QUERY_LDS_STACK"), records && !hook_off("PT_TRACE_LDS_REC"), out);
}

int walk_grid(const void* kernel, size_t lds_usable, int num_cus, int64_t items, WalkPlan& plan, const char* what) {
    int per_cu = 0;
    if (int rc = plan_grid(kernel, plan.lds_bytes, lds_usable, num_cus, items, &per_cu, &plan.grid, what)) return rc;
    plan.stack_ints = plan.lds_stack ? 0 : (size_t)plan.grid * plan.rows * kBlock;
    plan.rec_words = plan.lds_rec ? 0 : (size_t)plan.grid * plan.rec * kBlock;
    return PT_OK;
}

// ---- scene predicates
// Whether a scene takes the flat path: at most kMaxFlatLeaves leaves, and
// triangle ranks that fit the path records' 16 bits. pt_ctx_set_scene starts the hipRTC
// compile, plan_render picks the flat kernels and pt_rtc_check compiles by this one rule.
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
    if (hook_off("PT_DARK")) return false;
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

// The last-ray rule's box (shade, pt_trace.h; the proof is with emit_reject, pt_math.h): the union
// E of the leaf boxes of every leaf that holds an EMIT triangle. The boxes are the binary
// tree's leaf nodes, which are the boxes every kernel form and the reference test before a
// triangle: the flat list copies them (pack_scene), the wide tree stores them with its
// triangles (or forms the same box from a single triangle's vertices), and a caller-built
// tree's leaf box may be larger than its triangles. An ancestor's box failing only removes
// more tests, so a ray that fails every emitter leaf box tests no emitter triangle.
// Only dark scenes (scene_dark): the last segment then returns +0 for anything but an emitter
// and the levels above it unwind +0 to +0. Emitters may have any emission. A NaN in an
// emitter leaf's box (the proof orders the planes) turns the rule off.
EmitBox scene_emit_box(const PackedScene& ps, bool dark) {
    EmitBox e;
    if (!dark || hook_off("PT_EMIT_REJECT")) return e;
    for (int a = 0; a < 3; a++) {
        e.lo[a] = std::numeric_limits<float>::infinity();
        e.hi[a] = -std::numeric_limits<float>::infinity();
    }
    const size_t ntri = ps.mats.size() / 2;
    for (size_t n = 0; 2 * n + 1 < ps.nodes.size(); n++) {
        const f4 p = ps.nodes[2 * n], q = ps.nodes[2 * n + 1];
        const int a = __builtin_bit_cast(int, q.z), b = __builtin_bit_cast(int, q.w);
        if (a >= 0) continue;  // interior
        bool emits = false;
        for (int i = -a - 1; i <= b && i >= 0 && (size_t)i < ntri; i++)
            if (__builtin_bit_cast(int, ps.mats[2 * (size_t)i].x) == PT_MAT_EMIT) emits = true;
        if (!emits) continue;
        const float lb[3] = {p.x, p.y, p.z}, rt[3] = {p.w, q.x, q.y};
        for (int ax = 0; ax < 3; ax++) {
            if (!(lb[ax] <= rt[ax])) return EmitBox();  // NaN or an inverted box: no claim
            e.lo[ax] = std::min(e.lo[ax], lb[ax]);
            e.hi[ax] = std::max(e.hi[ax], rt[ax]);
        }
    }
    e.on = true;
    // the flat kernels use the slab test of E (emit_slab_reject); PT_EMIT_REJECT=sign keeps them
    // on the sign rule alone (the scene kernel through PT_EMIT_SIGN_ONLY in its source, the table
    // kernels through TraceArgs::emit_on): the A/B of the two rules
    const char* h = hook_env("PT_EMIT_REJECT");
    e.sign_only = h && strcmp(h, "sign") == 0;
    return e;
}

int emit_mode(const EmitBox& e) {
    if (!e.on) return 0;
    if (e.sign_only) return kEmitSignOnly;
    return emit_box_empty(v3{e.lo[0], e.lo[1], e.lo[2]}, v3{e.hi[0], e.hi[1], e.hi[2]}) ? kEmitSlabEmpty : kEmitSlab;
}

// Whether the flat kernel may unwind with pre-doubled albedo (finish_path<., true>: L * 2a
// instead of (2L) * a, the same bits while 2L cannot overflow). Requires every material
// finite with |2 * albedo| finite, and the radiance bound B_{j+1} = e + (2 a B_j) c over
// PT_MAX_DEPTH levels (a, e: the largest |albedo| and |emission| components, c: |cos| <= 1
// with a margin for rounding) below 2^125. PT_ALBEDO_X2=0 (test hook) turns it off.
bool albedo_x2_ok(const PackedScene& ps) {
    if (hook_off("PT_ALBEDO_X2")) return false;
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

}  // namespace pt

// Test hook (no device needed): place_walk under the hooks, as pt_ctx_trace plans (pt_hip_debug.h).
extern "C" int pt_debug_walk_placement(int32_t num_nodes, int32_t num_tris, int32_t tree_depth, int32_t tri_f4,
                                       int32_t rec_rows, uint64_t lds_usable, int32_t out[4]) {
    if (!out || num_nodes < 0 || num_tris < 0 || tri_f4 < 0 || rec_rows < 0)
        return pt::set_error(PT_E_ARG, "pt_debug_walk_placement: bad argument");
    pt::WalkPlan p{};
    pt::place_walk_hooked(num_nodes, num_tris, tree_depth, tri_f4, rec_rows, (size_t)lds_usable, true, p);
    out[0] = p.lds_scene;
    out[1] = p.lds_stack;
    out[2] = p.lds_rec;
    out[3] = (int32_t)p.lds_bytes;
    return PT_OK;
}
