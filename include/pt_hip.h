/*
 * pt_hip.h — C ABI of the MI355X path-tracing hot path (libpt_hip.so).
 *
 * This is the drop-in boundary for the per-pixel trace loop of the reference
 * (Blackgaurd/pathtracer-cpp). Every entry point below replaces one interface
 * of the reference; the replaced interface is cited as file:line into the
 * reference tree (pathtracer/...):
 *
 *   pt_render_f32 / pt_ctx_render   <- render_cpu()  render.h:62-104 (loop 80-88)
 *                                     render_gpu()  render.h:109-152 (tile loop 128-139)
 *                                     trace()       render.h:36-61
 *   pt_bvh_intersect / pt_ctx_intersect <- BVH::intersect() bvh.h:156-183 (batched; closest and any hit)
 *   pt_bvh_trace / pt_ctx_trace <- trace() render.h:36-61 (batched, caller's rays)
 *   pt_bvh_trace_grad / pt_ctx_trace_grad: its exact gradient w.r.t. color and emit_color
 *   pt_ctx_render_aov                <- Camera::get_ray camera.h:63-73 + BVH::intersect + Triangle::normal
 *                                       triangle.h:45-49 (the first hit of a sample, per pixel)
 *   pt_ctx_render_moments / pt_ctx_unconverged / pt_ctx_render_converge: the render's per-pixel
 *                                       sample moments, their error estimate, rendering to a noise target
 *   pt_ctx_render_adaptive: the same with the later rounds only for the pixels that miss the target
 *   pt_image_temporal / pt_ctx_temporal / pt_ctx_render_temporal <- render_realtime()'s moving camera,
 *                                       render.h:219-387: frames accumulated across camera moves by reprojection
 *   pt_bvh_build                     <- BVH::build()  bvh.h:79-155 (find_best_axis 48-78)
 *   pt_camera_init                   <- Camera::Camera() camera.h:33-61
 *   pt_sample_seed                   <- rng.h:32 global LCG (stream policy, see below)
 *   pt_image_to_rgb8                 <- Image::gamma_correct + save_png quantisation
 *                                       image.h:41-62
 *
 * Plain C types only (no torch, no C++ types). All functions are synchronous
 * and must be called from one host thread per context. Return value: 0 on
 * success, a negative PT_E* code on failure; pt_last_error() describes it.
 *
 * Stream policy (the only intended behaviour change vs the reference): the
 * reference draws every random number from ONE global LCG (rng.h:32), which
 * makes pixel values depend on every earlier pixel and cannot be parallelised.
 * Here the same LCG (rng.h:14-20) is re-seeded before every sample with
 * pt_sample_seed(h*W + w, s, seed). trace()/get_ray()/the BVH are unchanged,
 * so with this seeding the GPU output is bit-identical to the reference's
 * render loop run with the same per-sample reseed (tests/golden).
 */
#ifndef PT_HIP_H
#define PT_HIP_H

#if !defined(__HIPCC_RTC__)  /* hipRTC (scene-specialised kernels) provides the fixed-width types */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 3

/* Reference constants (linalg.h:10-12, render.h:16, rng.h:3). */
#define PT_SEED 1u
#define PT_MAX_DEPTH 64          /* kernel limit on `depth` (reference GL path: 20, shader.h:35) */

/* Error codes. */
#define PT_OK 0
#define PT_E_ARG (-1)            /* invalid argument (null pointer, bad size, bad node graph) */
#define PT_E_EMPTY (-2)          /* no triangles in scene (render.h:64-67)                 */
#define PT_E_HIP (-3)            /* HIP runtime error (no device, launch failure, OOM)      */
#define PT_E_IO (-4)             /* file write failure (image.h:61)                         */
#define PT_E_RUNAWAY (-5)        /* specular rejection loop hit its bound   */

/* Material type values, identical to Material::Type (material.h:28-32). */
#define PT_MAT_EMIT 1
#define PT_MAT_DIFFUSE 2
#define PT_MAT_SPECULAR 3

/* BVHNode in the reference's own 40-byte AoS layout (bvh.h:12-16):
 * AABB {vec3 lb, rt} then int left, right, tri_start, tri_end.
 * Leaf <=> left == -1 && right == -1 (bvh.h:25-27). */
typedef struct pt_bvh_node {
    float lb[3];
    float rt[3];
    int32_t left, right;
    int32_t tri_start, tri_end;
} pt_bvh_node;

/* Material in the reference's 32-byte layout (material.h:27-37). */
typedef struct pt_material {
    int32_t type;                /* PT_MAT_* */
    float color[3];              /* albedo (surface_color, render.h:56) */
    float emit[3];               /* emit_color (render.h:45, 55)        */
    float roughness;             /* specular jitter scale (material.h:21) */
} pt_material;

/* A scene = the arrays a built BVH owns (bvh.h:32-34). Host pointers, caller-owned. */
typedef struct pt_scene {
    int32_t num_tris;
    const float* verts;          /* num_tris * 9 floats: v1, v2, v3 of triangle i (triangle.h:10) */
    const pt_material* materials;/* num_tris entries, material of triangle i                    */
    int32_t num_nodes;
    const pt_bvh_node* nodes;    /* num_nodes entries, root = 0                                 */
    const int32_t* tri_idx;      /* num_tris entries (bvh.h:33)                                  */
} pt_scene;

/* Camera parameters the ray generator reads (camera.h:19-25, get_ray 63-73),
 * precomputed on the host by pt_camera_init. transform holds the 3x3 rotation
 * rows right, up, -forward (camera.h:55-57). */
typedef struct pt_camera {
    float pos[3];
    int32_t res[2];              /* width, height */
    float v_res[2];
    float cell_size;
    float distance;
    float transform[9];          /* row-major 3x3 */
} pt_camera;

/* Progress of a render (optional, pt_params.progress): `done` of `total` pixel-samples
 * are complete. Called from the rendering call's own threads (one at a time, never
 * concurrently), with done increasing to total; the drop-in render_cpu / render_gpu turn
 * it into the reference's per-row / per-chunk console lines (render.h:87, 136). */
typedef void (*pt_progress_fn)(void* user, int64_t done, int64_t total);

/* Render parameters. */
typedef struct pt_params {
    int32_t spp;                 /* samples per pixel (render_*: `samples`) */
    int32_t depth;               /* max path segments (render_*: `depth`)   */
    uint32_t seed;               /* stream seed, PT_SEED for the reference  */
    int32_t part_index;          /* row partition for multi-GPU: this part  */
    int32_t part_count;          /*   number of parts (1 = whole image)     */
    int32_t band_rows;           /*   rows per band; row h belongs to part (h / band_rows) % part_count */
    int32_t batch_spp;           /* samples per accumulation batch (radiance slab of 12 B per
                                    sample and pixel), 0 = auto. With several batches two slabs
                                    alternate (fused accumulation) when both fit the slab budget;
                                    an explicit batch that does not fit twice is summed by a
                                    separate pass instead, never resized */
    int32_t samples_per_item;    /* samples per work item (lane-level scheduling unit), 0 = auto */
    pt_progress_fn progress;     /* NULL = no progress reports                */
    void* progress_user;         /*   its first argument                      */
} pt_params;

#define PT_MAX_DEVICES 16        /* devices of one pt_render_*_devices call */

/* Statistics of one render call. */
typedef struct pt_stats {
    uint64_t rays;               /* traced segments = BVH::intersect calls (bvh.h:156) */
    uint64_t paths;              /* camera samples */
    uint64_t runaway;            /* specular rejection loops that hit the bound (0 normally) */
    double kernel_ms;            /* sum of trace-kernel durations (HIP events); devices: the slowest part's */
    double reduce_ms;            /* sum of accumulate-kernel durations           */
    double total_ms;             /* end-to-end wall time of the call             */
    int32_t trace_launches;      /* number of trace-kernel launches              */
    int32_t rows;                /* rows rendered by this part                    */
    int32_t kernel_path;         /* PT_PATH_*: which trace kernel ran              */
    /* pt_render_*_devices only (zero otherwise): */
    int32_t n_devices;           /* parts = listed devices                                     */
    int32_t gather_path;         /* PT_GATHER_*: how the parts met                              */
    double gather_ms;            /* RCCL gather + row assembly on the first device (HIP events) */
    double device_kernel_ms[PT_MAX_DEVICES];  /* per part: trace-kernel time                  */
    double device_render_ms[PT_MAX_DEVICES];  /* per part: context + scene upload + render    */
    uint64_t device_rays[PT_MAX_DEVICES];     /* per part: traced segments                    */
} pt_stats;

/* pt_stats.gather_path values. */
#define PT_GATHER_NONE 0         /* single context                                          */
#define PT_GATHER_RCCL 1         /* RCCL send/recv group to the first device + device assembly */
#define PT_GATHER_HOST 2         /* parts copied to the host, rows placed there (a device listed
                                    twice, or PT_TEST_HOOKS=1 PT_GATHER=host) */
#define PT_GATHER_HOST_FALLBACK 3 /* as PT_GATHER_HOST, because RCCL was unavailable or its group
                                    failed (that set of communicators aborted and dropped; a
                                    line on stderr for every such frame) */

/* pt_stats.kernel_path values. */
#define PT_PATH_TREE_GLOBAL 0    /* child-pair tree walk, scene read through L1/L2 */
#define PT_PATH_TREE_LDS 1       /* child-pair tree walk, scene in LDS             */
#define PT_PATH_FLAT_TABLE 2     /* flat leaf list, generic kernel-argument table  */
#define PT_PATH_FLAT_RTC 3       /* flat leaf list, hipRTC scene-specialised kernel */
#define PT_PATH_WIDE 4           /* wide (4/8-child) tree walk, scene read through L1/L2 */
#define PT_PATH_FLAT_TABLE_FAST 5 /* flat leaf list, kernel-argument table with the scene's flags */

/* ---- stream policy ---------------------------------------------------- */
#if defined(__HIPCC__)
#define PT_INLINE static inline __host__ __device__
#else
#define PT_INLINE static inline
#endif
/* lowbias32 integer finaliser (public-domain constants). */
PT_INLINE uint32_t pt_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}
/* LCG state for sample `sample` of pixel `pixel` = h * W + w (h = 0 is the bottom
 * row, as Image::pixels, image.h:11). */
PT_INLINE uint32_t pt_sample_seed(uint32_t pixel, uint32_t sample, uint32_t seed) {
    return pt_mix32(pt_mix32(pt_mix32(seed) ^ pixel) + sample);
}

/* ---- library / errors ------------------------------------------------- */
int pt_abi_version(void);
const char* pt_last_error(void);
int pt_device_count(void);

/* ---- host-side scene preparation (replaces BVH::build, Camera ctor) ---- */
/* Build the reference's SAH BVH (bvh.h:79-155) over num_tris triangles.
 * nodes_out must hold 2*num_tris-1 entries, tri_idx_out num_tris entries.
 * Returns the node count (>0) or a negative error code. The output is
 * bit-identical to BVH::build (same nodes, order, boxes, tri_idx). */
int pt_bvh_build(int32_t num_tris, const float* verts, pt_bvh_node* nodes_out,
                 int32_t* tri_idx_out);

/* Camera ctor arithmetic (camera.h:33-61). fov in radians. Returns PT_E_ARG
 * when forward and up are nearly parallel (camera.h:41-45). */
int pt_camera_init(const float pos[3], const float forward[3], const float up[3],
                   int32_t res_x, int32_t res_y, float fov, float distance,
                   pt_camera* out);

/* Validate a scene's node graph and report how the kernel will traverse it
 * (no device needed). info (may be NULL) receives: [0] reachable nodes,
 * [1] tree depth, [2] leaves on the exact flat path (0 = tree traversal),
 * [3] reference LIFO stack bound. Same checks as pt_ctx_set_scene. */
int pt_scene_validate(const pt_scene* scene, int32_t info[4]);
/* Extended form: info[0..3] as pt_scene_validate, then [4] wide nodes (0 = no wide
 * tree), [5] wide width, [6] wide levels, [7] wide nodes staged in LDS, [8] triangles in
 * wide-leaf order, [9] bytes per wide triangle record (48: vertices only, the leaf box is
 * the triangle's AABB; 64: with the stored leaf box; 0 = no wide tree).
 * Writes min(n, PT_SCENE_INFO_N) entries; returns PT_SCENE_INFO_N. */
#define PT_SCENE_INFO_N 10
int pt_scene_info(const pt_scene* scene, int32_t* info, int32_t n);

/* ---- rendering --------------------------------------------------------- */
typedef struct pt_ctx pt_ctx;

/* Create a context bound to HIP device `device` (its own stream). */
int pt_ctx_create(int device, pt_ctx** out);
void pt_ctx_destroy(pt_ctx* ctx);

/* Pack the scene to the device layout (SoA, tri_idx order) and upload it. A flat
 * scene (<= 64 leaves) also starts compiling its scene-specialised kernel (hipRTC,
 * ~0.4 s) on a background thread: renders do not wait for it; their launches run the
 * generic flat kernel until it is ready and then switch to it (bit-identical images
 * either way). */
int pt_ctx_set_scene(pt_ctx* ctx, const pt_scene* scene);

/* Wait for the scene's background preparation (the hipRTC compile) and load its result,
 * so every later render runs the specialised kernel. Optional. */
int pt_ctx_prepare(pt_ctx* ctx);

/* Wait for every background scene-kernel compile of the process; returns how many were still
 * running. No compile is left running at exit either way (the library waits in an exit
 * handler), but a host whose own teardown changes signal handlers before the C exit handlers
 * run (Python's faulthandler is disabled in interpreter finalisation) calls it first: the
 * Python package does, at interpreter exit. */
int pt_rtc_wait(void);

/* Render this part's rows. Output is the linear per-pixel mean after /spp
 * (image.h:37-40), float32 RGB, rows of this part in increasing h, h = 0
 * first. `out` is a DEVICE pointer when out_is_device != 0 (e.g. a torch
 * tensor on the context's device), otherwise a host pointer. Size:
 * pt_part_rows(...) * res_x * 3 floats. The call returns after the result is
 * complete (the context's stream is synchronised). */
int pt_ctx_render(pt_ctx* ctx, const pt_camera* cam, const pt_params* params,
                  float* out, int out_is_device, pt_stats* stats);

/* Progressive rendering (render_realtime's frame accumulation, render.h:219-387, offscreen):
 * adds samples [s_first, s_first + s_count) of this part to the context's running sum and
 * writes the running mean. s_first == 0 starts a new sum; otherwise s_first must equal the
 * samples already summed with the same camera and depth/seed/partition (else PT_E_ARG).
 * After every call the image is bit-identical to pt_ctx_render with spp = s_first +
 * s_count (params->spp is ignored). Any other render on the context ends the sum. */
int pt_ctx_render_progressive(pt_ctx* ctx, const pt_camera* cam, const pt_params* params, int32_t s_first,
                              int32_t s_count, float* out, int out_is_device, pt_stats* stats);

/* ---- per-pixel sample moments, error estimates, rendering to a noise target ----
 * r_s = the float32 radiance pt_ctx_render adds for sample s of a pixel and channel. Per pixel of
 * the part and channel, in the layout of `out` (rows*W*3), every pointer optional (NULL = skipped):
 *   sum    S = sum over s of (double)r_s, individually rounded double additions in sample order
 *          from +0.0
 *   sumsq  Q = sum over s of (double)r_s * (double)r_s (the product is exact in double), same order
 *   sem    the standard error of the mean with n = the samples summed so far:
 *          (float)sqrt(max(0, (Q - S*S/n) / (n - 1)) / n), evaluated in double; +inf for n < 2
 * S and Q are defined bit for bit and do not depend on how the samples are cut into launches. */
typedef struct pt_moments {
    double* sum;
    double* sumsq;
    float*  sem;
} pt_moments;

/* pt_ctx_render_progressive that also keeps S and Q: adds samples [s_first, s_first + s_count) to
 * the context's running MOMENTS sum. s_first == 0 starts one; otherwise the call must continue
 * this context's running moments sum with the same camera, depth, seed and partition (else
 * PT_E_ARG; a sum started by pt_ctx_render_progressive cannot be continued here, nor the other
 * way round). Any other render on the context ends the sum; queries, pt_ctx_trace and
 * pt_ctx_trace_grad leave it valid. `out` (optional) receives the running mean, bit-identical to
 * pt_ctx_render with spp = s_first + s_count; `mom` (optional) the moments after this call.
 * out_is_device covers `out` and the three pointers of `mom`. Every launch's slab is summed by a
 * pass of its own (no fused accumulation), which keeps six doubles per pixel on the device. */
int pt_ctx_render_moments(pt_ctx* ctx, const pt_camera* cam, const pt_params* params, int32_t s_first,
                          int32_t s_count, float* out, const pt_moments* mom, int out_is_device, pt_stats* stats);

/* Convergence count. With n samples summed, a channel is converged iff
 *     n*Q - S*S  <=  (n-1) * t*t,   t = rel*|S| + abs*n        (n >= 2)
 * which is sem <= rel*|mean| + abs with every division and the square root cleared away. It is
 * evaluated in double, every operation rounded on its own, in this order: a = n*Q; b = S*S;
 * l = a - b; t = rel*|S| + abs*n; r = (n-1)*(t*t); converged = l <= r (rel and abs widened from
 * float). A pixel is converged iff its three channels are; n < 2: none is; a NaN makes the
 * comparison false (unconverged). *count = the unconverged pixels; mask (optional, npix bytes):
 * 1 for an unconverged pixel, else 0. A pixel whose samples so far are all +0 counts as converged
 * (S = Q = 0): a minimum sample count is the guard. rel >= 0, abs >= 0, not both 0 (else PT_E_ARG). */
/* On the host over the caller's arrays (npix*3 doubles each; no device needed). */
int pt_moments_unconverged(const double* sum, const double* sumsq, int64_t npix, int32_t n, float rel, float abs,
                           int64_t* count, uint8_t* mask);
/* On the context's current moments sum (PT_E_ARG without one): the same count, by a device
 * reduction; mask_is_device != 0: `mask` is a device pointer. */
int pt_ctx_unconverged(pt_ctx* ctx, float rel, float abs, int64_t* count, uint8_t* mask, int mask_is_device);

/* Render until the noise target is met. Round boundaries: n_0 = min_spp, then n_{k+1} =
 * min(max_spp, n_k + step), or min(max_spp, 2 n_k) when step == 0. After each boundary the
 * unconverged count is read back (8 bytes); the render stops at the first boundary whose count
 * <= max_unconverged, or at max_spp. */
typedef struct pt_converge {
    float rel, abs;              /* the criterion above; rel >= 0, abs >= 0, not both 0 */
    int32_t min_spp, max_spp;    /* 2 <= min_spp <= max_spp */
    int32_t step;                /* samples per round after the first (>= 0); 0 = double */
    int64_t max_unconverged;     /* stop when count <= this */
} pt_converge;
typedef struct pt_converge_stats {
    int32_t spp, rounds;         /* samples per pixel rendered; boundaries evaluated */
    int64_t unconverged;         /* the count at the last boundary */
    uint64_t rays;               /* summed over the rounds, as the times below */
    double kernel_ms, reduce_ms, total_ms;
} pt_converge_stats;
/* params->spp is ignored. The image (`out`, optional) is bit-identical to pt_ctx_render at spp =
 * cs->spp; `mom` (optional) as pt_ctx_render_moments. The moments sum stays valid afterwards, so
 * pt_ctx_render_moments can continue it from cs->spp. PT_E_RUNAWAY is reported as by
 * pt_ctx_render (the rounds still run and the results are written). */
int pt_ctx_render_converge(pt_ctx* ctx, const pt_camera* cam, const pt_params* params, const pt_converge* conv,
                           float* out, const pt_moments* mom, int out_is_device, pt_converge_stats* cs);

/* Adaptive sampling: pt_ctx_render_converge that spends its later rounds only on the pixels that
 * still miss the criterion. The round boundaries are pt_ctx_render_converge's. Dense rounds give
 * every pixel of the part the round's samples (the render kernels, as pt_ctx_render_moments). At
 * the first boundary whose unconverged count is <= sparse_below * npix (and > max_unconverged) the
 * render switches to per-pixel rounds and stays there: the pixels unconverged at that boundary
 * become the active list, every other pixel is frozen with n_p = that boundary. A per-pixel round
 * gives the listed pixels samples [n_k, n_{k+1}); then the criterion is evaluated over the list
 * alone with n = n_{k+1}, and the pixels that meet it leave with n_p = n_{k+1}. A frozen pixel is
 * never evaluated or sampled again, so the active pixels always share one sample count and the
 * list only shrinks. The render stops when the list holds at most max_unconverged pixels, or at
 * max_spp; the pixels still listed keep the last boundary as n_p.
 *
 * Per pixel and channel, with the pixel's own n_p: out = (the float32 in-order sum of samples
 * 0..n_p-1) / (float)n_p, bit-identical to pt_ctx_render at spp = n_p; mom->sum and mom->sumsq are
 * the sums above over those n_p samples; mom->sem uses n = n_p; spp_out[q] = n_p. Nothing depends
 * on the order of the list or on how a round is cut into launches. A per-pixel round runs the
 * binary walk (pt_ctx_trace's kernel fed with the render's camera rays), which on small scenes is
 * slower per ray than the render kernels: sparse_below is the active fraction below which it pays. */
typedef struct pt_adaptive {
    pt_converge conv;            /* criterion, min_spp, max_spp, step, max_unconverged: as pt_ctx_render_converge */
    float sparse_below;          /* 0: the library's default for the scene's kernel family (flat, wide, tree);
                                    < 0: never switch (the call is then pt_ctx_render_converge);
                                    >= 1: per-pixel rounds from the first boundary on */
} pt_adaptive;
typedef struct pt_adaptive_stats {
    int32_t rounds;              /* boundaries evaluated */
    int32_t dense_rounds;        /* of them, rounds rendered for every pixel */
    int32_t max_spp;             /* the largest n_p (the last boundary) */
    int32_t sparse_launches;     /* trace launches of the per-pixel rounds */
    int64_t unconverged;         /* pixels that miss the criterion at the end (the final list, or count) */
    int64_t samples;             /* sum of n_p over the part: the pixel-samples rendered */
    uint64_t rays;               /* all rounds */
    uint64_t sparse_rays;        /* of them, rays of the per-pixel rounds */
    double kernel_ms, reduce_ms, total_ms;   /* reduce_ms: accumulation, criterion and list passes */
    double sparse_kernel_ms;     /* of kernel_ms, the trace kernels of the per-pixel rounds */
} pt_adaptive_stats;
/* params->spp is ignored. out, mom, spp_out (npix int32) and st are optional; out_is_device covers
 * out, the pointers of mom and spp_out. If a per-pixel round ran, the context's running sum is no
 * longer uniform and ends (pt_ctx_unconverged and a pt_ctx_render_moments continuation then return
 * PT_E_ARG, as after any other render); otherwise the state is pt_ctx_render_converge's and stays
 * valid. Argument errors and PT_E_RUNAWAY are reported as by pt_ctx_render_converge. The caveat of
 * the criterion holds per pixel: one whose first min_spp samples are all +0 is frozen there. */
int pt_ctx_render_adaptive(pt_ctx* ctx, const pt_camera* cam, const pt_params* params, const pt_adaptive* ad,
                           float* out, const pt_moments* mom, int32_t* spp_out, int out_is_device,
                           pt_adaptive_stats* st);

/* pt_ctx_render followed by gamma_correct + save_png quantisation on the device
 * (image.h:41-55): out receives rows*W*3 bytes of this part (row order as pt_ctx_render;
 * flip != 0 reverses it: top row first, as the PNG of a whole image), equal to
 * pt_image_to_rgb8 of the linear image. Requires gamma > 0. */
int pt_ctx_render_rgb8(pt_ctx* ctx, const pt_camera* cam, const pt_params* params, float gamma, int flip,
                       uint8_t* out, int out_is_device, pt_stats* stats);

/* ---- ray queries and first-hit AOVs (BVH::intersect, bvh.h:156-183) ----------
 * The answer for a ray (o, d) is what BVH::intersect returns on the scene's BVH: nodes popped
 * LIFO (right child first), AABB::intersect_inv with inv = 1 / d, a leaf's triangles in tri_idx
 * order, the winner replaced only when t_ < t, t starting at 1e30f. Result: the index into the
 * caller's triangle array (tri_idx[i], -1 for a miss) and t (1e30f for a miss). The walk defines
 * the answer (ties, triangles whose box the slab test misses), for any float in o and d.
 * Rays are two arrays of n * 3 floats: origins and (unnormalised) directions. */
#define PT_QUERY_CLOSEST 0
#define PT_QUERY_ANY 1           /* occlusion: out[i] = 1 iff the closest hit's t < tmax[i] (strict) */

/* The reference walk on the host over the caller's own arrays (no device needed). The scene is
 * validated as by pt_scene_validate on every call, so pass rays in batches. n == 0: PT_OK. */
int pt_bvh_intersect(const pt_scene* scene, const float* origins, const float* dirs, int64_t n,
                     float* t_out, int32_t* tri_out);

/* Statistics of one query or AOV call. */
typedef struct pt_query_stats {
    uint64_t rays;               /* rays traced (AOV: pixels of the part)                       */
    uint64_t hits;               /* rays with a hit (PT_QUERY_ANY: occluded rays)               */
    double kernel_ms;            /* sum of the kernel durations (HIP events)                    */
    double total_ms;             /* end-to-end wall time of the call                            */
    int32_t launches;            /* kernel launches                                             */
    int32_t lds_scene;           /* 1: nodes and triangles staged in LDS; 0: read through L1/L2 */
    int32_t lds_stack;           /* 1: traversal stack rows in LDS; 0: in a global buffer       */
} pt_query_stats;

/* Closest hit or occlusion for n rays on the context's scene (the binary child-pair walk for
 * every scene). PT_QUERY_CLOSEST: t_out[i] and out[i] (triangle or -1), both required.
 * PT_QUERY_ANY: out[i] = 0 / 1, t_out ignored; tmax (n floats) may be NULL = 1e30f for every
 * ray. is_device != 0: origins, dirs, tmax, t_out and out are DEVICE pointers on the context's
 * device (read and written in place), otherwise host pointers. n == 0 is PT_OK and launches
 * nothing; large n is cut into several launches. The call returns after the results are
 * complete (the context's stream is synchronised) and leaves a progressive sum as it is. */
int pt_ctx_intersect(pt_ctx* ctx, const float* origins, const float* dirs, int64_t n, int mode,
                     const float* tmax, float* t_out, int32_t* out, int is_device, pt_query_stats* stats);

/* First-hit channels of one sample; every pointer is optional (NULL = skipped). Per pixel, rows
 * in pt_ctx_render's order for the partition:
 *   t        1 float   hit t, 1e30f for a miss
 *   tri      1 int32   index into the caller's triangles, -1 for a miss
 *   normal   3 floats  Triangle::normal(ray_d, .) (triangle.h:45-49), +0 for a miss
 *   albedo   3 floats  material.color, +0 for a miss
 *   emission 3 floats  material.emit_color, +0 for a miss
 *   ray      6 floats  o.xyz, d.xyz of the camera ray (hit or miss) */
typedef struct pt_aov {
    float* t;
    int32_t* tri;
    float* normal;
    float* albedo;
    float* emission;
    float* ray;
} pt_aov;

/* The first hit of sample `sample` of every pixel of this part: the ray pt_ctx_render starts for
 * that sample (LCG state pt_sample_seed(h*W + w, sample, params->seed), Camera::get_ray) and its
 * BVH::intersect answer. params gives seed and partition; spp, depth and the batch fields are
 * ignored. out_is_device != 0: the channel pointers are device pointers. Synchronous, and
 * leaves a progressive sum as it is. */
int pt_ctx_render_aov(pt_ctx* ctx, const pt_camera* cam, const pt_params* params, int32_t sample,
                      const pt_aov* out, int out_is_device, pt_query_stats* stats);

/* ---- variance-guided a-trous denoiser over AOVs and sample moments -----------------
 * An edge-avoiding a-trous wavelet filter (the spatial part of SVGF) over a whole image of W x H
 * pixels, rows in pt_ctx_render's order, guided by the first hit's channels and, optionally, by
 * the variance of the mean. The result is defined bit for bit: only + - * / sqrt and comparisons
 * in float32, each rounded on its own (no fused multiply-add, no exp), so the host form and the
 * device form return the same bits.
 *
 * Inputs. color: 3 floats per pixel. var (optional): 3 floats per pixel, the variance of color
 * as a mean (pt_moments_variance). Guides: normal, t, tri and emission are pt_aov's channels of
 * the same names; position (3 floats) is the first hit's point, per component o + d * t (one
 * multiplication, then one addition, as trace() forms its hit point). All five are required.
 * A pixel's class: 0 for a miss (tri < 0), 2 for a hit with any emission channel != 0, else 1.
 *
 * Pass i = 0 .. passes-1 runs with stride s = 2^i and takes (c, v) to (c', v') for every pixel
 * p = (x, y). Every dot product is ((a.x*b.x) + (a.y*b.y)) + (a.z*b.z).
 *  1. l(q) = ((0.25f*c_r) + (0.5f*c_g)) + (0.25f*c_b).
 *  2. With var only: vt_ch = the 3x3 mean of v_ch around p (stride 1), weights g = [1/4, 1/2, 1/4]
 *     per axis, rows j the outer loop and columns k the inner, both ascending, in-image taps only:
 *     acc += (g_j*g_k) * v, wacc += g_j*g_k, vt = acc / wacc.
 *     sig_p = ((0.25f*sqrtf(vt_r)) + (0.5f*sqrtf(vt_g))) + (0.25f*sqrtf(vt_b));
 *     den_p = (sigma_l*sig_p) + eps.
 *  3. tau_p = sigma_z * t_p.
 *  4. Taps: j = -2..2 outer, k = -2..2 inner, q = (x + k*s, y + j*s); a tap outside the image is
 *     skipped. h = [1/16, 1/4, 3/8, 1/4, 1/16], hh = h_j * h_k (exact). The centre tap has w = 1.
 *     For every other tap: class_q != class_p skips it. class_p == 0: wg = 1; otherwise
 *         dn = n_p . n_q, set to 0 unless dn > 0, then squared normal_pow_log2 times (dn = dn*dn);
 *         dl = | n_p . (X_q - X_p) |  (the difference per component first);
 *         wz = (dl < tau_p) ? (tau_p - dl) / tau_p : 0;   wg = dn * wz.
 *     Without var wl = 1; with it xl = |l_p - l_q| / den_p and wl = 1 / (1 + xl*xl).
 *     w = wg * wl; unless w > 0 the tap is skipped (a NaN skips it too). Then, per channel,
 *         kq = hh * w;  A_ch += kq * c_ch(q);  B_ch += (kq*kq) * v_ch(q);  Wsum += kq
 *     (A, B and Wsum start at +0; B only with var).
 *  5. c'_ch = A_ch / Wsum; v'_ch = B_ch / (Wsum*Wsum). The centre tap keeps Wsum >= 9/64.
 * The guides, tau and the classes are those of the input for every pass.
 *
 * Consequences. With var, a NaN or infinite colour of a neighbour never enters another pixel's
 * sum (its wl is NaN or 0); without var the luminance does not gate, only the guides do. A NaN
 * centre stays NaN. A pixel whose prefiltered variance vt is negative or NaN in a channel keeps
 * its centre tap only. A +inf variance (n < 2) makes every luminance weight of that pixel 1
 * (or NaN, hence skipped, for an infinite or NaN neighbour). First-hit guides cannot see edges
 * inside a mirror's reflection: those are blurred.
 *
 * Passes ping-pong between two buffers of the implementation; out (W*H*3) and var_out (optional,
 * W*H*3, only with var; else PT_E_ARG) receive the last pass's result and may alias color and var. */
typedef struct pt_denoise_guides {
    const float* normal;         /* 3 floats per pixel */
    const float* t;              /* 1 float  */
    const int32_t* tri;          /* 1 int32  */
    const float* emission;       /* 3 floats */
    const float* position;       /* 3 floats: o + d * t per component */
} pt_denoise_guides;

/* A 0 selects the default, so the values in effect are passes 1..8, normal_pow_log2 1..10 and
 * positive floats; a negative or NaN value, passes > 8 or normal_pow_log2 > 10 is PT_E_ARG.
 * A NULL pt_denoise_params selects every default. */
typedef struct pt_denoise_params {   /* 20 bytes */
    int32_t passes;              /* 0 (default: 5) or 1..8 */
    float sigma_l;               /* > 0, default 1: luminance tolerance in standard deviations */
    float sigma_z;               /* > 0, default 0.01: plane-distance tolerance as a fraction of t_p */
    int32_t normal_pow_log2;     /* 0 (default: 7, power 128) or 1..10: squarings of the normal dot product */
    float eps;                   /* > 0, default 1e-6: added to the luminance denominator */
} pt_denoise_params;

#define PT_DENOISE_DIRECT 1      /* one pixel per lane, every tap read through L1/L2 */
#define PT_DENOISE_LDS 2         /* a 32x16 tile and its halo staged in LDS (stride 1 only) */
typedef struct pt_denoise_stats {    /* 96 bytes */
    double kernel_ms;            /* pack and pass kernels (HIP events) */
    double total_ms;             /* end-to-end wall time of the call   */
    int32_t passes;              /* passes run */
    int32_t launches;            /* kernel launches (pack + passes) */
    int32_t form[8];             /* per pass i (stride 2^i): PT_DENOISE_DIRECT or PT_DENOISE_LDS; 0: not run */
    float pass_ms[8];            /* per pass: its kernel's duration */
    float pack_ms;               /* the pack kernel's duration */
    int32_t reserved;
} pt_denoise_stats;

/* The variance of the mean from the sample moments (pt_moments: S = sum, Q = sumsq), per pixel
 * and channel, in double, every operation rounded on its own:
 *     m = (S*S)/n;  d = (Q - m)/(n - 1);  d = d > 0 ? d : 0;  var = (float)(d/n);  +inf for n < 2.
 * n is `n` for every pixel, or with spp != NULL the pixel's own spp[q] (npix int32:
 * pt_ctx_render_adaptive's spp_out; `n` is then ignored). This is not sem*sem: sem is rounded
 * after its square root. sum, sumsq: npix*3 doubles; var_out: npix*3 floats. Host, no device. */
int pt_moments_variance(const double* sum, const double* sumsq, int64_t npix, int32_t n, const int32_t* spp,
                        float* var_out);
/* The same by a kernel on the context's device; is_device != 0: every pointer is a device pointer. */
int pt_ctx_moments_variance(pt_ctx* ctx, const double* sum, const double* sumsq, int64_t npix, int32_t n,
                            const int32_t* spp, float* var_out, int is_device);

/* The filter on the host (no device needed). W, H >= 1, W*H <= 2^30. */
int pt_image_denoise(int32_t W, int32_t H, const float* color, const float* var, const pt_denoise_guides* guides,
                     const pt_denoise_params* params, float* out, float* var_out);
/* The filter on the context's device, bit-identical to pt_image_denoise. is_device != 0: color,
 * var, the guides, out and var_out are device pointers on the context's device. Needs no scene,
 * is synchronous and leaves a running sum as it is. stats is optional. */
int pt_ctx_denoise(pt_ctx* ctx, int32_t W, int32_t H, const float* color, const float* var,
                   const pt_denoise_guides* guides, const pt_denoise_params* params, float* out, float* var_out,
                   int is_device, pt_denoise_stats* stats);

typedef struct pt_denoised_stats {
    double total_ms;             /* end-to-end wall time of the call */
    double aov_ms, variance_ms;  /* the AOV kernel's and the position + variance kernels' durations */
    pt_denoise_stats denoise;
} pt_denoised_stats;
/* Render and denoise on the device without a host round trip between the steps:
 * pt_ctx_render_adaptive (params, adaptive); pt_ctx_render_aov of sample 0 at params->seed;
 * position = o + d * t; pt_moments_variance with the per-pixel n_p; pt_ctx_denoise with var.
 * Needs params->part_count <= 1 (else PT_E_ARG: rows dealt to other GPUs have no neighbours).
 * out (W*H*3) is bit-identical to making the four calls by hand; noisy_out (optional, W*H*3)
 * receives the unfiltered image and spp_out (optional, W*H int32) the n_p; out_is_device covers
 * the three. render_stats (a pt_adaptive_stats) and stats are optional. Errors are reported as by
 * the pieces; after PT_E_RUNAWAY of the render the filter still runs and the code is returned. */
int pt_ctx_render_denoised(pt_ctx* ctx, const pt_camera* cam, const pt_params* params, const pt_adaptive* adaptive,
                           const pt_denoise_params* denoise_params, float* out, float* noisy_out, int32_t* spp_out,
                           int out_is_device, pt_adaptive_stats* render_stats, pt_denoised_stats* stats);

/* ---- temporal reprojection: accumulating frames across camera moves ----------------
 * The temporal part of SVGF for a static scene and a moving camera (render_realtime's use,
 * render.h:219-387): every pixel's first hit is projected into the previous frame's camera, the
 * previous frame's accumulated colour is gathered there where the surfaces agree, and the two are
 * blended. The result and its variance are what the a-trous filter above takes. Defined bit for
 * bit: float32 throughout, only + - * /, floorf, fabsf and comparisons, each rounded on its own (no
 * fused multiply-add), every dot product ((a.x*b.x) + (a.y*b.y)) + (a.z*b.z); the host form and the
 * device form return the same bits.
 *
 * Planes. All are W x H, rows in pt_ctx_render's order. A history (pt_temporal_history) is seven
 * planes: color, m2 (the accumulated second moment of the frames' means), var: 3 floats each;
 * hist: 1 int32, the frames accumulated (>= 1 once written; < 1 marks a hole that is never read);
 * normal, position: 3 floats, cls: 1 int32, the guides of the frame that wrote it. cls is the
 * denoiser's class: 0 for a miss (tri < 0), 2 for a hit with any emission channel != 0, else 1.
 * A call reads the history `prev` (NULL: the first frame, every pixel is without history) and
 * writes every plane of `next`. Every pointer of `next` is required; of `prev`, every one but
 * `var`, which is read in sample mode only. It is a gather: a plane of `prev` that overlaps a
 * plane of `next` in memory is PT_E_ARG. `next` may alias the current frame's inputs (a pixel
 * reads its own inputs before it writes).
 *
 * Inputs. cam_cur and cam_prev (required with prev; only pos, v_res, cell_size, distance and
 * transform are read, not res), the current frame's color c (3 floats per pixel), its variance v
 * as a mean (optional, pt_moments_variance), the denoiser's five guides of the current frame
 * (pt_denoise_guides, all required) and pt_temporal_params.
 *
 * proj(cam, X), the inverse of Camera::get_ray (camera.h:63-73) without its jitter:
 *     d = X - cam.pos per component;  cx, cy, cz = d . row 0, 1, 2 of cam.transform;
 *     valid only if cz < 0 (false for a NaN);  k = (0.0f - cam.distance) / cz;
 *     fx = ((cx*k) + (0.5f*cam.v_res[0])) / cam.cell_size;  fy = ((cy*k) + (0.5f*cam.v_res[1])) / cam.cell_size.
 *
 * Per pixel p = (w, h), with n_p, X_p, t_p, cls_p the current guides:
 *  1. cls_p == 0: no history (a miss carries no hit point).
 *  2. (fxc, fyc) = proj(cam_cur, X_p), (fxp, fyp) = proj(cam_prev, X_p); either invalid: no history.
 *     gx = (float)w + (fxp - fxc); gy = (float)h + (fyp - fyc). This is the motion-vector form: the
 *     AOV's hit point is jittered inside its pixel, and the projection into the current camera
 *     takes that offset out again.
 *  3. Unless gx > -1 && gx < (float)W && gy > -1 && gy < (float)H: no history (a NaN fails).
 *     x0 = (int)floorf(gx); ax = gx - (float)x0; y0 and ay likewise.
 *  4. Taps: j = 0, 1 outer, k = 0, 1 inner, q = (x0 + k, y0 + j); a tap outside the image is
 *     skipped. wx = [1.0f - ax, ax], wy likewise, bw = wx_k * wy_j. A tap counts only if, tested in
 *     this order, bw > 0; hist_prev(q) >= 1; cls_prev(q) == cls_p; n_p . n_prev(q) > normal_min;
 *     |n_p . (X_prev(q) - X_p)| < sigma_z * t_p (the difference per component first); and every
 *     channel of color_prev(q) has fabsf(c) < +inf. For a counting tap: Wsum += bw; per channel
 *     A += bw*color_prev(q), M += bw*m2_prev(q) and, in sample mode, V += bw*var_prev(q) (all from
 *     +0); Nmin = min(Nmin, hist_prev(q)).
 *  5. Unless Wsum > 0: no history. Otherwise the pixel reuses its history: per channel pc = A/Wsum,
 *     pm = M/Wsum, pv = V/Wsum; N' = min(Nmin, max_history - 1) + 1; alpha = 1.0f/(float)N';
 *     b = 1.0f - alpha;
 *         c'  = (b*pc) + (alpha*c);      m2' = (b*pm) + (alpha*(c*c));
 *         sample mode:   v' = ((b*b)*pv) + ((alpha*alpha)*v)  (independent estimates: the variances
 *                        add with squared weights);
 *         temporal mode: d = m2' - (c'*c'); d = d > 0 ? d : 0; v' = d*alpha.
 *  6. No history: c' = c, m2' = c*c, N' = 1; v' = v in sample mode, +inf in temporal mode
 *     (pt_moments_variance's convention below two samples: the filter then lets the guides decide).
 *  7. next receives c', m2', v', N' and the current frame's normal, position and cls.
 * `reused` is the number of pixels that took step 5.
 *
 * Consequences. With cam_prev equal to cam_cur bit for bit the two projections are the same bits,
 * their difference is exactly 0 and the lookup is exactly pixel p with weight 1: a static camera
 * never blurs its history, and c' follows c_N = (b*c_{N-1}) + (alpha*c) with alpha = 1/N until N
 * reaches max_history, where it stays. A NaN or infinite current colour goes into c' of its own
 * pixel only: the next frame's taps drop it (the test on color_prev), so it lasts one frame and
 * the pixel starts again. m2_prev and var_prev are not tested; a history written by this function
 * from finite frames holds none. A camera that looks away from a hit point (cz >= 0, in either
 * camera) gives no history, as does a projection that overflows (inf - inf is a NaN). The planes
 * of prev are W x H of this call: after a change of resolution the caller passes prev = NULL. var
 * is interpolated linearly, not with squared weights, on purpose: neighbouring histories share
 * most of their samples after a move, so they are correlated and squared weights would promise
 * too much. hist above max_history (a history written with a larger one) is clamped by step 5. */
typedef struct pt_temporal_history {
    float* color;                /* 3 floats per pixel: the accumulated, unfiltered colour */
    float* m2;                   /* 3 floats: the accumulated c*c */
    float* var;                  /* 3 floats: v' */
    int32_t* hist;               /* 1 int32: N' */
    float* normal;               /* 3 floats */
    float* position;             /* 3 floats */
    int32_t* cls;                /* 1 int32: 0, 1 or 2 */
} pt_temporal_history;

#define PT_TEMPORAL_VAR_SAMPLE 1   /* v' from the frames' own variances; needs var and, with prev, prev->var */
#define PT_TEMPORAL_VAR_TEMPORAL 2 /* v' from the accumulated moments; var is ignored */
/* A 0 selects the default; max_history outside 0..65535, a negative or NaN float, normal_min >= 1
 * or another variance_mode is PT_E_ARG. A NULL pt_temporal_params selects every default. */
typedef struct pt_temporal_params {  /* 16 bytes */
    int32_t max_history;         /* 0 (default: 32) or 1..65535 */
    float sigma_z;               /* > 0, default 0.01: plane-distance tolerance as a fraction of t_p */
    float normal_min;            /* in (0, 1), default 0.9 */
    int32_t variance_mode;       /* 0 (default: sample mode with var, else temporal mode) or PT_TEMPORAL_VAR_* */
} pt_temporal_params;

typedef struct pt_temporal_stats {   /* 24 bytes */
    double kernel_ms;            /* the kernel's duration (HIP events) */
    double total_ms;             /* end-to-end wall time of the call   */
    int64_t reused;              /* pixels that reused their history   */
} pt_temporal_stats;

/* One frame's accumulation on the host (no device needed). W, H >= 1, W*H <= 2^30. reused is optional. */
int pt_image_temporal(int32_t W, int32_t H, const pt_camera* cam_cur, const pt_camera* cam_prev, const float* color,
                      const float* var, const pt_denoise_guides* guides, const pt_temporal_history* prev,
                      const pt_temporal_history* next, const pt_temporal_params* params, int64_t* reused);
/* The same on the context's device, bit-identical, `reused` (counted by ballot, one atomic per
 * wave) included. is_device != 0: color, var, the guides and every plane of prev and next are
 * device pointers on the context's device. Needs no scene, is synchronous and leaves a running sum
 * as it is. stats is optional. */
int pt_ctx_temporal(pt_ctx* ctx, int32_t W, int32_t H, const pt_camera* cam_cur, const pt_camera* cam_prev,
                    const float* color, const float* var, const pt_denoise_guides* guides,
                    const pt_temporal_history* prev, const pt_temporal_history* next,
                    const pt_temporal_params* params, int is_device, pt_temporal_stats* stats);

typedef struct pt_render_temporal_stats {
    double total_ms;             /* end-to-end wall time of the call */
    double render_ms;            /* pt_ctx_render_moments' total_ms */
    double aov_ms, variance_ms;  /* the AOV kernel's and the position + variance kernels' durations */
    uint64_t rays;               /* the render's traced segments */
    int32_t had_history;         /* 1: the frame was accumulated onto the context's history, 0: it started one */
    int32_t variance_mode;       /* PT_TEMPORAL_VAR_SAMPLE (spp >= 2) or PT_TEMPORAL_VAR_TEMPORAL (spp == 1) */
    pt_temporal_stats temporal;
    pt_denoise_stats denoise;
} pt_render_temporal_stats;
/* One frame of a camera path without a host round trip between the steps:
 *   pt_ctx_render_moments of params->spp samples from s_first = 0 at params->seed;
 *   pt_ctx_render_aov of sample 0 at params->seed; position = o + d * t;
 *   with spp >= 2 pt_ctx_moments_variance (n = spp) and sample mode, with spp == 1 no var and temporal mode
 *     (temporal_params->variance_mode must be 0 or that mode, else PT_E_ARG);
 *   pt_ctx_temporal against the history and the camera the context kept from its last such call;
 *   pt_ctx_denoise of (c', v') into out.
 * The caller changes params->seed from frame to frame: frames of one seed repeat their noise and
 * accumulate nothing. The context owns two histories and alternates between them; the unfiltered
 * c' is what is kept (and what accumulated_out, optional, W*H*3, receives), never the filtered
 * image. The history is dropped (the next frame starts one) by reset != 0 (before this frame), by
 * pt_ctx_set_scene, by a resolution other than the kept one and by any error return of this call,
 * PT_E_RUNAWAY included (out is still written then). Needs params->part_count <= 1 (else PT_E_ARG).
 * out (W*H*3) is bit-identical to making the calls by hand; out_is_device covers out and
 * accumulated_out. Ends a running sum, as any render does. */
int pt_ctx_render_temporal(pt_ctx* ctx, const pt_camera* cam, const pt_params* params,
                           const pt_temporal_params* temporal_params, const pt_denoise_params* denoise_params,
                           int reset, float* out, float* accumulated_out, int out_is_device,
                           pt_render_temporal_stats* stats);

/* ---- radiance along caller-supplied rays (trace(), render.h:36-61) ------------
 * rgb_out[3 i ..] = (sum over s of trace(bvh, o_i, d_i, depth)) / (float)spp: the sum runs in
 * float32 in sample order s = 0, 1, ... from +0 and is divided per channel (image.h:37-40); with
 * spp == 1 the result is the sample itself. Sample s of ray i runs the reference's LCG from its
 * given state; no camera draws are made (the ray is the caller's), and directions are used as
 * given (unnormalised), exactly as trace() would. Rays are two arrays of n * 3 floats, as for
 * pt_ctx_intersect. */
typedef struct pt_trace_params {
    int32_t depth;               /* trace()'s depth, 0..PT_MAX_DEPTH; 0: every result +0, no ray traced (render.h:37) */
    int32_t spp;                 /* samples per ray, 1..(1 << 20) */
    uint32_t seed;
    const uint32_t* states;      /* optional, n * spp: LCG state sample s of ray i starts with, at [i * spp + s].
                                    NULL: pt_sample_seed((uint32_t)i, s, seed), i = the ray's index in the call */
} pt_trace_params;

typedef struct pt_trace_stats {  /* 64 bytes */
    uint64_t rays;               /* traced segments = BVH::intersect calls */
    uint64_t paths;              /* n * spp */
    uint64_t runaway;            /* specular rejection loops that hit the bound (0 normally) */
    double kernel_ms;            /* sum of the trace-kernel durations (HIP events)  */
    double reduce_ms;            /* sum of the in-order sum passes' durations       */
    double total_ms;             /* end-to-end wall time of the call                */
    int32_t launches;            /* trace-kernel launches                           */
    int32_t lds_scene;           /* 1: nodes, triangles and materials staged in LDS */
    int32_t lds_stack;           /* 1: traversal stack rows in LDS                  */
    int32_t lds_records;         /* 1: path records in LDS; 0: in a global buffer   */
} pt_trace_stats;

/* trace() on the host over the caller's own arrays (no device needed), bit-identical to
 * pt_ctx_trace. The scene is validated as by pt_scene_validate on every call. */
int pt_bvh_trace(const pt_scene* scene, const float* origins, const float* dirs, int64_t n,
                 const pt_trace_params* params, float* rgb_out, pt_trace_stats* stats);

/* trace() for n rays on the context's scene (the binary child-pair walk for every scene).
 * is_device != 0: origins, dirs, params->states and rgb_out are DEVICE pointers on the context's
 * device (the inputs are left untouched), otherwise host pointers. n == 0 is PT_OK and launches
 * nothing; large n * spp is cut into several launches over rays. A specular rejection loop that
 * hits its bound is reported as by pt_ctx_render (PT_E_RUNAWAY, the results are still written).
 * Synchronous, and leaves a progressive sum as it is. */
int pt_ctx_trace(pt_ctx* ctx, const float* origins, const float* dirs, int64_t n,
                 const pt_trace_params* params, float* rgb_out, int is_device, pt_trace_stats* stats);

/* ---- material gradients of trace() along caller-supplied rays -------------------
 * trace() draws its directions from the normal, the incoming direction and the roughness only
 * (material.h:6-25), so a path's geometry does not depend on color or emit_color and the radiance
 * is a polynomial in them, L_k = emit_k + ((2 L_{k+1}) color_k) cos_k (render.h:60): the
 * derivative below is exact, without reparameterisation or bias. One call evaluates the radiance
 * at (optionally) changed colours and emissions and/or back-propagates dLoss/d rgb_out to them.
 * Material type and roughness always come from the scene; rays, spp, depth, seed and states are
 * pt_ctx_trace's.
 *
 * Forward: rgb_out is bit-identical to pt_ctx_trace on a scene whose materials carry the override
 * values (no override: to pt_ctx_trace itself), the in-order float32 sum over samples included.
 *
 * Per-path terms: float32, no contraction, in this operation order per channel. Path (i, s) has
 * bounces k = 0 .. K-1 on triangles h_k with cosines c_k, then a terminal (an EMIT hit, a hit on
 * the last allowed segment, or a miss). w = grad_rgb[i] / (float)spp; T_0 = w,
 * T_{k+1} = ((2 T_k) color_{h_k}) c_k; L_{k+1} is the unwinding's value below bounce k (the
 * forward bits). In ascending k: bounce k adds T_k to grad_emit[h_k] and ((2 T_k) L_{k+1}) c_k
 * to grad_color[h_k]; a terminal that is a hit adds T_K to grad_emit[h_K] (and nothing to
 * grad_color: its factor is trace(depth 0) = 0); a miss adds nothing. Indices are the caller's
 * triangle indices: a triangle that sits in several leaves of a caller-built tree gets one sum.
 *
 * Sum: each destination is the sum of its float32 terms in float64, in any order (so within
 * gamma_{N-1} sum|t| of the exact sum of its N terms); a call with n = 1, spp = 1 adds in k order
 * and is reproducible bit for bit. A term that is +-0 is counted in `terms` and leaves its
 * destination as it is. Non-finite rays, materials or upstream gradients, and products that
 * overflow, give non-finite terms; per destination and channel the sum then has the class that
 * float64 addition gives in any order (N float32 terms cannot overflow a double): NaN if a term
 * is NaN or if +inf and -inf both occur, +inf if only +inf occurs, -inf if only -inf occurs. A
 * channel all of whose terms are finite keeps its bound whatever the other channels and
 * destinations hold. A scene's dark-path shortcut never drops a grad_emit term (a dark path still
 * carries T_k != 0). */
typedef struct pt_trace_grad_io {
    const float* color;     /* optional, num_tris*3: albedo to evaluate at, caller's triangle order; NULL = the scene's */
    const float* emit;      /* optional, num_tris*3: emit_color to evaluate at; NULL = the scene's        */
    const float* grad_rgb;  /* n*3: dLoss/d rgb_out; required if grad_color or grad_emit is given (else ignored) */
    float*  rgb_out;        /* optional, n*3: the forward value at these materials                         */
    double* grad_color;     /* optional, num_tris*3: dLoss/d color, overwritten                            */
    double* grad_emit;      /* optional, num_tris*3: dLoss/d emit_color, overwritten                       */
} pt_trace_grad_io;

typedef struct pt_grad_stats {
    pt_trace_stats trace;   /* as pt_ctx_trace fills it */
    uint64_t terms;         /* contributions added to the requested ones of grad_color, grad_emit (3 channels = 1 term) */
    double grad_ms;         /* zeroing, override gather, flush: everything but the path kernel */
    int32_t lds_table;      /* 1: per-block gradient table in LDS; 0: global atomics only */
    int32_t reserved;
} pt_grad_stats;

/* On the context's scene. is_device != 0: the rays, params->states and every pointer in io are
 * DEVICE pointers on the context's device (inputs left untouched), otherwise host pointers.
 * n == 0 is PT_OK, launches nothing and zeroes the gradient outputs; depth 0 zeroes every output.
 * Launches are cut as pt_ctx_trace cuts them; runaway loops are reported as it reports them.
 * Synchronous; uses buffers of its own, so a progressive sum stays valid, and the override never
 * reaches the scene. */
int pt_ctx_trace_grad(pt_ctx* ctx, const float* origins, const float* dirs, int64_t n,
                      const pt_trace_params* params, const pt_trace_grad_io* io, int is_device,
                      pt_grad_stats* stats);
/* The same terms on the host over the caller's own arrays (no device needed), summed in double in
 * (ray, sample, k) order; rgb_out bit-identical to pt_bvh_trace at the override values. */
int pt_bvh_trace_grad(const pt_scene* scene, const float* origins, const float* dirs, int64_t n,
                      const pt_trace_params* params, const pt_trace_grad_io* io, pt_grad_stats* stats);

/* ---- light sampling (next-event estimation) -------------------------------------
 * An opt-in estimator beside trace(): a diffuse vertex also samples a point on the emitters and
 * tests its visibility with one extra closest-hit walk. Its expected value is trace()'s at every
 * depth (below); every other entry point keeps its bits. All arithmetic is float32 with + - * /,
 * fabsf and comparisons, each operation rounded on its own (no contraction, correctly rounded
 * division), in the order written; csrc/pt_nee.h states it once for the host form and the kernels.
 *
 * Light table (made on the host per scene). The lights are the triangles j, in the caller's
 * triangle order, whose material type is PT_MAT_EMIT, whose emit is finite with some channel > 0,
 * and whose area a_j = 0.5f * sqrtf(dot(c, c)), c = cross(v2 - v1, v3 - v1), is finite and > 0.
 * cdf_j is the running float32 sum of a_j from +0 and A its last entry. With no such triangle, or
 * with A not finite, the scene has no lights: no light draw is made and no direct term is added.
 * kA = A / 3.14159274f (A / (float)M_PI) is formed once.
 *
 * Path (i, s) in forward form: T = (1, 1, 1), L = (+0, +0, +0), sampled = false; the LCG state and
 * the ray are pt_ctx_trace's. For k = 1 .. depth:
 *   1. BVH::intersect. A miss ends the path.
 *   2. An EMIT hit: L = L + T o emit, unless `sampled` is true and the triangle is in the light
 *      table (then nothing is added). The path ends.
 *   3. Any other hit: L = L + T o emit_h. n (faced as triangle.h:48), hp = o + d t and
 *      new_o = hp + n * 1e-4f are trace()'s.
 *   4. Light draw, when the material samples the hemisphere (every type but EMIT and SPECULAR),
 *      the scene has lights and k < depth:
 *        x1, x2, x3 = rand01() in this order, before the BRDF draw;
 *        j = the first light with cdf_j > x1 * A, the last light when there is none;
 *        (u, v) = (x2, x3), replaced by (1 - u, 1 - v) when u + v > 1;
 *        y = (v1 + e1 * u) + e2 * v with e1 = v2 - v1, e2 = v3 - v1 of light j;
 *        w = y - new_o, cx = dot(n, w), cy = fabsf(dot(n_j, w)) with n_j = normalize(cross(e1, e2))
 *        (not faced), r2 = dot(w, w);
 *        if cx > 0 && cy > 0 && r2 > 0 the shadow segment is walked: BVH::intersect of the ray
 *        (new_o, w), w unnormalised; the light is visible exactly when that hit's triangle index
 *        (the caller's numbering) is j, and then
 *            L = L + ((T o color_h) o emit_j) * (((cx / r2) * (cy / r2)) * kA);
 *        sampled = true, whether or not a shadow segment ran.
 *      Without a light draw, sampled = false.
 *   5. k == depth ends the path (the reference's last BRDF draw cannot be observed and is not made).
 *   6. new_d by Material::reflected_dir with trace()'s draws and its bound on the specular
 *      rejection loop; c = dot(n, new_d); T = ((2 * T) o color_h) * c; the ray becomes (new_o, new_d).
 * dot is (x x + y y) + z z and `o` the per-channel product, as everywhere in this header.
 *
 * Expectation. At a vertex that samples the hemisphere uniformly, trace()'s term
 * 2 cos rho Le(first hit) is the area integral of rho / pi * Le * cosx cosy / r^2 * V over the
 * emitters; step 4 estimates that integral with density 1 / A, and the EMIT hit it replaces is
 * dropped by `sampled`. The connection at hit k stands for an EMIT hit at k + 1, so it runs for
 * k < depth only and the depth cut is the same. Emission of other materials, unlisted EMIT
 * triangles and everything after a SPECULAR bounce stay with BRDF sampling.
 * Not in this definition: Russian roulette, light sampling at SPECULAR vertices. An emitter that
 * touches a diffuse surface gives the term of step 4 a heavy 1 / r^2 tail; the weighted estimator
 * below (PT_NEE_MIS_BALANCE, opt-in) removes it.
 *
 * The per-ray result is pt_ctx_trace's: the float32 sum over samples in order from +0, / spp.
 *
 * ---- the weighted estimator (multiple importance sampling, balance heuristic) ----
 * PT_NEE_MIS_BALANCE combines a vertex's light sample with the EMIT hit of its BRDF sample, which the
 * estimator above drops. It is steps 1-6 above with the same draws in the same order, so the
 * geometry, the LCG states, the segment counts, shadow_rays and light_draws of every path are the
 * unweighted estimator's. sqrtf and / are correctly rounded, each operation rounded on its own as
 * above. Let hA = 0.5f * kA (A / 2 pi; an exact scaling of kA). Two steps change:
 *
 *   Step 4, when the connection is allowed (cx > 0 && cy > 0 && r2 > 0):
 *        a = cy / r2 (the quotient g already holds), s = sqrtf(r2),
 *        wl = 1 / (1 + (a * hA) / s),
 *        and a visible light adds ((T o color_h) o emit_j) * (g * wl), g = ((cx / r2) * a) * kA.
 *   Step 2, an EMIT hit whose triangle is in the light table while `sampled` is true adds
 *        L = L + (T o emit) * wb instead of nothing, with
 *        cyd = fabsf(dot(n_hit, d)), n_hit the hit triangle's unit normal as trace() forms it (not
 *        faced), d the segment's direction, a = cyd / t, wb = 1 / (1 + t / (a * hA)).
 *   Every other case of step 2 is unchanged.
 *
 * wl = p_l / (p_l + p_b) and wb = p_b / (p_l + p_b) in solid angle: the area density 1 / A is
 * p_l = s^3 / (A cy) seen from the vertex, and Material::reflected_dir's hemisphere sample is
 * uniform (sin theta = -(2u - 1) is uniform, and the sample is flipped to the normal's side), so
 * p_b = 1 / 2 pi and p_b / p_l = a hA / s (step 4), a hA / t (step 2, for a unit d). d is a
 * hemisphere sample, unit to a few ulps, so for the same point the two weights sum to 1 to about
 * 1e-7, far below any sampling error; no normalisation is added to make it exact.
 *   * g * wl <= 2 cx / s <= 2 before rounding (g wl = 2 (cx / r2) q / (1 + q / s) with q = a hA, and
 *     q / (1 + q / s) < s; cx <= s because n is unit): a direct term is at most
 *     2 (T o color_h o emit_j) in every scene, and the 1 / r^2 tail is gone.
 *   * t > 0 and s > 0 wherever the weights are formed. Each weight is 1 / (1 + ratio) and not
 *     p / (p + p'): s / (s + a hA) is inf / inf = NaN where r2 overflows (a vertex far from a
 *     light: there g = +0 and the unweighted term is +0), and (a hA) / (t + a hA) is NaN where a hA
 *     overflows. In the form above an overflowing or vanishing operand gives a weight of +0 or 1:
 *     r2 = inf gives wl = 1 beside g = +0, a hA = inf gives wl = +0 and wb = 1, a hA = +0 gives
 *     wb = +0. What remains is g itself overflowing to inf beside wl = +0 (NaN), where the
 *     unweighted term is already inf.
 *   * The weights are evaluated whether or not the vertex's own light sample could contribute
 *     (cx <= 0, or occluded): the densities belong to the techniques, not to the sample drawn.
 *   * A light that sits in two leaves, or twice in the scene, is weighted as the visibility rule
 *     of step 4 counts it: by its caller's triangle index, with the table's A. */
#define PT_NEE_MIS_NONE 0        /* the estimator as first defined: an EMIT hit after a light draw adds nothing */
#define PT_NEE_MIS_BALANCE 1     /* the weighted estimator */
typedef struct pt_nee_options {  /* 16 bytes */
    int32_t mis;                 /* PT_NEE_MIS_*; any other value is PT_E_ARG */
    int32_t reserved[3];         /* must be 0 */
} pt_nee_options;

typedef struct pt_nee_stats {    /* 88 bytes */
    pt_trace_stats trace;        /* as pt_ctx_trace fills it; trace.rays counts path AND shadow segments */
    uint64_t shadow_rays;        /* shadow segments walked */
    uint64_t light_draws;        /* vertices that drew a light (step 4) */
    int32_t lights;              /* rows of the light table */
    float light_area;            /* A (0 without lights) */
} pt_nee_stats;

/* The light table of a scene (validated as by pt_scene_validate): *count = its rows, *area = A
 * (0 rows and 0.0f without lights); the first min(*count, cap) rows go to tri_out (the caller's
 * triangle indices) and cdf_out, either of which may be NULL. */
int pt_scene_lights(const pt_scene* scene, int32_t* tri_out, float* cdf_out, int64_t cap, int64_t* count,
                    float* area);

/* The estimator on the host over the caller's own arrays (no device needed), bit-identical to
 * pt_ctx_trace_nee. Arguments as pt_bvh_trace. */
int pt_bvh_trace_nee(const pt_scene* scene, const float* origins, const float* dirs, int64_t n,
                     const pt_trace_params* params, float* rgb_out, pt_nee_stats* stats);

/* The estimator for n rays on the context's scene; pointers, launch cuts, PT_E_RUNAWAY and
 * synchronisation as pt_ctx_trace. Uses buffers of its own and leaves a running sum valid. */
int pt_ctx_trace_nee(pt_ctx* ctx, const float* origins, const float* dirs, int64_t n,
                     const pt_trace_params* params, float* rgb_out, int is_device, pt_nee_stats* stats);

/* The estimator along the render's own camera rays: sample s of pixel p starts the LCG at
 * pt_sample_seed(p, s, seed) and makes Camera::get_ray's two draws first, so its first hits are
 * pt_ctx_render_aov's. img_out (rows*W*3) receives the float32 sum of params->spp samples in sample
 * order, / spp; `moments` (optional, every pointer optional) the sums S, Q and sem of those
 * samples as pt_ctx_render_moments defines them. The part fields work as in pt_ctx_render;
 * batch_spp and samples_per_item are not read. One-shot: there is no continuation, and the call
 * ends a running sum, as any render does. is_device covers img_out and the pointers of moments. */
int pt_ctx_render_nee(pt_ctx* ctx, const pt_camera* cam, const pt_params* params, float* img_out,
                      const pt_moments* moments, int is_device, pt_nee_stats* stats);

/* The three calls above with options: `options` NULL or mis == PT_NEE_MIS_NONE is the call above
 * (its bits, stats and errors; the three above are these with NULL), PT_NEE_MIS_BALANCE the
 * weighted estimator. Host and device forms stay bit-identical, and the stats have the same meaning. */
int pt_bvh_trace_nee_opt(const pt_scene* scene, const float* origins, const float* dirs, int64_t n,
                         const pt_trace_params* params, float* rgb_out, pt_nee_stats* stats,
                         const pt_nee_options* options);
int pt_ctx_trace_nee_opt(pt_ctx* ctx, const float* origins, const float* dirs, int64_t n,
                         const pt_trace_params* params, float* rgb_out, int is_device, pt_nee_stats* stats,
                         const pt_nee_options* options);
int pt_ctx_render_nee_opt(pt_ctx* ctx, const pt_camera* cam, const pt_params* params, float* img_out,
                          const pt_moments* moments, int is_device, pt_nee_stats* stats,
                          const pt_nee_options* options);

/* ---- material gradients of the light-sampling estimator --------------------------
 * The path geometry, the light choice (by area) and the balance-heuristic weights depend only on
 * geometry, roughness and the LCG, so the estimator above (steps 1-6, unweighted or
 * PT_NEE_MIS_BALANCE) is still a polynomial in color and emit_color, and the derivative below is
 * exact: no bias, no reparameterisation. The conventions are pt_ctx_trace_grad's: float32, one
 * rounding per operation, no contraction, `o` the per-channel product, the caller's triangle
 * indices; csrc/pt_nee.h states the arithmetic once for the host form and the kernel.
 *
 * Forward. rgb_out is the forward-form value of steps 1-6 evaluated at the override color / emit.
 * The light table (membership, cdf, A, kA, geometry) is ALWAYS that of the scene (the context's;
 * for the host form that of pt_scene_lights(scene)); it is never derived again from the override.
 * Only the emission of light j is taken from the override row of its triangle. So without
 * overrides, or with overrides under which pt_scene_lights would return the same table, rgb_out is
 * bit-identical to pt_ctx_trace_nee_opt; with any other override (a light's emission set to zero,
 * another EMIT triangle lit) it is the estimator over the scene's table: a consistent polynomial
 * whose gradient is the one returned, but not the estimator of the overridden scene.
 *
 * Per-path quantities. Path (i, s) has bounces k = 0 .. K-1 (non-EMIT hits that went on to the
 * BRDF draw of step 6) on triangles h_k with cosines c_k, then a terminal. A bounce whose light
 * draw was visible also has (j_k, g_k): the light's triangle and the scalar step 4 forms, g or
 * g * wl. The terminal is a miss; a non-EMIT hit on the last allowed segment; or an EMIT hit with
 * multiplier m: m = 1 when the hit is plain (step 2 adds T o emit), m = wb in the weighted
 * estimator's changed case, and in the unweighted estimator the hit that `sampled` and the table
 * drop is called dropped: it adds nothing below and is not counted.
 * w = grad_rgb[i] / (float)spp; Tw_0 = w, Tw_{k+1} = ((2 Tw_k) o color_{h_k}) * c_k.
 *
 * Suffix radiance per unit throughput, backwards: R_K is the terminal's value (emit * m for a
 * weighted hit, emit for a plain hit and for the last segment's non-EMIT hit, +0 for a miss or a
 * dropped hit); R_k = (emit_{h_k} + D_k) + ((2 R_{k+1}) o color_{h_k}) * c_k with
 * D_k = (color_{h_k} o emit_{j_k}) * g_k at a visible light draw; otherwise there is no D_k and
 * R_k = emit_{h_k} + ((2 R_{k+1}) o color_{h_k}) * c_k, pt_ctx_trace_grad's unwinding.
 *
 * Terms, in ascending k and in this order within a bounce:
 *   1. grad_emit[h_k] += Tw_k;
 *   2. with a visible light: grad_emit[j_k] += (Tw_k o color_{h_k}) * g_k, then
 *      grad_color[h_k] += (Tw_k o emit_{j_k}) * g_k;
 *   3. grad_color[h_k] += ((2 Tw_k) o R_{k+1}) * c_k.
 * A terminal hit then adds Tw_K * m to grad_emit[h_K] (Tw_K itself for a plain hit and for the last
 * segment's non-EMIT hit). A light draw that was not visible, or whose connection was not allowed,
 * adds nothing.
 *
 * Sums, `terms` and the degenerate cases are pt_ctx_trace_grad's: each destination is the float64
 * sum of its float32 terms in any order; n = 1, spp = 1 adds in the order above, bit for bit; a
 * term counts once for its three channels, only for a requested output, also when it is +-0 (it
 * is then not added); n == 0 zeroes the gradient outputs, depth 0 every output. */
typedef struct pt_nee_grad_stats {
    pt_nee_stats nee;       /* as pt_ctx_trace_nee_opt fills it */
    uint64_t terms;         /* contributions added to the requested ones of grad_color, grad_emit */
    double grad_ms;         /* zeroing, gathers, split: everything but the path kernel */
    int32_t lds_table;      /* 1: per-block gradient table in LDS; 0: global atomics only */
    int32_t reserved;
} pt_nee_grad_stats;

/* The terms on the host over the caller's own arrays (no device needed), summed in double in
 * (ray, sample, k) order; rgb_out as stated above. options NULL = PT_NEE_MIS_NONE. */
int pt_bvh_trace_nee_grad(const pt_scene* scene, const float* origins, const float* dirs, int64_t n,
                          const pt_trace_params* params, const pt_trace_grad_io* io,
                          pt_nee_grad_stats* stats, const pt_nee_options* options);
/* On the context's scene. Arguments, pointers (is_device covers the rays, params->states and every
 * pointer in io), launch cuts, PT_E_RUNAWAY and synchronisation as pt_ctx_trace_grad; options as
 * pt_ctx_trace_nee_opt. Uses buffers of its own: a running sum stays valid, and the override
 * never reaches the scene or its light table. */
int pt_ctx_trace_nee_grad(pt_ctx* ctx, const float* origins, const float* dirs, int64_t n,
                          const pt_trace_params* params, const pt_trace_grad_io* io, int is_device,
                          pt_nee_grad_stats* stats, const pt_nee_options* options);

/* ---- material gradients of the rendered image along its own camera rays ----------
 * The two gradients above for the image pt_ctx_render / pt_ctx_render_nee_opt compute: every
 * sample of a pixel has its own jittered camera ray, and one call covers all of them.
 *
 * Arguments. pt_trace_grad_io is reused unchanged with n = the part's pixels (rows * W):
 * grad_rgb and rgb_out are rows * W * 3 floats in the render's row order; color, emit, grad_color
 * and grad_emit are num_tris * 3 in the caller's triangle order. pt_params is read as
 * pt_ctx_render_nee reads it: spp (>= 1), depth (0..PT_MAX_DEPTH), seed and the three part fields;
 * batch_spp and samples_per_item are not read. `options` as in pt_ctx_trace_nee_opt.
 *
 * Sample (p, s) of part-local pixel p is the render's: its LCG starts at
 * pt_sample_seed(global pixel, s, seed), Camera::get_ray makes its two draws (the y jitter first),
 * and the path is then trace()'s (pt_*_render_grad) or steps 1-6 of the light-sampling definition
 * (pt_*_render_nee_grad).
 *
 * Forward: rgb_out is the float32 sum over s in order from +0, divided by (float)spp. Without
 * overrides it is bit-identical to pt_ctx_render / pt_ctx_render_nee_opt for the same camera,
 * params and part; with overrides it follows the forward rules of pt_ctx_trace_grad /
 * pt_ctx_trace_nee_grad unchanged (the light table is always the scene's).
 *
 * Terms: exactly those sections' per-path terms with w = grad_rgb[p] / (float)spp; the float64
 * any-order sums, the meaning of `terms` and the rules for +-0 terms are theirs. spp = 1 with a
 * 1x1 camera adds in k order and is reproducible bit for bit. The gradients of parts 0..N-1 each
 * cover their own pixels, and their sum is the whole frame's gradient (what a data-parallel fit
 * over several devices adds up).
 *
 * Degenerate cases: a part with no rows is PT_OK and zeroes the gradient outputs; depth 0 zeroes
 * every output; grad_color or grad_emit without grad_rgb is PT_E_ARG (for a part with pixels).
 * Stats are filled as by the ray forms, with paths = rows * W * spp. */

/* On the host over the caller's own arrays (no device needed): the camera ray in float32 with each
 * operation rounded on its own, bit-identical to the device's; sums in double in
 * (pixel, sample, k) order. */
int pt_bvh_render_grad(const pt_scene* scene, const pt_camera* cam, const pt_params* params,
                       const pt_trace_grad_io* io, pt_grad_stats* stats);
int pt_bvh_render_nee_grad(const pt_scene* scene, const pt_camera* cam, const pt_params* params,
                           const pt_trace_grad_io* io, pt_nee_grad_stats* stats,
                           const pt_nee_options* options);
/* On the context's scene. is_device != 0: every pointer in io is a DEVICE pointer on the context's
 * device (inputs left untouched), otherwise a host pointer. Launches are cut over samples; the
 * radiance slab and the in-order sum exist only when rgb_out is asked for, so a gradient-only call
 * (the backward pass of a fit) writes no radiance. PT_E_RUNAWAY is reported as by pt_ctx_render
 * (the results are still written). Synchronous; uses buffers of its own, so a progressive sum
 * stays valid (unlike pt_ctx_render_nee), and an override never reaches the scene or its light
 * table. */
int pt_ctx_render_grad(pt_ctx* ctx, const pt_camera* cam, const pt_params* params,
                       const pt_trace_grad_io* io, int is_device, pt_grad_stats* stats);
int pt_ctx_render_nee_grad(pt_ctx* ctx, const pt_camera* cam, const pt_params* params,
                           const pt_trace_grad_io* io, int is_device, pt_nee_grad_stats* stats,
                           const pt_nee_options* options);

/* Number of rows of part `part_index` for the given partition. */
int32_t pt_part_rows(int32_t res_y, int32_t part_index, int32_t part_count, int32_t band_rows);

/* One-shot: create context on device params->... (device 0), upload, render
 * the whole image (part 0 of 1) into host out_rgb (res_x*res_y*3 floats). */
int pt_render_f32(const pt_scene* scene, const pt_camera* cam, const pt_params* params,
                  float* out_rgb, pt_stats* stats);

/* One-shot on several GPUs of this process: part p of the row partition (bands of
 * params->band_rows rows, default 1; row h -> part (h / band) % n_devices) renders on
 * devices[p] from its own host thread into device memory; with distinct devices the
 * parts are gathered to devices[0] by one RCCL group of ncclSend/ncclRecv (communicators
 * from ncclCommInitAll, cached per device list) and assembled there, then copied to
 * out_rgb (the whole image, as pt_render_f32). A device may be listed more than once
 * (then the rows are assembled on the host). The image is bit-identical for any device
 * list (per-sample seeding); stats: rays/paths summed, kernel_ms the slowest part's,
 * per-device times and rays, gather path and time. Replaces render_gpu's tile loop on
 * one GL context (render.h:109-152, tiles 128-139) with every visible GPU. */
int pt_render_f32_devices(const pt_scene* scene, const pt_camera* cam, const pt_params* params,
                          const int32_t* devices, int32_t n_devices, float* out_rgb, pt_stats* stats);
/* As pt_render_f32_devices, then gamma_correct + save_png quantisation (image.h:41-55) on
 * devices[0] after the gather: rgb8 receives res_x*res_y*3 bytes, top row first, equal to
 * pt_image_to_rgb8 of the linear image (a quarter of its device-to-host bytes). */
int pt_render_rgb8_devices(const pt_scene* scene, const pt_camera* cam, const pt_params* params,
                           const int32_t* devices, int32_t n_devices, float gamma, uint8_t* rgb8,
                           pt_stats* stats);

/* ---- post-process (image.h:41-62) -------------------------------------- */
/* gamma (powf(x, 1/gamma)), clamp to [0,1], *255, truncate, vertical flip:
 * rgb8 is top row first, as the PNG written by Image::save_png. */
int pt_image_to_rgb8(const float* linear_rgb, int32_t res_x, int32_t res_y, float gamma,
                     uint8_t* rgb8);
/* Thresholds of the device quantiser for gamma > 0: thr255[k-1] = the least float x >= 0
 * whose 8-bit value under pt_image_to_rgb8 (host powf) is >= k, k = 1..255; *neg_mode
 * (if non-NULL) = how a negative value quantises: 0 -> 255 (NaN power), 1 -> 0 (odd
 * integer exponent), 2 -> as |x| (even integer exponent). */
int pt_rgb8_thresholds(float gamma, float* thr255, int32_t* neg_mode);
/* ---- OBJ/MTL ingestion: BVH::load_obj (bvh.h:184-242) through the reference's
 * vendored tinyobjloader (triangulation, number parsing and MTL rules restated in
 * csrc/pt_obj.cpp). Triangles come out in the order load_obj adds them. */
typedef struct pt_obj pt_obj;
/* Parse `filename`; MTL files are searched in mtl_search_path (':'-separated; NULL or
 * "" = the OBJ file's directory, as ObjReader::ParseFromFile). PT_E_IO if the file
 * cannot be opened; PT_E_ARG for a malformed face line, a face without a material or
 * a vertex index past the end (the reference's undefined behaviour). */
int pt_obj_load(const char* filename, const char* mtl_search_path, pt_obj** out);
int32_t pt_obj_num_tris(const pt_obj* obj);
/* verts: 9 floats per triangle (v1, v2, v3); mats: the bvh.h:220-238 mapping
 * (illum 1 -> DIFFUSE(Kd), 2 -> EMIT(Ka), else DIFFUSE(0.5)); illum: the MTL value
 * behind each triangle (load_obj reports "Unknown material type" for the others).
 * Any output may be NULL. */
int pt_obj_triangles(const pt_obj* obj, float* verts, pt_material* mats, int32_t* illum);
/* tinyobjloader-style warnings collected while parsing ("" if none). */
const char* pt_obj_warnings(const pt_obj* obj);
void pt_obj_free(pt_obj* obj);

/* Write an 8-bit RGB PNG (top row first). */
int pt_write_png(const char* filename, const uint8_t* rgb8, int32_t res_x, int32_t res_y);

/* ---- cached multi-device contexts ------------------------------------- */
/* pt_render_*_devices keep one context per listed device (keyed by the device list) and
 * the scene last uploaded to it, so a process that renders several scenes or frames in a
 * row (the reference's modified_cornell.cc renders six, modified_cornell.cc:14, 107) pays
 * context creation once and re-uploads a scene only when its arrays change. This frees
 * every cached context and its device memory (radiance slabs, scene, part buffers). Safe
 * to call at any time; a later pt_render_*_devices call creates fresh contexts. */
void pt_devices_release(void);

#ifdef __cplusplus
}
#endif
#endif /* PT_HIP_H */
