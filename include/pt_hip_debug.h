/*
 * pt_hip_debug.h — test and tuning hooks of libpt_hip.so, kept apart from the drop-in
 * boundary (include/pt_hip.h). Nothing a reference-side binding needs is declared here;
 * the tests (tests/test_capi.py, tests/test_gpu_parity.py, tests/test_math.py) call these
 * through ctypes. Every symbol is exported by libpt_hip.so.
 */
#ifndef PT_HIP_DEBUG_H
#define PT_HIP_DEBUG_H

#include "pt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Run the device copies of the path's math primitives on `device`:
 * which = 0: acosf(in[i]) -> out[i]
 *         1: sincosf(in[i]) -> out[2i] = sin, out[2i+1] = cos
 *         2: BRDF sample; in[9i..9i+8] = {lcg state (bits), material type (bits),
 *            roughness, d.xyz, n.xyz} -> out[4i..4i+3] = {dir.xyz, state after (bits)} */
int pt_debug_math(int device, int which, const float* in, int n, float* out);
/* Exhaustive check of a fast device sequence against its IEEE-exact counterpart over
 * every float bit pattern in [lo_bits, hi_bits] (NaN inputs skipped), on `device`:
 * which = 0: rcp_exact(x) vs 1.0f / x;  1: sqrt_exact(x) vs sqrtf(x);
 *         2: acosf fast vs restatement;  3: sincosf fast vs restatement (pt_math.h);
 *         4: div_by_rcp(x, b, RN(1/b)) vs x / b for a hashed divisor b per input x;
 *         5: rcp3_exact on {x, x, x} vs 1.0f / x, the unit-vector form for |x| <= 2, the two-sided
 *            form elsewhere;
 *         6: rcp3_exact on {x, b, c} vs the three IEEE reciprocals, b and c hashed per input and, for
 *            one input in 16, forced out of range (+-0, subnormal, 2^127, +-inf, (2^126, 2^128)), so
 *            that every wave holds lanes on both sides of the wave-uniform fallback;
 *         7: normalize_fast on {x, b, c} vs the IEEE square root and divisions, b and c in
 *            [2^-40, 2^40] and forced as in 6;  8: the same without the forced inputs;
 *         9: 6 without the forced inputs (waves keep the fast results), and with a NaN as b for one
 *            input in 16: that component must come out NaN (any payload), the other two exact.
 * *mismatches = number of differing results, *first_bad = lowest differing input bits
 * (0xffffffff if none). */
int pt_debug_sweep(int device, int which, uint32_t lo_bits, uint32_t hi_bits, uint64_t* mismatches,
                   uint32_t* first_bad);
/* The device quantiser (pt_ctx_render_rgb8's second half) on a host image: rgb8 = top
 * row first, as pt_image_to_rgb8. */
int pt_debug_rgb8(int device, const float* linear_rgb, int32_t res_x, int32_t res_y, float gamma, uint8_t* rgb8);
/* Test hook, no device needed: the multi-device gather's communicator cache driven through a
 * fake RCCL table whose call `fail_step` fails (0 init, 1 group start, 2 send, 3 recv,
 * 4 group end, -1 none); out[6] = {created, aborted, still live, cache entries after the
 * first gather, second gather got a fresh set, first gather's result}. */
int pt_debug_rccl_failover(int32_t n_devices, int32_t fail_step, int64_t* out);
/* Rebuild the wide tree (width 4 or 8) of `scene` and check its invariants exactly on the
 * host: quantised child boxes contain the reference's boxes, child links, triangle ranks
 * and exact leaf boxes, every triangle stored once. Returns the violation count (0 = ok). */
int pt_debug_wide_verify(const pt_scene* scene, int32_t width);
/* Test hook, no device needed: *hash = FNV-1a 64 of every array and scalar the scene packing
 * produces (device layout, flat leaves, wide tree), to check that the packing's thread
 * schedule (PT_PACK_THREADS) leaves its output bit-identical. */
int pt_debug_pack_hash(const pt_scene* scene, uint64_t* hash);
/* Generate (into src_out, if non-NULL) and compile the hipRTC scene-specialised flat
 * kernel for `scene` without touching a device. Returns the code-object size (> 0). */
int pt_rtc_check(const pt_scene* scene, char* src_out, size_t cap);
/* Test hook, no device needed: start the scene kernel's compile in the background, as
 * pt_ctx_set_scene does, and return at once (1: a compile is running, 0: already done). */
int pt_debug_rtc_start(const pt_scene* scene);
/* Test hook, no device needed: the scene kernel's code-object caches (an on-disk cache
 * under $PT_RTC_CACHE_DIR, $XDG_CACHE_HOME/pathtracer-amd/rtc or ~/.cache/pathtracer-amd/rtc,
 * off with PT_RTC_CACHE=0; entries verified by sha256 on load). op 0 forgets this process's
 * compiles, 1 disk hits, 2 rejected entries, 3 compiles so far, 4 the last compile's wall time
 * in microseconds, 5 compiles done by the compile server (bin/pt_rtc_server). */
int64_t pt_debug_rtc_cache(int32_t op);

/* Test hook: how a context's scene is rendered. out[0] = 1 if the scene kernel unwinds with
 * pre-doubled albedo (the host's radiance bound passed, pt_launch.hip: albedo_x2_ok), out[1] =
 * 1 if the scene holds a SPECULAR material, out[2] = 1 if a hipRTC scene kernel was requested
 * for the scene, out[3] = wide nodes (0 = no wide tree), out[4] = 1 if every bounce material is
 * dark (emission +0, finite albedo: finish_path skips the unwinding of +0 paths). */
int pt_debug_ctx_flags(const pt_ctx* ctx, int32_t out[5]);
/* Test hook: the launch plan of ctx's last pt_ctx_render* / pt_ctx_render_progressive call that
 * reached its launches (all zero before one). out[] in this order:
 *   [0] kernel_path (PT_PATH_*)   [1] flat   [2] wide   [3] pairs   [4] pair_queue (entries per wave)
 *   [5] lds_bytes (dynamic LDS per block)   [6] lds_scene
 *   [7] wide_rows   [8] wide_queue   [9] wide_top   [10] blocks_per_cu (of the last launch)
 *   [11] batch   [12] per_item   [13] fused   [14] tail
 *   [15] flags_pm (1 pixel-major bits, 0 sample-major, -1 dense slabs without flag bits)
 *   [16] trace_launches   [17] regen_thresh   [18] theta_lanes
 *   of the last launch (0 without one): [19] grid   [20] chunk   [21] static_items
 *   [22] acc_every (0 when that launch sums no earlier slab)
 *   [23] the context's num_cus.
 * [10] and [19..22] depend on the device's CU count, the others on the scene and parameters only. */
int pt_debug_ctx_plan(const pt_ctx* ctx, int64_t out[24]);
/* Test hook, no device needed: where the binary walk of the ray queries (tri_f4 = 3 float4 per
 * triangle in the LDS scene) and of pt_ctx_trace (tri_f4 = 5: with materials) keeps its data for a
 * tree of num_nodes nodes, num_tris triangles and depth tree_depth, rec_rows path-record rows
 * (depth - 1) and lds_usable bytes of LDS per CU, under the placement hooks (PT_LDS_SCENE_BYTES,
 * PT_QUERY_LDS_STACK, PT_TRACE_LDS_REC). out[] = {scene in LDS, stack in LDS, records in LDS,
 * dynamic LDS bytes per block}. */
int pt_debug_walk_placement(int32_t num_nodes, int32_t num_tris, int32_t tree_depth, int32_t tri_f4,
                            int32_t rec_rows, uint64_t lds_usable, int32_t out[4]);
/* Test hook, no device needed: 1 if `scene` passes the dark-path gate (every non-emitting
 * triangle: emission +0, finite albedo, a unit-length shading normal, SPECULAR roughness
 * |r| <= 1.15 so that cos theta is finite; pt_launch.hip scene_dark), 0 if not, < 0 on error. */
int pt_debug_scene_dark(const pt_scene* scene);
/* Test hook, no device needed: the last-ray rule's predicate (emit_reject, pt_math.h) on n
 * rays: box6[6i..] = {E lb.xyz, E rt.xyz}, org / dir 3 floats each -> out[i] = 1 if ray i provably
 * fails the reference's slab test for every box inside E. */
int pt_debug_emit_reject(const float* box6, const float* org, const float* dir, int64_t n, uint8_t* out);
/* Test hook, no device needed: the flat kernels' form of the rule (emit_slab_reject, pt_math.h) on
 * n rays: box6 and org as above, inv 3 floats each (the kernels pass 1 / dir) -> out[i] = 1 if E
 * itself fails the slab test, under the predicate's guard, or E is empty (lb > rt on an axis). */
int pt_debug_emit_slab_reject(const float* box6, const float* org, const float* inv, int64_t n, uint8_t* out);
/* Test hook for the one-verdict-per-ray policy (PT_DOMAIN_ONCE; rcp3_exact_v and
 * emit_slab_reject_given, pt_math.h) on n rays against ONE box: box6 = {E lb.xyz, E rt.xyz}, org / dir
 * 3 floats each; unit != 0 runs the unit-vector form of the predicate (the bounce's), 0 the two-sided
 * one (camera rays, the specular sample). device < 0: the host form, each ray its own wave; device
 * >= 0: one block of 256 threads on that device, ray i in lane i mod 64 of wave (i / 64) mod 4, where
 * the verdict is the wave's. out[6i..] = {rcp3_exact's own range predicate holds, finite_nonzero of
 * every component of inv (the slab guard's inv half), all_finite(inv) (the top-of-iteration test),
 * the new verdict (1 = "in the domain", the wave did not fall back), emit_slab_reject, the guard-free
 * form as shade_inv calls it (inv half: the verdict, or the per-lane test in a wave that fell back)};
 * inv3[3i..] = rcp3_exact_v's result. */
int pt_debug_domain_once(int device, const float* box6, const float* org, const float* dir, int64_t n, int unit,
                         uint8_t* out, float* inv3);
/* Test hook, no device needed: hemisphere_dir (pt_math.h, the host form) from LCG state lcg[i] about
 * the normal nrm[3i..] -> dir3[3i..]. */
int pt_debug_hemisphere_dir(const uint32_t* lcg, const float* nrm, int64_t n, float* dir3);
/* Test hook, no device needed: the emitter box the host computes for `scene` (the union of the
 * tree's leaf boxes that hold an EMIT triangle; lb = +inf, rt = -inf when there is none, which
 * rejects every last ray). Returns 1 if the rule is on (a dark scene, PT_EMIT_REJECT not 0), 0 if
 * off (out is then all zero), < 0 on error. */
int pt_debug_emit_box(const pt_scene* scene, float out[6]);
/* Test hook: the same for a context's scene (*on, box[6]), and *early = the paths the rule ended
 * in the context's last render. Counted only by kernels built with PT_COUNT_EARLY=1: the offline
 * render kernels are, the hipRTC scene kernel under PT_RTC_DEFINES=PT_COUNT_EARLY=1 (else 0).
 * Any pointer may be NULL. */
int pt_debug_ctx_emit_reject(const pt_ctx* ctx, int32_t* on, float box[6], uint64_t* early);
/* Test hook, no device needed: the loop control of the flat kernels' shared camera-ray stock
 * (pt_raystack.h), one decision per call. which = 0: 1 if the generator runs with `count` rays in
 * stock, n lanes without a path, `reserve`, and flag = the pool is dry; 1: count after a fill in
 * which n lanes got an item; 2: 1 if that fill found the pool dry; 3: the slot the lane of rank n
 * takes (< 0: none); 4: count after n lanes asked; 5: 1 if the wave is done (flag = a lane is on a
 * path, n = the pool is dry). < 0 on a bad `which`. */
int pt_debug_ray_stack(int32_t which, int32_t count, int32_t n, int32_t reserve, int32_t flag);
/* Test hook, no device needed: the dynamic LDS of a flat-kernel block (pt_flatlds.h) for a scene of
 * num_tris triangles, a box table of box_tab_bytes, pair queues of pair_queue entries per wave and
 * rec_size path records per lane. out: the byte offsets of [0] triangles [1] materials [2] camera
 * rows [3] winners [4] camera items [5] box table [6] pair queues [7] record triangles [8] record
 * cosines, and [9] the block's bytes (what plan_flat asks of the launch). */
int pt_debug_flat_lds(int32_t num_tris, int32_t box_tab_bytes, int32_t pair_queue, int32_t rec_size, uint32_t out[10]);
/* Test hook: process-wide counters. which = 0: contexts created (pt_ctx_create), 1: scene
 * uploads (pt_ctx_set_scene), 2: cached multi-device context sets live, 3: uploads skipped
 * because a cached context already held the same scene. */
int64_t pt_debug_counter(int32_t which);
/* Test hook, no device needed: the host form's camera ray (pt_bvh_render_grad) of sample `sample` of
 * the n part-local pixels first .. first + n - 1 of the part `params` names: org and dir (n * 3
 * floats each) and states (n), the LCG state after Camera::get_ray's two draws. */
int pt_debug_host_camera_rays(const pt_camera* cam, const pt_params* params, int32_t sample, int64_t first, int64_t n,
                              float* org, float* dir, uint32_t* states);

#ifdef __cplusplus
}
#endif
#endif /* PT_HIP_DEBUG_H */
