// pt_nee_grad.h — the boundary between pt_kernel.hip (pt_ctx_trace_nee_grad, pt_ctx_render_nee_grad)
// and pt_nee_grad.hip: material gradients of the light-sampling estimator on caller-supplied rays
//  and on the render's own camera rays (§3.29). Host only.
#pragma once

#include "pt_launch.h"

namespace pt {

// The light-sampling kernels' placement (stack rows, the scene with materials) with `levels` =
// depth - 1 path records of FOUR words a lane (packed triangle, cosine, light or -1, g), placed as
// 2 x levels of place_walk's two-word record rows, and then, as GradPlan, the block's gradient
// table: 6 doubles per caller triangle, 16-byte aligned.
struct NeeGradPlan {
    WalkPlan walk;   // rec = 2 * levels; lds_bytes includes the table
    int levels;      // record levels per lane
    int lds_tab;     // 1: per-block table in LDS, flushed once; 0: global atomics only
    size_t tab_off;  // byte offset of the table in the block's LDS
    int camera = 0;  // 1: the kernels fed from the part's camera rays (pt_nee_grad_cam_kernel)
};
// `table_rows`: the caller's triangles; `items`: rays x samples of the largest launch; depth >= 1.
// PT_GRAD_LDS=0 and PT_TRACE_LDS_REC=0 (test hooks) force the global forms.
int nee_grad_plan(const QueryScene& sc, int table_rows, size_t lds_usable, int num_cus, int depth, int64_t items,
                  NeeGradPlan& plan, bool camera = false);

// One launch over p.m rays x p.spp samples (device pointers); no synchronisation. p.ctr: 6 zeroed
// u64 as nee_launch's, [2] counts the terms. p.grec: 2 * plan.walk.rec_words words.
struct NeeGradLaunch {
    PathsLaunch p;
    const f4* mats;         // the materials to evaluate at (the scene's own or grad_gather_mats' output)
    const f4* lemit;        // per light: the emission to evaluate at (nee_grad_gather_lights' output)
    const float* grad_rgb;  // p.m x 3, or nullptr: forward only
    double* table;          // table_rows x 6 doubles {d color rgb, d emit rgb}, zeroed by the caller
    int32_t table_rows;
    int want_rgb, want_color, want_emit;
    int mis;                // PT_NEE_MIS_*
    // A camera plan's launch, as GradLaunch's: samples [s_begin, s_begin + p.spp) of the part's
    // p.m = shape->npix pixels, the terms weighted by grad_rgb[pixel] / (float)spp_total.
    const pt_camera* cam;
    const pt_params* prm;
    const PartShape* shape;
    int32_t s_begin, spp_total;
};
int nee_grad_launch(void* stream, const QueryScene& sc, const NeeGradPlan& plan, const NeeGradLaunch& l,
                    const NeeLights& lights);
// out[j] = the emission of light j: row lights.tri[j] of the caller-ordered override `emit`, or
// (emit nullptr) the light table's own copy. out holds lights.count float4.
int nee_grad_gather_lights(void* stream, const NeeLights& lights, const float* emit, f4* out);

}  // namespace pt
