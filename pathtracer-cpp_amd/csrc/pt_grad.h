// pt_grad.h — the boundary between pt_kernel.hip (pt_ctx_trace_grad, pt_ctx_render_grad) and
// pt_grad.hip: material gradients of trace() on caller-supplied rays and on the
// render's own camera rays (§3.29). Host only.
#pragma once

#include "pt_launch.h"

namespace pt {

// pt_ctx_trace's placement (paths_plan) with one more part after the records: the block's
// gradient table, 6 doubles per caller triangle, 16-byte aligned.
struct GradPlan {
    WalkPlan walk;     // lds_bytes includes the table
    int lds_tab;       // 1: per-block table in LDS, flushed once; 0: global atomics only
    size_t tab_off;    // byte offset of the table in the block's LDS
    int camera = 0;    // 1: the kernels fed from the part's camera rays (pt_grad_cam_kernel)
};
// `table_rows`: the caller's triangles; `items`: rays x samples of the largest launch; depth >= 1.
// PT_GRAD_LDS=0 (test hook) forces the global form. camera: plan for the camera-ray kernels.
void grad_place(const QueryScene& sc, int table_rows, size_t lds_usable, int depth, GradPlan& plan);
int grad_plan(const QueryScene& sc, int table_rows, size_t lds_usable, int num_cus, int depth, int64_t items,
              GradPlan& plan, bool camera = false);

// One launch over p.m rays x p.spp samples (device pointers); no synchronisation. p.ctr[2] counts
// the terms. `mats`: the materials to evaluate at, 2 float4 per packed triangle (the scene's own
// or grad_gather_mats' output).
struct GradLaunch {
    PathsLaunch p;
    const f4* mats;
    const float* grad_rgb;  // p.m x 3, or nullptr: forward only
    double* table;          // table_rows x 6 doubles {d color rgb, d emit rgb}, zeroed by the caller
    int32_t table_rows;
    int want_rgb, want_color, want_emit;
    // A camera plan's launch: samples [s_begin, s_begin + p.spp) of the part's p.m = shape->npix
    // pixels, as nee_launch takes them; the terms' weight is grad_rgb[pixel] / (float)spp_total.
    // p.org, p.dir, p.states and p.ray_base are not read; p.slab may be nullptr without want_rgb.
    const pt_camera* cam;
    const pt_params* prm;
    const PartShape* shape;
    int32_t s_begin, spp_total;
};
int grad_launch(void* stream, const QueryScene& sc, const GradPlan& plan, const GradLaunch& l);
// out[2 r], out[2 r + 1] = the scene's material of packed triangle r with color / emit replaced by
// the caller-ordered override rows (either may be nullptr).
int grad_gather_mats(void* stream, const QueryScene& sc, const float* color, const float* emit, f4* out);
// grad_color[3 t + c] = table[6 t + c], grad_emit[3 t + c] = table[6 t + 3 + c] (either may be nullptr).
int grad_split_table(void* stream, const double* table, int32_t table_rows, double* grad_color, double* grad_emit);

}  // namespace pt
