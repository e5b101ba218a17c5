// pt_rtc.h — the flat path's scene-specialised kernel (pt_trace_flat_rtc): its
// source generated per scene, compiled through hipRTC in the background, cached per process and on
// disk, loaded per device (pt_rtc.hip). pt_kernel.hip starts a job in pt_ctx_set_scene and renders
// pick the kernel up when it is ready.
#pragma once

#include <hip/hip_runtime_api.h>

#include <future>
#include <memory>
#include <string>
#include <vector>

#include "pt_internal.h"

namespace pt {

// A hipRTC compile's result: the code object, or why there is none.
struct RtcCode {
    std::vector<char> code;
    std::string status;
    std::string disk_key;  // set when the code object was read from the on-disk cache
};
typedef std::shared_future<std::shared_ptr<const RtcCode>> RtcFuture;

// What is fixed once pt_ctx_set_scene has run and the scene kernel's source holds as constants
// (PT_KCONST). Test hooks and a failed theta-table allocation can move these
// between set_scene and a launch: a launch whose plan differs does not run that kernel
// (plan_render, pt_kernel.hip).
struct RtcBaked {
    bool on = false;  // PT_KCONST != 0: the values below are constants of the source (off: it reads the arguments)
    int num_tri4 = 0, num_mat4 = 0;  // float4 counts of the LDS scene copy
    int box_tab_bytes = 0;           // the box-level pairs' LDS table
    bool pairs = false;              // the pair queues are on (pair_queue > 0)
    int theta_lanes = 0;             // theta_choice's lane bound; 0: the table path is not compiled
    // whether a kernel built with these may run a launch with `plan`'s values
    bool runs(const RtcBaked& plan) const {
        return !on || (num_tri4 == plan.num_tri4 && num_mat4 == plan.num_mat4 && box_tab_bytes == plan.box_tab_bytes &&
                       pairs == plan.pairs && theta_lanes == plan.theta_lanes);
    }
};
// The values for a scene of `num_tris` triangles under the hooks as they are now (theta_lanes:
// what theta_choice intends; a launch compares what it got).
RtcBaked rtc_baked(int num_tris, bool specular, int flat_boxes);
// The theta table's lane bound a scene asks for (theta_choice and rtc_baked go by this one rule).
int theta_lanes_wanted(bool specular);

// Box-level pairs (PT_BOX_PAIRS=1, test hook): the number of distinct leaf boxes when every leaf
// holds one triangle and no box bounds more than two leaves (`tab`: the kernel's LDS table), else 0.
int flat_box_pairs(const std::vector<f4>& leaves, int n, std::vector<uint16_t>* tab = nullptr);
// Every leaf of the flat list holds exactly one triangle.
bool leaves_single(const std::vector<f4>& leaves, int n);
// The scene kernel's source for a flat leaf list and the scene's flags (scene_has_specular,
// PackedScene::coords_small, albedo_x2_ok, scene_dark: pt_launch.h).
// `emit`: the last-ray rule's box (scene_emit_box), baked in as literals when it is on.
// `baked`: what else the source holds as constants.
std::string rtc_flat_source(const std::vector<f4>& leaves, int n, bool specular, bool tri_fast, bool albedo_x2,
                            bool dark, const EmitBox& emit, const RtcBaked& baked);
// The compile job for `src`, shared by every context and device that asks for the same source.
RtcFuture rtc_job(const std::string& src);
// Whether compiles can run in the background (else rtc_job's compile runs on first get()).
bool rtc_async_ready();
// Wait for every background compile started so far; returns how many were still running.
int rtc_wait_all();
// Load a finished compile of `src` on `device` (once per device and source); nullptr and `status`
// when there is none ("evicted": a disk-cache entry the runtime refused, to be compiled again).
hipFunction_t rtc_load(int device, const std::string& src, const RtcCode& code, std::string& status);

}  // namespace pt
