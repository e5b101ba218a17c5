// pt_nee.hip — the light-sampling estimator (include/pt_hip.h: the definition)
// over the binary child-pair walk (gfx950).
//
//   pt_nee_kernel<kLdsScene, kLdsStack>      the caller's buffer of rays (BufferRays, pt_paths.h)
//   pt_nee_cam_kernel<kLdsScene, kLdsStack>  the part's own camera rays (PartRays, pt_paths.h)
//   pt_nee_mis_kernel, pt_nee_mis_cam_kernel the same two with the balance-heuristic weights
//                                            (PT_NEE_MIS_BALANCE; kMis in shade_nee)
//
// The loop is pt_paths.h's one-path-per-lane loop: a work item is (ray or pixel, sample), numbered
// sample-major, a lane takes its next item by claim_item, and item j's radiance is record j of
// the launch's dense slab [sample][ray][rgb]; the per-ray sum over samples is the separate
// in-order pass of pt_ctx_trace. The path runs in forward form (throughput T and radiance L in
// registers), so there are no path records: the LDS holds only the scene and the stack.
//
// One loop iteration is ONE closest-hit walk of every lane with an item: either the next segment
// of its path, or the pending shadow segment of the vertex it just shaded. shade_nee makes the
// vertex's draws at once (the light's three, then the BRDF's), and when the light can contribute
// it puts the shadow ray (new_o, w) in front of the bounce ray (new_o, new_d), whose direction
// waits in registers beside the term a visible light adds. So intersect_tree runs once per
// iteration for the whole wave instead of once per kind of segment.
//
// Termination: every iteration advances each lane with an item, either from segment k to k + 1
// (shade_nee increments k, and ends the item at k == depth at the latest) or from its shadow
// segment to the bounce it held back (a shadow segment is only ever queued by shade_nee, never by
// another shadow segment). An item therefore ends within 2 * depth iterations, and a lane without
// an item either claims one or, once the pool is empty, stays out for good.
//
// Slab-form gate: as in paths_body, evaluated on every iteration (a caller's ray can be
// non-finite, and after it so can a bounce origin or a shadow direction).
//
// LDS: [nodes, tris, mats (kLdsScene)] [stack: rows x kBlock int (kLdsStack)], every part a
// multiple of 16 B; otherwise the stack rows are P.gstack[block][row][lane].
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>

#include "pt_nee.h"
#include "pt_paths.h"

namespace pt {

static_assert(kSpecularIterBound == kMaxSpecularIters, "host and device bound of the specular rejection loop");

// The light table on the device and the call's two counters.
struct NeeArgs {
    const float* __restrict__ cdf;            // per light: running area sum
    const int32_t* __restrict__ ltri;         // per light: the caller's triangle index
    const float4* __restrict__ lgeom;         // per light: kNeeLightF4 rows (pt_internal.h: LightTable::geom)
    const uint8_t* __restrict__ listed;       // per caller triangle: 1 when it is a light
    const int32_t* __restrict__ rank_tri;     // rank position -> the caller's triangle index
    unsigned long long* __restrict__ nctr;    // [0] shadow segments, [1] light draws
    int nlights;
    float area, kA;
};

__device__ __forceinline__ v3 f4_xyz(float4 a) { return v3{a.x, a.y, a.z}; }

// Steps 2-6 of the definition for segment k + 1 of the path, after its BVH::intersect. Returns
// true when the path ends here. Otherwise T, sampled and o are the next segment's, and the lane's
// next walk is (o, d): the bounce ray, or (shadow set) the shadow ray, with the bounce direction in
// `bd`, the light's triangle in `lj` and the term a visible light adds in `C`. kMis: the light's
// weight is folded into C here, before the shadow walk, and an EMIT hit on a listed triangle after
// a light draw adds its weighted emission (d is that vertex's hemisphere sample, t its distance), so
// nothing more than without the weights stays live across intersect_tree.
template <bool kMis>
__device__ __forceinline__ bool shade_nee(const TraceArgs& A, const NeeArgs& N, const float4* __restrict__ mats,
                                          const float4* __restrict__ tris, int hit, float t, Lcg& g, v3& o, v3& d, int& k,
                                          v3& T, v3& L, bool& sampled, bool& shadow, v3& bd, v3& C, int& lj, bool& drew) {
    k++;
    if (hit < 0) return true;
    const float4 m0 = mats[2 * hit], m1 = mats[2 * hit + 1];
    const int type = __float_as_int(m0.x);
    const v3 emit{m1.x, m1.y, m1.z};
    if (type == PT_MAT_EMIT) {
        // the emitter the last vertex's light draw stood for adds nothing
        bool add_it = true;
        if (sampled) add_it = N.listed[N.rank_tri[hit]] == 0;
        if (add_it) L = nee_add_emit(L, T, emit);
        if (kMis && !add_it) {  // the BRDF sample reached a light: its share of the two techniques
            const float4 th = tris[3 * hit + 2];
            L = nee_add_emit_weighted(L, T, emit, nee_brdf_weight(v3{th.y, th.z, th.w}, d, t, N.kA));
        }
        return true;
    }
    L = nee_add_emit(L, T, emit);
    if (k >= A.depth) return true;  // no light draw at k == depth, and the last BRDF draw is not made
    const v3 color{m0.y, m0.z, m0.w};
    const float4 tn = tris[3 * hit + 2];
    v3 n{tn.y, tn.z, tn.w};
    if (!(dot(n, d) < 0.0f)) n = neg(n);  // triangle.h:48
    const v3 hp = add(o, scale(d, t));
    const v3 no = add(hp, scale(n, 1e-4f));  // SHIFT_BIAS, render.h:16, 52
    const bool draw = type != PT_MAT_SPECULAR && N.nlights > 0;
    bool want = false;
    v3 w{0.0f, 0.0f, 0.0f};
    if (draw) {
        const float x1 = g.next01();
        const float x2 = g.next01();
        const float x3 = g.next01();
        const int j = nee_pick(N.cdf, N.nlights, x1 * N.area);
        const float4* __restrict__ G = N.lgeom + (size_t)kNeeLightF4 * j;
        const v3 y = nee_point(f4_xyz(G[0]), f4_xyz(G[1]), f4_xyz(G[2]), x2, x3);
        float gw;
        if (kMis ? nee_connect_mis(y, no, n, f4_xyz(G[3]), N.kA, w, gw) : nee_connect(y, no, n, f4_xyz(G[3]), N.kA, w, gw)) {
            want = true;
            C = nee_direct(T, color, f4_xyz(G[4]), gw);
            lj = N.ltri[j];
        }
    }
    sampled = draw;
    drew = draw;
    v3 nd;
    if (type == PT_MAT_SPECULAR) {
        if (!specular_dir(g, d, n, m1.w, kMaxSpecularIters, nd)) atomicAdd(A.ctr + 3, 1ull);
    } else {
        // shade's choice (pt_trace.h): the theta table in waves with few sampling lanes
#if PT_THETA_TAB == 1
        nd = hemisphere_dir_tab(g, n, kernarg_args()->theta_tab);
#elif PT_THETA_TAB == 2
        if ((int)__popcll(__ballot(true)) <= kernarg_args()->theta_lanes)
            nd = hemisphere_dir_tab(g, n, kernarg_args()->theta_tab);
        else
            nd = hemisphere_dir(g, n);
#else
        nd = hemisphere_dir(g, n);
#endif
    }
    T = nee_throughput(T, color, dot(n, nd));
    o = no;
    if (want) {
        d = w;
        bd = nd;
        shadow = true;
    } else {
        d = nd;
    }
    return false;
}

template <class Rays, bool kLdsScene, bool kLdsStack, bool kMis>
__device__ __forceinline__ void nee_body(const TraceArgs& A, const PathArgs& P, const NeeArgs& N) {
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
    int* __restrict__ stk = kLdsStack ? reinterpret_cast<int*>(lds4 + scene4) : P.gstack + (size_t)blockIdx.x * P.rows * kBlock;

    bool alive = true;     // the pool may still hold items for this lane
    bool active = false;   // the lane has an item in flight
    bool shadow = false;   // its next walk is the pending shadow segment of its last vertex
    bool sampled = false;  // that vertex drew a light
    uint32_t item = 0;
    Lcg g{0};
    v3 o{0, 0, 0}, d{0, 0, 1};
    v3 T{1, 1, 1}, L{0, 0, 0};
    v3 bd{0, 0, 1}, C{0, 0, 0};  // while a shadow segment is pending: the bounce direction, the light's term
    int lj = -1;                 // and the light's triangle (the caller's index)
    int k = 0;                   // segments of the path walked so far
    unsigned long long n_rays = 0, n_shadow = 0, n_draws = 0;  // this wave's (wave-uniform)
    Pool pool = pool_start(A);

    while (true) {
        const bool need = alive && !active;
        if (__any(need)) {
            claim_item(A, lane, need, pool, alive, item);
            if (need && alive) {  // item < total_items = m * spp
                const uint32_t sm = fdiv(item, A.div_npix), i = item - sm * P.m;
                Rays::load(A, P, i, sm, g, o, d);
                k = 0;
                T = v3{1.0f, 1.0f, 1.0f};
                L = v3{0.0f, 0.0f, 0.0f};
                sampled = false;
                shadow = false;
                active = true;
            }
        }
        if (!__any(active)) break;

        // ---- BVH::intersect (bvh.h:156-183) of the path segment or the shadow segment
        float t = 0.0f;
        int hit = -1;
        n_rays += (unsigned long long)__popcll(__ballot(active));
        n_shadow += (unsigned long long)__popcll(__ballot(active && shadow));
        const v3 inv = rcp3_exact(d, active);  // bvh.h:157
        const bool fast = !P.force_exact && __all(!active || query_ray_bounded(o, inv));
        if (active)
            hit = fast ? intersect_tree<true>(nodes, tris, stk, tid, o, d, inv, t)
                       : intersect_tree<false>(nodes, tris, stk, tid, o, d, inv, t);
        bool end = false, drew = false;
        if (active) {
            if (shadow) {
                // visible exactly when the closest hit is the light's own triangle
                if (hit >= 0 && N.rank_tri[hit] == lj) L = add(L, C);
                d = bd;
                shadow = false;
            } else {
                end = shade_nee<kMis>(A, N, mats, tris, hit, t, g, o, d, k, T, L, sampled, shadow, bd, C, lj, drew);
            }
        }
        n_draws += (unsigned long long)__popcll(__ballot(drew));
        if (end) {
            *reinterpret_cast<float3*>(A.radiance + 3 * (size_t)item) = make_float3(L.x, L.y, L.z);  // slab_at's layout
            active = false;
        }
    }
    count_rays_wave(A, lane, n_rays);
    if (lane == 0) {
        if (n_shadow) atomicAdd(N.nctr, n_shadow);
        if (n_draws) atomicAdd(N.nctr + 1, n_draws);
    }
}

template <bool kLdsScene, bool kLdsStack>
__global__ __launch_bounds__(kBlock) void pt_nee_kernel(TraceArgs A, PathArgs P, NeeArgs N) {
    nee_body<BufferRays, kLdsScene, kLdsStack, false>(A, P, N);
}

template <bool kLdsScene, bool kLdsStack>
__global__ __launch_bounds__(kBlock) void pt_nee_cam_kernel(TraceArgs A, PathArgs P, NeeArgs N) {
    nee_body<PartRays, kLdsScene, kLdsStack, false>(A, P, N);
}

template <bool kLdsScene, bool kLdsStack>
__global__ __launch_bounds__(kBlock) void pt_nee_mis_kernel(TraceArgs A, PathArgs P, NeeArgs N) {
    nee_body<BufferRays, kLdsScene, kLdsStack, true>(A, P, N);
}

template <bool kLdsScene, bool kLdsStack>
__global__ __launch_bounds__(kBlock) void pt_nee_mis_cam_kernel(TraceArgs A, PathArgs P, NeeArgs N) {
    nee_body<PartRays, kLdsScene, kLdsStack, true>(A, P, N);
}

namespace {

using NeeKernel = void (*)(TraceArgs, PathArgs, NeeArgs);

NeeKernel nee_kernel(bool camera, bool lds_scene, bool lds_stack, int mis) {
    if (mis == PT_NEE_MIS_BALANCE) {
        if (camera)
            return lds_scene ? (lds_stack ? pt_nee_mis_cam_kernel<true, true> : pt_nee_mis_cam_kernel<true, false>)
                             : (lds_stack ? pt_nee_mis_cam_kernel<false, true> : pt_nee_mis_cam_kernel<false, false>);
        return lds_scene ? (lds_stack ? pt_nee_mis_kernel<true, true> : pt_nee_mis_kernel<true, false>)
                         : (lds_stack ? pt_nee_mis_kernel<false, true> : pt_nee_mis_kernel<false, false>);
    }
    if (camera)
        return lds_scene ? (lds_stack ? pt_nee_cam_kernel<true, true> : pt_nee_cam_kernel<true, false>)
                         : (lds_stack ? pt_nee_cam_kernel<false, true> : pt_nee_cam_kernel<false, false>);
    return lds_scene ? (lds_stack ? pt_nee_kernel<true, true> : pt_nee_kernel<true, false>)
                     : (lds_stack ? pt_nee_kernel<false, true> : pt_nee_kernel<false, false>);
}

}  // namespace

// Placement and grid by the binary walk's shared rules (pt_launch.h), as paths_plan with no
// record rows: the stack rows, then nodes, triangles and materials (5 float4 per triangle).
int nee_plan(bool camera, int mis, const QueryScene& sc, size_t lds_usable, int num_cus, int64_t items, WalkPlan& plan) {
    place_walk_hooked(sc.num_nodes, sc.num_tris, sc.tree_depth, 5, 0, lds_usable, true, plan);
    return walk_grid((const void*)nee_kernel(camera, plan.lds_scene, plan.lds_stack, mis), lds_usable, num_cus, items, plan,
                     camera ? "light-sampling render" : "light-sampling trace");
}

int nee_launch(void* stream, const QueryScene& sc, const WalkPlan& plan, const PathsLaunch& l, const NeeLights& lights,
               int mis, int32_t s_begin, const pt_camera* cam, const pt_params* prm, const PartShape* shape) {
    const unsigned long long total = (unsigned long long)l.m * (unsigned long long)l.spp;
    if (l.m <= 0 || l.spp <= 0 || l.depth <= 0 || total >= (1ull << 31) || s_begin < 0 || (cam && (!prm || !shape)) ||
        (mis != PT_NEE_MIS_NONE && mis != PT_NEE_MIS_BALANCE) ||
        (cam && l.m != shape->npix) || (lights.count > 0 && (!lights.cdf || !lights.tri || !lights.geom || !lights.listed)))
        return set_error(PT_E_ARG, "light-sampling launch of %d rays x %d samples from %d, depth %d", l.m, l.spp, s_begin,
                         l.depth);
    const int grid = (int)std::min<unsigned long long>((unsigned long long)plan.grid, (total + kBlock - 1) / kBlock);
    TraceArgs A;
    PathArgs P;
    paths_args(sc, plan, l, grid, A, P);
    if (cam) {
        // the fields camera_ray and part_row read, as adaptive_launch fills them: the items stay
        // numbered over the part's m = npix pixels
        fill_camera(A, cam, *shape, prm);
        A.npix = l.m;
        A.div_npix = make_fastdiv((uint32_t)l.m);
        A.s_begin = s_begin;
    }
    NeeArgs N{};
    N.cdf = lights.cdf;
    N.ltri = lights.tri;
    N.lgeom = reinterpret_cast<const float4*>(lights.geom);
    N.listed = lights.listed;
    N.rank_tri = sc.rank_tri;
    N.nctr = l.ctr + 4;
    N.nlights = lights.count;
    N.area = lights.area;
    N.kA = lights.kA;
    hipLaunchKernelGGL(nee_kernel(cam != nullptr, plan.lds_scene, plan.lds_stack, mis), dim3(grid), dim3(kBlock), plan.lds_bytes,
                       (hipStream_t)stream, A, P, N);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PT_E_HIP, "light-sampling launch failed: %s", hipGetErrorString(e));
    return PT_OK;
}

}  // namespace pt
