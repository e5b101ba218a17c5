// pt_nee_grad.hip — material gradients of the light-sampling estimator along a caller's rays, over
// the binary child-pair walk (gfx950). DESIGN.md §3.26; the definition is in include/pt_hip.h
// ("material gradients of the light-sampling estimator"), the arithmetic in pt_nee.h.
//
//   pt_nee_grad_kernel<kLdsScene, kLdsStack, kLdsRec, kLdsTab>  pt_nee_kernel's loop (one item per
//       lane, ONE closest-hit walk per iteration: the next path segment, or the shadow segment put
//       in front of the bounce the vertex held back), with a record per bounce. A path that ends
//       stores its forward L (pt_nee_kernel's bits), and then runs the throughput pass Tw in
//       ascending k, adding the terms; R_{k+1} of bounce k is unwound again from the records for
//       every k (the records hold four words a level, R three: pt_grad.hip's deep-path form, here
//       at every depth — at depth 5 that is at most 6 more suffix steps a path, against its walks).
//   pt_nee_grad_cam_kernel<...>  the same loop fed from the part's own camera rays (PartRays,
//       pt_paths.h): the render gradients of DESIGN.md §3.29, grad_rgb indexed by the part-local pixel
//   pt_nee_grad_lights_kernel  the per-call emission of every light: its override row, or the table's
//
// The weights are a runtime choice (NeeGradArgs::mis, uniform): the two estimators share every
// kernel, so there are 16 instantiations per ray source and not 32. The walk, the samplers and the light choice are
// the forward estimator's, untouched: they depend on geometry, roughness and the LCG only. The
// fields of NeeGradArgs are re-read from the kernarg segment where they are used (ng_args): held in
// SGPRs across the walk they spilled (31-42 SGPRs, and a private segment in half the kernels).
//
// Records: four words per level and lane — the packed triangle, the cosine, the light's index in
// the table (-1 until its shadow segment found it visible) and g (g wl with the weights) — as
// [4][levels][kBlock] words in LDS (kLdsRec) or in the block's part of the global buffer.
// Gradient table, its LDS form and the +-0 rule: pt_grad.hip's. Rows are the caller's triangles,
// so a light that sits in two leaves gets one sum.
//
// LDS: [nodes, tris, mats (kLdsScene)] [stack (kLdsStack)] [records (kLdsRec)], then the table
// (kLdsTab) at NeeGradArgs::tab_off.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <string.h>

#include <algorithm>

#include "pt_nee.h"
#include "pt_nee_grad.h"
#include "pt_paths.h"

namespace pt {

static_assert(kSpecularIterBound == kMaxSpecularIters, "host and device bound of the specular rejection loop");

// The light table on the device, the call's counters and the gradient side of the launch.
struct NeeGradArgs {
    const float* __restrict__ cdf;          // per light: running area sum
    const int32_t* __restrict__ ltri;       // per light: the caller's triangle index
    const float4* __restrict__ lgeom;       // per light: kNeeLightF4 rows (the emission row is NOT read here)
    const float4* __restrict__ lemit;       // per light: the emission to evaluate at
    const uint8_t* __restrict__ listed;     // per caller triangle: 1 when it is a light
    const int32_t* __restrict__ rank_tri;   // rank position -> the caller's triangle index
    unsigned long long* __restrict__ nctr;  // [0] shadow segments, [1] light draws
    const float* __restrict__ grad_rgb;     // m x 3, or nullptr: forward only
    double* table;                          // [rows][6], global
    int nlights;
    float area, kA;
    int mis;                                // PT_NEE_MIS_*
    int levels;                             // record levels per lane
    int table_rows;
    uint32_t tab_off;                       // kLdsTab: byte offset of the block's table in LDS
    float spp_f;                            // (float)spp of the call (a render's launches are cut over samples)
    int want_rgb, want_color, want_emit;
};

// The kernel's third argument where the launch put it (the kernarg segment lays the three structs
// out as a struct of them), re-read at every use as kernarg_args() is: the fields only a path's end
// needs then cost a scalar load there and no SGPR across the walk.
struct NeeGradKernargs {
    TraceArgs A;
    PathArgs P;
    NeeGradArgs N;
};
static_assert(alignof(TraceArgs) == 8 && alignof(PathArgs) == 8 && alignof(NeeGradArgs) == 8 &&
                  offsetof(NeeGradKernargs, N) == sizeof(TraceArgs) + sizeof(PathArgs),
              "the kernarg segment's layout of (TraceArgs, PathArgs, NeeGradArgs)");
__device__ __forceinline__ const __attribute__((address_space(4))) NeeGradArgs* ng_args() {
    const __attribute__((address_space(4))) char* K =
        (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(K));
    return (const __attribute__((address_space(4))) NeeGradArgs*)(K + offsetof(NeeGradKernargs, N));
}

__device__ __forceinline__ v3 ng_xyz(float4 a) { return v3{a.x, a.y, a.z}; }
__device__ __forceinline__ v3 ng_yzw(float4 a) { return v3{a.y, a.z, a.w}; }

// pt_grad.hip's adds: the hardware add of the table's address space; +-0 leaves every sum as it is.
__device__ __forceinline__ void ng_add(double* __restrict__ tab, int at, float v) {
    if (v == 0.0f) return;
    unsafeAtomicAdd(tab + at, (double)v);
}
__device__ __forceinline__ void ng_add3(double* __restrict__ tab, int row, int part, v3 t) {
    const int at = 6 * row + 3 * part;
    ng_add(tab, at, t.x);
    ng_add(tab, at + 1, t.y);
    ng_add(tab, at + 2, t.z);
}

// A lane's records: word q of level j of `rec` = the block's [4][levels][kBlock] words + tid.
__device__ __forceinline__ int& rec_at(int* __restrict__ rec, int levels, int q, int j) {
    return rec[(q * levels + j) * kBlock];
}
#define REC_TRI(j) rec_at(rec, levels, 0, j)
#define REC_COS(j) __int_as_float(rec_at(rec, levels, 1, j))
#define REC_LIGHT(j) rec_at(rec, levels, 2, j)
#define REC_G(j) __int_as_float(rec_at(rec, levels, 3, j))

// shade_nee (pt_nee.hip) with the weights chosen at run time and a record per bounce: steps 2-6 of
// the definition for segment k + 1 of the path, after its BVH::intersect. Returns true when the
// path ends here, with its terminal in (end_kind, end_m); `hit` is then the terminal's triangle.
// Otherwise level k - 1 of the records holds the bounce (its light word -1: the shadow segment
// sets it), and the lane's next walk is as shade_nee leaves it, with the light's INDEX in lj.
__device__ __forceinline__ bool shade_nee_rec(const TraceArgs& A, const float4* __restrict__ mats,
                                              const float4* __restrict__ tris, int* __restrict__ rec, int levels, int hit,
                                              float t, Lcg& g, v3& o, v3& d, int& k, v3& T, v3& L, bool& sampled, bool& shadow,
                                              v3& bd, v3& C, int& lj, bool& drew, int& end_kind, float& end_m) {
    const auto* N = ng_args();  // re-read where used: nothing of it is held across the walk
    const bool mis = N->mis == PT_NEE_MIS_BALANCE;
    k++;
    end_kind = kNeeEndNone;
    end_m = 1.0f;
    if (hit < 0) return true;
    const float4 m0 = mats[2 * hit], m1 = mats[2 * hit + 1];
    const int type = __float_as_int(m0.x);
    const v3 emit{m1.x, m1.y, m1.z};
    if (type == PT_MAT_EMIT) {
        bool add_it = true;
        if (sampled) add_it = N->listed[N->rank_tri[hit]] == 0;
        if (add_it) {
            L = nee_add_emit(L, T, emit);
            end_kind = kNeeEndPlain;
        } else if (mis) {  // the BRDF sample reached a light: its share of the two techniques
            const float4 th = tris[3 * hit + 2];
            end_m = nee_brdf_weight(v3{th.y, th.z, th.w}, d, t, N->kA);
            L = nee_add_emit_weighted(L, T, emit, end_m);
            end_kind = kNeeEndWeighted;
        }
        return true;
    }
    L = nee_add_emit(L, T, emit);
    if (k >= A.depth) {  // no light draw at k == depth, and the last BRDF draw is not made
        end_kind = kNeeEndPlain;
        return true;
    }
    const v3 color{m0.y, m0.z, m0.w};
    const float4 tn = tris[3 * hit + 2];
    v3 n{tn.y, tn.z, tn.w};
    if (!(dot(n, d) < 0.0f)) n = neg(n);  // triangle.h:48
    const v3 hp = add(o, scale(d, t));
    const v3 no = add(hp, scale(n, 1e-4f));  // SHIFT_BIAS, render.h:16, 52
    const bool draw = type != PT_MAT_SPECULAR && N->nlights > 0;
    bool want = false;
    v3 w{0.0f, 0.0f, 0.0f};
    float gw = 0.0f;
    if (draw) {
        const float x1 = g.next01();
        const float x2 = g.next01();
        const float x3 = g.next01();
        const int j = nee_pick(N->cdf, N->nlights, x1 * N->area);
        const float4* __restrict__ G = N->lgeom + (size_t)kNeeLightF4 * j;
        const v3 y = nee_point(ng_xyz(G[0]), ng_xyz(G[1]), ng_xyz(G[2]), x2, x3);
        if (mis ? nee_connect_mis(y, no, n, ng_xyz(G[3]), N->kA, w, gw) : nee_connect(y, no, n, ng_xyz(G[3]), N->kA, w, gw)) {
            want = true;
            C = nee_direct(T, color, ng_xyz(N->lemit[j]), gw);
            lj = j;
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
    const float c = dot(n, nd);
    rec_at(rec, levels, 0, k - 1) = hit;  // k - 1 <= depth - 2 < levels
    rec_at(rec, levels, 1, k - 1) = __float_as_int(c);
    rec_at(rec, levels, 2, k - 1) = -1;
    rec_at(rec, levels, 3, k - 1) = __float_as_int(gw);
    T = nee_throughput(T, color, c);
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

// The end of a path of K bounces with the terminal (end_kind, end_m) on packed triangle `hit`:
// the throughput pass in ascending k, with R_{k+1} unwound from the records for every k. `tab`:
// the block's LDS table (kLdsTab), else the global one is used. Returns the terms it counted.
template <bool kLdsTab>
__device__ __forceinline__ uint32_t nee_grad_finish(const float4* __restrict__ mats, int* __restrict__ rec, int levels,
                                                    double* __restrict__ lds_tab, int K, int hit, int end_kind, float end_m,
                                                    uint32_t ray) {
    const auto* N = ng_args();
    double* __restrict__ tab = kLdsTab ? lds_tab : N->table;
    const float* __restrict__ gr = N->grad_rgb + 3 * (size_t)ray;
    const float fs = N->spp_f;
    v3 Tw{gr[0] / fs, gr[1] / fs, gr[2] / fs};
    const bool want_color = N->want_color != 0, want_emit = N->want_emit != 0;
    uint32_t terms = 0;
    for (int j = 0; j < K; j++) {
        const int t = REC_TRI(j);
        const float c = REC_COS(j);
        const int row = N->rank_tri[t];
        if (want_color) {  // the colour term first (the registers of its unwinding are free again
                           // before the adds); it is ADDED in its place below
            v3 R{0.0f, 0.0f, 0.0f};
            if (end_kind != kNeeEndNone) R = nee_end_value(end_kind, ng_xyz(mats[2 * hit + 1]), end_m);
            for (int i = K - 1; i > j; i--) {
                const int ti = REC_TRI(i);
                const int li = REC_LIGHT(i);
                const bool lit = li >= 0;
                R = nee_suffix(ng_xyz(mats[2 * ti + 1]), ng_yzw(mats[2 * ti]), REC_COS(i), R, lit,
                               lit ? ng_xyz(N->lemit[li]) : v3{0.0f, 0.0f, 0.0f}, REC_G(i));
            }
            const v3 term = nee_throughput(Tw, R, c);
            const v3 color = ng_yzw(mats[2 * t]);
            const int lj = REC_LIGHT(j);
            if (want_emit) {
                ng_add3(tab, row, 1, Tw);
                terms++;
            }
            if (lj >= 0) {
                const float gj = REC_G(j);
                if (want_emit) {
                    ng_add3(tab, N->ltri[lj], 1, nee_pair(Tw, color, gj));
                    terms++;
                }
                ng_add3(tab, row, 0, nee_pair(Tw, ng_xyz(N->lemit[lj]), gj));
                terms++;
            }
            ng_add3(tab, row, 0, term);
            terms++;
            Tw = nee_throughput(Tw, color, c);
        } else {  // d emit alone
            const v3 color = ng_yzw(mats[2 * t]);
            const int lj = REC_LIGHT(j);
            ng_add3(tab, row, 1, Tw);
            terms++;
            if (lj >= 0) {
                ng_add3(tab, N->ltri[lj], 1, nee_pair(Tw, color, REC_G(j)));
                terms++;
            }
            Tw = nee_throughput(Tw, color, c);
        }
    }
    if (end_kind != kNeeEndNone && want_emit) {
        ng_add3(tab, N->rank_tri[hit], 1, nee_end_term(end_kind, Tw, end_m));
        terms++;
    }
    return terms;
}

// __launch_bounds__'s second argument (waves per SIMD): left to itself the register allocator stops
// at 83-87 VGPRs, 5 waves; asked for 6 it fits 78-79 with no spill (make resource-usage-nee-grad).
template <class Rays, bool kLdsScene, bool kLdsStack, bool kLdsRec, bool kLdsTab>
__device__ __forceinline__ void nee_grad_body(const TraceArgs& A, const PathArgs& P, const NeeGradArgs& N) {
    extern __shared__ float4 lds4[];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const float4* __restrict__ nodes = A.nodes;
    const float4* __restrict__ tris = A.tris;
    const float4* __restrict__ mats = A.mats;
    const int scene4 = kLdsScene ? A.num_node4 + A.num_tri4 + A.num_mat4 : 0;
    double* tab = nullptr;
    if (kLdsTab) {
        tab = reinterpret_cast<double*>(reinterpret_cast<char*>(lds4) + N.tab_off);
        for (int i = tid; i < 6 * N.table_rows; i += kBlock) tab[i] = 0.0;
    }
    if (kLdsScene) {
        float4* s_nodes = lds4;
        float4* s_tris = lds4 + A.num_node4;
        float4* s_mats = s_tris + A.num_tri4;
        for (int i = tid; i < A.num_node4; i += kBlock) s_nodes[i] = A.nodes[i];
        for (int i = tid; i < A.num_tri4; i += kBlock) s_tris[i] = A.tris[i];
        for (int i = tid; i < A.num_mat4; i += kBlock) s_mats[i] = A.mats[i];
        nodes = s_nodes;
        tris = s_tris;
        mats = s_mats;
    }
    if (kLdsScene || kLdsTab) __syncthreads();
    int* const lds_stk = reinterpret_cast<int*>(lds4 + scene4);
    int* const lds_rec = lds_stk + (kLdsStack ? P.rows * kBlock : 0);
    int* __restrict__ stk = kLdsStack ? lds_stk : P.gstack + (size_t)blockIdx.x * P.rows * kBlock;
    const int levels = N.levels;
    int* __restrict__ rec = (kLdsRec ? lds_rec : P.grec_tri + (size_t)blockIdx.x * 4 * levels * kBlock) + tid;
    const bool grads = N.grad_rgb != nullptr && (N.want_color || N.want_emit);

    bool alive = true;     // the pool may still hold items for this lane
    bool active = false;   // the lane has an item in flight
    bool shadow = false;   // its next walk is the pending shadow segment of its last vertex
    bool sampled = false;  // that vertex drew a light
    uint32_t item = 0;
    Lcg g{0};
    v3 o{0, 0, 0}, d{0, 0, 1};
    v3 T{1, 1, 1}, L{0, 0, 0};
    v3 bd{0, 0, 1}, C{0, 0, 0};  // while a shadow segment is pending: the bounce direction, the light's term
    int lj = -1;                 // and the light's index in the table
    int k = 0;                   // segments of the path walked so far
    unsigned long long n_rays = 0, n_shadow = 0, n_draws = 0;  // this wave's (wave-uniform)
    uint32_t n_terms = 0;                                      // this lane's terms
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
        int end_kind = kNeeEndNone;
        float end_m = 1.0f;
        if (active) {
            if (shadow) {
                // visible exactly when the closest hit is the light's own triangle
                if (hit >= 0 && ng_args()->rank_tri[hit] == ng_args()->ltri[lj]) {
                    L = add(L, C);
                    rec_at(rec, levels, 2, k - 1) = lj;
                }
                d = bd;
                shadow = false;
            } else {
                end = shade_nee_rec(A, mats, tris, rec, levels, hit, t, g, o, d, k, T, L, sampled, shadow, bd, C, lj, drew,
                                    end_kind, end_m);
            }
        }
        n_draws += (unsigned long long)__popcll(__ballot(drew));
        if (end) {
            if (ng_args()->want_rgb)
                *reinterpret_cast<float3*>(A.radiance + 3 * (size_t)item) = make_float3(L.x, L.y, L.z);  // slab_at's layout
            if (grads) {
                const uint32_t sm = fdiv(item, A.div_npix);
                n_terms += nee_grad_finish<kLdsTab>(mats, rec, levels, tab, k - 1, hit, end_kind, end_m, item - sm * P.m);
            }
            active = false;
        }
    }
    count_rays_wave(A, lane, n_rays);
    if (lane == 0) {
        if (n_shadow) atomicAdd(N.nctr, n_shadow);
        if (n_draws) atomicAdd(N.nctr + 1, n_draws);
    }
    {  // the terms: wave reduction, one atomic per wave
        unsigned long long r = n_terms;
        for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off);
        if (lane == 0 && r) atomicAdd(A.ctr + 2, r);
    }
    if (kLdsTab) {
        __syncthreads();
        for (int i = tid; i < 6 * N.table_rows; i += kBlock) {
            const double v = tab[i];
            if (!(v == 0.0)) unsafeAtomicAdd(N.table + i, v);  // a NaN goes through
        }
    }
}

template <bool kLdsScene, bool kLdsStack, bool kLdsRec, bool kLdsTab>
__global__ __launch_bounds__(kBlock, 6) void pt_nee_grad_kernel(TraceArgs A, PathArgs P, NeeGradArgs N) {
    nee_grad_body<BufferRays, kLdsScene, kLdsStack, kLdsRec, kLdsTab>(A, P, N);
}

// The part's own camera rays: item (pixel i, sample A.s_begin + sm), grad_rgb by the part-local pixel.
template <bool kLdsScene, bool kLdsStack, bool kLdsRec, bool kLdsTab>
__global__ __launch_bounds__(kBlock, 6) void pt_nee_grad_cam_kernel(TraceArgs A, PathArgs P, NeeGradArgs N) {
    nee_grad_body<PartRays, kLdsScene, kLdsStack, kLdsRec, kLdsTab>(A, P, N);
}

// out[j] = the emission light j is evaluated at
__global__ __launch_bounds__(kBlock) void pt_nee_grad_lights_kernel(const float4* __restrict__ lgeom,
                                                                    const int32_t* __restrict__ ltri,
                                                                    const float* __restrict__ emit, float4* __restrict__ out,
                                                                    int nlights) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= nlights) return;
    float4 e = lgeom[(size_t)kNeeLightF4 * j + 4];
    if (emit) {
        const size_t t = (size_t)ltri[j];
        e = make_float4(emit[3 * t], emit[3 * t + 1], emit[3 * t + 2], 0.0f);
    }
    out[j] = e;
}

namespace {

using NeeGradKernel = void (*)(TraceArgs, PathArgs, NeeGradArgs);

template <bool kLdsScene, bool kLdsStack>
NeeGradKernel nee_grad_kernel_t(bool lds_rec, bool lds_tab) {
    return lds_rec ? (lds_tab ? pt_nee_grad_kernel<kLdsScene, kLdsStack, true, true>
                              : pt_nee_grad_kernel<kLdsScene, kLdsStack, true, false>)
                   : (lds_tab ? pt_nee_grad_kernel<kLdsScene, kLdsStack, false, true>
                              : pt_nee_grad_kernel<kLdsScene, kLdsStack, false, false>);
}
template <bool kLdsScene, bool kLdsStack>
NeeGradKernel nee_grad_cam_kernel_t(bool lds_rec, bool lds_tab) {
    return lds_rec ? (lds_tab ? pt_nee_grad_cam_kernel<kLdsScene, kLdsStack, true, true>
                              : pt_nee_grad_cam_kernel<kLdsScene, kLdsStack, true, false>)
                   : (lds_tab ? pt_nee_grad_cam_kernel<kLdsScene, kLdsStack, false, true>
                              : pt_nee_grad_cam_kernel<kLdsScene, kLdsStack, false, false>);
}
NeeGradKernel nee_grad_kernel(const NeeGradPlan& p) {
    const bool r = p.walk.lds_rec, t = p.lds_tab;
    if (p.camera)
        return p.walk.lds_scene
                   ? (p.walk.lds_stack ? nee_grad_cam_kernel_t<true, true>(r, t) : nee_grad_cam_kernel_t<true, false>(r, t))
                   : (p.walk.lds_stack ? nee_grad_cam_kernel_t<false, true>(r, t) : nee_grad_cam_kernel_t<false, false>(r, t));
    return p.walk.lds_scene ? (p.walk.lds_stack ? nee_grad_kernel_t<true, true>(r, t) : nee_grad_kernel_t<true, false>(r, t))
                            : (p.walk.lds_stack ? nee_grad_kernel_t<false, true>(r, t) : nee_grad_kernel_t<false, false>(r, t));
}

}  // namespace

// nee_plan's placement with 2 x (depth - 1) of place_walk's two-word record rows (four words a
// level), then the table while it fits the same cap beside them (grad_place's rule).
int nee_grad_plan(const QueryScene& sc, int table_rows, size_t lds_usable, int num_cus, int depth, int64_t items,
                  NeeGradPlan& plan, bool camera) {
    plan.levels = std::max(0, depth - 1);
    plan.camera = camera ? 1 : 0;
    place_walk_hooked(sc.num_nodes, sc.num_tris, sc.tree_depth, 5, 2 * plan.levels, lds_usable, true, plan.walk);
    const size_t cap = std::min<size_t>(64 * 1024, lds_usable / 2);
    const size_t off = (plan.walk.lds_bytes + 15) / 16 * 16;
    const size_t tab_b = 6 * sizeof(double) * (size_t)table_rows;
    plan.lds_tab = !hook_off("PT_GRAD_LDS") && table_rows > 0 && lds_round(off + tab_b) <= cap;
    plan.tab_off = plan.lds_tab ? off : 0;
    if (plan.lds_tab) plan.walk.lds_bytes = off + tab_b;
    return walk_grid((const void*)nee_grad_kernel(plan), lds_usable, num_cus, items, plan.walk,
                     camera ? "render_nee_grad" : "trace_nee_grad");
}

int nee_grad_launch(void* stream, const QueryScene& sc, const NeeGradPlan& plan, const NeeGradLaunch& gl,
                    const NeeLights& lights) {
    const PathsLaunch& l = gl.p;
    const WalkPlan& wp = plan.walk;
    const unsigned long long total = (unsigned long long)l.m * (unsigned long long)l.spp;
    if (l.m <= 0 || l.spp <= 0 || l.depth <= 0 || total >= (1ull << 31) || l.depth - 1 > plan.levels ||
        (gl.mis != PT_NEE_MIS_NONE && gl.mis != PT_NEE_MIS_BALANCE) ||
        (lights.count > 0 && (!lights.cdf || !lights.tri || !lights.geom || !lights.listed || !gl.lemit)))
        return set_error(PT_E_ARG, "trace_nee_grad launch of %d rays x %d samples, depth %d", l.m, l.spp, l.depth);
    if (gl.table_rows <= 0 || !gl.table || !gl.mats) return set_error(PT_E_ARG, "trace_nee_grad launch without a table");
    if (!wp.lds_rec && plan.levels > 0 && !l.grec) return set_error(PT_E_ARG, "trace_nee_grad launch without a record buffer");
    if ((plan.camera != 0) != (gl.cam != nullptr) ||
        (gl.cam && (!gl.prm || !gl.shape || l.m != gl.shape->npix || gl.s_begin < 0 || gl.spp_total < l.spp)))
        return set_error(PT_E_ARG, "render_nee_grad launch of %d pixels x %d samples from %d", l.m, l.spp, gl.s_begin);
    const int grid = (int)std::min<unsigned long long>((unsigned long long)wp.grid, (total + kBlock - 1) / kBlock);
    TraceArgs A;
    PathArgs P;
    paths_args(sc, wp, l, grid, A, P);
    A.mats = reinterpret_cast<const float4*>(gl.mats);
    A.dark = 0;
    A.acc_chunks = 0;  // no fused accumulation: ctr[2] counts the terms
    if (gl.cam) {
        // the fields camera_ray and part_row read, as nee_launch fills them: the items stay numbered
        // over the part's m = npix pixels
        fill_camera(A, gl.cam, *gl.shape, gl.prm);
        A.npix = l.m;
        A.div_npix = make_fastdiv((uint32_t)l.m);
        A.s_begin = gl.s_begin;
    }
    NeeGradArgs N{};
    N.cdf = lights.cdf;
    N.ltri = lights.tri;
    N.lgeom = reinterpret_cast<const float4*>(lights.geom);
    N.lemit = reinterpret_cast<const float4*>(gl.lemit);
    N.listed = lights.listed;
    N.rank_tri = sc.rank_tri;
    N.nctr = l.ctr + 4;
    N.grad_rgb = gl.grad_rgb;
    N.table = gl.table;
    N.nlights = lights.count;
    N.area = lights.area;
    N.kA = lights.kA;
    N.mis = gl.mis;
    N.levels = plan.levels;
    N.table_rows = gl.table_rows;
    N.tab_off = (uint32_t)plan.tab_off;
    N.spp_f = (float)(gl.cam ? gl.spp_total : l.spp);
    N.want_rgb = gl.want_rgb;
    N.want_color = gl.want_color;
    N.want_emit = gl.want_emit;
    hipLaunchKernelGGL(nee_grad_kernel(plan), dim3(grid), dim3(kBlock), wp.lds_bytes, (hipStream_t)stream, A, P, N);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PT_E_HIP, "trace_nee_grad launch failed: %s", hipGetErrorString(e));
    return PT_OK;
}

int nee_grad_gather_lights(void* stream, const NeeLights& lights, const float* emit, f4* out) {
    if (lights.count <= 0) return PT_OK;
    hipLaunchKernelGGL(pt_nee_grad_lights_kernel, dim3((lights.count + kBlock - 1) / kBlock), dim3(kBlock), 0,
                       (hipStream_t)stream, reinterpret_cast<const float4*>(lights.geom), lights.tri, emit,
                       reinterpret_cast<float4*>(out), lights.count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(PT_E_HIP, "trace_nee_grad light gather failed: %s", hipGetErrorString(e));
    return PT_OK;
}

#undef REC_TRI
#undef REC_COS
#undef REC_LIGHT
#undef REC_G

}  // namespace pt
