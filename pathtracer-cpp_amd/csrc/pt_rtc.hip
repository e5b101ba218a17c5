// pt_rtc.hip — the flat path's scene kernel (pt_rtc.h): the generator of its source, the hipRTC
// compile (in the compile server's process, or here), the process's and the on-disk code-object
// caches, and the load of a finished compile on a device. No kernel is defined here.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <errno.h>
#include <fcntl.h>
#include <link.h>
#include <signal.h>
#include <spawn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <fstream>
#include <future>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

extern char** environ;

#include "pt_hip_debug.h"
#include "pt_launch.h"
#include "pt_rtc.h"
#include "pt_sha256.h"
#include "pt_trace.h"

// Sources of pt_trace.h, pt_math.h, pt_raystack.h, pt_flatlds.h and pt_hip.h, embedded at build time
// (build/pt_rtc_blob.cpp).
extern "C" const char* pt_rtc_src_trace;
extern "C" const char* pt_rtc_src_math;
extern "C" const char* pt_rtc_src_stack;
extern "C" const char* pt_rtc_src_lds;
extern "C" const char* pt_rtc_src_hip;

namespace pt {

namespace {

std::string hexf(float v) {
    char b[64];
    snprintf(b, sizeof(b), "%af", (double)v);
    return b;
}

// hexf, and an infinity spelled so that it compiles (the empty emitter box).
std::string litf(float v) {
    if (v == std::numeric_limits<float>::infinity()) return "__builtin_inff()";
    if (v == -std::numeric_limits<float>::infinity()) return "-__builtin_inff()";
    return hexf(v);
}

}  // namespace

// Box-level pairs (PT_BOX_PAIRS, the hipRTC flat kernel): when every leaf holds one triangle
// (leaf k = triangle rank k) and no distinct leaf box bounds more than two leaves, the box
// mask carries one bit per DISTINCT box (Cornell: 20 for 32 leaves) and a pair (lane, box)
// tests the box's one or two triangles. Returns the number of distinct boxes in that case
// (the LDS table the kernel reads: one uint16 (rank0 | rank1 << 8, 0xff = none) per box),
// else 0. Box u is numbered by its first leaf, as in flat_mask_source.
// Off unless PT_BOX_PAIRS=1 (test hook): measured 2.2% slower on Cornell, 1.6% on modified
// Cornell r=0.3 and Cornell depth 8 (profiles/r05_ab/box_pairs) — the pair rounds' second
// triangle test and its divergence cost more than the 12 fewer mask bits save.
int flat_box_pairs(const std::vector<f4>& leaves, int n, std::vector<uint16_t>* tab) {
    const char* e = hook_env("PT_BOX_PAIRS");
    if (!e || *e != '1') return 0;
    std::map<std::vector<uint32_t>, int> box_id;
    std::vector<std::vector<int>> box_leaves;
    for (int k = 0; k < n; k++) {
        const f4 a = leaves[2 * k], b = leaves[2 * k + 1];
        if (__builtin_bit_cast(int, b.z) != k || __builtin_bit_cast(int, b.w) != k) return 0;  // not one triangle per leaf
        const std::vector<uint32_t> key = {f2u(a.x), f2u(a.y), f2u(a.z), f2u(a.w), f2u(b.x), f2u(b.y)};
        auto it = box_id.find(key);
        if (it == box_id.end()) {
            it = box_id.emplace(key, (int)box_leaves.size()).first;
            box_leaves.emplace_back();
        }
        box_leaves[it->second].push_back(k);
    }
    for (const auto& l : box_leaves)
        if (l.size() > 2 || l.back() > 254) return 0;
    if (tab) {
        tab->clear();
        for (const auto& l : box_leaves) tab->push_back((uint16_t)(l[0] | ((l.size() > 1 ? l[1] : 0xff) << 8)));
    }
    return (int)box_leaves.size();
}

// Whether leaf k of the flat list holds exactly triangle rank k (every BVH::build tree).
bool leaves_single(const std::vector<f4>& leaves, int n) {
    for (int k = 0; k < n; k++)
        if (__builtin_bit_cast(int, leaves[2 * k + 1].z) != k || __builtin_bit_cast(int, leaves[2 * k + 1].w) != k)
            return false;
    return true;
}

namespace {

// The flat path's leaf-box test for one scene as straight-line code: each distinct box
// plane (c - o) * inv is computed once, boxes shared by several leaves are tested once,
// and a flat axis (lb == rt) needs no min/max. Same IEEE operations as slab_hit_finite.
std::string flat_mask_source(const std::vector<f4>& leaves, int n, bool specular, bool tri_fast, bool albedo_x2,
                             bool dark, const EmitBox& emit, const RtcBaked& baked) {
    std::vector<std::map<uint32_t, int>> planes(3);
    auto plane = [&](int ax, float c) {
        auto it = planes[ax].find(f2u(c));
        if (it != planes[ax].end()) return it->second;
        const int id = (int)planes[ax].size();
        planes[ax][f2u(c)] = id;
        return id;
    };
    std::string body;
    std::map<std::vector<uint32_t>, int> box_id;
    std::vector<unsigned long long> box_bits;
    struct BoxExpr {
        std::string lo[3], hi[3];
    };
    std::vector<BoxExpr> boxes;
    for (int k = 0; k < n; k++) {
        const f4 a = leaves[2 * k], b = leaves[2 * k + 1];
        const float lb[3] = {a.x, a.y, a.z}, rt[3] = {a.w, b.x, b.y};
        std::vector<uint32_t> key = {f2u(lb[0]), f2u(lb[1]), f2u(lb[2]), f2u(rt[0]), f2u(rt[1]), f2u(rt[2])};
        auto it = box_id.find(key);
        if (it != box_id.end()) {
            box_bits[it->second] |= 1ull << k;
            continue;
        }
        const int id = (int)box_bits.size();
        box_id[key] = id;
        box_bits.push_back(1ull << k);
        BoxExpr e;
        const char ax_name[3] = {'x', 'y', 'z'};
        for (int ax = 0; ax < 3; ax++) {
            const std::string p1 = std::string("t") + ax_name[ax] + std::to_string(plane(ax, lb[ax]));
            const std::string p2 = std::string("t") + ax_name[ax] + std::to_string(plane(ax, rt[ax]));
            if (p1 == p2) {
                e.lo[ax] = e.hi[ax] = p1;
            } else {
                e.lo[ax] = "__builtin_fminf(" + p1 + ", " + p2 + ")";
                e.hi[ax] = "__builtin_fmaxf(" + p1 + ", " + p2 + ")";
            }
        }
        boxes.push_back(e);
    }
    // tmin = max(lo_x, lo_y, lo_z, 0): the clamp to 0 is applied to one axis term and that
    // clamped term is computed once for every box that shares it (PT_SHARED_CLAMP; the same
    // maximum: max is associative and commutative on non-NaN values, and which zero a tie
    // returns does not change the comparison), instead of one max(., 0) per box.
    std::map<std::string, int> lo_uses;
    for (const BoxExpr& e : boxes)
        for (int ax = 0; ax < 3; ax++) lo_uses[e.lo[ax]]++;
    std::map<std::string, std::string> clamp_name;
    std::string clamps, tests, tests_plain, tests_sign;
    for (size_t id = 0; id < boxes.size(); id++) {
        const BoxExpr& e = boxes[id];
        int cax = 0;
        for (int ax = 1; ax < 3; ax++)
            if (lo_uses[e.lo[ax]] > lo_uses[e.lo[cax]]) cax = ax;
        auto cn = clamp_name.find(e.lo[cax]);
        if (cn == clamp_name.end()) {
            const std::string nm = "c" + std::to_string(clamp_name.size());
            clamps += "        const float " + nm + " = __builtin_fmaxf(" + e.lo[cax] + ", 0.0f);\n";
            cn = clamp_name.emplace(e.lo[cax], nm).first;
        }
        const int a1 = cax == 0 ? 1 : 0, a2 = cax == 2 ? 1 : 2;
        const std::string tmax = "__builtin_fminf(__builtin_fminf(" + e.hi[0] + ", " + e.hi[1] + "), " + e.hi[2] + ")";
        tests += "        const bool b" + std::to_string(id) + " = __builtin_fmaxf(__builtin_fmaxf(" + e.lo[a1] + ", " +
                 e.lo[a2] + "), " + cn->second + ") <= " + tmax + ";\n";
        tests_plain += "        const bool b" + std::to_string(id) + " = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(" +
                       e.lo[0] + ", " + e.lo[1] + "), " + e.lo[2] + "), 0.0f) <= " + tmax + ";\n";
        // sign-bit form (PT_SIGN_MASK): tmax + 0 turns a -0 exit value (origin on a plane,
        // 1 / d < 0) into +0, which the comparison above treats as equal to 0
        tests_sign += "        const uint32_t f" + std::to_string(id) + " = box_fail_bits(__builtin_fmaxf(__builtin_fmaxf(" +
                      e.lo[0] + ", " + e.lo[1] + "), " + e.lo[2] + "), " + tmax + " + 0.0f);\n";
    }
    tests = "#if KSIGN\n" + tests_sign + "#elif PT_SHARED_CLAMP\n" + clamps + tests + "#else\n" + tests_plain + "#endif\n";
    const char ax_name[3] = {'x', 'y', 'z'};
    // Plane values two at a time (v_pk_add_f32 + v_pk_mul_f32: the same two IEEE
    // operations per value, half the instructions); PT_PK_PLANES=0 emits scalar code.
    body += "#if PT_PK_PLANES\n";
    for (int ax = 0; ax < 3; ax++) {
        const std::string comp(1, ax_name[ax]);
        std::vector<std::pair<uint32_t, int>> ps(planes[ax].begin(), planes[ax].end());
        if (ps.empty()) continue;
        body += "        const f2v o" + comp + "2 = {o." + comp + ", o." + comp + "}, i" + comp + "2 = {inv." + comp +
                ", inv." + comp + "};\n";
        for (size_t i = 0; i < ps.size(); i += 2) {
            const auto& a = ps[i];
            const auto& b = ps[i + 1 < ps.size() ? i + 1 : i];
            const std::string pv = "p" + comp + std::to_string(i);
            body += "        const f2v " + pv + " = (f2v{" + hexf(u2f(a.first)) + ", " + hexf(u2f(b.first)) + "} - o" +
                    comp + "2) * i" + comp + "2;\n";
            body += "        const float t" + comp + std::to_string(a.second) + " = " + pv + ".x;\n";
            if (i + 1 < ps.size()) body += "        const float t" + comp + std::to_string(b.second) + " = " + pv + ".y;\n";
        }
    }
    body += "#else\n";
    for (int ax = 0; ax < 3; ax++)
        for (const auto& kv : planes[ax]) {
            const std::string comp(1, ax_name[ax]);
            body += "        const float t" + comp + std::to_string(kv.second) + " = (" + hexf(u2f(kv.first)) +
                    " - o." + comp + ") * inv." + comp + ";\n";
        }
    body += "#endif\n";
    // Leaf bits shifted in from the top leaf down, m = 2m + b: one add-with-carry per
    // leaf with the box test's lane mask as the carry, no constants held in registers.
    // PT_MULTI_LEAF_OR: a box holding several leaves (the two triangles of a quad) sets all
    // their bits with one select + or after the chain, whose steps for those leaves are
    // plain doublings (v_add_u32, which dual-issues) instead of one carry add (main VALU
    // port only) per leaf.
    std::vector<int> leaf_box(n, -1);
    for (size_t i = 0; i < box_bits.size(); i++)
        for (int k = 0; k < n; k++)
            if (box_bits[i] >> k & 1) leaf_box[k] = (int)i;
    auto multi = [&](int k) { return __builtin_popcountll(box_bits[leaf_box[k]]) > 1; };
    std::string acc = "        uint32_t lo = 0, hi = 0;\n#if KSIGN\n";
    for (int k = n - 1; k >= 0; k--) {  // fail bits shifted in, then inverted
        const char* w = k >= 32 ? "hi" : "lo";
        acc += std::string("        ") + w + " = shl1_add_sign(" + w + ", f" + std::to_string(leaf_box[k]) + ");\n";
    }
    acc += "        lo = ~lo" + std::string(n < 32 ? " & " + std::to_string((1u << n) - 1u) + "u" : "") + ";\n";
    if (n > 32) acc += "        hi = ~hi" + std::string(n < 64 ? " & " + std::to_string((uint32_t)((1ull << (n - 32)) - 1u)) + "u" : "") + ";\n";
    acc += "#else\n";
    for (int k = n - 1; k >= 0; k--) {
        const char* w = k >= 32 ? "hi" : "lo";
        const std::string bit = std::string("#if PT_ADDC_MASK\n        ") + w + " = shl1_add_bit(" + w +
                                ", __builtin_amdgcn_ballot_w64(b" + std::to_string(leaf_box[k]) + "));\n#else\n        " + w +
                                " = " + w + " + " + w + " + (b" + std::to_string(leaf_box[k]) + " ? 1u : 0u);\n#endif\n";
        if (multi(k))
            acc += std::string("#if PT_MULTI_LEAF_OR\n        ") + w + " = dbl_u32(" + w + ");\n#else\n" + bit + "#endif\n";
        else
            acc += bit;
    }
    acc += "#if PT_MULTI_LEAF_OR\n";
    for (size_t i = 0; i < box_bits.size(); i++) {
        const unsigned long long m = box_bits[i];
        if (__builtin_popcountll(m) < 2) continue;
        const std::string bal = "__builtin_amdgcn_ballot_w64(b" + std::to_string(i) + ")";
        if ((uint32_t)m)
            acc += "        lo = or_if_bit(lo, " + std::to_string((uint32_t)m) + "u, " + bal + ");\n";
        if ((uint32_t)(m >> 32))
            acc += "        hi = or_if_bit(hi, " + std::to_string((uint32_t)(m >> 32)) + "u, " + bal + ");\n";
    }
    acc += "#endif\n";
    acc += "#endif\n";  // KSIGN
    // box-level pairs: one bit per distinct box, box u at bit u
    std::vector<uint16_t> box_tab;
    const int nbox = flat_box_pairs(leaves, n, &box_tab);
    if (nbox > 0) {
        std::string chain = "        lo = 0;\n        hi = 0;\n";
        for (int u = nbox - 1; u >= 0; u--) {
            const char* w = u >= 32 ? "hi" : "lo";
            chain += std::string("        ") + w + " = shl1_add_bit(" + w + ", __builtin_amdgcn_ballot_w64(b" +
                     std::to_string(u) + "));\n";
        }
        acc = "#if KBOX\n        uint32_t lo, hi;\n" + chain + "#else\n" + acc + "#endif\n";
    }
    acc += "        const unsigned long long m = ((unsigned long long)hi << 32) | lo;\n";
    const bool single = leaves_single(leaves, n);  // leaf k holds exactly triangle rank k
    // the sign-bit box bits need finite plane values: scene coordinates below 2^60 (tri_fast's
    // condition) with the kernel's ray bound (bounded_ray)
    const bool sign = tri_fast;
    std::string tabs = "{";
    for (size_t u = 0; u < box_tab.size(); u++) tabs += (u ? ", " : "") + std::to_string(box_tab[u]) + "u";
    tabs += box_tab.empty() ? "0u}" : "}";
    // the last-ray rule (shade): the emitter box as literals, so the kernel compares against
    // constants and holds no registers for it; off: the rule is not compiled in
    std::string rej = "    using EmitRej = NoEmitReject;\n";
    if (emit.on)
        rej = "    struct EmitRej {\n        static constexpr bool kCompiled = true;\n"
              "        __device__ __forceinline__ static bool on() { return true; }\n"
              "        __device__ __forceinline__ static bool rejected(v3 o, v3 d) {\n"
              "            return emit_reject(v3{" + litf(emit.lo[0]) + ", " + litf(emit.lo[1]) + ", " + litf(emit.lo[2]) +
              "}, v3{" + litf(emit.hi[0]) + ", " + litf(emit.hi[1]) + ", " + litf(emit.hi[2]) + "}, o, d);\n"
              "        }\n"
              // the slab rule, which the flat body runs with the inv it carries (shade_inv); under
              // PT_EMIT_SIGN_ONLY (test hook) the member above alone, and no carried inv
              "        static constexpr bool kSlab = !PT_EMIT_SIGN_ONLY;\n"
              "        __device__ __forceinline__ static bool rejected_slab(v3 o, v3, v3 inv) {\n"
              "            return emit_slab_reject(v3{" + litf(emit.lo[0]) + ", " + litf(emit.lo[1]) + ", " + litf(emit.lo[2]) +
              "}, v3{" + litf(emit.hi[0]) + ", " + litf(emit.hi[1]) + ", " + litf(emit.hi[2]) + "}, o, inv);\n"
              "        }\n"
              // the same with the inv half of the guard handed in (PT_DOMAIN_ONCE, shade_inv)
              "        __device__ __forceinline__ static bool rejected_slab_given(v3 o, v3, v3 inv, bool inv_ok) {\n"
              "            return emit_slab_reject_given(v3{" + litf(emit.lo[0]) + ", " + litf(emit.lo[1]) + ", " + litf(emit.lo[2]) +
              "}, v3{" + litf(emit.hi[0]) + ", " + litf(emit.hi[1]) + ", " + litf(emit.hi[2]) + "}, o, inv, inv_ok);\n"
              "        }\n    };\n";
    return std::string("#ifndef PT_FLAT_SIGN_MASK\n#define PT_FLAT_SIGN_MASK 0\n#endif\n#define KSIGN (PT_FLAT_SIGN_MASK && ") +
           (sign ? "1" : "0") + ")\n" + "#define KBOX " + (nbox > 0 ? "(!KSIGN)" : "0") + "\n" +
           "namespace pt {\nstruct SceneBoxMask {\n    static constexpr bool kSignMask = KSIGN;\n"
           "    static constexpr bool kBoxPairs = KBOX;\n    static constexpr bool kCamInvGen = PT_CAM_INV == 2;\n"
           "    static constexpr bool kRayStack = PT_RAY_STACK != 0;\n"
           "    static constexpr bool kDomOnce = PT_DOMAIN_ONCE != 0;\n"  // DomOnce, pt_trace.h
           "    static constexpr int kBoxes = " + std::to_string(nbox) +
           ";\n    static constexpr uint16_t kBoxTab[" + std::to_string(std::max<size_t>(1, box_tab.size())) + "] = " + tabs +
           ";\n    static constexpr bool kMask32 = " +
           (n <= 32 ? "true" : "false") + ";\n    static constexpr bool kSingleTri = " + (single ? "true" : "false") +
           ";\n    static constexpr bool kSpecular = " + (specular ? "true" : "false") +
           ";\n    static constexpr bool kTriFast = " + (tri_fast ? "true" : "false") +
           ";\n    static constexpr bool kAlbedoX2 = " + (albedo_x2 ? "true" : "false") +
           ";\n    static constexpr bool kDarkKnown = true;\n    static constexpr bool kDark = " + (dark ? "true" : "false") +
           // what pt_ctx_set_scene fixes (BakedConsts, pt_trace.h), under PT_KCONST
           ";\n    static constexpr bool kBaked = PT_KCONST != 0;\n    static constexpr int kNumTri4 = " +
           std::to_string(baked.num_tri4) + ", kNumMat4 = " + std::to_string(baked.num_mat4) +
           ", kBoxTabBytes = " + std::to_string(baked.box_tab_bytes) + ", kThetaLanes = " + std::to_string(baked.theta_lanes) +
           ";\n    static constexpr bool kPairs = " + (baked.pairs ? "true" : "false") +
           ";\n" + rej + "    __device__ __forceinline__ static unsigned long long "
           "mask(const TraceArgs&, v3 o, v3 inv) {\n" +
           body + tests + acc + "        return m;\n    }\n};\n}  // namespace pt\n";
}

struct RtcCache {
    std::mutex mu;
    std::map<std::string, RtcFuture> code;                        // source -> compile job
    std::map<std::pair<int, std::string>, hipFunction_t> funcs;   // (device, source) -> loaded kernel
    std::set<std::string> refused;  // disk keys whose code object the runtime refused: never read again
};
RtcCache& rtc_cache() {
    static RtcCache* c = new RtcCache();  // never destroyed: modules live for the process
    return *c;
}

// Waves per SIMD the scene kernel is register-allocated for: 8 (<= 64 VGPRs; with the
// AMDGPU pressure trackers below it needs 62-63 and no scratch, and 8 blocks of <= 20 KB
// fit the LDS): +2.4 % on Cornell, +2.2 % on config 3 against 7 (profiles/r04_sched).
int rtc_waves() {
    const int w = hook_int("PT_RTC_WAVES", 8);
    return (w >= 1 && w <= 8) ? w : 8;
}

// specular: the scene holds a SPECULAR material (else the sampler is compiled out).
// PT_RTC_DEFINES="NAME=VALUE,..." adds macros to the generated source (A/B experiments).
std::string rtc_defines() {
    const char* e = hook_env("PT_RTC_DEFINES");
    std::string out;
    if (!e) return out;
    std::stringstream ss(e);
    std::string item;
    while (std::getline(ss, item, ',')) {
        const size_t eq = item.find('=');
        if (!item.empty()) out += "#define " + (eq == std::string::npos ? item : item.substr(0, eq) + " " + item.substr(eq + 1)) + "\n";
    }
    return out;
}

// PT_RTC_FLAGS="-flag -flag ..." (or comma-separated) adds compiler options (A/B experiments; named in the
// generated source, so the per-process code cache keys on them).
std::vector<std::string> rtc_extra_flags() {
    std::vector<std::string> out;
    const char* e = hook_env("PT_RTC_FLAGS");
    if (!e) return out;
    std::string flags(e);
    std::replace(flags.begin(), flags.end(), ',', ' ');  // "-mllvm,-opt" in env lists that split on spaces
    std::stringstream ss(flags);
    std::string f;
    while (ss >> f) out.push_back(f);
    return out;
}

}  // namespace

// PT_KCONST (default 1; PT_RTC_DEFINES="PT_KCONST=0" is the A/B hook): whether the generated
// source holds RtcBaked's values as constants.
bool rtc_kconst_on() {
    const std::string d = rtc_defines(), key = "#define PT_KCONST ";
    const size_t at = d.rfind(key);  // the source tests PT_KCONST != 0: so does this
    return at == std::string::npos || strtol(d.c_str() + at + key.size(), nullptr, 0) != 0;
}

// theta_choice's lane bound before the table is asked for (pt_kernel.hip): PT_THETA_LANES (tuning
// hook) or 32 in scenes with a SPECULAR material, else 0; 0 in builds without the table.
int theta_lanes_wanted(bool specular) {
#if PT_THETA_TAB
    return hook_int("PT_THETA_LANES", specular ? 32 : 0);
#else
    (void)specular;
    return 0;
#endif
}

RtcBaked rtc_baked(int num_tris, bool specular, int flat_boxes) {
    RtcBaked k;
    k.on = rtc_kconst_on();
    k.num_tri4 = 3 * num_tris;
    k.num_mat4 = 2 * num_tris;
    k.box_tab_bytes = (int)flat_box_tab_bytes((unsigned)flat_boxes);
    k.pairs = !hook_off("PT_PAIRS");
    k.theta_lanes = theta_lanes_wanted(specular);
    return k;
}

std::string rtc_flat_source(const std::vector<f4>& leaves, int n, bool specular, bool tri_fast, bool albedo_x2,
                            bool dark, const EmitBox& emit, const RtcBaked& baked) {
    std::string fl = "// extra flags:";
    for (const std::string& f : rtc_extra_flags()) fl += " " + f;
    // camera fields from the kernel's argument registers at 8 waves: +0.5-1.0 % on configs
    // 2, 3, 5 against the kernarg-segment form the offline kernels keep (profiles/r04_switches).
    // threadIdx.x re-read at each use (fresh_tid) only in scenes with the specular sampler:
    // without it the kernel has VGPRs to spare at 8 waves and plain threadIdx.x is +0.5-1.2 %
    // (configs 2, 5); with it plain threadIdx.x costs SGPR spill lanes, -0.3 % (config 3)
    return fl + "\n" + rtc_defines() + (emit.on && emit.sign_only ? "#define PT_EMIT_SIGN_ONLY 1\n" : "") +
           (ray_stack_on(specular) ? "#define PT_RAY_RESERVE " + std::to_string(ray_reserve()) + "\n" : "#define PT_RAY_STACK 0\n") +
           "#define PT_WAVES " + std::to_string(rtc_waves()) +
           "\n#define PT_FLAT_ONLY 1\n#ifndef PT_KCONST\n#define PT_KCONST 1\n#endif\n#ifndef PT_CAM_KERNARG\n#define PT_CAM_KERNARG 0\n#endif\n"
           "#ifndef PT_FRESH_TID\n#define PT_FRESH_TID " + (specular ? "1" : "0") + "\n#endif\n"
           "typedef __hip_internal::int32_t int32_t; typedef __hip_internal::uint32_t uint32_t;\n"
           "typedef __hip_internal::int64_t int64_t; typedef __hip_internal::uint64_t uint64_t;\n"
           "typedef __hip_internal::uint8_t uint8_t; typedef __hip_internal::uint16_t uint16_t;\n"
           "#if !defined(__HIP_DEVICE_COMPILE__)\n#error expected a device compilation (pt_math.h fast paths)\n#endif\n"
           "#include \"pt_trace.h\"\n" +
           flat_mask_source(leaves, n, specular, tri_fast, albedo_x2, dark, emit, baked) +
           "extern \"C\" __global__ __launch_bounds__(256, PT_WAVES) void pt_trace_flat_rtc(pt::TraceArgs A) {\n"
           "    pt::trace_body_flat<pt::SceneBoxMask>(A);\n}\n";
}

namespace {

// The hipRTC options of the scene kernel. The numerics flags of the offline build
// (Makefile): bit parity depends on them.
// -fno-slp-vectorize: the SLP vectorizer packs the path's scalar f32 math into
// v_pk_* pairs at the price of register shuffles (~20 v_mov per triangle test):
// 44.0 -> 49.0 Grays/s without it (bit-identical either way).
// -disable-machine-licm: as for the offline kernels (Makefile), loop-invariant values are
// not hoisted into registers live across the megakernel loop (60.1 vs 59.4 Grays/s).
// -amdgpu-use-amdgpu-trackers: the scheduler tracks register pressure with the AMDGPU
// trackers; the kernel then needs 62 VGPRs instead of 67 (at 7 waves) and fits 8 waves
// without scratch (LLVM's own trackers: 64 VGPRs and 12 B of scratch at 8). Scheduling
// only: the arithmetic and its bits are unchanged.
std::vector<std::string> rtc_flags() {
    std::vector<std::string> flags = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                                      "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
                                      "-fno-gpu-flush-denormals-to-zero", "-fno-slp-vectorize",
                                      "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-use-amdgpu-trackers"};
#ifdef PT_STAMPS
    flags.push_back("-DPT_STAMPS");
#endif
    for (const std::string& f : rtc_extra_flags()) flags.push_back(f);
    return flags;
}

// ---- on-disk code-object cache: a later process starts on the scene kernel at once
// instead of compiling it again (~0.4 s) while its first launches run the generic kernel.
// Directory: $PT_RTC_CACHE_DIR, else $XDG_CACHE_HOME/pathtracer-amd/rtc, else
// ~/.cache/pathtracer-amd/rtc; PT_RTC_CACHE=0 turns it off. Entry <key>.co, key = sha256 of
// the generated source, the embedded device headers, the compile options, the hipRTC
// version, the HIP runtime version and this format's tag; the file holds a header (magic,
// key, payload size, the payload's sha256) verified on every load, and an entry that fails
// any check is ignored, recompiled and rewritten. Only entries owned by the current user and
// writable by nobody else are read (the directory is created 0700), and an entry whose code
// object the runtime refuses to load is deleted and compiled again (rtc_resolve). Writes go
// to a temporary file renamed into place.
std::atomic<int64_t> g_rtc_disk_hits{0}, g_rtc_disk_rejects{0}, g_rtc_compiles{0};
std::atomic<int64_t> g_rtc_last_compile_us{0}, g_rtc_server_compiles{0};  // pt_debug_rtc_cache 4, 5
constexpr char kRtcMagic[8] = {'P', 'T', 'R', 'T', 'C', '0', '0', '1'};

std::string rtc_cache_dir() {
    const char* off = getenv("PT_RTC_CACHE");
    if (off && *off == '0') return "";
    const char* d = getenv("PT_RTC_CACHE_DIR");
    if (d && *d) return d;
    const char* x = getenv("XDG_CACHE_HOME");
    if (x && *x) return std::string(x) + "/pathtracer-amd/rtc";
    const char* h = getenv("HOME");
    if (h && *h) return std::string(h) + "/.cache/pathtracer-amd/rtc";
    return "";
}

// The file of the loaded library that defines `addr` ("" if none).
std::string lib_of(const void* addr) {
    Dl_info di;
    return dladdr(addr, &di) && di.dli_fname ? std::string(di.dli_fname) : std::string();
}

// The libraries a compile in this process uses: amd_comgr if something loaded it already
// (PyTorch's wheel ships its own, and hipRTC then uses that one), then hipRTC; with
// `runtime`, also the HIP runtime library.
std::vector<std::string> rtc_compiler_libs(bool runtime) {
    std::vector<std::string> libs;
    if (void* h = dlopen("libamd_comgr.so.3", RTLD_NOW | RTLD_NOLOAD)) {
        struct link_map* lm = nullptr;
        if (dlinfo(h, RTLD_DI_LINKMAP, &lm) == 0 && lm && lm->l_name && *lm->l_name) libs.push_back(lm->l_name);
        dlclose(h);
    }
    const std::string rtc = lib_of(reinterpret_cast<const void*>(&hiprtcCompileProgram));
    if (!rtc.empty()) libs.push_back(rtc);
    if (runtime) {
        const std::string hip = lib_of(reinterpret_cast<const void*>(&hipModuleLoadData));
        if (!hip.empty()) libs.push_back(hip);
    }
    return libs;
}

std::string rtc_key(const std::string& src) {
    Sha256 k;
    k.update("pathtracer-amd hipRTC code object v1");
    k.update(src.c_str(), src.size() + 1);
    for (const char* h : {pt_rtc_src_trace, pt_rtc_src_math, pt_rtc_src_stack, pt_rtc_src_lds, pt_rtc_src_hip})
        k.update(h, strlen(h) + 1);
    for (const std::string& f : rtc_flags()) k.update(f.c_str(), f.size() + 1);
    int maj = 0, mnr = 0;
    (void)hiprtcVersion(&maj, &mnr);
    k.update(std::to_string(maj) + "." + std::to_string(mnr));
    // the headers this library was built with, and the identity (path, size, modification
    // time) of the libraries that compile and load the code object in this process: hipRTC,
    // amd_comgr when it is loaded, and the HIP runtime whose loader runs it (no HIP call:
    // pt_rtc_check keys compiles on hosts without a device). An upgraded runtime is a new key;
    // a code object a runtime still refuses is evicted and compiled again (rtc_load).
    k.update(std::to_string(HIP_VERSION) + " " + HIP_VERSION_GITHASH);
    for (const std::string& lib : rtc_compiler_libs(true)) {
        struct stat st;
        const bool ok = stat(lib.c_str(), &st) == 0;
        k.update(lib + " " + (ok ? std::to_string((long long)st.st_size) + " " + std::to_string((long long)st.st_mtime) : "?"));
    }
    return k.hex();
}

// The cache directory is used only if it belongs to this user and nobody else can write to
// it (an existing directory keeps its mode: mkdir's 0700 applies only to new ones).
bool rtc_dir_private(const std::string& dir) {
    struct stat st;
    return stat(dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode) && st.st_uid == geteuid() &&
           !(st.st_mode & (S_IWGRP | S_IWOTH));
}

bool rtc_disk_load(const std::string& key, std::vector<char>& code) {
    const std::string dir = rtc_cache_dir();
    if (dir.empty()) return false;
    if (!rtc_dir_private(dir)) {
        g_rtc_disk_rejects++;
        return false;
    }
    // the checks bind to the file actually read: no symlink is followed, and the owner, mode
    // and type come from the open descriptor
    const std::string path = dir + "/" + key + ".co";
    const int fd = open(path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
    if (fd < 0) {
        if (errno == ELOOP) g_rtc_disk_rejects++;
        return false;
    }
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_uid != geteuid() || (st.st_mode & (S_IWGRP | S_IWOTH)) || !S_ISREG(st.st_mode)) {
        close(fd);
        g_rtc_disk_rejects++;  // another user's (or a shared-writable) entry is never run
        return false;
    }
    auto rd = [fd](void* p, size_t n) {
        char* c = static_cast<char*>(p);
        while (n > 0) {
            const ssize_t r = read(fd, c, n);
            if (r <= 0) return false;
            c += r;
            n -= (size_t)r;
        }
        return true;
    };
    char magic[8], kh[64];
    uint64_t size = 0;
    uint8_t sum[32], got[32];
    bool ok = rd(magic, 8) && memcmp(magic, kRtcMagic, 8) == 0 && rd(kh, 64) && memcmp(kh, key.data(), 64) == 0 &&
              rd(&size, 8) && size > 0 && size < ((uint64_t)1 << 30) && (uint64_t)st.st_size == 112 + size &&
              rd(sum, 32);
    if (ok) {
        code.resize(size);
        ok = rd(code.data(), size);
    }
    close(fd);
    if (ok) {
        Sha256 p;
        p.update(code.data(), code.size());
        p.digest(got);
        ok = memcmp(got, sum, 32) == 0;
    }
    if (!ok) {
        code.clear();
        g_rtc_disk_rejects++;
        return false;
    }
    g_rtc_disk_hits++;
    return true;
}

void rtc_disk_store(const std::string& key, const std::vector<char>& code) {
    const std::string dir = rtc_cache_dir();
    if (dir.empty() || code.empty()) return;
    for (size_t i = 1; i <= dir.size(); i++)  // mkdir -p
        if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0700);
    if (!rtc_dir_private(dir)) return;
    std::ostringstream tn;
    tn << dir << "/" << key << ".co.tmp." << getpid() << "." << std::this_thread::get_id();
    const std::string tmp = tn.str();
    {
        const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0600);  // owner-only entry
        if (fd < 0) return;
        close(fd);
        std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
        if (!f) return;
        uint8_t sum[32];
        Sha256 p;
        p.update(code.data(), code.size());
        p.digest(sum);
        const uint64_t size = code.size();
        f.write(kRtcMagic, 8);
        f.write(key.data(), 64);
        f.write(reinterpret_cast<const char*>(&size), 8);
        f.write(reinterpret_cast<const char*>(sum), 32);
        f.write(code.data(), (std::streamsize)code.size());
        if (!f) {
            f.close();
            (void)unlink(tmp.c_str());
            return;
        }
    }
    if (rename(tmp.c_str(), (dir + "/" + key + ".co").c_str()) != 0) (void)unlink(tmp.c_str());
}

// ---- compile server (tools/pt_rtc_server.cc): the compiles run in a child process that
// loads the same hipRTC / amd_comgr libraries as this one. In this process a compile on a
// background thread runs inside amd_comgr, whose lazily constructed statics register their
// destructors with atexit during the compile — after any handler that waits for it — so a
// process exiting with a compile in flight destroyed them under it (SIGSEGV in the compile
// thread, a call through a destroyed object from amd_comgr_do_action; reproduced without a
// GPU, tests/test_rtc_exit.py). With the server, exit only closes a socket.
// One server per process, started on the first compile, one request at a time; it exits at
// end of input. PT_RTC_SERVER=0 (test hook), a missing server binary or a failed exchange:
// the compile runs in this process (the round-5 form).
struct RtcServer {
    std::mutex mu;
    pid_t pid = -1;
    int fd = -1;
    bool broken = false;  // could not start or failed: compile in this process from then on
};
RtcServer& rtc_server() {
    static RtcServer* s = new RtcServer();  // never destroyed (used by threads at exit)
    return *s;
}

// bin/pt_rtc_server next to this library's lib/ directory ("" if absent)
std::string rtc_server_path() {
    if (hook_off("PT_RTC_SERVER")) return "";
    std::string p = lib_of(reinterpret_cast<const void*>(&rtc_server_path));
    const size_t k = p.rfind('/');
    if (k == std::string::npos) return "";
    p = p.substr(0, k) + "/../bin/pt_rtc_server";
    return access(p.c_str(), X_OK) == 0 ? p : "";
}

bool rtc_server_start(RtcServer& s) {
    const std::string path = rtc_server_path();
    if (path.empty()) return false;
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0, sv) != 0) return false;
    std::vector<std::string> args{path};
    for (const std::string& lib : rtc_compiler_libs(false)) args.insert(args.end(), {"--lib", lib});
    std::vector<char*> argv;
    for (std::string& a : args) argv.push_back(&a[0]);
    argv.push_back(nullptr);
    posix_spawn_file_actions_t fa;
    posix_spawnattr_t at;
    posix_spawn_file_actions_init(&fa);
    posix_spawn_file_actions_adddup2(&fa, sv[1], 0);
    posix_spawn_file_actions_adddup2(&fa, sv[1], 1);
    posix_spawn_file_actions_addclosefrom_np(&fa, 3);  // no GPU or other descriptors of ours in the child
    posix_spawnattr_init(&at);
    sigset_t none, dflt;
    sigemptyset(&none);
    sigemptyset(&dflt);
    sigaddset(&dflt, SIGPIPE);
    posix_spawnattr_setsigmask(&at, &none);
    posix_spawnattr_setsigdefault(&at, &dflt);
    posix_spawnattr_setflags(&at, POSIX_SPAWN_SETSIGMASK | POSIX_SPAWN_SETSIGDEF);
    pid_t pid = -1;
    const int rc = posix_spawn(&pid, path.c_str(), &fa, &at, argv.data(), environ);
    posix_spawn_file_actions_destroy(&fa);
    posix_spawnattr_destroy(&at);
    close(sv[1]);
    if (rc != 0) {
        close(sv[0]);
        return false;
    }
    s.pid = pid;
    s.fd = sv[0];
    return true;
}

void rtc_server_stop(RtcServer& s) {
    if (s.fd >= 0) close(s.fd);
    if (s.pid > 0) {
        kill(s.pid, SIGKILL);
        (void)waitpid(s.pid, nullptr, 0);
    }
    s.fd = -1;
    s.pid = -1;
    s.broken = true;
}

// One compile through the server; false if the exchange failed (then the caller compiles here).
bool rtc_server_compile(const std::string& src, RtcCode& out) {
    RtcServer& s = rtc_server();
    std::lock_guard<std::mutex> lock(s.mu);
    if (s.broken) return false;
    if (s.fd < 0 && !rtc_server_start(s)) {
        s.broken = true;
        return false;
    }
    const int fd = s.fd;
    auto put = [fd](const void* p, size_t n) {
        const char* c = static_cast<const char*>(p);
        while (n > 0) {
            const ssize_t r = send(fd, c, n, MSG_NOSIGNAL);
            if (r <= 0) return false;
            c += r;
            n -= (size_t)r;
        }
        return true;
    };
    auto get = [fd](void* p, size_t n) {
        char* c = static_cast<char*>(p);
        while (n > 0) {
            const ssize_t r = recv(fd, c, n, 0);
            if (r <= 0) return false;
            c += r;
            n -= (size_t)r;
        }
        return true;
    };
    auto put_str = [&put](const char* str, size_t n) {
        const uint64_t len = n;
        return put(&len, 8) && put(str, n);
    };
    const char* hdrs[] = {pt_rtc_src_trace, pt_rtc_src_math, pt_rtc_src_stack, pt_rtc_src_lds, pt_rtc_src_hip};
    const char* names[] = {"pt_trace.h", "pt_math.h", "pt_raystack.h", "pt_flatlds.h", "pt_hip.h"};
    const std::vector<std::string> flags = rtc_flags();
    const uint32_t head[3] = {0x51525450u /* "PTRQ" */, 5u, (uint32_t)flags.size()};
    bool ok = put(head, 12) && put_str(src.data(), src.size());
    for (int i = 0; ok && i < 5; i++) ok = put_str(names[i], strlen(names[i])) && put_str(hdrs[i], strlen(hdrs[i]));
    for (size_t i = 0; ok && i < flags.size(); i++) ok = put_str(flags[i].data(), flags[i].size());
    uint32_t resp[2] = {0, 0};
    uint64_t n = 0;
    ok = ok && get(resp, 8) && resp[0] == 0x53525450u /* "PTRS" */ && get(&n, 8) && n < ((uint64_t)1 << 30);
    std::vector<char> bytes;
    if (ok) {
        bytes.resize(n);
        ok = n == 0 || get(bytes.data(), n);
    }
    if (!ok) {
        rtc_server_stop(s);
        return false;
    }
    if (resp[1] == 1) {
        out.code = std::move(bytes);
    } else {
        out.status = "hipRTC compile failed: " + std::string(bytes.begin(), bytes.begin() + std::min<size_t>(bytes.size(), 400));
    }
    return true;
}

// Compile `src` to a code object (or an error status), stored in the disk cache under
// `key`. Runs on a background thread: through the compile server when there is one.
std::shared_ptr<const RtcCode> rtc_compile(const std::string& src, const std::string& key) {
    auto out = std::make_shared<RtcCode>();
    g_rtc_compiles++;
    const auto t0 = std::chrono::steady_clock::now();
    auto done = [&t0]() {
        g_rtc_last_compile_us =
            std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    };
    if (rtc_server_compile(src, *out)) {
        done();
        g_rtc_server_compiles++;
        if (!out->code.empty()) rtc_disk_store(key, out->code);
        return out;
    }
    const char* hdrs[] = {pt_rtc_src_trace, pt_rtc_src_math, pt_rtc_src_stack, pt_rtc_src_lds, pt_rtc_src_hip};
    const char* names[] = {"pt_trace.h", "pt_math.h", "pt_raystack.h", "pt_flatlds.h", "pt_hip.h"};
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "pt_trace_flat_rtc.hip", 5, hdrs, names) != HIPRTC_SUCCESS) {
        out->status = "hiprtcCreateProgram failed";
        return out;
    }
    const std::vector<std::string> flags = rtc_flags();
    std::vector<const char*> opts;
    for (const std::string& f : flags) opts.push_back(f.c_str());
    if (hiprtcCompileProgram(prog, (int)opts.size(), opts.data()) != HIPRTC_SUCCESS) {
        size_t ls = 0;
        hiprtcGetProgramLogSize(prog, &ls);
        std::string log(ls, '\0');
        if (ls) hiprtcGetProgramLog(prog, &log[0]);
        out->status = "hipRTC compile failed: " + log.substr(0, 400);
    } else {
        size_t cs = 0;
        hiprtcGetCodeSize(prog, &cs);
        out->code.resize(cs);
        hiprtcGetCode(prog, out->code.data());
        done();
        rtc_disk_store(key, out->code);
    }
    hiprtcDestroyProgram(&prog);
    return out;
}

}  // namespace

// Wait for every background compile started so far (deferred jobs are not run); returns how
// many were still running.
int rtc_wait_all() {
    std::vector<RtcFuture> jobs;
    {
        RtcCache& c = rtc_cache();
        std::lock_guard<std::mutex> lock(c.mu);
        for (auto& kv : c.code) jobs.push_back(kv.second);
    }
    int running = 0;
    for (RtcFuture& f : jobs) {
        if (!f.valid()) continue;
        const std::future_status st = f.wait_for(std::chrono::seconds(0));
        if (st == std::future_status::deferred) continue;
        if (st != std::future_status::ready) running++;
        f.wait();
    }
    return running;
}

// Background compiles: with the compile server the exit handler below only waits for its
// answer (so the code object reaches the disk cache for the next process). Without a server
// the compile runs in this process, and the compiler library is loaded first so that at least
// its load-time statics outlive the handler (exit() runs handlers in reverse registration
// order); the statics it constructs during a compile are not covered (see RtcServer), which is
// why the server is the default. No compiler library: compiles run synchronously.
bool rtc_async_ready() {
    static const bool ok = [] {
        if (rtc_server_path().empty()) {
            void* h = dlopen("libamd_comgr.so.3", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("libamd_comgr.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) return false;
        }
        std::atexit([] { (void)rtc_wait_all(); });
        return true;
    }();
    return ok;
}

// The compile job for `src`: the process's own result if it has one, else a verified
// entry of the disk cache (read here, so the first launch already finds the kernel ready),
// else a compile started on first request (on a background thread when possible); shared
// by every context and device that asks for the same source.
RtcFuture rtc_job(const std::string& src) {
    RtcCache& cache = rtc_cache();
    const bool async = rtc_async_ready();
    std::lock_guard<std::mutex> lock(cache.mu);
    auto it = cache.code.find(src);
    if (it != cache.code.end()) return it->second;
    const std::string key = rtc_key(src);
    RtcFuture f;
    auto disk = std::make_shared<RtcCode>();
    // an entry the runtime refused once is never read again (rtc_load): the retry compiles
    if (!cache.refused.count(key) && rtc_disk_load(key, disk->code)) {
        disk->disk_key = key;
        std::promise<std::shared_ptr<const RtcCode>> p;
        p.set_value(disk);
        f = p.get_future().share();
    } else {
        f = async ? std::async(std::launch::async, rtc_compile, src, key).share()
                  : std::async(std::launch::deferred, rtc_compile, src, key).share();
    }
    cache.code.emplace(src, f);
    return f;
}

// Load a finished compile of `src` on `device` (once per device and source).
hipFunction_t rtc_load(int device, const std::string& src, const RtcCode& code, std::string& status) {
    if (code.code.empty()) {
        status = code.status;
        return nullptr;
    }
    RtcCache& cache = rtc_cache();
    std::lock_guard<std::mutex> lock(cache.mu);
    auto fit = cache.funcs.find({device, src});
    if (fit != cache.funcs.end()) return fit->second;
    hipModule_t mod;
    hipFunction_t fn;
    if (hipModuleLoadData(&mod, code.code.data()) != hipSuccess ||
        hipModuleGetFunction(&fn, mod, "pt_trace_flat_rtc") != hipSuccess) {
        status = "hipModuleLoadData/GetFunction failed";
        if (!code.disk_key.empty()) {  // a cached entry this runtime refuses: evicted, compiled again
            const std::string dir = rtc_cache_dir();
            if (!dir.empty()) (void)unlink((dir + "/" + code.disk_key + ".co").c_str());
            g_rtc_disk_rejects++;
            cache.code.erase(src);
            // marked even if the unlink failed (a read-only cache): the next job for this
            // source compiles instead of reading the entry again, so the retry happens once
            cache.refused.insert(code.disk_key);
            status = "evicted";
        }
        return nullptr;
    }
    cache.funcs[{device, src}] = fn;
    status.clear();
    return fn;
}

}  // namespace pt

using namespace pt;

extern "C" {

// Test hook: generate and compile the scene-specialised flat kernel without a device.
int pt_rtc_check(const pt_scene* scene, char* src_out, size_t cap) {
    PackedScene ps;
    const int rc = pack_scene(scene, ps);
    if (rc) return rc;
    if (!flat_eligible(ps))
        return set_error(PT_E_ARG, "scene has no flat leaf list (%d leaves, %d triangles)", ps.num_leaves, ps.num_tris);
    const std::string src =
        rtc_flat_source(ps.leaves, ps.num_leaves, scene_has_specular(ps), ps.coords_small, albedo_x2_ok(ps), scene_dark(ps),
                        scene_emit_box(ps, scene_dark(ps)),
                        rtc_baked(ps.num_tris, scene_has_specular(ps), flat_box_pairs(ps.leaves, ps.num_leaves)));
    if (src_out && cap) {
        const size_t n = std::min(cap - 1, src.size());
        memcpy(src_out, src.data(), n);
        src_out[n] = 0;
    }
    const std::shared_ptr<const RtcCode> code = rtc_job(src).get();
    if (code->code.empty()) return set_error(PT_E_HIP, "%s", code->status.c_str());
    return (int)code->code.size();
}

// Test hook (no device needed): start the scene kernel's compile as pt_ctx_set_scene does (in
// the background) and return at once: 1 if a compile is running, 0 if the job was already
// done (a disk-cache hit or an earlier compile).
int pt_debug_rtc_start(const pt_scene* scene) {
    PackedScene ps;
    const int rc = pack_scene(scene, ps);
    if (rc) return rc;
    if (!flat_eligible(ps))
        return set_error(PT_E_ARG, "scene has no flat leaf list (%d leaves, %d triangles)", ps.num_leaves, ps.num_tris);
    const RtcFuture f = rtc_job(
        rtc_flat_source(ps.leaves, ps.num_leaves, scene_has_specular(ps), ps.coords_small, albedo_x2_ok(ps), scene_dark(ps),
                        scene_emit_box(ps, scene_dark(ps)),
                        rtc_baked(ps.num_tris, scene_has_specular(ps), flat_box_pairs(ps.leaves, ps.num_leaves))));
    return f.wait_for(std::chrono::seconds(0)) == std::future_status::ready ? 0 : 1;
}

// Test hook (no device needed): the hipRTC code-object caches. op 0 forgets this process's
// compiles and loaded scene kernels (later requests go to the disk cache or compile again;
// contexts keep the kernels they hold), 1 / 2 / 3 return the disk-cache hits, the rejected
// (corrupt or mismatched) entries and the compiles so far.
int64_t pt_debug_rtc_cache(int32_t op) {
    if (op == 0) {
        RtcCache& c = rtc_cache();
        std::lock_guard<std::mutex> lock(c.mu);
        for (auto& kv : c.code) kv.second.wait();
        c.code.clear();
        c.funcs.clear();  // the modules stay loaded (a context may still launch them)
        return 0;
    }
    if (op == 1) return g_rtc_disk_hits.load();
    if (op == 2) return g_rtc_disk_rejects.load();
    if (op == 3) return g_rtc_compiles.load();
    if (op == 4) return g_rtc_last_compile_us.load();
    if (op == 5) return g_rtc_server_compiles.load();
    return set_error(PT_E_ARG, "pt_debug_rtc_cache: bad op %d", op);
}

}  // extern "C"
