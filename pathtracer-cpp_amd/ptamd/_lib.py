"""ctypes binding of libpt_hip.so (C ABI declared in include/pt_hip.h).

The library is built in-tree (``make -C pathtracer-cpp_amd``); loading fails
loudly when it is missing — there is no fallback implementation.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
import subprocess
from typing import Optional

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # pathtracer-cpp_amd/
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.environ.get("PT_LIB") or os.path.join(PKG_ROOT, "lib", "libpt_hip.so")

PT_OK, PT_E_ARG, PT_E_EMPTY, PT_E_HIP, PT_E_IO, PT_E_RUNAWAY = 0, -1, -2, -3, -4, -5
PT_SEED = 1
PT_MAX_DEPTH = 64

EXPORTED = (
    "pt_abi_version", "pt_last_error", "pt_device_count", "pt_bvh_build", "pt_camera_init",
    "pt_ctx_create", "pt_ctx_destroy", "pt_ctx_set_scene", "pt_ctx_prepare", "pt_rtc_wait", "pt_ctx_render", "pt_part_rows",
    "pt_render_f32", "pt_image_to_rgb8", "pt_write_png", "pt_debug_math", "pt_debug_sweep", "pt_scene_validate", "pt_rtc_check",
    "pt_ctx_render_progressive", "pt_ctx_render_rgb8", "pt_rgb8_thresholds", "pt_debug_rgb8",
    "pt_obj_load", "pt_obj_num_tris", "pt_obj_triangles", "pt_obj_warnings", "pt_obj_free",
    "pt_render_f32_devices", "pt_render_rgb8_devices", "pt_scene_info", "pt_debug_wide_verify",
    "pt_debug_rccl_failover", "pt_debug_rtc_cache", "pt_devices_release", "pt_debug_ctx_flags", "pt_debug_counter",
    "pt_debug_scene_dark", "pt_debug_rtc_start", "pt_debug_pack_hash",
    "pt_bvh_intersect", "pt_ctx_intersect", "pt_ctx_render_aov",
    "pt_bvh_trace", "pt_ctx_trace", "pt_debug_ctx_plan", "pt_debug_walk_placement",
    "pt_bvh_trace_grad", "pt_ctx_trace_grad",
    "pt_debug_emit_reject", "pt_debug_emit_box", "pt_debug_ctx_emit_reject", "pt_debug_emit_slab_reject", "pt_debug_ray_stack",
    "pt_ctx_render_moments", "pt_moments_unconverged", "pt_ctx_unconverged", "pt_ctx_render_converge",
    "pt_ctx_render_adaptive",
    "pt_moments_variance", "pt_ctx_moments_variance", "pt_image_denoise", "pt_ctx_denoise", "pt_ctx_render_denoised",
    "pt_image_temporal", "pt_ctx_temporal", "pt_ctx_render_temporal",
    "pt_scene_lights", "pt_bvh_trace_nee", "pt_ctx_trace_nee", "pt_ctx_render_nee",
    "pt_bvh_trace_nee_opt", "pt_ctx_trace_nee_opt", "pt_ctx_render_nee_opt",
    "pt_bvh_trace_nee_grad", "pt_ctx_trace_nee_grad",
    "pt_bvh_render_grad", "pt_bvh_render_nee_grad", "pt_ctx_render_grad", "pt_ctx_render_nee_grad",
    "pt_debug_host_camera_rays",
)
PT_NEE_MIS_NONE, PT_NEE_MIS_BALANCE = 0, 1
PT_MAX_DEVICES = 16


class pt_bvh_node(C.Structure):
    _fields_ = [("lb", C.c_float * 3), ("rt", C.c_float * 3), ("left", C.c_int32), ("right", C.c_int32),
                ("tri_start", C.c_int32), ("tri_end", C.c_int32)]


class pt_material(C.Structure):
    _fields_ = [("type", C.c_int32), ("color", C.c_float * 3), ("emit", C.c_float * 3), ("roughness", C.c_float)]


class pt_scene(C.Structure):
    _fields_ = [("num_tris", C.c_int32), ("verts", C.c_void_p), ("materials", C.c_void_p),
                ("num_nodes", C.c_int32), ("nodes", C.c_void_p), ("tri_idx", C.c_void_p)]


class pt_camera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("res", C.c_int32 * 2), ("v_res", C.c_float * 2), ("cell_size", C.c_float),
                ("distance", C.c_float), ("transform", C.c_float * 9)]


class pt_params(C.Structure):
    _fields_ = [("spp", C.c_int32), ("depth", C.c_int32), ("seed", C.c_uint32), ("part_index", C.c_int32),
                ("part_count", C.c_int32), ("band_rows", C.c_int32), ("batch_spp", C.c_int32),
                ("samples_per_item", C.c_int32), ("progress", C.c_void_p), ("progress_user", C.c_void_p)]


class pt_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("paths", C.c_uint64), ("runaway", C.c_uint64), ("kernel_ms", C.c_double),
                ("reduce_ms", C.c_double), ("total_ms", C.c_double), ("trace_launches", C.c_int32),
                ("rows", C.c_int32), ("kernel_path", C.c_int32), ("n_devices", C.c_int32),
                ("gather_path", C.c_int32), ("gather_ms", C.c_double),
                ("device_kernel_ms", C.c_double * PT_MAX_DEVICES), ("device_render_ms", C.c_double * PT_MAX_DEVICES),
                ("device_rays", C.c_uint64 * PT_MAX_DEVICES)]

    PATHS = {0: "pt_trace_kernel<false,false> (tree, global)", 1: "pt_trace_kernel<true,false> (tree, LDS)",
             2: "pt_trace_kernel<true,true> (flat, table)", 3: "pt_trace_flat_rtc (flat, hipRTC-specialised)",
             4: "pt_trace_kernel<false,false,W> (wide tree, global)",
             5: "pt_flat_fast_kernel (flat, table with the scene's flags)"}

    GATHERS = {0: "none", 1: "rccl", 2: "host", 3: "host (RCCL unavailable or failed)"}

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_}
        n = max(self.n_devices, 0)
        for k in ("device_kernel_ms", "device_render_ms", "device_rays"):
            d[k] = list(d[k])[:n]
        return d


PT_QUERY_CLOSEST, PT_QUERY_ANY = 0, 1


class pt_query_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("hits", C.c_uint64), ("kernel_ms", C.c_double), ("total_ms", C.c_double),
                ("launches", C.c_int32), ("lds_scene", C.c_int32), ("lds_stack", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class pt_trace_params(C.Structure):
    """trace() on caller-supplied rays (include/pt_hip.h); states NULL = pt_sample_seed(i, s, seed)."""
    _fields_ = [("depth", C.c_int32), ("spp", C.c_int32), ("seed", C.c_uint32), ("states", C.c_void_p)]


class pt_trace_stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("paths", C.c_uint64), ("runaway", C.c_uint64), ("kernel_ms", C.c_double),
                ("reduce_ms", C.c_double), ("total_ms", C.c_double), ("launches", C.c_int32),
                ("lds_scene", C.c_int32), ("lds_stack", C.c_int32), ("lds_records", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class pt_trace_grad_io(C.Structure):
    """Overrides, upstream gradient and outputs of trace_grad (include/pt_hip.h); NULL = not given / not wanted."""
    _fields_ = [("color", C.c_void_p), ("emit", C.c_void_p), ("grad_rgb", C.c_void_p), ("rgb_out", C.c_void_p),
                ("grad_color", C.c_void_p), ("grad_emit", C.c_void_p)]


class pt_grad_stats(C.Structure):
    _fields_ = [("trace", pt_trace_stats), ("terms", C.c_uint64), ("grad_ms", C.c_double), ("lds_table", C.c_int32),
                ("reserved", C.c_int32)]

    def as_dict(self) -> dict:
        d = self.trace.as_dict()
        d.update(terms=self.terms, grad_ms=self.grad_ms, lds_table=self.lds_table)
        return d


class pt_nee_stats(C.Structure):
    """Light sampling (include/pt_hip.h): pt_trace_stats (rays = path and shadow segments) and the light counts."""
    _fields_ = [("trace", pt_trace_stats), ("shadow_rays", C.c_uint64), ("light_draws", C.c_uint64),
                ("lights", C.c_int32), ("light_area", C.c_float)]

    def as_dict(self) -> dict:
        d = self.trace.as_dict()
        d.update(shadow_rays=self.shadow_rays, light_draws=self.light_draws, lights=self.lights, light_area=self.light_area)
        return d


class pt_nee_options(C.Structure):
    """Options of the *_nee_opt calls (include/pt_hip.h): mis = PT_NEE_MIS_*, the reserved words 0."""
    _fields_ = [("mis", C.c_int32), ("reserved", C.c_int32 * 3)]


class pt_nee_grad_stats(C.Structure):
    """Material gradients of the light-sampling estimator (include/pt_hip.h): pt_nee_stats and pt_grad_stats' own fields."""
    _fields_ = [("nee", pt_nee_stats), ("terms", C.c_uint64), ("grad_ms", C.c_double), ("lds_table", C.c_int32),
                ("reserved", C.c_int32)]

    def as_dict(self) -> dict:
        d = self.nee.as_dict()
        d.update(terms=self.terms, grad_ms=self.grad_ms, lds_table=self.lds_table)
        return d


class pt_moments(C.Structure):
    """Per-pixel sample moments (include/pt_hip.h); a NULL pointer skips the output."""
    NAMES = ("sum", "sumsq", "sem")
    _fields_ = [(k, C.c_void_p) for k in NAMES]


class pt_converge(C.Structure):
    _fields_ = [("rel", C.c_float), ("abs", C.c_float), ("min_spp", C.c_int32), ("max_spp", C.c_int32),
                ("step", C.c_int32), ("max_unconverged", C.c_int64)]


class pt_converge_stats(C.Structure):
    _fields_ = [("spp", C.c_int32), ("rounds", C.c_int32), ("unconverged", C.c_int64), ("rays", C.c_uint64),
                ("kernel_ms", C.c_double), ("reduce_ms", C.c_double), ("total_ms", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class pt_adaptive(C.Structure):
    """Adaptive sampling (include/pt_hip.h): pt_converge and the active fraction at which the rounds go per pixel."""
    _fields_ = [("conv", pt_converge), ("sparse_below", C.c_float)]


class pt_adaptive_stats(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("dense_rounds", C.c_int32), ("max_spp", C.c_int32),
                ("sparse_launches", C.c_int32), ("unconverged", C.c_int64), ("samples", C.c_int64),
                ("rays", C.c_uint64), ("sparse_rays", C.c_uint64), ("kernel_ms", C.c_double),
                ("reduce_ms", C.c_double), ("total_ms", C.c_double), ("sparse_kernel_ms", C.c_double)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class pt_denoise_guides(C.Structure):
    """The denoiser's first-hit guides (include/pt_hip.h): all five are needed."""
    NAMES = ("normal", "t", "tri", "emission", "position")
    WIDTH = {"normal": 3, "t": 1, "tri": 1, "emission": 3, "position": 3}
    _fields_ = [(k, C.c_void_p) for k in NAMES]


class pt_denoise_params(C.Structure):
    """A 0 selects the default: 5 passes, sigma_l 1, sigma_z 0.01, normal power 2^7, eps 1e-6."""
    _fields_ = [("passes", C.c_int32), ("sigma_l", C.c_float), ("sigma_z", C.c_float), ("normal_pow_log2", C.c_int32),
                ("eps", C.c_float)]


PT_DENOISE_DIRECT, PT_DENOISE_LDS = 1, 2


class pt_denoise_stats(C.Structure):
    FORMS = {0: None, PT_DENOISE_DIRECT: "direct", PT_DENOISE_LDS: "lds"}
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("passes", C.c_int32), ("launches", C.c_int32),
                ("form", C.c_int32 * 8), ("pass_ms", C.c_float * 8), ("pack_ms", C.c_float), ("reserved", C.c_int32)]

    def as_dict(self) -> dict:
        n = self.passes
        return {"kernel_ms": self.kernel_ms, "total_ms": self.total_ms, "passes": n, "launches": self.launches,
                "form": [self.FORMS[f] for f in list(self.form)[:n]], "pass_ms": list(self.pass_ms)[:n],
                "pack_ms": self.pack_ms}


class pt_denoised_stats(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("aov_ms", C.c_double), ("variance_ms", C.c_double),
                ("denoise", pt_denoise_stats)]


class pt_temporal_history(C.Structure):
    """The seven planes of an accumulated history (include/pt_hip.h)."""
    NAMES = ("color", "m2", "var", "hist", "normal", "position", "cls")
    WIDTH = {"color": 3, "m2": 3, "var": 3, "hist": 1, "normal": 3, "position": 3, "cls": 1}
    INT = ("hist", "cls")
    _fields_ = [(k, C.c_void_p) for k in NAMES]


PT_TEMPORAL_VAR_SAMPLE, PT_TEMPORAL_VAR_TEMPORAL = 1, 2


class pt_temporal_params(C.Structure):
    """A 0 selects the default: max_history 32, sigma_z 0.01, normal_min 0.9, sample mode with a variance."""
    _fields_ = [("max_history", C.c_int32), ("sigma_z", C.c_float), ("normal_min", C.c_float),
                ("variance_mode", C.c_int32)]


class pt_temporal_stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("reused", C.c_int64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class pt_render_temporal_stats(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("render_ms", C.c_double), ("aov_ms", C.c_double), ("variance_ms", C.c_double),
                ("rays", C.c_uint64), ("had_history", C.c_int32), ("variance_mode", C.c_int32),
                ("temporal", pt_temporal_stats), ("denoise", pt_denoise_stats)]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_[:7]}
        d.update(temporal=self.temporal.as_dict(), denoise=self.denoise.as_dict(), reused=self.temporal.reused)
        return d


class pt_aov(C.Structure):
    """First-hit channels (include/pt_hip.h); a NULL pointer skips the channel."""
    CHANNELS = ("t", "tri", "normal", "albedo", "emission", "ray")
    WIDTH = {"t": 1, "tri": 1, "normal": 3, "albedo": 3, "emission": 3, "ray": 6}
    _fields_ = [(k, C.c_void_p) for k in CHANNELS]


assert C.sizeof(pt_bvh_node) == 40 and C.sizeof(pt_material) == 32 and C.sizeof(pt_trace_stats) == 64
assert C.sizeof(pt_nee_stats) == 88
assert C.sizeof(pt_nee_options) == 16
assert C.sizeof(pt_nee_grad_stats) == 112
assert C.sizeof(pt_denoise_params) == 20 and C.sizeof(pt_denoise_stats) == 96 and C.sizeof(pt_denoise_guides) == 40
assert C.sizeof(pt_temporal_params) == 16 and C.sizeof(pt_temporal_stats) == 24 and C.sizeof(pt_temporal_history) == 56


class PTError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{msg} (code {code})")
        self.code = code


_lib: Optional[C.CDLL] = None


def build(force: bool = False) -> str:
    """Compile libpt_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-C", PKG_ROOT], check=True)
    return LIB_PATH


def _torch_runtime_first() -> None:
    """PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, no
    SONAME); libpt_hip.so links the system one (/opt/rocm). With both in one process,
    torch.cuda fails ("No HIP GPUs are available") when the system runtime initialised the
    devices first, while the other order works. So when torch is installed its runtime is
    brought up first (import + device count), and the two coexist."""
    import importlib.util
    if importlib.util.find_spec("torch") is None:
        return
    import torch
    torch.cuda.device_count()


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libpt_hip.so not built at {LIB_PATH}: run `make -C pathtracer-cpp_amd` "
                               "(there is no CPU fallback)")
        _torch_runtime_first()
        L = C.CDLL(LIB_PATH)
        P = C.c_void_p
        L.pt_abi_version.restype = C.c_int
        L.pt_last_error.restype = C.c_char_p
        L.pt_device_count.restype = C.c_int
        L.pt_bvh_build.argtypes = [C.c_int32, P, P, P]
        L.pt_camera_init.argtypes = [P, P, P, C.c_int32, C.c_int32, C.c_float, C.c_float, C.POINTER(pt_camera)]
        L.pt_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.pt_ctx_destroy.argtypes = [P]
        L.pt_ctx_destroy.restype = None
        L.pt_ctx_set_scene.argtypes = [P, C.POINTER(pt_scene)]
        L.pt_ctx_prepare.argtypes = [P]
        L.pt_rtc_wait.argtypes = []
        L.pt_rtc_wait.restype = C.c_int
        # no background compile left running into interpreter finalisation (pt_rtc_wait)
        atexit.register(L.pt_rtc_wait)
        L.pt_ctx_render.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params), P, C.c_int, C.POINTER(pt_stats)]
        L.pt_part_rows.argtypes = [C.c_int32] * 4
        L.pt_part_rows.restype = C.c_int32
        L.pt_render_f32.argtypes = [C.POINTER(pt_scene), C.POINTER(pt_camera), C.POINTER(pt_params), P,
                                    C.POINTER(pt_stats)]
        L.pt_image_to_rgb8.argtypes = [P, C.c_int32, C.c_int32, C.c_float, P]
        L.pt_write_png.argtypes = [C.c_char_p, P, C.c_int32, C.c_int32]
        L.pt_debug_math.argtypes = [C.c_int, C.c_int, P, C.c_int, P]
        L.pt_debug_sweep.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, P, P]
        L.pt_ctx_render_progressive.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params), C.c_int32,
                                                C.c_int32, P, C.c_int, C.POINTER(pt_stats)]
        L.pt_ctx_render_rgb8.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params), C.c_float, C.c_int, P,
                                         C.c_int, C.POINTER(pt_stats)]
        L.pt_rgb8_thresholds.argtypes = [C.c_float, P, P]
        L.pt_debug_rgb8.argtypes = [C.c_int, P, C.c_int32, C.c_int32, C.c_float, P]
        L.pt_render_f32_devices.argtypes = [C.POINTER(pt_scene), C.POINTER(pt_camera), C.POINTER(pt_params), P,
                                            C.c_int32, P, C.POINTER(pt_stats)]
        L.pt_render_rgb8_devices.argtypes = [C.POINTER(pt_scene), C.POINTER(pt_camera), C.POINTER(pt_params), P,
                                             C.c_int32, C.c_float, P, C.POINTER(pt_stats)]
        L.pt_obj_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
        L.pt_obj_num_tris.argtypes = [P]
        L.pt_obj_num_tris.restype = C.c_int32
        L.pt_obj_triangles.argtypes = [P, P, P, P]
        L.pt_obj_warnings.argtypes = [P]
        L.pt_obj_warnings.restype = C.c_char_p
        L.pt_obj_free.argtypes = [P]
        L.pt_obj_free.restype = None
        L.pt_scene_validate.argtypes = [C.POINTER(pt_scene), P]
        L.pt_scene_info.argtypes = [C.POINTER(pt_scene), P, C.c_int32]
        L.pt_debug_wide_verify.argtypes = [C.POINTER(pt_scene), C.c_int32]
        L.pt_rtc_check.argtypes = [C.POINTER(pt_scene), C.c_char_p, C.c_size_t]
        L.pt_bvh_intersect.argtypes = [C.POINTER(pt_scene), P, P, C.c_int64, P, P]
        L.pt_ctx_intersect.argtypes = [P, P, P, C.c_int64, C.c_int, P, P, P, C.c_int, C.POINTER(pt_query_stats)]
        L.pt_ctx_render_aov.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params), C.c_int32, C.POINTER(pt_aov),
                                        C.c_int, C.POINTER(pt_query_stats)]
        L.pt_bvh_trace.argtypes = [C.POINTER(pt_scene), P, P, C.c_int64, C.POINTER(pt_trace_params), P,
                                   C.POINTER(pt_trace_stats)]
        L.pt_ctx_trace.argtypes = [P, P, P, C.c_int64, C.POINTER(pt_trace_params), P, C.c_int, C.POINTER(pt_trace_stats)]
        if hasattr(L, "pt_ctx_trace_grad"):  # absent from older builds used in A/B runs
            L.pt_bvh_trace_grad.argtypes = [C.POINTER(pt_scene), P, P, C.c_int64, C.POINTER(pt_trace_params),
                                            C.POINTER(pt_trace_grad_io), C.POINTER(pt_grad_stats)]
            L.pt_ctx_trace_grad.argtypes = [P, P, P, C.c_int64, C.POINTER(pt_trace_params), C.POINTER(pt_trace_grad_io),
                                            C.c_int, C.POINTER(pt_grad_stats)]
        if hasattr(L, "pt_ctx_render_moments"):  # absent from older builds used in A/B runs
            L.pt_ctx_render_moments.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params), C.c_int32, C.c_int32, P,
                                                C.POINTER(pt_moments), C.c_int, C.POINTER(pt_stats)]
            L.pt_moments_unconverged.argtypes = [P, P, C.c_int64, C.c_int32, C.c_float, C.c_float,
                                                 C.POINTER(C.c_int64), P]
            L.pt_ctx_unconverged.argtypes = [P, C.c_float, C.c_float, C.POINTER(C.c_int64), P, C.c_int]
            L.pt_ctx_render_converge.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params), C.POINTER(pt_converge), P,
                                                 C.POINTER(pt_moments), C.c_int, C.POINTER(pt_converge_stats)]
        if hasattr(L, "pt_ctx_render_adaptive"):  # absent from older builds used in A/B runs
            L.pt_ctx_render_adaptive.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params), C.POINTER(pt_adaptive), P,
                                                 C.POINTER(pt_moments), P, C.c_int, C.POINTER(pt_adaptive_stats)]
        if hasattr(L, "pt_ctx_denoise"):  # absent from older builds used in A/B runs
            L.pt_moments_variance.argtypes = [P, P, C.c_int64, C.c_int32, P, P]
            L.pt_ctx_moments_variance.argtypes = [P, P, P, C.c_int64, C.c_int32, P, P, C.c_int]
            L.pt_image_denoise.argtypes = [C.c_int32, C.c_int32, P, P, C.POINTER(pt_denoise_guides),
                                           C.POINTER(pt_denoise_params), P, P]
            L.pt_ctx_denoise.argtypes = [P, C.c_int32, C.c_int32, P, P, C.POINTER(pt_denoise_guides),
                                         C.POINTER(pt_denoise_params), P, P, C.c_int, C.POINTER(pt_denoise_stats)]
            L.pt_ctx_render_denoised.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params), C.POINTER(pt_adaptive),
                                                 C.POINTER(pt_denoise_params), P, P, P, C.c_int,
                                                 C.POINTER(pt_adaptive_stats), C.POINTER(pt_denoised_stats)]
        if hasattr(L, "pt_ctx_temporal"):  # absent from older builds used in A/B runs
            L.pt_image_temporal.argtypes = [C.c_int32, C.c_int32, C.POINTER(pt_camera), C.POINTER(pt_camera), P, P,
                                            C.POINTER(pt_denoise_guides), C.POINTER(pt_temporal_history),
                                            C.POINTER(pt_temporal_history), C.POINTER(pt_temporal_params),
                                            C.POINTER(C.c_int64)]
            L.pt_ctx_temporal.argtypes = [P, C.c_int32, C.c_int32, C.POINTER(pt_camera), C.POINTER(pt_camera), P, P,
                                          C.POINTER(pt_denoise_guides), C.POINTER(pt_temporal_history),
                                          C.POINTER(pt_temporal_history), C.POINTER(pt_temporal_params), C.c_int,
                                          C.POINTER(pt_temporal_stats)]
            L.pt_ctx_render_temporal.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params),
                                                 C.POINTER(pt_temporal_params), C.POINTER(pt_denoise_params), C.c_int,
                                                 P, P, C.c_int, C.POINTER(pt_render_temporal_stats)]
        if hasattr(L, "pt_ctx_trace_nee"):  # absent from older builds used in A/B runs
            L.pt_scene_lights.argtypes = [C.POINTER(pt_scene), P, P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_float)]
            L.pt_bvh_trace_nee.argtypes = [C.POINTER(pt_scene), P, P, C.c_int64, C.POINTER(pt_trace_params), P,
                                           C.POINTER(pt_nee_stats)]
            L.pt_ctx_trace_nee.argtypes = [P, P, P, C.c_int64, C.POINTER(pt_trace_params), P, C.c_int,
                                           C.POINTER(pt_nee_stats)]
            L.pt_ctx_render_nee.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params), P, C.POINTER(pt_moments),
                                            C.c_int, C.POINTER(pt_nee_stats)]
        if hasattr(L, "pt_ctx_trace_nee_opt"):  # absent from older builds used in A/B runs
            L.pt_bvh_trace_nee_opt.argtypes = L.pt_bvh_trace_nee.argtypes + [C.POINTER(pt_nee_options)]
            L.pt_ctx_trace_nee_opt.argtypes = L.pt_ctx_trace_nee.argtypes + [C.POINTER(pt_nee_options)]
            L.pt_ctx_render_nee_opt.argtypes = L.pt_ctx_render_nee.argtypes + [C.POINTER(pt_nee_options)]
        if hasattr(L, "pt_ctx_trace_nee_grad"):  # absent from older builds used in A/B runs
            L.pt_bvh_trace_nee_grad.argtypes = [C.POINTER(pt_scene), P, P, C.c_int64, C.POINTER(pt_trace_params),
                                                C.POINTER(pt_trace_grad_io), C.POINTER(pt_nee_grad_stats),
                                                C.POINTER(pt_nee_options)]
            L.pt_ctx_trace_nee_grad.argtypes = [P, P, P, C.c_int64, C.POINTER(pt_trace_params), C.POINTER(pt_trace_grad_io),
                                                C.c_int, C.POINTER(pt_nee_grad_stats), C.POINTER(pt_nee_options)]
        if hasattr(L, "pt_ctx_render_grad"):  # absent from older builds used in A/B runs
            L.pt_bvh_render_grad.argtypes = [C.POINTER(pt_scene), C.POINTER(pt_camera), C.POINTER(pt_params),
                                             C.POINTER(pt_trace_grad_io), C.POINTER(pt_grad_stats)]
            L.pt_bvh_render_nee_grad.argtypes = [C.POINTER(pt_scene), C.POINTER(pt_camera), C.POINTER(pt_params),
                                                 C.POINTER(pt_trace_grad_io), C.POINTER(pt_nee_grad_stats),
                                                 C.POINTER(pt_nee_options)]
            L.pt_ctx_render_grad.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params), C.POINTER(pt_trace_grad_io),
                                             C.c_int, C.POINTER(pt_grad_stats)]
            L.pt_ctx_render_nee_grad.argtypes = [P, C.POINTER(pt_camera), C.POINTER(pt_params), C.POINTER(pt_trace_grad_io),
                                                 C.c_int, C.POINTER(pt_nee_grad_stats), C.POINTER(pt_nee_options)]
            L.pt_debug_host_camera_rays.argtypes = [C.POINTER(pt_camera), C.POINTER(pt_params), C.c_int32, C.c_int64,
                                                    C.c_int64, P, P, P]
        if hasattr(L, "pt_debug_rccl_failover"):  # test hooks (absent from older builds used in A/B runs)
            L.pt_debug_rccl_failover.argtypes = [C.c_int32, C.c_int32, P]
        if hasattr(L, "pt_debug_rtc_cache"):
            L.pt_debug_rtc_cache.argtypes = [C.c_int32]
            L.pt_debug_rtc_cache.restype = C.c_int64
        if hasattr(L, "pt_devices_release"):
            L.pt_devices_release.argtypes = []
            L.pt_devices_release.restype = None
        if hasattr(L, "pt_debug_ctx_flags"):
            L.pt_debug_ctx_flags.argtypes = [P, P]
        if hasattr(L, "pt_debug_ctx_plan"):
            L.pt_debug_ctx_plan.argtypes = [P, P]
        if hasattr(L, "pt_debug_walk_placement"):
            L.pt_debug_walk_placement.argtypes = [C.c_int32] * 5 + [C.c_uint64, P]
        if hasattr(L, "pt_debug_scene_dark"):
            L.pt_debug_scene_dark.argtypes = [C.POINTER(pt_scene)]
        if hasattr(L, "pt_debug_pack_hash"):
            L.pt_debug_pack_hash.argtypes = [C.POINTER(pt_scene), C.POINTER(C.c_uint64)]
        if hasattr(L, "pt_debug_rtc_start"):
            L.pt_debug_rtc_start.argtypes = [C.POINTER(pt_scene)]
        if hasattr(L, "pt_debug_emit_reject"):  # absent from older builds used in A/B runs
            L.pt_debug_emit_reject.argtypes = [P, P, P, C.c_int64, P]
            L.pt_debug_emit_box.argtypes = [C.POINTER(pt_scene), P]
            L.pt_debug_ctx_emit_reject.argtypes = [P, P, P, P]
        if hasattr(L, "pt_debug_emit_slab_reject"):
            L.pt_debug_emit_slab_reject.argtypes = [P, P, P, C.c_int64, P]
        if hasattr(L, "pt_debug_counter"):
            L.pt_debug_counter.argtypes = [C.c_int32]
            L.pt_debug_counter.restype = C.c_int64
        if L.pt_abi_version() != 3:
            raise RuntimeError("libpt_hip.so ABI version mismatch")
        _lib = L
    return _lib


def check(rc: int) -> int:
    if rc < 0:
        raise PTError(rc, lib().pt_last_error().decode(errors="replace"))
    return rc
