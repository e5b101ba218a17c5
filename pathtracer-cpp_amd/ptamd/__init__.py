"""ptamd — Python host layer over libpt_hip.so, mirroring the reference's C++ API.

Reference interface (Blackgaurd/pathtracer-cpp, pathtracer/):
  Material(type, color, emit_color, roughness)     material.h:27-52
  Triangle(v1, v2, v3, material)                   triangle.h:7-23
  BVH.add_triangle / size / empty / build          bvh.h:30-155
  Camera(pos, forward, up, res, fov, distance)     camera.h:33-61
  render_cpu(camera, bvh, samples, depth, file)    render.h:62-104
  render_gpu(camera, bvh, samples, depth, chunk, file) render.h:109-152

Both render entry points run the gfx950 trace kernel (the reference's CPU loop
and its GL tile loop are the path being replaced); they keep the reference's
argument meaning, messages and bool/exception behaviour. `render()` returns the
linear image (the mean after /spp, before gamma) for programmatic use.
"""
from __future__ import annotations

import array
import ctypes as C
import itertools
import math
import operator
import os
import sys
import time
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import PT_TEMPORAL_VAR_SAMPLE, PT_TEMPORAL_VAR_TEMPORAL  # noqa: F401
from ._lib import PT_MAX_DEPTH, PT_SEED, PTError, build, check, lib  # noqa: F401
from . import scenes  # noqa: F401

EMIT, DIFFUSE, SPECULAR = 1, 2, 3

NODE_DTYPE = np.dtype([("lb", "<f4", 3), ("rt", "<f4", 3), ("left", "<i4"), ("right", "<i4"),
                       ("tri_start", "<i4"), ("tri_end", "<i4")])
# pt_material (include/pt_hip.h, material.h:27-37): 32 bytes, no padding
MATERIAL_DTYPE = np.dtype([("type", "<i4"), ("color", "<f4", 3), ("emit", "<f4", 3), ("roughness", "<f4")])
assert MATERIAL_DTYPE.itemsize == C.sizeof(_lib.pt_material)


def _f3(v) -> Tuple[float, float, float]:
    if isinstance(v, (int, float)):
        return (float(v),) * 3
    return tuple(float(c) for c in v)


@dataclass
class Material:
    type: int
    color: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    emit_color: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    roughness: float = 0.0
    EMIT = EMIT
    DIFFUSE = DIFFUSE
    SPECULAR = SPECULAR

    def __post_init__(self):
        self.color = _f3(self.color)
        self.emit_color = _f3(self.emit_color)
        self.roughness = float(self.roughness)


@dataclass
class Triangle:
    v1: Tuple[float, float, float]
    v2: Tuple[float, float, float]
    v3: Tuple[float, float, float]
    material: Material


def _rays(origins, directions) -> Tuple[np.ndarray, np.ndarray]:
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions must both be (n, 3)")
    return o, d


def _states(states, n: int, samples: int) -> Optional[np.ndarray]:
    if states is None:
        return None
    st = np.ascontiguousarray(states, dtype=np.uint32).reshape(-1)
    if st.shape[0] != n * samples:
        raise ValueError("states must hold n x samples uint32 values")
    return st


def _host_rays(origins, directions, depth: int, samples: int, seed: int, states):
    """The numpy arguments of a call along the caller's rays: (origins, directions, n, pt_trace_params,
    the states array the params point into)."""
    o, d = _rays(origins, directions)
    n = o.shape[0]
    st_arr = _states(states, n, samples)
    prm = _lib.pt_trace_params(depth, samples, seed, st_arr.ctypes.data if st_arr is not None else None)
    return o, d, n, prm, st_arr


def _is_tensor(x) -> bool:
    return hasattr(x, "data_ptr")


GRAD_WANT = ("rgb", "color", "emit")


def _own_device_tensors(device: int, *tensors) -> None:
    """The rule of the device-pointer paths that read tensors torch may still be writing
    (Renderer.denoise, moments_variance, render_denoised, aov(device=True)): every tensor is on
    the context's device, and the work queued on torch's current stream of that device is
    complete before the library's own stream (which does not order itself after torch's) touches
    them. The library synchronises its stream before it returns, so torch may use the results at once."""
    import torch
    for x in tensors:
        if x is not None and (not x.is_cuda or x.device.index != device):
            raise ValueError(f"tensors must be on the context's device cuda:{device}")
    torch.cuda.current_stream(device).synchronize()


def _grad_want(want) -> Tuple[str, ...]:
    want = tuple(want)
    for k in want:
        if k not in GRAD_WANT:
            raise ValueError(f"want: {k!r} is not one of {GRAD_WANT}")
    return want


def _grad_io_host(num_tris: int, n: int, grad_rgb, color, emit, want):
    """pt_trace_grad_io over numpy arrays: (io, results dict, arrays to keep alive)."""
    want = _grad_want(want)
    keep, res, io = [], {}, _lib.pt_trace_grad_io()
    for key, val, rows in (("color", color, num_tris), ("emit", emit, num_tris), ("grad_rgb", grad_rgb, n)):
        if val is None:
            continue
        a = np.ascontiguousarray(val, dtype=np.float32).reshape(-1)
        if a.shape[0] != 3 * rows:
            raise ValueError(f"{key} must hold {rows} x 3 values")
        keep.append(a)
        setattr(io, key, a.ctypes.data)
    if ("color" in want or "emit" in want) and grad_rgb is None:
        raise ValueError("grad_rgb is needed for the gradients")
    if "rgb" in want:
        res["rgb"] = np.empty((n, 3), dtype=np.float32)
        io.rgb_out = res["rgb"].ctypes.data
    for k in ("color", "emit"):
        if k in want:
            res[k] = np.empty((num_tris, 3), dtype=np.float64)
            setattr(io, "grad_" + k, res[k].ctypes.data)
    return io, res, keep


@dataclass
class BVH:
    """Scene container = the reference's BVH (bvh.h:30-37): triangles + built tree."""
    triangles: List[Triangle] = field(default_factory=list)
    built: bool = False
    nodes: Optional[np.ndarray] = None
    tri_idx: Optional[np.ndarray] = None

    def add_triangle(self, tri: Triangle) -> None:
        self.built = False
        self._packed = None
        self.triangles.append(tri)
        # the C ABI's fields appended as the triangle is added (the reference's Triangle
        # constructor works at add time too, triangle.h:14-23): build() and the scene upload
        # then view these buffers instead of converting ~10^5 Python objects (config 4: the
        # Python packing took longer than the builder itself)
        if self._inc is None:
            self._inc = (array.array("d"), array.array("d"), array.array("i"), [])
        vb, mb, tb, objs = self._inc
        if len(objs) == len(self.triangles) - 1:
            m = tri.material
            vb.extend(tri.v1)
            vb.extend(tri.v2)
            vb.extend(tri.v3)
            mb.extend(m.color)
            mb.extend(m.emit_color)
            mb.append(m.roughness)
            tb.append(m.type)
            objs.append(tri)

    def size(self) -> int:
        return len(self.triangles)

    def empty(self) -> bool:
        return not self.triangles

    # packed arrays in the C ABI layout, made once per triangle list (build() and every
    # renderer's scene upload share them; add_triangle drops them)
    _packed: Optional[tuple] = field(default=None, init=False, repr=False, compare=False)
    # add_triangle's buffers: (vertices as doubles, color / emit / roughness as doubles,
    # material types, the triangles they were taken from)
    _inc: Optional[tuple] = field(default=None, init=False, repr=False, compare=False)

    def _pack(self) -> tuple:
        if self._packed is None or self._packed[0] != len(self.triangles):
            inc = self._inc
            if inc is not None and len(inc[3]) == len(self.triangles) and \
                    all(map(operator.is_, inc[3], self.triangles)):  # nothing replaced behind add_triangle
                self._packed = (len(self.triangles), self._verts_inc(), self._materials_inc())
            else:
                self._packed = (len(self.triangles), self._verts(), self._materials())
        return self._packed

    def _verts_inc(self) -> np.ndarray:
        v = np.frombuffer(self._inc[0], dtype=np.float64)
        return np.ascontiguousarray(v.astype(np.float32).reshape(-1, 9))

    def _materials_inc(self):
        n = len(self.triangles)
        vals = np.frombuffer(self._inc[1], dtype=np.float64).reshape(n, 7).astype(np.float32)
        arr = np.zeros(max(n, 1), dtype=MATERIAL_DTYPE)
        if n:
            arr["type"] = np.frombuffer(self._inc[2], dtype=np.int32)
            arr["color"] = vals[:, 0:3]
            arr["emit"] = vals[:, 3:6]
            arr["roughness"] = vals[:, 6]
        m = (_lib.pt_material * max(n, 1)).from_buffer(arr)
        m._keep = arr
        return m

    def verts(self) -> np.ndarray:
        return self._pack()[1]

    def materials(self):
        return self._pack()[2]

    def _verts(self) -> np.ndarray:
        # doubles rounded to float once, as the reference's vec3 constructor does
        n = len(self.triangles)
        v = np.fromiter(itertools.chain.from_iterable((*t.v1, *t.v2, *t.v3) for t in self.triangles),
                        dtype=np.float64, count=9 * n)
        return np.ascontiguousarray(v.astype(np.float32).reshape(-1, 9))

    def _materials(self):
        """pt_material per triangle: a ctypes array over a numpy buffer, filled column by
        column (each float rounded once to float32, as the reference's fields hold it)."""
        n = len(self.triangles)
        ms = [t.material for t in self.triangles]
        vals = np.fromiter(itertools.chain.from_iterable((*m.color, *m.emit_color, m.roughness) for m in ms),
                           dtype=np.float64, count=7 * n).reshape(n, 7).astype(np.float32)
        arr = np.zeros(max(n, 1), dtype=MATERIAL_DTYPE)
        if n:
            arr["type"] = np.fromiter((m.type for m in ms), dtype=np.int32, count=n)
            arr["color"] = vals[:, 0:3]
            arr["emit"] = vals[:, 3:6]
            arr["roughness"] = vals[:, 6]
        m = (_lib.pt_material * max(n, 1)).from_buffer(arr)
        m._keep = arr  # the ctypes array views arr's memory
        return m

    def build(self) -> None:
        """BVH::build (bvh.h:79-155), bit-identical output, O(n log^2 n)."""
        if self.built:
            return
        n = len(self.triangles)
        if n == 0:
            raise PTError(_lib.PT_E_EMPTY, "No triangles in scene.")
        verts = self.verts()
        nodes = np.zeros(2 * n - 1, dtype=NODE_DTYPE)
        idx = np.zeros(n, dtype=np.int32)
        cnt = check(lib().pt_bvh_build(n, verts.ctypes.data, nodes.ctypes.data, idx.ctypes.data))
        self.nodes, self.tri_idx, self.built = nodes[:cnt].copy(), idx, True

    def load_obj(self, filename: str, mtl_path: str = "./") -> None:
        """BVH::load_obj (bvh.h:184-242): the OBJ's triangles (tinyobjloader's parsing and
        triangulation, restated in csrc/pt_obj.cpp) with the bvh.h:220-238 material
        mapping, appended in file order. Raises PTError where the reference throws
        (unreadable file, malformed face) and where it has undefined behaviour (a face
        without a material, a vertex index past the end)."""
        h = C.c_void_p()
        check(lib().pt_obj_load(filename.encode(), mtl_path.encode(), C.byref(h)))
        try:
            warn = lib().pt_obj_warnings(h).decode(errors="replace")
            n = lib().pt_obj_num_tris(h)
            verts = np.empty((n, 9), dtype=np.float32)
            mats = (_lib.pt_material * max(n, 1))()
            illum = np.empty(n, dtype=np.int32)
            check(lib().pt_obj_triangles(h, verts.ctypes.data, C.addressof(mats), illum.ctypes.data))
        finally:
            lib().pt_obj_free(h)
        if warn:
            print("TinyObjLoader: " + warn, file=sys.stderr)
        v = verts.astype(np.float64).tolist()
        for i in range(n):
            if illum[i] not in (1, 2):
                print(f"Unknown material type with illum: {illum[i]}\nUsing default material: Diffuse(0.5)",
                      file=sys.stderr)
            m = mats[i]
            self.add_triangle(Triangle(tuple(v[i][0:3]), tuple(v[i][3:6]), tuple(v[i][6:9]),
                                       Material(m.type, tuple(m.color), tuple(m.emit), m.roughness)))

    def intersect(self, origins, directions):
        """BVH::intersect (bvh.h:156-183) for a batch of rays on the host (pt_bvh_intersect; no
        device needed): origins and directions (n, 3) float32 -> (t (n,) float32, tri (n,) int32),
        tri = index into `triangles` or -1, t = 1e30 for a miss."""
        ref = _SceneRef(self)
        o, d = _rays(origins, directions)
        t = np.empty(o.shape[0], dtype=np.float32)
        tri = np.empty(o.shape[0], dtype=np.int32)
        check(lib().pt_bvh_intersect(C.byref(ref.s), o.ctypes.data, d.ctypes.data, o.shape[0], t.ctypes.data,
                                     tri.ctypes.data))
        return t, tri

    def trace(self, origins, directions, depth: int, samples: int = 1, seed: int = PT_SEED, states=None):
        """trace() (render.h:36-61) along a batch of rays on the host (pt_bvh_trace; no device
        needed), bit-identical to Renderer.trace: origins and directions (n, 3) float32 ->
        (rgb (n, 3) float32, stats). rgb[i] is the float32 sum of `samples` paths of ray i in
        order, divided by `samples`; sample s of ray i starts the LCG at states[i, s] (uint32,
        (n, samples)) or, with states None, at pt_sample_seed(i, s, seed)."""
        return self._trace_host(lib().pt_bvh_trace, _lib.pt_trace_stats, origins, directions, depth, samples, seed, states)

    def trace_nee(self, origins, directions, depth: int, samples: int = 1, seed: int = PT_SEED, states=None,
                  mis: bool = False):
        """The light-sampling estimator (include/pt_hip.h: next-event estimation, the same expected
        value as trace() at every depth) along a batch of rays on the host (pt_bvh_trace_nee; no
        device needed), bit-identical to Renderer.trace_nee. Arguments and result as trace(); the
        stats also count shadow_rays and light_draws (rays = path and shadow segments together).
        `mis`: the weighted estimator (PT_NEE_MIS_BALANCE, pt_bvh_trace_nee_opt): the same draws and
        counts, with the light sample and the BRDF sample's EMIT hit combined by the balance heuristic."""
        return self._trace_host(_nee_call("pt_bvh_trace_nee", mis), _lib.pt_nee_stats, origins, directions, depth, samples,
                                seed, states)

    def _trace_host(self, fn, stats_type, origins, directions, depth, samples, seed, states):
        ref = _SceneRef(self)
        o, d, n, prm, _keep = _host_rays(origins, directions, depth, samples, seed, states)
        rgb = np.empty((n, 3), dtype=np.float32)
        st = stats_type()
        check(fn(C.byref(ref.s), o.ctypes.data, d.ctypes.data, n, C.byref(prm), rgb.ctypes.data, C.byref(st)))
        return rgb, st.as_dict()

    def trace_grad(self, origins, directions, grad_rgb, depth: int, samples: int = 1, seed: int = PT_SEED, states=None,
                   color=None, emit=None, want=GRAD_WANT):
        """Renderer.trace_grad on the host (pt_bvh_trace_grad; no device needed): the same
        per-path terms, summed in double in (ray, sample, bounce) order."""
        ref = _SceneRef(self)
        o, d, n, prm, _st = _host_rays(origins, directions, depth, samples, seed, states)
        io, res, _keep = _grad_io_host(len(self.triangles), n, grad_rgb, color, emit, want)
        st = _lib.pt_grad_stats()
        check(lib().pt_bvh_trace_grad(C.byref(ref.s), o.ctypes.data, d.ctypes.data, n, C.byref(prm), C.byref(io),
                                      C.byref(st)))
        return res, st.as_dict()

    def trace_nee_grad(self, origins, directions, grad_rgb, depth: int, samples: int = 1, seed: int = PT_SEED,
                       states=None, color=None, emit=None, want=GRAD_WANT, mis: bool = False):
        """Renderer.trace_nee_grad on the host (pt_bvh_trace_nee_grad; no device needed): the same
        per-path terms, summed in double in (ray, sample, bounce) order."""
        ref = _SceneRef(self)
        o, d, n, prm, _st = _host_rays(origins, directions, depth, samples, seed, states)
        io, res, _keep = _grad_io_host(len(self.triangles), n, grad_rgb, color, emit, want)
        st = _lib.pt_nee_grad_stats()
        check(lib().pt_bvh_trace_nee_grad(C.byref(ref.s), o.ctypes.data, d.ctypes.data, n, C.byref(prm), C.byref(io),
                                          C.byref(st), _nee_options(mis)))
        return res, st.as_dict()

    def render_grad(self, camera: "Camera", grad_img, samples: int, depth: int, seed: int = PT_SEED, color=None, emit=None,
                    want=GRAD_WANT, light_sampling: bool = False, mis: bool = False):
        """Renderer.render_grad on the host for the whole frame (pt_bvh_render_grad /
        pt_bvh_render_nee_grad; no device needed): the camera ray stated on the host, bit for bit the
        device's, and the same per-path terms, summed in double in (pixel, sample, bounce) order."""
        if mis and not light_sampling:
            raise ValueError("mis needs light_sampling")
        ref = _SceneRef(self)
        W, H = camera.res
        prm = _lib.pt_params(samples, depth, seed, 0, 1, 1, 0, 0)
        io, res, _keep = _grad_io_host(len(self.triangles), H * W, grad_img, color, emit, want)
        if light_sampling:
            st = _lib.pt_nee_grad_stats()
            check(lib().pt_bvh_render_nee_grad(C.byref(ref.s), C.byref(camera.c), C.byref(prm), C.byref(io), C.byref(st),
                                               _nee_options(mis)))
        else:
            st = _lib.pt_grad_stats()
            check(lib().pt_bvh_render_grad(C.byref(ref.s), C.byref(camera.c), C.byref(prm), C.byref(io), C.byref(st)))
        if "rgb" in res:
            res["rgb"] = res["rgb"].reshape(H, W, 3)
        return res, st.as_dict()

    @classmethod
    def from_scene(cls, scene) -> "BVH":
        b = cls()
        for (a, bb, c), m in zip(scene.tris, scene.mats):
            b.add_triangle(Triangle(a, bb, c, Material(m.type, m.color, m.emit, m.roughness)))
        return b


class Camera:
    """Camera ctor arithmetic (camera.h:33-61) computed by pt_camera_init."""

    def __init__(self, pos, forward, up, res: Tuple[int, int], fov: float, distance: float = 1.0):
        self.pos, self.forward, self.up = _f3(pos), _f3(forward), _f3(up)
        self.res = (int(res[0]), int(res[1]))
        self.fov = float(np.float32(fov))
        self.distance = float(np.float32(distance))
        self.c = _lib.pt_camera()
        f = lambda v: np.array(v, dtype=np.float64).astype(np.float32)
        p, fw, u = f(self.pos), f(self.forward), f(self.up)
        check(lib().pt_camera_init(p.ctypes.data, fw.ctypes.data, u.ctypes.data, self.res[0], self.res[1],
                                   C.c_float(self.fov), C.c_float(self.distance), C.byref(self.c)))

    @classmethod
    def from_spec(cls, spec) -> "Camera":
        return cls(spec.pos, spec.forward, spec.up, spec.res, spec.fov, spec.distance)


class _SceneRef:
    """Keeps the numpy/ctypes arrays alive while a pt_scene points into them."""

    def __init__(self, bvh: BVH):
        if bvh.empty():
            raise PTError(_lib.PT_E_EMPTY, "No triangles in scene.")
        if not bvh.built:
            bvh.build()
        self.verts = bvh.verts()
        self.mats = bvh.materials()
        self.nodes = np.ascontiguousarray(bvh.nodes)
        self.idx = np.ascontiguousarray(bvh.tri_idx, dtype=np.int32)
        self.s = _lib.pt_scene(len(bvh.triangles), self.verts.ctypes.data, C.addressof(self.mats),
                               self.nodes.shape[0], self.nodes.ctypes.data, self.idx.ctypes.data)


SCENE_INFO_KEYS = ("nodes", "tree_depth", "flat_leaves", "ref_stack", "wide_nodes", "wide_width", "wide_levels",
                   "wide_top", "wide_tris", "wide_record_bytes")


def _nee_call(name: str, mis: bool):
    """The light-sampling entry point `name`, or with `mis` its *_opt form bound to PT_NEE_MIS_BALANCE."""
    if not mis:
        return getattr(lib(), name)
    fn = getattr(lib(), name + "_opt")
    opt = _lib.pt_nee_options(_lib.PT_NEE_MIS_BALANCE, (0, 0, 0))
    return lambda *args: fn(*args, C.byref(opt))


def _nee_options(mis: bool):
    """The options argument of a light-sampling call: NULL, or with `mis` PT_NEE_MIS_BALANCE by reference."""
    return C.byref(_lib.pt_nee_options(_lib.PT_NEE_MIS_BALANCE, (0, 0, 0))) if mis else None


def scene_info(bvh: BVH) -> dict:
    """How the kernels will traverse `bvh` (pt_scene_info; no device needed)."""
    ref = _SceneRef(bvh)
    info = np.zeros(len(SCENE_INFO_KEYS), dtype=np.int32)
    check(lib().pt_scene_info(C.byref(ref.s), info.ctypes.data, len(info)))
    return dict(zip(SCENE_INFO_KEYS, info.tolist()))


def scene_lights(bvh: BVH) -> dict:
    """The light table of `bvh` as the light-sampling estimator reads it (pt_scene_lights; no device
    needed): {"tri": the lights' indices into `triangles` (int32), "cdf": the running float32 sum
    of their areas, "area": its last entry (0.0 without lights)}."""
    ref = _SceneRef(bvh)
    n = len(bvh.triangles)
    tri = np.empty(n, dtype=np.int32)
    cdf = np.empty(n, dtype=np.float32)
    count, area = C.c_int64(0), C.c_float(0.0)
    check(lib().pt_scene_lights(C.byref(ref.s), tri.ctypes.data, cdf.ctypes.data, n, C.byref(count), C.byref(area)))
    return {"tri": tri[:count.value].copy(), "cdf": cdf[:count.value].copy(), "area": np.float32(area.value)}


class Renderer:
    """A device context (pt_ctx): scene resident in HBM, repeated renders."""

    def __init__(self, device: int = 0):
        self.device = device
        h = C.c_void_p()
        check(lib().pt_ctx_create(device, C.byref(h)))
        self.h = h
        self.num_tris = 0  # triangles of the scene set_scene uploaded (trace_grad's override / gradient rows)
        self._mom_pixels = 0  # pixels of the part the running moments sum covers (unconverged's mask)

    def close(self) -> None:
        if getattr(self, "h", None):
            lib().pt_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def flags(self) -> dict:
        """How this context renders its scene (test hook pt_debug_ctx_flags)."""
        out = (C.c_int32 * 5)()
        check(lib().pt_debug_ctx_flags(self.h, out))
        d = {"albedo_x2": bool(out[0]), "specular": bool(out[1]), "rtc": bool(out[2]), "wide_nodes": out[3],
             "dark": bool(out[4])}
        if hasattr(lib(), "pt_debug_ctx_emit_reject"):  # absent from older builds used in A/B runs
            on, box = C.c_int32(0), (C.c_float * 6)()
            check(lib().pt_debug_ctx_emit_reject(self.h, C.byref(on), box, None))
            d["emit_reject"] = bool(on.value)
            d["emit_box"] = list(box)
        return d

    def early_ends(self) -> int:
        """Paths the last-ray rule ended in this context's last render (test hook; counted by the
        offline kernels, and by the hipRTC scene kernel under PT_RTC_DEFINES=PT_COUNT_EARLY=1)."""
        n = C.c_uint64(0)
        check(lib().pt_debug_ctx_emit_reject(self.h, None, None, C.byref(n)))
        return n.value

    PLAN_KEYS = ("kernel_path", "flat", "wide", "pairs", "pair_queue", "lds_bytes", "lds_scene", "wide_rows",
                 "wide_queue", "wide_top", "blocks_per_cu", "batch", "per_item", "fused", "tail", "flags_pm",
                 "trace_launches", "regen_thresh", "theta_lanes", "grid", "chunk", "static_items", "acc_every",
                 "num_cus")

    def plan(self) -> dict:
        """The launch plan of this context's last render (test hook pt_debug_ctx_plan)."""
        out = (C.c_int64 * len(self.PLAN_KEYS))()
        check(lib().pt_debug_ctx_plan(self.h, out))
        return dict(zip(self.PLAN_KEYS, list(out)))

    def set_scene(self, bvh: BVH) -> None:
        ref = _SceneRef(bvh)
        check(lib().pt_ctx_set_scene(self.h, C.byref(ref.s)))
        self.num_tris = len(bvh.triangles)

    def prepare(self) -> None:
        """Wait for the scene's background hipRTC compile (pt_ctx_prepare)."""
        check(lib().pt_ctx_prepare(self.h))

    @staticmethod
    def part_rows(res_y: int, part_index: int, part_count: int, band_rows: int) -> int:
        return lib().pt_part_rows(res_y, part_index, part_count, band_rows)

    def render(self, camera: Camera, samples: int, depth: int, seed: int = PT_SEED, part_index: int = 0,
               part_count: int = 1, band_rows: int = 1, out=None, batch_spp: int = 0,
               samples_per_item: int = 0):
        """Render this part's rows. `out`: None (returns numpy), or a torch CUDA tensor
        (float32, rows*W*3 elements) written in place on this context's device."""
        W, H = camera.res
        rows = self.part_rows(H, part_index, part_count, band_rows)
        prm = _lib.pt_params(samples, depth, seed, part_index, part_count, band_rows, batch_spp, samples_per_item)
        st = _lib.pt_stats()
        if out is None:
            img = np.empty((rows, W, 3), dtype=np.float32)
            check(lib().pt_ctx_render(self.h, C.byref(camera.c), C.byref(prm), img.ctypes.data, 0, C.byref(st)))
            return img, st.as_dict()
        if out.numel() != rows * W * 3 or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor with rows*W*3 elements")
        check(lib().pt_ctx_render(self.h, C.byref(camera.c), C.byref(prm), C.c_void_p(out.data_ptr()), 1,
                                  C.byref(st)))
        return out, st.as_dict()

    def render_progressive(self, camera: Camera, s_first: int, s_count: int, depth: int, seed: int = PT_SEED,
                           part_index: int = 0, part_count: int = 1, band_rows: int = 1, out=None,
                           batch_spp: int = 0, samples_per_item: int = 0):
        """Frame accumulation (render_realtime, render.h:219-387, offscreen): adds samples
        [s_first, s_first + s_count) to this context's running sum and returns the running
        mean, bit-identical to render() with s_first + s_count samples. s_first = 0 starts
        a new sum; otherwise it must continue the last one (same camera, depth, seed and
        partition) or PTError is raised. Any other render on this context ends the sum."""
        W, H = camera.res
        rows = self.part_rows(H, part_index, part_count, band_rows)
        prm = _lib.pt_params(s_first + s_count, depth, seed, part_index, part_count, band_rows, batch_spp,
                             samples_per_item)
        st = _lib.pt_stats()
        if out is None:
            img = np.empty((rows, W, 3), dtype=np.float32)
            check(lib().pt_ctx_render_progressive(self.h, C.byref(camera.c), C.byref(prm), s_first, s_count,
                                                  img.ctypes.data, 0, C.byref(st)))
            return img, st.as_dict()
        if out.numel() != rows * W * 3 or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor with rows*W*3 elements")
        check(lib().pt_ctx_render_progressive(self.h, C.byref(camera.c), C.byref(prm), s_first, s_count,
                                              C.c_void_p(out.data_ptr()), 1, C.byref(st)))
        return out, st.as_dict()

    def _moments_io(self, rows: int, W: int, want, out):
        """The image and the wanted moments of a part as (img, moments dict, image pointer,
        pt_moments, is_device): numpy arrays, or with `out` a torch tensor (float32, rows*W*3
        elements, on this context's device) tensors beside it."""
        want = tuple(want)
        for k in want:
            if k not in _lib.pt_moments.NAMES:
                raise ValueError(f"want: {k!r} is not one of {_lib.pt_moments.NAMES}")
        mom, res = _lib.pt_moments(), {}
        if out is None:
            img = np.empty((rows, W, 3), dtype=np.float32)
            for k in want:
                res[k] = np.empty((rows, W, 3), dtype=np.float32 if k == "sem" else np.float64)
                setattr(mom, k, res[k].ctypes.data)
            return img, res, C.c_void_p(img.ctypes.data), mom, 0
        import torch
        if not _is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or out.numel() != rows * W * 3 \
                or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor with rows*W*3 elements on the context's device")
        for k in want:
            res[k] = torch.empty((rows, W, 3), dtype=torch.float32 if k == "sem" else torch.float64, device=out.device)
            setattr(mom, k, res[k].data_ptr())
        return out, res, C.c_void_p(out.data_ptr()), mom, 1

    def render_moments(self, camera: Camera, s_first: int, s_count: int, depth: int, seed: int = PT_SEED,
                       part_index: int = 0, part_count: int = 1, band_rows: int = 1, out=None,
                       batch_spp: int = 0, samples_per_item: int = 0, want: Sequence[str] = _lib.pt_moments.NAMES):
        """render_progressive that also keeps the per-pixel sample moments (pt_ctx_render_moments):
        adds samples [s_first, s_first + s_count) to this context's running moments sum and
        returns (img, moments, stats). img is the running mean, bit-identical to render() with
        s_first + s_count samples; moments holds the entries of `want`, each (rows, W, 3):
        "sum" and "sumsq" (float64: the sums of the float32 samples and of their squares, added
        in sample order) and "sem" (float32: the standard error of the mean, +inf below two
        samples). s_first = 0 starts a sum; otherwise it must continue the last moments sum (same
        camera, depth, seed and partition; a render_progressive sum cannot be continued here, nor
        the other way round) or PTError is raised. `out`: None (numpy results) or a torch float32
        tensor on this context's device, written in place; the moments are then tensors there."""
        W, H = camera.res
        rows = self.part_rows(H, part_index, part_count, band_rows)
        prm = _lib.pt_params(s_first + s_count, depth, seed, part_index, part_count, band_rows, batch_spp,
                             samples_per_item)
        img, res, img_ptr, mom, dev = self._moments_io(rows, W, want, out)
        st = _lib.pt_stats()
        check(lib().pt_ctx_render_moments(self.h, C.byref(camera.c), C.byref(prm), s_first, s_count, img_ptr,
                                          C.byref(mom), dev, C.byref(st)))
        self._mom_pixels = rows * W
        return img, res, st.as_dict()

    def unconverged(self, rel: float, abs: float = 0.0, mask: bool = False):
        """Pixels of this context's running moments sum that miss the noise target
        sem <= rel * |mean| + abs in some channel (pt_ctx_unconverged; PTError without a moments
        sum): the count, or with mask=True (count, uint8 array of the part's pixels, 1 =
        unconverged). Equal to moments_unconverged() on the same sums."""
        n = C.c_int64(0)
        m = np.empty(self._mom_pixels, dtype=np.uint8) if mask else None
        check(lib().pt_ctx_unconverged(self.h, C.c_float(rel), C.c_float(abs), C.byref(n),
                                       m.ctypes.data if mask else None, 0))
        return (n.value, m) if mask else n.value

    def render_converge(self, camera: Camera, depth: int, rel: float, abs: float = 0.0, min_samples: int = 16,
                        max_samples: int = 4096, step: int = 0, max_unconverged: int = 0, seed: int = PT_SEED,
                        part_index: int = 0, part_count: int = 1, band_rows: int = 1, out=None, batch_spp: int = 0,
                        samples_per_item: int = 0, want: Sequence[str] = _lib.pt_moments.NAMES):
        """Render to a noise target (pt_ctx_render_converge): rounds end at min_samples, then
        every `step` samples later (step = 0: at twice the samples), never past max_samples; the
        render stops at the first round end where at most max_unconverged pixels miss
        sem <= rel * |mean| + abs, or at max_samples. Returns (img, moments, info): img
        bit-identical to render() with info["spp"] samples, moments as render_moments, info =
        {"spp", "rounds", "unconverged", "rays", "kernel_ms", "reduce_ms", "total_ms"}. The
        moments sum stays valid: render_moments can continue it from info["spp"]. A pixel whose
        samples so far are all zero counts as converged; min_samples is the guard."""
        W, H = camera.res
        rows = self.part_rows(H, part_index, part_count, band_rows)
        prm = _lib.pt_params(0, depth, seed, part_index, part_count, band_rows, batch_spp, samples_per_item)
        cv = _lib.pt_converge(rel, abs, min_samples, max_samples, step, max_unconverged)
        img, res, img_ptr, mom, dev = self._moments_io(rows, W, want, out)
        cs = _lib.pt_converge_stats()
        check(lib().pt_ctx_render_converge(self.h, C.byref(camera.c), C.byref(prm), C.byref(cv), img_ptr,
                                           C.byref(mom), dev, C.byref(cs)))
        self._mom_pixels = rows * W
        return img, res, cs.as_dict()

    def render_adaptive(self, camera: Camera, depth: int, rel: float, abs: float = 0.0, min_samples: int = 16,
                        max_samples: int = 4096, step: int = 0, max_unconverged: int = 0, sparse_below: float = 0.0,
                        seed: int = PT_SEED, part_index: int = 0, part_count: int = 1, band_rows: int = 1, out=None,
                        want: Sequence[str] = _lib.pt_moments.NAMES):
        """render_converge that spends its later rounds only on the pixels that still miss the
        target (pt_ctx_render_adaptive). The round ends are render_converge's. At the first one
        where at most sparse_below * pixels (and more than max_unconverged) miss the target, those
        pixels become the active list and every other pixel is frozen with that sample count; from
        then on only listed pixels are sampled and evaluated, and one that meets the target leaves
        the list with the round's sample count. sparse_below = 0: the library's default for the
        scene's kernel; < 0: never (the call is render_converge); >= 1: from the first round end.
        Returns (img, moments, spp, info). spp (rows, W) int32 is each pixel's sample count n_p;
        a pixel of img holds the bits of render() with n_p samples, moments "sum" and "sumsq" are
        over its n_p samples and "sem" uses n_p. info = {"rounds", "dense_rounds", "max_spp",
        "sparse_launches", "unconverged", "samples" (the sum of n_p), "rays", "sparse_rays",
        "kernel_ms", "reduce_ms", "total_ms", "sparse_kernel_ms"}. After per-pixel rounds the context holds no running
        moments sum (unconverged() and a render_moments continuation raise PTError); without them
        the state is render_converge's. `out`: None (numpy results) or a torch float32 tensor on
        this context's device, written in place; moments and spp are then tensors there."""
        W, H = camera.res
        rows = self.part_rows(H, part_index, part_count, band_rows)
        img, res, img_ptr, mom, dev = self._moments_io(rows, W, want, out)
        if dev:
            import torch
            spp = torch.empty((rows, W), dtype=torch.int32, device=out.device)
            spp_ptr = C.c_void_p(spp.data_ptr())
        else:
            spp = np.empty((rows, W), dtype=np.int32)
            spp_ptr = C.c_void_p(spp.ctypes.data)
        prm = _lib.pt_params(0, depth, seed, part_index, part_count, band_rows, 0, 0)
        ad = _lib.pt_adaptive(_lib.pt_converge(rel, abs, min_samples, max_samples, step, max_unconverged), sparse_below)
        st = _lib.pt_adaptive_stats()
        check(lib().pt_ctx_render_adaptive(self.h, C.byref(camera.c), C.byref(prm), C.byref(ad), img_ptr, C.byref(mom),
                                           spp_ptr, dev, C.byref(st)))
        self._mom_pixels = rows * W
        return img, res, spp, st.as_dict()

    def render_rgb8(self, camera: Camera, samples: int, depth: int, gamma: float = 2.2, flip: bool = True,
                    seed: int = PT_SEED, part_index: int = 0, part_count: int = 1, band_rows: int = 1, out=None,
                    batch_spp: int = 0, samples_per_item: int = 0):
        """render() + gamma_correct + save_png quantisation on the device (render.h:97-100,
        image.h:41-55): uint8 (rows, W, 3), equal to to_rgb8(render(...)) for a whole image
        (flip=True: top row first). `out`: None (numpy) or a torch uint8 CUDA tensor."""
        W, H = camera.res
        rows = self.part_rows(H, part_index, part_count, band_rows)
        prm = _lib.pt_params(samples, depth, seed, part_index, part_count, band_rows, batch_spp, samples_per_item)
        st = _lib.pt_stats()
        if out is None:
            img = np.empty((rows, W, 3), dtype=np.uint8)
            check(lib().pt_ctx_render_rgb8(self.h, C.byref(camera.c), C.byref(prm), C.c_float(gamma), int(flip),
                                           img.ctypes.data, 0, C.byref(st)))
            return img, st.as_dict()
        if out.numel() != rows * W * 3 or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor with rows*W*3 elements")
        check(lib().pt_ctx_render_rgb8(self.h, C.byref(camera.c), C.byref(prm), C.c_float(gamma), int(flip),
                                       C.c_void_p(out.data_ptr()), 1, C.byref(st)))
        return out, st.as_dict()

    def intersect(self, origins, directions, any_hit: bool = False, tmax=None, out=None):
        """Closest hit or occlusion for a batch of rays on this context's scene (pt_ctx_intersect;
        the answer is BVH::intersect's, bvh.h:156-183). numpy (n, 3) float32 in: returns
        ((t, tri), stats), or (occluded, stats) with any_hit (int32 0 / 1: t < tmax, tmax (n,)
        or None = 1e30). Contiguous float32 torch tensors on this context's device go through
        the device-pointer path: `out` = (t, tri) tensors (float32, int32), or the int32
        `occluded` tensor with any_hit, written in place and returned. Tensors follow the rule of
        the device-pointer paths: on the context's device, and torch's current stream is waited for
        before they are read."""
        st = _lib.pt_query_stats()
        mode = _lib.PT_QUERY_ANY if any_hit else _lib.PT_QUERY_CLOSEST
        if _is_tensor(origins):
            n = origins.numel() // 3
            tens = [origins, directions] + ([tmax] if tmax is not None else [])
            if out is None:
                import torch
                tri = torch.empty(n, dtype=torch.int32, device=origins.device)
                out = tri if any_hit else (torch.empty(n, dtype=torch.float32, device=origins.device), tri)
            outs = [out] if any_hit else list(out)
            self._device_tensors([(origins, None), (directions, 3 * n)] + [(x, n) for x in tens[2:] + outs],
                                 "tensors must be contiguous 32-bit tensors on the context's device",
                                 "directions must hold n x 3 elements, tmax and the outputs n")
            ptrs = [C.c_void_p(x.data_ptr()) for x in tens + outs]
            check(lib().pt_ctx_intersect(self.h, ptrs[0], ptrs[1], n, mode, ptrs[2] if tmax is not None else None,
                                         None if any_hit else ptrs[-2], ptrs[-1], 1, C.byref(st)))
            return out, st.as_dict()
        o, d = _rays(origins, directions)
        n = o.shape[0]
        tm = None
        if tmax is not None:
            tm = np.ascontiguousarray(tmax, dtype=np.float32).reshape(-1)
            if tm.shape[0] != n:
                raise ValueError("tmax must hold one float per ray")
        t = np.empty(n, dtype=np.float32)
        res = np.empty(n, dtype=np.int32)
        check(lib().pt_ctx_intersect(self.h, o.ctypes.data, d.ctypes.data, n, mode,
                                     tm.ctypes.data if tm is not None else None,
                                     None if any_hit else t.ctypes.data, res.ctypes.data, 0, C.byref(st)))
        return (res if any_hit else (t, res)), st.as_dict()

    def trace(self, origins, directions, depth: int, samples: int = 1, seed: int = PT_SEED, states=None, out=None):
        """Radiance along a batch of the caller's rays on this context's scene (pt_ctx_trace;
        every path is trace()'s, render.h:36-61): (rgb (n, 3) float32, stats). rgb[i] is the
        float32 sum of `samples` paths of ray i in order, divided by `samples`; sample s of ray i
        starts the LCG at states[i, s] (uint32, n x samples) or, with states None, at
        pt_sample_seed(i, s, seed). numpy arrays go through host pointers. Contiguous torch
        tensors on this context's device (float32 rays, `states` of a 32-bit integer type) go
        through the device-pointer path: `out`, a float32 tensor of n x 3 elements, is written
        in place and returned, and the inputs are left untouched. Tensors follow the rule of the
        device-pointer paths: on the context's device, and torch's current stream is waited for
        before they are read."""
        return self._caller_rays(lib().pt_ctx_trace, _lib.pt_trace_stats, origins, directions, depth, samples, seed, states, out)

    def trace_nee(self, origins, directions, depth: int, samples: int = 1, seed: int = PT_SEED, states=None, out=None,
                  mis: bool = False):
        """The light-sampling estimator (include/pt_hip.h) along a batch of the caller's rays on
        this context's scene (pt_ctx_trace_nee): arguments, numpy and tensor paths as trace(),
        bit-identical to BVH.trace_nee. Tensors follow the rule of the device-pointer paths: on
        the context's device, and torch's current stream is waited for before they are read.
        `mis`: the weighted estimator (PT_NEE_MIS_BALANCE, pt_ctx_trace_nee_opt), as BVH.trace_nee's."""
        return self._caller_rays(_nee_call("pt_ctx_trace_nee", mis), _lib.pt_nee_stats, origins, directions, depth, samples,
                                 seed, states, out)

    def _device_tensors(self, items, message: str, count_message: Optional[str] = None, dtype=None) -> None:
        """The checks of a tensor path on (tensor, element count or None) pairs: each a contiguous
        CUDA tensor of a 32-bit type (or of `dtype`), else ValueError(message); each of its count,
        else ValueError(count_message or message); then the rule of `_own_device_tensors`."""
        for x, _ in items:
            if not _is_tensor(x) or not x.is_contiguous() or not x.is_cuda or \
                    (x.element_size() != 4 if dtype is None else x.dtype != dtype):
                raise ValueError(message)
        if any(cnt is not None and x.numel() != cnt for x, cnt in items):
            raise ValueError(count_message or message)
        _own_device_tensors(self.device, *(x for x, _ in items))

    def _caller_rays(self, fn, stats_type, origins, directions, depth, samples, seed, states, out):
        """pt_ctx_trace or pt_ctx_trace_nee (`fn`) along the caller's rays: the tensor path and the numpy path."""
        st = stats_type()
        if _is_tensor(origins):
            n = origins.numel() // 3
            if out is None:
                import torch
                out = torch.empty((n, 3), dtype=torch.float32, device=origins.device)
            self._device_tensors([(origins, None), (directions, 3 * n), (out, 3 * n)] +
                                 ([(states, n * samples)] if states is not None else []),
                                 "tensors must be contiguous 32-bit tensors on the context's device",
                                 "directions and out must hold n x 3 elements, states n x samples")
            prm = _lib.pt_trace_params(depth, samples, seed, states.data_ptr() if states is not None else None)
            check(fn(self.h, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()), n, C.byref(prm),
                     C.c_void_p(out.data_ptr()), 1, C.byref(st)))
            return out, st.as_dict()
        o, d, n, prm, _keep = _host_rays(origins, directions, depth, samples, seed, states)
        rgb = np.empty((n, 3), dtype=np.float32)
        check(fn(self.h, o.ctypes.data, d.ctypes.data, n, C.byref(prm), rgb.ctypes.data, 0, C.byref(st)))
        return rgb, st.as_dict()

    def render_nee(self, camera: Camera, samples: int, depth: int, seed: int = PT_SEED, part_index: int = 0,
                   part_count: int = 1, band_rows: int = 1, out=None, want: Sequence[str] = (), mis: bool = False):
        """Render this part's rows with the light-sampling estimator (pt_ctx_render_nee) along the
        render's own camera rays: (img, moments, stats). img is the float32 sum of `samples`
        samples per pixel in sample order, divided by `samples`; moments holds the entries of
        `want` ("sum", "sumsq", "sem", as render_moments defines them) over those samples. One
        shot: it cannot be continued, and it ends this context's running sum. `out`: None (numpy
        results) or a torch float32 tensor on this context's device, written in place; the moments
        are then tensors there. `mis`: the weighted estimator (PT_NEE_MIS_BALANCE,
        pt_ctx_render_nee_opt), as trace_nee's."""
        W, H = camera.res
        rows = self.part_rows(H, part_index, part_count, band_rows)
        prm = _lib.pt_params(samples, depth, seed, part_index, part_count, band_rows, 0, 0)
        img, res, img_ptr, mom, dev = self._moments_io(rows, W, want, out)
        if dev:
            _own_device_tensors(self.device, out)
        st = _lib.pt_nee_stats()
        check(_nee_call("pt_ctx_render_nee", mis)(self.h, C.byref(camera.c), C.byref(prm), img_ptr, C.byref(mom), dev, C.byref(st)))
        return img, res, st.as_dict()

    def trace_grad(self, origins, directions, grad_rgb, depth: int, samples: int = 1, seed: int = PT_SEED, states=None,
                   color=None, emit=None, want=GRAD_WANT):
        """Radiance of trace() along the caller's rays at (optionally) changed materials, and
        its exact gradient with respect to them (pt_ctx_trace_grad; the contract is in
        include/pt_hip.h). `color` / `emit`: (num_tris, 3) float32 albedo / emit_color to evaluate
        at, in the order of the BVH's triangles, None = the scene's (types and roughness always
        the scene's; the scene itself is not changed). `grad_rgb`: (n, 3) float32 dLoss/d rgb,
        needed for the gradients. Returns ({"rgb": (n, 3) float32, "color": (num_tris, 3)
        float64 = dLoss/d color, "emit": likewise} restricted to `want`, stats). Rays, samples,
        seed and states are trace()'s. numpy arrays go through host pointers; contiguous torch
        tensors on this context's device (every array argument then) through device pointers,
        the results are tensors there, and the inputs are left untouched. Tensors follow the rule
        of the device-pointer paths: on the context's device, and torch's current stream is waited
        for before they are read."""
        return self._trace_grad(lib().pt_ctx_trace_grad, _lib.pt_grad_stats(), origins, directions, grad_rgb, depth,
                                samples, seed, states, color, emit, want)

    def trace_nee_grad(self, origins, directions, grad_rgb, depth: int, samples: int = 1, seed: int = PT_SEED,
                       states=None, color=None, emit=None, want=GRAD_WANT, mis: bool = False):
        """trace_grad for the light-sampling estimator (pt_ctx_trace_nee_grad; the definition is in
        include/pt_hip.h): the radiance Renderer.trace_nee gives at (optionally) changed materials
        and its exact gradient with respect to them. Arguments, results, numpy and tensor paths are
        trace_grad's; `mis` is trace_nee's (the weights do not depend on the materials). The light
        table is always the scene's: an override changes a light's emission, never which
        triangles are lights. The stats add shadow_rays, light_draws, lights and light_area."""
        fn = lib().pt_ctx_trace_nee_grad
        return self._trace_grad(lambda *args: fn(*args, _nee_options(mis)), _lib.pt_nee_grad_stats(), origins, directions,
                                grad_rgb, depth, samples, seed, states, color, emit, want)

    def render_grad(self, camera: Camera, grad_img, samples: int, depth: int, seed: int = PT_SEED, part_index: int = 0,
                    part_count: int = 1, band_rows: int = 1, color=None, emit=None, want=GRAD_WANT,
                    light_sampling: bool = False, mis: bool = False):
        """The image render() (or, with `light_sampling`, render_nee(mis=mis)) gives for this part at
        (optionally) changed materials, and its exact gradient with respect to every triangle's
        color and emit_color (pt_ctx_render_grad / pt_ctx_render_nee_grad; the contract is in
        include/pt_hip.h): every sample of a pixel runs along its own jittered camera ray, in one
        call. `grad_img`: (rows, W, 3) float32 dLoss/d image in render()'s row order, needed for the
        gradients; `color` / `emit`, `want` and the results are trace_grad's, with "rgb" of shape
        (rows, W, 3). Without "rgb" in `want` no radiance is written (the backward pass of a fit).
        The gradients of the parts of a frame sum to the frame's. numpy arrays go through host
        pointers; contiguous float32 torch tensors on this context's device (every array argument
        then, at least one of them) through device pointers, under the rule of the device-pointer
        paths. Unlike render_nee the call leaves this context's running sum valid."""
        if mis and not light_sampling:
            raise ValueError("mis needs light_sampling")
        W, H = camera.res
        rows = self.part_rows(H, part_index, part_count, band_rows)
        n, T = rows * W, self.num_tris
        prm = _lib.pt_params(samples, depth, seed, part_index, part_count, band_rows, 0, 0)
        if light_sampling:
            st = _lib.pt_nee_grad_stats()
            call = lambda io, dev: lib().pt_ctx_render_nee_grad(self.h, C.byref(camera.c), C.byref(prm), C.byref(io), dev,
                                                                C.byref(st), _nee_options(mis))
        else:
            st = _lib.pt_grad_stats()
            call = lambda io, dev: lib().pt_ctx_render_grad(self.h, C.byref(camera.c), C.byref(prm), C.byref(io), dev,
                                                            C.byref(st))
        given = [x for x in (grad_img, color, emit) if x is not None]
        if any(_is_tensor(x) for x in given):
            import torch
            want = _grad_want(want)
            io, res, f32 = _lib.pt_trace_grad_io(), {}, []
            for key, val, cnt in (("color", color, 3 * T), ("emit", emit, 3 * T), ("grad_rgb", grad_img, 3 * n)):
                if val is not None:
                    f32.append((val, cnt))
                    if _is_tensor(val):
                        setattr(io, key, val.data_ptr())
            self._device_tensors(f32, "grad_img, color and emit must be contiguous float32 tensors of rows x W x 3 / "
                                 "num_tris x 3 elements on the context's device", dtype=torch.float32)
            if ("color" in want or "emit" in want) and grad_img is None:
                raise ValueError("grad_img is needed for the gradients")
            dev = torch.device("cuda", self.device)
            if "rgb" in want:
                res["rgb"] = torch.empty((rows, W, 3), dtype=torch.float32, device=dev)
                io.rgb_out = res["rgb"].data_ptr()
            for k in ("color", "emit"):
                if k in want:
                    res[k] = torch.empty((T, 3), dtype=torch.float64, device=dev)
                    setattr(io, "grad_" + k, res[k].data_ptr())
            check(call(io, 1))
            return res, st.as_dict()
        io, res, _keep = _grad_io_host(T, n, grad_img, color, emit, want)
        check(call(io, 0))
        if "rgb" in res:
            res["rgb"] = res["rgb"].reshape(rows, W, 3)
        return res, st.as_dict()

    def _trace_grad(self, fn, st, origins, directions, grad_rgb, depth, samples, seed, states, color, emit, want):
        """pt_ctx_trace_grad or pt_ctx_trace_nee_grad (`fn`, stats `st`): the tensor path and the numpy path."""
        if _is_tensor(origins):
            import torch
            want = _grad_want(want)
            n = origins.numel() // 3
            T = self.num_tris
            io, res = _lib.pt_trace_grad_io(), {}
            f32 = [(origins, 3 * n), (directions, 3 * n)]
            for key, val, cnt in (("color", color, 3 * T), ("emit", emit, 3 * T), ("grad_rgb", grad_rgb, 3 * n)):
                if val is not None:
                    f32.append((val, cnt))
                    setattr(io, key, val.data_ptr())
            self._device_tensors(f32, "rays, color, emit and grad_rgb must be contiguous float32 tensors of n x 3 / "
                                 "num_tris x 3 elements on the context's device", dtype=torch.float32)
            if states is not None:
                self._device_tensors([(states, n * samples)], "states must be a contiguous 32-bit tensor of n x samples "
                                     "elements on the context's device")
            if ("color" in want or "emit" in want) and grad_rgb is None:
                raise ValueError("grad_rgb is needed for the gradients")
            if "rgb" in want:
                res["rgb"] = torch.empty((n, 3), dtype=torch.float32, device=origins.device)
                io.rgb_out = res["rgb"].data_ptr()
            for k in ("color", "emit"):
                if k in want:
                    res[k] = torch.empty((T, 3), dtype=torch.float64, device=origins.device)
                    setattr(io, "grad_" + k, res[k].data_ptr())
            prm = _lib.pt_trace_params(depth, samples, seed, states.data_ptr() if states is not None else None)
            check(fn(self.h, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()), n, C.byref(prm), C.byref(io), 1,
                     C.byref(st)))
            return res, st.as_dict()
        o, d, n, prm, _st = _host_rays(origins, directions, depth, samples, seed, states)
        io, res, _keep = _grad_io_host(self.num_tris, n, grad_rgb, color, emit, want)
        check(fn(self.h, o.ctypes.data, d.ctypes.data, n, C.byref(prm), C.byref(io), 0, C.byref(st)))
        return res, st.as_dict()

    def aov(self, camera: Camera, sample: int = 0, seed: int = PT_SEED,
            channels: Sequence[str] = _lib.pt_aov.CHANNELS, part_index: int = 0, part_count: int = 1,
            band_rows: int = 1, device: bool = False):
        """First-hit channels of sample `sample` of this part's pixels (pt_ctx_render_aov): a
        dict of (rows, W) arrays for "t" (float32) and "tri" (int32), (rows, W, 3) for
        "normal", "albedo", "emission" and (rows, W, 6) for "ray" (o.xyz, d.xyz), rows in
        render()'s order, + stats. device=True: torch tensors on this context's device, written
        through device pointers."""
        W, H = camera.res
        rows = self.part_rows(H, part_index, part_count, band_rows)
        prm = _lib.pt_params(1, 1, seed, part_index, part_count, band_rows, 0, 0)
        res, aov = {}, _lib.pt_aov()
        if device:
            import torch
            dev = torch.device("cuda", self.device)
        for k in channels:
            w = _lib.pt_aov.WIDTH[k]  # KeyError: not a channel
            shape = (rows, W) if w == 1 else (rows, W, w)
            if device:
                res[k] = torch.empty(shape, dtype=torch.int32 if k == "tri" else torch.float32, device=dev)
                setattr(aov, k, res[k].data_ptr())
            else:
                res[k] = np.empty(shape, dtype=np.int32 if k == "tri" else np.float32)
                setattr(aov, k, res[k].ctypes.data)
        if device:
            _own_device_tensors(self.device)  # the fresh tensors' memory may belong to work torch still has queued
        st = _lib.pt_query_stats()
        check(lib().pt_ctx_render_aov(self.h, C.byref(camera.c), C.byref(prm), sample, C.byref(aov), int(device),
                                      C.byref(st)))
        return res, st.as_dict()

    def moments_variance(self, sum, sumsq, n: int = 0, spp=None):
        """moments_variance() by a kernel on this context's device (pt_ctx_moments_variance), the
        same bits. numpy arrays go through host pointers; contiguous torch tensors on this
        context's device (float64 sums, int32 spp) through device pointers, the result is a
        tensor there. The call first waits for the work queued on torch's current stream of the
        device (the tensors may come from torch operations still in flight)."""
        if _is_tensor(sum):
            import torch
            for x, dt in ((sum, torch.float64), (sumsq, torch.float64)) + (((spp, torch.int32),) if spp is not None else ()):
                if not _is_tensor(x) or not x.is_cuda or not x.is_contiguous() or x.dtype != dt:
                    raise ValueError("sum and sumsq must be contiguous float64 tensors, spp int32, on the context's device")
            npix = sum.numel() // 3
            if sum.numel() != 3 * npix or sumsq.numel() != 3 * npix or (spp is not None and spp.numel() != npix):
                raise ValueError("sum and sumsq must hold pixels x 3 elements, spp one per pixel")
            var = torch.empty(sum.shape, dtype=torch.float32, device=sum.device)
            _own_device_tensors(self.device, sum, sumsq, spp)
            check(lib().pt_ctx_moments_variance(self.h, C.c_void_p(sum.data_ptr()), C.c_void_p(sumsq.data_ptr()), npix, n,
                                                C.c_void_p(spp.data_ptr()) if spp is not None else None,
                                                C.c_void_p(var.data_ptr()), 1))
            return var
        S, Q, sp, npix = _variance_args(sum, sumsq, spp)
        var = np.empty(S.shape, dtype=np.float32)
        check(lib().pt_ctx_moments_variance(self.h, S.ctypes.data, Q.ctypes.data, npix, n,
                                            sp.ctypes.data if sp is not None else None, var.ctypes.data, 0))
        return var

    def denoise(self, color, guides, var=None, passes: int = 0, sigma_l: float = 0.0, sigma_z: float = 0.0,
                normal_pow_log2: int = 0, eps: float = 0.0, out=None, var_out=None):
        """denoise() on this context's device (pt_ctx_denoise), the same bits: (out, var_out or
        None, stats). numpy arrays go through host pointers. Contiguous torch tensors on this
        context's device (float32; guides["tri"] int32) go through device pointers: `out` (and
        `var_out`, only with var) are written in place and may be `color` (and `var`)
        themselves; without them new tensors are made (var_out whenever var is given). The
        library's stream does not order itself after torch's: the call first waits for the work
        queued on torch's current stream of the device, so guides from denoise_guides() or any
        other torch operation still in flight are complete when the filter reads them, and it
        returns after its own work is complete. With numpy arrays `out` and `var_out` must be
        None (ValueError). stats =
        {"kernel_ms", "total_ms", "passes", "launches", "form" (per pass "direct" or "lds"),
        "pass_ms", "pack_ms"}. Needs no scene and leaves a running sum as it is."""
        prm = _lib.pt_denoise_params(passes, sigma_l, sigma_z, normal_pow_log2, eps)
        st = _lib.pt_denoise_stats()
        if _is_tensor(color):
            import torch
            if color.dim() != 3 or color.shape[2] != 3:
                raise ValueError("color must have shape (H, W, 3)")
            H, W = color.shape[0], color.shape[1]
            if out is None:
                out = torch.empty_like(color)
            if var is not None and var_out is None:
                var_out = torch.empty_like(color)
            g = _lib.pt_denoise_guides()
            tens = [(color, 3, torch.float32), (out, 3, torch.float32)]
            tens += [(x, 3, torch.float32) for x in (var, var_out) if x is not None]
            for k in _lib.pt_denoise_guides.NAMES:
                x = guides[k]
                tens.append((x, _lib.pt_denoise_guides.WIDTH[k], torch.int32 if k == "tri" else torch.float32))
                setattr(g, k, x.data_ptr() if _is_tensor(x) else None)
            for x, w, dt in tens:
                if not _is_tensor(x) or not x.is_cuda or not x.is_contiguous() or x.dtype != dt or x.numel() != H * W * w:
                    raise ValueError("color, var, the guides and the outputs must be contiguous float32 (tri: int32) "
                                     "tensors of H*W*width elements on the context's device")
            _own_device_tensors(self.device, *[x for x, _, _ in tens])
            check(lib().pt_ctx_denoise(self.h, W, H, C.c_void_p(color.data_ptr()),
                                       C.c_void_p(var.data_ptr()) if var is not None else None, C.byref(g), C.byref(prm),
                                       C.c_void_p(out.data_ptr()),
                                       C.c_void_p(var_out.data_ptr()) if var_out is not None else None, 1, C.byref(st)))
            return out, var_out, st.as_dict()
        if out is not None or var_out is not None:
            raise ValueError("out and var_out are for torch tensors; numpy results are returned")
        W, H, c, v, g, _keep = _denoise_args(color, var, guides)
        res = np.empty((H, W, 3), dtype=np.float32)
        vres = np.empty((H, W, 3), dtype=np.float32) if v is not None else None
        check(lib().pt_ctx_denoise(self.h, W, H, c.ctypes.data, v.ctypes.data if v is not None else None, C.byref(g),
                                   C.byref(prm), res.ctypes.data, vres.ctypes.data if vres is not None else None, 0,
                                   C.byref(st)))
        return res, vres, st.as_dict()

    def render_denoised(self, camera: Camera, depth: int, rel: float, abs: float = 0.0, min_samples: int = 16,
                        max_samples: int = 4096, step: int = 0, max_unconverged: int = 0, sparse_below: float = 0.0,
                        seed: int = PT_SEED, part_count: int = 1, passes: int = 0, sigma_l: float = 0.0,
                        sigma_z: float = 0.0, normal_pow_log2: int = 0, eps: float = 0.0, out=None):
        """render_adaptive + the first-hit guides of sample 0 + the variance of the mean with each
        pixel's own sample count + denoise, all on the device (pt_ctx_render_denoised): (img,
        noisy, spp, info). img is bit-identical to making the four calls by hand, noisy and spp
        are render_adaptive's image and sample counts. info = render_adaptive's, with "denoise"
        (Renderer.denoise's stats), "aov_ms", "variance_ms" and the whole call's "total_ms". The
        whole image must be on this device: part_count > 1 raises PTError. `out`: None (numpy
        results) or a float32 torch tensor of H*W*3 elements on this context's device, written in
        place (after the work queued on torch's current stream of the device is complete); noisy
        and spp are then tensors there."""
        W, H = camera.res
        prm = _lib.pt_params(0, depth, seed, 0, part_count, 1, 0, 0)
        ad = _lib.pt_adaptive(_lib.pt_converge(rel, abs, min_samples, max_samples, step, max_unconverged), sparse_below)
        dp = _lib.pt_denoise_params(passes, sigma_l, sigma_z, normal_pow_log2, eps)
        rs, ds = _lib.pt_adaptive_stats(), _lib.pt_denoised_stats()
        if out is None:
            img = np.empty((H, W, 3), dtype=np.float32)
            noisy = np.empty((H, W, 3), dtype=np.float32)
            spp = np.empty((H, W), dtype=np.int32)
            ptrs, dev = (img.ctypes.data, noisy.ctypes.data, spp.ctypes.data), 0
        else:
            import torch
            if not _is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or out.numel() != H * W * 3 \
                    or not out.is_contiguous():
                raise ValueError("out must be a contiguous float32 tensor with H*W*3 elements on the context's device")
            img = out
            noisy = torch.empty((H, W, 3), dtype=torch.float32, device=out.device)
            spp = torch.empty((H, W), dtype=torch.int32, device=out.device)
            ptrs, dev = (img.data_ptr(), noisy.data_ptr(), spp.data_ptr()), 1
            _own_device_tensors(self.device, out)
        check(lib().pt_ctx_render_denoised(self.h, C.byref(camera.c), C.byref(prm), C.byref(ad), C.byref(dp),
                                           C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]), C.c_void_p(ptrs[2]), dev,
                                           C.byref(rs), C.byref(ds)))
        info = rs.as_dict()
        info["render_ms"] = info["total_ms"]
        info.update(denoise=ds.denoise.as_dict(), aov_ms=ds.aov_ms, variance_ms=ds.variance_ms, total_ms=ds.total_ms)
        return img, noisy, spp, info

    def temporal_accumulate(self, color, guides, camera: Camera, prev: Optional["TemporalHistory"] = None,
                            prev_camera: Optional[Camera] = None, var=None, max_history: int = 0, sigma_z: float = 0.0,
                            normal_min: float = 0.0, variance_mode: int = 0, out: Optional["TemporalHistory"] = None):
        """temporal_accumulate() on this context's device (pt_ctx_temporal), the same bits:
        (next, stats) with stats = {"kernel_ms", "total_ms", "reused"}. numpy arrays go through
        host pointers (`out` must then be None). Contiguous torch tensors on this context's device
        (float32; guides["tri"], hist and cls int32) go through device pointers: color, var, every
        guide and every plane of `prev` must then be such tensors (ValueError otherwise), `next` is
        `out` or a new TemporalHistory of tensors, and must not share memory with `prev`
        (PTError). The validation and the wait for torch's current stream are Renderer.denoise's.
        The inputs are left untouched. Needs no scene and leaves a running sum as it is."""
        prm = _lib.pt_temporal_params(max_history, sigma_z, normal_min, variance_mode)
        st = _lib.pt_temporal_stats()
        if prev is not None and prev_camera is None:
            raise ValueError("prev needs prev_camera")
        pc = C.byref(prev_camera.c) if prev is not None else None
        if _is_tensor(color):
            import torch
            if color.dim() != 3 or color.shape[2] != 3:
                raise ValueError("color must have shape (H, W, 3)")
            H, W = color.shape[0], color.shape[1]
            if out is None:
                out = TemporalHistory.empty(W, H, like=color)
            tens = [(color, 3, torch.float32)] + ([(var, 3, torch.float32)] if var is not None else [])
            g = _lib.pt_denoise_guides()
            for k in _lib.pt_denoise_guides.NAMES:
                x = guides[k]
                tens.append((x, _lib.pt_denoise_guides.WIDTH[k], torch.int32 if k == "tri" else torch.float32))
                setattr(g, k, x.data_ptr() if _is_tensor(x) else None)
            hs = []
            for h in (prev, out):
                s = _lib.pt_temporal_history()
                for k in _lib.pt_temporal_history.NAMES if h is not None else ():
                    x = getattr(h, k)
                    if x is None and h is prev and k == "var":
                        continue  # the library reports it when sample mode needs it
                    tens.append((x, _lib.pt_temporal_history.WIDTH[k],
                                 torch.int32 if k in _lib.pt_temporal_history.INT else torch.float32))
                    setattr(s, k, x.data_ptr() if _is_tensor(x) else None)
                hs.append(s)
            for x, w, dt in tens:
                if not _is_tensor(x) or not x.is_cuda or not x.is_contiguous() or x.dtype != dt or x.numel() != H * W * w:
                    raise ValueError("color, var, the guides and the histories' planes must be contiguous float32 "
                                     "(tri, hist, cls: int32) tensors of H*W*width elements on the context's device")
            _own_device_tensors(self.device, *[x for x, _, _ in tens])
            check(lib().pt_ctx_temporal(self.h, W, H, C.byref(camera.c), pc, C.c_void_p(color.data_ptr()),
                                        C.c_void_p(var.data_ptr()) if var is not None else None, C.byref(g),
                                        C.byref(hs[0]) if prev is not None else None, C.byref(hs[1]), C.byref(prm), 1,
                                        C.byref(st)))
            return out, st.as_dict()
        if out is not None:
            raise ValueError("out is for torch tensors; numpy results are returned")
        _no_tensors(color, var, guides)
        W, H, c, v, g, _keep = _denoise_args(color, var, guides)
        ps, _pkeep = _history_host(prev, W, H) if prev is not None else (None, None)
        nxt = TemporalHistory.empty(W, H)
        ns, _nkeep = _history_host(nxt, W, H)
        check(lib().pt_ctx_temporal(self.h, W, H, C.byref(camera.c), pc, c.ctypes.data,
                                    v.ctypes.data if v is not None else None, C.byref(g),
                                    C.byref(ps) if ps is not None else None, C.byref(ns), C.byref(prm), 0, C.byref(st)))
        return nxt, st.as_dict()

    def render_temporal(self, camera: Camera, spp: int, depth: int, seed: int = PT_SEED, reset: bool = False,
                        max_history: int = 0, temporal_sigma_z: float = 0.0, normal_min: float = 0.0, passes: int = 0,
                        sigma_l: float = 0.0, sigma_z: float = 0.0, normal_pow_log2: int = 0, eps: float = 0.0,
                        part_count: int = 1, out=None):
        """One frame of a camera path, all on the device (pt_ctx_render_temporal): render_moments
        of `spp` samples + the first-hit guides of sample 0 + the variance of the mean (spp >= 2;
        with spp = 1 the accumulated moments give it) + temporal_accumulate onto the history this
        context kept from its last render_temporal + denoise. Returns (img, accumulated, info):
        img is bit-identical to making the calls by hand, accumulated is the unfiltered
        accumulation (what the context keeps as history). Change `seed` from frame to frame.
        The history is dropped by reset=True, set_scene, another resolution or an error.
        info = {"total_ms", "render_ms", "aov_ms", "variance_ms", "rays", "had_history",
        "variance_mode", "reused", "temporal", "denoise"}. part_count > 1 raises PTError. `out`:
        None (numpy results) or a float32 torch tensor of H*W*3 elements on this context's device,
        written in place (after the work queued on torch's current stream of the device is
        complete); accumulated is then a tensor there."""
        W, H = camera.res
        prm = _lib.pt_params(spp, depth, seed, 0, part_count, 1, 0, 0)
        tp = _lib.pt_temporal_params(max_history, temporal_sigma_z, normal_min, 0)
        dp = _lib.pt_denoise_params(passes, sigma_l, sigma_z, normal_pow_log2, eps)
        st = _lib.pt_render_temporal_stats()
        if out is None:
            img = np.empty((H, W, 3), dtype=np.float32)
            acc = np.empty((H, W, 3), dtype=np.float32)
            ptrs, dev = (img.ctypes.data, acc.ctypes.data), 0
        else:
            import torch
            if not _is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or out.numel() != H * W * 3 \
                    or not out.is_contiguous():
                raise ValueError("out must be a contiguous float32 tensor with H*W*3 elements on the context's device")
            img = out
            acc = torch.empty((H, W, 3), dtype=torch.float32, device=out.device)
            ptrs, dev = (img.data_ptr(), acc.data_ptr()), 1
            _own_device_tensors(self.device, out)
        check(lib().pt_ctx_render_temporal(self.h, C.byref(camera.c), C.byref(prm), C.byref(tp), C.byref(dp), int(bool(reset)),
                                           C.c_void_p(ptrs[0]), C.c_void_p(ptrs[1]), dev, C.byref(st)))
        return img, acc, st.as_dict()


def render(camera: Camera, bvh: BVH, samples: int, depth: int, seed: int = PT_SEED, device: int = 0,
           devices: Optional[Sequence[int]] = None, band_rows: int = 1, **kw):
    """Linear image (H, W, 3) float32, h = 0 the bottom row (Image::pixels), + stats.
    `devices`: render on several GPUs of this process (pt_render_f32_devices: row bands
    dealt to the devices, one host thread each); the image does not depend on it."""
    if devices is not None:
        if not bvh.built:
            bvh.build()
        ref = _SceneRef(bvh)
        W, H = camera.res
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        prm = _lib.pt_params(samples, depth, seed, 0, len(dv), band_rows, kw.get("batch_spp", 0),
                             kw.get("samples_per_item", 0))
        img = np.empty((H, W, 3), dtype=np.float32)
        st = _lib.pt_stats()
        check(lib().pt_render_f32_devices(C.byref(ref.s), C.byref(camera.c), C.byref(prm), dv.ctypes.data,
                                          len(dv), img.ctypes.data, C.byref(st)))
        return img, st.as_dict()
    r = Renderer(device)
    try:
        r.set_scene(bvh)
        return r.render(camera, samples, depth, seed=seed, **kw)
    finally:
        r.close()


PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64)


def render_rgb8(camera: Camera, bvh: BVH, samples: int, depth: int, devices: Sequence[int], gamma: float = 2.2,
                seed: int = PT_SEED, band_rows: int = 1, progress=None, **kw):
    """render() on several GPUs of this process + gamma_correct / save_png quantisation on
    the first device after the RCCL gather (pt_render_rgb8_devices): (H, W, 3) uint8, top
    row first (the PNG's rows), + stats. progress(done, total): called as pixel-samples
    complete (pt_params.progress)."""
    if not bvh.built:
        bvh.build()
    ref = _SceneRef(bvh)
    W, H = camera.res
    dv = np.ascontiguousarray(devices, dtype=np.int32)
    prm = _lib.pt_params(samples, depth, seed, 0, len(dv), band_rows, kw.get("batch_spp", 0),
                         kw.get("samples_per_item", 0))
    cb = None
    if progress is not None:
        cb = PROGRESS_FN(lambda _user, done, total: progress(done, total))
        prm.progress = C.cast(cb, C.c_void_p)
    img = np.empty((H, W, 3), dtype=np.uint8)
    st = _lib.pt_stats()
    check(lib().pt_render_rgb8_devices(C.byref(ref.s), C.byref(camera.c), C.byref(prm), dv.ctypes.data, len(dv),
                                       C.c_float(gamma), img.ctypes.data, C.byref(st)))
    del cb
    return img, st.as_dict()


def moments_unconverged(sum, sumsq, n: int, rel: float, abs: float = 0.0, mask: bool = False):
    """The convergence count of per-pixel sample moments on the host (pt_moments_unconverged; no
    device needed): `sum` and `sumsq` (..., 3) float64 as Renderer.render_moments returns them
    after n samples. A pixel is converged iff n*Q - S*S <= (n-1) * (rel*|S| + abs*n)^2 holds in
    its three channels (sem <= rel*|mean| + abs without its divisions), evaluated in double; below
    two samples none is, and a NaN leaves its pixel unconverged. Returns the unconverged count,
    or with mask=True (count, uint8 array, 1 = unconverged)."""
    S = np.ascontiguousarray(sum, dtype=np.float64)
    Q = np.ascontiguousarray(sumsq, dtype=np.float64)
    if S.shape != Q.shape or S.size % 3:
        raise ValueError("sum and sumsq must have the same shape, three channels per pixel")
    npix = S.size // 3
    cnt = C.c_int64(0)
    m = np.empty(npix, dtype=np.uint8) if mask else None
    check(lib().pt_moments_unconverged(S.ctypes.data, Q.ctypes.data, npix, n, C.c_float(rel), C.c_float(abs),
                                       C.byref(cnt), m.ctypes.data if mask else None))
    return (cnt.value, m) if mask else cnt.value


def _variance_args(sum, sumsq, spp):
    S = np.ascontiguousarray(sum, dtype=np.float64)
    Q = np.ascontiguousarray(sumsq, dtype=np.float64)
    if S.shape != Q.shape or S.size % 3:
        raise ValueError("sum and sumsq must have the same shape, three channels per pixel")
    npix = S.size // 3
    sp = None
    if spp is not None:
        sp = np.ascontiguousarray(spp, dtype=np.int32)
        if sp.size != npix:
            raise ValueError("spp must hold one count per pixel")
    return S, Q, sp, npix


def moments_variance(sum, sumsq, n: int = 0, spp=None) -> np.ndarray:
    """The variance of the mean from per-pixel sample moments on the host (pt_moments_variance; no
    device needed): float32, the shape of `sum`. Per channel, in double: max(0, (Q - S*S/n) /
    (n - 1)) / n, +inf below two samples. n: one count for the image, or with `spp` (int32, one
    per pixel: render_adaptive's) each pixel's own. Not sem**2: sem is rounded after its root."""
    S, Q, sp, npix = _variance_args(sum, sumsq, spp)
    var = np.empty(S.shape, dtype=np.float32)
    check(lib().pt_moments_variance(S.ctypes.data, Q.ctypes.data, npix, n, sp.ctypes.data if sp is not None else None,
                                    var.ctypes.data))
    return var


def denoise_guides(aov: dict) -> dict:
    """The denoiser's guides from Renderer.aov's channels ("normal", "t", "tri", "emission" and
    "ray"): those four and "position" = o + d * t in float32, the multiplication rounded before
    the addition (as trace() forms its hit point). numpy arrays or torch tensors; on tensors the
    two operations are queued on torch's current stream, which Renderer.denoise waits for."""
    ray, t = aov["ray"], aov["t"]
    m = ray[..., 3:6] * t[..., None]
    pos = ray[..., 0:3] + m
    pos = pos.contiguous() if _is_tensor(pos) else np.ascontiguousarray(pos, dtype=np.float32)
    return {"normal": aov["normal"], "t": t, "tri": aov["tri"], "emission": aov["emission"], "position": pos}


def _denoise_args(color, var, guides):
    c = np.ascontiguousarray(color, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("color must have shape (H, W, 3)")
    H, W = c.shape[0], c.shape[1]
    v = None
    if var is not None:
        v = np.ascontiguousarray(var, dtype=np.float32)
        if v.shape != c.shape:
            raise ValueError("var must have the shape of color")
    g, keep = _lib.pt_denoise_guides(), []
    for k in _lib.pt_denoise_guides.NAMES:
        a = guides.get(k)
        if a is None:
            continue  # the library reports the missing guide
        a = np.ascontiguousarray(a, dtype=np.int32 if k == "tri" else np.float32)
        if a.size != H * W * _lib.pt_denoise_guides.WIDTH[k]:
            raise ValueError(f"guides[{k!r}] must hold H*W*{_lib.pt_denoise_guides.WIDTH[k]} elements")
        keep.append(a)
        setattr(g, k, a.ctypes.data)
    return W, H, c, v, g, keep


def denoise(color, guides, var=None, passes: int = 0, sigma_l: float = 0.0, sigma_z: float = 0.0,
            normal_pow_log2: int = 0, eps: float = 0.0):
    """The variance-guided a-trous denoiser on the host (pt_image_denoise; no device needed; the
    definition is in include/pt_hip.h): `passes` (default 5) edge-avoiding B3-spline passes with
    strides 1, 2, 4, ... over `color` (H, W, 3) float32, rows in render()'s order. A tap counts
    by the agreement of the first hit's normals (power 2**normal_pow_log2, default 2**7), by the
    distance of its hit point from the centre's tangent plane (sigma_z, default 0.01, of the hit
    distance) and, with `var` (the variance of the mean, moments_variance()), by the luminance
    difference in standard deviations (sigma_l, default 1); misses, emitters and other hits never
    mix. guides: denoise_guides() of an AOV. Returns (out, var_out): var_out is the filtered
    variance, None without `var`. A 0 selects a parameter's default."""
    W, H, c, v, g, _keep = _denoise_args(color, var, guides)
    prm = _lib.pt_denoise_params(passes, sigma_l, sigma_z, normal_pow_log2, eps)
    out = np.empty((H, W, 3), dtype=np.float32)
    vout = np.empty((H, W, 3), dtype=np.float32) if v is not None else None
    check(lib().pt_image_denoise(W, H, c.ctypes.data, v.ctypes.data if v is not None else None, C.byref(g), C.byref(prm),
                                 out.ctypes.data, vout.ctypes.data if vout is not None else None))
    return out, vout


class TemporalHistory:
    """The seven planes of an accumulated history (pt_temporal_history, include/pt_hip.h), numpy
    arrays or torch tensors, rows in render()'s order: color, m2, var, normal, position (H, W, 3)
    float32; hist (frames accumulated, < 1 marks a hole) and cls (H, W) int32."""
    NAMES = _lib.pt_temporal_history.NAMES

    def __init__(self, color, m2, var, hist, normal, position, cls):
        self.color, self.m2, self.var, self.hist = color, m2, var, hist
        self.normal, self.position, self.cls = normal, position, cls

    @classmethod
    def empty(cls, W: int, H: int, like=None) -> "TemporalHistory":
        """A history of holes (every plane 0, so hist marks nothing as written): numpy arrays, or
        with `like` a torch tensor, tensors on its device."""
        planes = {}
        for k in cls.NAMES:
            w = _lib.pt_temporal_history.WIDTH[k]
            shape = (H, W) if w == 1 else (H, W, w)
            integer = k in _lib.pt_temporal_history.INT
            if _is_tensor(like):
                import torch
                planes[k] = torch.zeros(shape, dtype=torch.int32 if integer else torch.float32, device=like.device)
            else:
                planes[k] = np.zeros(shape, dtype=np.int32 if integer else np.float32)
        return cls(**planes)

    def planes(self) -> dict:
        return {k: getattr(self, k) for k in self.NAMES}


def _history_host(h: TemporalHistory, W: int, H: int):
    """pt_temporal_history over a numpy history's own arrays (no copies: `next` is written in place)."""
    s, keep = _lib.pt_temporal_history(), []
    for k in _lib.pt_temporal_history.NAMES:
        a = getattr(h, k)
        if a is None:
            continue  # the library reports a missing plane
        dt = np.int32 if k in _lib.pt_temporal_history.INT else np.float32
        if _is_tensor(a) or not isinstance(a, np.ndarray) or a.dtype != dt or not a.flags.c_contiguous \
                or a.size != H * W * _lib.pt_temporal_history.WIDTH[k]:
            raise ValueError(f"history plane {k!r} must be a contiguous {np.dtype(dt).name} numpy array of "
                             f"H*W*{_lib.pt_temporal_history.WIDTH[k]} elements")
        keep.append(a)
        setattr(s, k, a.ctypes.data)
    return s, keep


def _no_tensors(color, var, guides) -> None:
    if any(_is_tensor(x) for x in (color, var) + tuple(guides.values())):
        raise ValueError("numpy arrays and torch tensors cannot be mixed in one call")


def temporal_accumulate(color, guides, camera: Camera, prev: Optional[TemporalHistory] = None,
                        prev_camera: Optional[Camera] = None, var=None, max_history: int = 0, sigma_z: float = 0.0,
                        normal_min: float = 0.0, variance_mode: int = 0):
    """One frame of temporal reprojection on the host (pt_image_temporal; no device needed; the
    definition is in include/pt_hip.h): every pixel's first hit (guides: denoise_guides() of the
    frame's AOV) is projected into `prev_camera`, the history `prev` is gathered there
    bilinearly where class, normal (normal_min, default 0.9) and tangent-plane distance (sigma_z,
    default 0.01, of the hit distance) agree, and blended with `color` (H, W, 3) with weight
    1/N, N <= max_history (default 32). `var`: the variance of `color` as a mean
    (moments_variance()); with it (variance_mode 0 or PT_TEMPORAL_VAR_SAMPLE) the variances are
    combined, without it (or PT_TEMPORAL_VAR_TEMPORAL) the accumulated moments give the variance.
    prev = None starts a history. Returns (next, reused): a new TemporalHistory whose color and
    var are what denoise() takes, and the number of pixels that reused their history."""
    _no_tensors(color, var, guides)
    W, H, c, v, g, _keep = _denoise_args(color, var, guides)
    if prev is not None and prev_camera is None:
        raise ValueError("prev needs prev_camera")
    ps, _pkeep = _history_host(prev, W, H) if prev is not None else (None, None)
    nxt = TemporalHistory.empty(W, H)
    ns, _nkeep = _history_host(nxt, W, H)
    prm = _lib.pt_temporal_params(max_history, sigma_z, normal_min, variance_mode)
    reused = C.c_int64(0)
    check(lib().pt_image_temporal(W, H, C.byref(camera.c), C.byref(prev_camera.c) if prev is not None else None,
                                  c.ctypes.data, v.ctypes.data if v is not None else None, C.byref(g),
                                  C.byref(ps) if ps is not None else None, C.byref(ns), C.byref(prm), C.byref(reused)))
    return nxt, reused.value


def devices_release() -> None:
    """Free the contexts pt_render_*_devices keeps per device list (pt_devices_release)."""
    lib().pt_devices_release()


def debug_counter(which: int) -> int:
    """Process-wide counters (test hook pt_debug_counter): 0 contexts created, 1 scene
    uploads, 2 cached device sets live, 3 uploads skipped on a cached context."""
    return int(lib().pt_debug_counter(which))


def visible_devices() -> List[int]:
    """Every visible GPU, or PT_DEVICES="0,2,..." (as the C++ drop-in)."""
    env = os.environ.get("PT_DEVICES", "")
    devs = [int(t) for t in env.split(",") if t.strip()]
    return devs or list(range(max(lib().pt_device_count(), 1)))


def to_rgb8(img: np.ndarray, gamma: float = 2.2) -> np.ndarray:
    """gamma_correct + save_png quantisation + flip (image.h:41-55): top row first."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    H, W = img.shape[:2]
    out = np.empty((H, W, 3), dtype=np.uint8)
    check(lib().pt_image_to_rgb8(img.ctypes.data, W, H, C.c_float(gamma), out.ctypes.data))
    return out


def rgb8_thresholds(gamma: float = 2.2):
    """The device quantiser's table: (thr (255,) float32, neg_mode); thr[k-1] = least
    float whose 8-bit value under to_rgb8 is >= k (pt_rgb8_thresholds)."""
    thr = np.empty(255, dtype=np.float32)
    mode = C.c_int32()
    check(lib().pt_rgb8_thresholds(C.c_float(gamma), thr.ctypes.data, C.byref(mode)))
    return thr, mode.value


def device_rgb8(img: np.ndarray, gamma: float = 2.2, device: int = 0) -> np.ndarray:
    """to_rgb8 computed by the device quantiser (test hook pt_debug_rgb8)."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    H, W = img.shape[:2]
    out = np.empty((H, W, 3), dtype=np.uint8)
    check(lib().pt_debug_rgb8(device, img.ctypes.data, W, H, C.c_float(gamma), out.ctypes.data))
    return out


def save_png(img: np.ndarray, filename: str, gamma: float = 2.2) -> bool:
    rgb = to_rgb8(img, gamma)
    rc = lib().pt_write_png(filename.encode(), rgb.ctypes.data, rgb.shape[1], rgb.shape[0])
    if rc < 0:
        print(lib().pt_last_error().decode(), file=sys.stderr)
        return False
    return True


def _render_to_file(camera: Camera, bvh: BVH, samples: int, depth: int, filename: str, unit: str, total: int,
                    after_done: str) -> bool:
    """render.h:62-104 / 109-152 around the device render: the reference's console lines
    (per row / per chunk progress as the library reports it, "Done in", "Saved to"), the
    image gamma-corrected and quantised on the device, its bytes written as the PNG."""
    if bvh.empty():
        print("No triangles in scene.", file=sys.stderr)
        return False
    if not bvh.built:
        print("Bounding volume heirarchy not built.\nBuilding...", file=sys.stderr)
        bvh.build()
    t0 = time.perf_counter()
    print(f"Rendered: 0/{total} {unit}.", end="", flush=True)
    printed = [0]

    def advance(k):
        while printed[0] < min(k, total):
            printed[0] += 1
            print(f"\rRendered: {printed[0]}/{total} {unit}.", end="", flush=True)

    rgb, _ = render_rgb8(camera, bvh, samples, depth, visible_devices(),
                         progress=lambda done, tot: advance(done * total // tot if tot else total))
    advance(total)
    print(f"\nDone in {math.floor((time.perf_counter() - t0) * 1000) / 1000:.2f} seconds.{after_done}")
    rc = lib().pt_write_png(filename.encode(), rgb.ctypes.data, rgb.shape[1], rgb.shape[0])
    if rc < 0:
        print(f"Failed to write image to file: {filename}", file=sys.stderr)
    print(f"Saved to {filename}")
    return True


def render_cpu(camera: Camera, bvh: BVH, samples: int, depth: int, filename: str) -> bool:
    """render.h:62-104 signature; the trace loop runs on the GPU."""
    return _render_to_file(camera, bvh, samples, depth, filename, "rows", camera.res[1], "\nColor correcting...")


def render_gpu(camera: Camera, bvh: BVH, samples: int, depth: int, chunk_size: Sequence[int], filename: str) -> bool:
    """render.h:109-152 signature; `chunk_size` only sets the progress granularity
    (the persistent kernel needs no watchdog-sized tiles)."""
    cx, cy = (chunk_size, chunk_size) if isinstance(chunk_size, int) else tuple(chunk_size)
    chunks = -(-camera.res[0] // cx) * -(-camera.res[1] // cy)
    return _render_to_file(camera, bvh, samples, depth, filename, "chunks", chunks, "")
