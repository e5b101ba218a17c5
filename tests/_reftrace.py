"""Expected answers of the trace tests (test infrastructure): trace() (render.h:36-61) restated
in Python over the oracle's primitives. The hit is `_refwalk.ref_walk`'s (BVH::intersect over
`oracle_slab` and `oracle_tri_hit`), the new direction and LCG state are `oracle_brdf`'s
(Material::reflected_dir), the rest is float32 numpy in linalg.h's operation order. Nothing here
calls the library under test.

A path is walked once to the largest depth a test asks for (`walk_paths`); `radiance` then gives
trace(depth) for any smaller depth from the same records, because the first segments of a path
do not depend on the depth it is cut at."""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple

import numpy as np

import _oracle as O
import _refwalk as RW
import _treecases as TC

F32 = np.float32
EMIT = 1
NOT_TRACED = -2


def lcg_step(s: np.ndarray, times: int = 1) -> np.ndarray:
    """s = 1664525 s + 1013904223 mod 2^32 (rng.h:14-20), `times` times."""
    s = np.asarray(s, dtype=np.uint64)
    for _ in range(times):
        s = (s * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(0xFFFFFFFF)
    return s.astype(np.uint32)


def sample_seeds(n: int, samples: int, seed: int, first: int = 0) -> np.ndarray:
    """pt_sample_seed(first + i, s, seed) as the oracle computes it: (n, samples) uint32."""
    f = O.lib().oracle_sample_seed
    return np.array([[f(first + i, s, seed) for s in range(samples)] for i in range(n)], dtype=np.uint32).reshape(n, samples)


def _dot(a, b):
    """linalg.h's dot: (x x + y y) + z z, every product and sum rounded to float32."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


class Paths(NamedTuple):
    tri: np.ndarray    # (depth, n) int32: the triangle hit on segment k, -1 a miss, NOT_TRACED after the path's end
    cos: np.ndarray    # (depth, n) float32: hit_n . new_d of a bounce
    state: np.ndarray  # (depth, n) uint32: the LCG state after segment k's BRDF draw (bounces only)
    init: np.ndarray   # (n,) uint32: the states the paths started with
    mtype: np.ndarray
    mvals: np.ndarray


def walk_paths(nodes, idx, verts, mtype, mvals, org, dirs, states, depth: int) -> Paths:
    """Every ray's path to `depth` segments, all rays one segment at a time. A non-emitter draws
    its BRDF sample on every segment, the last one included (render.h:51 comes before the
    recursive call)."""
    L = O.lib()
    L.oracle_brdf.restype = C.c_uint32
    verts = np.ascontiguousarray(verts, dtype=F32)
    mtype = np.ascontiguousarray(mtype, dtype=np.int32)
    mvals = np.ascontiguousarray(mvals, dtype=F32)
    o = np.array(org, dtype=F32).reshape(-1, 3)
    d = np.array(dirs, dtype=F32).reshape(-1, 3)
    n = o.shape[0]
    st = np.array(states, dtype=np.uint32).reshape(n).copy()
    init = st.copy()
    tri = np.full((depth, n), NOT_TRACED, dtype=np.int32)
    cos = np.zeros((depth, n), dtype=F32)
    state = np.zeros((depth, n), dtype=np.uint32)
    active = np.arange(n)
    nd = np.zeros(3, dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(depth):
            if active.size == 0:
                break
            t, hit = RW.ref_walk(nodes, idx, verts, o[active], d[active])
            tri[k, active] = hit
            go = (hit >= 0) & (mtype[np.maximum(hit, 0)] != EMIT)
            rays, ht, tt = active[go], hit[go], t[go]
            v = verts[ht]
            nrm = _cross(v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3])
            nrm = (nrm / np.sqrt(_dot(nrm, nrm))[:, None]).astype(F32)
            flip = ~(_dot(nrm, d[rays]) < 0)
            nrm[flip] = -nrm[flip]
            p = o[rays] + d[rays] * tt[:, None]
            for j, r in enumerate(rays.tolist()):
                dj, nj = np.ascontiguousarray(d[r]), np.ascontiguousarray(nrm[j])
                st[r] = L.oracle_brdf(int(st[r]), int(mtype[ht[j]]), C.c_float(mvals[ht[j], 6]), dj.ctypes.data,
                                      nj.ctypes.data, nd.ctypes.data)
                d[r] = nd
            o[rays] = p + nrm * F32(1e-4)
            cos[k, rays] = _dot(nrm, d[rays])
            state[k, rays] = st[rays]
            active = rays
    return Paths(tri, cos, state, init, mtype, mvals)


def radiance(P: Paths, depth: int):
    """trace(depth) of every path: (rgb (n, 3) float32, final LCG state (n,), segments (n,)). An
    EMIT hit ends the path with its emit, a miss or depth used up with 0; then, backwards,
    L = emit + ((2 L) color) c."""
    assert depth <= P.tri.shape[0]
    n = P.tri.shape[1]
    L = np.zeros((n, 3), dtype=F32)
    final = P.init.copy()
    segs = np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(depth):
            traced = P.tri[k] != NOT_TRACED
            segs += traced
            bounce = (P.tri[k] >= 0) & (P.mtype[np.maximum(P.tri[k], 0)] != EMIT)
            final[bounce] = P.state[k, bounce]
        for k in range(depth - 1, -1, -1):
            h = P.tri[k]
            hit = h >= 0
            emit = P.mvals[np.maximum(h, 0), 3:6]
            color = P.mvals[np.maximum(h, 0), 0:3]
            is_emit = hit & (P.mtype[np.maximum(h, 0)] == EMIT)
            bounce = hit & ~is_emit
            folded = emit + ((F32(2) * L) * color) * P.cos[k][:, None]
            L = np.where(is_emit[:, None], emit, np.where(bounce[:, None], folded, L)).astype(F32)
    return L, final, segs


def head(P: Paths, n: int) -> Paths:
    """The first n paths."""
    return Paths(P.tri[:, :n], P.cos[:, :n], P.state[:, :n], P.init[:n], P.mtype, P.mvals)


def trace(nodes, idx, verts, mtype, mvals, org, dirs, states, depth: int):
    return radiance(walk_paths(nodes, idx, verts, mtype, mvals, org, dirs, states, depth), depth)


def same_bits(a, b) -> np.ndarray:
    """Per channel: bits equal, or both NaN (NaN payloads differ between hosts and the GPU)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what=""):
    ok = same_bits(got, want).reshape(len(want), -1).all(axis=1)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} rays differ, first {bad[:4]}: got {np.asarray(got)[bad[:4]]}, want {np.asarray(want)[bad[:4]]}"


# ---------------------------------------------------------------- scenes and ray sets
SCENES = ("cornell", "random_3_40", "random_7_300", "sphere12")
GLOW = ("cornell", "sphere12")  # their plain rays almost never reach the light


def make_scene(name: str, res=(16, 16)):
    """`name`, or "<scene>+glow": every non-EMIT material given a small seeded emission, so that
    every hit path returns a non-zero value (and finish_path's dark-path skip is off)."""
    base, _, variant = name.partition("+")
    sc = RW.make_scene(base, res)
    if variant == "glow":
        import dataclasses
        e = np.random.default_rng(11).uniform(0.01, 0.2, (len(sc.mats), 3)).astype(F32)
        sc.mats = [m if m.type == EMIT else dataclasses.replace(m, emit=tuple(float(c) for c in e[i]))
                   for i, m in enumerate(sc.mats)]
    else:
        assert not variant
    return sc


ALL = SCENES + tuple(g + "+glow" for g in GLOW)
MAX_DEPTH = 8


@functools.lru_cache(maxsize=None)
def scene_arrays(name: str):
    base = name.partition("+")[0]
    verts, nodes, idx = RW.oracle_bvh(base)
    _, mtype, mvals = O.pack_scene(make_scene(name))
    return verts, nodes, idx, mtype, mvals


@functools.lru_cache(maxsize=None)
def paths(name: str, n: int = 512, seed: int = 1, explicit: bool = False, depth: int = MAX_DEPTH) -> Paths:
    """The first n rays of `_refwalk.expected(scene)` walked to `depth` segments, one sample each:
    default seeding pt_sample_seed(i, 0, seed), or (explicit) the states of `explicit_states`."""
    verts, nodes, idx, mtype, mvals = scene_arrays(name)
    o, d, _, _ = RW.expected(name.partition("+")[0])
    st = explicit_states(n) if explicit else sample_seeds(n, 1, seed)[:, 0]
    return walk_paths(nodes, idx, verts, mtype, mvals, o[:n], d[:n], st, depth)


def explicit_states(n: int) -> np.ndarray:
    return np.random.default_rng(77).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def rays(name: str, n: int):
    o, d, _, _ = RW.expected(name.partition("+")[0])
    return o[:n], d[:n]


def check_floor(name: str, rgb: np.ndarray, P: Paths, depth: int):
    """A test cannot pass on zeros: glow sets are non-zero on every hit ray and hit >= 0.75 n;
    random_7_300 at depth >= 5 is non-zero on >= 0.5 n (the fractions for sets of 256 rays or more)."""
    n = rgb.shape[0]
    nonzero = int((rgb.view(np.uint32).reshape(n, 3) != 0).any(axis=1).sum())
    if name.endswith("+glow"):
        hits = int((P.tri[0, :n] >= 0).sum())
        assert nonzero == hits and (n < 256 or hits >= 0.75 * n), (name, nonzero, hits, n)
    elif name == "random_7_300" and depth >= 5 and n >= 256:
        assert nonzero >= 0.5 * n, (name, nonzero, n)


def camera_rays(scene, seed: int):
    """Camera::get_ray (camera.h:63-73) for sample 0 of every pixel, in float32 numpy: the y jitter
    is drawn first (g++ evaluates the vec3's arguments right to left), from the LCG state
    pt_sample_seed(h W + w, 0, seed). Returns (origins, directions, the states after the two
    draws), pixels in row order h W + w."""
    c = O.camera(scene)
    W, H = scene.camera.res
    pos, (vx, vy, cell, dist), T = c[0:3], c[5:9], c[9:18].reshape(3, 3)
    s0 = sample_seeds(W * H, 1, seed)[:, 0]
    s1, s2 = lcg_step(s0, 1), lcg_step(s0, 2)
    with np.errstate(all="ignore"):
        jy = s1.astype(F32) / F32(4294967296.0)
        jx = s2.astype(F32) / F32(4294967296.0)
        w = (np.arange(W * H) % W).astype(F32)
        h = (np.arange(W * H) // W).astype(F32)
        cam = np.stack([(w + jx) * cell - vx / F32(2), (h + jy) * cell - vy / F32(2), np.full(W * H, -dist, dtype=F32)], axis=-1)
        d = np.stack([_dot(cam, T[:, k][None, :]) for k in range(3)], axis=-1).astype(F32)
        d = (d / np.sqrt(_dot(d, d))[:, None]).astype(F32)
    o = np.repeat(pos[None, :].astype(F32), W * H, axis=0)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), s2


# ---------------------------------------------------------------- expectations shared by the CPU and GPU tests
TREES = [("cornell", "merged5"), ("cornell", "chain_left"), ("cornell", "empty"), ("cornell", "uncontained"),
         ("mcornell", "duplicated"), ("mcornell", "dropped")]


def mean_of_samples(trace_one, n, spp, seed):
    """The float32 sum, in sample order from +0, of the spp single-sample results (sample s of ray
    i started at pt_sample_seed(i, s, seed)), divided by float32(spp)."""
    states = sample_seeds(n, spp, seed)
    acc = np.zeros((n, 3), dtype=F32)
    with np.errstate(all="ignore"):
        for s in range(spp):
            acc = acc + trace_one(np.ascontiguousarray(states[:, s]))
        return (acc / F32(spp)).astype(F32)


@functools.lru_cache(maxsize=None)
def nonfinite_expected(depth=5):
    verts, nodes, idx, mtype, mvals = scene_arrays("random_7_300")
    o, d = RW.nonfinite_rays()
    rgb, _, segs = trace(nodes, idx, verts, mtype, mvals, o, d, sample_seeds(16, 1, 1)[:, 0], depth)
    return o, d, rgb, segs


@functools.lru_cache(maxsize=None)
def tree_expected(name, variant, depth=5):
    """_reftrace on the case's own nodes and tri_idx (272 rays, 16 of them non-finite)."""
    c = TC.case(name, variant)
    _, mtype, _ = O.pack_scene(TC.scene(name))
    o, d = TC.rays()
    rgb, _, segs = trace(c.nodes, c.idx, c.verts, mtype, c.mvals, o, d, sample_seeds(o.shape[0], 1, 1)[:, 0], depth)
    return o, d, rgb, int(segs.sum())




def overflow_scene():
    """A unit-scale dark SPECULAR triangle under a small light. A ray straight down with
    |d| = 2e38 hits it at a finite point, 2 (d . n) overflows, the reflected direction and its
    cosine are NaN, the next segment misses, and render.h:60 returns 0 + ((2 * 0) * color) * NaN."""
    from ptamd import scenes
    cam = scenes.CameraSpec((0.25, 0.25, 3.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), (4, 4), 40.0, 1.0)
    sc = scenes.Scene("overflow", cam)
    sc.add([((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))], scenes.Material.make(scenes.SPECULAR, 0.5, 0, 0.1))
    sc.add([((0.0, 0.0, 2.0), (0.0, 1.0, 2.0), (1.0, 0.0, 2.0))], scenes.Material.make(scenes.EMIT, 0, (1.0, 1.0, 1.0)))
    return sc


@functools.lru_cache(maxsize=None)
def overflow_expected(depth=3):
    """64 rays onto the triangle: every fourth with the overflowing direction, the others ordinary."""
    verts, _, _ = O.pack_scene(overflow_scene())
    _, mtype, mvals = O.pack_scene(overflow_scene())
    nodes, idx = O.bvh_build(verts)
    o = np.tile(np.array([[0.25, 0.25, 1.0]], dtype=F32), (64, 1))
    d = np.tile(np.array([[0.0, 0.0, -1.0]], dtype=F32), (64, 1))
    d[::4, 2] = F32(-2e38)
    rgb, _, segs = trace(nodes, idx, verts, mtype, mvals, o, d, sample_seeds(64, 1, 1)[:, 0], depth)
    assert np.isnan(rgb[::4]).all() and not np.isnan(rgb[1::4]).any()
    return o, d, rgb, int(segs.sum())
