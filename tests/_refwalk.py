"""Expected answers of the ray-query tests (test infrastructure): BVH::intersect
(bvh.h:156-183) restated in Python over the oracle's own BVH (`_oracle.bvh_build`) and its
two primitives, `oracle_slab` (AABB::intersect_inv) and `oracle_tri_hit`
(Triangle::intersect). Nothing here calls the library under test."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import _oracle as O
from _randscene import random_scene

T_MISS = np.float32(1e30)  # FLOAT_INF


def _lib():
    L = O.lib()
    L.oracle_slab.restype = C.c_int
    L.oracle_tri_hit.restype = C.c_int
    return L


def inverse(d: np.ndarray) -> np.ndarray:
    """1 / d in float32; division by zero gives inf (bvh.h:157)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return (np.float32(1) / d.astype(np.float32)).astype(np.float32)


def ref_walk(nodes: np.ndarray, idx: np.ndarray, verts: np.ndarray, org: np.ndarray, dirs: np.ndarray):
    """(t (n,) float32, tri (n,) int32): nodes popped LIFO with the right child first, the
    slab test on 1 / d, a leaf's triangles in tri_idx order, the winner replaced only when
    t_ < t, t from 1e30f; tri = tri_idx[i] or -1."""
    L = _lib()
    slab, tri_hit = L.oracle_slab, L.oracle_tri_hit
    nodes = np.ascontiguousarray(nodes)
    verts = np.ascontiguousarray(verts, dtype=np.float32)
    org = np.ascontiguousarray(org, dtype=np.float32)
    dirs = np.ascontiguousarray(dirs, dtype=np.float32)
    inv = np.ascontiguousarray(inverse(dirs))
    nb, vb, ob, db, ib = (a.ctypes.data for a in (nodes, verts, org, dirs, inv))
    left, right = nodes["left"].tolist(), nodes["right"].tolist()
    ts, te = nodes["tri_start"].tolist(), nodes["tri_end"].tolist()
    tidx = idx.tolist()
    n = org.shape[0]
    t_out = np.empty(n, dtype=np.float32)
    tri_out = np.empty(n, dtype=np.int32)
    tt = C.c_float()
    ptt = C.addressof(tt)
    for r in range(n):
        po, pd, pi = ob + 12 * r, db + 12 * r, ib + 12 * r
        stack = [0]
        ret, t = -1, float(T_MISS)
        while stack:
            k = stack.pop()
            if not slab(nb + 40 * k, nb + 40 * k + 12, po, pi):
                continue
            if left[k] == -1 and right[k] == -1:
                for i in range(ts[k], te[k] + 1):
                    ti = tidx[i]
                    if tri_hit(vb + 36 * ti, po, pd, ptt) and tt.value < t:
                        t, ret = tt.value, ti
            else:
                stack.append(left[k])
                stack.append(right[k])
        t_out[r], tri_out[r] = t, ret
    return t_out, tri_out


def ray_set(seed: int, n: int):
    """Seeded rays: origins uniform in [0, 500]^3, directions normal (unnormalised); every
    10th ray has one direction component exactly 0, every 50th is axis-aligned, 5 % start in
    [-300, -50]^3 and point away from the room (misses), ray 1 has d = (0, 0, 0)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(0, 500, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    for i in range(0, n, 10):
        d[i, rng.integers(3)] = 0.0
    for i in range(0, n, 50):
        a = rng.integers(3)
        d[i] = 0.0
        d[i, a] = rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)
    out = rng.choice(n, max(1, n // 20), replace=False)
    o[out] = rng.uniform(-300, -50, (len(out), 3)).astype(np.float32)
    d[out] = -np.abs(rng.normal(size=(len(out), 3))).astype(np.float32) - np.float32(0.01)
    if n > 1:
        d[1] = 0.0
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def nonfinite_rays():
    """16 rays with inf or NaN components (the oracle primitives define their answers)."""
    rng = np.random.default_rng(99)
    o = rng.uniform(0, 500, (16, 3)).astype(np.float32)
    d = rng.normal(size=(16, 3)).astype(np.float32)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    d[0, 0], d[1, 1], d[2, 2] = inf, -inf, nan
    d[3] = (inf, inf, inf)
    d[4] = (nan, nan, nan)
    o[5, 0], o[6, 1], o[7, 2] = inf, -inf, nan
    o[8] = (nan, nan, nan)
    o[9], d[9] = (inf, 250, 250), (-1, 0, 0)
    d[10] = (0, inf, 0)
    d[11] = (nan, 0, 1)
    o[12], d[12] = (250, 250, 250), (inf, 1, 1)
    o[13, 0], d[13, 0] = nan, nan
    d[14] = (1e-45, 1, 1)     # a denormal component: 1 / d overflows to inf
    d[15] = (3e38, -3e38, 1)  # huge components: 1 / d is denormal
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def make_scene(name: str, res=(16, 16)):
    from ptamd import scenes
    if name == "cornell":
        return scenes.cornell(tuple(res))
    if name.startswith("random_"):
        _, seed, ntris = name.split("_")
        return random_scene(int(seed), int(ntris), tuple(res))
    if name.startswith("sphere"):
        return scenes.sphere_in_cornell(int(name[len("sphere"):]), tuple(res))
    raise KeyError(name)


# rays per scene: the helper takes well under a second for each set (a few ctypes calls per ray)
RAYS = {"cornell": 1024, "random_3_40": 1024, "random_7_300": 512, "sphere12": 512}


@functools.lru_cache(maxsize=None)
def oracle_bvh(name: str):
    verts, _, _ = O.pack_scene(make_scene(name))
    nodes, idx = O.bvh_build(verts)
    return verts, nodes, idx


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """(origins, directions, t, tri) of the scene's ray set, computed once per process."""
    verts, nodes, idx = oracle_bvh(name)
    o, d = ray_set(1000 + len(name), RAYS[name])
    t, tri = ref_walk(nodes, idx, verts, o, d)
    for a in (o, d, t, tri):
        a.setflags(write=False)
    return o, d, t, tri


@functools.lru_cache(maxsize=None)
def expected_nonfinite(name: str):
    verts, nodes, idx = oracle_bvh(name)
    o, d = nonfinite_rays()
    t, tri = ref_walk(nodes, idx, verts, o, d)
    for a in (o, d, t, tri):
        a.setflags(write=False)
    return o, d, t, tri


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
