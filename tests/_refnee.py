"""Expected answers of the light-sampling tests (test infrastructure): the estimator of
include/pt_hip.h ("light sampling (next-event estimation)") restated in Python from that header
text, over the oracle's primitives. Path and shadow segments are `_refwalk.ref_walk`'s
(BVH::intersect over `oracle_slab` and `oracle_tri_hit`), the light's three draws are
`oracle_lcg`'s, the new direction and LCG state `oracle_brdf`'s (Material::reflected_dir); the
rest is float32 numpy, one rounding per operation, in the header's operation order. Nothing here
calls the library under test.

A path is walked once to the largest depth a test asks for (`walk`); `radiance` then gives the
estimator at any smaller depth D from the same records: the first D - 1 vertices of a path do not
depend on D, and vertex D adds only its hit's emission (no light draw at k == depth)."""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple

import numpy as np

import _oracle as O
import _reftrace as RT
import _refwalk as RW
import _treecases as TC

F32 = np.float32
EMIT, SPECULAR = 1, 3
_dot, _cross = RT._dot, RT._cross


class Lights(NamedTuple):
    tri: np.ndarray     # (nl,) int32: the caller's triangle index of each light
    cdf: np.ndarray     # (nl,) float32: running sum of the areas
    area: np.float32    # A (0 without lights)
    kA: np.float32      # A / (float)M_PI
    listed: np.ndarray  # (num_tris,) bool
    v1: np.ndarray      # (nl, 3) each
    e1: np.ndarray
    e2: np.ndarray
    n: np.ndarray       # normalize(cross(e1, e2)), not faced
    emit: np.ndarray


def light_table(verts, mtype, mvals) -> Lights:
    verts = np.ascontiguousarray(verts, dtype=F32)
    mvals = np.ascontiguousarray(mvals, dtype=F32)
    tri, cdf, rows = [], [], []
    run = F32(0)
    with np.errstate(all="ignore"):
        for j in range(verts.shape[0]):
            if int(mtype[j]) != EMIT:
                continue
            e = mvals[j, 3:6]
            if not np.isfinite(e).all() or not (e > 0).any():
                continue
            v1 = verts[j, 0:3]
            e1, e2 = verts[j, 3:6] - v1, verts[j, 6:9] - v1
            c = _cross(e1, e2)
            ln = np.sqrt(_dot(c, c))
            a = F32(0.5) * ln
            if not np.isfinite(a) or not a > 0:
                continue
            run = F32(run + a)
            tri.append(j)
            cdf.append(run)
            rows.append((v1, e1, e2, (c / ln).astype(F32), e))
        nt = verts.shape[0]
        if not tri or not np.isfinite(run):
            z = np.zeros((0, 3), dtype=F32)
            return Lights(np.zeros(0, np.int32), np.zeros(0, F32), F32(0), F32(0), np.zeros(nt, bool), z, z, z, z, z)
        listed = np.zeros(nt, bool)
        listed[tri] = True
        col = lambda i: np.array([r[i] for r in rows], dtype=F32)
        return Lights(np.array(tri, np.int32), np.array(cdf, F32), F32(run), F32(run / F32(np.pi)), listed, col(0), col(1),
                      col(2), col(3), col(4))


class Paths(NamedTuple):
    after: np.ndarray   # (depth, n, 3) float32: L after steps 2-3 of segment k + 1 (before that vertex's light draw)
    traced: np.ndarray  # (depth, n) bool: the path walked segment k + 1
    shadow: np.ndarray  # (depth, n) bool: the vertex of segment k + 1 walked a shadow segment
    drew: np.ndarray    # (depth, n) bool: it drew a light
    lights: Lights


def walk(nodes, idx, verts, mtype, mvals, org, dirs, states, depth: int) -> Paths:
    """Every ray's path to `depth` segments, all rays one segment at a time. Vertex k < depth makes
    its light draw and then its BRDF draw; vertex `depth` makes neither."""
    L_ = O.lib()
    L_.oracle_brdf.restype = C.c_uint32
    verts = np.ascontiguousarray(verts, dtype=F32)
    mtype = np.ascontiguousarray(mtype, dtype=np.int32)
    mvals = np.ascontiguousarray(mvals, dtype=F32)
    lt = light_table(verts, mtype, mvals)
    nl = lt.tri.shape[0]
    o = np.array(org, dtype=F32).reshape(-1, 3)
    d = np.array(dirs, dtype=F32).reshape(-1, 3)
    n = o.shape[0]
    st = np.array(states, dtype=np.uint32).reshape(n).copy()
    T = np.ones((n, 3), dtype=F32)
    L = np.zeros((n, 3), dtype=F32)
    sampled = np.zeros(n, bool)
    after = np.zeros((depth, n, 3), dtype=F32)
    traced = np.zeros((depth, n), bool)
    shadow = np.zeros((depth, n), bool)
    drew = np.zeros((depth, n), bool)
    active = np.arange(n)
    nd = np.zeros(3, dtype=F32)
    s3 = np.zeros(3, dtype=np.uint32)
    x3 = np.zeros(3, dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(1, depth + 1):
            if active.size == 0:
                break
            t, hit = RW.ref_walk(nodes, idx, verts, o[active], d[active])  # step 1
            traced[k - 1, active] = True
            h0 = np.maximum(hit, 0)
            is_emit = (hit >= 0) & (mtype[h0] == EMIT)
            add = (hit >= 0) & ~(is_emit & sampled[active] & lt.listed[h0])  # steps 2 and 3
            ra = active[add]
            L[ra] = L[ra] + T[ra] * mvals[hit[add], 3:6]
            after[k - 1:] = L  # paths that ended earlier keep their value, at every later level too
            go = (hit >= 0) & ~is_emit
            if k == depth:  # step 5
                break
            rays, ht, tt = active[go], hit[go], t[go]
            v = verts[ht]
            nrm = _cross(v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3])
            nrm = (nrm / np.sqrt(_dot(nrm, nrm))[:, None]).astype(F32)
            flip = ~(_dot(nrm, d[rays]) < 0)
            nrm[flip] = -nrm[flip]
            p = o[rays] + d[rays] * tt[:, None]
            no = (p + nrm * F32(1e-4)).astype(F32)
            # step 4: the light draws of this level, then their shadow segments in one batch
            sh_ray, sh_w, sh_j, sh_c = [], [], [], []
            for i, r in enumerate(rays.tolist()):
                draw = int(mtype[ht[i]]) != SPECULAR and nl > 0
                sampled[r] = draw
                if not draw:
                    continue
                drew[k - 1, r] = True
                L_.oracle_lcg(int(st[r]), 3, s3.ctypes.data, x3.ctypes.data)
                st[r] = s3[2]
                x1, x2, x3_ = F32(x3[0]), F32(x3[1]), F32(x3[2])
                xa = F32(x1 * lt.area)
                j = min(int(np.searchsorted(lt.cdf, xa, side="right")), nl - 1)  # the first cdf_j > xa, else the last
                u, vv = x2, x3_
                if F32(u + vv) > F32(1):
                    u, vv = F32(F32(1) - u), F32(F32(1) - vv)
                y = (lt.v1[j] + lt.e1[j] * u) + lt.e2[j] * vv
                w = (y - no[i]).astype(F32)
                cx = _dot(nrm[i], w)
                cy = np.abs(_dot(lt.n[j], w))
                r2 = _dot(w, w)
                if cx > 0 and cy > 0 and r2 > 0:
                    g = F32(F32(F32(cx / r2) * F32(cy / r2)) * lt.kA)
                    sh_ray.append(i)
                    sh_w.append(w)
                    sh_j.append(j)
                    sh_c.append(((T[r] * mvals[ht[i], 0:3]) * lt.emit[j]) * g)
            if sh_ray:
                si = np.array(sh_ray)
                _, sh_hit = RW.ref_walk(nodes, idx, verts, no[si], np.array(sh_w, dtype=F32))
                shadow[k - 1, rays[si]] = True
                for m, i in enumerate(sh_ray):
                    if int(sh_hit[m]) == int(lt.tri[sh_j[m]]):
                        L[rays[i]] = L[rays[i]] + sh_c[m].astype(F32)
            # step 6
            for i, r in enumerate(rays.tolist()):
                dj, nj = np.ascontiguousarray(d[r]), np.ascontiguousarray(nrm[i])
                st[r] = L_.oracle_brdf(int(st[r]), int(mtype[ht[i]]), C.c_float(mvals[ht[i], 6]), dj.ctypes.data,
                                       nj.ctypes.data, nd.ctypes.data)
                d[r] = nd
            c = _dot(nrm, d[rays])
            T[rays] = ((F32(2) * T[rays]) * mvals[ht, 0:3]) * c[:, None]
            o[rays] = no
            active = rays
    return Paths(after, traced, shadow, drew, lt)


def radiance(P: Paths, depth: int):
    """The estimator at `depth` of every path: (rgb (n, 3) float32, segments (n,): path and shadow
    segments together, shadow segments (n,), light draws (n,))."""
    assert 0 <= depth <= P.after.shape[0]
    n = P.after.shape[1]
    if depth == 0:
        z = np.zeros(n, dtype=np.int64)
        return np.zeros((n, 3), dtype=F32), z, z, z
    sh = P.shadow[:depth - 1].sum(axis=0).astype(np.int64)
    dr = P.drew[:depth - 1].sum(axis=0).astype(np.int64)
    segs = P.traced[:depth].sum(axis=0).astype(np.int64) + sh
    return P.after[depth - 1].copy(), segs, sh, dr


def head(P: Paths, n: int) -> Paths:
    return Paths(P.after[:, :n], P.traced[:, :n], P.shadow[:, :n], P.drew[:, :n], P.lights)


def trace(nodes, idx, verts, mtype, mvals, org, dirs, states, depth: int):
    return radiance(walk(nodes, idx, verts, mtype, mvals, org, dirs, states, depth), depth)


# ---------------------------------------------------------------- expectations shared by the CPU and GPU tests
SCENES = ("cornell", "cornell+glow", "random_3_40", "random_7_300", "sphere12")
DEPTHS = (1, 2, 5, 8)
TREES = [("cornell", "merged5"), ("cornell", "chain_left"), ("mcornell", "duplicated"), ("mcornell", "dropped")]


@functools.lru_cache(maxsize=None)
def paths(name: str, n: int = 512, seed: int = 1, explicit: bool = False, depth: int = RT.MAX_DEPTH) -> Paths:
    """`_reftrace.paths`' rays and states, walked by this estimator."""
    verts, nodes, idx, mtype, mvals = RT.scene_arrays(name)
    o, d = RT.rays(name, n)
    st = RT.explicit_states(n) if explicit else RT.sample_seeds(n, 1, seed)[:, 0]
    return walk(nodes, idx, verts, mtype, mvals, o, d, st, depth)


@functools.lru_cache(maxsize=None)
def lights(name: str) -> Lights:
    verts, _, _, mtype, mvals = RT.scene_arrays(name)
    return light_table(verts, mtype, mvals)


@functools.lru_cache(maxsize=None)
def nonfinite_expected(depth=5):
    verts, nodes, idx, mtype, mvals = RT.scene_arrays("random_7_300")
    o, d = RW.nonfinite_rays()
    rgb, segs, sh, _ = trace(nodes, idx, verts, mtype, mvals, o, d, RT.sample_seeds(16, 1, 1)[:, 0], depth)
    return o, d, rgb, int(segs.sum()), int(sh.sum())


@functools.lru_cache(maxsize=None)
def tree_expected(name, variant, depth=5):
    """The estimator on the case's own nodes and tri_idx (272 rays, 16 of them non-finite)."""
    c = TC.case(name, variant)
    _, mtype, _ = O.pack_scene(TC.scene(name))
    o, d = TC.rays()
    rgb, segs, sh, _ = trace(c.nodes, c.idx, c.verts, mtype, c.mvals, o, d, RT.sample_seeds(o.shape[0], 1, 1)[:, 0], depth)
    return o, d, rgb, int(segs.sum()), int(sh.sum())


def edge_lights_scene():
    """Cornell with two more EMIT triangles that are no lights: one of zero emission and one
    degenerate (zero area); the table must leave both out."""
    from ptamd import scenes
    sc = scenes.cornell((8, 8))
    sc.add([((100.0, 100.0, 100.0), (200.0, 100.0, 100.0), (100.0, 200.0, 100.0))], scenes.Material.make(scenes.EMIT, 0, (0.0, 0.0, 0.0)))
    sc.add([((300.0, 300.0, 300.0), (350.0, 350.0, 350.0), (400.0, 400.0, 400.0))], scenes.Material.make(scenes.EMIT, 0, (5.0, 5.0, 5.0)))
    return sc
