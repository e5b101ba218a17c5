"""Expected answers of the weighted light-sampling tests (test infrastructure): the estimator of
include/pt_hip.h ("the weighted estimator (multiple importance sampling, balance heuristic)")
restated in Python from that header text. It is `_refnee.walk` (the unweighted estimator's
restatement: the same segments, draws and light table, over the oracle's primitives) with the two
steps the header changes: step 4 multiplies a visible light's term by wl, and step 2 adds
(T o emit) wb at an EMIT hit on a listed triangle after a light draw. float32 numpy, one rounding
per operation, in the header's operation order. Nothing here calls the library under test.

`walk` also records which vertices took either weighted case, so a test can show that its
comparison is not vacuous."""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple

import numpy as np

import _oracle as O
import _refnee as RN
import _reftrace as RT
import _refwalk as RW
import _treecases as TC

F32 = np.float32
EMIT, SPECULAR = RN.EMIT, RN.SPECULAR
_dot, _cross = RT._dot, RT._cross


class Paths(NamedTuple):
    after: np.ndarray   # (depth, n, 3) float32: L after steps 2-3 of segment k + 1 (before that vertex's light draw)
    traced: np.ndarray  # (depth, n) bool: the path walked segment k + 1
    shadow: np.ndarray  # (depth, n) bool: the vertex of segment k + 1 walked a shadow segment
    drew: np.ndarray    # (depth, n) bool: it drew a light
    whit: np.ndarray    # (depth, n) bool: segment k + 1 ended in a weighted EMIT hit (step 2)
    wvis: np.ndarray    # (depth, n) bool: the vertex of segment k + 1 added a weighted visible light (step 4)
    lights: RN.Lights


def _unit_normals(v):
    nrm = _cross(v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3])
    return (nrm / np.sqrt(_dot(nrm, nrm))[:, None]).astype(F32)


def walk(nodes, idx, verts, mtype, mvals, org, dirs, states, depth: int) -> Paths:
    """Every ray's path to `depth` segments, all rays one segment at a time (as `_refnee.walk`)."""
    L_ = O.lib()
    L_.oracle_brdf.restype = C.c_uint32
    verts = np.ascontiguousarray(verts, dtype=F32)
    mtype = np.ascontiguousarray(mtype, dtype=np.int32)
    mvals = np.ascontiguousarray(mvals, dtype=F32)
    lt = RN.light_table(verts, mtype, mvals)
    nl = lt.tri.shape[0]
    hA = F32(F32(0.5) * lt.kA)
    one = F32(1)
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
    whit = np.zeros((depth, n), bool)
    wvis = np.zeros((depth, n), bool)
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
            weighted = is_emit & sampled[active] & lt.listed[h0]  # step 2's changed case
            add = (hit >= 0) & ~weighted  # steps 2 and 3 as they were
            ra = active[add]
            L[ra] = L[ra] + T[ra] * mvals[hit[add], 3:6]
            rw = active[weighted]
            if rw.size:
                hw, tw = hit[weighted], t[weighted].astype(F32)
                cyd = np.abs(_dot(_unit_normals(verts[hw]), d[rw])).astype(F32)
                a = (cyd / tw).astype(F32)
                wb = (one / (one + tw / (a * hA).astype(F32)).astype(F32)).astype(F32)
                L[rw] = L[rw] + ((T[rw] * mvals[hw, 3:6]) * wb[:, None]).astype(F32)
                whit[k - 1, rw] = True
            after[k - 1:] = L  # paths that ended earlier keep their value, at every later level too
            go = (hit >= 0) & ~is_emit
            if k == depth:  # step 5
                break
            rays, ht, tt = active[go], hit[go], t[go]
            nrm = _unit_normals(verts[ht])
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
                    a = F32(cy / r2)
                    s = F32(np.sqrt(F32(r2)))
                    wl = F32(one / F32(one + F32(F32(a * hA) / s)))
                    g = F32(F32(F32(cx / r2) * a) * lt.kA)
                    gw = F32(g * wl)
                    sh_ray.append(i)
                    sh_w.append(w)
                    sh_j.append(j)
                    sh_c.append(((T[r] * mvals[ht[i], 0:3]) * lt.emit[j]) * gw)
            if sh_ray:
                si = np.array(sh_ray)
                _, sh_hit = RW.ref_walk(nodes, idx, verts, no[si], np.array(sh_w, dtype=F32))
                shadow[k - 1, rays[si]] = True
                for m, i in enumerate(sh_ray):
                    if int(sh_hit[m]) == int(lt.tri[sh_j[m]]):
                        L[rays[i]] = L[rays[i]] + sh_c[m].astype(F32)
                        wvis[k - 1, rays[i]] = True
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
    return Paths(after, traced, shadow, drew, whit, wvis, lt)


def radiance(P: Paths, depth: int):
    """The estimator at `depth` of every path: (rgb (n, 3) float32, segments (n,): path and shadow
    segments together, shadow segments (n,), light draws (n,))."""
    return RN.radiance(RN.Paths(P.after, P.traced, P.shadow, P.drew, P.lights), depth)


def weighted_counts(P: Paths, depth: int):
    """(paths that ended in a weighted EMIT hit, paths that added a weighted visible light) at `depth`."""
    if depth == 0:
        return 0, 0
    return int(P.whit[:depth].any(axis=0).sum()), int(P.wvis[:depth - 1].any(axis=0).sum())


def head(P: Paths, n: int) -> Paths:
    return Paths(P.after[:, :n], P.traced[:, :n], P.shadow[:, :n], P.drew[:, :n], P.whit[:, :n], P.wvis[:, :n], P.lights)


def trace(nodes, idx, verts, mtype, mvals, org, dirs, states, depth: int):
    return radiance(walk(nodes, idx, verts, mtype, mvals, org, dirs, states, depth), depth)


# ---------------------------------------------------------------- expectations shared by the CPU and GPU tests
@functools.lru_cache(maxsize=None)
def paths(name: str, n: int = 512, seed: int = 1, explicit: bool = False, depth: int = RT.MAX_DEPTH) -> Paths:
    """`_refnee.paths`' rays and states, walked by the weighted estimator."""
    verts, nodes, idx, mtype, mvals = RT.scene_arrays(name)
    o, d = RT.rays(name, n)
    st = RT.explicit_states(n) if explicit else RT.sample_seeds(n, 1, seed)[:, 0]
    return walk(nodes, idx, verts, mtype, mvals, o, d, st, depth)


@functools.lru_cache(maxsize=None)
def nonfinite_expected(depth=5):
    verts, nodes, idx, mtype, mvals = RT.scene_arrays("random_7_300")
    o, d = RW.nonfinite_rays()
    rgb, segs, sh, _ = trace(nodes, idx, verts, mtype, mvals, o, d, RT.sample_seeds(16, 1, 1)[:, 0], depth)
    return o, d, rgb, int(segs.sum()), int(sh.sum())


@functools.lru_cache(maxsize=None)
def tree_expected(name, variant, depth=5):
    """The weighted estimator on the case's own nodes and tri_idx (272 rays, 16 of them non-finite)."""
    c = TC.case(name, variant)
    _, mtype, _ = O.pack_scene(TC.scene(name))
    o, d = TC.rays()
    P = walk(c.nodes, c.idx, c.verts, mtype, c.mvals, o, d, RT.sample_seeds(o.shape[0], 1, 1)[:, 0], depth)
    rgb, segs, sh, _ = radiance(P, depth)
    return o, d, rgb, int(segs.sum()), int(sh.sum()), weighted_counts(P, depth)


# ---------------------------------------------------------------- the edge rays of tri3
EDGE_N = 65536


def tri3_scene():
    """tests/test_render.cc's scene: the blue emitter (o, x, z) shares an edge with the white
    diffuse triangle (o, x, y)."""
    from ptamd import scenes
    return scenes.tri3((16, 16))


@functools.lru_cache(maxsize=None)
def edge_rays(n: int = EDGE_N):
    """n rays from (1.8, 1.8, 1.8) to targets (px, py, 0) on the diffuse triangle that crowd the
    shared edge y = 0: px uniform in [0.05, 0.8], py = uniform(0, 0.1)^2. Directions normalised in
    double, then rounded to float32. The first k rays do not depend on n."""
    rng = np.random.default_rng(5)
    px = rng.uniform(0.05, 0.8, EDGE_N)
    py = rng.uniform(0, 0.1, EDGE_N) ** 2
    eye = np.array([1.8, 1.8, 1.8])
    dd = np.stack([px, py, np.zeros(EDGE_N)], axis=-1) - eye
    dd /= np.linalg.norm(dd, axis=1)[:, None]
    o = np.repeat(eye[None, :], EDGE_N, axis=0).astype(F32)
    return np.ascontiguousarray(o[:n]), np.ascontiguousarray(dd.astype(F32)[:n])


@functools.lru_cache(maxsize=None)
def edge_paths(n: int = 256, depth: int = 5) -> Paths:
    """The first n edge rays on tri3, seeded pt_sample_seed(i, 0, 1), walked by the weighted estimator."""
    verts, mtype, mvals = O.pack_scene(tri3_scene())
    nodes, idx = O.bvh_build(verts)
    o, d = edge_rays(n)
    return walk(nodes, idx, verts, mtype, mvals, o, d, RT.sample_seeds(n, 1, 1)[:, 0], depth)
