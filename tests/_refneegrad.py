"""Expected material gradients of the light-sampling estimator (test infrastructure): the per-path
quantities and terms of include/pt_hip.h ("material gradients of the light-sampling estimator")
restated in numpy from that header text alone. Nothing here calls the library under test.

`walk` is `_refnee.walk` / `_refmis.walk` (the same segments, draws and light table over the oracle's
primitives: `_refwalk.ref_walk`, `oracle_lcg`, `oracle_brdf`, `_refnee.light_table`) keeping what
those two throw away: per segment the triangle hit, what kind of hit it was, the bounce's cosine,
and at a visible light draw the light's triangle and the scalar g (g wl with the weights). A path is
walked once to the largest depth a test asks for; `path_terms` evaluates the definition at any
smaller depth from the same records (the first D - 1 vertices of a path do not depend on D, and
vertex D makes no draw), in float32 (the contract's arithmetic) or in float64 / complex128 (the
same formulas in that type, for the complex-step check).

Path p has bounces k = 0 .. K-1 on triangles h_k with cosines c_k, then a terminal.
w = grad_rgb[ray] / float32(spp); Tw_0 = w, Tw_{k+1} = ((2 Tw_k) color_k) c_k.
R_K = the terminal's value; R_k = (emit_k + D_k) + ((2 R_{k+1}) color_k) c_k with
D_k = (color_k emit_j) g_k at a visible light draw, no D_k otherwise. Bounce k adds, in this order,
Tw_k to d emit[h_k]; with a visible light (Tw_k color_k) g_k to d emit[j_k] and (Tw_k emit_j) g_k
to d color[h_k]; then ((2 Tw_k) R_{k+1}) c_k to d color[h_k]. A terminal hit adds Tw_K m to
d emit[h_K]; a dropped hit and a miss add nothing."""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple

import numpy as np

import _oracle as O
import _refgrad as RG
import _refmis as RM
import _refnee as RN
import _reftrace as RT
import _refwalk as RW
import _treecases as TC

F32 = np.float32
EMIT, SPECULAR = RN.EMIT, RN.SPECULAR
_dot, _cross = RT._dot, RT._cross
COLOR, EMIT_K = RG.COLOR, RG.EMIT_K
# what a segment's hit was
MISS, PLAIN, WEIGHTED, DROPPED, SURFACE = 0, 1, 2, 3, 4
# which case a term came from
T_BOUNCE, T_LIGHT, T_SUFFIX, T_END, T_END_WEIGHTED = 0, 1, 2, 3, 4


class Walk(NamedTuple):
    hit: np.ndarray     # (depth, n) int64: the triangle segment k + 1 hit (-1: a miss or not walked)
    kind: np.ndarray    # (depth, n) int8: MISS, PLAIN / WEIGHTED / DROPPED (an EMIT hit), SURFACE (any other hit)
    cos: np.ndarray     # (depth, n) float32: the cosine of the bounce at a SURFACE hit that went on
    light: np.ndarray   # (depth, n) int64: the visible light's triangle at that vertex, else -1
    g: np.ndarray       # (depth, n) float32: its g (g wl with the weights)
    wb: np.ndarray      # (depth, n) float32: a WEIGHTED hit's multiplier
    traced: np.ndarray  # (depth, n) bool
    shadow: np.ndarray  # (depth, n) bool
    drew: np.ndarray    # (depth, n) bool
    mtype: np.ndarray
    mvals: np.ndarray
    lights: RN.Lights
    mis: bool


def _unit_normals(v):
    nrm = _cross(v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3])
    return (nrm / np.sqrt(_dot(nrm, nrm))[:, None]).astype(F32)


def walk(nodes, idx, verts, mtype, mvals, org, dirs, states, depth: int, mis: bool) -> Walk:
    """Every ray's path to `depth` segments, all rays one segment at a time: steps 1-6 of the
    definition's geometry (no radiance is formed here)."""
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
    sampled = np.zeros(n, bool)
    hit_r = np.full((depth, n), -1, dtype=np.int64)
    kind = np.zeros((depth, n), dtype=np.int8)
    cos = np.zeros((depth, n), dtype=F32)
    light = np.full((depth, n), -1, dtype=np.int64)
    g_r = np.zeros((depth, n), dtype=F32)
    wb_r = np.ones((depth, n), dtype=F32)
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
            hit_r[k - 1, active] = hit
            h0 = np.maximum(hit, 0)
            is_emit = (hit >= 0) & (mtype[h0] == EMIT)
            after_draw = is_emit & sampled[active] & lt.listed[h0]  # step 2's special case
            kk = np.where(hit < 0, MISS, np.where(is_emit, PLAIN, SURFACE)).astype(np.int8)
            kk[after_draw] = WEIGHTED if mis else DROPPED
            kind[k - 1, active] = kk
            if mis and after_draw.any():
                rw = active[after_draw]
                hw, tw = hit[after_draw], t[after_draw].astype(F32)
                cyd = np.abs(_dot(_unit_normals(verts[hw]), d[rw])).astype(F32)
                a = (cyd / tw).astype(F32)
                wb_r[k - 1, rw] = (one / (one + tw / (a * hA).astype(F32)).astype(F32)).astype(F32)
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
            sh_ray, sh_w, sh_j, sh_g = [], [], [], []
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
                    if mis:
                        a = F32(cy / r2)
                        s = F32(np.sqrt(F32(r2)))
                        wl = F32(one / F32(one + F32(F32(a * hA) / s)))
                        gg = F32(F32(F32(F32(cx / r2) * a) * lt.kA) * wl)
                    else:
                        gg = F32(F32(F32(cx / r2) * F32(cy / r2)) * lt.kA)
                    sh_ray.append(i)
                    sh_w.append(w)
                    sh_j.append(j)
                    sh_g.append(gg)
            if sh_ray:
                si = np.array(sh_ray)
                _, sh_hit = RW.ref_walk(nodes, idx, verts, no[si], np.array(sh_w, dtype=F32))
                shadow[k - 1, rays[si]] = True
                for m, i in enumerate(sh_ray):
                    if int(sh_hit[m]) == int(lt.tri[sh_j[m]]):
                        light[k - 1, rays[i]] = int(lt.tri[sh_j[m]])
                        g_r[k - 1, rays[i]] = sh_g[m]
            # step 6
            for i, r in enumerate(rays.tolist()):
                dj, nj = np.ascontiguousarray(d[r]), np.ascontiguousarray(nrm[i])
                st[r] = L_.oracle_brdf(int(st[r]), int(mtype[ht[i]]), C.c_float(mvals[ht[i], 6]), dj.ctypes.data,
                                       nj.ctypes.data, nd.ctypes.data)
                d[r] = nd
            cos[k - 1, rays] = _dot(nrm, d[rays])
            o[rays] = no
            active = rays
    return Walk(hit_r, kind, cos, light, g_r, wb_r, traced, shadow, drew, mtype, mvals, lt, mis)


class Terms(NamedTuple):
    kind: np.ndarray   # (M,) 0 = d color, 1 = d emit
    tri: np.ndarray    # (M,) the caller's triangle
    val: np.ndarray    # (M, 3) the term, in (path, k) order and the definition's order within a bounce
    path: np.ndarray   # (M,) the path it came from
    case: np.ndarray   # (M,) T_BOUNCE (Tw_k), T_LIGHT (a visible light's pair), T_SUFFIX, T_END, T_END_WEIGHTED
    rgb: np.ndarray    # (paths, 3) the forward-form value of every path
    dropped: int       # paths that ended in a dropped hit
    segments: int      # path and shadow segments together, at this depth
    shadow: int
    draws: int


def path_terms(W: Walk, depth: int, grad_rgb, spp: int = 1, color=None, emit=None, dtype=F32) -> Terms:
    """The terms of every path of W cut at `depth`; path p belongs to ray p // spp. `color`, `emit`:
    (T, 3) values to evaluate at (default: W.mvals'); the light table stays W's, and only the
    emission of a light is read from `emit`."""
    assert 1 <= depth <= W.hit.shape[0]
    color = np.asarray(W.mvals[:, 0:3] if color is None else color).astype(dtype)
    emit = np.asarray(W.mvals[:, 3:6] if emit is None else emit).astype(dtype)
    gr = np.asarray(grad_rgb).reshape(-1, 3).astype(dtype)
    two, fs = dtype(2), dtype(spp)
    n = W.hit.shape[1]
    assert gr.shape[0] * spp == n
    kind, tri, val, path, case = [], [], [], [], []
    rgb = np.zeros((n, 3), dtype=dtype)
    dropped = 0

    def put(kd, tr, v, p, cs):
        kind.append(kd)
        tri.append(tr)
        val.append(v)
        path.append(p)
        case.append(cs)

    with np.errstate(all="ignore"):
        for p in range(n):
            hs, cs, ls, gs = [], [], [], []  # the bounces
            end, end_kind, m = -1, MISS, dtype(1)
            T = np.ones(3, dtype=dtype)
            L = np.zeros(3, dtype=dtype)
            for k in range(depth):  # the forward form, steps 1-6
                h = int(W.hit[k, p])
                kd = int(W.kind[k, p])
                if h < 0:
                    break
                if kd != SURFACE:
                    end, end_kind = h, kd
                    if kd == PLAIN:
                        L = L + T * emit[h]
                    elif kd == WEIGHTED:
                        m = dtype(W.wb[k, p])
                        L = L + (T * emit[h]) * m
                    else:
                        dropped += 1
                    break
                L = L + T * emit[h]
                if k + 1 == depth:
                    end, end_kind = h, PLAIN
                    break
                lj = int(W.light[k, p])
                g = dtype(W.g[k, p])
                c = dtype(W.cos[k, p])
                if lj >= 0:
                    L = L + ((T * color[h]) * emit[lj]) * g
                hs.append(h)
                cs.append(c)
                ls.append(lj)
                gs.append(g)
                T = ((two * T) * color[h]) * c
            rgb[p] = L
            K = len(hs)
            R = np.zeros(3, dtype=dtype)  # the suffix pass
            if end_kind == PLAIN:
                R = emit[end]
            elif end_kind == WEIGHTED:
                R = emit[end] * m
            below = [None] * K
            for k in range(K - 1, -1, -1):
                below[k] = R
                e = emit[hs[k]] + (color[hs[k]] * emit[ls[k]]) * gs[k] if ls[k] >= 0 else emit[hs[k]]
                R = e + ((two * R) * color[hs[k]]) * cs[k]
            Tw = gr[p // spp] / fs  # the throughput pass
            for k in range(K):
                h = hs[k]
                put(EMIT_K, h, Tw, p, T_BOUNCE)
                if ls[k] >= 0:
                    put(EMIT_K, ls[k], (Tw * color[h]) * gs[k], p, T_LIGHT)
                    put(COLOR, h, (Tw * emit[ls[k]]) * gs[k], p, T_LIGHT)
                put(COLOR, h, ((two * Tw) * below[k]) * cs[k], p, T_SUFFIX)
                Tw = ((two * Tw) * color[h]) * cs[k]
            if end_kind == PLAIN:
                put(EMIT_K, end, Tw, p, T_END)
            elif end_kind == WEIGHTED:
                put(EMIT_K, end, Tw * m, p, T_END_WEIGHTED)
    sh = int(W.shadow[:depth - 1].sum())
    return Terms(np.array(kind, dtype=np.int64), np.array(tri, dtype=np.int64), np.array(val, dtype=dtype).reshape(-1, 3),
                 np.array(path, dtype=np.int64), np.array(case, dtype=np.int64), rgb, dropped,
                 int(W.traced[:depth].sum()) + sh, sh, int(W.drew[:depth - 1].sum()))


def summarize(t: Terms, num_tris: int) -> RG.Summary:
    """`_refgrad.summarize` (exact sums, counts, the any-order tolerance, the (path, k)-ordered sums)."""
    return RG.summarize(RG.Terms(t.kind, t.tri, t.val, t.path, t.rgb), num_tris)


def case_counts(t: Terms, case: int, num_tris: int) -> np.ndarray:
    """(2, T): per destination, the terms that came from `case`."""
    out = np.zeros((2, num_tris), dtype=np.int64)
    sel = t.case == case
    np.add.at(out, (t.kind[sel], t.tri[sel]), 1)
    return out


def mean_rgb(t: Terms, spp: int) -> np.ndarray:
    return RG.mean_rgb(RG.Terms(t.kind, t.tri, t.val, t.path, t.rgb), spp)


# ---------------------------------------------------------------- expectations shared by the CPU and GPU tests
SCENES = ("cornell+glow", "random_7_300", "tri3")
DEPTHS = (1, 2, 5, 8)
N = 257


@functools.lru_cache(maxsize=None)
def scene_arrays(name: str):
    """(verts, nodes, idx, mtype, mvals) of `_reftrace`'s scenes, of "tri3" (`_refmis.tri3_scene`) and
    of "no_lights" (`diffuse_emitter_scene`)."""
    if name in ("tri3", "no_lights"):
        verts, mtype, mvals = O.pack_scene(make_scene(name))
        nodes, idx = O.bvh_build(verts)
        return verts, nodes, idx, mtype, mvals
    return RT.scene_arrays(name)


def make_scene(name: str):
    return RM.tri3_scene() if name == "tri3" else diffuse_emitter_scene() if name == "no_lights" else RT.make_scene(name)


def diffuse_emitter_scene():
    """cornell+glow with its emitter made a DIFFUSE material that keeps its emission: a scene
    without lights (every path still returns a non-zero value)."""
    import dataclasses
    from ptamd import scenes
    sc = RT.make_scene("cornell+glow")
    sc.mats = [dataclasses.replace(m, type=scenes.DIFFUSE, color=(0.5, 0.5, 0.5)) if m.type == scenes.EMIT else m
               for m in sc.mats]
    return sc


def rays(name: str, n: int):
    """The scene's ray set: `_reftrace.rays` (Cornell's for "no_lights"), and for "tri3" the edge rays of `_refmis`."""
    return RM.edge_rays(n) if name == "tri3" else RT.rays("cornell" if name == "no_lights" else name, n)


@functools.lru_cache(maxsize=None)
def walked(name: str, n: int, spp: int, mis: bool, seed: int = 1, depth: int = RT.MAX_DEPTH) -> Walk:
    """Sample s of ray i of `rays(name, n)` as path i * spp + s, started at pt_sample_seed(i, s, seed)."""
    verts, nodes, idx, mtype, mvals = scene_arrays(name)
    o, d = rays(name, n)
    st = RT.sample_seeds(n, spp, seed).reshape(-1)
    return walk(nodes, idx, verts, mtype, mvals, np.repeat(o, spp, axis=0), np.repeat(d, spp, axis=0), st, depth, mis)


@functools.lru_cache(maxsize=None)
def expected(name: str, n: int, depth: int, spp: int, mis: bool, override: bool = False, walk_depth: int = 0):
    """(Terms, Summary) of the first n rays of the scene's set with `_refgrad.grad_rgb(n)`;
    `override`: at `_refgrad.overrides`' values (the light table stays the scene's)."""
    W = walked(name, n, spp, mis, depth=walk_depth or RT.MAX_DEPTH)
    num_tris = W.mvals.shape[0]
    color, emit = RG.overrides(num_tris) if override else (None, None)
    t = path_terms(W, depth, RG.grad_rgb(n), spp, color, emit)
    return t, summarize(t, num_tris)


@functools.lru_cache(maxsize=None)
def tree_expected(name, variant, mis: bool, depth=5):
    """The 256 finite rays of `_treecases.rays` on the case's own nodes and tri_idx, at
    `_refgrad.overrides`' materials: (o, d, Terms, Summary)."""
    c = TC.case(name, variant)
    _, mtype, _ = O.pack_scene(TC.scene(name))
    o, d = TC.rays()
    o, d = np.ascontiguousarray(o[:256]), np.ascontiguousarray(d[:256])
    st = RT.sample_seeds(256, 1, 1)[:, 0]
    W = walk(c.nodes, c.idx, c.verts, mtype, c.mvals, o, d, st, depth, mis)
    color, emit = RG.overrides(c.verts.shape[0])
    t = path_terms(W, depth, RG.grad_rgb(256), 1, color, emit)
    return o, d, t, summarize(t, c.verts.shape[0])
