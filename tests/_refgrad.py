"""Expected material gradients of trace() (test infrastructure): the per-path terms of
include/pt_hip.h's contract computed from `_reftrace.Paths` (the triangle and cosine of every
segment), `grad_rgb` and the material values, in numpy float32 in the contract's operation order.
Nothing here calls the library under test.

Path (i, s) has bounces k = 0 .. K-1 on triangles h_k with cosines c_k, then a terminal.
w = grad_rgb[i] / float32(spp); T_0 = w, T_{k+1} = ((2 T_k) color_{h_k}) c_k; L_{k+1} is the
unwinding's value below bounce k. Bounce k adds T_k to d emit[h_k] and ((2 T_k) L_{k+1}) c_k to
d color[h_k]; a terminal that is a hit adds T_K to d emit[h_K]; a miss adds nothing.

Per destination (kind, triangle) and channel `summarize` gives the exactly rounded sum of the terms
(math.fsum), their count N and sum of magnitudes, and the tolerance N 2^-52 sum|t|: any order of
summing N float64 values stays within gamma_{N-1} sum|t| <= (N-1) 2^-53 sum|t| (1 + O(N 2^-53)) of
the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); twice the
first-order bound covers the higher-order terms. It is derived, not measured."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

import _oracle as O
import _reftrace as RT
import _treecases as TC

F32 = np.float32
COLOR, EMIT_K = 0, 1  # kinds of destination


class Terms(NamedTuple):
    kind: np.ndarray  # (M,) 0 = d color, 1 = d emit
    tri: np.ndarray   # (M,) the caller's triangle
    val: np.ndarray   # (M, 3) the term, in (path, k) order; a bounce's d emit term before its d color term
    path: np.ndarray  # (M,) the path it came from
    rgb: np.ndarray   # (paths, 3) the forward value of every path (the unwinding's result)


def path_terms(P: RT.Paths, depth: int, grad_rgb, spp: int = 1, color=None, emit=None, dtype=F32) -> Terms:
    """The terms of every path of P cut at `depth`; path p belongs to ray p // spp. `color`,
    `emit`: (T, 3) values to evaluate at (default: P.mvals'). dtype float32 is the contract's
    arithmetic; float64 (or complex128) evaluates the same formulas in that type."""
    assert depth <= P.tri.shape[0]
    color = np.asarray(P.mvals[:, 0:3] if color is None else color).astype(dtype)
    emit = np.asarray(P.mvals[:, 3:6] if emit is None else emit).astype(dtype)
    g = np.asarray(grad_rgb).reshape(-1, 3).astype(dtype)
    two, zero, fs = dtype(2), dtype(0), dtype(spp)
    n = P.tri.shape[1]
    assert g.shape[0] * spp == n
    kind, tri, val, path = [], [], [], []
    rgb = np.zeros((n, 3), dtype=dtype)
    with np.errstate(all="ignore"):
        for p in range(n):
            hs, term = [], -1
            for k in range(depth):
                h = int(P.tri[k, p])
                if h < 0:
                    break  # a miss
                if P.mtype[h] == RT.EMIT or k + 1 >= depth:
                    term = h
                    break
                hs.append(h)
            L = np.zeros(3, dtype=dtype)
            if term >= 0:
                L = emit[term] if P.mtype[term] == RT.EMIT else emit[term] + zero * color[term]
            below = [None] * len(hs)
            for k in range(len(hs) - 1, -1, -1):
                below[k] = L
                L = emit[hs[k]] + ((two * L) * color[hs[k]]) * dtype(P.cos[k, p])
            rgb[p] = L
            T = g[p // spp] / fs
            for k, h in enumerate(hs):
                c = dtype(P.cos[k, p])
                kind += [EMIT_K, COLOR]
                tri += [h, h]
                val += [T, ((two * T) * below[k]) * c]
                path += [p, p]
                T = ((two * T) * color[h]) * c
            if term >= 0:
                kind.append(EMIT_K)
                tri.append(term)
                val.append(T)
                path.append(p)
    return Terms(np.array(kind, dtype=np.int64), np.array(tri, dtype=np.int64),
                 np.array(val, dtype=dtype).reshape(-1, 3), np.array(path, dtype=np.int64), rgb)


class Summary(NamedTuple):
    exact: np.ndarray    # (2, T, 3) float64: math.fsum of the destination's terms
    count: np.ndarray    # (2, T) terms per destination
    sabs: np.ndarray     # (2, T, 3) sum of |term|
    tol: np.ndarray      # (2, T, 3) count * 2^-52 * sabs
    ordered: np.ndarray  # (2, T, 3) the terms added in double in (path, k) order
    terms: int           # all terms


def summarize(t: Terms, num_tris: int) -> Summary:
    exact = np.zeros((2, num_tris, 3))
    sabs = np.zeros((2, num_tris, 3))
    ordered = np.zeros((2, num_tris, 3))
    count = np.zeros((2, num_tris), dtype=np.int64)
    v = t.val.astype(np.float64)
    with np.errstate(all="ignore"):
        for i in range(len(t.kind)):
            ordered[t.kind[i], t.tri[i]] += v[i]
    for kind in (COLOR, EMIT_K):
        for tri in np.unique(t.tri[t.kind == kind]):
            rows = v[(t.kind == kind) & (t.tri == tri)]
            count[kind, tri] = rows.shape[0]
            for c in range(3):
                exact[kind, tri, c] = math.fsum(rows[:, c].tolist())
                sabs[kind, tri, c] = math.fsum(np.abs(rows[:, c]).tolist())
    tol = count[:, :, None] * 2.0 ** -52 * sabs
    return Summary(exact, count, sabs, tol, ordered, len(t.kind))


def assert_within(got_color, got_emit, S: Summary, what="", scale=1.0, extra=None):
    """Every destination and channel within its tolerance (times `scale`, plus `extra` (2, T, 3))."""
    for kind, got in ((COLOR, got_color), (EMIT_K, got_emit)):
        got = np.asarray(got, dtype=np.float64).reshape(-1, 3)
        assert got.shape == S.exact[kind].shape, (what, got.shape)
        tol = S.tol[kind] * scale + (0.0 if extra is None else extra[kind])
        err = np.abs(got - S.exact[kind])
        bad = np.argwhere(~(err <= tol))
        assert bad.size == 0, (f"{what}: {'d color' if kind == COLOR else 'd emit'}: {len(bad)} entries outside the tolerance, "
                               f"first {bad[:3].tolist()}: got {[got[tuple(b)] for b in bad[:3]]}, "
                               f"want {[S.exact[kind][tuple(b)] for b in bad[:3]]}, tol {[tol[tuple(b)] for b in bad[:3]]}")


def grad_rgb(n: int) -> np.ndarray:
    """The upstream gradient every test uses: default_rng(5).uniform(-1, 1), (n, 3) float32."""
    return np.random.default_rng(5).uniform(-1, 1, (n, 3)).astype(F32)


def overrides(num_tris: int):
    """Seeded override rows, uniform in [0.05, 0.95]: (color, emit), each (T, 3) float32."""
    r = np.random.default_rng(23)
    return r.uniform(0.05, 0.95, (num_tris, 3)).astype(F32), r.uniform(0.05, 0.95, (num_tris, 3)).astype(F32)


@functools.lru_cache(maxsize=None)
def paths_spp(name: str, n: int, spp: int, seed: int, depth: int) -> RT.Paths:
    """Sample s of ray i of `_reftrace.rays(name, n)` as path i * spp + s, started at
    pt_sample_seed(i, s, seed) and walked to `depth` segments."""
    if spp == 1 and seed == 1 and n <= 512 and depth <= RT.MAX_DEPTH:
        return RT.head(RT.paths(name), n)  # the walk the trace tests share
    verts, nodes, idx, mtype, mvals = RT.scene_arrays(name)
    o, d = RT.rays(name, n)
    st = RT.sample_seeds(n, spp, seed).reshape(-1)
    return RT.walk_paths(nodes, idx, verts, mtype, mvals, np.repeat(o, spp, axis=0), np.repeat(d, spp, axis=0), st, depth)


@functools.lru_cache(maxsize=None)
def expected(name: str, n: int, depth: int, spp: int = 1, seed: int = 1, override: bool = False, walk_depth: int = 0):
    """(Terms, Summary) of the first n rays of the scene's set with grad_rgb(n); `override`: at
    `overrides`' values. walk_depth: the depth the shared walk goes to (default: 5, or `depth`)."""
    P = paths_spp(name, n, spp, seed, walk_depth or max(depth, 5))
    num_tris = P.mvals.shape[0]
    color, emit = overrides(num_tris) if override else (None, None)
    t = path_terms(P, depth, grad_rgb(n), spp, color, emit)
    return t, summarize(t, num_tris)


@functools.lru_cache(maxsize=None)
def tree_expected(name, variant, depth=5):
    """The 256 finite rays of `_treecases.rays` on the case's own nodes and tri_idx, at
    `overrides`' materials (every term non-zero): (o, d, states, Terms, Summary)."""
    c = TC.case(name, variant)
    _, mtype, _ = O.pack_scene(TC.scene(name))
    o, d = TC.rays()
    o, d = np.ascontiguousarray(o[:256]), np.ascontiguousarray(d[:256])
    st = RT.sample_seeds(256, 1, 1)[:, 0]
    P = RT.walk_paths(c.nodes, c.idx, c.verts, mtype, c.mvals, o, d, st, depth)
    color, emit = overrides(c.verts.shape[0])
    t = path_terms(P, depth, grad_rgb(256), 1, color, emit)
    return o, d, st, t, summarize(t, c.verts.shape[0])


def mean_rgb(t: Terms, spp: int) -> np.ndarray:
    """The float32 in-order sum of every ray's samples, divided by float32(spp)."""
    r = t.rgb.reshape(-1, spp, 3).astype(F32)
    acc = np.zeros((r.shape[0], 3), dtype=F32)
    with np.errstate(all="ignore"):
        for s in range(spp):
            acc = acc + r[:, s]
        return (acc / F32(spp)).astype(F32)
