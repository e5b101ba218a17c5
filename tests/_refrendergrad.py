"""Material gradients of the rendered image along its own camera rays (include/pt_hip.h: "material
gradients of the rendered image ..."), restated over the restatements of the ray forms.

Sample s of pixel p is `camera_rays(scene, seed, s)`: `_reftrace.camera_rays` generalised to sample
s (the LCG starts at pt_sample_seed(p, s, seed); the states handed to the path are those after the
camera's two draws). The terms are `_refgrad.path_terms` / `_refneegrad.path_terms` of every
sample's paths with grad_rgb = fl(G / spp) and their own spp = 1: the ray forms divide by 1, so the
float32 terms are bit-equal to the definition's w = G[p] / (float)spp.

Sums: `exact` is the exact sum of every term of every sample, `ordered` the terms added in double in
(pixel, sample, k) order, and the tolerance the sum over the samples of `_refgrad.summarize`'s
any-order tolerance of that sample's terms. No tolerance of its own is introduced here.
"""
from __future__ import annotations

import functools

import numpy as np

import _oracle as O
import _refgrad as RG
import _refneegrad as NG
import _reftrace as RT

F32 = np.float32
MODES = ("plain", "nee", "nee+mis")
SCENES = ("cornell+glow", "random_7_300")


def mode_kw(mode: str) -> dict:
    return {"plain": {}, "nee": {"light_sampling": True}, "nee+mis": {"light_sampling": True, "mis": True}}[mode]


def camera_rays(scene, seed: int, s: int = 0):
    """Camera::get_ray (camera.h:63-73) for sample s of every pixel, as `_reftrace.camera_rays` states
    it for sample 0: (origins, directions, the states after the two draws), pixels in row order."""
    c = O.camera(scene)
    W, H = scene.camera.res
    pos, (vx, vy, cell, dist), T = c[0:3], c[5:9], c[9:18].reshape(3, 3)
    s0 = RT.sample_seeds(W * H, s + 1, seed)[:, s]
    s1, s2 = RT.lcg_step(s0, 1), RT.lcg_step(s0, 2)
    with np.errstate(all="ignore"):
        jy = s1.astype(F32) / F32(4294967296.0)
        jx = s2.astype(F32) / F32(4294967296.0)
        w = (np.arange(W * H) % W).astype(F32)
        h = (np.arange(W * H) // W).astype(F32)
        cam = np.stack([(w + jx) * cell - vx / F32(2), (h + jy) * cell - vy / F32(2), np.full(W * H, -dist, dtype=F32)], axis=-1)
        d = np.stack([RT._dot(cam, T[:, k][None, :]) for k in range(3)], axis=-1).astype(F32)
        d = (d / np.sqrt(RT._dot(d, d))[:, None]).astype(F32)
    o = np.repeat(pos[None, :].astype(F32), W * H, axis=0)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), s2


def grad_img(res) -> np.ndarray:
    """The upstream gradient of a W x H frame: `_refgrad.grad_rgb` of its pixels, (H, W, 3)."""
    W, H = res
    return RG.grad_rgb(W * H).reshape(H, W, 3)


def scaled(G: np.ndarray, spp: int) -> np.ndarray:
    """fl(G / spp): what the per-sample loop hands to the ray forms."""
    with np.errstate(all="ignore"):
        return (np.asarray(G, dtype=F32).reshape(-1, 3) / F32(spp)).astype(F32)


class Expected:
    """What one render_grad call must return: the forward image, the summed terms, the counters."""

    def __init__(self, rgb, S, rays, shadow, draws, nonzero):
        self.rgb, self.S, self.rays, self.shadow, self.draws, self.nonzero = rgb, S, rays, shadow, draws, nonzero


def _segments(P: RT.Paths, depth: int) -> int:
    """Segments trace() walks to `depth` on the paths of P."""
    return int((P.tri[:depth] != RT.NOT_TRACED).sum())


@functools.lru_cache(maxsize=None)
def expected(name: str, res, spp: int, depth: int, seed: int, mode: str, override: bool = False) -> Expected:
    """The whole frame of `_reftrace.make_scene(name, res)` with `grad_img(res)`; `override`: at
    `_refgrad.overrides`' values (the light table stays the scene's)."""
    sc = RT.make_scene(name, tuple(res))
    verts, nodes, idx, mtype, mvals = RT.scene_arrays(name)
    T = mvals.shape[0]
    W, H = res
    n = W * H
    color, emit = RG.overrides(T) if override else (None, None)
    gs = scaled(grad_img(res), spp)
    per, tol = [], np.zeros((2, T, 3))
    rays = shadow = draws = 0
    acc = np.zeros((n, 3), dtype=F32)
    for s in range(spp):
        o, d, st = camera_rays(sc, seed, s)
        if mode == "plain":
            P = RT.walk_paths(nodes, idx, verts, mtype, mvals, o, d, st, max(depth, 1))
            t = RG.path_terms(P, depth, gs, 1, color, emit)
            rays += _segments(P, depth)
        else:
            Wk = NG.walk(nodes, idx, verts, mtype, mvals, o, d, st, max(depth, 1), mode == "nee+mis")
            nt = NG.path_terms(Wk, depth, gs, 1, color, emit)
            rays, shadow, draws = rays + nt.segments, shadow + nt.shadow, draws + nt.draws
            t = RG.Terms(nt.kind, nt.tri, nt.val, nt.path, nt.rgb)
        with np.errstate(all="ignore"):
            acc = acc + t.rgb.astype(F32)
        tol += RG.summarize(t, T).tol
        per.append(t)
    # every term in (pixel, sample, k) order: a stable sort of (sample, pixel, k) by pixel
    kind = np.concatenate([t.kind for t in per])
    tri = np.concatenate([t.tri for t in per])
    val = np.concatenate([t.val for t in per])
    path = np.concatenate([t.path for t in per])
    order = np.argsort(path, kind="stable")
    S = RG.summarize(RG.Terms(kind[order], tri[order], val[order], path[order], per[0].rgb), T)._replace(tol=tol)
    with np.errstate(all="ignore"):
        rgb = (acc / F32(spp)).astype(F32).reshape(H, W, 3)
    nonzero = bool(np.any(S.exact[RG.COLOR] != 0)) and bool(np.any(S.exact[RG.EMIT_K] != 0))
    return Expected(rgb, S, rays, shadow, draws, nonzero)


def objects(name: str, res):
    """(scene, built ptamd.BVH, ptamd.Camera) of `_reftrace.make_scene(name, res)`."""
    import ptamd
    sc = RT.make_scene(name, tuple(res))
    b = ptamd.BVH.from_scene(sc)
    b.build()
    return sc, b, ptamd.Camera.from_spec(sc.camera)


def check_stats(st: dict, E: Expected, npix: int, spp: int, mode: str, what=""):
    assert st["terms"] == E.S.terms and st["rays"] == E.rays and st["paths"] == npix * spp, (what, st, E.S.terms, E.rays)
    if mode != "plain":
        assert st["shadow_rays"] == E.shadow and st["light_draws"] == E.draws, (what, st, E.shadow, E.draws)


def same_result(a: dict, b: dict, S: RG.Summary, what=""):
    """Two render_grad results of the same call: rgb bit-equal, gradients within the tolerance of the exact sums."""
    if "rgb" in a or "rgb" in b:
        RT.assert_same(np.asarray(a["rgb"]).reshape(-1, 3), np.asarray(b["rgb"]).reshape(-1, 3), what)
    for r in (a, b):
        RG.assert_within(r["color"], r["emit"], S, what)
