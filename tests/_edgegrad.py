"""The gradient kernels on edge scenes, edge materials and every kernel form (test infrastructure):
the case tables of tests/test_edge_grad_cpu.py (the host forms) and tests/test_edge_grad_gpu.py
(pt_grad_kernel, pt_grad_cam_kernel, pt_nee_grad_kernel, pt_nee_grad_cam_kernel), the expected
terms of every case, and the rule one call is held to. DESIGN.md §3.30 lists which case drives
which kernel form and gate. Nothing here calls the library under test.

The terms are `_refgrad.path_terms` / `_refneegrad.path_terms` over `_reftrace.walk_paths` /
`_refneegrad.walk` on the oracle's tree of the scene (`_edgescenes.arrays` for a member of
tests/_edgescenes.py, `_reftrace.scene_arrays` for "cornell+glow" and the random scenes). A ray set
is named by a hashable key (`paths_of`), so every walk is cached: a walk runs once at the largest
sample count and depth a test asks for, and a smaller sample count is a slice of it (sample s of
ray i starts at pt_sample_seed(i, s, seed) whatever the count).

Camera rays are one more ray set: sample s of pixel p is path p * spp + s along
`_refrendergrad.camera_rays(scene, seed, s)`, with the upstream gradient G[p] and the call's spp
(fl(G / spp) / 1 == G / (float)spp bit for bit, so these are `_refrendergrad.expected`'s terms for
any member). Their tolerance is `_refgrad.summarize`'s over all N terms of a destination, the
any-order bound of include/pt_hip.h.

The rule for one call (`assert_call`): rgb bit-equal (NaN = NaN) to the restatement and to the host
form; `terms` the restatement's count of terms of the requested kinds; every other count the host
form's; a destination channel whose terms are all finite within N 2^-52 sum|t| of the exact sum
(`_refgrad.summarize`, no tolerance of its own); and a channel with a non-finite term of the class
float64 addition gives in any order (N float32 terms cannot overflow a double: N 2^128 << 2^1024):
NaN iff some term is NaN or both infinities occur, +inf iff only +inf occurs, -inf iff only -inf.
A +-0 term is counted and leaves its destination as it is (a destination of zero terms alone has
tolerance 0: it must be 0)."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import _edgelights as EL
import _edgescenes as E
import _refgrad as RG
import _refneegrad as NG
import _refrendergrad as RR
import _reftrace as RT
import _refwalk as RW

F32 = np.float32
MODES = RR.MODES
COLOR, EMIT_K = RG.COLOR, RG.EMIT_K
DEPTH = 5
SEED = EL.SEED        # the ray forms' seed
RENDER_SEED = 7       # render_grad's
FINITE, NAN, PINF, NINF = 0, 1, 2, 3
WANT_BOTH = ("rgb", "color", "emit")
WANTS = (("emit",), ("color",), ("rgb", "emit"))

# ---------------------------------------------------------------- the case tables
# A: edge members along caller rays (`_edgescenes.query_rays`, at most 480 rays), 1 and 3 samples
A_BASES = ("cornell", "random_4_150")
A_FAMILY = ("scaled/-12", "scaled/20", "scaled/26", "scaled/51", "doubled/base", "doubled/alt", "degenerate",
            "outlier/sheet_2^40/d", "outlier/vertex_2^60/d", "outlier/maxfloat/s", "far_light/65", "far_light/110",
            "far_light_big/30", "far_light_big/62")
A_MEMBERS = tuple(f"{b}/{m}" for b in A_BASES for m in A_FAMILY)
A_EMPTY = "cornell/scaled/100"  # no ray hits: no term, every output +0
A_SAMPLES = (1, 3)
A_MIN_CHANNELS = 30  # non-zero channels in each of d color and d emit (not where `sparse`; see `channel_floor`)


def sparse(member: str) -> bool:
    """scaled/26 (SHIFT_BIAS is absorbed: paths end at their first bounce), scaled/51 and scaled/100
    (hardly a query ray hits, or none): the members the channel floor does not apply to."""
    _, family, arg = E.parse(member)
    return family == "scaled" and int(arg[0]) in (26, 51, 100)


# Where the plain estimator's d color falls short of A_MIN_CHANNELS on the restatement: Cornell's
# plain paths rarely reach its one light (`_reftrace.GLOW`), so L_{k+1} is 0 below most bounces.
# (member, samples) -> the non-zero d color channels measured on the restatement; the floor there is
# half of it, rounded down. Every other member, mode and sample count keeps A_MIN_CHANNELS in both
# tables: on Cornell, plain, the doubled members (62-74) and the 2^40 sheet (78 / 88) at both sample
# counts, and vertex_2^60/d (30), maxfloat/s (39) and far_light_big/30 and /62 (30) at 3 samples.
PLAIN_COLOR_SHORT = {
    ("cornell/scaled/-12", 1): 18, ("cornell/scaled/-12", 3): 27,
    ("cornell/scaled/20", 1): 1, ("cornell/scaled/20", 3): 16,
    ("cornell/degenerate", 1): 18, ("cornell/degenerate", 3): 27,
    ("cornell/outlier/vertex_2^60/d", 1): 14,
    ("cornell/outlier/maxfloat/s", 1): 20,
    ("cornell/far_light/65", 1): 18, ("cornell/far_light/65", 3): 27,
    ("cornell/far_light/110", 1): 12, ("cornell/far_light/110", 3): 26,
    ("cornell/far_light_big/30", 1): 18,
    ("cornell/far_light_big/62", 1): 18,
    ("cornell", 1): 6,  # `big_dir_rays` on the base (192 rays, 1 sample)
}


def channel_floors(member: str, mode: str, spp: int) -> tuple:
    """(floor of d color, floor of d emit) in non-zero channels."""
    short = PLAIN_COLOR_SHORT.get((member, spp)) if mode == "plain" else None
    return (A_MIN_CHANNELS if short is None else short // 2), A_MIN_CHANNELS


def channel_floor(member: str, mode: str, spp: int, channels) -> bool:
    lo = channel_floors(member, mode, spp)
    return channels[COLOR] >= lo[COLOR] and channels[EMIT_K] >= lo[EMIT_K]


# B: crafted LCG states, large and small directions, non-finite rays
STATE_CASES = tuple((m, k) for m in EL.STATE_MEMBERS_GPU for k in ("edge", "tie"))
BIG_BASES = EL.LIGHT_BASES
NONFINITE_SCENE, NONFINITE_N, NONFINITE_AT = "random_7_300", 257, 60  # rays 60 .. 75: across the first wave's end
# C: edge members along camera rays
C_MEMBERS = ("cornell/far_camera/61", "cornell/scaled/20", "random_4_150/doubled/base", "cornell/degenerate",
             "random_4_150/scaled/-12", "cornell/far_light/65")
C_RES, C_SPP = (16, 12), 2
C_CHUNKED = "cornell/degenerate"  # once more with PT_RENDER_GRAD_CHUNK=1: two launches
C_MIN_CHANNELS = 30
# D, E: edge values on cornell+glow
D_SCENE, D_N, D_SPP, D_SEED = "cornell+glow", 257, 3, 1
D_RES = (33, 17)
D_RENDER_MODES = ("plain", "nee+mis")
# the floors of a ray-form run of D at seed D_SEED. The restatement gives, over the three modes,
# E1: 1221-1252 terms of zeros alone, 672-691 with a subnormal channel, 49-51 NaN / 15-30 +inf /
# 9-11 -inf channels and 94-106 finite non-zero ones; E2: 914-1031, 592-653, 102-103 / 7-13 / 9-10
# and 60-64
D_FLOORS = dict(zero_terms=100, subnormal_terms=100, per_class=5, finite_nonzero=50)
# render_grad at D_RES, D_SPP samples, RENDER_SEED: each floor at most half of the least the
# restatement gives over E1, E2 and D_RENDER_MODES: 2566-3730 terms of zeros alone, 1177-1389 with a
# subnormal channel, 49-135 NaN / 22-83 +inf / 3-9 -inf channels and 21-60 finite non-zero ones
D_RENDER_FLOORS = dict(zero_terms=1000, subnormal_terms=500, nan=20, pinf=10, ninf=1, finite_nonzero=10)
# F: every placement
F_SCENES = ("random_7_300", "cornell+glow")
F_CALLS = (("trace_grad", "plain"), ("trace_nee_grad", "nee+mis"), ("render_grad", "plain"), ("render_grad", "nee+mis"))
F_N, F_SPP = 257, 3


# ---------------------------------------------------------------- scenes
def edge_member(member: str) -> bool:
    return "+" not in member


@functools.lru_cache(maxsize=None)
def arrays(member: str):
    """(verts, mtype, mvals, nodes, idx) with the oracle's tree."""
    if edge_member(member):
        return E.arrays(member)[1:]
    verts, nodes, idx, mtype, mvals = RT.scene_arrays(member)
    return verts, mtype, mvals, nodes, idx


def make_scene(member: str, res):
    return E.make(member, tuple(res)) if edge_member(member) else RT.make_scene(member, tuple(res))


def num_tris(member: str) -> int:
    return arrays(member)[2].shape[0]


# ---------------------------------------------------------------- ray sets
@functools.lru_cache(maxsize=None)
def nonfinite_set():
    o, d = RT.rays(NONFINITE_SCENE, NONFINITE_N)
    o, d = o.copy(), d.copy()
    no, nd = RW.nonfinite_rays()
    o[NONFINITE_AT:NONFINITE_AT + 16], d[NONFINITE_AT:NONFINITE_AT + 16] = no, nd
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def rays_of(member: str, rays: tuple):
    """A caller's ray set by key: (origins, directions, explicit states or None).
    ("query",) `_edgescenes.query_rays(member)`; ("state", kind) `_edgelights.state_rays`;
    ("big",) `_edgelights.big_dir_rays`; ("nonfinite",) `nonfinite_set`; ("set", n) the first n of
    `_reftrace.rays`; ("one", n, i) ray i of that set alone."""
    kind = rays[0]
    if kind == "query":
        o, d = E.query_rays(member)
        return o, d, None
    if kind == "state":
        return EL.state_rays(member, rays[1])
    if kind == "big":
        o, d, _ = EL.big_dir_rays(member)
        return o, d, None
    if kind == "nonfinite":
        o, d = nonfinite_set()
        return o, d, None
    o, d = RT.rays(member, rays[1])
    if kind == "one":
        i = rays[2]
        return np.ascontiguousarray(o[i:i + 1]), np.ascontiguousarray(d[i:i + 1]), None
    assert kind == "set"
    return np.ascontiguousarray(o), np.ascontiguousarray(d), None


def _paths_of(member: str, rays: tuple, spp: int, seed: int):
    """(origins, directions, states) of every path, path i * spp + s = sample s of ray (pixel) i."""
    if rays[0] == "camera":  # ("camera", res)
        sc = make_scene(member, rays[1])
        per = [RR.camera_rays(sc, seed, s) for s in range(spp)]
        return tuple(np.ascontiguousarray(np.stack([p[q] for p in per], axis=1).reshape((-1, 3) if q < 2 else (-1,)))
                     for q in range(3))
    o, d, st = rays_of(member, rays)
    if st is not None:
        assert spp == 1
        return o, d, st
    return np.repeat(o, spp, axis=0), np.repeat(d, spp, axis=0), RT.sample_seeds(o.shape[0], spp, seed).reshape(-1)


def max_spp(rays: tuple) -> int:
    """The sample count a set is walked at (smaller counts are slices)."""
    return {"query": 3, "state": 1, "big": 1, "nonfinite": 3, "set": 3, "one": 1, "camera": 0}[rays[0]]


@functools.lru_cache(maxsize=None)
def _walked(member: str, rays: tuple, spp: int, seed: int, mode: str):
    verts, mtype, mvals, nodes, idx = arrays(member)
    o, d, st = _paths_of(member, rays, spp, seed)
    if mode == "plain":
        return RT.walk_paths(nodes, idx, verts, mtype, mvals, o, d, st, DEPTH)
    return NG.walk(nodes, idx, verts, mtype, mvals, o, d, st, DEPTH, mode == "nee+mis")


def _every(W, step: int):
    """Sample 0 of every ray of a walk of `step` samples a ray."""
    cut = lambda a: a[:, ::step] if isinstance(a, np.ndarray) and a.ndim == 2 and a.shape[0] == DEPTH else a  # noqa: E731
    if isinstance(W, RT.Paths):
        return RT.Paths(W.tri[:, ::step], W.cos[:, ::step], W.state[:, ::step], W.init[::step], W.mtype, W.mvals)
    return W._replace(**{k: cut(getattr(W, k)) for k in ("hit", "kind", "cos", "light", "g", "wb", "traced", "shadow", "drew")})


def walked(member: str, rays: tuple, spp: int, seed: int, mode: str):
    top = max_spp(rays) or spp
    assert spp in (1, top), (rays, spp)
    W = _walked(member, rays, top, seed, mode)
    return W if spp == top else _every(W, top)


# ---------------------------------------------------------------- edge values
@functools.lru_cache(maxsize=None)
def busy(member: str, rays: tuple, spp: int, seed: int, mode: str):
    """The twelve triangles with the most terms (both tables together) of the mode's restatement at
    the scene's own materials, most first (ties: the lower index)."""
    n = _paths_of(member, rays, spp, seed)[0].shape[0] // spp
    W = walked(member, rays, spp, seed, mode)
    t = (RG if mode == "plain" else NG).path_terms(W, DEPTH, np.ones((n, 3), dtype=F32), spp)
    cnt = np.bincount(t.tri, minlength=num_tris(member))
    order = np.argsort(-cnt, kind="stable")[:12]
    assert cnt[order[-1]] > 0
    return tuple(int(x) for x in order)


def edge_grad(n: int, which: str) -> np.ndarray:
    """E1: `_refgrad.grad_rgb` with rows 0::7 = 2^-140, 1::7 = 2^100, 2::7 = 0 and channel 1 of rows
    3::7 = -0; E2: and rows 4::31 = 3e38."""
    g = RG.grad_rgb(n).copy()
    g[0::7] = F32(2.0 ** -140)
    g[1::7] = F32(2.0 ** 100)
    g[2::7] = F32(0)
    g[3::7, 1] = F32(-0.0)
    if which == "E2":
        g[4::31] = F32(3e38)
    return g


def edge_mats(member: str, b: tuple, which: str):
    """(color, emit): `_refgrad.overrides` with the rows of the busy triangles b set to zeros,
    subnormals, -0, negative and huge values (E1), and to inf, NaN and -inf as well (E2)."""
    color, emit = RG.overrides(num_tris(member))
    inf, nan = F32(np.inf), F32(np.nan)
    color[b[0]] = 0
    color[b[1]] = (1e-40, -0.0, 0.5)
    color[b[2]] = F32(2.0 ** 40)
    emit[b[2]] = F32(2.0 ** 60)
    emit[b[3]] = (-3, 0, 1e-44)
    color[b[4]] = F32(-0.75)
    if which == "E2":
        color[b[5]] = (inf, 0.5, 0.5)
        emit[b[6]] = (0.5, nan, 0.5)
        emit[b[7]] = (0.5, 0.5, -inf)
    return color, emit


def inputs(member: str, rays: tuple, spp: int, seed: int, grad: str, mats, mode: str = "plain"):
    """(grad_rgb (n, 3), color or None, emit or None) of a call. grad: "rgb" (`_refgrad.grad_rgb`), "E1",
    "E2"; mats: None (the scene's), "overrides", "E1", "E2", or ("E1", "color") / ("E1", "emit"): that
    one override alone."""
    n = _paths_of(member, rays, spp, seed)[0].shape[0] // spp
    g = RG.grad_rgb(n) if grad == "rgb" else edge_grad(n, grad)
    if mats is None:
        return g, None, None
    if mats == "overrides":
        return (g,) + RG.overrides(num_tris(member))
    which, only = (mats, None) if isinstance(mats, str) else mats
    # a single path takes the busy triangles of the whole set (frame) it belongs to
    if rays[0] == "one":
        b = busy(member, ("set", D_N), D_SPP, D_SEED, mode)
    elif rays == ("camera", (1, 1)):
        b = busy(member, ("camera", D_RES), D_SPP, RENDER_SEED, mode)
    else:
        b = busy(member, rays, spp, seed, mode)
    color, emit = edge_mats(member, b, which)
    return g, (None if only == "emit" else color), (None if only == "color" else emit)


# ---------------------------------------------------------------- expected values
class Expected:
    """What one call must return (hashed by identity: `terms` hands out one object per case)."""

    def __init__(self, t, case, rgb, rays, shadow, draws, tris):
        self.t = t            # RG.Terms: every term, in (path, k) order
        self.case = case      # `_refneegrad`'s case of every term (None: plain)
        self.rgb = rgb        # (n, 3): the float32 in-order mean of each ray's samples
        self.rays = rays      # path and shadow segments
        self.shadow, self.draws, self.tris = shadow, draws, tris


@functools.lru_cache(maxsize=None)
def terms(member: str, rays: tuple, mode: str, spp: int = 1, seed: int = SEED, grad: str = "rgb", mats=None,
          depth: int = DEPTH) -> Expected:
    W = walked(member, rays, spp, seed, mode)
    g, color, emit = inputs(member, rays, spp, seed, grad, mats, mode)
    if mode == "plain":
        t = RG.path_terms(W, depth, g, spp, color, emit)
        return Expected(t, None, RG.mean_rgb(t, spp), RR._segments(W, depth), 0, 0, num_tris(member))
    nt = NG.path_terms(W, depth, g, spp, color, emit)
    t = RG.Terms(nt.kind, nt.tri, nt.val, nt.path, nt.rgb)
    return Expected(t, nt.case, RG.mean_rgb(t, spp), nt.segments, nt.shadow, nt.draws, num_tris(member))


class Summary(NamedTuple):
    S: RG.Summary    # `_refgrad.summarize` of the requested terms with every non-finite channel value taken as 0
    cls: np.ndarray  # (2, T, 3) FINITE / NAN / PINF / NINF: the class of the sum of the channel's terms
    zero_terms: int       # terms with three +-0 channels
    subnormal_terms: int  # terms with a subnormal float32 channel


def kinds_of(want) -> tuple:
    return tuple(k for k, name in ((COLOR, "color"), (EMIT_K, "emit")) if name in want)


def summarize(X: Expected, want=WANT_BOTH) -> Summary:
    return _summarize(X, kinds_of(want))


@functools.lru_cache(maxsize=256)
def _summarize(X: Expected, kinds: tuple) -> Summary:
    sel = np.isin(X.t.kind, kinds)
    kind, tri, val = X.t.kind[sel], X.t.tri[sel], X.t.val[sel].astype(F32)
    seen = np.zeros((3, 2, X.tris, 3), dtype=bool)  # NaN, +inf, -inf among the channel's terms
    for q, hit in enumerate((np.isnan(val), val == np.inf, val == -np.inf)):
        for c in range(3):
            seen[q, kind[hit[:, c]], tri[hit[:, c]], c] = True
    cls = np.zeros((2, X.tris, 3), dtype=np.int8)
    cls[seen[1]] = PINF
    cls[seen[2]] = NINF
    cls[seen[0] | (seen[1] & seen[2])] = NAN
    fin = np.where(np.isfinite(val), val, F32(0))
    S = RG.summarize(RG.Terms(kind, tri, fin, X.t.path[sel], X.t.rgb), X.tris)
    tiny = np.finfo(F32).tiny
    return Summary(S, cls, int((val == 0).all(axis=1).sum()), int(((val != 0) & (np.abs(val) < tiny)).any(axis=1).sum()))


def class_counts(Z: Summary) -> dict:
    """What the non-vacuity conditions count: channels of each class, and finite non-zero ones."""
    return dict(nan=int((Z.cls == NAN).sum()), pinf=int((Z.cls == PINF).sum()), ninf=int((Z.cls == NINF).sum()),
                finite_nonzero=int(((Z.cls == FINITE) & (Z.S.exact != 0)).sum()), zero_terms=Z.zero_terms,
                subnormal_terms=Z.subnormal_terms, terms=Z.S.terms)


def nonzero_channels(Z: Summary, kind: int) -> int:
    return int(((Z.cls[kind] != FINITE) | (Z.S.exact[kind] != 0)).sum())


def assert_floors(Z: Summary, floors: dict, what=""):
    c = class_counts(Z)
    for k in ("zero_terms", "subnormal_terms", "finite_nonzero", "nan", "pinf", "ninf"):
        assert c[k] >= floors.get(k, floors.get("per_class")), (what, k, c)


COUNTS = ("rays", "paths")
LIGHT_COUNTS = ("shadow_rays", "light_draws", "lights")


def assert_call(got: dict, st: dict, X: Expected, want=WANT_BOTH, what="", host=None, st_h=None, shape=None):
    """One call's result and stats against the restatement X, and against the host form's
    (host, st_h) where given. `shape`: (H, W) of a render_grad image."""
    Z = summarize(X, want)
    assert set(got) == set(want), (what, sorted(got), want)
    if "rgb" in want:
        rgb = np.asarray(got["rgb"])
        assert rgb.shape == ((X.rgb.shape[0], 3) if shape is None else (shape[0], shape[1], 3)), (what, rgb.shape)
        RT.assert_same(rgb.reshape(-1, 3), X.rgb, what + ": rgb vs the restatement")
        if host is not None:
            RT.assert_same(rgb.reshape(-1, 3), np.asarray(host["rgb"]).reshape(-1, 3), what + ": rgb vs the host form")
    assert st["terms"] == Z.S.terms, (what, st["terms"], Z.S.terms)
    assert st["rays"] == X.rays, (what, st["rays"], X.rays)
    if X.case is not None:  # a mode with lights: the stats must carry the light counts
        assert st["shadow_rays"] == X.shadow and st["light_draws"] == X.draws, (what, st, X.shadow, X.draws)
    if st_h is not None:
        keys = COUNTS + (LIGHT_COUNTS if X.case is not None else ())
        assert {k: st[k] for k in keys} == {k: st_h[k] for k in keys} and st["terms"] == st_h["terms"], (what, st, st_h)
    for kind, name in ((COLOR, "color"), (EMIT_K, "emit")):
        if name not in want:
            continue
        a = np.asarray(got[name], dtype=np.float64)
        assert a.shape == (X.tris, 3), (what, name, a.shape)
        cls = Z.cls[kind]
        got_cls = np.select([np.isnan(a), a == np.inf, a == -np.inf], [NAN, PINF, NINF], FINITE)
        bad = np.argwhere(got_cls != cls)
        assert bad.size == 0, (f"{what}: d {name}: {len(bad)} channels of the wrong class (0 finite, 1 NaN, 2 +inf, 3 -inf), "
                               f"first {bad[:4].tolist()}: got {[a[tuple(b)] for b in bad[:4]]}, "
                               f"want class {[int(cls[tuple(b)]) for b in bad[:4]]}")
        fin = cls == FINITE
        err = np.abs(np.where(fin, a, 0.0) - Z.S.exact[kind])
        bad = np.argwhere(fin & ~(err <= Z.S.tol[kind]))
        assert bad.size == 0, (f"{what}: d {name}: {len(bad)} entries outside the tolerance, first {bad[:3].tolist()}: "
                               f"got {[a[tuple(b)] for b in bad[:3]]}, want {[Z.S.exact[kind][tuple(b)] for b in bad[:3]]}, "
                               f"tol {[Z.S.tol[kind][tuple(b)] for b in bad[:3]]}")
    return Z


# ---------------------------------------------------------------- doubled members
def tie_losers(member: str, X: Expected) -> np.ndarray:
    """The triangles of a doubled member that lose their tie: triangles 2 i and 2 i + 1 are the same
    three points, every ray that reaches them ties, and the walk keeps one of them. A pair both of
    whose triangles get a term (its two copies sit in different leaves, and the ray decides which
    comes first) has no loser."""
    cnt = np.bincount(X.t.tri, minlength=X.tris).reshape(-1, 2)
    lose = np.zeros_like(cnt, dtype=bool)
    lose[:, 0] = (cnt[:, 0] == 0) & (cnt[:, 1] > 0)
    lose[:, 1] = (cnt[:, 1] == 0) & (cnt[:, 0] > 0)
    return np.flatnonzero(lose.reshape(-1))


# ---------------------------------------------------------------- how a test calls
def ray_call(obj, member: str, rays: tuple, mode: str, spp: int = 1, seed: int = SEED, grad: str = "rgb", mats=None,
             want=WANT_BOTH, depth: int = DEPTH):
    """trace_grad / trace_nee_grad of `obj` (a ptamd.BVH: the host form; a ptamd.Renderer: the device)."""
    o, d, st = rays_of(member, rays)
    g, color, emit = inputs(member, rays, spp, seed, grad, mats, mode)
    kw = dict(samples=spp, seed=seed, states=st, color=color, emit=emit, want=want)
    if mode == "plain":
        return obj.trace_grad(o, d, g, depth, **kw)
    return obj.trace_nee_grad(o, d, g, depth, mis=mode == "nee+mis", **kw)


def render_call(obj, cam, member: str, res, mode: str, spp: int, seed: int = RENDER_SEED, grad: str = "rgb", mats=None,
                want=WANT_BOTH, depth: int = DEPTH):
    W, H = res
    g, color, emit = inputs(member, ("camera", tuple(res)), spp, seed, grad, mats, mode)
    return obj.render_grad(cam, g.reshape(H, W, 3), spp, depth, seed=seed, color=color, emit=emit, want=want, **RR.mode_kw(mode))
