"""Light sampling at extreme scales, on exact ties and at the light table's edges (test
infrastructure, float32 throughout): the members of tests/_edgescenes.py that the light-sampling
tests run (LIGHT_MEMBERS, with the families far_light and far_light_big added for them), LCG
states crafted so that a path's first light draw sits on an edge of the draw's arithmetic
(`edge_states`, `cdf_tie_states`), caller rays with large and small finite directions
(`big_dir_rays`), and the expected values: `_refnee.walk` / `_refmis.walk` over
`_edgescenes.arrays(member)`'s oracle tree, cached. DESIGN.md §3.25 lists which family drives
which gate. Nothing here calls the library under test."""
from __future__ import annotations

import functools

import numpy as np

import _edgescenes as E
import _oracle as O
import _refmis as RM
import _refnee as RN
import _reftrace as RT
import _refwalk as RW

F32 = np.float32
LIGHT_BASES = ("cornell", "random_4_150")
SEED = 3
DEPTHS = (2, 5)
SAMPLES = (1, 3)
MAX_DEPTH, MAX_SAMPLES = max(DEPTHS), max(SAMPLES)


def _members():
    out = []
    for b in LIGHT_BASES:
        out += [f"{b}/scaled/{k}" for k in (-12, 20, 23, 25, 26)]
        out += [f"{b}/doubled/base", f"{b}/doubled/alt", f"{b}/degenerate", f"{b}/outlier/sheet_2^40/d",
                f"{b}/outlier/vertex_2^60/d", f"{b}/far_camera/61"]
        out += [f"{b}/far_light/{k}" for k in (40, 63, 65, 100, 110, 120)]
        out += [f"{b}/far_light_big/{k}" for k in (30, 62)]
    return tuple(out + ["random_4_150/scaled/33", "cornell/scaled/22", "cornell/scaled/24"])


LIGHT_MEMBERS = _members()
# the members of the placement, render_nee and crafted-state tests
PLACEMENT_MEMBERS = ("cornell/scaled/20", "random_4_150/scaled/26", "cornell/far_light/65", "cornell/far_light/110",
                     "random_4_150/far_light/120", "random_4_150/doubled/alt", "cornell/degenerate")
RENDER_MEMBERS = ("cornell/far_camera/61", "cornell/scaled/20", "random_4_150/scaled/-12", "cornell/far_light/65",
                  "random_4_150/doubled/base")
STATE_MEMBERS_CPU = ("cornell", "random_4_150", "cornell/degenerate", "random_4_150/degenerate")
STATE_MEMBERS_GPU = ("cornell", "random_4_150", "random_4_150/degenerate")


def dim(member: str) -> bool:
    """Members where SHIFT_BIAS is absorbed or the areas overflow: few or no shadow segments."""
    _, family, arg = E.parse(member)
    return family == "scaled" and int(arg[0]) in (25, 26, 33)


@functools.lru_cache(maxsize=None)
def lights(member: str) -> RN.Lights:
    _, verts, mtype, mvals, _, _ = E.arrays(member)
    return RN.light_table(verts, mtype, mvals)


# ---------------------------------------------------------------- expected values
@functools.lru_cache(maxsize=None)
def seeds(n: int, samples: int = MAX_SAMPLES) -> np.ndarray:
    """pt_sample_seed(i, s, SEED): (n, samples); column s does not depend on `samples`."""
    st = RT.sample_seeds(n, samples, SEED)
    st.setflags(write=False)
    return st


def _walk(member: str, mis: bool, o, d, states, depth: int):
    _, verts, mtype, mvals, nodes, idx = E.arrays(member)
    return (RM if mis else RN).walk(nodes, idx, verts, mtype, mvals, o, d, states, depth)


@functools.lru_cache(maxsize=None)
def sample_paths(member: str, mis: bool, s: int):
    """Sample s of the member's query rays, walked to MAX_DEPTH."""
    o, d = E.query_rays(member)
    return _walk(member, mis, o, d, seeds(o.shape[0])[:, s], MAX_DEPTH)


def radiance(P, depth: int):
    return RM.radiance(P, depth) if isinstance(P, RM.Paths) else RN.radiance(P, depth)


@functools.lru_cache(maxsize=None)
def expected(member: str, mis: bool, depth: int, samples: int):
    """(rgb (n, 3): the float32 sum of the samples in order from +0, divided by float32(samples);
    path and shadow segments; shadow segments; light draws) of the member's query rays."""
    n = E.query_rays(member)[0].shape[0]
    acc = np.zeros((n, 3), dtype=F32)
    segs = sh = dr = 0
    with np.errstate(all="ignore"):
        for s in range(samples):
            rgb, a, b, c = radiance(sample_paths(member, mis, s), depth)
            acc = acc + rgb
            segs, sh, dr = segs + int(a.sum()), sh + int(b.sum()), dr + int(c.sum())
        out = (acc / F32(samples)).astype(F32) if samples > 1 else acc
    out.setflags(write=False)
    return out, segs, sh, dr


def lit_rays(rgb) -> int:
    return int((RW.bits(rgb).reshape(-1, 3) != 0).any(axis=1).sum())


# ---------------------------------------------------------------- crafted LCG states
LCG_A, LCG_C = 1664525, 1013904223
LCG_A_INV = pow(LCG_A, -1, 1 << 32)


def lcg_prev(s, times: int = 1):
    """The state before s: (s - c) a^-1 mod 2^32, `times` times (the inverse of `_reftrace.lcg_step`)."""
    shape = np.shape(s)
    s = np.atleast_1d(np.asarray(s, dtype=np.uint64))  # arrays wrap mod 2^64 silently
    for _ in range(times):
        s = ((s + np.uint64((1 << 32) - LCG_C)) * np.uint64(LCG_A_INV)) & np.uint64(0xFFFFFFFF)
    return s.astype(np.uint32).reshape(shape)


def draws(states, count: int = 3):
    """(states (n, count) uint32, draws (n, count) float32) of the next `count` draws, by oracle_lcg."""
    states = np.asarray(states, dtype=np.uint32).reshape(-1)
    s = np.zeros((states.shape[0], count), dtype=np.uint32)
    x = np.zeros((states.shape[0], count), dtype=F32)
    f = O.lib().oracle_lcg
    for i, s0 in enumerate(states.tolist()):
        f(int(s0), count, s[i].ctypes.data, x[i].ctypes.data)
    return s, x


@functools.lru_cache(maxsize=None)
def one_edge() -> int:
    """The first LCG state whose draw is exactly 1.0f, located with oracle_lcg among the states
    from 0xFFFFFE00 up (the draws are monotone in the state, checked)."""
    cand = np.arange(0xFFFFFE00, 1 << 32, dtype=np.uint64).astype(np.uint32)
    s, x = draws(lcg_prev(cand), 1)
    assert np.array_equal(s[:, 0], cand) and (np.diff(x[:, 0]) >= 0).all() and x[0, 0] < 1 and x[-1, 0] == 1
    return int(cand[np.flatnonzero(x[:, 0] == F32(1))[0]])


@functools.lru_cache(maxsize=None)
def edge_states(n: int):
    """(states (n,), class (n,), target (n,)): ray i's first, second or third draw (class 0, 1, 2)
    of its first light draw is the one the LCG state `target` produces, targets 0xFFFFFFFF, the
    first state that yields 1.0f, the one before it (0xFFFFFF80 and 0xFFFFFF7F are the candidates;
    `one_edge` locates them), 0 and 1, the fifteen combinations cycled over the rays. A caller's
    ray makes no draw before its first vertex, so the state given is the one that vertex's light
    draw starts from."""
    e = one_edge()
    assert e in (0xFFFFFF80, 0xFFFFFF7F + 1)
    targets = np.array([0xFFFFFFFF, e, e - 1, 0, 1], dtype=np.uint32)
    cls = np.arange(n) % 3
    tgt = targets[(np.arange(n) // 3) % 5]
    st = np.array([lcg_prev(t, c + 1) for t, c in zip(tgt, cls)], dtype=np.uint32)
    s, _ = draws(st, 3)
    assert np.array_equal(s[np.arange(n), cls], tgt)
    for a in (st, cls, tgt):
        a.setflags(write=False)
    return st, cls, tgt


def first_draw(lt: RN.Lights, states):
    """What the first light draw from `states` does, restated: (xa, last: the pick falls through
    to the last light because no cdf_j > xa, folded: x2 + x3 > 1)."""
    _, x = draws(states, 3)
    with np.errstate(all="ignore"):
        xa = (x[:, 0] * lt.area).astype(F32)
        return xa, xa >= lt.cdf[-1], (x[:, 1] + x[:, 2]).astype(F32) > F32(1)


def cdf_tie_states(lt: RN.Lights, n: int):
    """(states (n,), j (n,), side (n,)): states whose first draw x1 has F32(x1 A) equal to cdf[j]
    bit for bit (side 0: the pick's strict compare passes cdf[j] over), and for each the state of
    the float x1 just below (side 1), cycled over n rays. Found by trying the states around
    cdf[j] / A 2^32, every 2^6-th over 2^14 (a float32 draw near 1/2 covers 2^8 states). A j
    that no state ties with is left out; None when no j ties."""
    assert lt.tri.size >= 2
    found = []
    for j in range(lt.tri.size - 1):
        c = int(float(lt.cdf[j]) / float(lt.area) * 2.0 ** 32)
        cand = np.unique(np.clip(c + 64 * np.arange(-128, 129), 0, (1 << 32) - 1)).astype(np.uint64)
        x1 = cand.astype(np.uint32).astype(F32) / F32(4294967296.0)
        tie = np.flatnonzero(RW.bits(x1 * lt.area) == RW.bits(lt.cdf[j:j + 1])[0])
        if tie.size:
            below = np.flatnonzero(x1 < x1[tie[0]])
            found.append((int(cand[tie[0]]), j, 0))
            if below.size:
                found.append((int(cand[below[-1]]), j, 1))
    if not found:
        return None
    rows = [found[i % len(found)] for i in range(n)]
    st = lcg_prev(np.array([r[0] for r in rows], dtype=np.uint32))
    j, side = np.array([r[1] for r in rows]), np.array([r[2] for r in rows])
    # the oracle's own draw agrees with the search's arithmetic
    _, x = draws(st, 1)
    xa = (x[:, 0] * lt.area).astype(F32)
    assert np.array_equal(RW.bits(xa[side == 0]), RW.bits(lt.cdf[j[side == 0]]))
    assert (xa[side == 1] < lt.cdf[j[side == 1]]).all()
    return st, j, side


N_STATE_RAYS = 240


@functools.lru_cache(maxsize=None)
def state_rays(member: str, kind: str):
    """(origins, directions, states) of the crafted-state runs: the first N_STATE_RAYS of
    `_refwalk.ray_set(2000, 256)` with `edge_states` ("edge") or `cdf_tie_states` ("tie")."""
    o, d = RW.ray_set(2000, 256)
    o, d = np.ascontiguousarray(o[:N_STATE_RAYS]), np.ascontiguousarray(d[:N_STATE_RAYS])
    if kind == "edge":
        st = edge_states(N_STATE_RAYS)[0]
    else:
        found = cdf_tie_states(lights(member), N_STATE_RAYS)
        assert found is not None, member
        st = found[0]
    for a in (o, d):
        a.setflags(write=False)
    return o, d, st


@functools.lru_cache(maxsize=None)
def state_paths(member: str, kind: str, mis: bool):
    o, d, st = state_rays(member, kind)
    return _walk(member, mis, o, d, st, MAX_DEPTH)


# ---------------------------------------------------------------- large and small finite directions
BIG_EXPONENTS = (61, 90, 100, 101, 110, 126, -61, -90, -101, -110, -126)
N_BIG, N_BIG_UNIFORM = 192, 132


@functools.lru_cache(maxsize=None)
def big_dir_rays(base: str):
    """N_BIG rays from rays of `_refwalk.ray_set` that hit `base`: N_BIG_UNIFORM with the whole
    direction times 2^e, the others with the component of least magnitude times 2^e, e cycled over
    BIG_EXPONENTS: |1 / d| on both sides of 2^60 and of 2^-100, |d| on both sides of 2^±126.
    A hit's t scales by 2^-e, so the source rays are hits with 1 <= t <= 700: t 2^-e stays a
    normal float for every e > 0, and below 1e30 for e >= -90. Returns (origins, directions, e)."""
    _, verts, _, _, nodes, idx = E.arrays(base)
    o, d = RW.ray_set(2100, 512)
    t, tri = RW.ref_walk(nodes, idx, verts, o, d)
    # (a component under 1, so that 2^-61 d has |1 / d| past 2^60)
    ok = np.flatnonzero((tri >= 0) & (t >= 1) & (t <= 700) & (d != 0).all(axis=1) & (np.abs(d).min(axis=1) < 1))[:N_BIG]
    assert ok.size == N_BIG, (base, ok.size)
    o, d = o[ok].copy(), d[ok].copy()
    e = np.array([BIG_EXPONENTS[i % len(BIG_EXPONENTS)] for i in range(N_BIG)])
    with np.errstate(all="ignore"):
        for i in range(N_BIG):
            s = F32(2.0) ** F32(e[i])
            if i < N_BIG_UNIFORM:
                d[i] = d[i] * s
            else:
                a = int(np.abs(d[i]).argmin())
                d[i, a] = d[i, a] * s
    assert np.isfinite(d).all()
    # the kernels choose the slab form per wave: the positive exponents first, so that the first
    # 64 rays are a wave wholly inside the fast form's domain and the last 64 one wholly outside
    order = np.argsort(e < 0, kind="stable")
    o, d, e = o[order], d[order], e[order]
    with np.errstate(all="ignore"):
        worst = np.abs(F32(1) / d).max(axis=1)
    assert (worst[:64] <= F32(2.0 ** 60)).all() and (worst[-64:] > F32(2.0 ** 60)).all()
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    for a in (o, d, e):
        a.setflags(write=False)
    return o, d, e


@functools.lru_cache(maxsize=None)
def big_dir_expected(base: str):
    """(t, tri) of `big_dir_rays` under `_refwalk.ref_walk`."""
    _, verts, _, _, nodes, idx = E.arrays(base)
    o, d, _ = big_dir_rays(base)
    t, tri = RW.ref_walk(nodes, idx, verts, o, d)
    t.setflags(write=False)
    tri.setflags(write=False)
    return t, tri


@functools.lru_cache(maxsize=None)
def big_dir_paths(base: str, mis: bool):
    o, d, _ = big_dir_rays(base)
    return _walk(base, mis, o, d, seeds(N_BIG)[:, 0], MAX_DEPTH)
