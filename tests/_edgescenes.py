"""Scenes outside the kernels' fast domains and scenes with exact ties (test infrastructure,
float32 throughout): tests/test_edge_scenes_cpu.py pins the host library, the oracle and the
compiled reference on them, tests/test_edge_scenes_gpu.py renders and queries them on every
kernel path. DESIGN.md §3.17 lists which family drives which gate.

A member is named "<base>/<family>/<argument>":
  outlier   the base plus one triangle (DIFFUSE "d" or SPECULAR roughness 0.2 "s") with a vertex
            at 2^60, far away in the plane x = 2^60, or a sheet through the room at y = 250 / 260
            with corners at 2^40, 2^62 or 3e38;
  scaled    every vertex and the camera position times 2^k;
  doubled   every triangle twice in a row, the base material and an alternate, in both orders;
  degenerate  the base plus three EMIT triangles: a point, a segment and a 2^-14-thin sliver;
  far_camera  the base seen along +z from z = -2^k through a field of view of 600 / 2^k radians:
            camera rays with |o| past 2^60 (k = 61) and 2^64 (k = 66) and |1 / d| near 2^60 that
            still hit the scene (the scaled family reaches such origins only where every ray misses).
Two more families serve the light-sampling tests only (tests/_edgelights.py; not in MEMBERS):
  far_light      the base plus one EMIT triangle of side 100 at z = -2^k: shadow segments whose
                 unnormalised direction has a component near 2^k;
  far_light_big  the same with z = -2^k and sides 2^(k - 10): an area that absorbs the base's
                 lights in the table's running sum (k = 30) or overflows and is dropped (k = 62).
No NaN or infinite vertex: the builder rejects them."""
from __future__ import annotations

import functools

import numpy as np

import _oracle as O
import _reftrace as RT
import _refwalk as RW

F32 = np.float32
BASES = ("cornell", "random_2_40", "random_4_150")
FLAT_BASES = ("cornell", "random_2_40")  # <= 64 leaves: the flat leaf list
OUTLIER_KINDS = ("vertex_2^60", "far_small", "sheet_2^62", "maxfloat", "sheet_2^40")
SCALES = (-12, 20, 33, 34, 51, 100)
ONE_LEAF_KINDS = ("sheet_2^62", "maxfloat")  # the SAH costs overflow: one root leaf holds every triangle
BIG_KINDS = ("vertex_2^60", "far_small", "sheet_2^62", "maxfloat")  # a coordinate >= 2^60


def _f(x) -> float:
    return float(F32(x))


def base_scene(base: str, res):
    return RW.make_scene(base, tuple(res))


def _outlier_tri(kind: str):
    big = 2.0 ** 60
    if kind == "vertex_2^60":
        return ((big, 0.0, 0.0), (300.0, 600.0, 300.0), (300.0, 600.0, 310.0))
    if kind == "far_small":
        return ((big, 200.0, 200.0), (big, 300.0, 200.0), (big, 200.0, 300.0))
    y, g = {"sheet_2^62": (250.0, 2.0 ** 62), "maxfloat": (260.0, _f(3e38)), "sheet_2^40": (250.0, 2.0 ** 40)}[kind]
    return ((-g, y, -g), (g, y, -g), (0.0, y, g))


def outlier(base, kind: str, mat: str):
    """The 2^40 sheet is the one outlier that rays meet: |e1 x e2|^2 = 2^164 overflows, its unit
    normal is 0 and so is every cosine on it, so it reflects nothing. It emits a little, so that
    the pixels that see it are lit; the others do not emit (a dark base stays dark)."""
    from ptamd import scenes
    emit = tuple(_f(c) for c in (0.25, 0.125, 0.0625)) if kind == "sheet_2^40" else 0
    color = tuple(_f(c) for c in (0.7, 0.6, 0.5))
    m = (scenes.Material.make(scenes.DIFFUSE, color, emit) if mat == "d"
         else scenes.Material.make(scenes.SPECULAR, color, emit, _f(0.2)))
    sc = scenes.Scene(f"{base.name}/outlier/{kind}/{mat}", base.camera, list(base.tris), list(base.mats))
    sc.add([_outlier_tri(kind)], m)
    return sc


def scaled(base, k: int):
    """Every vertex and the camera position times 2^k, the product rounded to float32 (exact
    unless it leaves the normal range); fov and distance untouched."""
    from ptamd import scenes
    s = F32(2.0) ** F32(k)
    with np.errstate(all="ignore"):
        mul = lambda p: tuple(float(F32(c) * s) for c in p)  # noqa: E731
        c = base.camera
        cam = scenes.CameraSpec(mul(c.pos), c.forward, c.up, c.res, c.fov_deg, c.distance)
        tris = [tuple(mul(p) for p in t) for t in base.tris]
    assert np.isfinite(np.array(tris)).all()
    return scenes.Scene(f"{base.name}/scaled/{k}", cam, tris, list(base.mats))


def doubled(base, first: str):
    from ptamd import scenes
    alt = scenes.Material.make(scenes.DIFFUSE, tuple(_f(c) for c in (0.1, 0.9, 0.1)), tuple(_f(c) for c in (0.3, 0.0, 0.3)))
    sc = scenes.Scene(f"{base.name}/doubled/{first}", base.camera)
    for t, m in zip(base.tris, base.mats):
        for mm in ((m, alt) if first == "base" else (alt, m)):
            sc.add([t], mm)
    return sc


SLIVER = ((50.0, 250.0, 250.0), (500.0, 250.0, 250.0), (500.0, 250.0 + 2.0 ** -14, 250.0))


def degenerate(base):
    from ptamd import scenes
    sc = scenes.Scene(f"{base.name}/degenerate", base.camera, list(base.tris), list(base.mats))
    e = lambda r, g, b: scenes.Material.make(scenes.EMIT, 0, (r, g, b))  # noqa: E731
    p = (250.0, 200.0, 250.0)
    sc.add([(p, p, p)], e(5.0, 0.0, 0.0))                                                     # a point: NaN normal
    sc.add([((100.0, 100.0, 100.0), (200.0, 200.0, 200.0), (400.0, 400.0, 400.0))], e(0.0, 5.0, 0.0))  # a segment
    sc.add([SLIVER], e(2.0, 2.0, 4.0))
    return sc


FAR_CAMERAS = (61, 66)


def far_camera(base, k: int):
    import math
    from ptamd import scenes
    c = base.camera
    cam = scenes.CameraSpec((250.0, 250.0, -(2.0 ** k)), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), c.res,
                            _f(math.degrees(600.0 / 2.0 ** k)), 1.0)
    return scenes.Scene(f"{base.name}/far_camera/{k}", cam, list(base.tris), list(base.mats))


def far_light(base, k: int, side=100.0, family: str = "far_light"):
    """The base plus one EMIT triangle ((200, 200, z), (200 + side, 200, z), (200, 200 + side, z)),
    z = -2^k, emission (4, 2, 1): on Cornell that is the open side, so the room sees it."""
    from ptamd import scenes
    z = -(2.0 ** k)
    sc = scenes.Scene(f"{base.name}/{family}/{k}", base.camera, list(base.tris), list(base.mats))
    sc.add([((200.0, 200.0, z), (200.0 + side, 200.0, z), (200.0, 200.0 + side, z))],
           scenes.Material.make(scenes.EMIT, 0, (4.0, 2.0, 1.0)))
    return sc


def far_light_big(base, k: int):
    return far_light(base, k, 2.0 ** (k - 10), "far_light_big")


def _members():
    out = []
    for b in BASES:
        out += [f"{b}/outlier/{k}/{m}" for k in OUTLIER_KINDS for m in "ds"]
        out += [f"{b}/scaled/{k}" for k in SCALES]
        out += [f"{b}/doubled/{f}" for f in ("base", "alt")]
        out += [f"{b}/degenerate"]
        out += [f"{b}/far_camera/{k}" for k in FAR_CAMERAS]
    return tuple(out)


MEMBERS = _members()
# the members of the query, AOV and caller-ray tests
QUERY_MEMBERS = tuple(f"{b}/{m}" for b in ("cornell", "random_4_150")
                      for m in ("outlier/vertex_2^60/d", "outlier/sheet_2^62/s", "scaled/20", "scaled/33", "scaled/34",
                                "scaled/51", "doubled/base", "doubled/alt", "far_camera/61", "far_camera/66"))


def parse(member: str):
    base, family, *arg = member.split("/")
    return base, family, arg


def make(member: str, res):
    if "/" not in member:  # a base itself
        return base_scene(member, res)
    base, family, arg = parse(member)
    b = base_scene(base, res)
    if family == "outlier":
        return outlier(b, arg[0], arg[1])
    if family == "scaled":
        return scaled(b, int(arg[0]))
    if family == "doubled":
        return doubled(b, arg[0])
    if family == "far_camera":
        return far_camera(b, int(arg[0]))
    if family == "far_light":
        return far_light(b, int(arg[0]))
    if family == "far_light_big":
        return far_light_big(b, int(arg[0]))
    assert family == "degenerate" and not arg
    return degenerate(b)


def scale_of(member: str) -> np.float32:
    _, family, arg = parse(member)
    return F32(2.0) ** F32(int(arg[0])) if family == "scaled" else F32(1)


def coords_big(member: str) -> bool:
    """Whether a vertex coordinate reaches 2^60 (the host's coords_small is then false)."""
    _, family, arg = parse(member)
    return (family == "outlier" and arg[0] in BIG_KINDS) or (family == "scaled" and int(arg[0]) >= 51)


def one_leaf(member: str) -> bool:
    """Whether the builder's SAH costs overflow, so that one root leaf holds every triangle."""
    _, family, arg = parse(member)
    return (family == "outlier" and arg[0] in ONE_LEAF_KINDS) or (family == "scaled" and int(arg[0]) >= 51)


def far_rays(seed: int, n: int, scale):
    """Rays from 2^58 .. 2^67 away along an axis, tilted so that they cross the (scaled) room:
    origins on both sides of the 2^60 and 2^64 domain bounds, and 1 / d of the tilted components
    on both sides of 2^60."""
    rng = np.random.default_rng(seed)
    s = np.float64(scale)
    o = (rng.uniform(50, 450, (n, 3)) * s)
    d = np.zeros((n, 3))
    for i in range(n):
        a, sign, m = i % 3, (1.0 if (i // 3) % 2 else -1.0), 2.0 ** (58 + i % 10)
        d[i] = rng.uniform(-100, 100, 3) * s / m
        d[i, a] = sign
        o[i, a] = -sign * m
    return np.ascontiguousarray(o.astype(F32)), np.ascontiguousarray(d.astype(F32))


# Triangle::intersect rejects |a| < EPS with a = e1 . (d x e2) a float and EPS = 1e-6 a double
# (triangle.h:31): the floats 0x1.0c6f78p-20 and 0x1.0c6f7ap-20 (= 1e-6f) are below it, the next
# one, 0x1.0c6f7cp-20, is not.
EPS_BELOW = (float.fromhex("0x1.0c6f78p-20"), float.fromhex("0x1.0c6f7ap-20"))
EPS_ABOVE = float.fromhex("0x1.0c6f7cp-20")
N_NEAR, N_FAR, N_EPS = 256, 128, 3 * 32


def _tri_a(verts9, d):
    """a of Triangle::intersect (triangle.h:28-30) in float32, linalg.h's operation order."""
    e1, e2 = verts9[..., 3:6] - verts9[..., 0:3], verts9[..., 6:9] - verts9[..., 0:3]
    return RT._dot(e1, RT._cross(d, e2))


def eps_rays(member: str, o, d, tri, per_class: int = N_EPS // 3):
    """Rays on the threshold of the triangle test's EPS compare: for rays (o, d) that hit triangle
    tri, the direction rescaled (a is linear in d) until |a| on that triangle is exactly one of
    EPS_BELOW (the reference rejects the triangle: the ray goes on to whatever lies behind) or
    EPS_ABOVE (it accepts it). Returns (origins, directions, class 0 / 1 / 2, triangle), classes
    interleaved; found by trying the floats around the scale that the quotient suggests."""
    verts = arrays(member)[1]
    targets = EPS_BELOW + (EPS_ABOVE,)
    out = [[] for _ in targets]
    steps = np.arange(-300, 301)
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(tri >= 0):
            a0 = float(_tri_a(verts[tri[i]], d[i]))
            if not np.isfinite(a0) or abs(a0) < 1e-3:
                continue
            for c, tgt in enumerate(targets):
                if len(out[c]) >= per_class:
                    continue
                c0 = F32(tgt / abs(a0))
                # the floats around c0, 300 to either side
                cs = (c0.view(np.uint32) + steps).astype(np.uint32).view(F32)
                dd = (d[i][None, :] * cs[:, None]).astype(F32)
                ok = np.flatnonzero(np.abs(_tri_a(verts[tri[i]][None, :], dd)) == F32(tgt))
                if ok.size:
                    out[c].append((o[i], dd[ok[0]], c, tri[i]))
            if all(len(x) >= per_class for x in out):
                break
    # (at some scales one of the two floats below EPS is hardly ever reached: either one binds)
    assert len(out[0]) + len(out[1]) >= per_class and len(out[2]) >= per_class // 2, (member, [len(x) for x in out])
    rows = [r for k in range(per_class) for x in out for r in x[k:k + 1]]
    return (np.ascontiguousarray(np.array([r[0] for r in rows], dtype=F32)),
            np.ascontiguousarray(np.array([r[1] for r in rows], dtype=F32)),
            np.array([r[2] for r in rows]), np.array([r[3] for r in rows], dtype=np.int32))


@functools.lru_cache(maxsize=None)
def _query_rays(member: str):
    s = scale_of(member)
    o, d = RW.ray_set(2000 + len(member), N_NEAR)
    with np.errstate(all="ignore"):
        o = (o * s).astype(F32)
    fo, fd = far_rays(3000 + len(member), N_FAR, s)
    _, verts, _, _, nodes, idx = arrays(member)
    t, tri = RW.ref_walk(nodes, idx, verts, o, d)
    if (tri >= 0).sum() < 64:  # a scene that rays hardly hit (scales >= 2^33) has no threshold rays
        eo, ed, ec, et = np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, int), np.zeros(0, np.int32)
    else:
        eo, ed, ec, et = eps_rays(member, o, d, tri)
    o, d = np.ascontiguousarray(np.concatenate([o, fo, eo])), np.ascontiguousarray(np.concatenate([d, fd, ed]))
    for a in (o, d, ec, et):
        a.setflags(write=False)
    return o, d, ec, et


def query_rays(member: str):
    """N_NEAR rays of `_refwalk.ray_set` with the origins times the member's scale, N_FAR
    `far_rays`, then (where the scene is hit at all) N_EPS `eps_rays`."""
    return _query_rays(member)[:2]


def eps_classes(member: str):
    """(class, triangle) of the threshold rays at the end of `query_rays`."""
    return _query_rays(member)[2:]


@functools.lru_cache(maxsize=None)
def arrays(member: str, res=(16, 12)):
    """(scene, verts, mtype, mvals, nodes, idx) with the oracle's tree; read-only."""
    sc = make(member, res)
    verts, mtype, mvals = O.pack_scene(sc)
    nodes, idx = O.bvh_build(verts)
    for a in (verts, mtype, mvals, nodes, idx):
        a.setflags(write=False)
    return sc, verts, mtype, mvals, nodes, idx


@functools.lru_cache(maxsize=None)
def query_expected(member: str):
    """(origins, directions, t, tri) of the member's query rays under `_refwalk.ref_walk`."""
    _, verts, _, _, nodes, idx = arrays(member)
    o, d = query_rays(member)
    t, tri = RW.ref_walk(nodes, idx, verts, o, d)
    for a in (o, d, t, tri):
        a.setflags(write=False)
    return o, d, t, tri


def lit_share(img: np.ndarray) -> float:
    """Share of pixels with a non-zero channel."""
    px = np.ascontiguousarray(img, dtype=F32).reshape(-1, 3)
    return float((px.view(np.uint32) != 0).any(axis=1).mean())


def first_hit_rate(member: str, res=(16, 12), seed: int = 1) -> float:
    """Share of sample-0 camera rays that hit a triangle, by the restated walk."""
    sc, verts, _, _, nodes, idx = arrays(member, tuple(res))
    o, d, _ = RT.camera_rays(sc, seed)
    _, tri = RW.ref_walk(nodes, idx, verts, o, d)
    return float((tri >= 0).mean())
