"""The caller-tree cases shared by tests/test_trees_cpu.py, tests/test_trees_gpu.py and
tests/golden/gen_trees.py (test infrastructure): a scene, one of tests/_trees.py's transforms
of the oracle's BVH::build tree for it (`_oracle.bvh_build`, bit-identical to the product
builder's), and the oracle's answers on that tree (`_refwalk.ref_walk`), each made once per
process and left unchanged. Only `to_bvh` touches the library under test."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import _oracle as O
import _refwalk as RW
import _trees as T
from _randscene import random_scene

K_BIG = 140  # sphere12: leaves of 25, 135 and 136 triangles under one wide node (296 > 255)

# transforms whose leaves partition the positions and whose boxes nest: flat list and wide tree
CONTAINED = ("merged2", "merged5", "merged31", "root_leaf", "chain_right", "chain_left", "empty")
# valid trees the packer keeps off the flat and wide paths (identity ranks, or no nesting)
TREE_ONLY = ("duplicated", "dropped", "uncontained")
VARIANTS = CONTAINED + TREE_ONLY


def scene(name: str, res=(24, 20)):
    from ptamd import scenes
    res = tuple(res)
    if name == "cornell":
        return scenes.cornell(res)
    if name == "mcornell":
        return scenes.modified_cornell(0.3, res)
    if name == "sphere12":
        return scenes.sphere_in_cornell(12, res)
    if name == "onetri":  # one emitting triangle in front of Cornell's camera: most paths miss
        sc = scenes.Scene("onetri", scenes.cornell(res).camera)
        sc.add([((178.0, 178.0, 100.0), (378.0, 178.0, 100.0), (278.0, 400.0, 120.0))],
               scenes.Material.make(scenes.EMIT, 0, (1.0, 0.5, 0.25)))
        return sc
    if name.startswith("rand"):  # rand61, rand71: the room's 12 triangles + random ones
        n = int(name[4:])
        return random_scene(n, n - 12, res)
    raise KeyError(name)


class Case(NamedTuple):
    name: str
    variant: str
    verts: np.ndarray   # (nt, 9) float32
    mvals: np.ndarray   # (nt, 7) float32: color, emit, roughness
    nodes: np.ndarray   # the caller's tree
    idx: np.ndarray
    base_nodes: np.ndarray  # BVH::build's tree
    base_idx: np.ndarray
    tri: int            # the triangle `duplicated` / `dropped` act on (the camera's centre ray hits it)


@functools.lru_cache(maxsize=None)
def _base(name: str):
    sc = scene(name)
    verts, _, mvals = O.pack_scene(sc)
    nodes, idx = O.bvh_build(verts)
    c = sc.camera
    o = np.array([c.pos], dtype=np.float32)
    d = np.array([c.forward], dtype=np.float32)
    _, tri = RW.ref_walk(nodes, idx, verts, o, d)
    return verts, mvals, nodes, idx, int(tri[0])


def transform(variant: str, nodes, idx, verts, tri: int):
    if variant.startswith("merged"):
        return T.merged(nodes, idx, int(variant[6:]))
    if variant == "root_leaf":
        return T.root_leaf(nodes, idx)
    if variant in ("chain_right", "chain_left"):
        return T.chain(nodes, idx, verts, variant == "chain_right")
    if variant == "empty":
        return T.with_empty_leaves(nodes, idx)
    if variant == "duplicated":
        return T.duplicated(nodes, idx, tri)
    if variant == "dropped":
        return T.dropped(nodes, idx, tri)
    if variant == "uncontained":
        return T.uncontained(nodes, idx)
    if variant == "build":
        return nodes.copy(), idx.copy()
    raise KeyError(variant)


@functools.lru_cache(maxsize=None)
def case(name: str, variant: str) -> Case:
    verts, mvals, nodes, idx, tri = _base(name)
    assert tri >= 0 or name == "onetri" or variant not in ("duplicated", "dropped")
    n2, i2 = transform(variant, nodes, idx, verts, tri)
    for a in (n2, i2):
        a.setflags(write=False)
    return Case(name, variant, verts, mvals, n2, i2, nodes, idx, tri)


def to_bvh(ptamd, c: Case):
    """A ptamd.BVH of the case's scene that carries the caller's tree instead of BVH::build's."""
    b = ptamd.BVH.from_scene(scene(c.name))
    b.nodes, b.tri_idx, b.built = c.nodes.copy(), c.idx.copy(), True
    return b


def rays():
    """256 seeded rays + the 16 with inf / NaN components (272)."""
    o, d = RW.ray_set(4242, 256)
    o2, d2 = RW.nonfinite_rays()
    return np.concatenate([o, o2]), np.concatenate([d, d2])


@functools.lru_cache(maxsize=None)
def expected(name: str, variant: str):
    """(origins, directions, t, tri): the oracle's walk of the caller's nodes."""
    c = case(name, variant)
    o, d = rays()
    t, tri = RW.ref_walk(c.nodes, c.idx, c.verts, o, d)
    for a in (o, d, t, tri):
        a.setflags(write=False)
    return o, d, t, tri


@functools.lru_cache(maxsize=None)
def oracle_image(name: str, variant: str, res=(24, 20), spp: int = 4, depth: int = 5):
    c = case(name, variant)
    img, rays_ = O.render(scene(name, res), spp, depth, nodes=np.ascontiguousarray(c.nodes), idx=np.ascontiguousarray(c.idx))
    img.setflags(write=False)
    return img, rays_
