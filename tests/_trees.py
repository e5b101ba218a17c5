"""Caller-built BVH trees for the tests (test infrastructure: numpy only, nothing here calls
the library under test). Every transform takes the node array and tri_idx that BVH::build
gives for a scene and returns new `(nodes, tri_idx)` arrays that pt_scene_validate accepts:
the shapes another builder could hand to pt_ctx_set_scene (multi-triangle and empty leaves,
a root leaf, degenerate chains, leaves that do not partition the triangles, boxes that do
not nest). `reachable`, `depth` and `leaf_sizes` restate what a transform implies, for the
tests' expectations."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np


def is_leaf(nodes: np.ndarray, n: int) -> bool:
    return nodes["left"][n] == -1 and nodes["right"][n] == -1


def _walk(nodes: np.ndarray) -> List[Tuple[int, int]]:
    """(node, depth) of every node reachable from the root."""
    out, st = [], [(0, 0)]
    while st:
        n, d = st.pop()
        out.append((n, d))
        if not is_leaf(nodes, n):
            st.append((int(nodes["left"][n]), d + 1))
            st.append((int(nodes["right"][n]), d + 1))
    return out


def reachable(nodes: np.ndarray) -> int:
    return len(_walk(nodes))


def depth(nodes: np.ndarray) -> int:
    return max(d for _, d in _walk(nodes))


def leaf_sizes(nodes: np.ndarray) -> List[int]:
    """Triangles per reachable leaf (0 for an empty leaf)."""
    return [max(0, int(nodes["tri_end"][n]) - int(nodes["tri_start"][n]) + 1)
            for n, _ in _walk(nodes) if is_leaf(nodes, n)]


def merge_leaf_pairs(nodes: np.ndarray, every: int = 2) -> int:
    """Turn every `every`-th interior node whose children are both one-triangle leaves with
    adjacent ranges into a two-triangle leaf (a tree the C ABI accepts from any builder), in
    place. Returns the nodes merged."""
    merged_ = 0
    for n in range(len(nodes)):
        l, r = nodes["left"][n], nodes["right"][n]
        if l == -1 or (n % every):
            continue
        kids = [l, r]
        if all(nodes["left"][k] == -1 and nodes["right"][k] == -1 and
               nodes["tri_start"][k] == nodes["tri_end"][k] for k in kids):
            s0, s1 = sorted(int(nodes["tri_start"][k]) for k in kids)
            if s1 == s0 + 1:
                nodes["left"][n] = nodes["right"][n] = -1
                nodes["tri_start"][n], nodes["tri_end"][n] = s0, s1
                merged_ += 1
    return merged_


def merged(nodes: np.ndarray, tri_idx: np.ndarray, k: int):
    """Every maximal subtree that holds at most `k` triangles over a contiguous range of
    positions becomes one leaf with the subtree root's box. The nodes below it stay in the
    array, unreachable (num_nodes = visits < len(nodes))."""
    nodes = nodes.copy()
    span = {}  # node -> (first position, last position, triangles)

    def measure(n):
        if is_leaf(nodes, n):
            s, e = int(nodes["tri_start"][n]), int(nodes["tri_end"][n])
            span[n] = (s, e, e - s + 1)
        else:
            a, b = measure(int(nodes["left"][n])), measure(int(nodes["right"][n]))
            span[n] = (min(a[0], b[0]), max(a[1], b[1]), a[2] + b[2])
        return span[n]

    measure(0)
    st = [0]
    while st:
        n = st.pop()
        if is_leaf(nodes, n):
            continue
        s, e, cnt = span[n]
        if cnt <= k and e - s + 1 == cnt:
            nodes["left"][n] = nodes["right"][n] = -1
            nodes["tri_start"][n], nodes["tri_end"][n] = s, e
        else:
            st += [int(nodes["left"][n]), int(nodes["right"][n])]
    return nodes, tri_idx.copy()


def root_leaf(nodes: np.ndarray, tri_idx: np.ndarray):
    """One node: the leaf [0, nt - 1] with the root's box."""
    out = nodes[:1].copy()
    out["left"][0] = out["right"][0] = -1
    out["tri_start"][0], out["tri_end"][0] = 0, len(tri_idx) - 1
    return out, tri_idx.copy()


def chain(nodes: np.ndarray, tri_idx: np.ndarray, verts: np.ndarray, right_deep: bool, seed: int = 7):
    """A degenerate tree of depth nt - 1 over the triangles sorted by centroid x (ties broken
    by a seeded permutation; the sorted order is the chain's own tri_idx): interior node i =
    {leaf(i), node i + 1}, the last one {leaf(nt - 2), leaf(nt - 1)}. right_deep: the inner
    child is the right one, which BVH::intersect pops first, so its stack grows by one leaf per
    level; otherwise the mirror image, whose stack never holds more than two nodes. Leaf boxes
    are the triangles' AABBs, inner boxes their exact float32 unions."""
    nt = len(tri_idx)
    v = np.asarray(verts, dtype=np.float32).reshape(nt, 3, 3)
    if nt == 1:
        return root_leaf(nodes, tri_idx)
    cx = (v[:, :, 0].astype(np.float64).sum(axis=1)) / 3.0
    order = np.lexsort((np.random.default_rng(seed).permutation(nt), cx)).astype(np.int32)
    lo, hi = v[order].min(axis=1), v[order].max(axis=1)  # leaf boxes in chain order
    out = np.zeros(2 * nt - 1, dtype=nodes.dtype)
    suffix_lo = np.minimum.accumulate(lo[::-1], axis=0)[::-1]
    suffix_hi = np.maximum.accumulate(hi[::-1], axis=0)[::-1]
    for i in range(nt - 1):
        inner = i + 1 if i + 1 < nt - 1 else (nt - 1) + (nt - 1)  # the last pair: two leaves
        leaf = (nt - 1) + i
        out["lb"][i], out["rt"][i] = suffix_lo[i], suffix_hi[i]
        out["left"][i], out["right"][i] = (leaf, inner) if right_deep else (inner, leaf)
        out["tri_start"][i], out["tri_end"][i] = i, nt - 1
    for j in range(nt):
        n = (nt - 1) + j
        out["lb"][n], out["rt"][n] = lo[j], hi[j]
        out["left"][n] = out["right"][n] = -1
        out["tri_start"][n] = out["tri_end"][n] = j
    return out, order


def with_empty_leaves(nodes: np.ndarray, tri_idx: np.ndarray, every: int = 4):
    """Every `every`-th reachable leaf becomes an interior node over {a copy of the leaf, an
    empty leaf (tri_start = 1, tri_end = 0) with the same box}, the empty one alternately on
    the right and on the left."""
    leaves = [n for n, _ in _walk(nodes) if is_leaf(nodes, n)][::every]
    out = np.concatenate([nodes, np.zeros(2 * len(leaves), dtype=nodes.dtype)])
    for k, n in enumerate(leaves):
        full, empty = len(nodes) + 2 * k, len(nodes) + 2 * k + 1
        out[full] = out[n]
        out[empty] = out[n]
        out["tri_start"][empty], out["tri_end"][empty] = 1, 0
        out["left"][n], out["right"][n] = (full, empty) if k % 2 == 0 else (empty, full)
    return out, tri_idx.copy()


def _leaf_of(nodes: np.ndarray, tri_idx: np.ndarray, tri: int) -> int:
    pos = int(np.flatnonzero(tri_idx == tri)[0])
    for n, _ in _walk(nodes):
        if is_leaf(nodes, n) and nodes["tri_start"][n] <= pos <= nodes["tri_end"][n]:
            return n
    raise KeyError(tri)


def duplicated(nodes: np.ndarray, tri_idx: np.ndarray, tri: int):
    """The leaf that holds triangle `tri` becomes the parent of two leaves over its range: the
    leaves no longer partition the positions (a triangle is tested twice, with equal t)."""
    n = _leaf_of(nodes, tri_idx, tri)
    out = np.concatenate([nodes, np.zeros(2, dtype=nodes.dtype)])
    out[len(nodes)] = out[n]
    out[len(nodes) + 1] = out[n]
    out["left"][n], out["right"][n] = len(nodes), len(nodes) + 1
    return out, tri_idx.copy()


def dropped(nodes: np.ndarray, tri_idx: np.ndarray, tri: int):
    """The leaf that holds triangle `tri` (a one-triangle leaf) is made empty: the triangle is
    in no leaf, so no ray can hit it."""
    n = _leaf_of(nodes, tri_idx, tri)
    assert nodes["tri_start"][n] == nodes["tri_end"][n]
    out = nodes.copy()
    out["tri_start"][n], out["tri_end"][n] = 1, 0
    return out, tri_idx.copy()


def uncontained(nodes: np.ndarray, tri_idx: np.ndarray):
    """The first interior node below the root with a child that reaches past the node's lower x
    plane gets rt.x = lb.x: a valid tree whose boxes do not nest (the walk then skips subtrees
    a nested tree would enter, so only the tree walk may render it)."""
    out = nodes.copy()
    for n, d in sorted(_walk(nodes)):
        if d == 0 or is_leaf(nodes, n):
            continue
        kids = [int(nodes["left"][n]), int(nodes["right"][n])]
        if any(nodes["rt"][c][0] > nodes["lb"][n][0] for c in kids):
            out["rt"][n][0] = out["lb"][n][0]
            return out, tri_idx.copy()
    raise ValueError("no interior node below the root to shrink")


def dump_bvh_bytes(nodes: np.ndarray, tri_idx: np.ndarray) -> bytes:
    """The tree-file format the reference harness reads and writes: int32 node count, int32
    triangle count, the 40-B nodes, tri_idx."""
    return (np.array([len(nodes), len(tri_idx)], dtype="<i4").tobytes() + np.ascontiguousarray(nodes).tobytes() +
            np.ascontiguousarray(tri_idx, dtype="<i4").tobytes())
