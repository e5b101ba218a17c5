#!/usr/bin/env python3
"""Generate the caller-tree fixtures in tests/golden/ from the UNMODIFIED reference.

Runs in the development container only (needs oracle/_ref/pt_ref, see
oracle/ref/build_ref.sh). For each entry of CASES the tree that tests/_trees.py makes of the
scene's BVH::build tree is written in the harness's own --dump-bvh format and rendered by the
reference with --load-bvh: its BVH::intersect then walks the caller's nodes. The committed
outputs are data: the images (<name>.npy) and trees.json with the sha256 of each scene and
tree file, so an edit to a scene or a transform invalidates the fixture instead of silently
changing it. The reference prints no ray count; the oracle's own count for the same tree is
recorded beside the image ("oracle_rays") so it cannot drift unnoticed.

Usage: python tests/golden/gen_trees.py
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "pathtracer-cpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _oracle as O  # noqa: E402
import _treecases as TC  # noqa: E402
import _trees as T  # noqa: E402

RES, SPP, DEPTH = (24, 20), 4, 5
# (fixture name, scene, variant)
CASES = [("tree_cornell_merged5", "cornell", "merged5"), ("tree_cornell_chain_right", "cornell", "chain_right"),
         ("tree_cornell_empty", "cornell", "empty"), ("tree_cornell_dropped", "cornell", "dropped")]


def main() -> None:
    if not O.ref_available():
        sys.exit("oracle/_ref/pt_ref is not built")
    meta = {"images": {}}
    for name, scene_name, variant in CASES:
        sc = TC.scene(scene_name, RES)
        c = TC.case(scene_name, variant)
        blob = T.dump_bvh_bytes(c.nodes, c.idx)
        with tempfile.TemporaryDirectory() as td:
            tree = os.path.join(td, "tree.bvh")
            with open(tree, "wb") as f:
                f.write(blob)
            img, m = O.ref_run(sc, SPP, DEPTH, extra=["--load-bvh", tree])
        assert m["nodes"] == len(c.nodes) and m["tris"] == len(c.idx), m
        _, rays = TC.oracle_image(scene_name, variant, RES, SPP, DEPTH)
        np.save(os.path.join(HERE, name + ".npy"), img, allow_pickle=False)
        meta["images"][name] = {
            "scene": scene_name, "variant": variant, "res": list(RES), "spp": SPP, "depth": DEPTH,
            "scene_sha256": hashlib.sha256(sc.with_res(1, 1).to_ptscene().encode()).hexdigest(),
            "tree_sha256": hashlib.sha256(blob).hexdigest(), "nodes": len(c.nodes), "oracle_rays": rays}
        print(name, img.shape, rays)
    with open(os.path.join(HERE, "trees.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
