"""The scene kernel with the scene's constants baked in and the launch's values read once
(PT_KCONST), against the oracle's bits and ray counts at 32 x 32, 8 spp."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RES, SPP = (32, 32), 8
PATH_RTC = 3  # PT_PATH_FLAT_RTC


@pytest.fixture(scope="module")
def pt():
    import ptamd
    if ptamd.lib().pt_device_count() <= 0:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    return ptamd


def _scene(name):
    from ptamd import scenes
    return scenes.cornell(RES) if name == "cornell" else scenes.modified_cornell(0.3, RES)


@pytest.fixture(scope="module")
def refs():
    """The oracle's image and ray count of every (scene, depth) the tests render, computed once."""
    import _oracle as O
    cases = [("cornell", d) for d in (1, 2, 5, 8)] + [("mcornell", d) for d in (5, 8)]
    return {(n, d): O.render(_scene(n), SPP, d) for n, d in cases}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(img, st, ref, what):
    want, rays = ref
    assert np.array_equal(_bits(img), _bits(want)) and st["rays"] == rays, what


def _lds_bytes(pt, num_tris, queue, depth):
    out = (C.c_uint32 * 10)()
    assert pt.lib().pt_debug_flat_lds(num_tris, 0, queue, max(1, depth - 1), out) == 0
    return out[9]


def test_cornell_depths_up_and_down_on_one_context(pt, refs):
    """Depth 1, 2, 5, 8 and back on one context: depth 8 changes rec_size and, through the LDS
    fit, the queue capacity, so the launches differ in the part of the layout that a launch sizes.
    Every launch runs the scene kernel, in the block the layout function gives."""
    sc = _scene("cornell")
    cam = pt.Camera.from_spec(sc.camera)
    r = pt.Renderer(0)
    try:
        r.set_scene(pt.BVH.from_scene(sc))
        queues = {}
        for depth in (1, 2, 5, 8, 8, 5, 2, 1):
            img, st = r.render(cam, SPP, depth)
            assert st["kernel_path"] == PATH_RTC, depth
            _check(img, st, refs[("cornell", depth)], depth)
            plan = r.plan()
            assert plan["lds_bytes"] == _lds_bytes(pt, len(sc.tris), plan["pair_queue"], depth), (depth, plan)
            assert queues.setdefault(depth, plan["pair_queue"]) == plan["pair_queue"]
        assert queues[8] < queues[5] == 512  # the records of depth 8 leave room for shorter queues only
    finally:
        r.close()


def test_modified_cornell_with_the_theta_table(pt, refs):
    """34 leaves, a SPECULAR material: the theta table's lane bound is a constant of this kernel."""
    sc = _scene("mcornell")
    cam = pt.Camera.from_spec(sc.camera)
    r = pt.Renderer(0)
    try:
        r.set_scene(pt.BVH.from_scene(sc))
        for depth in (5, 8, 5):
            img, st = r.render(cam, SPP, depth)
            assert st["kernel_path"] == PATH_RTC and r.plan()["theta_lanes"] == 32, depth
            _check(img, st, refs[("mcornell", depth)], depth)
    finally:
        r.close()


def test_scene_a_b_a_on_one_context(pt, refs):
    """Cornell, modified Cornell, Cornell again: no constant of the previous scene survives."""
    r = pt.Renderer(0)
    try:
        for name in ("cornell", "mcornell", "cornell"):
            sc = _scene(name)
            r.set_scene(pt.BVH.from_scene(sc))
            for depth in (5, 8):
                img, st = r.render(pt.Camera.from_spec(sc.camera), SPP, depth)
                assert st["kernel_path"] == PATH_RTC, (name, depth)
                _check(img, st, refs[(name, depth)], (name, depth))
    finally:
        r.close()


_CHILD = """
import hashlib, json, sys
sys.path[:0] = [%r, %r]
import numpy as np
import ptamd
from ptamd import scenes
out = []
for name, depth in (("cornell", 5), ("cornell", 8), ("mcornell", 5)):
    sc = scenes.cornell((32, 32)) if name == "cornell" else scenes.modified_cornell(0.3, (32, 32))
    img, st = ptamd.render(ptamd.Camera.from_spec(sc.camera), ptamd.BVH.from_scene(sc), 8, depth, device=0)
    out.append([name, depth, hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest(), int(st["rays"]),
                int(st["kernel_path"])])
print(json.dumps(out))
"""


@pytest.mark.parametrize("hook", [{"PT_PAIR_QUEUE": "16"}, {"PT_PAIRS": "0"}, {"PT_RTC_DEFINES": "PT_KCONST=0"},
                                  {"PT_RTC_DEFINES": "PT_KCONST=0", "PT_BOX_PAIRS": "1"}, {"PT_BOX_PAIRS": "1"}])
def test_hooks_set_before_the_library_loads(pt, refs, hook):
    """A child process with the hook in its environment from the start: the overflow fallback under
    the new layout (16-entry queues), no pair queues at all (the per-lane loops are compiled in
    again), the macro at 0 (the scene kernel reads the arguments as before), and box-level pairs
    (their LDS table lies before the queues in the new layout) with the macro at 0 and at 1."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CHILD % (os.path.join(root, "pathtracer-cpp_amd"), os.path.join(root, "tests"))
    env = dict(os.environ, **hook)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    for name, depth, sha, rays, path in json.loads(out.stdout.strip().splitlines()[-1]):
        want, want_rays = refs[(name, depth)]
        assert path == PATH_RTC, (hook, name, depth)
        assert sha == hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest() and rays == want_rays, (hook, name, depth)


@pytest.mark.parametrize("name,hook,value", [("cornell", "PT_PAIRS", "0"), ("mcornell", "PT_THETA_LANES", "0")])
def test_hook_changed_between_set_scene_and_render(pt, refs, monkeypatch, name, hook, value):
    """The loaded scene kernel holds pt_ctx_set_scene's values; a hook that changes the plan before
    the render must keep that kernel from running: the launch takes a table kernel (the oracle's
    bits), and later renders are the oracle's too, whichever kernel the new compile gives them."""
    sc = _scene(name)
    cam = pt.Camera.from_spec(sc.camera)
    r = pt.Renderer(0)
    try:
        r.set_scene(pt.BVH.from_scene(sc))
        img, st = r.render(cam, SPP, 5)
        assert st["kernel_path"] == PATH_RTC
        _check(img, st, refs[(name, 5)], "before")
        monkeypatch.setenv(hook, value)
        img, st = r.render(cam, SPP, 5)
        assert st["kernel_path"] != PATH_RTC, (hook, st["kernel_path"])
        _check(img, st, refs[(name, 5)], "changed")
        img, st = r.render(cam, SPP, 5)
        _check(img, st, refs[(name, 5)], "changed, again")
        monkeypatch.delenv(hook)
        img, st = r.render(cam, SPP, 5)
        assert st["kernel_path"] != PATH_RTC  # the kernel requested above holds the hook's values
        _check(img, st, refs[(name, 5)], "back")
        r.prepare()  # waits for the compile requested for the current values
        img, st = r.render(cam, SPP, 5)
        assert st["kernel_path"] == PATH_RTC
        _check(img, st, refs[(name, 5)], "back, compiled")
    finally:
        r.close()
