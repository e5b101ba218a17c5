"""Ray queries without a device: pt_bvh_intersect (the reference walk, bvh.h:156-183, on the
host), ptamd.BVH.intersect, the C++ drop-in's BVH::intersect / intersect_batch, and the argument
handling of the new entry points. Expected values: tests/_refwalk.py (the oracle)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _refwalk as RW
from conftest import ROOT

PKG = os.path.join(ROOT, "pathtracer-cpp_amd")
SCENES = ["random_3_40", "random_7_300", "cornell"]


def _bvh(name):
    import ptamd
    b = ptamd.BVH.from_scene(RW.make_scene(name))
    b.build()
    return b


def _scene_ref(name):
    import ptamd
    return ptamd._SceneRef(_bvh(name))


def _host_intersect(ref, o, d):
    import ptamd
    n = o.shape[0]
    t = np.full(n, -1, dtype=np.float32)
    tri = np.full(n, -7, dtype=np.int32)
    rc = ptamd.lib().pt_bvh_intersect(C.byref(ref.s), o.ctypes.data, d.ctypes.data, n, t.ctypes.data, tri.ctypes.data)
    assert rc == 0, ptamd.lib().pt_last_error()
    return t, tri


def _same(t, tri, t_ref, tri_ref):
    bad = np.flatnonzero((RW.bits(t) != RW.bits(t_ref)) | (tri != tri_ref))
    assert bad.size == 0, f"{bad.size} rays differ, first {bad[:5]}: got {t[bad[:5]]} {tri[bad[:5]]}, " \
                          f"want {t_ref[bad[:5]]} {tri_ref[bad[:5]]}"


@pytest.mark.parametrize("name", SCENES)
def test_builder_matches_the_oracle_tree(name):
    """The helper walks the oracle's BVH, the library its own: they are the same tree."""
    _, nodes, idx = RW.oracle_bvh(name)
    b = _bvh(name)
    assert b.nodes.tobytes() == nodes.tobytes() and np.array_equal(b.tri_idx, idx)


@pytest.mark.parametrize("name", SCENES)
def test_pt_bvh_intersect_matches_reference_walk(name):
    o, d, t_ref, tri_ref = RW.expected(name)
    assert (tri_ref >= 0).sum() > len(tri_ref) // 4 and (tri_ref < 0).sum() >= len(tri_ref) // 20
    _same(*_host_intersect(_scene_ref(name), o, d), t_ref, tri_ref)


@pytest.mark.parametrize("name", SCENES)
def test_pt_bvh_intersect_nonfinite_rays(name):
    o, d, t_ref, tri_ref = RW.expected_nonfinite(name)
    _same(*_host_intersect(_scene_ref(name), o, d), t_ref, tri_ref)


@pytest.mark.parametrize("name", SCENES)
def test_python_bvh_intersect(name):
    o, d, t_ref, tri_ref = RW.expected(name)
    t, tri = _bvh(name).intersect(o, d)
    assert t.dtype == np.float32 and tri.dtype == np.int32
    _same(t, tri, t_ref, tri_ref)


def _hex_lines(a):
    return "\n".join(" ".join(f"{x:08x}" for x in row) for row in RW.bits(a).reshape(a.shape[0], -1).tolist())


def test_dropin_cpp_intersect(tmp_path):
    """BVH::intersect of the drop-in header (the reference's signature, const, on the host) and
    its intersect_batch extension on Cornell, 64 rays."""
    exe = tmp_path / "dropin_intersect"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I" + PKG,
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dropin_intersect.cc"),
                        "-L" + os.path.join(PKG, "lib"), "-lpt_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    verts, _, _ = RW.oracle_bvh("cornell")
    o, d, t_ref, tri_ref = (a[:64] for a in RW.expected("cornell"))
    text = f"{verts.shape[0]} 64\n{_hex_lines(verts)}\n{_hex_lines(np.concatenate([o, d], axis=1))}\n"
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(rows) == 64
    for k in (0, 2):  # intersect(), then intersect_batch()
        tri = np.array([int(x[k]) for x in rows], dtype=np.int32)
        t = np.array([int(x[k + 1], 16) for x in rows], dtype=np.uint32).view(np.float32)
        _same(t, tri, t_ref, tri_ref)


def test_argument_handling():
    import ptamd
    from ptamd import _lib
    L = ptamd.lib()
    ref = _scene_ref("cornell")
    o, d, _, _ = RW.expected("cornell")
    t = np.zeros(4, dtype=np.float32)
    tri = np.zeros(4, dtype=np.int32)

    def arg_error(rc):
        assert rc == _lib.PT_E_ARG
        assert L.pt_last_error()  # a message

    assert L.pt_bvh_intersect(C.byref(ref.s), None, None, 0, None, None) == 0  # n == 0
    arg_error(L.pt_bvh_intersect(C.byref(ref.s), o.ctypes.data, d.ctypes.data, -1, t.ctypes.data, tri.ctypes.data))
    arg_error(L.pt_bvh_intersect(None, o.ctypes.data, d.ctypes.data, 4, t.ctypes.data, tri.ctypes.data))
    arg_error(L.pt_bvh_intersect(C.byref(ref.s), None, d.ctypes.data, 4, t.ctypes.data, tri.ctypes.data))
    arg_error(L.pt_bvh_intersect(C.byref(ref.s), o.ctypes.data, d.ctypes.data, 4, None, tri.ctypes.data))
    arg_error(L.pt_bvh_intersect(C.byref(ref.s), o.ctypes.data, d.ctypes.data, 4, t.ctypes.data, None))
    bad = _lib.pt_scene(ref.s.num_tris, ref.s.verts, ref.s.materials, ref.s.num_nodes, ref.s.nodes, None)
    arg_error(L.pt_bvh_intersect(C.byref(bad), o.ctypes.data, d.ctypes.data, 4, t.ctypes.data, tri.ctypes.data))
    # a NULL context (no device needed for these returns)
    st = _lib.pt_query_stats()
    arg_error(L.pt_ctx_intersect(None, o.ctypes.data, d.ctypes.data, 4, _lib.PT_QUERY_CLOSEST, None, t.ctypes.data,
                                 tri.ctypes.data, 0, C.byref(st)))
    arg_error(L.pt_ctx_intersect(None, None, None, 0, _lib.PT_QUERY_ANY, None, None, None, 0, None))
    cam = ptamd.Camera.from_spec(RW.make_scene("cornell").camera)
    prm = _lib.pt_params(1, 1, 1, 0, 1, 1, 0, 0)
    aov = _lib.pt_aov()
    arg_error(L.pt_ctx_render_aov(None, C.byref(cam.c), C.byref(prm), 0, C.byref(aov), 0, C.byref(st)))
    arg_error(L.pt_ctx_render_aov(None, None, None, 0, None, 0, None))


def test_abi_version_and_new_symbols():
    import ptamd
    L = ptamd.lib()
    assert L.pt_abi_version() == 3
    for name in ("pt_bvh_intersect", "pt_ctx_intersect", "pt_ctx_render_aov"):
        assert hasattr(L, name), name
        assert name in ptamd._lib.EXPORTED
    assert C.sizeof(ptamd._lib.pt_query_stats) == 48 and C.sizeof(ptamd._lib.pt_aov) == 48
