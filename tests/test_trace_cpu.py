"""trace() on caller-supplied rays without a device: pt_bvh_trace (the host path, bit-identical
to the GPU's), ptamd.BVH.trace, the C++ drop-in's trace() / BVH::trace_batch, and the argument
handling of pt_bvh_trace / pt_ctx_trace. Expected values: tests/_reftrace.py (trace() restated
over the oracle's primitives), itself anchored on `_oracle.render` here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _oracle as O
import _reftrace as RT
import _refwalk as RW
import _treecases as TC
from _plans import _planned
from conftest import ROOT

PKG = os.path.join(ROOT, "pathtracer-cpp_amd")
F32 = np.float32
N = 256
DEPTHS = (1, 2, 5, 8)


@functools.lru_cache(maxsize=None)
def _bvh(name):
    import ptamd
    b = ptamd.BVH.from_scene(RT.make_scene(name))
    b.build()
    return b


@pytest.mark.parametrize("name,depth", [("cornell", 5), ("random_7_300", 4), ("random_3_40", 3)])
@pytest.mark.parametrize("seed", [1, 7])
def test_restatement_matches_oracle_render(name, depth, seed):
    """The checker itself: camera rays (sample 0 of an 8 x 8 frame) traced by _reftrace from the
    state after the camera's two draws give `_oracle.render(spp=1)`'s bits and ray count."""
    sc = RW.make_scene(name, (8, 8))
    verts, nodes, idx, mtype, mvals = RT.scene_arrays(name)
    o, d, st = RT.camera_rays(sc, seed)
    rgb, _, segs = RT.trace(nodes, idx, verts, mtype, mvals, o, d, st, depth)
    ref, rays = O.render(sc, 1, depth, seed)
    RT.assert_same(rgb, ref.reshape(-1, 3), "restatement vs oracle render")
    assert int(segs.sum()) == rays
    assert RW.bits(ref).any()


@pytest.mark.parametrize("explicit", [False, True], ids=["seeded", "states"])
@pytest.mark.parametrize("name", RT.ALL)
def test_pt_bvh_trace_matches_restatement(name, explicit):
    o, d = RT.rays(name, N)
    P = RT.head(RT.paths(name, explicit=explicit), N)
    states = RT.explicit_states(512)[:N] if explicit else None
    for depth in DEPTHS:
        want, _, segs = RT.radiance(P, depth)
        got, st = _bvh(name).trace(o, d, depth, states=states)
        assert got.dtype == np.float32 and got.shape == (N, 3)
        RT.assert_same(got, want, f"{name} depth {depth}")
        assert st["rays"] == int(segs.sum()) and st["paths"] == N and st["runaway"] == 0
        RT.check_floor(name, got, P, depth)


@pytest.mark.parametrize("name", ["random_7_300", "cornell+glow"])
def test_depth_one_and_zero(name):
    o, d = RT.rays(name, N)
    b = _bvh(name)
    _, tri = b.intersect(o, d)
    _, _, _, _, mvals = RT.scene_arrays(name)
    want = np.where((tri >= 0)[:, None], mvals[np.maximum(tri, 0), 3:6], F32(0)).astype(F32)
    got, st = b.trace(o, d, 1)
    assert np.array_equal(RW.bits(got), RW.bits(want)) and st["rays"] == N
    assert RW.bits(want).any()
    got, st = b.trace(o, d, 0)
    assert not RW.bits(got).any() and st["rays"] == 0 and st["paths"] == N


@pytest.mark.parametrize("spp", [2, 7])
@pytest.mark.parametrize("name", ["random_7_300", "cornell+glow"])
def test_samples_sum_in_order(name, spp):
    o, d = RT.rays(name, 65)
    b = _bvh(name)
    want = RT.mean_of_samples(lambda st: b.trace(o, d, 5, states=st)[0], 65, spp, 3)
    got, st = b.trace(o, d, 5, samples=spp, seed=3)
    RT.assert_same(got, want, f"{name} spp {spp}")
    assert st["paths"] == 65 * spp
    # the same through explicit states, laid out [ray][sample]
    got2, _ = b.trace(o, d, 5, samples=spp, states=RT.sample_seeds(65, spp, 3))
    RT.assert_same(got2, want)


def test_nonfinite_rays():
    """inf and NaN in origins and directions on a scene with SPECULAR triangles: the restatement's
    answers, a NaN where it has one."""
    o, d, want, segs = RT.nonfinite_expected()
    got, st = _bvh("random_7_300").trace(o, d, 5)
    RT.assert_same(got, want, "non-finite rays")
    assert st["rays"] == int(segs.sum()) > 16


def test_overflowing_direction_on_specular_gives_nan():
    """The dark-scene shortcut (a path ending at +0 folds to +0) does not hold for a NaN cosine."""
    import ptamd
    o, d, want, segs = RT.overflow_expected()
    b = ptamd.BVH.from_scene(RT.overflow_scene())
    got, st = b.trace(o, d, 3)
    RT.assert_same(got, want, "overflow")
    assert st["rays"] == segs


@pytest.mark.parametrize("name,variant", RT.TREES)
def test_caller_built_trees(name, variant):
    import ptamd
    o, d, want, segs = RT.tree_expected(name, variant)
    got, st = TC.to_bvh(ptamd, TC.case(name, variant)).trace(o, d, 5)
    RT.assert_same(got, want, f"{name} {variant}")
    assert st["rays"] == segs


def test_argument_handling():
    import ptamd
    from ptamd import _lib
    L = ptamd.lib()
    ref = ptamd._SceneRef(_bvh("cornell"))
    o, d = RT.rays("cornell", 4)
    rgb = np.zeros((4, 3), dtype=np.float32)
    st = _lib.pt_trace_stats()
    ok = _lib.pt_trace_params(5, 1, 1, None)

    def arg_error(rc):
        assert rc == _lib.PT_E_ARG
        assert L.pt_last_error()  # a message

    def host(scene=ref.s, org=o.ctypes.data, dirs=d.ctypes.data, n=4, prm=ok, out=rgb.ctypes.data):
        return L.pt_bvh_trace(C.byref(scene) if scene is not None else None, org, dirs, n,
                              C.byref(prm) if prm is not None else None, out, C.byref(st))

    assert host() == 0
    assert host(org=None, dirs=None, n=0, out=None) == 0  # n == 0
    arg_error(host(n=-1))
    arg_error(host(scene=None))
    arg_error(host(org=None))
    arg_error(host(dirs=None))
    arg_error(host(out=None))
    arg_error(host(prm=None))
    for depth, spp in ((-1, 1), (_lib.PT_MAX_DEPTH + 1, 1), (5, 0), (5, -3), (5, (1 << 20) + 1)):
        arg_error(host(prm=_lib.pt_trace_params(depth, spp, 1, None)))
    assert host(prm=_lib.pt_trace_params(_lib.PT_MAX_DEPTH, 1, 1, None)) == 0
    bad = _lib.pt_scene(ref.s.num_tris, ref.s.verts, ref.s.materials, ref.s.num_nodes, ref.s.nodes, None)
    arg_error(host(scene=bad))  # a scene pt_scene_validate refuses
    # a NULL context (no device needed for these returns)
    arg_error(L.pt_ctx_trace(None, o.ctypes.data, d.ctypes.data, 4, C.byref(ok), rgb.ctypes.data, 0, C.byref(st)))
    arg_error(L.pt_ctx_trace(None, None, None, 0, None, None, 0, None))
    with pytest.raises(ValueError):
        _bvh("cornell").trace(o, d, 5, samples=2, states=np.zeros(4, dtype=np.uint32))


def test_abi_version_and_new_symbols():
    import ptamd
    L = ptamd.lib()
    assert L.pt_abi_version() == 3
    for name in ("pt_bvh_trace", "pt_ctx_trace"):
        assert hasattr(L, name), name
        assert name in ptamd._lib.EXPORTED
    assert C.sizeof(ptamd._lib.pt_trace_stats) == 64
    assert C.sizeof(ptamd._lib.pt_trace_params) == 24


def _hex_row(a):
    return " ".join(f"{x:08x}" for x in RW.bits(np.asarray(a, dtype=F32)).reshape(-1).tolist())


@pytest.mark.parametrize("name", ["cornell", "cornell+glow"])
def test_dropin_cpp_trace(tmp_path, name):
    """trace() of the drop-in header (the reference's signature, drawing from the global rng from
    call to call) and BVH::trace_batch on Cornell and its glow variant, 64 rays, depth 5."""
    exe = tmp_path / "dropin_trace"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I" + PKG,
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "dropin_trace.cc"),
                        "-L" + os.path.join(PKG, "lib"), "-lpt_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    n, depth, seed = 64, 5, 9
    verts, nodes, idx, mtype, mvals = RT.scene_arrays(name)
    o, d = RT.rays(name, n)
    tris = "\n".join(f"{_hex_row(verts[i])} {int(mtype[i])} {_hex_row(mvals[i])}" for i in range(verts.shape[0]))
    rays = "\n".join(_hex_row(np.concatenate([o[i], d[i]])) for i in range(n))
    r = subprocess.run([str(exe)], input=f"{verts.shape[0]} {n} {depth} {seed}\n{tris}\n{rays}\n", capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = np.array([[int(x, 16) for x in ln.split()] for ln in r.stdout.strip().splitlines()], dtype=np.uint32)
    assert rows.shape == (n, 6)
    got = rows.view(np.float32)
    # trace(): the global stream continues from ray to ray
    chained = np.zeros((n, 3), dtype=F32)
    state = np.array([12345], dtype=np.uint32)
    for i in range(n):
        rgb, state, _ = RT.trace(nodes, idx, verts, mtype, mvals, o[i:i + 1], d[i:i + 1], state, depth)
        chained[i] = rgb[0]
    RT.assert_same(got[:, 0:3], chained, "drop-in trace()")
    if name.endswith("+glow"):
        assert (RW.bits(chained) != 0).any(axis=1).sum() >= 0.75 * n
    # trace_batch(): per-ray streams pt_sample_seed(i, 0, seed)
    want, _, _ = RT.trace(nodes, idx, verts, mtype, mvals, o, d, RT.sample_seeds(n, 1, seed)[:, 0], depth)
    RT.assert_same(got[:, 3:6], want, "drop-in trace_batch()")


def _placement(nodes, tris, tree_depth, tri_f4, rec_rows, lds_usable=161280):
    import ptamd
    out = (C.c_int32 * 4)()
    ptamd.check(ptamd.lib().pt_debug_walk_placement(nodes, tris, tree_depth, tri_f4, rec_rows, lds_usable, out))
    return {"lds_scene": out[0], "lds_stack": out[1], "lds_records": out[2]}, out[3]


def _want(nodes, tris, tree_depth, tri_f4, rec_rows, lds_usable=161280, **rule):
    return _planned({"nodes": nodes, "tree_depth": tree_depth}, tris, rec_rows + 1, lds_usable=lds_usable, tri_f4=tri_f4,
                    **rule)


# (nodes, triangles, tree depth, float4 per triangle, record rows): (scene, stack, records) in LDS.
# With 161,280 B of LDS per CU the cap is 65,536 B: 64 stack rows of 1,024 B fill it (no room
# for the 256-B scene beside them), 65 do not;
# 16 (2 * 24 + 5 * 400) = 32,768 B of scene is the default budget, one node more is over it;
# beside an 8-row stack (8,192 B) and no scene, 28 record rows of 2,048 B fit, 29 do not.
BOUNDARIES = [((3, 2, 64, 5, 0), (0, 1, 1)), ((3, 2, 65, 5, 0), (1, 0, 1)),
              ((24, 400, 8, 5, 0), (1, 1, 1)), ((25, 400, 8, 5, 0), (0, 1, 1)),
              ((1000, 1000, 8, 5, 28), (0, 1, 1)), ((1000, 1000, 8, 5, 29), (0, 1, 0))]


@pytest.mark.parametrize("shape,flags", BOUNDARIES)
def test_walk_placement_boundaries(shape, flags, monkeypatch):
    """place_walk (pt_launch.hip), the one placement rule of the ray queries and pt_ctx_trace,
    against its restatement tests/_plans.py::_planned at the sizes where each part stops fitting."""
    for hook in ("PT_LDS_SCENE_BYTES", "PT_QUERY_LDS_STACK", "PT_TRACE_LDS_REC"):
        monkeypatch.delenv(hook, raising=False)
    if shape[4] >= 28:
        monkeypatch.setenv("PT_LDS_SCENE_BYTES", "0")  # a zero scene budget: stack and records only
    rule = dict(scene_budget=0) if shape[4] >= 28 else {}
    got, lds_bytes = _placement(*shape)
    assert got == _want(*shape, **rule)
    assert (got["lds_scene"], got["lds_stack"], got["lds_records"]) == flags
    nodes, tris, depth, tri_f4, rec = shape
    assert lds_bytes == (got["lds_scene"] * 16 * (2 * nodes + tri_f4 * tris) + got["lds_stack"] * 1024 * depth +
                         got["lds_records"] * 2048 * rec)
    assert lds_bytes <= 65536


def test_walk_placement_usable_lds_and_hooks(monkeypatch):
    for hook in ("PT_LDS_SCENE_BYTES", "PT_QUERY_LDS_STACK", "PT_TRACE_LDS_REC"):
        monkeypatch.delenv(hook, raising=False)
    # 65,536 B per CU halve the cap: 32 stack rows fit, 33 do not; the scene no longer fits beside them
    for depth, stack in ((32, 1), (33, 0)):
        got, _ = _placement(24, 400, depth, 5, 4, 65536)
        assert got == _want(24, 400, depth, 5, 4, 65536) and got["lds_stack"] == stack and got["lds_scene"] == 1 - stack
    # no usable LDS: nothing is placed there
    got, lds_bytes = _placement(24, 400, 8, 5, 4, 0)
    assert got == _want(24, 400, 8, 5, 4, 0) == {"lds_scene": 0, "lds_stack": 0, "lds_records": 0} and lds_bytes == 0
    # 3 float4 per triangle (queries) fit the budget where 5 (with materials) do not
    assert _placement(24, 600, 8, 3, 0)[0]["lds_scene"] == 1 and _placement(24, 600, 8, 5, 0)[0]["lds_scene"] == 0
    assert _placement(24, 600, 8, 3, 0)[0] == _want(24, 600, 8, 3, 0)
    assert _placement(24, 600, 8, 5, 0)[0] == _want(24, 600, 8, 5, 0)
    shape = (24, 600, 8, 5, 4)
    for hook, value, rule, off in (("PT_QUERY_LDS_STACK", "0", dict(stack=False), "lds_stack"),
                                   ("PT_TRACE_LDS_REC", "0", dict(rec=False), "lds_records"),
                                   ("PT_LDS_SCENE_BYTES", "0", dict(scene_budget=0), "lds_scene"),
                                   ("PT_LDS_SCENE_BYTES", "65536", dict(scene_budget=65536), None)):
        monkeypatch.setenv(hook, value)
        got, _ = _placement(*shape)
        monkeypatch.delenv(hook)
        assert got == _want(*shape, **rule), (hook, value)
        if off:
            assert got[off] == 0
        else:
            assert got["lds_scene"] == 1 and _placement(*shape)[0]["lds_scene"] == 0  # 16 * 3,048 B: over 32 KiB only
