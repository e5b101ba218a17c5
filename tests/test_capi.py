"""C ABI of libpt_hip.so on the CPU (no compute calls need a GPU here):
exported symbols, the exact BVH builder, camera setup, row partitions,
post-process and PNG output, and error behaviour."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _oracle as O
from _trees import merge_leaf_pairs as _merge_leaf_pairs
from conftest import ROOT, load_golden, scene_for, scene_hash


@pytest.fixture(scope="module")
def pt():
    import ptamd
    ptamd.build()
    return ptamd


def declared_functions(header="pt_hip.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"^\s*(?:int|void|int32_t|int64_t|const char\*)\s+(pt_\w+)\s*\(", src, flags=re.M))
    return names


def test_boundary_header_holds_no_test_hooks():
    """include/pt_hip.h declares the drop-in surface only; the test and tuning hooks live in
    include/pt_hip_debug.h."""
    public, debug = declared_functions(), declared_functions("pt_hip_debug.h")
    assert not {n for n in public if n.startswith("pt_debug") or n == "pt_rtc_check"}, public
    assert {"pt_debug_math", "pt_debug_sweep", "pt_debug_rgb8", "pt_debug_rccl_failover", "pt_debug_wide_verify",
            "pt_rtc_check", "pt_debug_rtc_cache", "pt_debug_ctx_flags", "pt_debug_counter",
            "pt_debug_scene_dark", "pt_debug_pack_hash"} <= debug
    assert not public & debug


def test_library_exports_every_declared_symbol(pt):
    names = declared_functions() | declared_functions("pt_hip_debug.h")
    assert {"pt_render_f32", "pt_ctx_render", "pt_bvh_build", "pt_camera_init", "pt_devices_release"} <= names
    out = subprocess.run(["nm", "-D", "--defined-only", pt._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (pt_\w+)", out))
    assert names <= exported, names - exported
    assert set(pt._lib.EXPORTED) <= exported
    lib = pt.lib()
    for n in names:
        getattr(lib, n)  # resolvable through ctypes
    assert lib.pt_abi_version() == 3


def test_dark_gate_needs_finite_cos_theta(pt):
    """The dark-path gate (pt_launch.hip scene_dark) also requires every path's
    cos theta to be finite (VERDICT r5 finding 1): SPECULAR roughness |r| <= 1.15, so that
    specular_sample's refl + j (material.h:15-25) never cancels, and unit-length shading normals
    (a collinear or underflowing sliver normalises to NaN, triangle.h:45-49)."""
    from ptamd import scenes

    def dark(sc):
        ref = pt._SceneRef(pt.BVH.from_scene(sc))  # keeps the arrays alive during the call
        return pt.lib().pt_debug_scene_dark(C.byref(ref.s))

    assert dark(scenes.cornell((8, 8))) == 1
    for r, want in ((0.0, 1), (0.8, 1), (1.15, 1), (-1.15, 1), (1.16, 0), (2.0, 0), (-2.0, 0), (float("nan"), 0),
                    (float("inf"), 0)):
        assert dark(scenes.modified_cornell(r, (8, 8))) == want, r
    for sliver in (((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0)),  # collinear: cross = 0
                   ((0.0, 0.0, 0.0), (1e-30, 0.0, 0.0), (0.0, 1e-30, 0.0))):  # cross underflows to 0
        sc = scenes.cornell((8, 8))
        sc.add([sliver], scenes.Material.make(scenes.DIFFUSE, (0.5, 0.5, 0.5), 0, 0))
        assert dark(sc) == 0, sliver
    # an emitting sliver does not matter (paths end on emitters)
    sc = scenes.cornell((8, 8))
    sc.add([((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0))], scenes.Material.make(scenes.EMIT, 0, 1, 0))
    assert dark(sc) == 1


def test_no_device_is_a_loud_error(pt):
    if pt.lib().pt_device_count() > 0:
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = pt.lib().pt_ctx_create(0, C.byref(h))
    assert rc == pt._lib.PT_E_HIP
    assert b"device" in pt.lib().pt_last_error()


@pytest.mark.parametrize("name", ["bvh_cornell", "bvh_mcornell", "bvh_tri3"])
def test_builder_matches_reference_fixture(pt, golden_meta, name):
    sc = scene_for(golden_meta["bvh"][name]["scene"], [8, 8])
    b = pt.BVH.from_scene(sc)
    b.build()
    assert b.nodes.tobytes() == load_golden(name + "_nodes").tobytes()
    assert np.array_equal(b.tri_idx, load_golden(name + "_idx"))


def test_sorted_builder_equals_resorting_builder(pt, monkeypatch):
    """The round-6 builder (per-axis lists sorted once, split stably at every partition) gives
    the round-5 builder's tree (every node's axes sorted again, PT_BUILD_RESORT=1) bit for bit:
    the example scenes, seeded random scenes, the 2k-triangle sphere, and grids with many equal
    centroids (tie groups whose least position decides, -0 against +0 among them)."""
    from ptamd import scenes
    from _randscene import random_scene
    grid = scenes.Scene("grid", scenes.cornell((8, 8)).camera)
    for i in range(24):
        for j in range(24):
            x, y = float(i % 6), float(j % 5)  # repeated centroids on every axis
            z = -0.0 if (i + j) % 3 == 0 else 0.0
            grid.add([((x, y, z), (x + 1.0, y, z), (x, y + 1.0, z))], scenes.Material.make(scenes.DIFFUSE, 0.5, 0))
    cases = [scenes.cornell((8, 8)), scenes.modified_cornell(0.3, (8, 8)), scenes.tri3((8, 8)),
             scenes.sphere_in_cornell(32, (8, 8)), grid] + [random_scene(s, n, (8, 8)) for s, n in ((1, 40), (7, 300), (9, 3000))]
    for sc in cases:
        out = []
        for resort in ("0", "1"):
            monkeypatch.setenv("PT_BUILD_RESORT", resort)
            b = pt.BVH.from_scene(sc)
            b.build()
            out.append((b.nodes.tobytes(), b.tri_idx.tobytes()))
        assert out[0] == out[1], sc.name


def test_builder_matches_reference_on_config4_mesh(pt, golden_meta):
    """Config 4's 99,044-triangle mesh: the product builder's node array and tri_idx
    hash to the reference BVH::build's own dump (380 s there, ~0.1 s here)."""
    import hashlib
    m = golden_meta["bvh_hash"]["sphere223_in_cornell"]
    sc = scene_for("sphere223_in_cornell", [8, 8])
    assert scene_hash(sc) == m["scene_sha256"]
    b = pt.BVH.from_scene(sc)
    b.build()
    assert len(b.nodes) == m["nodes"]
    h = hashlib.sha256(b.nodes.tobytes() + np.ascontiguousarray(b.tri_idx, dtype=np.int32).tobytes()).hexdigest()
    assert h == m["sha256_nodes_then_tri_idx"]


def _random_scene(rng, n, grid=None):
    if grid:  # many coincident centroids and equal costs: exercises tie-breaking
        base = rng.integers(0, grid, size=(n, 3)).astype(np.float64)
        offs = rng.integers(-2, 3, size=(n, 3, 3)).astype(np.float64)
        v = base[:, None, :] + offs
    else:
        v = (rng.normal(size=(n, 3)) * rng.uniform(1, 50))[:, None, :] + rng.normal(size=(n, 3, 3)) * rng.uniform(0.01, 3)
    return np.ascontiguousarray(v.reshape(n, 9).astype(np.float32))


@pytest.mark.parametrize("seed,n,grid", [(1, 50, None), (2, 300, None), (3, 1000, None), (4, 200, 4),
                                         (5, 700, 6), (6, 1, None), (7, 2, None), (8, 64, 1)])
def test_builder_matches_quadratic_restatement(pt, seed, n, grid):
    """The O(n log^2 n) builder against the oracle's O(n^2) restatement of BVH::build."""
    verts = _random_scene(np.random.default_rng(seed), n, grid)
    ref_nodes, ref_idx = O.bvh_build(verts)
    nodes = np.zeros(max(2 * n - 1, 1), dtype=pt.NODE_DTYPE)
    idx = np.zeros(n, dtype=np.int32)
    cnt = pt.check(pt.lib().pt_bvh_build(n, verts.ctypes.data, nodes.ctypes.data, idx.ctypes.data))
    assert cnt == len(ref_nodes)
    assert nodes[:cnt].tobytes() == ref_nodes.tobytes()
    assert np.array_equal(idx, ref_idx)


def test_builder_rejects_bad_input(pt):
    verts = np.zeros((2, 9), np.float32)
    verts[0, 3] = np.nan
    nodes = np.zeros(3, dtype=pt.NODE_DTYPE)
    idx = np.zeros(2, np.int32)
    assert pt.lib().pt_bvh_build(2, verts.ctypes.data, nodes.ctypes.data, idx.ctypes.data) == pt._lib.PT_E_ARG
    assert pt.lib().pt_bvh_build(0, verts.ctypes.data, nodes.ctypes.data, idx.ctypes.data) == pt._lib.PT_E_EMPTY


@pytest.mark.parametrize("factory", ["cornell", "modified_cornell_r0.3", "tri3"])
def test_camera_matches_oracle(pt, factory):
    sc = scene_for(factory, (321, 123))
    cam = pt.Camera.from_spec(sc.camera)
    c = cam.c
    mine = np.array([*c.pos, c.res[0], c.res[1], *c.v_res, c.cell_size, c.distance, *c.transform], np.float32)
    assert mine.tobytes() == O.camera(sc).tobytes()


def test_camera_degenerate_up_vector(pt):
    with pytest.raises(pt.PTError):
        pt.Camera((0, 0, 0), (0, 1, 0), (0, 1, 0), (8, 8), 1.0, 1.0)


@pytest.mark.parametrize("H,parts,band", [(45, 3, 4), (1024, 8, 8), (7, 8, 1), (100, 1, 8), (33, 5, 16)])
def test_part_rows_partition(pt, H, parts, band):
    counts = [pt.Renderer.part_rows(H, p, parts, band) for p in range(parts)]
    assert sum(counts) == H
    for p in range(parts):
        assert counts[p] == sum(1 for h in range(H) if (h // band) % parts == p)
    assert pt.Renderer.part_rows(H, parts, parts, band) == 0


def test_rgb8_matches_reference_quantisation(pt):
    """gamma_correct(2.2) + save_png quantisation + vertical flip (image.h:41-55),
    restated with numpy float32 ops and glibc powf through ctypes."""
    rng = np.random.default_rng(3)
    img = rng.uniform(-0.2, 1.4, size=(5, 7, 3)).astype(np.float32)
    img[0, 0] = [0, 1, 0.5]
    img[1, 1] = [np.nan, np.inf, -np.inf]
    got = pt.to_rgb8(img)
    libm = C.CDLL("libm.so.6")
    libm.powf.argtypes = [C.c_float, C.c_float]
    libm.powf.restype = C.c_float
    inv = np.float32(1) / np.float32(2.2)
    exp = np.zeros_like(got)
    for h in range(5):
        for w in range(7):
            for c in range(3):
                x = np.float32(libm.powf(float(img[5 - h - 1, w, c]), float(inv)))
                x = x if x < 1 else np.float32(1)      # std::min(1, x)
                x = x if 0 < x else np.float32(0)      # std::max(0, .)
                exp[h, w, c] = np.uint8(int(np.float32(x * np.float32(255))))
    assert np.array_equal(got, exp)


def test_png_roundtrip(pt, tmp_path):
    from PIL import Image as PILImage
    img = np.random.default_rng(0).uniform(0, 1, size=(17, 29, 3)).astype(np.float32)
    f = str(tmp_path / "x.png")
    assert pt.save_png(img, f)
    back = np.asarray(PILImage.open(f).convert("RGB"))
    assert np.array_equal(back, pt.to_rgb8(img))
    assert not pt.save_png(img, str(tmp_path / "no" / "such" / "dir.png"))


def _scene_with_nodes(pt, name, edit):
    from ptamd import _lib
    b = pt.BVH.from_scene(scene_for(name, (8, 8)))
    b.build()
    ref = pt._SceneRef(b)
    nodes = ref.nodes.copy()
    edit(nodes)
    s = _lib.pt_scene(ref.s.num_tris, ref.verts.ctypes.data, C.addressof(ref.mats), nodes.shape[0],
                      nodes.ctypes.data, ref.idx.ctypes.data)
    info = np.zeros(4, np.int32)
    return pt.lib().pt_scene_validate(C.byref(s), info.ctypes.data), info, (ref, nodes)


def test_scene_validation(pt):
    from ptamd import _lib
    rc, info, _ = _scene_with_nodes(pt, "cornell", lambda n: None)
    assert rc == 0 and info[0] == 63 and info[2] == 32  # Cornell: flat path over 32 leaves
    rc, info, _ = _scene_with_nodes(pt, "tri3", lambda n: None)
    assert rc == 0 and info[2] == 3

    def cycle(n):
        n[0]["left"] = 0
        n[0]["right"] = 0
    assert _scene_with_nodes(pt, "tri3", cycle)[0] == _lib.PT_E_ARG

    def half_leaf(n):
        n[0]["left"] = -1  # interior with one -1 child: the reference would index nodes[-1]
    assert _scene_with_nodes(pt, "tri3", half_leaf)[0] == _lib.PT_E_ARG

    def bad_range(n):
        leaf = np.where((n["left"] == -1) & (n["right"] == -1))[0][0]
        n[leaf]["tri_end"] = 99
    assert _scene_with_nodes(pt, "tri3", bad_range)[0] == _lib.PT_E_ARG

    def shrink_root(n):  # breaks box containment: still valid, but no flat path
        n[0]["rt"][0] = n[0]["lb"][0]
    rc, info, _ = _scene_with_nodes(pt, "cornell", shrink_root)
    assert rc == 0 and info[2] == 0


def test_empty_scene(pt):
    b = pt.BVH()
    with pytest.raises(pt.PTError):
        b.build()
    assert not pt.render_cpu(pt.Camera((0, 0, 0), (0, 0, 1), (0, 1, 0), (4, 4), 1.0), b, 1, 1, "/tmp/_x.png")


@pytest.mark.parametrize("name,boxes", [("cornell", 20), ("modified_cornell_r0.3", 21), ("tri3", 3)])
def test_rtc_specialised_kernel_compiles(pt, name, boxes):
    """hipRTC generates and compiles the scene-specialised flat kernel (no device needed):
    one slab test per distinct leaf box, one (c - o) * inv per distinct plane."""
    ref = pt._SceneRef(pt.BVH.from_scene(scene_for(name, (8, 8))))
    buf = C.create_string_buffer(400000)
    size = pt.lib().pt_rtc_check(C.byref(ref.s), buf, len(buf))
    assert size > 1000, pt.lib().pt_last_error()
    src = buf.value.decode()
    sign = src.split("#if KSIGN\n")[1].split("#elif PT_SHARED_CLAMP\n")[0]
    shared, plain = src.split("#elif PT_SHARED_CLAMP\n")[1].split("#endif\n")[0].split("#else\n")
    assert shared.count("const bool b") == boxes and plain.count("const bool b") == boxes
    # the sign-bit form (compiled only with PT_FLAT_SIGN_MASK=1, off by default: measured slower,
    # DESIGN.md §3.9; allowed where the coordinates are below 2^60): one fail word per box,
    # tmax + 0 (a -0 exit value counts as 0); test_origin_on_box_planes_bitexact runs it on the GPU
    assert sign.count("box_fail_bits(") == boxes and sign.count(" + 0.0f)") == boxes
    # the clamp of tmin to 0: one per distinct axis term, never more than one per box
    assert 0 < shared.count("const float c") <= boxes and "0.0f) <=" in plain and "0.0f) <=" not in shared
    assert "pt_trace_flat_rtc" in src and "SceneBoxMask" in src


def _rtc_source(pt, bvh):
    ref = pt._SceneRef(bvh)
    buf = C.create_string_buffer(400000)
    assert pt.lib().pt_rtc_check(C.byref(ref.s), buf, len(buf)) > 1000, pt.lib().pt_last_error()
    return buf.value.decode()


@pytest.mark.parametrize("case,on", [("cornell", True), ("mcornell", True), ("emit_2^100", False),
                                     ("albedo_2^127", False), ("albedo_inf", False), ("hook_off", False)])
def test_rtc_albedo_x2_gate(pt, monkeypatch, case, on):
    """The flat kernel unwinds with pre-doubled albedo (finish_path<., true>) only when the
    host can bound the radiance below 2^125 over PT_MAX_DEPTH levels with every material
    finite (pt_launch.hip: albedo_x2_ok); otherwise it keeps (2L) * albedo."""
    from ptamd import scenes
    b = pt.BVH.from_scene(scene_for("modified_cornell_r0.3" if case == "mcornell" else "cornell", (8, 8)))
    scale = {"emit_2^100": ("emit", 2.0 ** 100), "albedo_2^127": ("color", 2.0 ** 127),
             "albedo_inf": ("color", float("inf"))}.get(case)
    if scale:
        field_, f = scale
        t = b.triangles[0]
        m = t.material
        vals = {"color": m.color, "emit": m.emit_color}
        vals[field_] = tuple(c * f if c else f for c in vals[field_])
        b.triangles[0] = pt.Triangle(t.v1, t.v2, t.v3, pt.Material(m.type, vals["color"], vals["emit"], m.roughness))
        b.built = False
        b._packed = None
    if case == "hook_off":
        monkeypatch.setenv("PT_TEST_HOOKS", "1")
        monkeypatch.setenv("PT_ALBEDO_X2", "0")
    src = _rtc_source(pt, b)
    assert f"kAlbedoX2 = {'true' if on else 'false'};" in src


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("factory", ["sphere223", "sphere32", "cornell", "mcornell", "grid"])
def test_wide_tree_invariants(pt, width, factory):
    """The quantised wide tree: checked exactly on the host
    (pt_debug_wide_verify) — every quantised child box contains the reference's node box
    as real numbers, child links, ranks and exact leaf boxes right, each triangle stored
    once. Includes config 4's 99,044-triangle mesh and a far-from-origin, tiny-extent grid
    (quantisation steps at the float ulp)."""
    from ptamd import scenes
    if factory.startswith("sphere"):
        sc = scenes.sphere_in_cornell(int(factory[6:]), (8, 8))
    elif factory == "cornell":
        sc = scenes.cornell((8, 8))
    elif factory == "mcornell":
        sc = scenes.modified_cornell(0.3, (8, 8))
    else:
        rng = np.random.default_rng(3)
        base = np.array([3.0e5, -7.5e4, 1.25e6])
        tris = []
        for _ in range(300):
            c = base + rng.uniform(-0.05, 0.05, 3)
            tris.append(tuple(tuple(float(np.float32(x)) for x in c + rng.uniform(-1e-3, 1e-3, 3)) for _ in range(3)))
        cam = scenes.CameraSpec(tuple(base - [0, 0, 1]), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (8, 8), 60.0, 1.0)
        sc = scenes.Scene("grid", cam, tris, [scenes.Material.make(2, (0.5, 0.5, 0.5), (0, 0, 0))] * len(tris))
    bvh = pt.BVH.from_scene(sc)
    bvh.build()
    ref = pt._SceneRef(bvh)
    assert pt.lib().pt_debug_wide_verify(C.byref(ref.s), width) == 0


def test_scene_arrays_round_each_value_once(pt):
    """BVH.verts()/materials() (the ctypes scene the C ABI reads) hold every value rounded
    once to float32, field by field, as the reference's float members do: signed zeros,
    doubles between floats and per-triangle material objects included."""
    import ptamd
    m_a = ptamd.Material(ptamd.DIFFUSE, (0.1, 0.2, 0.30000001), (-0.0, 0.0, 1e-40), 0.3)
    m_b = ptamd.Material(ptamd.SPECULAR, (1.0 / 3.0, 2.5, 7.0), (0.0, 0.0, 0.0), 0.123456789)
    bvh = ptamd.BVH()
    rng = np.random.default_rng(3)
    for i in range(50):
        v = rng.normal(size=9) * 100.0
        bvh.add_triangle(ptamd.Triangle(tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:9]),
                                        m_a if i % 3 else ptamd.Material(m_b.type, m_b.color, m_b.emit_color,
                                                                         m_b.roughness)))
    verts = bvh.verts()
    mats = bvh.materials()
    for i, t in enumerate(bvh.triangles):
        want = np.array([*t.v1, *t.v2, *t.v3], dtype=np.float64).astype(np.float32)
        assert verts[i].view(np.uint32).tolist() == want.view(np.uint32).tolist()
        m = t.material
        assert mats[i].type == m.type
        for got, ref in ((list(mats[i].color), m.color), (list(mats[i].emit), m.emit_color),
                         ([mats[i].roughness], [m.roughness])):
            assert np.array(got, dtype=np.float32).view(np.uint32).tolist() == \
                np.array(ref, dtype=np.float64).astype(np.float32).view(np.uint32).tolist()


def test_builder_signed_zero_and_tied_centroids(pt):
    """Ranges of >= 1024 triangles sort their sweep keys by radix: centroids of -0 and +0
    (equal for the reference's `<`) and long runs of tied values must keep the
    reference's (value, position) order."""
    rng = np.random.default_rng(11)
    n = 1100
    v = rng.integers(-3, 4, size=(n, 3, 3)).astype(np.float32)
    v[: n // 2, :, 0] = np.where(rng.random((n // 2, 3)) < 0.5, -0.0, 0.0)  # x centroids of +-0
    v[:, 1, 1] += 0.5  # non-degenerate triangles
    verts = np.ascontiguousarray(v.reshape(n, 9))
    ref_nodes, ref_idx = O.bvh_build(verts)
    nodes = np.zeros(2 * n - 1, dtype=pt.NODE_DTYPE)
    idx = np.zeros(n, dtype=np.int32)
    cnt = pt.check(pt.lib().pt_bvh_build(n, verts.ctypes.data, nodes.ctypes.data, idx.ctypes.data))
    assert cnt == len(ref_nodes)
    assert nodes[:cnt].tobytes() == ref_nodes.tobytes()
    assert np.array_equal(idx, ref_idx)


def test_wide_tree_shape_and_lds_top(pt, monkeypatch):
    """Config 4's 99,044-triangle mesh: the SAH-optimal collapse gives
    19,216 8-wide nodes on 12 levels (the greedy round-2 rule: 35,417 on 10); every leaf
    holds one triangle, so the triangle records are the compact 48-B form; the LDS top
    offer is an index prefix of 4 KiB (32 nodes), or the whole levels that fit in it (the
    root, its 8 children and the third level's 10 nodes) with PT_WIDE_TOP_PARTIAL=0. No
    device needed (pt_scene_info)."""
    from ptamd import scenes
    bvh = pt.BVH.from_scene(scenes.sphere_in_cornell(223, (8, 8)))
    bvh.build()
    info = pt.scene_info(bvh)
    assert (info["wide_nodes"], info["wide_levels"], info["wide_width"]) == (19216, 12, 8)
    assert info["wide_tris"] == 99044 and info["wide_top"] == 32 and info["wide_record_bytes"] == 48
    monkeypatch.setenv("PT_WIDE_TOP_PARTIAL", "0")
    assert pt.scene_info(bvh)["wide_top"] == 19
    monkeypatch.setenv("PT_WIDE_COLLAPSE", "greedy")
    g = pt.scene_info(bvh)
    assert (g["wide_nodes"], g["wide_levels"]) == (35417, 10)


def shrink_leaf_boxes(nodes: np.ndarray, tri_idx: np.ndarray, verts: np.ndarray, every: int = 3) -> int:
    """Shrink the box of every `every`-th single-triangle leaf to the middle of its
    triangle's AABB on each axis where the AABB has extent (a tree a caller could hand to
    the C ABI: still contained in every ancestor box). Returns the leaves changed."""
    changed = 0
    leaves = np.nonzero((nodes["left"] == -1) & (nodes["right"] == -1))[0]
    for k, n in enumerate(leaves):
        if k % every:
            continue
        v = verts[tri_idx[nodes["tri_start"][n]]].reshape(3, 3)
        lo, hi = v.min(axis=0), v.max(axis=0)
        span = hi - lo
        nodes["lb"][n] = np.where(span > 0, lo + np.float32(0.3) * span, lo).astype(np.float32)
        nodes["rt"][n] = np.where(span > 0, hi - np.float32(0.3) * span, hi).astype(np.float32)
        changed += 1
    return changed


def test_wide_records_keep_leaf_box_unless_triangle_aabb(pt):
    """The 48-B wide triangle records rebuild a leaf's box from its vertices, so they are
    chosen only when every single-triangle leaf's box IS its triangle's AABB (trees from
    BVH::build). A tree with other leaf boxes (here: shrunk, still nested in their
    ancestors) keeps the 64-B records that carry the stored box (pt_host.cpp
    build_wide), and its wide tree still verifies exactly."""
    from ptamd import scenes
    bvh = pt.BVH.from_scene(scenes.sphere_in_cornell(32, (8, 8)))
    bvh.build()
    assert pt.scene_info(bvh)["wide_record_bytes"] == 48
    nodes = bvh.nodes.copy()
    assert shrink_leaf_boxes(nodes, bvh.tri_idx, bvh.verts()) > 0
    bvh.nodes = nodes
    info = pt.scene_info(bvh)
    assert info["wide_nodes"] > 0 and info["wide_record_bytes"] == 64
    ref = pt._SceneRef(bvh)  # keeps the arrays alive during the call
    assert pt.lib().pt_debug_wide_verify(C.byref(ref.s), 8) == 0


def test_scene_packing_is_thread_count_independent(pt, monkeypatch):
    """pack_scene runs the SAH collapse, the wide nodes and triangle records, the node array
    and the rank-ordered triangles on several threads (round 6): its output
    (every array and scalar, pt_debug_pack_hash) is the same at 1, 3 and 8 threads for a mesh
    large enough to take every threaded branch, in each plane format and width, for trees with
    shrunk leaf boxes (64-B records) and with two-triangle leaves, and for a random scene."""
    from ptamd import scenes
    from _randscene import random_scene

    def bvh_of(sc, edit=None):
        b = pt.BVH.from_scene(sc)
        b.build()
        if edit:
            nodes = b.nodes.copy()
            assert edit(nodes, b) > 0
            b.nodes = nodes
        return b

    sphere = bvh_of(scenes.sphere_in_cornell(130, (8, 8)))
    assert len(sphere.triangles) > 16384  # node array past the threaded threshold
    cases = [(sphere, {}), (sphere, {"PT_WIDE_PLANES": "byte"}), (sphere, {"PT_WIDE_PLANES": "f32"}),
             (sphere, {"PT_WIDE_W": "4"}), (sphere, {"PT_WIDE_COLLAPSE": "greedy"}),
             (bvh_of(scenes.sphere_in_cornell(60, (8, 8)), lambda n, b: shrink_leaf_boxes(n, b.tri_idx, b.verts())), {}),
             (bvh_of(scenes.sphere_in_cornell(60, (8, 8)), lambda n, b: _merge_leaf_pairs(n)), {}),
             (bvh_of(random_scene(9, 3000, (8, 8))), {})]
    for b, env in cases:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ref = pt._SceneRef(b)  # keeps the arrays alive during the calls
        hashes = set()
        for threads in ("1", "3", "8"):
            monkeypatch.setenv("PT_PACK_THREADS", threads)
            h = C.c_uint64()
            pt.check(pt.lib().pt_debug_pack_hash(C.byref(ref.s), C.byref(h)))
            hashes.add(h.value)
        assert len(hashes) == 1, env
        assert pt.lib().pt_debug_wide_verify(C.byref(ref.s), int(env.get("PT_WIDE_W", 8))) == 0
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("fail_step", [-1, 0, 1, 2, 3, 4])
@pytest.mark.parametrize("n_devices", [1, 2, 8])
def test_rccl_failed_group_aborts_its_communicators(pt, fail_step, n_devices):
    """Multi-device gather (pt_multi.hip): a failure anywhere in the RCCL path — init, group
    start, a send, a recv, group end — leaves no live communicator behind (every one of the
    failed set is ncclCommAbort'ed), takes the set out of the cache, and the next gather over
    the same devices gets a fresh set. Driven through a fake RCCL table (no device needed)."""
    out = np.zeros(6, dtype=np.int64)
    assert pt.lib().pt_debug_rccl_failover(n_devices, fail_step, out.ctypes.data) == 0
    created, aborted, live, entries, fresh, first_rc = out.tolist()
    if fail_step == -1:
        assert first_rc == 0 and entries == 1 and aborted == 0
        assert created == n_devices and live == n_devices and fresh == 0  # the cached set is reused
    else:
        assert first_rc != 0 and entries == 0
        init_made = n_devices // 2 if fail_step == 0 else n_devices
        assert aborted == init_made  # every communicator the failed attempt created
        assert created == init_made + n_devices and live == n_devices and fresh == 1


def test_rtc_disk_cache_reuses_and_rejects_corrupt_entries(pt, tmp_path, monkeypatch):
    """The scene kernel's on-disk code-object cache (pt_rtc.hip): a compile is stored
    under sha256(source, device headers, options, hipRTC version); a later request (here:
    after this process forgets its own compiles) loads the verified entry instead of
    compiling; a corrupted, truncated or foreign entry is rejected, recompiled and
    rewritten. hipRTC compiles without a device (pt_rtc_check)."""
    import ptamd
    from ptamd import scenes
    monkeypatch.setenv("PT_RTC_CACHE_DIR", str(tmp_path))
    L = pt.lib()
    bvh = ptamd.BVH.from_scene(scenes.cornell((8, 8)))
    bvh.build()
    ref = pt._SceneRef(bvh)
    stat = lambda: (L.pt_debug_rtc_cache(1), L.pt_debug_rtc_cache(2), L.pt_debug_rtc_cache(3))
    assert L.pt_debug_rtc_cache(0) == 0
    h0, r0, c0 = stat()
    size = L.pt_rtc_check(C.byref(ref.s), None, 0)
    assert size > 0 and stat() == (h0, r0, c0 + 1)
    entries = list(tmp_path.glob("*.co"))
    assert len(entries) == 1 and len(entries[0].stem) == 64
    good = entries[0].read_bytes()
    assert good[:8] == b"PTRTC001" and len(good) == 8 + 64 + 8 + 32 + size
    L.pt_debug_rtc_cache(0)
    assert L.pt_rtc_check(C.byref(ref.s), None, 0) == size and stat() == (h0 + 1, r0, c0 + 1)
    bad_payload = bytearray(good)
    bad_payload[-7] ^= 0x40
    for k, bad in enumerate((bytes(bad_payload), good[:-16], good[:8] + b"0" * 64 + good[72:])):
        entries[0].write_bytes(bad)
        L.pt_debug_rtc_cache(0)
        assert L.pt_rtc_check(C.byref(ref.s), None, 0) == size
        assert stat() == (h0 + 1, r0 + k + 1, c0 + k + 2), k
        assert entries[0].read_bytes() == good, k  # the recompiled entry replaced the bad one
    monkeypatch.setenv("PT_RTC_CACHE", "0")  # off: neither read nor written
    entries[0].unlink()
    L.pt_debug_rtc_cache(0)
    assert L.pt_rtc_check(C.byref(ref.s), None, 0) == size and not list(tmp_path.glob("*.co"))


def test_rtc_disk_cache_trusts_only_owner_only_entries(pt, tmp_path, monkeypatch):
    """the cache directory is created 0700, entries 0600, and an entry writable by
    group or others is never loaded as GPU code (it is rejected and recompiled)."""
    import os
    import stat as S
    import ptamd
    from ptamd import scenes
    d = tmp_path / "cache"
    monkeypatch.setenv("PT_RTC_CACHE_DIR", str(d))
    L = pt.lib()
    sc = scenes.cornell((8, 8))
    a, b, c = sc.tris[3]
    sc.tris[3] = ((a[0] + 0.375, a[1], a[2]), b, c)  # a source no other CPU test compiles
    bvh = ptamd.BVH.from_scene(sc)
    bvh.build()
    ref = pt._SceneRef(bvh)
    L.pt_debug_rtc_cache(0)
    assert L.pt_rtc_check(C.byref(ref.s), None, 0) > 0
    assert S.S_IMODE(os.stat(d).st_mode) == 0o700
    (entry,) = list(d.glob("*.co"))
    assert S.S_IMODE(os.stat(entry).st_mode) == 0o600
    os.chmod(entry, 0o666)
    r0, c0 = L.pt_debug_rtc_cache(2), L.pt_debug_rtc_cache(3)
    L.pt_debug_rtc_cache(0)
    assert L.pt_rtc_check(C.byref(ref.s), None, 0) > 0
    assert L.pt_debug_rtc_cache(2) == r0 + 1 and L.pt_debug_rtc_cache(3) == c0 + 1
