"""Caller-built trees on every GPU kernel path (tests/_trees.py's transforms through
pt_ctx_set_scene): renders, ray queries and first-hit AOVs, float32 bits and ray counts
against the oracle walking the same nodes (`_oracle.render(nodes=, idx=)`,
`_refwalk.ref_walk`; the oracle's caller-tree walk is pinned to the compiled reference by
tests/test_trees_cpu.py). No tolerances. Each case asserts the kernel path it ran on
(pt_stats.kernel_path: 0 / 1 tree walk, 2 flat table, 3 flat hipRTC, 4 wide, 5 flat table with
the scene's flags), so none can pass on another path than the one it names."""
import numpy as np
import pytest

import _oracle as O
import _refwalk as RW
import _treecases as TC
import _trees as T

pytestmark = pytest.mark.gpu

RES, SPP, DEPTH = (24, 20), 4, 5
F32 = np.float32
TREE_WALK = {"PT_FLAT": "0", "PT_WIDE": "0"}
# kernel-path modes of the render matrix: (hooks, the path a contained partition tree takes)
MODES = {"default": ({}, 3), "table": ({"PT_RTC": "0"}, 2), "table_generic": ({"PT_RTC": "0", "PT_FLAT_FAST": "0"}, 2),
         "wide": ({"PT_WIDE": "1"}, 4), "tree": (TREE_WALK, (0, 1))}
FLAT_VARIANTS = ("merged2", "merged5", "root_leaf", "empty", "chain_right", "chain_left")


@pytest.fixture(scope="module")
def ptamd_mod():
    import ptamd
    if ptamd.lib().pt_device_count() <= 0:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    return ptamd


def _render(ptamd, monkeypatch, name, variant, env, res=RES, spp=SPP, depth=DEPTH):
    """Render the case under the hooks of `env`, compare with the oracle on the same nodes
    (bits and ray count) and return (stats, context flags)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = TC.scene(name, res)
    r = ptamd.Renderer(0)
    try:
        r.set_scene(TC.to_bvh(ptamd, TC.case(name, variant)))
        img, st = r.render(ptamd.Camera.from_spec(sc.camera), spp, depth)
        flags = r.flags()
    finally:
        r.close()
    ref, rays = TC.oracle_image(name, variant, tuple(res), spp, depth)
    bad = np.flatnonzero(RW.bits(img).reshape(-1) != RW.bits(ref).reshape(-1))
    print(f"{name}/{variant} {env}: kernel_path {st['kernel_path']}, rays {st['rays']} (oracle {rays}), "
          f"{bad.size} differing floats")
    assert bad.size == 0 and st["rays"] == rays, (name, variant, env, st["kernel_path"])
    return st, flags


def _is(path, want):
    return path in want if isinstance(want, tuple) else path == want


# ---------------------------------------------------------------- render matrix
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("variant", FLAT_VARIANTS)
@pytest.mark.parametrize("name", ["cornell", "mcornell"])
def test_contained_trees_on_every_path(ptamd_mod, monkeypatch, name, variant, mode):
    """Nested partition trees of at most 64 leaves: the hipRTC flat kernel by default, the table
    kernels with PT_RTC=0, the wide walk with PT_WIDE=1, the tree walk with both off. The table
    kernel with the scene's flags (5) needs leaf k = triangle rank k, which only the chains
    keep; multi-triangle and empty leaves run the generic table kernel (2). A root leaf has no
    wide tree (pack_scene builds one only under an interior root): PT_WIDE=1 leaves it flat."""
    env, want = MODES[mode]
    if mode == "table" and variant.startswith("chain"):
        want = 5
    if mode == "wide" and variant == "root_leaf":
        want = 3
    st, flags = _render(ptamd_mod, monkeypatch, name, variant, env)
    assert _is(st["kernel_path"], want), (st["kernel_path"], want)
    if variant == "root_leaf":
        assert flags["wide_nodes"] == 0
    else:
        assert flags["wide_nodes"] > 0


@pytest.mark.parametrize("env", [{"PT_PAIRS": "0"}, {"PT_PAIR_QUEUE": "16"}, {"PT_BOX_PAIRS": "1"},
                                 {"PT_FORCE_EXACT_SLAB": "1"}, {"PT_RTC": "0", "PT_PAIRS": "0"},
                                 {"PT_RTC": "0", "PT_PAIR_QUEUE": "16"}])
@pytest.mark.parametrize("name", ["cornell", "mcornell"])
def test_two_triangle_leaves_pair_rounds_and_lane_loops(ptamd_mod, monkeypatch, name, env):
    """merged(2) on the flat kernels' separate multi-triangle code: the per-lane loops
    (PT_PAIRS=0), a 16-entry pair queue (overflow falls back to them), box-level pairs asked
    for and declined (they need one triangle per leaf: the generated source says kBoxes = 0)
    and the exact slab form; hipRTC-specialised and table kernel."""
    if "PT_BOX_PAIRS" in env:
        from test_capi import _rtc_source
        monkeypatch.setenv("PT_BOX_PAIRS", "1")
        assert "kBoxes = 0;" in _rtc_source(ptamd_mod, TC.to_bvh(ptamd_mod, TC.case(name, "merged2")))
        assert "kBoxes = 0;" not in _rtc_source(ptamd_mod, TC.to_bvh(ptamd_mod, TC.case(name, "build")))
    st, _ = _render(ptamd_mod, monkeypatch, name, "merged2", env)
    assert st["kernel_path"] == (2 if "PT_RTC" in env else 3)


@pytest.mark.parametrize("env", [{}, {"PT_FLAT": "1", "PT_WIDE": "1"}, {"PT_RTC": "0"}])
@pytest.mark.parametrize("variant", TC.TREE_ONLY)
@pytest.mark.parametrize("name", ["cornell", "mcornell"])
def test_non_partition_and_unnested_trees_take_the_tree_walk(ptamd_mod, monkeypatch, name, variant, env):
    """duplicated / dropped (identity ranks) and uncontained (boxes that do not nest): no flat
    list, no wide tree, no hipRTC kernel, whatever PT_FLAT and PT_WIDE ask for."""
    st, flags = _render(ptamd_mod, monkeypatch, name, variant, env)
    assert st["kernel_path"] in (0, 1) and flags["wide_nodes"] == 0 and not flags["rtc"]
    if variant == "dropped" and not env:  # the triangle is invisible: another image than BVH::build's tree
        base, _ = TC.oracle_image(name, "build")
        assert not np.array_equal(RW.bits(base), RW.bits(TC.oracle_image(name, variant)[0]))


@pytest.mark.parametrize("env", [{"PT_WIDE_W": "4", "PT_WIDE_PLANES": "byte"}, {"PT_WIDE_W": "4", "PT_WIDE_PLANES": "f16"},
                                 {"PT_WIDE_W": "4", "PT_WIDE_PLANES": "f32"}, {"PT_WIDE_W": "8", "PT_WIDE_PLANES": "byte"},
                                 {"PT_WIDE_W": "8", "PT_WIDE_PLANES": "f16"}, {"PT_WIDE_W": "8", "PT_WIDE_PLANES": "f32"}])
def test_wide_walk_leaf_range_decode(ptamd_mod, monkeypatch, env):
    """The sphere scene with leaves of up to 31 triangles (8 x 31 = 248 <= 255: the leaf ends
    are bytes) on the wide walk's general leaf-range decode, both widths, every plane format.
    Its 16 leaves fit the flat list, so PT_WIDE=1 asks for the wide walk."""
    st, flags = _render(ptamd_mod, monkeypatch, "sphere12", "merged31", dict(env, PT_WIDE="1"))
    assert st["kernel_path"] == 4 and flags["wide_nodes"] > 0


@pytest.mark.parametrize("variant,path", [("merged2", 4), ("merged5", 4), ("empty", 4), ("chain_right", 4),
                                          ("chain_left", 4)])
def test_sphere_trees_past_the_flat_list_take_the_wide_walk(ptamd_mod, monkeypatch, variant, path):
    """More than 64 leaves: the wide walk by itself (no hook), with multi-triangle leaves,
    empty leaves (skipped by the wide builder) and 296-level chains (43 wide levels; the exact
    walk's stack rows in global memory)."""
    st, flags = _render(ptamd_mod, monkeypatch, "sphere12", variant, {})
    assert st["kernel_path"] == path and flags["wide_nodes"] > 0


@pytest.mark.parametrize("env,want", [({"PT_WIDE": "1"}, 3), (dict(TREE_WALK, PT_WIDE="1", PT_FLAT="0"), (0, 1)),
                                      ({"PT_WIDE": "1", "PT_RTC": "0"}, 2)])
def test_wide_builder_fallback_past_255_leaf_triangles(ptamd_mod, monkeypatch, env, want):
    """merged(K_BIG): one wide node would collect 296 > 255 leaf triangles, so the scene gets
    no wide tree and PT_WIDE=1 cannot give the wide walk; leaves of 135 and 136 triangles on
    the flat kernels' range loops and on the tree walk."""
    variant = f"merged{TC.K_BIG}"
    assert ptamd_mod.scene_info(TC.to_bvh(ptamd_mod, TC.case("sphere12", variant)))["wide_nodes"] == 0
    st, flags = _render(ptamd_mod, monkeypatch, "sphere12", variant, env)
    assert flags["wide_nodes"] == 0 and _is(st["kernel_path"], want)


@pytest.mark.parametrize("env,want", [({}, 3), ({"PT_RTC": "0"}, 5), ({"PT_RTC": "0", "PT_FLAT_FAST": "0"}, 2),
                                      ({"PT_WIDE": "1"}, 3), (TREE_WALK, 1)])
def test_one_triangle_scene(ptamd_mod, monkeypatch, env, want):
    """One emitting triangle in front of the camera: a one-node tree, most paths miss. Its leaf
    holds triangle rank 0 alone, so the table kernel with the scene's flags (5) applies."""
    st, flags = _render(ptamd_mod, monkeypatch, "onetri", "root_leaf", env)
    assert flags["wide_nodes"] == 0 and _is(st["kernel_path"], want)
    assert 0 < st["rays"] <= RES[0] * RES[1] * SPP  # every path ends at its first ray: a hit emits, a miss is black


# ---------------------------------------------------------------- queries and AOVs
def _same(t, tri, t_ref, tri_ref):
    bad = np.flatnonzero((RW.bits(t) != RW.bits(t_ref)) | (tri != tri_ref))
    assert bad.size == 0, f"{bad.size} rays differ, first {bad[:5]}: got {t[bad[:5]]} {tri[bad[:5]]}, " \
                          f"want {t_ref[bad[:5]]} {tri_ref[bad[:5]]}"


def _any_hit_case(t_ref, tri_ref):
    """Per-ray tmax as tests/test_query_gpu.py's test_any_hit: below, at and just above the
    closest hit and no bound for hits; 1 and no bound for misses."""
    n = t_ref.shape[0]
    pick = np.random.default_rng(5).integers(4, size=n)
    with np.errstate(invalid="ignore"):
        hit_choices = np.stack([F32(0.5) * t_ref, t_ref, np.nextafter(t_ref, F32(np.inf)), np.full(n, 1e30, F32)])
    miss_choices = np.stack([np.full(n, 1.0, F32), np.full(n, 1e30, F32)])
    tmax = np.where(tri_ref >= 0, hit_choices[pick, np.arange(n)], miss_choices[pick % 2, np.arange(n)]).astype(F32)
    return tmax, (t_ref < tmax).astype(np.int32)


@pytest.fixture()
def renderer(ptamd_mod, monkeypatch):
    """A context for one caller tree; no hipRTC compile (queries and AOVs never use it)."""
    monkeypatch.setenv("PT_RTC", "0")
    made = []

    def get(name, variant):
        r = ptamd_mod.Renderer(0)
        made.append(r)
        r.set_scene(TC.to_bvh(ptamd_mod, TC.case(name, variant)))
        return r

    yield get
    for r in made:
        r.close()


QUERY_CASES = [(n, v) for n in ("cornell", "mcornell") for v in TC.VARIANTS if v != "merged31"] + \
              [("sphere12", "merged31"), ("sphere12", f"merged{TC.K_BIG}"), ("sphere12", "chain_right"), ("onetri", "root_leaf")]


@pytest.mark.parametrize("name,variant", QUERY_CASES)
def test_queries_on_caller_trees(renderer, name, variant):
    """Renderer.intersect, closest hit and any hit with a per-ray tmax, against the oracle's walk
    of the caller's nodes: 256 seeded rays and the 16 with inf / NaN components. The triangle
    ids are the caller's (through tri_idx for the chains, through identity ranks where the
    leaves do not partition the positions)."""
    r = renderer(name, variant)
    o, d, t_ref, tri_ref = TC.expected(name, variant)
    (t, tri), st = r.intersect(o, d)
    _same(t, tri, t_ref, tri_ref)
    assert st["rays"] == o.shape[0] and st["hits"] == int((tri_ref >= 0).sum()) and st["launches"] == 1
    assert st["lds_stack"] == (1 if T.depth(TC.case(name, variant).nodes) <= 64 else 0)
    tmax, want = _any_hit_case(t_ref, tri_ref)
    assert (tri_ref >= 0).any() and (name == "onetri" or 0 < want.sum() < (tri_ref >= 0).sum())
    occ, st = r.intersect(o, d, any_hit=True, tmax=tmax)
    assert np.array_equal(occ, want) and st["hits"] == int(want.sum())
    occ, _ = r.intersect(o, d, any_hit=True)
    assert np.array_equal(occ, (tri_ref >= 0).astype(np.int32))


@pytest.mark.parametrize("name,variant", QUERY_CASES)
def test_aov_on_caller_trees(ptamd_mod, renderer, name, variant):
    """Renderer.aov at 16 x 16: `tri` is the caller's triangle id (the oracle's walk of the ray
    channel over the caller's nodes), `albedo` and `emission` that triangle's material, `t` and
    `tri` equal a query of the `ray` channel, and a dropped triangle never appears."""
    c = TC.case(name, variant)
    r = renderer(name, variant)
    cam = ptamd_mod.Camera.from_spec(TC.scene(name, (16, 16)).camera)
    a, st = r.aov(cam, sample=0)
    o, d = a["ray"][..., 0:3].reshape(-1, 3), a["ray"][..., 3:6].reshape(-1, 3)
    t_ref, tri_ref = RW.ref_walk(c.nodes, c.idx, c.verts, o, d)
    _same(a["t"].reshape(-1), a["tri"].reshape(-1), t_ref, tri_ref)
    (t, tri), _ = r.intersect(o, d)
    _same(t, tri, a["t"].reshape(-1), a["tri"].reshape(-1))
    hit = a["tri"] >= 0
    assert hit.any() and st["rays"] == 256 and st["hits"] == int(hit.sum())
    for ch, cols in (("albedo", slice(0, 3)), ("emission", slice(3, 6))):
        assert np.array_equal(RW.bits(a[ch][hit]), RW.bits(c.mvals[a["tri"][hit], cols]))
        assert not RW.bits(a[ch][~hit]).any()
    if variant in ("dropped", "duplicated"):
        # the camera's centre ray hits the triangle in BVH::build's tree, so its pixels see it
        _, base_tri = RW.ref_walk(c.base_nodes, c.base_idx, c.verts, o, d)
        assert c.tri in base_tri.tolist()
        assert (c.tri in a["tri"].reshape(-1).tolist()) == (variant == "duplicated")


# ---------------------------------------------------------------- depth
def test_query_stack_rows_by_tree_depth(renderer):
    """Right-deep chains of depth 60 and 70 (61 and 71 triangles in the random-scene room) fill
    the child-pair walk's stack to its bound: the rows stay in LDS up to 64 (lds_stack 1) and
    go to global memory past that (0), with no hook set; both match the oracle."""
    for name, lds in (("rand61", 1), ("rand71", 0)):
        c = TC.case(name, "chain_right")
        assert T.depth(c.nodes) == len(c.idx) - 1 == int(name[4:]) - 1
        r = renderer(name, "chain_right")
        o, d, t_ref, tri_ref = TC.expected(name, "chain_right")
        (t, tri), st = r.intersect(o, d)
        _same(t, tri, t_ref, tri_ref)
        assert st["lds_stack"] == lds, (name, st)
        tmax, want = _any_hit_case(t_ref, tri_ref)
        occ, st = r.intersect(o, d, any_hit=True, tmax=tmax)
        assert np.array_equal(occ, want) and st["lds_stack"] == lds


@pytest.mark.parametrize("name,env,want", [("rand61", {}, 3), ("rand61", {"PT_WIDE": "1"}, 4), ("rand71", {}, 4),
                                           ("rand71", {"PT_WIDE_W": "4"}, 4)])
def test_deep_chains_render_on_flat_and_wide_paths(ptamd_mod, monkeypatch, name, env, want):
    """The depth-60 chain has 61 leaves (the flat list holds 64), the depth-70 chain 71 (wide by
    itself); the exact walk of both keeps tree-depth stack rows in global memory."""
    st, _ = _render(ptamd_mod, monkeypatch, name, "chain_right", env)
    assert st["kernel_path"] == want


@pytest.mark.parametrize("name", ["rand61", "rand71"])
def test_deep_chains_render_on_the_tree_walk(ptamd_mod, monkeypatch, name):
    """The tree-walk kernel keeps one stack row per tree level in LDS: 256 lanes x (60 + 8) and
    (70 + 8) rows x 4 B = 68 and 78 KiB of dynamic LDS at path depth 5, more than 64 KiB."""
    st, _ = _render(ptamd_mod, monkeypatch, name, "chain_right", TREE_WALK)
    assert st["kernel_path"] == 0


def test_tree_walk_refuses_a_stack_past_the_lds(ptamd_mod, monkeypatch):
    """The 296-triangle chain (depth 295) on the tree walk would need 256 x (295 + 8) x 4 B =
    303 KiB of LDS: a loud PT_E_ARG before any launch, and the context still renders the same
    scene on the wide walk afterwards."""
    for k, v in TREE_WALK.items():
        monkeypatch.setenv(k, v)
    sc = TC.scene("sphere12", RES)
    cam = ptamd_mod.Camera.from_spec(sc.camera)
    r = ptamd_mod.Renderer(0)
    try:
        r.set_scene(TC.to_bvh(ptamd_mod, TC.case("sphere12", "chain_right")))
        with pytest.raises(ptamd_mod.PTError) as e:
            r.render(cam, SPP, DEPTH)
        assert e.value.code == ptamd_mod._lib.PT_E_ARG and "LDS" in str(e.value)
        for k in TREE_WALK:
            monkeypatch.delenv(k)
        img, st = r.render(cam, SPP, DEPTH)
    finally:
        r.close()
    ref, rays = TC.oracle_image("sphere12", "chain_right")
    assert st["kernel_path"] == 4 and np.array_equal(RW.bits(img), RW.bits(ref)) and st["rays"] == rays
