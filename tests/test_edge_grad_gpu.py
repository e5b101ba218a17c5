"""The gradient kernels (pt_grad_kernel, pt_grad_cam_kernel, pt_nee_grad_kernel,
pt_nee_grad_cam_kernel through Renderer.trace_grad, trace_nee_grad and render_grad) on the cases of
tests/_edgegrad.py: edge scenes along caller and camera rays, crafted LCG states, large, small and
non-finite rays, edge values of the materials and of the upstream gradient, one output alone, and
every placement of scene, stack, records and table. Every call is held to `_edgegrad.assert_call`
against the restatement and the host form; tests/test_edge_grad_cpu.py holds the host form to the
same rule and checks on the restatement that no case is empty. DESIGN.md §3.30 lists which case
drives which kernel form. Each case is a handful of launches of at most 561 paths x 3 samples."""
import numpy as np
import pytest

import _edgegrad as EG
from _plans import _planned
from test_nee_gpu import PLACEMENTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts():
    """One context per (member, resolution), scene uploaded; closed at the end of the module. None
    of these tests renders with the flat kernels, so the scene-specialised one is not compiled."""
    import ptamd
    if ptamd.lib().pt_device_count() <= 0:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    made = {}

    def get(member, res=EG.C_RES):
        key = (member, tuple(res))
        if key not in made:
            sc = EG.make_scene(member, res)
            bvh = ptamd.BVH.from_scene(sc)
            bvh.build()
            r = ptamd.Renderer(0)
            with pytest.MonkeyPatch.context() as m:
                m.setenv("PT_RTC", "0")
                r.set_scene(bvh)
            made[key] = (r, bvh, ptamd.Camera.from_spec(sc.camera))
        return made[key]

    yield get
    for r, _, _ in made.values():
        r.close()


def _ray(contexts, member, rays, mode, what="", **kw):
    """The device against the restatement and the host form. Returns (result, stats, Expected, Summary)."""
    r, bvh, _ = contexts(member)
    want = kw.get("want", EG.WANT_BOTH)
    X = EG.terms(member, rays, mode, **{k: v for k, v in kw.items() if k != "want"})
    host, st_h = EG.ray_call(bvh, member, rays, mode, **kw)
    got, st = EG.ray_call(r, member, rays, mode, **kw)
    Z = EG.assert_call(got, st, X, want, what or f"{member} {rays} {mode} {kw}", host, st_h)
    return got, st, X, Z


def _render(contexts, member, res, mode, spp, what="", **kw):
    r, bvh, cam = contexts(member, res)
    want = kw.get("want", EG.WANT_BOTH)
    X = EG.terms(member, ("camera", tuple(res)), mode, spp, EG.RENDER_SEED, **{k: v for k, v in kw.items() if k != "want"})
    host, st_h = EG.render_call(bvh, cam, member, res, mode, spp, **kw)
    got, st = EG.render_call(r, cam, member, res, mode, spp, **kw)
    Z = EG.assert_call(got, st, X, want, what or f"{member} {res} {mode} {kw}", host, st_h, shape=(res[1], res[0]))
    return got, st, X, Z


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("mode", EG.MODES)
@pytest.mark.parametrize("member", EG.A_MEMBERS)
def test_edge_members_along_caller_rays(contexts, member, mode):
    """Scaled scenes, exact ties, degenerate emitters, the zero-normal sheet, one-leaf trees, far
    lights and lights that absorb the table, 1 and 3 samples. On a doubled member the triangle of a
    tied pair that loses the tie gets no term: the tie order inside the gradient loop."""
    for spp in EG.A_SAMPLES:
        got, st, X, _ = _ray(contexts, member, ("query",), mode, spp=spp)
        assert st["launches"] == 1
        if "/doubled/" in member:
            lose = EG.tie_losers(member, X)
            assert lose.size >= 10 and not got["color"][lose].any() and not got["emit"][lose].any()


@pytest.mark.parametrize("mode", EG.MODES)
def test_a_scene_no_ray_hits(contexts, mode):
    got, st, _, _ = _ray(contexts, EG.A_EMPTY, ("query",), mode, spp=3)
    assert st["terms"] == 0 and st["rays"] == st["paths"]
    for k in ("rgb", "color", "emit"):
        assert not np.ascontiguousarray(got[k]).view(np.uint8).any(), k  # +0 everywhere


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("mode", ["nee", "nee+mis"])
@pytest.mark.parametrize("member,kind", EG.STATE_CASES)
def test_crafted_states(contexts, member, kind, mode):
    """First light draws of exactly 1.0f, of 0 and 2^-32, on a cdf entry and one float below it."""
    _, st, _, _ = _ray(contexts, member, ("state", kind), mode)
    assert st["shadow_rays"] > 0


@pytest.mark.parametrize("exact_slab", [False, True], ids=["default", "exact_slab"])
@pytest.mark.parametrize("mode", EG.MODES)
@pytest.mark.parametrize("base", EG.BIG_BASES)
def test_big_directions(contexts, monkeypatch, base, mode, exact_slab):
    """Directions times 2^e, e in +-61 .. +-126: waves inside and outside the fast slab form's
    domain; once more with the exact slab walk forced inside the gradient loop."""
    if exact_slab:
        monkeypatch.setenv("PT_FORCE_EXACT_SLAB", "1")
    _ray(contexts, base, ("big",), mode, what=f"{base} {mode} exact_slab {exact_slab}")


@pytest.mark.parametrize("mode", EG.MODES)
def test_nonfinite_rays(contexts, mode):
    """Rays 60 .. 75 of 257 have inf and NaN components (both sides of a wave's end), 3 samples."""
    _ray(contexts, EG.NONFINITE_SCENE, ("nonfinite",), mode, spp=3)


# ---------------------------------------------------------------- C
@pytest.mark.parametrize("mode", EG.MODES)
@pytest.mark.parametrize("member", EG.C_MEMBERS)
def test_edge_members_along_camera_rays(contexts, monkeypatch, member, mode):
    _, st, _, _ = _render(contexts, member, EG.C_RES, mode, EG.C_SPP)
    assert st["launches"] == 1
    if member == EG.C_CHUNKED:
        monkeypatch.setenv("PT_RENDER_GRAD_CHUNK", "1")
        _, st, _, _ = _render(contexts, member, EG.C_RES, mode, EG.C_SPP, what=f"{member} {mode}: a launch per sample")
        assert st["launches"] == EG.C_SPP


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("which", ["E1", "E2"])
@pytest.mark.parametrize("mode", EG.MODES)
def test_edge_values_ray_forms(contexts, mode, which):
    """Zero, subnormal, negative, huge and (E2) non-finite materials and upstream gradients: zero
    terms are counted, every non-finite destination has the class its terms give, and a NaN in one
    row of the table leaves the other rows within their tolerance."""
    _, _, _, Z = _ray(contexts, EG.D_SCENE, ("set", EG.D_N), mode, spp=EG.D_SPP, seed=EG.D_SEED, grad=which, mats=which)
    EG.assert_floors(Z, EG.D_FLOORS, f"{mode} {which}")


@pytest.mark.parametrize("which", ["E1", "E2"])
@pytest.mark.parametrize("mode", EG.D_RENDER_MODES)
def test_edge_values_render(contexts, mode, which):
    _, _, _, Z = _render(contexts, EG.D_SCENE, EG.D_RES, mode, EG.D_SPP, grad=which, mats=which)
    EG.assert_floors(Z, EG.D_RENDER_FLOORS, f"render {mode} {which}")


@pytest.mark.parametrize("only", ["color", "emit"])
@pytest.mark.parametrize("mode", ["plain", "nee+mis"])
def test_one_override_alone(contexts, mode, only):
    """The gather kernel with a null pointer for the other override."""
    _ray(contexts, EG.D_SCENE, ("set", EG.D_N), mode, spp=EG.D_SPP, seed=EG.D_SEED, grad="E1", mats=("E1", only))
    _render(contexts, EG.D_SCENE, EG.D_RES, mode, EG.D_SPP, grad="E1", mats=("E1", only))


# ---------------------------------------------------------------- E
def _one_output(call, both_terms):
    counts = {}
    for want in EG.WANTS:
        counts[want] = call(want=want)[1]["terms"]  # the keys, the count of that kind and the values: assert_call
        assert 0 < counts[want] < both_terms
    assert counts[("emit",)] == counts[("rgb", "emit")] and counts[("emit",)] + counts[("color",)] == both_terms


def _same_arrays(part, whole, what):
    for k in part:
        assert np.array_equal(np.ascontiguousarray(part[k]).view(np.uint8), np.ascontiguousarray(whole[k]).view(np.uint8)), (what, k)


@pytest.mark.parametrize("mode", EG.MODES)
def test_one_output_alone_ray_forms(contexts, mode):
    """d emit alone (nee_grad_finish's own branch), d color alone, rgb with d emit: `terms` counts
    the requested kind only; n = 1, spp = 1 gives the bits of the call for both outputs."""
    kw = dict(spp=EG.D_SPP, seed=EG.D_SEED, grad="E1", mats="E1")
    rays = ("set", EG.D_N)
    both = _ray(contexts, EG.D_SCENE, rays, mode, **kw)[1]["terms"]
    _one_output(lambda want: _ray(contexts, EG.D_SCENE, rays, mode, want=want, **kw), both)
    for i in range(8):
        one = ("one", 8, i)
        whole = _ray(contexts, EG.D_SCENE, one, mode, seed=EG.D_SEED, mats="E1")[0]
        for want in EG.WANTS:
            _same_arrays(_ray(contexts, EG.D_SCENE, one, mode, seed=EG.D_SEED, mats="E1", want=want)[0], whole, (mode, i, want))


@pytest.mark.parametrize("mode", EG.MODES)
def test_one_output_alone_render(contexts, mode):
    kw = dict(grad="E1", mats="E1")
    both = _render(contexts, EG.D_SCENE, EG.D_RES, mode, EG.D_SPP, **kw)[1]["terms"]
    _one_output(lambda want: _render(contexts, EG.D_SCENE, EG.D_RES, mode, EG.D_SPP, want=want, **kw), both)
    whole = _render(contexts, EG.D_SCENE, (1, 1), mode, 1, mats="E1")[0]
    for want in EG.WANTS:
        _same_arrays(_render(contexts, EG.D_SCENE, (1, 1), mode, 1, mats="E1", want=want)[0], whole, (mode, want))


# ---------------------------------------------------------------- F
@pytest.mark.parametrize("grad_lds", [True, False], ids=["lds_table", "global_table"])
@pytest.mark.parametrize("hook,value,rule", PLACEMENTS)
@pytest.mark.parametrize("call,mode", EG.F_CALLS)
@pytest.mark.parametrize("name", EG.F_SCENES)
def test_every_placement(contexts, monkeypatch, name, call, mode, hook, value, rule, grad_lds):
    """Scene and stack in LDS or in global memory (where `mats` is the gathered override buffer) and
    the exact slab walk, each beside the LDS table and beside global atomics: the same rule, and
    the stats name the form that ran, by the placement rule of the binary walk (tests/_plans.py;
    the scene and the stack are placed before the records and the table)."""
    import ptamd
    _, bvh, _ = contexts(name)
    flags = ("lds_scene", "lds_stack")
    forced = _planned(ptamd.scene_info(bvh), EG.num_tris(name), EG.DEPTH, **rule)
    monkeypatch.setenv(hook, value)
    if not grad_lds:
        monkeypatch.setenv("PT_GRAD_LDS", "0")
    what = f"{name} {call} {mode} {hook}={value} PT_GRAD_LDS={int(grad_lds)}"
    if call == "render_grad":
        _, st, _, _ = _render(contexts, name, EG.C_RES, mode, EG.C_SPP, what=what, mats="overrides")
    else:
        _, st, _, _ = _ray(contexts, name, ("set", EG.F_N), mode, what=what, spp=EG.F_SPP, mats="overrides")
    assert {k: st[k] for k in flags} == {k: forced[k] for k in flags}, (what, st, forced)
    assert st["launches"] == 1
    if hook == "PT_LDS_SCENE_BYTES" and value == "0":
        assert st["lds_scene"] == 0
    if hook == "PT_QUERY_LDS_STACK":
        assert st["lds_stack"] == 0
    if not grad_lds:
        assert st["lds_table"] == 0
    elif name == "cornell+glow":  # 32 rows: the table fits beside everything
        assert st["lds_table"] == 1
