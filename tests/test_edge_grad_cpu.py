"""The gradient calls' host forms (BVH.trace_grad, BVH.trace_nee_grad, BVH.render_grad) on every
case of tests/_edgegrad.py against the restatements, under the rule of `_edgegrad.assert_call`, and
every non-vacuity condition of those cases on the restatement alone: tests/test_edge_grad_gpu.py
runs the same cases on the device and relies on both. No device is needed here."""
import numpy as np
import pytest

import _edgegrad as EG
import _edgelights as EL
import _refneegrad as NG


@pytest.fixture(scope="module")
def hosts():
    """One built BVH (and camera per resolution) per member."""
    import ptamd
    made = {}

    def get(member, res=EG.C_RES):
        key = (member, tuple(res))
        if key not in made:
            sc = EG.make_scene(member, res)
            bvh = ptamd.BVH.from_scene(sc)
            bvh.build()
            made[key] = (bvh, ptamd.Camera.from_spec(sc.camera))
        return made[key]

    return get


def _ray(hosts, member, rays, mode, what="", **kw):
    bvh, _ = hosts(member)
    X = EG.terms(member, rays, mode, **{k: v for k, v in kw.items() if k != "want"})
    got, st = EG.ray_call(bvh, member, rays, mode, **kw)
    Z = EG.assert_call(got, st, X, kw.get("want", EG.WANT_BOTH), what or f"{member} {rays} {mode} {kw}")
    assert st["paths"] == X.rgb.shape[0] * kw.get("spp", 1)
    return got, st, X, Z


def _render(hosts, member, res, mode, spp, what="", **kw):
    bvh, cam = hosts(member, res)
    rays = ("camera", tuple(res))
    X = EG.terms(member, rays, mode, spp, kw.pop("seed", EG.RENDER_SEED), **{k: v for k, v in kw.items() if k != "want"})
    got, st = EG.render_call(bvh, cam, member, res, mode, spp, **kw)
    Z = EG.assert_call(got, st, X, kw.get("want", EG.WANT_BOTH), what or f"{member} {res} {mode} {kw}", shape=(res[1], res[0]))
    assert st["paths"] == res[0] * res[1] * spp
    return got, st, X, Z


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("mode", EG.MODES)
@pytest.mark.parametrize("member", EG.A_MEMBERS)
def test_edge_members_along_caller_rays(hosts, member, mode):
    """Every listed member is kept. The floor of 30 non-zero channels holds in both tables except
    where `_edgegrad.PLAIN_COLOR_SHORT` names the plain estimator's d color on a Cornell member with
    its measured count (the floor is then half of it). scaled/51 is the family's one-leaf tree, and
    no neighbour with one leaf (2^51 and up) is hit by a query ray either: it has no term and no
    shadow segment, as scaled/100, and holds the forward value and the counts on that tree."""
    for spp in EG.A_SAMPLES:
        got, st, X, Z = _ray(hosts, member, ("query",), mode, spp=spp)
        channels = [EG.nonzero_channels(Z, k) for k in (EG.COLOR, EG.EMIT_K)]
        print(member, mode, "spp", spp, "terms", Z.S.terms, "non-zero channels (d color, d emit)", channels, "shadow", X.shadow)
        if not EG.sparse(member):
            assert EG.channel_floor(member, mode, spp, channels), (member, mode, spp, channels, EG.channel_floors(member, mode, spp))
            if mode == "plain" and (member, spp) in EG.PLAIN_COLOR_SHORT:  # the table's figure is the restatement's
                assert channels[EG.COLOR] == EG.PLAIN_COLOR_SHORT[member, spp] < EG.A_MIN_CHANNELS
        else:  # `sparse`: scaled/51 has no term at all; scaled/26 has terms, its paths end at their first bounce
            assert (Z.S.terms > 0) == ("/26" in member)
        if mode != "plain" and not EL.dim(member) and "/scaled/51" not in member:
            assert X.shadow > 0 and st["shadow_rays"] > 0
        if "/doubled/" in member:
            lose = EG.tie_losers(member, X)
            assert lose.size >= 10, (member, lose.size)
            assert not got["color"][lose].any() and not got["emit"][lose].any()


@pytest.mark.parametrize("mode", EG.MODES)
def test_a_scene_no_ray_hits(hosts, mode):
    got, st, X, Z = _ray(hosts, EG.A_EMPTY, ("query",), mode, spp=3)
    assert st["terms"] == 0 and Z.S.terms == 0 and st["rays"] == st["paths"]
    for k in ("rgb", "color", "emit"):
        assert not np.ascontiguousarray(got[k]).view(np.uint8).any(), k  # +0 everywhere


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("mode", ["nee", "nee+mis"])
@pytest.mark.parametrize("member,kind", EG.STATE_CASES)
def test_crafted_states(hosts, member, kind, mode):
    _, st, X, Z = _ray(hosts, member, ("state", kind), mode)
    c = EG.class_counts(Z)
    print(member, kind, mode, c)
    assert c["terms"] >= 500 and X.shadow > 0 and (X.case == NG.T_LIGHT).sum() > 0
    assert c["nan"] == c["pinf"] == c["ninf"] == 0


@pytest.mark.parametrize("mode", EG.MODES)
@pytest.mark.parametrize("base", EG.BIG_BASES)
def test_big_directions(hosts, base, mode):
    _, st, X, Z = _ray(hosts, base, ("big",), mode)
    c = EG.class_counts(Z)
    print(base, mode, c)
    assert c["terms"] >= 500 and c["nan"] == c["pinf"] == c["ninf"] == 0
    assert EG.channel_floor(base, mode, 1, [EG.nonzero_channels(Z, k) for k in (EG.COLOR, EG.EMIT_K)])


@pytest.mark.parametrize("mode", EG.MODES)
def test_nonfinite_rays(hosts, mode):
    """Sixteen rays with inf and NaN components among 257, three samples each: their paths' values
    are whatever the oracle's primitives make of them, and the finite rays' terms are untouched."""
    got, st, X, Z = _ray(hosts, EG.NONFINITE_SCENE, ("nonfinite",), mode, spp=3)
    at = np.arange(EG.NONFINITE_AT, EG.NONFINITE_AT + 16)
    from_bad = np.isin(X.t.path // 3, at)
    print(mode, EG.class_counts(Z), "terms of the non-finite rays", int(from_bad.sum()))
    assert Z.S.terms - from_bad.sum() >= 1000
    assert min(EG.nonzero_channels(Z, k) for k in (EG.COLOR, EG.EMIT_K)) >= EG.A_MIN_CHANNELS


# ---------------------------------------------------------------- C
@pytest.mark.parametrize("mode", EG.MODES)
@pytest.mark.parametrize("member", EG.C_MEMBERS)
def test_edge_members_along_camera_rays(hosts, member, mode):
    _, st, X, Z = _render(hosts, member, EG.C_RES, mode, EG.C_SPP)
    channels = [EG.nonzero_channels(Z, k) for k in (EG.COLOR, EG.EMIT_K)]
    print(member, mode, "terms", Z.S.terms, "non-zero channels", channels)
    assert Z.S.terms >= 500 and sum(channels) >= EG.C_MIN_CHANNELS  # (far_camera/61 plain: 0 + 33, all in d emit)


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("which", ["E1", "E2"])
@pytest.mark.parametrize("mode", EG.MODES)
def test_edge_values_ray_forms(hosts, mode, which):
    rays = ("set", EG.D_N)
    got, st, X, Z = _ray(hosts, EG.D_SCENE, rays, mode, spp=EG.D_SPP, seed=EG.D_SEED, grad=which, mats=which)
    bad_rgb = int((~np.isfinite(X.rgb)).any(axis=1).sum())
    print(mode, which, EG.class_counts(Z), "non-finite rgb rays", bad_rgb, "busy", EG.busy(EG.D_SCENE, rays, EG.D_SPP, EG.D_SEED, mode))
    EG.assert_floors(Z, EG.D_FLOORS, f"{mode} {which}")
    assert bad_rgb >= 40 if which == "E2" else bad_rgb <= 2  # E1: an overflow or two; E2: the NaN and inf rows reach the image
    # a NaN or an infinity in one row leaves the rows it does not reach alone
    assert ((Z.cls == EG.FINITE) & (Z.S.exact != 0)).any(axis=2).sum() >= 20


@pytest.mark.parametrize("which", ["E1", "E2"])
@pytest.mark.parametrize("mode", EG.D_RENDER_MODES)
def test_edge_values_render(hosts, mode, which):
    _, st, X, Z = _render(hosts, EG.D_SCENE, EG.D_RES, mode, EG.D_SPP, grad=which, mats=which)
    print(mode, which, EG.class_counts(Z))
    EG.assert_floors(Z, EG.D_RENDER_FLOORS, f"render {mode} {which}")


@pytest.mark.parametrize("only", ["color", "emit"])
@pytest.mark.parametrize("mode", ["plain", "nee+mis"])
def test_one_override_alone(hosts, mode, only):
    _, _, _, Z = _ray(hosts, EG.D_SCENE, ("set", EG.D_N), mode, spp=EG.D_SPP, seed=EG.D_SEED, grad="E1", mats=("E1", only))
    assert EG.class_counts(Z)["finite_nonzero"] >= EG.D_FLOORS["finite_nonzero"]
    _render(hosts, EG.D_SCENE, EG.D_RES, mode, EG.D_SPP, grad="E1", mats=("E1", only))


# ---------------------------------------------------------------- E
def _one_output(call, both_terms):
    """want = d emit alone, d color alone, rgb and d emit: only those keys (`assert_call`), `terms`
    the count of that kind, and the counts of the two kinds sum to the both-outputs count."""
    counts = {}
    for want in EG.WANTS:
        _, st, _, Z = call(want=want)
        counts[want] = st["terms"]
        assert 0 < st["terms"] < both_terms
    assert counts[("emit",)] == counts[("rgb", "emit")] and counts[("emit",)] + counts[("color",)] == both_terms
    return counts


@pytest.mark.parametrize("mode", EG.MODES)
def test_one_output_alone_ray_forms(hosts, mode):
    kw = dict(spp=EG.D_SPP, seed=EG.D_SEED, grad="E1", mats="E1")
    rays = ("set", EG.D_N)
    both = _ray(hosts, EG.D_SCENE, rays, mode, **kw)[1]["terms"]
    print(mode, _one_output(lambda want: _ray(hosts, EG.D_SCENE, rays, mode, want=want, **kw), both), both)
    _single_path(lambda member, rays, **k: _ray(hosts, member, rays, mode, **k), mode)


@pytest.mark.parametrize("mode", EG.MODES)
def test_one_output_alone_render(hosts, mode):
    kw = dict(grad="E1", mats="E1")
    both = _render(hosts, EG.D_SCENE, EG.D_RES, mode, EG.D_SPP, **kw)[1]["terms"]
    print(mode, _one_output(lambda want: _render(hosts, EG.D_SCENE, EG.D_RES, mode, EG.D_SPP, want=want, **kw), both), both)
    whole, _, X, _ = _render(hosts, EG.D_SCENE, (1, 1), mode, 1, mats="E1")
    # the one path has terms (2 plain; 4 with lights, 2 of them a visible light's pair)
    assert len(X.t.kind) >= 2 and (mode == "plain" or (X.case == NG.T_LIGHT).sum() >= 1)
    for want in EG.WANTS:
        part = _render(hosts, EG.D_SCENE, (1, 1), mode, 1, mats="E1", want=want)[0]
        for k in part:
            assert np.array_equal(part[k].view(np.uint8), whole[k].view(np.uint8)), (mode, want, k)


def _single_path(call, mode, n=8):
    """n = 1, spp = 1: the sums are added in k order, so one output alone is bit for bit the same
    array of the call for both. Of the 8 single rays 5 have terms (6-15 each; rays 0, 1 and 7 have
    none), and with lights rays 3, 4 and 5 have a visible light's pair of terms (6 each)."""
    with_terms = lit = 0
    for i in range(n):
        whole, _, X, _ = call(EG.D_SCENE, ("one", n, i), seed=EG.D_SEED, mats="E1")
        with_terms += len(X.t.kind) >= 6
        lit += mode != "plain" and bool((X.case == NG.T_LIGHT).sum() >= 2)
        for want in EG.WANTS:
            part = call(EG.D_SCENE, ("one", n, i), seed=EG.D_SEED, mats="E1", want=want)[0]
            for k in part:
                assert np.array_equal(part[k].view(np.uint8), whole[k].view(np.uint8)), (i, want, k)
    assert with_terms >= 4 and (mode == "plain" or lit >= 2), (mode, with_terms, lit)


# ---------------------------------------------------------------- F
@pytest.mark.parametrize("call,mode", EG.F_CALLS)
@pytest.mark.parametrize("name", EG.F_SCENES)
def test_placement_cases_on_the_host(hosts, name, call, mode):
    """The calls of the placement runs (the hooks reach the device only): `_refgrad.overrides`."""
    if call == "render_grad":
        _, _, _, Z = _render(hosts, name, EG.C_RES, mode, EG.C_SPP, mats="overrides")
    else:
        _, _, _, Z = _ray(hosts, name, ("set", EG.F_N), mode, spp=EG.F_SPP, mats="overrides")
    assert Z.S.terms >= 500 and min(EG.nonzero_channels(Z, k) for k in (EG.COLOR, EG.EMIT_K)) >= EG.A_MIN_CHANNELS
    assert (Z.cls == EG.FINITE).all()
