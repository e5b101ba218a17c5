"""The last-ray rule: in a dark scene a path whose LAST ray provably fails
the slab test of every leaf box that holds an emitter ends at +0 without tracing that ray.

CPU: the predicate (emit_reject, pt_math.h) against a float32 restatement of the reference's
AABB::intersect_inv on random and adversarial inputs, with no input skipped; the emitter box
the host computes; the generated scene-kernel source. GPU: float32 bits AND ray counts against
the oracle on every kernel path with the rule on and off, and the count of paths ended early
(test hook pt_debug_ctx_emit_reject; the offline kernels count it, the hipRTC scene kernel
under PT_RTC_DEFINES=PT_COUNT_EARLY=1)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import _oracle as O
import _trees as T

F32 = np.float32
INF = F32(np.inf)


@pytest.fixture(scope="module")
def pt():
    import ptamd
    return ptamd


# ---------------------------------------------------------------- the predicate (CPU)
def _reject(pt, box, o, d):
    box, o, d = (np.ascontiguousarray(a, dtype=F32) for a in (box, o, d))
    n = o.shape[0]
    out = np.zeros(n, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert pt.lib().pt_debug_emit_reject(p(box), p(o), p(d), n, p(out)) == 0
    return out.astype(bool)


def _intersect_inv(lb, rt, o, inv):
    """aabb.h:20-29 in float32: std::max(a, b) = (a < b) ? b : a, std::min(a, b) = (b < a) ? b : a,
    and the initializer-list forms as left folds with `<` (min_element / max_element)."""
    with np.errstate(all="ignore"):
        t1, t2 = ((lb - o) * inv).astype(F32), ((rt - o) * inv).astype(F32)
        hi = np.where(t1 < t2, t2, t1)
        lo = np.where(t2 < t1, t2, t1)
        tmax = hi[:, 0]
        tmax = np.where(hi[:, 1] < tmax, hi[:, 1], tmax)
        tmax = np.where(hi[:, 2] < tmax, hi[:, 2], tmax)
        tmin = lo[:, 0]
        tmin = np.where(tmin < lo[:, 1], lo[:, 1], tmin)
        tmin = np.where(tmin < lo[:, 2], lo[:, 2], tmin)
        return ~(tmax < 0) & (tmin <= tmax)


def _slab_hit_finite(lb, rt, o, inv):
    """slab_hit_finite (pt_math.h): IEEE min / max, max(tmin, 0) <= tmax."""
    with np.errstate(all="ignore"):
        t1, t2 = ((lb - o) * inv).astype(F32), ((rt - o) * inv).astype(F32)
        tmax = np.fmin(np.fmin(np.fmax(t1, t2)[:, 0], np.fmax(t1, t2)[:, 1]), np.fmax(t1, t2)[:, 2])
        tmin = np.fmax(np.fmax(np.fmin(t1, t2)[:, 0], np.fmin(t1, t2)[:, 1]), np.fmin(t1, t2)[:, 2])
        return np.fmax(tmin, F32(0)) <= tmax


def _check_implication(pt, elb, ert, lb, rt, o, d):
    """reject => not intersect_inv, for every row; returns the rejected mask."""
    assert np.all(elb <= lb) and np.all(lb <= rt) and np.all(rt <= ert)  # the inputs are boxes inside E
    with np.errstate(all="ignore"):
        inv = (F32(1) / d).astype(F32)
    rej = _reject(pt, np.concatenate([elb, ert], axis=1), o, d)
    hit = _intersect_inv(lb, rt, o, inv)
    bad = np.flatnonzero(rej & hit)
    assert bad.size == 0, (bad[:5], elb[bad[:5]], ert[bad[:5]], lb[bad[:5]], rt[bad[:5]], o[bad[:5]], d[bad[:5]])
    fin = np.isfinite(inv).all(axis=1) & ~np.isnan(o).any(axis=1)
    bad = np.flatnonzero(rej & fin & _slab_hit_finite(lb, rt, o, inv))
    assert bad.size == 0, bad[:5]
    return rej


def test_predicate_implies_slab_miss_random(pt):
    """10^6 seeded (box inside E, o, d): origins outside E on one axis at least, directions uniform
    in the cube. Not vacuous: between 40 % and 90 % are rejected."""
    n = 1_000_000
    g = np.random.default_rng(20261019)
    elb = g.uniform(-100, 100, (n, 3)).astype(F32)
    ert = (elb + g.uniform(0, 100, (n, 3)).astype(F32)).astype(F32)
    lb = np.clip((elb + g.uniform(0, 1, (n, 3)).astype(F32) * (ert - elb)).astype(F32), elb, ert)
    rt = np.clip((lb + g.uniform(0, 1, (n, 3)).astype(F32) * (ert - lb)).astype(F32), lb, ert)
    o = g.uniform(-250, 250, (n, 3)).astype(F32)
    ax, side = g.integers(0, 3, n), g.integers(0, 2, n)
    r = np.arange(n)
    dist = g.uniform(1e-3, 200, n).astype(F32)
    o[r, ax] = np.where(side == 0, elb[r, ax] - dist, ert[r, ax] + dist).astype(F32)
    d = g.uniform(-1, 1, (n, 3)).astype(F32)
    rej = _check_implication(pt, elb, ert, lb, rt, o, d)
    share = rej.mean()
    print(f"rejected share of the random set: {share:.4f}")
    assert 0.40 <= share <= 0.90


def _axis_cases():
    """One axis: (elb, ert, lb, rt, o, d) over E planes up to 2^60 (a one-point E and flat boxes
    included), o on a face and one ulp to either side, d over zeros, subnormals, 1, 2 and its
    neighbours, inf and NaN."""
    planes = [F32(x) for x in (0.0, 1.0, -1.0, 3.5, 2.0 ** 60, -(2.0 ** 60), 1e-40, -1e-40, 548.7)]
    two = F32(2)
    ds = []
    for v in (F32(0), F32(1e-45), F32(1e-39), F32(1), np.nextafter(two, F32(0)), two, np.nextafter(two, INF), INF):
        ds += [v, -v]
    ds.append(F32(np.nan))
    rows = []
    for a in planes:
        for b in planes:
            if not a <= b:
                continue
            mid = F32((np.float64(a) + np.float64(b)) / 2)
            for lb, rt in ((a, b), (a, a), (b, b), (mid, mid), (a, mid), (mid, b)):
                os_ = {a, b, np.nextafter(a, -INF), np.nextafter(a, INF), np.nextafter(b, -INF), np.nextafter(b, INF),
                       F32(0), F32(2.0 ** 60), F32(-(2.0 ** 60)), mid, INF, -INF}
                for o in os_:
                    for d in ds:
                        rows.append((a, b, lb, rt, o, d))
    return np.array(rows, dtype=F32)


def test_predicate_implies_slab_miss_adversarial(pt):
    """The adversarial grid on each axis in turn, the other two axes running through the same
    cases out of step (so a NaN or an infinity on an earlier axis meets a rejection on a later
    one), then 10^6 random triples of axis cases. Every row is checked."""
    A = _axis_cases()
    n = A.shape[0]
    assert n > 30_000
    total = 0
    for ax in range(3):
        cols = [np.roll(A, 7919 * ((k - ax) % 3), axis=0) for k in range(3)]
        stack = np.stack(cols, axis=1)  # (n, axis, field)
        f = [np.ascontiguousarray(stack[:, :, j]) for j in range(6)]
        total += _check_implication(pt, *f).sum()
    g = np.random.default_rng(7)
    pick = g.integers(0, n, (1_000_000, 3))
    stack = np.stack([A[pick[:, k]] for k in range(3)], axis=1)
    f = [np.ascontiguousarray(stack[:, :, j]) for j in range(6)]
    total += _check_implication(pt, *f).sum()
    assert total > 0
    # NaN anywhere in o or d on the deciding axis: not rejected by that axis; an all-NaN ray never
    nan3 = np.full((4, 3), np.nan, dtype=F32)
    one = np.ones((4, 3), dtype=F32)
    assert not _reject(pt, np.concatenate([one, one], axis=1), nan3, -one).any()
    assert not _reject(pt, np.concatenate([one, one], axis=1), -one, nan3).any()
    # the empty box (no emitter): any finite direction with a non-zero component is rejected
    empty = np.tile(np.array([np.inf] * 3 + [-np.inf] * 3, dtype=F32), (3, 1))
    d = np.array([[0, 0, 1], [-1e-45, 0, 0], [0, 0, 0]], dtype=F32)
    assert _reject(pt, empty, np.zeros((3, 3), dtype=F32), d).tolist() == [True, True, False]


# ---------------------------------------------------------------- the host's emitter box (CPU)
def _scene(kind: str, res=(36, 30)):
    from ptamd import scenes
    S = scenes
    if kind == "cornell":
        return S.cornell(res)
    if kind.startswith("mcornell_r"):
        return S.modified_cornell(float(kind[len("mcornell_r"):]), res)
    sc = S.cornell(res)
    white = S.Material.make(S.DIFFUSE, 1, 0, 0)
    if kind == "no_emitter":  # the light made DIFFUSE
        for i, m in enumerate(sc.mats):
            if m.type == S.EMIT:
                sc.mats[i] = white
    elif kind == "back_wall_emits":  # E spans the room
        sc.mats[6] = sc.mats[7] = S.Material.make(S.EMIT, 0, (0.5, 0.25, 1.0))
    elif kind == "two_lights":  # a second light in a far corner
        sc.add([((5.0, 5.0, 550.0), (40.0, 5.0, 550.0), (5.0, 40.0, 555.0))], S.Material.make(S.EMIT, 0, (3.0, 2.0, 1.0)))
    elif kind == "diffuse_emits":
        sc.mats[0] = S.Material(S.DIFFUSE, sc.mats[0].color, (0.25, 0.0, 0.0), 0.0)
    elif kind == "diffuse_emits_minus0":
        sc.mats[0] = S.Material(S.DIFFUSE, sc.mats[0].color, (-0.0, 0.0, 0.0), 0.0)
    elif kind == "albedo_inf":
        sc.mats[0] = S.Material(S.DIFFUSE, (float("inf"), 0.5, 0.5), sc.mats[0].emit, 0.0)
    else:
        raise KeyError(kind)
    return sc


def _bvh(pt, sc, merged: int = 0):
    """BVH::build's tree, or with merged > 0 the caller-built tree _trees.merged makes of it."""
    b = pt.BVH.from_scene(sc)
    b.build()
    if merged:
        nodes, idx = T.merged(b.nodes, b.tri_idx, merged)
        b.nodes, b.tri_idx = nodes, idx
    return b


def _emit_box(pt, bvh):
    ref = pt._SceneRef(bvh)
    out = (C.c_float * 6)()
    on = pt.lib().pt_debug_emit_box(C.byref(ref.s), out)
    assert on >= 0, pt.lib().pt_last_error()
    return bool(on), np.array(list(out), dtype=F32)


def _expected_box(sc, nodes, idx):
    """The union of the reachable leaf boxes that hold an EMIT triangle, restated."""
    from ptamd import scenes
    lo, hi = np.full(3, np.inf, dtype=F32), np.full(3, -np.inf, dtype=F32)
    st = [0]
    while st:
        n = st.pop()
        if T.is_leaf(nodes, n):
            tris = [int(idx[i]) for i in range(int(nodes["tri_start"][n]), int(nodes["tri_end"][n]) + 1)]
            if any(sc.mats[t].type == scenes.EMIT for t in tris):
                lo, hi = np.minimum(lo, nodes["lb"][n]), np.maximum(hi, nodes["rt"][n])
        else:
            st += [int(nodes["left"][n]), int(nodes["right"][n])]
    return np.concatenate([lo, hi]).astype(F32)


def test_emit_box_of_scenes(pt):
    light = np.array([213, 548.7, 227, 343, 548.7, 332], dtype=F32)
    for kind in ("cornell", "mcornell_r0.8"):
        b = _bvh(pt, _scene(kind))
        on, box = _emit_box(pt, b)
        assert on and box.tobytes() == light.tobytes(), (kind, box)
    sc = _scene("two_lights")
    b = _bvh(pt, sc)
    on, box = _emit_box(pt, b)
    want = np.array([5, 5, 227, 343, 548.7, 555], dtype=F32)
    assert on and box.tobytes() == want.tobytes() == _expected_box(sc, b.nodes, b.tri_idx).tobytes()
    on, box = _emit_box(pt, _bvh(pt, _scene("no_emitter")))
    assert on and box.tolist() == [np.inf] * 3 + [-np.inf] * 3  # the "reject all" encoding
    sc = _scene("back_wall_emits")
    b = _bvh(pt, sc)
    on, box = _emit_box(pt, b)
    assert on and box.tobytes() == _expected_box(sc, b.nodes, b.tri_idx).tobytes()
    assert box[0] == 0 and box[3] == 556 and box[1] == 0 and box[4] == F32(548.8)


def test_emit_box_is_the_trees_leaf_box(pt):
    """A caller-built tree (_trees.merged) whose emitter leaf also holds diffuse triangles and is
    larger than the emitters: the box is the tree's leaf box, not the triangles' AABB."""
    from ptamd import scenes
    sc = _scene("cornell")
    b = _bvh(pt, sc, merged=5)
    on, box = _emit_box(pt, b)
    want = _expected_box(sc, b.nodes, b.tri_idx)
    assert on and box.tobytes() == want.tobytes()
    light = np.array([213, 548.7, 227, 343, 548.7, 332], dtype=F32)
    assert np.all(box[:3] <= light[:3]) and np.all(box[3:] >= light[3:]) and box.tobytes() != light.tobytes()
    shared = False
    for n in range(len(b.nodes)):
        if T.is_leaf(b.nodes, n) and b.nodes["tri_start"][n] < b.nodes["tri_end"][n]:
            types = {sc.mats[int(b.tri_idx[i])].type for i in range(int(b.nodes["tri_start"][n]), int(b.nodes["tri_end"][n]) + 1)}
            shared |= scenes.EMIT in types and len(types) > 1
    assert shared  # the case is the one it is meant to be


@pytest.mark.parametrize("kind", ["diffuse_emits", "diffuse_emits_minus0", "albedo_inf", "mcornell_r2.0"])
def test_rule_off_in_scenes_that_are_not_dark(pt, kind):
    on, box = _emit_box(pt, _bvh(pt, _scene(kind)))
    assert not on and not box.any()


def test_rule_off_by_hook(pt, monkeypatch):
    monkeypatch.setenv("PT_EMIT_REJECT", "0")
    on, _ = _emit_box(pt, _bvh(pt, _scene("cornell")))
    assert not on


def _rtc_source(pt, bvh):
    ref = pt._SceneRef(bvh)
    buf = C.create_string_buffer(400000)
    assert pt.lib().pt_rtc_check(C.byref(ref.s), buf, len(buf)) > 1000, pt.lib().pt_last_error()
    return buf.value.decode()


def test_generated_source_holds_the_box_only_when_on(pt, monkeypatch):
    b = _bvh(pt, _scene("cornell"))
    on_src = _rtc_source(pt, b)
    m = re.search(r"emit_reject\(v3\{([^}]*)\}, v3\{([^}]*)\}, o, d\)", on_src)
    assert m and "struct EmitRej" in on_src
    lits = [float.fromhex(x.strip().rstrip("f")) for x in (m.group(1) + "," + m.group(2)).split(",")]
    assert np.array(lits, dtype=F32).tobytes() == np.array([213, 548.7, 227, 343, 548.7, 332], dtype=F32).tobytes()
    monkeypatch.setenv("PT_EMIT_REJECT", "0")
    off_src = _rtc_source(pt, b)
    assert "emit_reject(" not in off_src and "struct EmitRej" not in off_src
    # apart from that member the two sources are the same bytes
    block = on_src[on_src.index("    struct EmitRej {"):on_src.index("    __device__ __forceinline__ static unsigned long long mask(")]
    assert on_src.replace(block, "    using EmitRej = NoEmitReject;\n") == off_src
    # no emitter: infinities spelled so that they compile (pt_rtc_check compiled it)
    monkeypatch.delenv("PT_EMIT_REJECT")
    src = _rtc_source(pt, _bvh(pt, _scene("no_emitter")))
    assert "emit_reject(v3{__builtin_inff(), __builtin_inff(), __builtin_inff()}, v3{-__builtin_inff()," in src
    # not dark: no rule
    assert "emit_reject(" not in _rtc_source(pt, _bvh(pt, _scene("diffuse_emits")))


# ---------------------------------------------------------------- renders (GPU)
TREE_WALK = {"PT_FLAT": "0", "PT_WIDE": "0"}
COUNT_RTC = {"PT_RTC_DEFINES": "PT_COUNT_EARLY=1"}
# hooks -> the kernel path(s) a BVH::build tree of a dark flat scene takes
PATHS = {"rtc": (dict(COUNT_RTC), (3,)), "table_fast": ({"PT_RTC": "0"}, (5,)),
         "table": ({"PT_RTC": "0", "PT_FLAT_FAST": "0"}, (2,)), "wide": ({"PT_WIDE": "1"}, (4,)),
         "tree": (TREE_WALK, (0, 1))}


@pytest.fixture(scope="module")
def gpu(pt):
    if pt.lib().pt_device_count() <= 0:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    return pt


@functools.lru_cache(maxsize=None)
def _oracle(kind, res, spp, depth, merged=0):
    """(image, rays, rays of the same frame one level shallower), made once per process."""
    import ptamd
    sc = _scene(kind, res)
    kw = {}
    if merged:
        b = _bvh(ptamd, sc, merged)
        kw = dict(nodes=np.ascontiguousarray(b.nodes), idx=np.ascontiguousarray(b.tri_idx))
    img, rays = O.render(sc, spp, depth, **kw)
    shallower = O.render(sc, spp, depth - 1, **kw)[1] if depth > 1 else 0
    img.setflags(write=False)
    return img, rays, shallower


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(gpu, monkeypatch, kind, env, want_paths, rule, depth, res=(36, 30), spp=5, merged=0, expect_on=True):
    """One render under `env` with the rule on or off (PT_EMIT_REJECT=0): bits and rays against the
    oracle, the kernel path, flags(), and the early-end count's bounds. Returns that count."""
    sc = _scene(kind, res)
    ref, rays, shallower = _oracle(kind, tuple(res), spp, depth, merged)
    with monkeypatch.context() as mp:
        mp.setenv("PT_RTC_WAIT", "1")
        for k, v in env.items():
            mp.setenv(k, v)
        if not rule:
            mp.setenv("PT_EMIT_REJECT", "0")
        r = gpu.Renderer(0)
        try:
            r.set_scene(_bvh(gpu, sc, merged))
            flags = r.flags()
            img, st = r.render(gpu.Camera.from_spec(sc.camera), spp, depth)
            early = r.early_ends()
        finally:
            r.close()
    tag = (kind, env, rule, depth)
    print(f"{tag}: kernel_path {st['kernel_path']}, rays {st['rays']} (oracle {rays}), early ends {early}, "
          f"last segments {rays - shallower}")
    assert st["kernel_path"] in want_paths, tag
    assert flags["emit_reject"] == (rule and expect_on), tag
    same = _bits(img) == _bits(ref)
    if not expect_on:  # a scene that is not dark may hold NaN, whose payload is not part of the contract
        same |= np.isnan(img) & np.isnan(ref)
    assert same.all(), tag
    assert st["rays"] == rays, tag
    if not (rule and expect_on) or depth < 2:
        assert early == 0, tag  # depth 1 has no bounce: nothing to end
    else:
        # an early end replaces one last segment of the frame: at most as many as the oracle traced
        assert 0 < early <= rays - shallower <= st["paths"], tag
    return early


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [True, False])
@pytest.mark.parametrize("path", list(PATHS))
def test_cornell_depths_on_every_path(gpu, monkeypatch, path, rule):
    """Cornell at depth 1, 2, 3, 5 and 8 (8: the per-level record loop of the unwinding)."""
    env, want = PATHS[path]
    for depth in (1, 2, 3, 5, 8):
        _run(gpu, monkeypatch, "cornell", env, want, rule, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [True, False])
@pytest.mark.parametrize("path", list(PATHS))
def test_specular_room_on_every_path(gpu, monkeypatch, path, rule):
    """Modified Cornell r = 0.8: dark, the specular sampler's directions."""
    env, want = PATHS[path]
    for depth in (2, 5):
        _run(gpu, monkeypatch, "mcornell_r0.8", env, want, rule, depth)


@pytest.mark.gpu
def test_specular_room_that_is_not_dark_has_no_rule(gpu, monkeypatch):
    for path in ("rtc", "wide"):
        env, want = PATHS[path]
        want = (3,) if path == "rtc" else want
        _run(gpu, monkeypatch, "mcornell_r2.0", env, want, True, 5, expect_on=False)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_no_emitter_every_last_ray_ends_early(gpu, monkeypatch, path):
    """The light made DIFFUSE: the image is +0, the rays are the oracle's, and every path that
    reaches its second-to-last bounce ends there: exactly the last segments the oracle traced
    (its ray count at this depth minus the same frame's one level shallower)."""
    env, want = PATHS[path]
    for depth in (2, 5):
        early = _run(gpu, monkeypatch, "no_emitter", env, want, True, depth)
        ref, rays, shallower = _oracle("no_emitter", (36, 30), 5, depth)
        assert not _bits(ref).any()
        assert early == rays - shallower, (path, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["back_wall_emits", "two_lights"])
def test_large_emitter_boxes(gpu, monkeypatch, kind):
    """An emitter that fills the room (almost nothing is rejected) and a second light in a far
    corner (a large union box)."""
    for path in ("rtc", "table", "wide", "tree"):
        env, want = PATHS[path]
        _run(gpu, monkeypatch, kind, env, want, True, 5)
    _run(gpu, monkeypatch, kind, PATHS["rtc"][0], (3,), False, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [True, False])
def test_merged_leaves_with_an_emitter_among_diffuse_triangles(gpu, monkeypatch, rule):
    """_trees.merged(5): the emitter's leaf holds diffuse triangles too and its box is larger than
    the light; generic table kernel (2) and wide walk (4), plus the scene kernel and tree walk."""
    for path, want in (("table", (2,)), ("wide", (4,)), ("rtc", (3,)), ("tree", (0, 1))):
        _run(gpu, monkeypatch, "cornell", PATHS[path][0], want, rule, 5, merged=5)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["rtc", "table_fast", "wide", "tree"])
def test_mixed_depth_waves(gpu, monkeypatch, path):
    """One 64 x 1 frame at 70 spp, depth 3: rejected and surviving lanes meet in one wave."""
    env, want = PATHS[path]
    for rule in (True, False):
        _run(gpu, monkeypatch, "cornell", env, want, rule, 3, res=(64, 1), spp=70)


@pytest.mark.gpu
@pytest.mark.parametrize("hook", [{"PT_PAIR_QUEUE": "16"}, {"PT_PAIRS": "0"}, {"PT_FORCE_EXACT_SLAB": "2"}])
def test_flat_kernel_variants(gpu, monkeypatch, hook):
    """A 16-entry pair queue (overflows fall back to the lane loops), no pair queue, and waves on
    the exact walk next to waves on the fast path."""
    for path in ("rtc", "table_fast", "table") + (("wide", "tree") if "PT_FORCE_EXACT_SLAB" in hook else ()):
        env, want = PATHS[path]
        for kind in ("cornell", "mcornell_r0.8"):
            _run(gpu, monkeypatch, kind, {**env, **hook}, want, True, 5)
