"""One domain verdict per ray (PT_DOMAIN_ONCE) on the GPU.

Device functions: rcp3_exact_v's wave-level verdict and the slab rule without the inv half of its
guard (pt_debug_domain_once, one block) against the three predicates they replace, on crafted
rays arranged so that whole waves are inside the domain, whole waves outside, and most mixed.
Kernels: the scene kernel with the policy on, compiled out (PT_RTC_DEFINES=PT_DOMAIN_ONCE=0) and
with the exact walk forced in the odd waves, bit for bit and ray for ray against the oracle."""
import numpy as np
import pytest

import _edgescenes as ES
import test_domain_once_cpu as DC
from test_domain_once_cpu import F32, crafted  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
PATH_RTC = 3  # PT_PATH_FLAT_RTC


@pytest.fixture(scope="module")
def pt():
    import ptamd
    if ptamd.lib().pt_device_count() <= 0:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    return DC.bind(ptamd)


def _unit_rows(n, seed):
    """Unit vectors with every |component| in [2^-10, 1]: inside the domain of both forms."""
    g = np.random.default_rng(seed)
    v = g.uniform(0.05, 1.0, (n, 3)) * g.choice([-1.0, 1.0], (n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


@pytest.mark.parametrize("unit", [False, True])
def test_device_functions_against_the_predicates_they_replace(pt, crafted, unit):  # noqa: F811
    """Rounds of 256 rays, one wave per 64: [clean wave | the crafted rows, mixed with clean ones |
    ... | clean wave]. Wherever the verdict says "in the domain" the three old predicates hold; a
    wave of clean rays gets that verdict; the per-lane results (predicates, reciprocal bits, both
    forms of the slab rule) are the host's; and the guard-free slab rule equals the guarded one."""
    d, o = crafted
    if unit:
        keep = DC._unit_pre(d)
        d, o = d[keep], o[keep]
    clean = _unit_rows(1024, 7)
    co = np.tile(np.array([[278, 273, 300], [100, 600, 100]], dtype=F32), (512, 1))
    half = _unit_rows(d.shape[0], 8)  # the crafted rows interleaved with clean ones: mixed waves
    mix_d = np.stack([d, half], axis=1).reshape(-1, 3)
    mix_o = np.stack([o, o], axis=1).reshape(-1, 3)
    dd = np.concatenate([clean[:256], mix_d, np.repeat(clean[:1], (-mix_d.shape[0]) % 64, axis=0), clean[256:]])
    oo = np.concatenate([co[:256], mix_o, np.repeat(co[:1], (-mix_o.shape[0]) % 64, axis=0), co[256:]])
    n = dd.shape[0]
    assert n % 64 == 0 and 1000 < n < 8192
    dev, dinv = DC._probe(pt, oo, dd, unit, device=0)
    host, hinv = DC._probe(pt, oo, dd, unit)
    fast = dev[:, 3]
    assert dev[fast][:, :3].all()
    assert np.array_equal(dev[:, 4], dev[:, 5]) and dev[:, 4].any()
    assert np.array_equal(dev[:, [0, 1, 2, 4, 5]], host[:, [0, 1, 2, 4, 5]])
    nan = np.isnan(hinv)
    assert np.array_equal(np.isnan(dinv), nan) and np.array_equal(dinv[~nan].view(np.uint32), hinv[~nan].view(np.uint32))
    # the verdict is the wave's: "in" exactly where every ray of the wave is in by the host's per-ray verdict
    waves = host[:, 3].reshape(-1, 64).all(axis=1)
    assert np.array_equal(fast, np.repeat(waves, 64))
    assert waves[:4].all() and waves[-12:].all() and 0 < (~waves).sum()


# ---------------------------------------------------------------- renders
def _scene(name, res):
    from ptamd import scenes
    if name == "cornell":
        return scenes.cornell(res)
    if name == "mcornell":
        return scenes.modified_cornell(0.3, res)
    if name == "axis":  # tests/test_gpu_parity.py: tiny x / y components, huge inverse directions
        base = scenes.cornell(res)
        cam = scenes.CameraSpec((278.0, 274.4, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), res, 1e-3, 1.0)
        return scenes.Scene("axis", cam, list(base.tris), list(base.mats))
    if name == "axis_tiny":
        # the same camera through a field of view of 5.4e-36 degrees: the view plane is 2^-123 wide and a
        # cell 2^-126, so cx = (px + jx) cell - 2^-124 lies in [-2^-124, 2^-124] and is below 2^-126 in
        # magnitude (subnormal, or 0) for the two middle columns of eight, cy for the two middle rows:
        # 7 / 16 of the camera rays leave the reciprocal's domain (their inv overflows), the others and
        # every bounce ray are inside it
        base = scenes.cornell(res)
        cam = scenes.CameraSpec((278.0, 274.4, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), res, 5.4e-36, 1.0)
        return scenes.Scene("axis_tiny", cam, list(base.tris), list(base.mats))
    return ES.make(name, res)


# (scene, resolution, spp, depth). A launch's grid is min(items / 256, 8 blocks per CU), so the small
# frames give every wave one fill of its 64-slot stock. BIG is the case with refills: 2^21 items are
# 256 per wave on 256 CUs (215 on 304), so every wave's stock is filled, drained and filled again
# three times, with marked and unmarked rows in every fill; depth 3 keeps the oracle at two seconds.
BIG = ("axis_tiny", (8, 8), 32768, 3)
MARKED = (("axis_tiny", (8, 8), 48, 5), BIG)  # cases whose camera rays carry the mark
CASES = [("cornell", (16, 16), 4, 1), ("cornell", (16, 16), 4, 2), ("cornell", (16, 16), 4, 5),
         ("mcornell", (16, 16), 4, 5), ("axis", (8, 8), 48, 5), ("cornell/far_camera/61", (8, 8), 48, 5),
         ("cornell/far_camera/66", (8, 8), 48, 5), ("cornell", (16, 16), 4, 0), ("cornell", (6, 5), 2, 5), *MARKED]
# "count*": the kernel with PT_COUNT_DOM, whose counter (early_ends) takes the lane-segments that
# traced a marked ray, so the test knows from the run that the marked branch was taken
HOOKS = {"on": {}, "off": {"PT_RTC_DEFINES": "PT_DOMAIN_ONCE=0"}, "exact_odd_waves": {"PT_FORCE_EXACT_SLAB": "2"},
         "start_branch_inv": {"PT_RTC_DEFINES": "PT_CAM_INV=1"}, "count": {"PT_RTC_DEFINES": "PT_COUNT_DOM=1"},
         "count_start_branch_inv": {"PT_RTC_DEFINES": "PT_COUNT_DOM=1,PT_CAM_INV=1"},
         "count_exact_odd_waves": {"PT_RTC_DEFINES": "PT_COUNT_DOM=1", "PT_FORCE_EXACT_SLAB": "2"}}


@pytest.fixture(scope="module")
def refs():
    """The oracle's image and ray count of every case, computed once."""
    import _oracle as O
    out = {}
    for name, res, spp, depth in CASES:
        img, rays = O.render(_scene(name, res), spp, depth)
        img.setflags(write=False)
        out[(name, res, spp, depth)] = (img, rays)
    return out


@pytest.mark.parametrize("hook", list(HOOKS))
def test_scene_kernel_bits_and_rays(pt, refs, monkeypatch, hook):
    for case in CASES:
        name, res, spp, depth = case
        sc = _scene(name, res)
        with monkeypatch.context() as mp:
            mp.setenv("PT_RTC_WAIT", "1")
            for k, v in HOOKS[hook].items():
                mp.setenv(k, v)
            r = pt.Renderer(0)
            try:
                r.set_scene(pt.BVH.from_scene(sc))
                img, st = r.render(pt.Camera.from_spec(sc.camera), spp, depth)
                marked = r.early_ends()
            finally:
                r.close()
        want, rays = refs[case]
        print(f"{hook} {case}: kernel_path {st['kernel_path']}, rays {st['rays']} (oracle {rays}), marked lane-segments "
              f"{marked}, launches {st.get('trace_launches')}")
        assert st["kernel_path"] == PATH_RTC, (hook, case)
        got, nan = np.ascontiguousarray(img), np.isnan(want)  # any two NaNs count as equal (x86 and gfx950 differ in the payload of inf * 0)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), (hook, case)
        assert st["rays"] == rays, (hook, case)
        if hook.startswith("count"):
            paths = res[0] * res[1] * spp
            if case in MARKED:
                # at least 7 / 16 of the camera rays are marked (more: the verdict is the wave's, so a fill
                # with one ray outside marks its whole batch) and trace their first segment marked; a
                # bounce ray is inside the domain and drops the mark at its first test, so the marked
                # segments stay below the ray count: both kinds met in the waves
                assert 0.3 * paths <= marked < rays, (hook, case, marked, paths, rays)
            elif name in ("cornell", "mcornell"):
                assert marked == 0, (hook, case, marked)  # ordinary cameras: the branch is never taken
        else:
            assert marked == 0, (hook, case, marked)  # no counter compiled in
