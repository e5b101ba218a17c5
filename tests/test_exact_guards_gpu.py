"""The wave-uniform range guards of the exact fast math (pt_math.h: rcp_exact, sqrt_exact,
rcp3_exact, normalize_fast) on the GPU: every lane runs the fast sequence, and one out-of-range
lane sends its whole wave through the IEEE operations. What that can get wrong is a wave with
lanes on both sides, so every case here mixes them: exhaustive sweeps whose waves always hold
forced out-of-range inputs, caller rays with a zero, a subnormal, a huge and an infinite direction
component inside a wave of ordinary ones, and renders in which one camera ray has d.x == 0."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as O
import _reftrace as RT

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def ptamd_mod():
    import ptamd
    if ptamd.lib().pt_device_count() <= 0:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    return ptamd


# ---------------------------------------------------------------- sweeps (pt_debug_sweep, all 2^32 bit patterns)
@pytest.mark.parametrize("which", [5, 6, 7, 8, 9])
def test_wave_uniform_guard_sweeps(ptamd_mod, which):
    """5: rcp3_exact on {x, x, x} against 1.0f / x, the unit-vector form (lower bound only) for
    |x| <= 2 and the two-sided form elsewhere. 6: rcp3_exact on {x, b, c} against the three IEEE
    reciprocals, with four lanes of every wave forced to +-0, a subnormal, 2^127, +-inf or a value
    in (2^126, 2^128) in b and c. 7: normalize_fast in the same arrangement against the IEEE square
    root and divisions; 8: the same without the forced lanes, so that waves keep the fast result.
    9: as 6 without the forced lanes, so that waves keep the fast reciprocals of three different
    components, and with a NaN as the second component of one input in 16: min3 / max3 skip it, the
    wave keeps the fast path, and that component must be a NaN (any payload) beside two exact ones.
    NaN inputs skipped, as in the older modes; about 0.1 s each."""
    lib = ptamd_mod.lib()
    bad, first = C.c_uint64(0), C.c_uint32(0)
    assert lib.pt_debug_sweep(0, which, 0, 0xFFFFFFFF, C.byref(bad), C.byref(first)) == 0, lib.pt_last_error()
    print(f"sweep {which}: {bad.value} mismatches, first 0x{first.value:08x}")
    assert bad.value == 0, f"{bad.value} mismatches, first input bits 0x{first.value:08x}"
    assert first.value == 0xFFFFFFFF


# ---------------------------------------------------------------- caller rays through trace()
SPECIAL = {3: (0, F32(0.0)), 17: (1, F32(-0.0)), 31: (2, np.array([0x00000123], np.uint32).view(F32)[0]),
           40: (0, F32(2.0) ** 127), 63: (1, F32(np.inf))}  # lane of wave 1 -> (component, value)


@functools.lru_cache(maxsize=None)
def _mixed_rays(name):
    """128 rays, two waves: wave 0 ordinary, wave 1 with five lanes' direction components replaced;
    and the restated trace()'s radiance and segment counts for them (depth 5, default seeding)."""
    o, d = RT.rays(name, 128)
    o, d = o.copy(), d.copy()
    for lane, (c, v) in SPECIAL.items():
        d[64 + lane, c] = v
    verts, nodes, idx, mtype, mvals = RT.scene_arrays(name)
    want, _, segs = RT.trace(nodes, idx, verts, mtype, mvals, o, d, RT.sample_seeds(128, 1, 1)[:, 0], 5)
    return o, d, want, segs


@pytest.mark.parametrize("name", ["cornell", "cornell+glow"])
def test_caller_rays_with_out_of_range_lanes(ptamd_mod, name):
    """Radiance bits and ray count of the two waves against the restated trace(): the lanes with a
    zero, -0, subnormal, 2^127 and +inf direction component take the IEEE reciprocals, and so does
    every ordinary lane of their wave, with the bits the fast sequence would have given it (the
    glow variant too, where every hit path returns a non-zero value).
    trace() on caller rays has one kernel family, pt_paths_kernel over the binary tree
    (pt_ctx_trace -> paths_launch), whatever kernel the scene's renders use: PT_RTC, PT_FLAT and
    PT_WIDE do not reach it. The scene kernel and the table kernels get their mixed wave from the
    renders below."""
    o, d, want, segs = _mixed_rays(name)
    r = ptamd_mod.Renderer(0)
    try:
        r.set_scene(ptamd_mod.BVH.from_scene(RT.make_scene(name)))
        got, st = r.trace(o, d, 5)
        first, _ = r.trace(o[:64], d[:64], 5)  # wave 0 alone: the all-ordinary wave keeps the fast path
    finally:
        r.close()
    RT.assert_same(got, want, name)
    RT.assert_same(first, want[:64], f"{name}: wave 0 alone")
    assert st["rays"] == int(segs.sum()) and st["paths"] == 128
    # the plan that ran: one launch of pt_paths_kernel, Cornell's scene, stacks and records in LDS
    assert st["launches"] == 1 and st["lds_scene"] == 1 and st["lds_stack"] == 1 and st["lds_records"] == 1
    if name.endswith("glow"):
        assert (got.view(np.uint32) != 0).any(axis=1).sum() >= 64


# ---------------------------------------------------------------- a camera ray with d.x == 0
# pt_sample_seed is a bijection of the seed, so the seed that gives a chosen pixel's sample 0 a
# chosen x jitter is solved for, not searched: 16 x 16 has cx == 0 in column 8 for a jitter of 0
# (LCG state 0 after the two draws), 15 x 15 in its centre column 7 for a jitter of 0.5 (state 2^31).
ZERO_CX = {(16, 16): 1170511184, (15, 15): 3737529250}


@functools.lru_cache(maxsize=None)
def _zero_cx_reference(res):
    from ptamd import scenes
    sc = scenes.cornell(res)
    seed = ZERO_CX[res]
    _, d, _ = RT.camera_rays(sc, seed)  # sample 0 of every pixel
    zero = np.flatnonzero(d[:, 0] == 0)
    ref, rays = O.render(sc, 4, 5, seed)
    return sc, seed, zero, ref, rays


@pytest.mark.parametrize("env,path", [({}, 3), ({"PT_RTC": "0"}, 5), ({"PT_RTC": "0", "PT_FLAT_FAST": "0"}, 2),
                                      ({"PT_FLAT": "0"}, 4)],
                         ids=["scene_kernel", "table_kernel_scene_flags", "table_kernel_generic", "wide_kernel"])
@pytest.mark.parametrize("res", sorted(ZERO_CX))
def test_render_with_a_zero_direction_component(ptamd_mod, monkeypatch, res, env, path):
    """Cornell, 4 spp, depth 5, seeded so that one camera sample's cx is exactly 0: its direction
    has d.x == 0 (checked on the CPU first), so 1 / d.x is the IEEE +inf and that lane's wave takes
    the fallback among ordinary lanes, wherever the kernel builds a camera ray's inv. Run on the
    hipRTC scene kernel, the table kernel with the scene's flags, the generic table kernel and the
    wide kernel, each checked by its kernel path. Bit for bit against the oracle."""
    sc, seed, zero, ref, rays = _zero_cx_reference(res)
    assert zero.size >= 1, "the oracle's camera rays hold no zero x component"
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bvh = ptamd_mod.BVH.from_scene(sc)
    img, st = ptamd_mod.render(ptamd_mod.Camera.from_spec(sc.camera), bvh, 4, 5, seed=seed)
    assert st["kernel_path"] == path
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), \
        f"{int((img.view(np.uint32) != ref.view(np.uint32)).sum())} words differ"
    assert st["rays"] == rays
    assert ref.view(np.uint32).any()
