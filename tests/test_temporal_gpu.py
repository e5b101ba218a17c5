"""Temporal reprojection on the GPU (pt_ctx_temporal, pt_ctx_render_temporal;
Renderer.temporal_accumulate, Renderer.render_temporal).

The yardstick is the host form (ptamd.temporal_accumulate), which tests/test_temporal_cpu.py ties
bit for bit to the numpy restatement of the contract. Every comparison is of bits (NaN equals
NaN). 131 x 67 spans more than two blocks of 64 x 4 pixels on both axes with odd remainders;
1 x 1 and 5 x 1 are the shapes where every tap but one falls outside the image."""
import dataclasses
import functools

import numpy as np
import pytest

import _refdenoise as RD
import _reftemporal as RT

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [(1, 1), (1, 7), (5, 1), (37, 23), (64, 64), (131, 67)]  # (W, H)
MODES = [RT.SAMPLE, RT.TEMPORAL]


@pytest.fixture(scope="module")
def ctx():
    """A context without a scene: the accumulation needs none."""
    import ptamd
    r = ptamd.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def cornell():
    import ptamd
    from ptamd import scenes
    sc = scenes.cornell((32, 32))
    r = ptamd.Renderer(0)
    bvh = ptamd.BVH.from_scene(sc)
    r.set_scene(bvh)
    moved = dataclasses.replace(sc.camera, pos=(sc.camera.pos[0] + 28.0, sc.camera.pos[1], sc.camera.pos[2]))
    yield r, bvh, ptamd.Camera.from_spec(sc.camera), ptamd.Camera.from_spec(moved)
    r.close()


def cameras(s):
    import ptamd
    cur = ptamd.Camera(*RT.camera_spec(s.cam_cur))
    return cur, (cur if s.cam_prev is s.cam_cur else ptamd.Camera(*RT.camera_spec(s.cam_prev)))


def history(planes):
    import ptamd
    return ptamd.TemporalHistory(**{k: np.ascontiguousarray(planes[k]) for k in RT.NAMES})


@functools.lru_cache(maxsize=None)
def host(W, H, move, mode):
    import ptamd
    s = RT.synthetic(W, H, seed=W * 100 + H, move=move)
    cur, old = cameras(s)
    return ptamd.temporal_accumulate(s.color, s.guides, cur, history(s.prev), old, var=s.var, variance_mode=mode)


def assert_history(got, want, what):
    for k in RT.NAMES:
        g, w = getattr(got, k), getattr(want, k)
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        if k in ("hist", "cls"):
            assert g.dtype == np.int32 and np.array_equal(g, w), f"{what}: {k}"
        else:
            RD.assert_same(g, w, f"{what}: {k}")


@pytest.mark.parametrize("move", RT.MOVES)
@pytest.mark.parametrize("W,H", SIZES)
def test_matches_the_host_form(ctx, W, H, move):
    s = RT.synthetic(W, H, seed=W * 100 + H, move=move)
    cur, old = cameras(s)
    for mode in MODES:
        want, want_reused = host(W, H, move, mode)
        got, st = ctx.temporal_accumulate(s.color, s.guides, cur, history(s.prev), old, var=s.var, variance_mode=mode)
        assert st["reused"] == want_reused
        assert_history(got, want, f"{W}x{H} {move} mode {mode}")
        assert st["kernel_ms"] > 0 and st["total_ms"] >= st["kernel_ms"]
    if move == "pixels" and W * H >= 20:
        hit = int((RD.classes(s.guides["tri"], s.guides["emission"]) != 0).sum())
        assert 0.3 * hit <= host(W, H, move, RT.SAMPLE)[1] <= 0.9 * hit


def test_first_frame(ctx):
    import ptamd
    s = RT.synthetic(131, 67, seed=2, move="pixels")
    cur, _ = cameras(s)
    for var in (s.var, None):
        want, _ = ptamd.temporal_accumulate(s.color, s.guides, cur, var=var)
        got, st = ctx.temporal_accumulate(s.color, s.guides, cur, var=var)
        assert st["reused"] == 0
        assert_history(got, want, "first frame")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def test_device_pointers_equal_host_pointers(ctx):
    import ptamd
    import torch
    W, H = 131, 67
    s = RT.synthetic(W, H, seed=W * 100 + H, move="pixels")
    cur, old = cameras(s)
    gd = {k: to_dev(v) for k, v in s.guides.items()}
    c, v = to_dev(s.color), to_dev(s.var)
    prev = ptamd.TemporalHistory(**{k: to_dev(s.prev[k]) for k in RT.NAMES})
    for mode in MODES:
        want, want_reused = host(W, H, "pixels", mode)
        got, st = ctx.temporal_accumulate(c, gd, cur, prev, old, var=v, variance_mode=mode)
        assert got.color.is_cuda and got.hist.dtype == torch.int32 and st["reused"] == want_reused
        assert_history(got, want, f"device pointers, mode {mode}")
    # into a history of the caller's
    out = ptamd.TemporalHistory.empty(W, H, like=c)
    got, _ = ctx.temporal_accumulate(c, gd, cur, prev, old, var=v, out=out)
    assert got is out
    assert_history(out, host(W, H, "pixels", RT.SAMPLE)[0], "out")
    # the inputs are left as they were
    assert np.array_equal(RD.bits(c.cpu().numpy()), RD.bits(s.color))
    assert np.array_equal(RD.bits(v.cpu().numpy()), RD.bits(s.var))
    for k in RT.NAMES:
        a = getattr(prev, k).cpu().numpy()
        assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(s.prev[k]).view(np.uint32)), k
    for k, x in gd.items():
        assert np.array_equal(x.cpu().numpy().view(np.uint32), s.guides[k].view(np.uint32)), k
    with pytest.raises(ValueError):  # not contiguous
        ctx.temporal_accumulate(c.transpose(0, 1).contiguous().transpose(0, 1), gd, cur, prev, old, var=v)
    with pytest.raises(ValueError):  # a tensor that is not on the context's device
        ctx.temporal_accumulate(c, dict(gd, t=gd["t"].cpu()), cur, prev, old, var=v)
    with pytest.raises(ValueError):  # a numpy guide beside tensors
        ctx.temporal_accumulate(c, dict(gd, t=s.guides["t"]), cur, prev, old, var=v)
    with pytest.raises(ValueError):  # a numpy history beside tensors
        ctx.temporal_accumulate(c, gd, cur, history(s.prev), old, var=v)
    with pytest.raises(ValueError):  # tensors beside a numpy colour
        ctx.temporal_accumulate(s.color, gd, cur, history(s.prev), old, var=s.var)
    with pytest.raises(ValueError):
        ctx.temporal_accumulate(c, gd, cur, ptamd.TemporalHistory(**dict(prev.planes(), hist=prev.hist.to(torch.float32))),
                                old, var=v)
    with pytest.raises(ValueError):  # numpy results are returned, not written in place
        ctx.temporal_accumulate(s.color, s.guides, cur, history(s.prev), old, var=s.var, out=ptamd.TemporalHistory.empty(W, H))
    # it is a gather: the next history may not share memory with the previous one
    with pytest.raises(ptamd.PTError):
        ctx.temporal_accumulate(c, gd, cur, prev, old, var=v, out=prev)
    with pytest.raises(ptamd.PTError):
        ctx.temporal_accumulate(c, gd, cur, prev, old, var=v,
                                out=ptamd.TemporalHistory(**dict(ptamd.TemporalHistory.empty(W, H, like=c).planes(), m2=prev.color)))


def test_argument_errors(ctx):
    import ptamd
    s = RT.synthetic(6, 4, seed=1, move="subpixel")
    cur, old = cameras(s)
    for kw in (dict(max_history=-1), dict(max_history=65536), dict(sigma_z=-1.0), dict(sigma_z=float("nan")),
               dict(normal_min=1.0), dict(variance_mode=3)):
        with pytest.raises(ptamd.PTError):
            ctx.temporal_accumulate(s.color, s.guides, cur, history(s.prev), old, var=s.var, **kw)
    with pytest.raises(ptamd.PTError):  # sample mode without a variance
        ctx.temporal_accumulate(s.color, s.guides, cur, history(s.prev), old, variance_mode=RT.SAMPLE)
    with pytest.raises(ptamd.PTError):
        ctx.temporal_accumulate(s.color, {k: v for k, v in s.guides.items() if k != "position"}, cur, history(s.prev), old)


def test_history_still_in_flight_on_torchs_stream(ctx):
    """The library's stream does not order itself after torch's, so the tensor path waits for
    torch's current stream first. Here the previous history's planes, the colour and the variance
    are the results of torch operations queued behind about a hundred milliseconds of matrix
    products: when Renderer.temporal_accumulate is called they are not written yet (their fresh
    memory holds whatever the allocator left there). Without the wait the results differ from the
    host form's."""
    import ptamd
    import torch
    W, H = 131, 67
    s = RT.synthetic(W, H, seed=W * 100 + H, move="pixels")
    cur, old = cameras(s)
    want, want_reused = host(W, H, "pixels", RT.SAMPLE)
    gd = {k: to_dev(v) for k, v in s.guides.items()}
    c0, v0 = to_dev(s.color), to_dev(s.var)
    p0 = {k: to_dev(s.prev[k]) for k in RT.NAMES}
    a = torch.randn((6144, 6144), device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):  # the second round reuses the first one's freed blocks
        b = a
        for _ in range(12):
            b = torch.tanh(b @ a * 1e-2)
        zero = (b[0, 0] * 0).nan_to_num()  # 0, known only when the products are done
        izero = zero.to(torch.int32)
        prev = ptamd.TemporalHistory(**{k: p0[k] + (izero if p0[k].dtype == torch.int32 else zero) for k in RT.NAMES})
        c, v = c0 + zero, v0 + zero
        got, st = ctx.temporal_accumulate(c, gd, cur, prev, old, var=v)
        assert st["reused"] == want_reused
        assert_history(got, want, "history in flight")
        del prev, c, v, got


def by_hand(r, cam, spp, depth, seed, hist, cam_old):
    """The five calls of one frame: render_moments, the AOV of sample 0 at the same seed (and its
    hit points), the variance of the mean, the accumulation, the filter."""
    import ptamd
    img, mom, _ = r.render_moments(cam, 0, spp, depth, seed=seed, want=("sum", "sumsq"))
    aov, _ = r.aov(cam, sample=0, seed=seed)
    g = ptamd.denoise_guides(aov)
    var = ptamd.moments_variance(mom["sum"], mom["sumsq"], spp) if spp >= 2 else None
    nxt, st = r.temporal_accumulate(img, g, cam, hist, cam_old, var=var)
    out, _, _ = r.denoise(nxt.color, g, nxt.var)
    return out, nxt, st["reused"]


@pytest.mark.parametrize("spp", [4, 1])
def test_render_temporal_equals_the_five_calls(cornell, spp):
    import ptamd
    import torch
    r, bvh, cam0, cam1 = cornell
    depth, cams, seeds = 3, [cam0, cam0, cam1], [11, 12, 13]
    frames = [r.render_temporal(cam, spp, depth, seed=seed, reset=(i == 0))
              for i, (cam, seed) in enumerate(zip(cams, seeds))]
    hist, cam_old = None, None
    for i, (cam, seed) in enumerate(zip(cams, seeds)):
        want, hist, reused = by_hand(r, cam, spp, depth, seed, hist, cam_old)
        cam_old = cam
        img, acc, info = frames[i]
        assert img.shape == (32, 32, 3) and img.dtype == F32
        RD.assert_same(img, want, f"spp {spp} frame {i}: out")
        RD.assert_same(acc, hist.color, f"spp {spp} frame {i}: accumulated")
        assert info["reused"] == reused and info["had_history"] == (1 if i else 0)
        assert info["variance_mode"] == (RT.SAMPLE if spp >= 2 else RT.TEMPORAL)
        assert info["denoise"]["passes"] == 5 and info["rays"] > 0 and info["total_ms"] > 0
        assert (reused > 300) == (i > 0)  # most of the 1024 pixels, also after the move
    assert (RD.bits(frames[2][0]) != RD.bits(frames[2][1])).mean() > 0.5  # the filter ran
    assert hist.hist.max() == 3
    first = by_hand(r, cam1, spp, depth, 13, None, None)
    # reset=True starts a history: the first-frame result
    img, acc, info = r.render_temporal(cam1, spp, depth, seed=13, reset=True)
    RD.assert_same(img, first[0], "reset")
    RD.assert_same(acc, first[1].color, "reset: accumulated")
    assert info["had_history"] == 0 and info["reused"] == 0
    # so does set_scene in between
    assert r.render_temporal(cam1, spp, depth, seed=14)[2]["had_history"] == 1
    r.set_scene(bvh)
    img, acc, info = r.render_temporal(cam1, spp, depth, seed=13)
    RD.assert_same(img, first[0], "after set_scene")
    assert info["had_history"] == 0
    # the same through device pointers, in place on a tensor
    out = torch.empty((32, 32, 3), dtype=torch.float32, device="cuda:0")
    img_d, acc_d, info = r.render_temporal(cam1, spp, depth, seed=13, reset=True, out=out)
    assert img_d is out and acc_d.is_cuda
    RD.assert_same(out.cpu().numpy(), first[0], "device pointers")
    RD.assert_same(acc_d.cpu().numpy(), first[1].color, "device pointers: accumulated")
    # explicit parameters reach both steps
    img2, _, _ = r.render_temporal(cam1, spp, depth, seed=13, reset=True, passes=2, max_history=2)
    assert not RD.same_bits(img2, first[0]).all()
    # rows dealt to other GPUs have no neighbours; an error drops the history
    with pytest.raises(ptamd.PTError):
        r.render_temporal(cam1, spp, depth, seed=15, part_count=2)
    assert r.render_temporal(cam1, spp, depth, seed=15)[2]["had_history"] == 0
    with pytest.raises(ptamd.PTError):
        r.render_temporal(cam1, spp, depth, seed=15, max_history=-1)


def test_a_running_sum_survives_temporal_accumulate(cornell):
    r, _, cam, _ = cornell
    whole, mom_whole, _ = r.render_moments(cam, 0, 12, 3, seed=2)
    r.render_moments(cam, 0, 8, 3, seed=2)
    s = RT.synthetic(37, 23, seed=1, move="pixels")
    cur, old = cameras(s)
    r.temporal_accumulate(s.color, s.guides, cur, history(s.prev), old, var=s.var)
    img, mom, _ = r.render_moments(cam, 8, 4, 3, seed=2)  # continues: PTError if the sum had ended
    assert np.array_equal(RD.bits(img), RD.bits(whole))
    assert np.array_equal(mom["sum"], mom_whole["sum"]) and np.array_equal(mom["sumsq"], mom_whole["sumsq"])
