"""The a-trous denoiser on the GPU (pt_ctx_denoise, pt_ctx_moments_variance, pt_ctx_render_denoised;
Renderer.denoise, Renderer.moments_variance, Renderer.render_denoised, Renderer.aov(device=True);
DESIGN.md §3.20).

The yardstick is the host form (ptamd.denoise, ptamd.moments_variance), which
tests/test_denoise_cpu.py ties bit for bit to the numpy restatement of the contract. Every
comparison is of bits (NaN equals NaN). 131 x 67 spans more than two tiles of either form (64 x 4
and 32 x 16 pixels) plus an odd remainder on both axes."""
import functools

import numpy as np
import pytest

import _refdenoise as RD

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SIZES = [(1, 1), (1, 7), (5, 1), (37, 23), (64, 64), (131, 67)]  # (W, H)
FORMS = [None, "0", "1"]  # PT_DENOISE_LDS: the default, every pass direct, stride 1 tiled


@pytest.fixture(scope="module")
def ctx():
    """A context without a scene: the filter needs none."""
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
    r.set_scene(ptamd.BVH.from_scene(sc))
    yield r, ptamd.Camera.from_spec(sc.camera)
    r.close()


@functools.lru_cache(maxsize=None)
def host(W, H, passes, with_var):
    import ptamd
    color, var, g = RD.synthetic(W, H, seed=W * 100 + H)
    return ptamd.denoise(color, g, var if with_var else None, passes=passes)


def set_form(monkeypatch, form):
    if form is None:
        monkeypatch.delenv("PT_DENOISE_LDS", raising=False)
    else:
        monkeypatch.setenv("PT_DENOISE_LDS", form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("W,H", SIZES)
def test_matches_the_host_form(ctx, monkeypatch, W, H, form):
    set_form(monkeypatch, form)
    color, var, g = RD.synthetic(W, H, seed=W * 100 + H)
    for with_var in (True, False):
        for passes in [1, 2, 5] + ([8] if (W, H) == (37, 23) else []):
            want, want_v = host(W, H, passes, with_var)
            got, got_v, st = ctx.denoise(color, g, var if with_var else None, passes=passes)
            what = f"{W}x{H} passes {passes} var {with_var} form {form}"
            RD.assert_same(got, want, what)
            if with_var:
                RD.assert_same(got_v, want_v, what + " variance")
            else:
                assert got_v is None
            assert st["passes"] == passes and st["launches"] == passes + 1 and len(st["form"]) == passes
            assert all(f == "direct" for f in st["form"][1:])
            if form is not None:
                assert st["form"][0] == ("lds" if form == "1" else "direct")
            assert st["kernel_ms"] > 0 and st["total_ms"] >= st["kernel_ms"]


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def test_device_pointers_equal_host_pointers(ctx):
    import torch
    W, H = 131, 67
    color, var, g = RD.synthetic(W, H, seed=W * 100 + H)
    want, want_v = host(W, H, 5, True)
    gd = {k: to_dev(v) for k, v in g.items()}
    c, v = to_dev(color), to_dev(var)
    out, vout, st = ctx.denoise(c, gd, v)
    assert out.is_cuda and out.data_ptr() != c.data_ptr()
    RD.assert_same(out.cpu().numpy(), want, "device pointers")
    RD.assert_same(vout.cpu().numpy(), want_v, "device pointers, variance")
    assert np.array_equal(RD.bits(c.cpu().numpy()), RD.bits(color))  # the inputs are left as they were
    # in place: out and var_out are the inputs themselves
    out2, vout2, _ = ctx.denoise(c, gd, v, out=c, var_out=v)
    assert out2 is c and vout2 is v
    RD.assert_same(c.cpu().numpy(), want, "in place")
    RD.assert_same(v.cpu().numpy(), want_v, "in place, variance")
    # without a variance
    out3, vout3, _ = ctx.denoise(to_dev(color), gd)
    assert vout3 is None
    RD.assert_same(out3.cpu().numpy(), host(W, H, 5, False)[0], "device pointers, no variance")
    with pytest.raises(ValueError):
        ctx.denoise(to_dev(color), dict(gd, tri=gd["tri"].to(torch.float32)))
    with pytest.raises(ValueError):
        ctx.denoise(to_dev(color), dict(gd, t=g["t"]))  # a numpy guide beside tensors
    with pytest.raises(ValueError):
        ctx.denoise(to_dev(color), dict(gd, t=gd["t"].cpu()))  # a tensor that is not on the context's device
    with pytest.raises(ValueError):
        ctx.denoise(color, g, var, out=np.empty_like(color))  # numpy results are returned, not written in place


def test_guides_still_in_flight_on_torchs_stream(ctx):
    """The library's stream does not order itself after torch's, so the tensor paths wait for
    torch's current stream first. Here the guides' hit points, the variance and the colour are the
    results of torch operations queued behind about a hundred milliseconds of matrix products:
    when Renderer.denoise is called they are not written yet (their fresh memory holds whatever
    the allocator left there). Without the wait the results differ from the host form's."""
    import ptamd
    import torch
    W, H = 131, 67
    color, var, g = RD.synthetic(W, H, seed=W * 100 + H)
    ray = np.concatenate([g["position"] - F32(0.5), np.full((H, W, 3), 0.25, F32)], axis=-1)
    aov_host = {k: v for k, v in dict(g, ray=ray, t=np.full((H, W), 2.0, F32)).items() if k != "position"}
    aov = {k: to_dev(v) for k, v in aov_host.items()}
    want, want_v = ptamd.denoise(color, ptamd.denoise_guides(aov_host), var)
    c0, v0 = to_dev(color), to_dev(var)
    a = torch.randn((6144, 6144), device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):  # the second round reuses the first one's freed blocks
        b = a
        for _ in range(12):
            b = torch.tanh(b @ a * 1e-2)
        zero = (b[0, 0] * 0).nan_to_num()  # 0, known only when the products are done
        gd = ptamd.denoise_guides(aov)     # queued behind them
        c, v = c0 + zero, v0 + zero
        out, vout, _ = ctx.denoise(c, gd, v)
        RD.assert_same(out.cpu().numpy(), want, "guides in flight")
        RD.assert_same(vout.cpu().numpy(), want_v, "guides in flight, variance")
        S = torch.full((W * H, 3), 2.0, dtype=torch.float64, device="cuda:0") + zero
        Q = torch.full((W * H, 3), 5.0, dtype=torch.float64, device="cuda:0") + zero
        got = ctx.moments_variance(S, Q, 4)
        RD.assert_same(got.cpu().numpy(), ptamd.moments_variance(np.full((W * H, 3), 2.0), np.full((W * H, 3), 5.0), 4),
                       "moments in flight")
        del gd, c, v, out, vout, S, Q, got


def test_argument_errors(ctx):
    import ptamd
    color, var, g = RD.synthetic(6, 4, nasty=False)
    for kw in (dict(passes=9), dict(passes=-1), dict(sigma_l=-1.0), dict(sigma_z=float("nan")), dict(normal_pow_log2=11),
               dict(eps=-1.0)):
        with pytest.raises(ptamd.PTError):
            ctx.denoise(color, g, var, **kw)
    with pytest.raises(ptamd.PTError):
        ctx.denoise(color, {k: v for k, v in g.items() if k != "position"}, var)


def test_moments_variance_equals_the_host_helper(ctx):
    import ptamd
    rng = np.random.default_rng(6)
    npix = 1000  # more than one block, not a multiple of it
    x = rng.uniform(0, 3, (12, npix, 3)).astype(F32).astype(F64)
    spp = rng.integers(0, 13, npix).astype(np.int32)
    S = np.stack([x[:n, i].sum(axis=0) for i, n in enumerate(spp)])
    Q = np.stack([(x[:n, i] ** 2).sum(axis=0) for i, n in enumerate(spp)])
    S[3, 0], Q[4, 1] = np.nan, -1.0
    want_pp = ptamd.moments_variance(S, Q, spp=spp)
    want_12 = ptamd.moments_variance(S, Q, 12)
    assert np.isposinf(want_pp[spp < 2]).all() and (spp < 2).any() and np.isfinite(want_pp[spp >= 2]).all()
    RD.assert_same(ctx.moments_variance(S, Q, spp=spp), want_pp, "host pointers, per-pixel n")
    RD.assert_same(ctx.moments_variance(S, Q, 12), want_12, "host pointers, one n")
    RD.assert_same(ctx.moments_variance(S, Q, 1), np.full((npix, 3), np.inf, F32), "n < 2")
    got = ctx.moments_variance(to_dev(S), to_dev(Q), spp=to_dev(spp))
    assert got.is_cuda
    RD.assert_same(got.cpu().numpy(), want_pp, "device pointers, per-pixel n")
    RD.assert_same(ctx.moments_variance(to_dev(S), to_dev(Q), 12).cpu().numpy(), want_12, "device pointers, one n")


def test_aov_on_the_device_equals_the_host_aov(cornell):
    r, cam = cornell
    a, st = r.aov(cam, sample=0, seed=7)
    d, std = r.aov(cam, sample=0, seed=7, device=True)
    assert set(d) == set(a) and std["rays"] == st["rays"] and std["hits"] == st["hits"] > 0
    for k in a:
        assert d[k].is_cuda and tuple(d[k].shape) == a[k].shape
        assert np.array_equal(d[k].cpu().numpy().view(np.uint32), a[k].view(np.uint32)), k
    only, _ = r.aov(cam, sample=3, seed=7, channels=("t", "ray"), device=True)
    ref, _ = r.aov(cam, sample=3, seed=7, channels=("t", "ray"))
    assert set(only) == {"t", "ray"} and np.array_equal(only["ray"].cpu().numpy().view(np.uint32), ref["ray"].view(np.uint32))


ADAPT = dict(depth=5, rel=0.2, min_samples=16, max_samples=64, seed=5)


def test_render_denoised_equals_the_four_calls(cornell):
    import ptamd
    import torch
    r, cam = cornell
    img, noisy, spp, info = r.render_denoised(cam, **ADAPT)
    # by hand: render_adaptive, the AOV of sample 0 at the same seed, the variance with n_p, the filter
    want_noisy, mom, want_spp, _ = r.render_adaptive(cam, want=("sum", "sumsq"), **ADAPT)
    aov, _ = r.aov(cam, sample=0, seed=ADAPT["seed"])
    var = ptamd.moments_variance(mom["sum"], mom["sumsq"], spp=want_spp)
    want, _ = ptamd.denoise(want_noisy, ptamd.denoise_guides(aov), var)
    assert img.shape == (32, 32, 3) and spp.shape == (32, 32) and spp.dtype == np.int32
    assert np.array_equal(spp, want_spp) and len(np.unique(spp)) > 1 and spp.min() >= 16 and spp.max() <= 64
    assert np.array_equal(RD.bits(noisy), RD.bits(want_noisy))
    RD.assert_same(img, want, "render_denoised")
    assert (RD.bits(img) != RD.bits(noisy)).mean() > 0.5  # the filter ran
    assert info["denoise"]["passes"] == 5 and info["max_spp"] == int(spp.max()) and info["rays"] > 0
    # the same through device pointers, in place on a tensor
    out = torch.empty((32, 32, 3), dtype=torch.float32, device="cuda:0")
    img_d, noisy_d, spp_d, _ = r.render_denoised(cam, out=out, **ADAPT)
    assert img_d is out and noisy_d.is_cuda and spp_d.is_cuda
    RD.assert_same(out.cpu().numpy(), want, "render_denoised, device pointers")
    assert np.array_equal(RD.bits(noisy_d.cpu().numpy()), RD.bits(want_noisy))
    assert np.array_equal(spp_d.cpu().numpy(), want_spp)
    # the device pieces by hand give the same bits as well
    aov_d, _ = r.aov(cam, sample=0, seed=ADAPT["seed"], device=True)
    var_d = r.moments_variance(to_dev(mom["sum"]), to_dev(mom["sumsq"]), spp=to_dev(want_spp))
    den_d, _, _ = r.denoise(to_dev(want_noisy), ptamd.denoise_guides(aov_d), var_d)
    RD.assert_same(den_d.cpu().numpy(), want, "the four device calls")
    # explicit filter parameters reach the filter
    img2, _, _, _ = r.render_denoised(cam, passes=2, sigma_l=3.0, **ADAPT)
    RD.assert_same(img2, ptamd.denoise(want_noisy, ptamd.denoise_guides(aov), var, passes=2, sigma_l=3.0)[0], "passes 2")
    # rows dealt to other GPUs have no neighbours
    with pytest.raises(ptamd.PTError):
        r.render_denoised(cam, part_count=2, **ADAPT)
    with pytest.raises(ptamd.PTError):
        r.render_denoised(cam, passes=9, **ADAPT)


def test_a_running_sum_survives_denoise(cornell):
    r, cam = cornell
    whole, mom_whole, _ = r.render_moments(cam, 0, 12, 5, seed=2)
    r.render_moments(cam, 0, 8, 5, seed=2)
    color, var, g = RD.synthetic(37, 23, seed=1)
    r.denoise(color, g, var)
    r.moments_variance(mom_whole["sum"], mom_whole["sumsq"], 12)
    img, mom, _ = r.render_moments(cam, 8, 4, 5, seed=2)  # continues: PTError if the sum had ended
    assert np.array_equal(RD.bits(img), RD.bits(whole))
    assert np.array_equal(mom["sum"], mom_whole["sum"]) and np.array_equal(mom["sumsq"], mom_whole["sumsq"])
    assert r.unconverged(0.1) >= 0
