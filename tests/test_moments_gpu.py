"""Per-pixel sample moments, the convergence count and rendering to a noise target on the GPU
(pt_ctx_render_moments, pt_ctx_unconverged, pt_ctx_render_converge).

The yardstick: none of the code under test produces the per-sample values r[s] compared against.
Sample s of every pixel is Renderer.aov's camera ray traced by Renderer.trace from the LCG state
after the camera's two draws (tests/test_trace_gpu.py::test_camera_ray_identity); S, Q and the
float32 image follow from r[s] by numpy loops in sample order, and every test first ties the
float32 mean to the CPU oracle's render bit for bit."""
import numpy as np
import pytest

import _oracle as O
import _reftrace as RT
from test_moments_cpu import np_unconverged

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DEPTH, SEED = 5, 3
DARK, GLOW = "cornell", "cornell+glow"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


@pytest.fixture(scope="module")
def renderers():
    """One context per (scene, resolution), scene uploaded; closed at the end of the module."""
    import ptamd
    made = {}

    def get(name, res=(16, 16)):
        key = (name, tuple(res))
        if key not in made:
            sc = RT.make_scene(name, res)
            r = ptamd.Renderer(0)
            r.set_scene(ptamd.BVH.from_scene(sc))
            made[key] = (r, sc, ptamd.Camera.from_spec(sc.camera))
        return made[key]

    yield get
    for r, _, _ in made.values():
        r.close()


@pytest.fixture(scope="module")
def yardstick(renderers):
    """r[s] of the whole image: (n, H, W, 3) float32, computed once per (scene, resolution) for the
    most samples any test asks for and left unchanged (callers slice it)."""
    made = {}
    most = {(GLOW, (16, 16)): 256, (DARK, (16, 16)): 300}

    def get(name, n, res=(16, 16)):
        key = (name, tuple(res))
        if key not in made:
            r, sc, cam = renderers(name, res)
            W, H = res
            count = most.get(key, 70)
            seeds = RT.sample_seeds(W * H, count, SEED)  # the pixel's global index h W + w
            rays = np.stack([r.aov(cam, sample=s, seed=SEED, channels=("ray",))[0]["ray"].reshape(-1, 6)
                             for s in range(count)])
            o = np.ascontiguousarray(rays[..., 0:3].reshape(-1, 3))
            d = np.ascontiguousarray(rays[..., 3:6].reshape(-1, 3))
            states = RT.lcg_step(seeds.T.reshape(-1), 2).reshape(-1, 1)  # [s][pixel], as the rays
            rgb, _ = r.trace(o, d, DEPTH, states=states)
            vals = rgb.reshape(count, H, W, 3)
            vals.setflags(write=False)
            made[key] = vals
        assert n <= made[key].shape[0]
        return made[key][:n]

    return get


def np_moments(r):
    """S, Q (float64, added in sample order from +0.0) and the float32 in-order mean of r[s]."""
    S, Q, acc = np.zeros(r.shape[1:], F64), np.zeros(r.shape[1:], F64), np.zeros(r.shape[1:], F32)
    for s in range(r.shape[0]):
        v = r[s].astype(F64)
        S = S + v
        Q = Q + v * v
        acc = acc + r[s]
    with np.errstate(all="ignore"):
        mean = acc / F32(r.shape[0])
    return S, Q, mean


def tied(yardstick, renderers, name, n, res=(16, 16)):
    """The yardstick's (S, Q, mean) of n samples, its mean first checked against the CPU oracle."""
    S, Q, mean = np_moments(yardstick(name, n, res))
    ref, _ = O.render(renderers(name, res)[1], n, DEPTH, SEED)
    assert np.array_equal(bits(mean), bits(ref)), f"{name} {res} n={n}: yardstick != oracle"
    return S, Q, mean


def np_sem(S, Q, n):
    if n < 2:
        return np.full(S.shape, np.inf, F32)
    dn = F64(n)
    var = (Q - S * S / dn) / (dn - F64(1))
    return np.sqrt(np.maximum(F64(0), var) / dn).astype(F32)


BATCHES = [(37, 13), (70, 70), (70, 0), (37, 0)]
HOOKS = [{}, {"PT_FLAGS_PM": "0"}, {"PT_FLAGS_PM": "1"}, {"PT_FLAGS": "0"}]


@pytest.mark.parametrize("res", [(16, 16), (7, 5)])
@pytest.mark.parametrize("name", [DARK, GLOW])
def test_sum_sumsq_image_bit_exact(renderers, yardstick, monkeypatch, name, res):
    """Dense slabs (glow) and flagged ones (dark; both bit layouts, and forced dense), three
    launches with odd tails, a launch past a 64-sample flag group, the automatic batch; on the dark
    scene also 300 samples in one launch: the walk's steps of 8 flag words and of 32 sample-major
    bits, each with a tail."""
    r, sc, cam = renderers(name, res)
    assert r.flags()["dark"] == (name == DARK)
    nonzero = 0
    for n, batch in BATCHES + ([(300, 0)] if (name, res) == (DARK, (16, 16)) else []):
        S, Q, mean = tied(yardstick, renderers, name, n, res)
        want_img, _ = r.render(cam, n, DEPTH, seed=SEED)
        assert np.array_equal(bits(want_img), bits(mean))
        for hooks in HOOKS:
            for k, v in hooks.items():
                monkeypatch.setenv(k, v)
            img, mom, st = r.render_moments(cam, 0, n, DEPTH, seed=SEED, batch_spp=batch)
            for k in hooks:
                monkeypatch.delenv(k)
            what = f"{name} {res} n={n} batch={batch} {hooks}"
            assert np.array_equal(bits(mom["sum"]), bits(S)), what
            assert np.array_equal(bits(mom["sumsq"]), bits(Q)), what
            assert np.array_equal(bits(img), bits(want_img)), what
            plan = r.plan()
            assert plan["fused"] == 0 and plan["trace_launches"] == (3 if batch == 13 else 1), (what, plan)
            # flagged slabs: pixel-major bits for a render of several launches, unless the hook says
            want_pm = -1 if name == GLOW or hooks.get("PT_FLAGS") == "0" else \
                int(hooks.get("PT_FLAGS_PM", "1" if batch == 13 else "0"))
            assert plan["flags_pm"] == want_pm, (what, plan)
        nonzero += int((S != 0).sum())
    assert nonzero > 0  # not a comparison of zeros


def test_continuation_and_mixing(renderers, yardstick):
    import ptamd
    r, sc, cam = renderers(DARK)
    g, _, gcam = renderers(GLOW)
    for rr, name, c in ((r, DARK, cam), (g, GLOW, gcam)):
        S, Q, mean = tied(yardstick, renderers, name, 70)
        S37, Q37, mean37 = tied(yardstick, renderers, name, 37)
        rr.render_moments(c, 0, 5, DEPTH, seed=SEED)
        img, mom, _ = rr.render_moments(c, 5, 32, DEPTH, seed=SEED)
        assert np.array_equal(bits(mom["sum"]), bits(S37)) and np.array_equal(bits(mom["sumsq"]), bits(Q37))
        assert np.array_equal(bits(img), bits(mean37))
        # a trace call (buffers of its own) leaves the sum valid
        o = np.zeros((3, 3), F32) + F32(0.5)
        d = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], F32)
        rr.trace(o, d, DEPTH)
        img, mom, _ = rr.render_moments(c, 37, 33, DEPTH, seed=SEED, batch_spp=9)
        one_img, one, _ = rr.render_moments(c, 0, 70, DEPTH, seed=SEED)
        for k in ("sum", "sumsq", "sem"):
            assert np.array_equal(bits(mom[k]), bits(one[k])), (name, k)
        assert np.array_equal(bits(mom["sum"]), bits(S)) and np.array_equal(bits(mom["sumsq"]), bits(Q))
        assert np.array_equal(bits(img), bits(one_img)) and np.array_equal(bits(img), bits(mean))
    # a moments sum cannot be continued by render_progressive, nor the other way round
    r.render_moments(cam, 0, 5, DEPTH, seed=SEED)
    with pytest.raises(ptamd.PTError):
        r.render_progressive(cam, 5, 3, DEPTH, seed=SEED)
    r.render_progressive(cam, 0, 5, DEPTH, seed=SEED)
    with pytest.raises(ptamd.PTError):
        r.render_moments(cam, 5, 3, DEPTH, seed=SEED)
    with pytest.raises(ptamd.PTError):
        r.unconverged(0.1)  # no moments sum
    r.render_progressive(cam, 5, 3, DEPTH, seed=SEED)  # the progressive sum itself still continues
    # another seed, a gap in the samples, or a plain render in between end the moments sum
    r.render_moments(cam, 0, 5, DEPTH, seed=SEED)
    with pytest.raises(ptamd.PTError):
        r.render_moments(cam, 5, 3, DEPTH, seed=SEED + 1)
    with pytest.raises(ptamd.PTError):
        r.render_moments(cam, 6, 3, DEPTH, seed=SEED)
    r.render_moments(cam, 0, 5, DEPTH, seed=SEED)
    r.render(cam, 2, DEPTH, seed=SEED)
    with pytest.raises(ptamd.PTError):
        r.render_moments(cam, 5, 3, DEPTH, seed=SEED)


@pytest.mark.parametrize("name", [DARK, GLOW])
def test_partition_rows(renderers, yardstick, name):
    r, sc, cam = renderers(name)
    n = 37
    S, Q, mean = tied(yardstick, renderers, name, n)
    rows = [h for h in range(16) if (h // 2) % 3 == 1]
    assert rows == [2, 3, 8, 9, 14, 15]
    part = dict(part_index=1, part_count=3, band_rows=2)
    img, mom, st = r.render_moments(cam, 0, 20, DEPTH, seed=SEED, batch_spp=7, **part)
    img, mom, st = r.render_moments(cam, 20, 17, DEPTH, seed=SEED, **part)
    assert img.shape == (6, 16, 3) and st["rows"] == 6
    assert np.array_equal(bits(mom["sum"]), bits(S[rows])) and np.array_equal(bits(mom["sumsq"]), bits(Q[rows]))
    assert np.array_equal(bits(img), bits(mean[rows]))
    whole_img, whole, _ = r.render_moments(cam, 0, n, DEPTH, seed=SEED)
    for k in ("sum", "sumsq", "sem"):
        assert np.array_equal(bits(mom[k]), bits(whole[k][rows])), k
    import ptamd
    with pytest.raises(ptamd.PTError):
        r.render_moments(cam, n, 1, DEPTH, seed=SEED, **part)  # the whole-image sum is another partition


def test_sem(renderers, yardstick):
    """Equal to numpy's double evaluation rounded to float32, or the float beside it (the
    device's double square root may differ by one double ulp)."""
    some = 0
    for name in (DARK, GLOW):
        r, sc, cam = renderers(name)
        for n in (2, 37, 70):
            S, Q, _ = tied(yardstick, renderers, name, n)
            _, mom, _ = r.render_moments(cam, 0, n, DEPTH, seed=SEED, want=("sem",))
            assert set(mom) == {"sem"} and mom["sem"].dtype == F32
            want = np_sem(S, Q, n)
            assert np.isfinite(want).all() and np.isfinite(mom["sem"]).all() and (mom["sem"] >= 0).all()
            off = np.abs(bits(mom["sem"]).astype(np.int64) - bits(want).astype(np.int64))
            assert off.max() <= 1, (name, n, int(off.max()))
            some += int((mom["sem"] > 0).sum())
        _, mom, _ = r.render_moments(cam, 0, 1, DEPTH, seed=SEED)
        assert np.array_equal(bits(mom["sem"]), bits(np.full((16, 16, 3), np.inf, F32)))
    assert some > 100


def test_count_and_mask(renderers, yardstick):
    import ptamd
    r, sc, cam = renderers(GLOW)
    n, npix = 37, 256
    S, Q, _ = tied(yardstick, renderers, GLOW, n)
    # tolerances from the yardstick: the median pixel's worst channel, so that about half converge
    mean = np.abs(S) / n
    sem = np_sem(S, Q, n).astype(F64)
    with np.errstate(all="ignore"):
        relerr = np.where(mean > 0, sem / mean, 0.0).max(axis=-1)
    pairs = [(float(F32(np.median(relerr))), 0.0), (0.0, float(F32(np.median(sem.max(axis=-1))))),
             (float(F32(0.5 * np.median(relerr))), float(F32(0.25 * np.median(sem.max(axis=-1)))))]
    _, mom, _ = r.render_moments(cam, 0, n, DEPTH, seed=SEED)
    assert np.array_equal(bits(mom["sum"]), bits(S)) and np.array_equal(bits(mom["sumsq"]), bits(Q))
    counts = []
    for rel, abs_ in pairs:
        want = np_unconverged(S, Q, n, rel, abs_).reshape(-1)
        assert 0 < int(want.sum()) < npix, (rel, abs_, int(want.sum()))  # the precondition, on the yardstick
        cnt, mask = r.unconverged(rel, abs_, mask=True)
        assert cnt == int(want.sum()) == r.unconverged(rel, abs_)
        assert np.array_equal(mask, want)
        assert cnt == ptamd.moments_unconverged(mom["sum"], mom["sumsq"], n, rel, abs_)
        counts.append(cnt)
    # an odd pixel count (less than a wave), a partition, and n < 2
    r2, _, cam2 = renderers(GLOW, (7, 5))
    S2, Q2, _ = tied(yardstick, renderers, GLOW, n, (7, 5))
    r2.render_moments(cam2, 0, n, DEPTH, seed=SEED)
    for rel, abs_ in pairs:
        want = np_unconverged(S2, Q2, n, rel, abs_).reshape(-1)
        cnt, mask = r2.unconverged(rel, abs_, mask=True)
        assert cnt == int(want.sum()) and np.array_equal(mask, want)
    r2.render_moments(cam2, 0, 1, DEPTH, seed=SEED)
    assert r2.unconverged(10.0, 10.0) == 35
    with pytest.raises(ptamd.PTError):
        r.unconverged(0.0, 0.0)
    with pytest.raises(ptamd.PTError):
        r.unconverged(-1.0, 1.0)


def boundaries(lo, hi, step):
    out = [lo]
    while out[-1] < hi:
        out.append(min(hi, out[-1] + step if step else 2 * out[-1]))
    return out


@pytest.mark.parametrize("step,pick", [(0, 3), (12, 5)])
def test_render_converge(renderers, yardstick, step, pick):
    r, sc, cam = renderers(GLOW)
    lo, hi, npix = 4, 256, 256
    bnd = boundaries(lo, hi, step)
    assert bnd[:3] == ([4, 8, 16] if step == 0 else [4, 16, 28]) and bnd[-1] == hi
    vals = yardstick(GLOW, hi)
    tied(yardstick, renderers, GLOW, hi)
    mom = {n: np_moments(vals[:n]) for n in bnd}
    # the tolerance: a little above the noisiest pixel's relative error at boundary `pick`
    S, Q, _ = mom[bnd[pick]]
    with np.errstate(all="ignore"):
        relerr = np.where(S != 0, np_sem(S, Q, bnd[pick]).astype(F64) / (np.abs(S) / bnd[pick]), 0.0)
    rel = float(F32(1.05 * relerr.max()))
    allowed = 3
    counts = [int(np_unconverged(mom[n][0], mom[n][1], n, rel, 0.0).sum()) for n in bnd]
    stop = next(k for k, c in enumerate(counts) if c <= allowed)
    assert 0 < stop < len(bnd) - 1, (counts, rel)  # the precondition: strictly inside (min, max)
    img, m, info = r.render_converge(cam, DEPTH, rel, min_samples=lo, max_samples=hi, step=step,
                                     max_unconverged=allowed, seed=SEED)
    assert (info["spp"], info["rounds"], info["unconverged"]) == (bnd[stop], stop + 1, counts[stop]), (info, counts)
    want_img, st = r.render(cam, info["spp"], DEPTH, seed=SEED)
    assert np.array_equal(bits(img), bits(want_img)) and np.array_equal(bits(img), bits(mom[bnd[stop]][2]))
    assert np.array_equal(bits(m["sum"]), bits(mom[bnd[stop]][0]))
    assert np.array_equal(bits(m["sumsq"]), bits(mom[bnd[stop]][1]))
    assert info["rays"] == st["rays"] and info["kernel_ms"] > 0


def test_render_converge_ends(renderers, yardstick):
    r, sc, cam = renderers(GLOW)
    lo, hi = 4, 256
    vals = yardstick(GLOW, hi)
    tied(yardstick, renderers, GLOW, hi)
    tiny = 1e-9
    counts = [int(np_unconverged(*np_moments(vals[:n])[:2], n, tiny, 0.0).sum()) for n in boundaries(lo, hi, 0)]
    assert min(counts) > 0  # a tolerance nothing meets
    img, m, info = r.render_converge(cam, DEPTH, tiny, min_samples=lo, max_samples=hi, seed=SEED)
    assert (info["spp"], info["rounds"], info["unconverged"]) == (hi, 7, counts[-1])
    S, Q, mean = np_moments(vals)
    assert np.array_equal(bits(img), bits(mean)) and np.array_equal(bits(m["sum"]), bits(S))
    # the sum stays valid: render_moments continues it
    import ptamd
    with pytest.raises(ptamd.PTError):
        r.render_moments(cam, hi - 1, 1, DEPTH, seed=SEED)
    r.render_converge(cam, DEPTH, tiny, min_samples=lo, max_samples=64, seed=SEED)
    img, m, _ = r.render_moments(cam, 64, 6, DEPTH, seed=SEED)
    S70, Q70, mean70 = np_moments(vals[:70])
    assert np.array_equal(bits(m["sum"]), bits(S70)) and np.array_equal(bits(m["sumsq"]), bits(Q70))
    assert np.array_equal(bits(img), bits(mean70))
    # every pixel allowed to miss: the first boundary ends the render
    img, m, info = r.render_converge(cam, DEPTH, tiny, min_samples=lo, max_samples=hi, max_unconverged=256, seed=SEED)
    assert (info["spp"], info["rounds"], info["unconverged"]) == (lo, 1, counts[0])
    assert np.array_equal(bits(img), bits(np_moments(vals[:lo])[2]))
    for bad in (dict(min_samples=1), dict(min_samples=8, max_samples=4), dict(step=-1)):
        with pytest.raises(ptamd.PTError):
            r.render_converge(cam, DEPTH, 0.1, **{**dict(min_samples=lo, max_samples=hi), **bad})
    with pytest.raises(ptamd.PTError):
        r.render_converge(cam, DEPTH, 0.0, 0.0)


def test_device_tensors(renderers, yardstick):
    import torch
    for name in (DARK, GLOW):
        r, sc, cam = renderers(name)
        n = 37
        S, Q, mean = tied(yardstick, renderers, name, n)
        dev = torch.device("cuda", 0)
        out = torch.empty((16, 16, 3), dtype=torch.float32, device=dev)
        r.render_moments(cam, 0, 20, DEPTH, seed=SEED, out=out)
        img, mom, _ = r.render_moments(cam, 20, 17, DEPTH, seed=SEED, out=out, batch_spp=5)
        assert img is out and all(v.is_cuda for v in mom.values())
        himg, hmom, _ = r.render_moments(cam, 0, n, DEPTH, seed=SEED)
        assert np.array_equal(bits(out.cpu().numpy()), bits(himg)) and np.array_equal(bits(himg), bits(mean))
        for k in ("sum", "sumsq", "sem"):
            assert np.array_equal(bits(mom[k].cpu().numpy()), bits(hmom[k])), (name, k)
        assert np.array_equal(bits(hmom["sum"]), bits(S)) and np.array_equal(bits(hmom["sumsq"]), bits(Q))
    r, sc, cam = renderers(GLOW)
    himg, hmom, hinfo = r.render_converge(cam, DEPTH, 0.2, min_samples=4, max_samples=64, seed=SEED)
    out = torch.zeros((16, 16, 3), dtype=torch.float32, device=dev)
    img, mom, info = r.render_converge(cam, DEPTH, 0.2, min_samples=4, max_samples=64, seed=SEED, out=out)
    assert {k: info[k] for k in ("spp", "rounds", "unconverged", "rays")} == \
           {k: hinfo[k] for k in ("spp", "rounds", "unconverged", "rays")}
    assert np.array_equal(bits(out.cpu().numpy()), bits(himg))
    for k in ("sum", "sumsq", "sem"):
        assert np.array_equal(bits(mom[k].cpu().numpy()), bits(hmom[k])), k
