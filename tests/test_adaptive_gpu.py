"""Adaptive sampling on the GPU (pt_ctx_render_adaptive, Renderer.render_adaptive).

The yardstick, as in tests/test_moments_gpu.py: none of the code under test produces it. Sample s
of every pixel is Renderer.aov's camera ray traced by Renderer.trace from the LCG state after the
camera's two draws; S, Q and the float32 image follow from r[s] by numpy loops in sample order, and
the float32 mean is first tied to the CPU oracle's render bit for bit at every sample count used.
tests/test_adaptive_cpu.py's restatement of the policy then predicts the boundaries, the active
sets, the n_p map and, per pixel from r[:n_p], the image, S, Q and sem.

The tolerances below were chosen per scene on the yardstick so that the vacuity guard holds: the
predicted n_p map has at least three distinct values, each on at least 5 % of the pixels, and a
pixel that ends at max_samples. Cornell is dark: a pixel whose first min_samples samples are all
zero freezes there (the documented caveat), and at 8 or 11 samples fewer than 5 % of the pixels
are lit at all, so the dark cases start at 64 samples, where enough pixels have seen the light."""
import numpy as np
import pytest

import _oracle as O
import _reftrace as RT
import _treecases as TC
from test_adaptive_cpu import boundaries, np_policy
from test_moments_gpu import bits, np_sem

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DEPTH, SEED = 5, 3
DARK, GLOW, TREE = "cornell", "cornell+glow", "cornell/merged5"
MOST = 256

# (min_samples, max_samples, step, rel, abs): the yardstick's n_p histogram beside each
DOUBLING = dict(lo=8, hi=256, step=0, rel=0.02, abs_=0.03)   # 16x16: {8: 24, 16: 15, 32: 37, 64: 69, 128: 90, 256: 21}
STEPPED = dict(lo=11, hi=70, step=13, rel=0.08, abs_=0.02)   # 16x16: {11: 24, 24: 43, 37: 57, 50: 48, 63: 44, 70: 40}
DOUBLING_7x5 = dict(DOUBLING, rel=0.05, abs_=0.02)           # {8: 2, 16: 2, 32: 3, 64: 6, 128: 19, 256: 3}
DARK_CASE = dict(lo=64, hi=256, step=64, rel=0.2, abs_=0.01)  # {64: 177, 128: 26, 192: 26, 256: 27}
TREE_CASE = dict(lo=64, hi=256, step=64, rel=0.1, abs_=0.015)  # 7x5: {64: 21, 128: 5, 192: 6, 256: 3}
# every pixel misses the target at 6 samples and 242 of 256 at 70: with sparse_below = 0.95 the
# first boundary is dense for all and the switch falls on the second; {70: 14, 134: 59, 198: 50, 256: 133}
SECOND = dict(lo=6, hi=256, step=64, rel=0.08, abs_=0.0)


def scene_of(name, res):
    return TC.scene("cornell", res) if name == TREE else RT.make_scene(name, res)


@pytest.fixture(scope="module")
def renderers():
    """Two contexts per (scene, resolution), scene uploaded: [0] runs the code under test, [1] the
    plain renders compared against; closed at the end of the module."""
    import ptamd
    made = {}

    def get(name, res=(16, 16)):
        key = (name, tuple(res))
        if key not in made:
            sc = scene_of(name, res)
            bvh = TC.to_bvh(ptamd, TC.case("cornell", "merged5")) if name == TREE else ptamd.BVH.from_scene(sc)
            rr = []
            for _ in range(2):
                r = ptamd.Renderer(0)
                r.set_scene(bvh)
                rr.append(r)
            made[key] = (rr[0], rr[1], sc, ptamd.Camera.from_spec(sc.camera))
        return made[key]

    yield get
    for r, r2, _, _ in made.values():
        r.close()
        r2.close()


class Yard:
    """r[s] of a whole image, (MOST, npix, 3) float32, with the rays and LCG states it was traced
    from ([s][pixel]), and its running sums at the sample counts asked for."""

    def __init__(self, r, sc, cam, tree):
        W, H = sc.camera.res
        self.sc, self.npix, self.W, self.H, self.tree = sc, W * H, W, H, tree
        seeds = RT.sample_seeds(W * H, MOST, SEED)  # the pixel's global index h W + w
        rays = np.stack([r.aov(cam, sample=s, seed=SEED, channels=("ray",))[0]["ray"].reshape(-1, 6)
                         for s in range(MOST)])
        self.o = np.ascontiguousarray(rays[..., 0:3])
        self.d = np.ascontiguousarray(rays[..., 3:6])
        self.states = RT.lcg_step(seeds.T.reshape(-1), 2).reshape(MOST, W * H)
        rgb, _ = r.trace(self.o.reshape(-1, 3), self.d.reshape(-1, 3), DEPTH, states=self.states.reshape(-1, 1))
        self.vals = rgb.reshape(MOST, W * H, 3)
        S, Q, acc = np.zeros((W * H, 3), F64), np.zeros((W * H, 3), F64), np.zeros((W * H, 3), F32)
        self.S, self.Q, self.acc = [S], [Q], [acc]
        for s in range(MOST):
            v = self.vals[s].astype(F64)
            S, Q, acc = S + v, Q + v * v, acc + self.vals[s]
            self.S.append(S)
            self.Q.append(Q)
            self.acc.append(acc)
        self.tied = set()

    def at(self, n):
        return self.S[n], self.Q[n]

    def mean(self, n):
        """The float32 in-order mean of n samples, tied to the CPU oracle the first time it is asked for."""
        m = self.acc[n] / F32(n)
        if n not in self.tied:
            kw = {}
            if self.tree:
                c = TC.case("cornell", "merged5")
                kw = dict(nodes=np.ascontiguousarray(c.nodes), idx=np.ascontiguousarray(c.idx))
            ref, _ = O.render(self.sc, n, DEPTH, SEED, **kw)
            assert np.array_equal(bits(m), bits(ref.reshape(-1, 3))), f"n={n}: yardstick != oracle"
            self.tied.add(n)
        return m


@pytest.fixture(scope="module")
def yard(renderers):
    made = {}

    def get(name, res=(16, 16)):
        key = (name, tuple(res))
        if key not in made:
            r, r2, sc, cam = renderers(name, res)
            made[key] = Yard(r2, sc, cam, name == TREE)
        return made[key]

    return get


def guard(spp, hi, reach_max=True):
    """The vacuity guard, on the yardstick's prediction."""
    values, counts = np.unique(spp, return_counts=True)
    hist = dict(zip(values.tolist(), counts.tolist()))
    assert len(values) >= 3, hist
    assert all(c >= 0.05 * spp.size for c in counts), hist
    if reach_max:
        assert hist.get(hi, 0) >= 1, hist


def predict(y, lo, hi, step, rel, abs_, max_unconverged=0, sparse_below=1.0, pixels=None):
    """The policy on the yardstick (over `pixels` of the image, default all): the np_policy dict
    with the predicted per-pixel image, S, Q and sem added."""
    pix = np.arange(y.npix) if pixels is None else np.asarray(pixels)

    def moments_at(n):
        S, Q = y.at(n)
        return S[pix], Q[pix]

    p = np_policy(moments_at, len(pix), lo, hi, step, rel, abs_, max_unconverged, sparse_below)
    spp = p["spp"]
    img, S, Q = np.zeros((len(pix), 3), F32), np.zeros((len(pix), 3), F64), np.zeros((len(pix), 3), F64)
    sem = np.zeros((len(pix), 3), F32)
    for n in np.unique(spp).tolist():
        m = spp == n
        img[m] = y.mean(n)[pix][m]
        S[m], Q[m] = y.S[n][pix][m], y.Q[n][pix][m]
        sem[m] = np_sem(S[m], Q[m], n)
    p.update(img=img, S=S, Q=Q, sem=sem, pix=pix)
    return p


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def check(got, p, what=""):
    img, mom, spp, info = got
    n = len(p["pix"])
    assert np.array_equal(host(spp).reshape(-1), p["spp"]), what
    assert host(spp).dtype == np.int32
    assert np.array_equal(bits(host(img).reshape(n, 3)), bits(p["img"])), what
    assert np.array_equal(bits(host(mom["sum"]).reshape(n, 3)), bits(p["S"])), what
    assert np.array_equal(bits(host(mom["sumsq"]).reshape(n, 3)), bits(p["Q"])), what
    off = np.abs(bits(host(mom["sem"]).reshape(n, 3)).astype(np.int64) - bits(p["sem"]).astype(np.int64))
    assert off.max() <= 1, (what, int(off.max()))
    assert (info["rounds"], info["dense_rounds"], info["unconverged"]) == \
           (p["rounds"], p["dense_rounds"], p["unconverged"]), (what, info)
    assert info["samples"] == int(p["spp"].sum()) and info["max_spp"] == int(p["spp"].max()), (what, info)
    assert (info["sparse_launches"] > 0) == bool(p["sparse"]), (what, info)


def run(r, cam, cfg, **kw):
    return r.render_adaptive(cam, DEPTH, cfg["rel"], cfg["abs_"], min_samples=cfg["lo"], max_samples=cfg["hi"],
                             step=cfg["step"], seed=SEED, **{"sparse_below": 1.0, **kw})


def same(a, b, what=""):
    """Two results of render_adaptive (numpy or tensors) hold the same bits."""
    assert np.array_equal(host(a[2]), host(b[2])), what
    assert np.array_equal(bits(host(a[0])), bits(host(b[0]))), what
    for k in ("sum", "sumsq", "sem"):
        assert np.array_equal(bits(host(a[1][k])), bits(host(b[1][k]))), (what, k)


CASES = [(GLOW, (16, 16), DOUBLING), (GLOW, (16, 16), STEPPED), (GLOW, (7, 5), DOUBLING_7x5), (GLOW, (7, 5), STEPPED),
         (DARK, (16, 16), DARK_CASE), (TREE, (7, 5), TREE_CASE)]


@pytest.mark.parametrize("name,res,cfg", CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_policy_bit_exact(renderers, yard, name, res, cfg):
    """Per-pixel rounds from the first boundary on. Every distinct n of the spp map: a plain render
    at n on the second context agrees bit for bit on the pixels with spp == n. info's rays are the
    dense round's plus the per-pixel rounds', those cross-checked against Renderer.trace on the
    same rays. Afterwards the context holds no running moments sum."""
    import ptamd
    r, r2, sc, cam = renderers(name, res)
    y = yard(name, res)
    p = predict(y, **cfg)
    guard(p["spp"], cfg["hi"])
    assert r.flags()["dark"] == (name != GLOW)
    got = run(r, cam, cfg)
    check(got, p, f"{name} {res}")
    img, mom, spp, info = got
    if name != GLOW:  # the caveat: the pixels that are all zero at min_samples froze there, the lit ones ran on
        zero = (y.S[cfg["lo"]] == 0).all(axis=-1)
        assert zero.sum() > 0 and (spp.reshape(-1)[zero] == cfg["lo"]).all() and (spp.reshape(-1)[~zero] > cfg["lo"]).any()
    dense_rays = None
    for n in np.unique(spp).tolist():
        want, st = r2.render(cam, n, DEPTH, seed=SEED)
        m = spp == n
        assert np.array_equal(bits(img[m]), bits(want[m])), (name, n)
        if n == cfg["lo"]:
            dense_rays = st["rays"]
    if dense_rays is None:
        dense_rays = r2.render(cam, cfg["lo"], DEPTH, seed=SEED)[1]["rays"]
    sparse_rays = 0
    for n0, n1, active in p["sparse"]:
        o, d, st = y.o[n0:n1, active], y.d[n0:n1, active], y.states[n0:n1, active]
        _, tst = r2.trace(o.reshape(-1, 3), d.reshape(-1, 3), DEPTH, states=st.reshape(-1, 1))
        sparse_rays += tst["rays"]
    assert info["sparse_rays"] == sparse_rays and info["rays"] == dense_rays + sparse_rays, info
    assert info["kernel_ms"] > 0 and info["sparse_launches"] == len(p["sparse"])
    with pytest.raises(ptamd.PTError):
        r.unconverged(cfg["rel"], cfg["abs_"])
    with pytest.raises(ptamd.PTError):
        r.render_moments(cam, int(spp.max()), 1, DEPTH, seed=SEED)


def test_never_sparse_is_render_converge(renderers, yard):
    r, r2, sc, cam = renderers(GLOW)
    y = yard(GLOW)
    cfg = dict(DOUBLING, hi=64)
    p = predict(y, **cfg, sparse_below=-1.0)
    assert len(np.unique(p["spp"])) == 1 and p["spp"][0] == 64 and p["unconverged"] > 0 and not p["sparse"]
    cimg, cmom, cinfo = r2.render_converge(cam, DEPTH, cfg["rel"], cfg["abs_"], min_samples=8, max_samples=64, seed=SEED)
    got = run(r, cam, cfg, sparse_below=-1.0)
    check(got, p)
    img, mom, spp, info = got
    assert np.array_equal(bits(img), bits(cimg)) and (spp == cinfo["spp"]).all()
    for k in ("sum", "sumsq", "sem"):
        assert np.array_equal(bits(mom[k]), bits(cmom[k])), k
    assert (info["rounds"], info["unconverged"], info["rays"]) == (cinfo["rounds"], cinfo["unconverged"], cinfo["rays"])
    assert info["sparse_launches"] == 0 and info["sparse_rays"] == 0
    # the sum stays a running moments sum
    assert r.unconverged(cfg["rel"], cfg["abs_"]) == p["unconverged"]
    img70, mom70, _ = r.render_moments(cam, 64, 6, DEPTH, seed=SEED)
    assert np.array_equal(bits(mom70["sum"].reshape(-1, 3)), bits(y.S[70]))
    assert np.array_equal(bits(img70.reshape(-1, 3)), bits(y.mean(70)))


def test_switch_on_second_boundary(renderers, yard):
    """Every pixel misses the target at the first boundary, so per-pixel rounds from the first
    boundary (sparse_below = 1) and a dense second round (0.95) sample the same pixels."""
    r, r2, sc, cam = renderers(GLOW)
    y = yard(GLOW)
    first = predict(y, **SECOND)
    guard(first["spp"], SECOND["hi"])
    p = predict(y, **SECOND, sparse_below=0.95)
    assert (first["dense_rounds"], p["dense_rounds"]) == (1, 2) and p["sparse"]
    assert np.array_equal(first["spp"], p["spp"])
    a = run(r, cam, SECOND, sparse_below=0.95)
    check(a, p)
    assert a[3]["dense_rounds"] == 2  # dense rounds really ran
    b = run(r, cam, SECOND)
    check(b, first)
    same(a, b)
    assert a[3]["sparse_rays"] < b[3]["sparse_rays"] and a[3]["samples"] == b[3]["samples"]


def test_max_unconverged_stops_early(renderers, yard):
    """The stop leaves the listed pixels at a boundary below max_samples, so the guard's third
    condition is replaced by: the render stopped early with exactly the predicted pixels left."""
    r, r2, sc, cam = renderers(GLOW)
    y = yard(GLOW)
    p = predict(y, **DOUBLING, max_unconverged=30)
    guard(p["spp"], DOUBLING["hi"], reach_max=False)
    assert p["spp"].max() == 128 and p["unconverged"] == 21 and p["rounds"] == 5
    left = np_policy(y.at, y.npix, 8, 128, 0, DOUBLING["rel"], DOUBLING["abs_"])["evals"][-1]
    assert int(left[2].sum()) == 21  # the pixels still unconverged at 128
    got = run(r, cam, DOUBLING, max_unconverged=30)
    check(got, p)
    assert (got[2].reshape(-1)[left[1][left[2]]] == 128).all()


def test_list_runs_down_to_one_and_to_zero(renderers, yard):
    r, r2, sc, cam = renderers(GLOW)
    y = yard(GLOW)
    one = dict(DOUBLING, rel=0.08, abs_=0.01)
    p = predict(y, **one)
    assert p["unconverged"] == 1 and len(p["sparse"]) == 5 and len(p["sparse"][-1][2]) > 1
    check(run(r, cam, one), p, "one")
    zero = dict(DOUBLING, rel=0.1, abs_=0.02)  # the list empties at 128, before max_samples
    p = predict(y, **zero)
    assert p["unconverged"] == 0 and p["spp"].max() == 128 and len(p["sparse"]) == 4
    check(run(r, cam, zero), p, "zero")
    easy = dict(DOUBLING, rel=10.0, abs_=10.0)  # met by every pixel at the first boundary: no list at all
    p = predict(y, **easy)
    assert p["unconverged"] == 0 and p["rounds"] == 1 and not p["sparse"]
    got = run(r, cam, easy)
    check(got, p, "easy")
    assert got[3]["sparse_launches"] == 0 and got[3]["sparse_rays"] == 0 and (got[2] == 8).all()
    assert r.unconverged(10.0, 10.0) == 0  # no per-pixel round ran: the moments sum stays


def launches_of(p, chunk):
    """The cut of a round of m listed pixels x c samples into launches of at most `chunk` items:
    over samples first, then over listed pixels."""
    out = []
    for n0, n1, active in p["sparse"]:
        m, c = len(active), n1 - n0
        m_l = min(m, chunk)
        c_l = min(c, max(1, chunk // m_l))
        out.append(-(-m // m_l) * -(-c // c_l))
    return out


def test_launch_cuts(renderers, yard, monkeypatch):
    r, r2, sc, cam = renderers(GLOW)
    y = yard(GLOW)
    p = predict(y, **STEPPED)
    guard(p["spp"], STEPPED["hi"])
    whole = run(r, cam, STEPPED)
    check(whole, p)
    m1 = len(p["sparse"][0][2])
    for chunk in (3 * m1, 100):  # 13 samples cut into 3+3+3+3+1; then pixels cut as well, one sample each
        cuts = launches_of(p, chunk)
        assert cuts[0] == (5 if chunk == 3 * m1 else 39), cuts
        monkeypatch.setenv("PT_ADAPTIVE_CHUNK", str(chunk))
        got = run(r, cam, STEPPED)
        monkeypatch.delenv("PT_ADAPTIVE_CHUNK")
        check(got, p, chunk)
        same(got, whole, chunk)
        assert got[3]["sparse_launches"] == sum(cuts) and got[3]["sparse_rays"] == whole[3]["sparse_rays"]


@pytest.mark.parametrize("hook", ["PT_QUERY_LDS_STACK=0", "PT_TRACE_LDS_REC=0", "PT_FORCE_EXACT_SLAB=1"])
def test_placement_hooks(renderers, yard, monkeypatch, hook):
    r, r2, sc, cam = renderers(GLOW, (7, 5))
    y = yard(GLOW, (7, 5))
    p = predict(y, **STEPPED)
    guard(p["spp"], STEPPED["hi"])
    k, v = hook.split("=")
    monkeypatch.setenv(k, v)
    got = run(r, cam, STEPPED)
    monkeypatch.delenv(k)
    check(got, p, hook)


def test_partition_rows(renderers, yard):
    """Part 1 of 2 with band_rows = 1: the odd rows. Seeding by the global pixel index makes them
    the whole-image run's rows (with sparse_below = 1 and max_unconverged = 0 a pixel's n_p
    depends on that pixel alone)."""
    r, r2, sc, cam = renderers(GLOW)
    y = yard(GLOW)
    rows = list(range(1, 16, 2))
    pix = np.concatenate([np.arange(16 * h, 16 * h + 16) for h in rows])
    p = predict(y, **STEPPED, pixels=pix)  # {11: 11, 24: 22, 37: 31, 50: 24, 63: 20, 70: 20}
    guard(p["spp"], STEPPED["hi"])
    got = run(r, cam, STEPPED, part_index=1, part_count=2, band_rows=1)
    assert got[0].shape == (8, 16, 3) and got[2].shape == (8, 16)
    check(got, p)
    whole = run(r, cam, STEPPED)
    assert np.array_equal(got[2], whole[2][rows]) and np.array_equal(bits(got[0]), bits(whole[0][rows]))
    assert np.array_equal(bits(got[1]["sum"]), bits(whole[1]["sum"][rows]))


def test_device_tensors(renderers, yard):
    import torch
    for name, cfg in ((GLOW, STEPPED), (DARK, DARK_CASE)):
        r, r2, sc, cam = renderers(name)
        y = yard(name)
        p = predict(y, **cfg)
        guard(p["spp"], cfg["hi"])
        out = torch.zeros((16, 16, 3), dtype=torch.float32, device=torch.device("cuda", 0))
        got = run(r, cam, cfg, out=out)
        img, mom, spp, info = got
        assert img is out and spp.is_cuda and spp.dtype == torch.int32 and all(v.is_cuda for v in mom.values())
        assert mom["sum"].dtype == torch.float64 and mom["sem"].dtype == torch.float32
        check(got, p, name)
        same(got, run(r, cam, cfg), name)
