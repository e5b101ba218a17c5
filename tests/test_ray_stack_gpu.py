"""The shared camera-ray stock of the flat kernels on the GPU: any lane of a wave
takes any prefetched camera ray, so which lane traces which sample changes, and nothing else may:
float32 bits AND ray counts against the CPU oracle on every flat kernel path (the hipRTC scene
kernel, the table kernel with the scene's flags, the generic table kernel), at sizes where the first
fill is partial, the pool runs dry at once, or one item is left for a second wave, and under the
hooks that change the loop around it."""
import functools

import numpy as np
import pytest

import _oracle as O
import _refwalk as RW

pytestmark = pytest.mark.gpu

# hooks -> the kernel path (test_last_ray.py selects them the same way)
PATHS = {"rtc": ({}, (3,)), "table_fast": ({"PT_RTC": "0"}, (5,)), "table": ({"PT_RTC": "0", "PT_FLAT_FAST": "0"}, (2,))}
FLAT = (2, 3, 5)


@pytest.fixture(scope="module")
def gpu():
    import ptamd
    if ptamd.lib().pt_device_count() <= 0:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    return ptamd


def _scene(kind, res):
    from ptamd import scenes
    if kind == "cornell":
        return scenes.cornell(tuple(res))
    if kind == "mcornell_r0.3":
        return scenes.modified_cornell(0.3, tuple(res))
    return RW.make_scene(kind, tuple(res))


@functools.lru_cache(maxsize=None)
def _oracle(kind, res, spp, depth):
    img, rays = O.render(_scene(kind, res), spp, depth)
    img.setflags(write=False)
    return img, rays


@functools.lru_cache(maxsize=None)
def _oracle_rows(kind, res, spp, depth, rows):
    return sum(O.render(_scene(kind, res), spp, depth, rows=(h, h + 1))[1] for h in rows)


def _same(img, ref):
    a, b = np.ascontiguousarray(img).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32)
    return bool(((a == b) | (np.isnan(img) & np.isnan(ref))).all())  # a NaN's payload is not part of the contract


class _Ctx:
    """A Renderer on `kind` at `res` created under the hooks of `path` plus `env`."""

    def __init__(self, gpu, monkeypatch, kind, res, path, env=None):
        self.gpu, self.mp, self.kind, self.res = gpu, monkeypatch, kind, tuple(res)
        self.env = {"PT_RTC_WAIT": "1", **PATHS[path][0], **(env or {})}
        self.want = PATHS[path][1]

    def __enter__(self):
        self.ctx = self.mp.context()
        mp = self.ctx.__enter__()
        for k, v in self.env.items():
            mp.setenv(k, v)
        sc = _scene(self.kind, self.res)
        self.cam = self.gpu.Camera.from_spec(sc.camera)
        self.r = self.gpu.Renderer(0)
        self.r.set_scene(self.gpu.BVH.from_scene(sc))
        return self

    def __exit__(self, *exc):
        self.r.close()
        return self.ctx.__exit__(*exc)


def _check(gpu, monkeypatch, kind, res, spp, depth, path, env=None, want=None):
    ref, rays = _oracle(kind, tuple(res), spp, depth)
    with _Ctx(gpu, monkeypatch, kind, res, path, env) as c:
        img, st = c.r.render(c.cam, spp, depth)
    tag = (kind, res, spp, depth, path, env)
    print(f"{tag}: kernel_path {st['kernel_path']}, rays {st['rays']} (oracle {rays})")
    assert st["kernel_path"] in (want or c.want), tag
    assert _same(img, ref), tag
    assert st["rays"] == rays, tag


@pytest.mark.parametrize("path", list(PATHS))
def test_cornell_sizes(gpu, monkeypatch, path):
    """546 pixels at 3 spp (not a multiple of 64); 15 items (fewer than one wave: the first fill is
    partial and the pool is dry at once); 65 items (one wave's worth and one more)."""
    _check(gpu, monkeypatch, "cornell", (26, 21), 3, 5, path)
    _check(gpu, monkeypatch, "cornell", (5, 3), 1, 5, path)
    _check(gpu, monkeypatch, "cornell", (13, 5), 1, 5, path)


@pytest.mark.parametrize("path", list(PATHS))
def test_cornell_depths(gpu, monkeypatch, path):
    """Depth 0 (no ray at all: every path ends in the iteration it starts), 1, 2 and 8."""
    for depth in (0, 1, 2, 8):
        _check(gpu, monkeypatch, "cornell", (26, 21), 3, depth, path)


@pytest.mark.parametrize("path", list(PATHS))
def test_specular_room(gpu, monkeypatch, path):
    """A scene with a SPECULAR material keeps the per-lane form by default: also with the stock
    forced on (and off)."""
    for env in ({}, {"PT_RAY_STACK": "1"}, {"PT_RAY_STACK": "0"}):
        _check(gpu, monkeypatch, "mcornell_r0.3", (32, 32), 4, 5, path, env)


@pytest.mark.parametrize("path", list(PATHS))
def test_random_scene(gpu, monkeypatch, path):
    """random_2_40 need not pass the gates of the table kernel with baked-in flags: any flat path."""
    _check(gpu, monkeypatch, "random_2_40", (26, 21), 3, 5, path, want=FLAT)


HOOKS = [{"PT_RAY_RESERVE": "0"}, {"PT_RAY_RESERVE": "8"}, {"PT_RAY_RESERVE": "64"}, {"PT_RAY_STACK": "0"},
         {"PT_REGEN_THRESH": "1"}, {"PT_REGEN_THRESH": "64"}, {"PT_RAY_STACK": "0", "PT_REGEN_THRESH": "1"},
         {"PT_RAY_STACK": "0", "PT_REGEN_THRESH": "64"}, {"PT_PAIR_QUEUE": "16"}, {"PT_PAIRS": "0"},
         {"PT_FORCE_EXACT_SLAB": "2"}]


@pytest.mark.parametrize("hook", HOOKS, ids=lambda h: ",".join(f"{k}={v}" for k, v in h.items()))
def test_hooks_on_every_flat_path(gpu, monkeypatch, hook):
    """The reserve, the per-lane form (with the threshold it reads), a 16-entry pair queue, no pair
    queue, and waves on the exact walk beside waves on the fast path."""
    for path in PATHS:
        _check(gpu, monkeypatch, "cornell", (26, 21), 3, 5, path, hook)


@pytest.mark.parametrize("path", list(PATHS))
def test_launch_shapes(gpu, monkeypatch, path):
    """Three launches with fused accumulation (a wave's exit drains the previous slab's sums), one
    part of three with 1-row bands, and a progressive render of two calls."""
    kind, res, spp, depth = "cornell", (26, 21), 3, 5
    ref, rays = _oracle(kind, res, spp, depth)
    with _Ctx(gpu, monkeypatch, kind, res, path) as c:
        img, st = c.r.render(c.cam, spp, depth, batch_spp=1)
        plan = c.r.plan()
        assert st["trace_launches"] == 3 and plan["fused"] == 1, (path, st, plan)
        assert st["kernel_path"] in c.want and _same(img, ref) and st["rays"] == rays, path

        rows = tuple(h for h in range(res[1]) if h % 3 == 1)
        img, st = c.r.render(c.cam, spp, depth, part_index=1, part_count=3, band_rows=1)
        assert img.shape[0] == len(rows) and _same(img, ref[list(rows)]), path
        assert st["rays"] == _oracle_rows(kind, res, spp, depth, rows), path

        _, rays2 = _oracle(kind, res, 2, depth)
        _, st_a = c.r.render_progressive(c.cam, 0, 2, depth)
        img, st_b = c.r.render_progressive(c.cam, 2, 1, depth)
        assert _same(img, ref), path
        assert st_a["rays"] == rays2 and st_a["rays"] + st_b["rays"] == rays, (path, st_a["rays"], st_b["rays"], rays)
