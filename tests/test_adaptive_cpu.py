"""The host side of adaptive sampling (pt_ctx_render_adaptive, include/pt_hip.h): the new structs
and symbol, Renderer.render_adaptive's argument checks, and the numpy restatement of the policy
that tests/test_adaptive_gpu.py predicts with, run on synthetic moments against
ptamd.moments_unconverged. No device needed."""
import ctypes as C

import numpy as np
import pytest

import ptamd
from ptamd import _lib
from test_moments_cpu import np_unconverged

F32, F64 = np.float32, np.float64


def boundaries(lo, hi, step):
    """pt_ctx_render_converge's round ends: lo, then + step (step = 0: doubled), capped at hi."""
    out = [lo]
    while out[-1] < hi:
        out.append(min(hi, out[-1] + step if step else 2 * out[-1]))
    return out


def np_policy(moments_at, npix, lo, hi, step, rel, abs_, max_unconverged=0, sparse_below=1.0):
    """include/pt_hip.h's adaptive policy restated. moments_at(n) -> (S, Q), each (npix, 3) float64:
    every pixel's sums over its first n samples. Dense rounds evaluate every pixel; at the first
    boundary whose count is <= sparse_below * npix (and > max_unconverged, and not the last one)
    the unconverged pixels become the active list and the others freeze; then only the list is
    evaluated, with the round's n, and only shrinks. Returns a dict: spp (npix,) int32; rounds;
    dense_rounds; unconverged (the final count); evals: one (n, active indices or None = all,
    unconverged mask over them) per boundary; sparse: one (n_from, n_to, active indices) per
    per-pixel round."""
    bnd = boundaries(lo, hi, step)
    spp = np.zeros(npix, dtype=np.int32)
    evals, sparse, active = [], [], None
    below = F64(F32(sparse_below)) * F64(npix)
    k = 0
    while True:  # dense rounds
        n = bnd[k]
        S, Q = moments_at(n)
        un = np_unconverged(S, Q, n, rel, abs_).astype(bool)
        evals.append((n, None, un))
        count = int(un.sum())
        if count <= max_unconverged or n >= hi:
            spp[:] = n
            return dict(spp=spp, rounds=k + 1, dense_rounds=k + 1, unconverged=count, evals=evals, sparse=sparse)
        if sparse_below > 0 and F64(count) <= below:
            active = np.flatnonzero(un)
            spp[~un] = n
            break
        k += 1
    dense_rounds = k + 1
    while len(active) > max_unconverged and n < hi:  # per-pixel rounds
        k += 1
        sparse.append((n, bnd[k], active))
        n = bnd[k]
        S, Q = moments_at(n)
        un = np_unconverged(S[active], Q[active], n, rel, abs_).astype(bool)
        evals.append((n, active, un))
        spp[active[~un]] = n
        active = active[un]
    spp[active] = n
    return dict(spp=spp, rounds=k + 1, dense_rounds=dense_rounds, unconverged=len(active), evals=evals, sparse=sparse)


def test_structs_and_symbol():
    L = ptamd.lib()
    assert L.pt_abi_version() == 3
    assert hasattr(L, "pt_ctx_render_adaptive") and "pt_ctx_render_adaptive" in _lib.EXPORTED
    # pt_adaptive: pt_converge (32 bytes, 8-aligned) + float + padding; pt_adaptive_stats: 4 int32,
    # 2 int64, 2 uint64, 4 double
    assert C.sizeof(_lib.pt_adaptive) == 40 and _lib.pt_adaptive.sparse_below.offset == 32
    assert C.sizeof(_lib.pt_adaptive_stats) == 80
    assert [f for f, _ in _lib.pt_adaptive_stats._fields_] == \
        ["rounds", "dense_rounds", "max_spp", "sparse_launches", "unconverged", "samples", "rays", "sparse_rays",
         "kernel_ms", "reduce_ms", "total_ms", "sparse_kernel_ms"]
    assert _lib.pt_adaptive_stats.unconverged.offset == 16 and _lib.pt_adaptive_stats.kernel_ms.offset == 48


def test_python_argument_checks():
    """ValueError before the context is touched: this Renderer has none, so a library call on it
    would return PT_E_ARG (PTError) instead."""
    import torch
    from ptamd import scenes
    r = ptamd.Renderer.__new__(ptamd.Renderer)
    r.h, r._mom_pixels = None, 0
    cam = ptamd.Camera.from_spec(scenes.cornell((16, 16)).camera)
    with pytest.raises(ValueError):
        r.render_adaptive(cam, 5, 0.1, want=("sum", "variance"))
    for out in (torch.empty((16, 16, 3), dtype=torch.float64),   # dtype
                torch.empty((16, 15, 3), dtype=torch.float32),   # shape
                torch.empty((16, 16, 3), dtype=torch.float32),   # not on the context's device
                np.empty((16, 16, 3), dtype=np.float32)):        # not a tensor
        with pytest.raises(ValueError):
            r.render_adaptive(cam, 5, 0.1, out=out)
    with pytest.raises(ptamd.PTError):
        r.render_adaptive(cam, 5, 0.1)  # the checks passed: the library refuses the missing context


@pytest.mark.parametrize("step,sparse_below,allowed", [(0, 1.0, 0), (5, 1.0, 0), (0, 0.5, 0), (3, 0.3, 7), (0, -1.0, 0),
                                                       (0, 1.0, 40)])
def test_policy_on_integer_moments(step, sparse_below, allowed):
    """Integer-valued samples whose spread differs from pixel to pixel, so that pixels leave at
    different boundaries: the restated policy's evaluation at every boundary equals
    ptamd.moments_unconverged on the same pixels, the list only shrinks, and the bookkeeping adds up."""
    rng = np.random.default_rng(7)
    npix, lo, hi = 301, 4, 64
    spread = rng.integers(0, 6, size=npix)  # 0: a constant pixel, converged at once
    r = (20 + rng.integers(-1, 2, size=(hi, npix, 3)) * spread[None, :, None]).astype(F64)
    cs, cq = np.cumsum(r, axis=0), np.cumsum(r * r, axis=0)

    def moments_at(n):
        return cs[n - 1], cq[n - 1]

    rel = 0.03
    p = np_policy(moments_at, npix, lo, hi, step, rel, 0.0, allowed, sparse_below)
    bnd = boundaries(lo, hi, step)
    assert [e[0] for e in p["evals"]] == bnd[:p["rounds"]]
    last = None
    for n, active, un in p["evals"]:
        S, Q = moments_at(n)
        if active is not None:
            S, Q = S[active], Q[active]
            assert last is None or set(active) <= set(last)  # the list only shrinks
            last = active
        cnt, mask = ptamd.moments_unconverged(S, Q, n, rel, 0.0, mask=True)
        assert np.array_equal(mask.astype(bool), un) and cnt == int(un.sum()), n
    spp = p["spp"]
    assert set(np.unique(spp)) <= set(bnd) and spp.min() >= lo
    assert p["unconverged"] <= allowed or spp.max() == hi
    if sparse_below < 0:
        assert p["sparse"] == [] and len(np.unique(spp)) == 1 and p["rounds"] == p["dense_rounds"]
    else:
        assert p["rounds"] == p["dense_rounds"] + len(p["sparse"])
    if (step, sparse_below, allowed) == (0, 1.0, 0):
        assert len(np.unique(spp)) >= 3 and p["dense_rounds"] == 1  # pixels leave at several boundaries
    if sparse_below == 0.5:
        assert p["dense_rounds"] > 1 and p["sparse"]  # the switch is not on the first boundary
    # the pixel-samples rendered: dense rounds for all, per-pixel rounds for the listed
    n_dense = bnd[p["dense_rounds"] - 1]
    assert int(spp.sum()) == npix * n_dense + sum((b - a) * len(act) for a, b, act in p["sparse"])
