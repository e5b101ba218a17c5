"""The loop control of the flat kernels' shared camera-ray stock (pt_raystack.h)
inside a lane-level model of trace_body_flat's loop, no GPU needed.

Every decision the kernel takes from the header (when to generate, the fill, which slot a rank
takes, the new count, the exit test) is taken here through the test hook pt_debug_ray_stack; the
model supplies what the kernel supplies: 64 lanes with path lengths, and claim_item's work pool
(items handed out in rank order from a wave-private range that is refilled by chunks of a head
several waves share, so that a fill can find the pool dry part-way)."""
import numpy as np
import pytest

LANES = 64


@pytest.fixture(scope="module")
def ctl():
    import ptamd
    f = ptamd.lib().pt_debug_ray_stack

    class Ctl:
        generate = staticmethod(lambda count, n_need, reserve, dry: bool(f(0, count, n_need, reserve, int(dry))))
        filled = staticmethod(lambda count, n_got: f(1, count, n_got, 0, 0))
        dry = staticmethod(lambda count, n_got: bool(f(2, count, n_got, 0, 0)))
        slot = staticmethod(lambda count, rank: f(3, count, rank, 0, 0))
        taken = staticmethod(lambda count, n_need: f(4, count, n_need, 0, 0))
        done = staticmethod(lambda any_active, count, dry: bool(f(5, count, int(dry), 0, int(any_active))))
    return Ctl


class Pool:
    """claim_item's pool for the waves of one launch: a shared head advanced by `chunk`."""

    def __init__(self, total, chunk):
        self.total, self.chunk, self.head = total, chunk, 0

    def claim(self, wave, cnt):
        """The items of ranks 0..cnt-1 (rank order); an item >= total is not handed out."""
        avail = wave["end"] - wave["next"]
        if avail < cnt:
            fresh = self.head
            self.head += self.chunk
            items = [wave["next"] + r if r < avail else fresh + (r - avail) for r in range(cnt)]
            wave["next"], wave["end"] = fresh + (cnt - avail), fresh + self.chunk
        else:
            items = [wave["next"] + r for r in range(cnt)]
            wave["next"] += cnt
        return [i for i in items if i < self.total], len(items)


def run(ctl, total, lengths, reserve, chunk=64, waves=1, max_iters=10_000_000):
    """All waves of a launch, one iteration each in turn. `lengths(n)` -> n path lengths >= 1.
    Returns (items traced in order, per-wave figures); asserts the invariants on the way."""
    pool = Pool(total, chunk)
    W = [dict(next=0, end=0, rem=np.zeros(LANES, int), slots=[None] * LANES, count=0, dry=False, done=False,
              iters=0, runs=0, gen_lanes=0, tracing=0) for _ in range(waves)]
    traced = []
    for _ in range(max_iters):
        if all(w["done"] for w in W):
            break
        for w in W:
            if w["done"]:
                continue
            active = w["rem"] > 0
            need = np.flatnonzero(~active)  # lane order = rank order (ballot + mbcnt)
            n_need = len(need)
            if ctl.generate(w["count"], n_need, reserve, w["dry"]):
                gen = list(range(w["count"], LANES))  # lanes count..63, each filling its own slot
                got, asked = pool.claim(w, len(gen))
                assert asked == len(gen)
                for lane, item in zip(gen, got):  # claim_item ranks them in lane order
                    assert w["slots"][lane] is None
                    w["slots"][lane] = item
                w["dry"] = ctl.dry(w["count"], len(got))
                assert w["dry"] == (len(got) < len(gen))
                w["count"] = ctl.filled(w["count"], len(got))
                w["runs"] += 1
                w["gen_lanes"] += len(got)
            # filled slots are always a prefix
            assert all((s is not None) == (i < w["count"]) for i, s in enumerate(w["slots"])), (w["count"], w["slots"])
            if n_need > 0 and w["count"] > 0:
                for rank, lane in enumerate(need):
                    s = ctl.slot(w["count"], rank)
                    if s >= 0:
                        assert s < w["count"] and w["slots"][s] is not None
                        traced.append(w["slots"][s])
                        w["slots"][s] = None
                        w["rem"][lane] = lengths(1)[0]
                w["count"] = ctl.taken(w["count"], n_need)
            active = w["rem"] > 0
            # no lane is left without a path while the stock holds a ray
            assert active.all() or w["count"] == 0
            assert all((s is not None) == (i < w["count"]) for i, s in enumerate(w["slots"]))
            if ctl.done(bool(active.any()), w["count"], w["dry"]):
                w["done"] = True
                continue
            assert active.any(), "the kernel's body needs a lane on a path once the exit test has failed"
            w["iters"] += 1
            w["tracing"] += int(active.sum())
            w["rem"][active] -= 1
    assert all(w["done"] for w in W), "the loop did not terminate"
    return traced, W


def _lengths(rng, lo, hi):
    return lambda n: rng.integers(lo, hi + 1, n)


@pytest.mark.parametrize("reserve", [0, 8, 64])
@pytest.mark.parametrize("total", [0, 1, 63, 64, 65, 64 * 1024 + 1])
def test_every_item_traced_once(ctl, total, reserve):
    """One wave; random path lengths 1..8, all 1 and all 8. (The large total only with random lengths
    and all 1: the others add nothing but time.)"""
    rng = np.random.default_rng(total * 131 + reserve)
    kinds = [_lengths(rng, 1, 8), _lengths(rng, 1, 1)] + ([_lengths(rng, 8, 8)] if total <= 65 else [])
    for lengths in kinds:
        traced, W = run(ctl, total, lengths, reserve, chunk=1024)
        assert sorted(traced) == list(range(total))
        assert W[0]["gen_lanes"] == total


@pytest.mark.parametrize("reserve", [0, 8, 64])
@pytest.mark.parametrize("chunk,waves,total", [(64, 3, 1000), (64, 4, 64 * 7 + 5), (128, 2, 128 * 3 + 70), (512, 5, 4097),
                                               (64, 2, 1), (64, 3, 65)])
def test_pool_runs_dry_mid_fill(ctl, chunk, waves, total, reserve):
    """Several waves on one head: a wave's fill gets a chunk whose tail lies past the last item, or
    no valid item at all; the filled slots stay a prefix and every item is traced exactly once."""
    rng = np.random.default_rng(chunk + waves + total + reserve)
    for lengths in (_lengths(rng, 1, 8), _lengths(rng, 1, 1), _lengths(rng, 8, 8)):
        traced, W = run(ctl, total, lengths, reserve, chunk=chunk, waves=waves)
        assert sorted(traced) == list(range(total))
        assert sum(w["gen_lanes"] for w in W) == total
        assert all(w["dry"] and w["count"] == 0 for w in W)


def test_reserve_0_gives_the_models_figures(ctl):
    """Path lengths 1..5 with mean 3.14 (the headline's traced iterations per path, an assumed
    distribution): the shared stock with reserve 0 runs the generator in 0.361 of the iterations with
    56.4 lanes and keeps all 64 lanes tracing (DESIGN.md §3.18's table). Bounds: the figures are
    means over ~10^4 iterations of a process with a ~3-iteration correlation; +-0.01 and +-1 lane
    are several standard errors. The tail (the last fills, the pool dry) is left in: it is < 0.1 %."""
    rng = np.random.default_rng(1)
    p = np.array([.08, .17, .30, .43, .02])
    lengths = lambda n: rng.choice(np.arange(1, 6), size=n, p=p)
    total = 200_000
    traced, W = run(ctl, total, lengths, 0, chunk=1024)
    assert len(traced) == total
    w = W[0]
    runs, lanes, tracing = w["runs"] / w["iters"], w["gen_lanes"] / w["runs"], w["tracing"] / w["iters"]
    print(f"reserve 0: {runs:.3f} generator runs per iteration, {lanes:.1f} lanes per run, {tracing:.2f} lanes tracing")
    assert abs(runs - 0.361) <= 0.01
    assert abs(lanes - 56.4) <= 1.0
    assert tracing >= 63.9


def test_decisions_at_the_edges(ctl):
    assert ctl.generate(0, 64, 0, False) and not ctl.generate(0, 64, 0, True)
    assert not ctl.generate(64, 64, 64, False)  # no slot to fill
    assert not ctl.generate(5, 5, 0, False) and ctl.generate(5, 6, 0, False) and ctl.generate(5, 0, 8, False)
    assert ctl.generate(63, 0, 64, False)
    assert ctl.slot(3, 0) == 2 and ctl.slot(3, 2) == 0 and ctl.slot(3, 3) < 0
    assert ctl.taken(3, 5) == 0 and ctl.taken(5, 3) == 2 and ctl.taken(0, 64) == 0
    assert ctl.dry(10, 53) and not ctl.dry(10, 54) and ctl.filled(10, 54) == 64
    assert ctl.done(False, 0, True) and not ctl.done(True, 0, True) and not ctl.done(False, 1, True)
    assert not ctl.done(False, 0, False)
