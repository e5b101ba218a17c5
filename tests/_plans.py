"""The host's launch rules restated for the tests: where the binary walk keeps its stack, scene and
records (pt_launch: place_walk), and how a launch sizes its grid and work pool (pool_sizing).
Defaults only: no tuning hook is modelled except where a parameter says so."""

K_BLOCK, K_WAVE, K_CHUNK = 256, 64, 1024
WAVES_PER_BLOCK = K_BLOCK // K_WAVE


def _planned(info, ntris, depth, scene_budget=32 * 1024, stack=True, rec=True, lds_usable=161280, tri_f4=5):
    """The binary walk's placement rule: stack rows, then the scene (tri_f4 float4 per triangle:
    5 with materials, 3 for queries), then the records go to LDS while they fit
    min(64 KiB, lds_usable / 2) in 256-byte granules."""
    cap = min(64 * 1024, lds_usable // 2)
    rnd = lambda b: -(-b // 256) * 256  # noqa: E731
    stack_b = 4 * 256 * max(1, info["tree_depth"])
    scene_b = 16 * (2 * info["nodes"] + tri_f4 * ntris)
    rec_b = 8 * 256 * (depth - 1)
    lds_stack = stack and rnd(stack_b) <= cap
    used = stack_b if lds_stack else 0
    lds_scene = scene_b <= scene_budget and rnd(scene_b + used) <= cap
    used += scene_b if lds_scene else 0
    lds_rec = rec and rnd(used + rec_b) <= cap
    return {"lds_scene": int(lds_scene), "lds_stack": int(lds_stack), "lds_records": int(lds_rec)}


def launch_samples(s_lo, spp, batch, tail):
    """Samples of each trace launch of a render of samples [s_lo, spp): full batches, and with a
    tail (fused accumulation, PT_TAIL_DIV) the last two launches are (left - tail, tail)."""
    out, s0 = [], s_lo
    while s0 < spp:
        left = spp - s0
        if tail <= 0 or left <= tail:
            sc = min(batch, left)
        else:
            sc = left - tail if left <= batch + tail else batch
        out.append(sc)
        s0 += sc
    return out


def pool(total_items, blocks_per_cu, num_cus, floor_items, acc_npix=0):
    """Grid and work pool of one launch of total_items work items: the refill size aims at 128
    refills per wave between floor_items (512 flat, 128 otherwise) and K_CHUNK; each wave starts
    with one refill's worth, or with its whole even share when that is under 4 K_CHUNK items.
    acc_npix > 0: the launch also sums the previous slab of acc_npix pixels (acc_every)."""
    grid = min(-(-total_items // K_BLOCK), blocks_per_cu * num_cus)
    waves = grid * WAVES_PER_BLOCK
    chunk = max(K_WAVE, min(K_CHUNK, max(min(K_CHUNK, floor_items), total_items // (waves * 128))))
    share = total_items // waves
    static_items = min(chunk, share)
    if share < 4 * K_CHUNK:
        static_items = max(static_items, share)
    acc_every = 0
    if acc_npix > 0:
        refills = max(1, (total_items - waves * static_items) // chunk)
        acc_every = max(1, refills // (2 * -(-acc_npix // K_WAVE)))
    return {"grid": grid, "chunk": chunk, "static_items": static_items, "acc_every": acc_every}
