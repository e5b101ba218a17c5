// pt_raystack.h — loop control of the flat kernels' shared camera-ray stock (trace_body_flat,
// DESIGN.md §3.18), as plain integer functions for the device and the host (test hook
// pt_debug_ray_stack: tests/test_ray_stack_cpu.py runs them inside a lane-level model).
//
// A wave keeps up to kRaySlots prefetched camera rays: slot s is LDS row s of the wave
// (next_ray, next_at) plus lane s's next_inv registers. The stock is a stack: a wave-uniform
// `count` says slots [0, count) are filled, and any lane may take any slot. `dry` says the work
// pool gave out during a fill, after which the generator never runs again.
#pragma once

#if defined(__HIPCC__)
#define PT_RS_HD __host__ __device__ __forceinline__
#else
#define PT_RS_HD inline
#endif

namespace pt {

constexpr int kRaySlots = 64;  // one slot per lane (more would need LDS the block does not have)

// Whether the generator runs at the top of an iteration in which n_need lanes have no path: when
// the stock cannot serve them with `reserve` to spare, and there is a slot to fill. With no lane
// on a path n_need is kRaySlots, so this also covers "nothing else is left to do".
PT_RS_HD bool ray_stack_generate(int count, int n_need, int reserve, bool dry) {
    return !dry && count < kRaySlots && count < n_need + reserve;
}
// A fill: lanes count..kRaySlots-1 each ask the pool for an item, ranked in lane order, and n_got
// of them (a prefix) get one and fill their own slot: the filled slots stay [0, count).
PT_RS_HD int ray_stack_filled(int count, int n_got) { return count + n_got; }
PT_RS_HD bool ray_stack_dry(int count, int n_got) { return n_got < kRaySlots - count; }
// The slot the lane of rank `rank` among the lanes without a path takes; < 0: none is left for it.
PT_RS_HD int ray_stack_slot(int count, int rank) { return count - 1 - rank; }
// The count after the n_need lanes without a path took what there was (a subtract and a max on
// the scalar unit; the form count - min(n_need, count) compiled to a saturating vector subtract).
PT_RS_HD int ray_stack_taken(int count, int n_need) {
    const int left = count - n_need;
    return left > 0 ? left : 0;
}
// The wave is done: no lane on a path, no ray in stock, and no item left to make one from.
PT_RS_HD bool ray_stack_done(bool any_active, int count, bool dry) { return !any_active && count == 0 && dry; }

}  // namespace pt
