// pt_flatlds.h — the dynamic LDS of a flat-kernel block (trace_body_flat) as one
// plain function for the device and the host: the kernel forms its array bases from it, the host
// sizes the launch with it (flat_lds_bytes, plan_flat), and the test hook pt_debug_flat_lds
// returns it (tests/test_kconst_cpu.py).
//
// The arrays whose size the scene fixes come first, so their byte offsets are constants of a
// kernel that knows the scene (the hipRTC scene kernel); the two a launch sizes — the pair queues
// (pair_queue, chosen from the LDS fit) and the path records (rec_size = depth - 1) — come last:
//   [triangles: num_tri4 float4] [materials: num_mat4 float4] [camera rows: kBlock float4]
//   [winners: kBlock u64] [camera items: kBlock u32] [box table: box_tab_bytes]
//   [pair queues: waves x pair_queue u16] [record triangles: rec_size x kBlock u16]
//   [record cosines: rec_size x kBlock float]
// Alignment: float4 arrays 16 B, the winners 8 B, the queues and the records after them 8 B
// (pair_queue is a multiple of 4 and the fixed part is rounded up to 8 B).
#pragma once

#if defined(__HIPCC__)
#define PT_FL_HD __host__ __device__ __forceinline__
#else
#define PT_FL_HD inline
#endif

namespace pt {

constexpr unsigned kFlatLdsBlock = 256, kFlatLdsWaves = 4;  // kBlock, kBlock / kWave (pt_trace.h asserts both)

struct FlatLds {
    unsigned tris, mats, next_ray, best, next_at, boxtab;  // scene-fixed byte offsets
    unsigned queues, rec_tri, rec_cos;                     // these move with pair_queue and rec_size
    unsigned bytes;                                        // the block's dynamic LDS
};

// The box-level pairs' table: one uint16 per distinct box, padded to 4 B.
PT_FL_HD constexpr unsigned flat_box_tab_bytes(unsigned boxes) { return (2u * boxes + 3u) & ~3u; }

// The scene-fixed part alone: the offset at which the queues begin.
PT_FL_HD constexpr unsigned flat_lds_fixed(unsigned num_tri4, unsigned num_mat4, unsigned box_tab_bytes) {
    return (16u * (num_tri4 + num_mat4) + (16u + 8u + 4u) * kFlatLdsBlock + box_tab_bytes + 7u) & ~7u;
}

PT_FL_HD constexpr FlatLds flat_lds_layout(unsigned num_tri4, unsigned num_mat4, unsigned box_tab_bytes, unsigned pair_queue,
                                           unsigned rec_size) {
    FlatLds l{};
    l.tris = 0u;
    l.mats = 16u * num_tri4;
    l.next_ray = l.mats + 16u * num_mat4;
    l.best = l.next_ray + 16u * kFlatLdsBlock;
    l.next_at = l.best + 8u * kFlatLdsBlock;
    l.boxtab = l.next_at + 4u * kFlatLdsBlock;
    l.queues = flat_lds_fixed(num_tri4, num_mat4, box_tab_bytes);
    l.rec_tri = l.queues + 2u * kFlatLdsWaves * pair_queue;
    l.rec_cos = l.rec_tri + 2u * kFlatLdsBlock * rec_size;
    l.bytes = l.rec_cos + 4u * kFlatLdsBlock * rec_size;
    return l;
}

}  // namespace pt
