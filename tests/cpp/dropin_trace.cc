// Test program of tests/test_trace_cpu.py: the drop-in's trace() and BVH::trace_batch().
// stdin: "T R depth seed", then T triangles (9 vertex floats, the material type as a decimal, then
// color.rgb emit.rgb roughness) and R rays (o.xyz d.xyz), every float as the hex of its bits. It adds
// the triangles, builds the BVH, seeds the global rng with 12345 ONCE, calls trace() ray after ray
// (the stream continues from call to call) and then trace_batch() with one sample per ray. Per ray
// it prints the hex of trace()'s rgb, then of trace_batch()'s.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pathtracer/pathtracer.h"

static float read_float() {
    unsigned u = 0;
    if (std::scanf("%x", &u) != 1) std::exit(2);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static unsigned bits_of(float f) {
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main() {
    int T = 0, R = 0, depth = 0;
    unsigned seed = 0;
    if (std::scanf("%d %d %d %u", &T, &R, &depth, &seed) != 4) return 2;
    BVH bvh;
    for (int i = 0; i < T; i++) {
        float v[9], m[7];
        int type = 0;
        for (float& x : v) x = read_float();
        if (std::scanf("%d", &type) != 1) return 2;
        for (float& x : m) x = read_float();
        const Material mat((Material::Type)type, vec3(m[0], m[1], m[2]), vec3(m[3], m[4], m[5]), m[6]);
        bvh.add_triangle(Triangle(vec3(v[0], v[1], v[2]), vec3(v[3], v[4], v[5]), vec3(v[6], v[7], v[8]), mat));
    }
    bvh.build();
    std::vector<float> o(3 * (size_t)R), d(3 * (size_t)R);
    for (int r = 0; r < R; r++) {
        for (int k = 0; k < 3; k++) o[3 * r + k] = read_float();
        for (int k = 0; k < 3; k++) d[3 * r + k] = read_float();
    }
    const BVH& cb = bvh;  // both take a const BVH, as the reference's trace()
    std::vector<vec3> one(R);
    rng.seed(12345);
    for (int r = 0; r < R; r++)
        one[r] = trace(cb, vec3(o[3 * r], o[3 * r + 1], o[3 * r + 2]), vec3(d[3 * r], d[3 * r + 1], d[3 * r + 2]), depth);
    std::vector<float> batch(3 * (size_t)R);
    cb.trace_batch(o.data(), d.data(), (size_t)R, depth, 1, seed, batch.data());
    for (int r = 0; r < R; r++)
        std::printf("%08x %08x %08x %08x %08x %08x\n", bits_of(one[r].x), bits_of(one[r].y), bits_of(one[r].z),
                    bits_of(batch[3 * r]), bits_of(batch[3 * r + 1]), bits_of(batch[3 * r + 2]));
    return 0;
}
