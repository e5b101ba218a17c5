// Test program of tests/test_query_cpu.py: the drop-in BVH's intersect() and intersect_batch().
// stdin: "T R", then T triangles (9 vertex floats) and R rays (o.xyz d.xyz), every float as the
// hex of its bits. It adds the triangles, builds the BVH and prints, per ray, the triangle and
// the hex of t from BVH::intersect, then the same pair from intersect_batch.
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
    int T = 0, R = 0;
    if (std::scanf("%d %d", &T, &R) != 2) return 2;
    BVH bvh;
    const Material grey(Material::DIFFUSE, vec3(0.5f, 0.5f, 0.5f), vec3(0, 0, 0), 0);
    for (int i = 0; i < T; i++) {
        float v[9];
        for (float& x : v) x = read_float();
        bvh.add_triangle(Triangle(vec3(v[0], v[1], v[2]), vec3(v[3], v[4], v[5]), vec3(v[6], v[7], v[8]), grey));
    }
    bvh.build();
    std::vector<float> o(3 * (size_t)R), d(3 * (size_t)R);
    for (int r = 0; r < R; r++) {
        for (int k = 0; k < 3; k++) o[3 * r + k] = read_float();
        for (int k = 0; k < 3; k++) d[3 * r + k] = read_float();
    }
    std::vector<float> bt(R);
    std::vector<int> btri(R);
    bvh.intersect_batch(o.data(), d.data(), (size_t)R, bt.data(), btri.data());
    const BVH& cb = bvh;  // intersect is const, as the reference's
    for (int r = 0; r < R; r++) {
        float t;
        const int tri = cb.intersect(vec3(o[3 * r], o[3 * r + 1], o[3 * r + 2]), vec3(d[3 * r], d[3 * r + 1], d[3 * r + 2]), t);
        std::printf("%d %08x %d %08x\n", tri, bits_of(t), btri[r], bits_of(bt[r]));
    }
    return 0;
}
