// A stand-alone caller of the fast builder's host twins (rrt_build_bvh_lbvh, rrt_refit_bvh_lbvh_world)
// on the edge shapes of tests/lbvh_scenes.py, for a sanitizer build of the host code
// (`make -C rustraytrace_amd/csrc lbvh_twin_asan` compiles rrt_host.cpp and this file with
// -fsanitize=address,undefined and runs the program; no device is touched). Every case is built in
// the three shapes, checked for a permutation order and consistent counts, and refitted over
// unchanged and over moved spheres. Exit code 0: all cases passed and the sanitizers were silent.
#include "rrt_hip.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct Case {
    std::string name;
    std::vector<RrtSphere> spheres;
    std::vector<RrtQuad> quads;
    std::vector<RrtMedium> media;
};

RrtSphere sphere(float x, float y, float z, float r) {
    RrtSphere s{};
    s.center_radius[0] = x, s.center_radius[1] = y, s.center_radius[2] = z, s.center_radius[3] = r;
    return s;
}

uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
float unit(uint32_t &s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

Case scattered(uint32_t n) {
    Case c;
    c.name = "scattered" + std::to_string(n);
    uint32_t s = 12345u + n;
    for (uint32_t i = 0; i < n; ++i) c.spheres.push_back(sphere(unit(s) * 20 - 10, unit(s) * 2, unit(s) * 20 - 10, 0.1f + 0.2f * unit(s)));
    return c;
}

int fails = 0;
void expect(bool ok, const std::string &what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s (%s)\n", what.c_str(), rrt_hip_last_error());
        ++fails;
    }
}

void run(const Case &c) {
    RrtSceneExt ext{};
    ext.n_quads = (uint32_t)c.quads.size(), ext.quads = c.quads.data();
    ext.n_media = (uint32_t)c.media.size(), ext.media = c.media.data();
    const bool has_ext = ext.n_quads || ext.n_media;
    const uint32_t n = (uint32_t)c.spheres.size(), n_prims = n + ext.n_quads + ext.n_media;
    std::vector<RrtSphere> moved = c.spheres;
    uint32_t s = 99u;
    for (RrtSphere &m : moved)
        for (int a = 0; a < 3; ++a) m.center_radius[a] += 0.1f * (unit(s) - 0.5f);
    const uint32_t shapes[3][2] = {{3, 80}, {1, 32}, {1, 80}};
    for (const auto &shape : shapes) {
        const std::string what = c.name + " leaf " + std::to_string(shape[0]) + " stride " + std::to_string(shape[1]);
        RrtBvhInfo info{};
        expect(rrt_build_bvh_lbvh(c.spheres.data(), n, has_ext ? &ext : nullptr, shape[0], shape[1], nullptr, 0, nullptr, &info) == RRT_OK,
               what + ": sizing");
        std::vector<uint8_t> nodes(info.node_bytes), again(info.node_bytes);
        std::vector<uint32_t> order(n_prims ? n_prims : 1), order2(n_prims ? n_prims : 1);
        expect(rrt_build_bvh_lbvh(c.spheres.data(), n, has_ext ? &ext : nullptr, shape[0], shape[1], nodes.data(), nodes.size(),
                                  order.data(), &info) == RRT_OK, what + ": build");
        std::vector<int> seen(n_prims, 0);
        for (uint32_t i = 0; i < n_prims; ++i)
            if (order[i] < n_prims) seen[order[i]]++;
        bool perm = true;
        for (int v : seen) perm = perm && v == 1;
        const uint32_t n_tree = n_prims - info.n_unbounded;
        expect(perm, what + ": the order is a permutation");
        expect(info.n_nodes >= 1 && info.node_bytes == (uint64_t)info.n_nodes * shape[1], what + ": node bytes");
        expect(info.max_leaf_size <= shape[0] && info.max_depth + 1 <= 63, what + ": leaf size and depth");
        expect(n_tree <= shape[0] || info.n_leaves == info.n_nodes + 1, what + ": a binary tree's leaf count");
        double sah = 0.0;
        RrtBvhInfo rinfo{};
        expect(rrt_refit_bvh_lbvh_world(c.spheres.data(), n, has_ext ? &ext : nullptr, shape[0], shape[1], c.spheres.data(),
                                        has_ext ? &ext : nullptr, again.data(), again.size(), order2.data(), &rinfo, &sah) == RRT_OK,
               what + ": refit over unchanged inputs");
        expect(again == nodes && order2 == order && std::memcmp(&rinfo, &info, sizeof info) == 0, what + ": a build is its own refit");
        expect(rrt_refit_bvh_lbvh_world(c.spheres.data(), n, has_ext ? &ext : nullptr, shape[0], shape[1], moved.data(),
                                        has_ext ? &ext : nullptr, again.data(), again.size(), order2.data(), &rinfo, &sah) == RRT_OK,
               what + ": refit over moved spheres");
        expect(order2 == order && rinfo.n_nodes == info.n_nodes, what + ": a refit keeps order and topology");
    }
}

}  // namespace

int main() {
    std::vector<Case> cases;
    for (uint32_t n : {2u, 3u, 63u, 64u, 65u, 257u}) cases.push_back(scattered(n));
    Case one;
    one.name = "one_centre64";
    for (int i = 0; i < 64; ++i) one.spheres.push_back(sphere(3.0f, 1.0f, -2.0f, 0.25f));
    cases.push_back(one);
    Case line;
    line.name = "line65";
    for (int i = 0; i < 65; ++i) line.spheres.push_back(sphere(-8.0f + 0.25f * i, 1.0f, -2.0f, 0.1f));
    cases.push_back(line);
    Case clusters = scattered(60);
    clusters.name = "clusters";
    for (int i = 30; i < 60; ++i) clusters.spheres[i].center_radius[0] += 1e6f;
    for (int i = 0; i < 30; ++i) clusters.spheres.push_back(sphere(0.5f + 1e-3f * i, 1.0f, 0.25f, 0.2f));
    cases.push_back(clusters);
    Case quads;
    quads.name = "quads";
    for (int i = 0; i < 5; ++i) {
        RrtQuad q{};
        q.q[0] = -3.0f + i, q.q[1] = -2.0f, q.q[2] = (float)i;
        q.u[0] = 0.5f * i, q.u[2] = -4.0f + i;
        q.v[1] = 4.0f - i;
        quads.quads.push_back(q);
    }
    cases.push_back(quads);
    Case fog = scattered(2);
    fog.name = "fog2";
    RrtMedium m{};
    m.sphere[3] = 5000.0f;  // holds everything: tested outside the tree of two
    m.boundary_kind = RRT_BOUNDARY_SPHERE;
    m.density = 0.01f;
    fog.media.push_back(m);
    cases.push_back(fog);
    for (const Case &c : cases) run(c);
    // refusals
    RrtBvhInfo info{};
    const Case c = scattered(8);
    expect(rrt_build_bvh_lbvh(nullptr, 8, nullptr, 3, 80, nullptr, 0, nullptr, &info) == RRT_E_INVALID, "null spheres are refused");
    expect(rrt_build_bvh_lbvh(c.spheres.data(), 8, nullptr, 0, 80, nullptr, 0, nullptr, &info) == RRT_E_INVALID, "max_leaf 0 is refused");
    expect(rrt_build_bvh_lbvh(c.spheres.data(), 8, nullptr, 8, 80, nullptr, 0, nullptr, &info) == RRT_E_INVALID, "max_leaf 8 is refused");
    expect(rrt_build_bvh_lbvh(c.spheres.data(), 8, nullptr, 3, 64, nullptr, 0, nullptr, &info) == RRT_E_INVALID, "stride 64 is refused");
    std::printf("lbvh_twin: %zu cases, %d failures\n", cases.size(), fails);
    return fails ? 1 : 0;
}
