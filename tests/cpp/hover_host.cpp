// hover_host.cpp -- the C++ host restatements of host/rasterizer.hpp (b32::hover_mesh / b32::box_select over vectors; no device) on a mesh
// file, for tests/test_hover.py.  Identity camera, 320x240, OrthoProjection { zoom 1, centre (0, 0) }.
//   usage: hover_host <mesh file> <see_through 0|1> <mx my>...
//   mesh file: "nv np", nv lines of three f32 as hex words, np lines "n i0 i1 ..."
//   output: per cursor "vertex vertex_dist(hex) edge_v0 edge_v1 edge_dist(hex) face face_depth(hex)", then the indices the rectangle
//   (30, 30, 210, 175) selects in mode 0 and in mode 1, one line each.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "rasterizer.hpp"

static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1]);
    size_t nv = 0, np = 0;
    in >> nv >> np;
    std::vector<b32::Vertex> verts(nv);
    for (auto& v : verts) {
        float* p[3] = { &v.pos.x, &v.pos.y, &v.pos.z };
        for (float* q : p) { std::string w; in >> w; const uint32_t u = (uint32_t)std::strtoul(w.c_str(), nullptr, 16); std::memcpy(q, &u, 4); }
    }
    std::vector<uint32_t> start{ 0 }, pv;
    for (size_t i = 0; i < np; ++i) {
        size_t n = 0; in >> n;
        for (size_t k = 0; k < n; ++k) { unsigned long long x = 0; in >> x; pv.push_back((uint32_t)x); }
        start.push_back((uint32_t)pv.size());
    }
    if (!in) return 3;
    const bool see = std::atoi(argv[2]) != 0;
    const b32::Camera cam;
    const b32::Vec3 ortho{ 1.0f, 0.0f, 0.0f };
    for (int a = 3; a + 1 < argc; a += 2) {
        const B32HoverResult r = b32::hover_mesh(verts, start, pv, std::nullopt, cam, 320, 240, b32::hover_params(std::strtof(argv[a], nullptr), std::strtof(argv[a + 1], nullptr), see), ortho);
        std::printf("%u %08x %u %u %08x %u %08x\n", r.vertex, bits(r.vertex_dist), r.edge_v0, r.edge_v1, bits(r.edge_dist), r.face, bits(r.face_depth));
    }
    for (uint32_t mode = 0; mode < 2; ++mode) {
        const b32::BoxSelection s = b32::box_select(verts, start, pv, std::nullopt, cam, 320, 240, 30.0f, 30.0f, 210.0f, 175.0f, mode, ortho);
        for (size_t i = 0; i < (mode ? np : nv); ++i) if (s.test(i)) std::printf("%zu ", i);
        std::printf("\n");
    }
    return 0;
}
