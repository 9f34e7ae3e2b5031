// Drives the pick entries of the C++ host mirror (bonnie-32_amd/host/rasterizer.hpp) end to end FROM A FILE:
//   pick_harness <scene.b32scene> <cull 0|1> <cos_f> <sin_f> <wx> <wy> <wz> <mx my>...
// The scene's mesh is uploaded once (b32::ResidentMesh) and picked twice per cursor in ONE call -- item 0 with the given placement, item 1
// with the identity -- through b32::pick_meshes (blocking) and, for the same cursor, through b32::pick_meshes_async + a ticket; the host
// restatement b32::pick_mesh runs beside it.  One line per cursor:
//   best hit tri depth_bits  hit tri depth_bits | async_best | host: hit tri depth_bits  hit tri depth_bits
// (compile with -ffp-contract=off: the host restatement must not be fused)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scenefile.hpp"

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
    if (argc < 10 || ((argc - 8) & 1)) return 2;
    try {
        const b32::SceneFile sc = b32::read_scene(argv[1]);
        const bool cull = std::atoi(argv[2]) != 0;
        b32::Placement placed;
        placed.cos_f = std::strtof(argv[3], nullptr); placed.sin_f = std::strtof(argv[4], nullptr);
        placed.world_pos = { std::strtof(argv[5], nullptr), std::strtof(argv[6], nullptr), std::strtof(argv[7], nullptr) };
        b32::Framebuffer fb(sc.width, sc.height);
        b32::ResidentMesh mesh(fb, sc.vertices, sc.faces, sc.textures);
        const std::vector<b32::PickItem> items{ { &mesh, placed }, { &mesh, b32::Placement{} } };
        void* out = b32_host_alloc(16 + 16 * items.size());
        if (!out) return 3;
        for (int a = 8; a + 1 < argc; a += 2) {
            const float mx = std::strtof(argv[a], nullptr), my = std::strtof(argv[a + 1], nullptr);
            const b32::PickResult r = b32::pick_meshes(fb, items, sc.camera, mx, my, std::nullopt, cull);
            const uint64_t t = b32::pick_meshes_async(fb, items, sc.camera, mx, my, out, std::nullopt, cull);
            b32::check(b32_ticket_wait(fb.ctx(), t), "ticket_wait");
            const b32::PickResult ra = b32::pick_result(out);
            if (ra.hits.size() != 2 || std::memcmp(ra.hits.data(), r.hits.data(), 2 * sizeof(B32PickHit)) != 0) return 4;
            std::printf("%d", r.best);
            for (const B32PickHit& h : r.hits) std::printf(" %u %u %08x", h.hit, h.tri, bits(h.depth));
            std::printf(" | %d | host:", ra.best);
            for (const b32::PickItem& it : items) {
                const B32PickHit h = b32::pick_mesh(sc.vertices, sc.faces, it.placement, sc.camera, sc.width, sc.height, mx, my, std::nullopt, cull);
                std::printf(" %u %u %08x", h.hit, h.tri, bits(h.depth));
            }
            std::printf("\n");
        }
        b32_host_free(out);
    } catch (const b32::Error& e) {
        std::fprintf(stderr, "b32::Error %d: %s\n", e.code, e.what());
        return 10;
    }
    return 0;
}
