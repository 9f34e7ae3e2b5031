// Drives the in-place edits of the C++ host mirror (bonnie-32_amd/host/rasterizer.hpp) end to end FROM A FILE:
//   patch_harness <scene.b32scene> <step> <dx> <dy> <dz>     (floats as strtof reads them: hex floats are exact)
// The scene's mesh is uploaded once (b32::ResidentMesh) with one more texture behind its own, 5 x 3 with texel k = 37 k + 1.  Then
//   vertices i with i % step == 0 get pos += (dx, dy, dz) and r ^= 255;
//   faces j with j % step == 1 get editor_alpha = 77 and black_transparent ^= 1;
//   the rectangle (1, 1) 3 x 2 of the extra texture gets texels 0x4000 + 16 row + col from an array 4 wide;
//   its rectangle (0, 0) 2 x 2 gets the indices {1, 0, 9, 2} looked up in the palette {0x1111, 0x2222, 0x3333}
// on the device, and b32::patch_* make the same edits to the host arrays.  Printed, the device's words | the host's: one line per vertex
// (9 words each), one per face (5), one for the extra texture (15).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scenefile.hpp"

template <class T>
static void words(const T& rec) {
    uint32_t w[sizeof(T) / 4];
    std::memcpy(w, &rec, sizeof(T));
    for (uint32_t x : w) std::printf(" %08x", x);
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    try {
        b32::SceneFile sc = b32::read_scene(argv[1]);
        const size_t step = (size_t)std::atoi(argv[2]);
        const float d[3] = { std::strtof(argv[3], nullptr), std::strtof(argv[4], nullptr), std::strtof(argv[5], nullptr) };
        if (!step) return 2;
        b32::Texture15 extra; extra.width = 5; extra.height = 3;
        for (uint32_t k = 0; k < 15; ++k) extra.pixels.push_back((uint16_t)(37 * k + 1));
        sc.textures.push_back(extra);
        const uint32_t tex = (uint32_t)sc.textures.size() - 1;
        std::vector<B32Vertex> hv; for (const auto& v : sc.vertices) hv.push_back(b32::detail::pack(v));
        std::vector<B32Face> hf; for (const auto& f : sc.faces) hf.push_back(b32::detail::pack(f));
        std::vector<uint16_t> ht = extra.pixels;

        b32::Framebuffer fb(sc.width, sc.height);
        b32::ResidentMesh mesh(fb, sc.vertices, sc.faces, sc.textures);
        std::vector<B32VertexPatch> vr;
        for (size_t i = 0; i < hv.size(); i += step) {
            B32VertexPatch r{ (uint32_t)i, hv[i] };
            for (int k = 0; k < 3; ++k) r.v.pos[k] += d[k];
            r.v.r ^= 255;
            vr.push_back(r);
        }
        std::vector<B32FacePatch> fr;
        for (size_t j = 1; j < hf.size(); j += step) {
            B32FacePatch r{ (uint32_t)j, hf[j] };
            r.f.editor_alpha = 77; r.f.black_transparent ^= 1;
            fr.push_back(r);
        }
        uint16_t block[2][4];
        for (int row = 0; row < 2; ++row) for (int col = 0; col < 4; ++col) block[row][col] = (uint16_t)(0x4000 + 16 * row + col);
        const uint8_t idx[4] = { 1, 0, 9, 2 };
        const std::vector<uint16_t> clut{ 0x1111, 0x2222, 0x3333 };
        mesh.patch_vertices(vr); mesh.patch_faces(fr);
        mesh.patch_texels(tex, 1, 1, 3, 2, &block[0][0], 4);
        mesh.patch_indexed(tex, 0, 0, 2, 2, idx, 2, clut);
        b32::patch_vertices(hv, vr); b32::patch_faces(hf, fr);
        b32::patch_texels(ht, 5, 1, 1, 3, 2, &block[0][0], 4);
        b32::patch_indexed(ht, 5, 0, 0, 2, 2, idx, 2, clut);

        const std::vector<B32Vertex> dv = mesh.read_vertices(0, (uint32_t)hv.size());
        const std::vector<B32Face> df = mesh.read_faces(0, (uint32_t)hf.size());
        const std::vector<uint16_t> dt = mesh.read_texels(tex, 5, 3);
        for (size_t i = 0; i < hv.size(); ++i) { std::printf("v"); words(dv[i]); std::printf(" |"); words(hv[i]); std::printf("\n"); }
        for (size_t j = 0; j < hf.size(); ++j) { std::printf("f"); words(df[j]); std::printf(" |"); words(hf[j]); std::printf("\n"); }
        std::printf("t");
        for (uint16_t x : dt) std::printf(" %08x", (unsigned)x);
        std::printf(" |");
        for (uint16_t x : ht) std::printf(" %08x", (unsigned)x);
        std::printf("\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "patch_harness: %s\n", e.what());
        return 1;
    }
    return 0;
}
