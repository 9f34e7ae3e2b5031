// skeleton_host.cpp -- csrc/b32_skeleton_body.h (the device code of b32_scene_build_skeleton's arithmetic) compiled for the host, for
// tests/test_skeleton.py.  No device, no library.  The bones are driven as the library drives them: tip, liveness, colour and alpha per
// bone on the host, then per drawn octahedron six vertex lanes and eight face lanes.
//   usage: skeleton_host <in> <out>
//   in : u32 n_bones, u32 vertex_offset; B32SkeletonStyle; n_bones B32SkelBone
//   out: u32 n_vertices, n_faces; n_vertices B32Vertex; n_faces B32Face; n_bones x 3 floats (every bone's tip)
#include <cstdio>
#include <vector>

#include "b32_skeleton_body.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t head[2];
    B32SkeletonStyle style;
    if (std::fread(head, 4, 2, in) != 2 || std::fread(&style, sizeof style, 1, in) != 1) return 3;
    const uint32_t n = head[0];
    if (n > B32_MAX_BONES) return 3;
    std::vector<B32SkelBone> bones(n);
    if (n && std::fread(bones.data(), sizeof(B32SkelBone), n, in) != n) return 3;
    std::fclose(in);

    std::vector<b32::SkelOct> octs(b32::SKEL_MAX_OCTS);
    std::vector<float> tips((size_t)n * 3);
    uint32_t n_octs = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (b32::skel_bone_oct(bones[i], style, i, octs[n_octs])) ++n_octs;
        b32::skel_tip(bones[i], &tips[(size_t)i * 3]);
    }
    if (b32::skel_preview_oct(style, octs[n_octs])) ++n_octs;

    std::vector<B32Vertex> verts((size_t)n_octs * b32::SKEL_OCT_VERTS);
    std::vector<B32Face> faces((size_t)n_octs * b32::SKEL_OCT_FACES);
    for (uint32_t o = 0; o < n_octs; ++o) {
        const uint32_t v0 = head[1] + o * b32::SKEL_OCT_VERTS;
        for (uint32_t k = 0; k < b32::SKEL_OCT_ELEMS; ++k) {
            if (k < b32::SKEL_OCT_VERTS) b32::skel_vertex(octs[o], k, verts[(size_t)o * b32::SKEL_OCT_VERTS + k]);
            else b32::skel_face(octs[o], k - b32::SKEL_OCT_VERTS, v0, faces[(size_t)o * b32::SKEL_OCT_FACES + (k - b32::SKEL_OCT_VERTS)]);
        }
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    const uint32_t counts[2] = { (uint32_t)verts.size(), (uint32_t)faces.size() };
    std::fwrite(counts, 4, 2, out);
    if (!verts.empty()) std::fwrite(verts.data(), sizeof(B32Vertex), verts.size(), out);
    if (!faces.empty()) std::fwrite(faces.data(), sizeof(B32Face), faces.size(), out);
    if (!tips.empty()) std::fwrite(tips.data(), sizeof(float), tips.size(), out);
    std::fclose(out);
    return 0;
}
