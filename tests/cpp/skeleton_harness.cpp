// Drives the skeleton entries of the C++ host mirror (bonnie-32_amd/host/rasterizer.hpp) end to end FROM A FILE:
//   skeleton_harness <scene.b32scene> <editor_alpha> <selected_bone> <n_bones> then per bone: px py pz rot_x rot_z length width parent
//   (floats as strtof reads them: hex floats are exact; parent -1: a root; width 0: display_width() resolves it)
// Every bone goes through b32::SkelBone::from_rig.  The scene's mesh is uploaded once (b32::ResidentMesh), the octahedra are built
// behind it on the device (build_skeleton) and the tail is read back; b32::skeleton_items runs beside it.  Output, hex words:
//   n_bones lines "B" + the ten words of the packed B32SkelBone
//   one line  "C" + body vertices, tail vertices, tail faces (b32_skeleton_counts)
//   per tail vertex "V" + nine words, per tail face "F" + five words, per item "I" + ten words
// Then build_skeleton with no bones must give the body back (exit code 4 otherwise).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scenefile.hpp"

template <class T>
static void words(const char* tag, const T& rec) {
    static_assert(sizeof(T) % 4 == 0, "whole words");
    unsigned w[sizeof(T) / 4];
    std::memcpy(w, &rec, sizeof(T));
    std::printf("%s", tag);
    for (unsigned x : w) std::printf(" %08x", x);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    try {
        const b32::SceneFile sc = b32::read_scene(argv[1]);
        B32SkeletonStyle style = b32::skeleton_style((uint8_t)std::atoi(argv[2]));
        style.selected_bone = std::atoi(argv[3]);
        const size_t n = (size_t)std::atoi(argv[4]);
        if ((size_t)argc != 5 + 8 * n) return 2;
        std::vector<b32::SkelBone> bones;
        for (size_t k = 0; k < n; ++k) {
            char** a = argv + 5 + 8 * k;
            const int parent = std::atoi(a[7]);
            bones.push_back(b32::SkelBone::from_rig({ std::strtof(a[0], nullptr), std::strtof(a[1], nullptr), std::strtof(a[2], nullptr) },
                                                    { std::strtof(a[3], nullptr), 0.0f, std::strtof(a[4], nullptr) }, std::strtof(a[5], nullptr),
                                                    std::strtof(a[6], nullptr), parent < 0 ? (uint32_t)B32_BONE_NONE : (uint32_t)parent));
        }
        const std::vector<B32SkelBone> tab = b32::pack_skeleton(bones);
        for (const auto& b : tab) words("B", b);
        uint32_t tv = 0, tf = 0;
        b32::check(b32_skeleton_counts(tab.data(), (uint32_t)tab.size(), &style, &tv, &tf), "skeleton_counts");
        const uint32_t nv = (uint32_t)sc.vertices.size(), nf = (uint32_t)sc.faces.size();
        std::printf("C %08x %08x %08x\n", nv, tv, tf);

        b32::Framebuffer fb(sc.width, sc.height);
        b32::ResidentMesh mesh(fb, sc.vertices, sc.faces, sc.textures);
        const std::vector<B32Vertex> body = mesh.read_vertices(0, nv);
        mesh.build_skeleton(bones, style);
        for (const auto& v : mesh.read_vertices(nv, tv)) words("V", v);
        std::vector<B32Face> faces(tf);
        if (tf) b32::check(b32_scene_read_faces(fb.ctx(), mesh.slot(), nf, tf, faces.data()), "scene_read_faces");
        for (const auto& f : faces) words("F", f);
        for (const auto& it : b32::skeleton_items(bones, style)) words("I", it);
        const std::vector<B32Vertex> kept = mesh.read_vertices(0, nv);
        if (nv && std::memcmp(kept.data(), body.data(), nv * sizeof(B32Vertex)) != 0) return 4;
        mesh.build_skeleton({}, style);
        B32Vertex past;
        if (b32_scene_read_vertices(fb.ctx(), mesh.slot(), nv, 1, &past) != B32_E_ARG) return 4;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "skeleton_harness: %s\n", e.what());
        return 1;
    }
    return 0;
}
