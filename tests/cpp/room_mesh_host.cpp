// room_mesh_host.cpp -- csrc/b32_room_mesh_body.h (the device code of b32_room_build_mesh's arithmetic) compiled for the host, for
// tests/test_room_mesh.py.  No device, no library.  The records are driven as k_room_mesh drives them: the prefix sums of the counts on
// the host, then per record twelve vertex slots, of which the first 2 or 4 also write the record's faces.
//   usage: room_mesh_host <in> <out>
//   in : u32 n, 0; B32RoomGrid; n B32SectorFace; n B32FaceMaterial
//   out: u32 n_vertices, n_faces; n_vertices B32Vertex; n_faces B32Face
#include <cstdio>
#include <vector>

#include "b32_room_mesh_body.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t head[2];
    B32RoomGrid grid;
    if (std::fread(head, 4, 2, in) != 2 || std::fread(&grid, sizeof grid, 1, in) != 1) return 3;
    const uint32_t n = head[0];
    std::vector<B32SectorFace> faces(n);
    std::vector<B32FaceMaterial> mats(n);
    if (n && std::fread(faces.data(), sizeof(B32SectorFace), n, in) != n) return 3;
    if (n && std::fread(mats.data(), sizeof(B32FaceMaterial), n, in) != n) return 3;
    std::fclose(in);

    std::vector<uint32_t> first_v((size_t)n + 1, 0u), first_f((size_t)n + 1, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        first_v[i + 1] = first_v[i] + b32::room_mesh_vertex_count(faces[i].kind, mats[i].normal_mode);
        first_f[i + 1] = first_f[i] + b32::room_mesh_face_count(mats[i].normal_mode);
    }
    std::vector<B32Vertex> verts(first_v[n]);
    std::vector<B32Face> out_faces(first_f[n]);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t nv = b32::room_mesh_vertex_count(faces[i].kind, mats[i].normal_mode), nf = b32::room_mesh_face_count(mats[i].normal_mode);
        for (uint32_t slot = 0; slot < b32::ROOM_MESH_SLOTS; ++slot) {
            if (slot < nv) b32::room_mesh_vertex(grid, faces[i], mats[i], slot, verts[first_v[i] + slot]);
            if (slot < nf) b32::room_mesh_face(faces[i], mats[i], slot, first_v[i], out_faces[first_f[i] + slot]);
        }
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    const uint32_t counts[2] = { first_v[n], first_f[n] };
    std::fwrite(counts, 4, 2, out);
    if (!verts.empty()) std::fwrite(verts.data(), sizeof(B32Vertex), verts.size(), out);
    if (!out_faces.empty()) std::fwrite(out_faces.data(), sizeof(B32Face), out_faces.size(), out);
    std::fclose(out);
    return 0;
}
