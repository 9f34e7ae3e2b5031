// room_host.cpp -- csrc/b32_room_body.h and csrc/b32_pick_words.h (the device code of b32_room_hover's and b32_room_box_select's arithmetic
// and of the three minima) compiled for the host, for tests/test_room_hover.py.  No device, no library.  The records are driven as k_room_hover drives them: record by record into three
// sets of minima per workgroup of 1024 records, the workgroups' minima folded (pick_fold) as the kernel's atomics fold them, and the
// winners' distance and depth recomputed from their records as k_room_hover_resolve does.
//   usage: room_host <in> <out>
//   in : u32 width, height, n, n_cursors, n_points, 0; 12 f32 camera (position, basis_x, basis_y, basis_z); B32RoomGrid;
//        2 f32 (vertex_threshold, edge_threshold); 4 f32 rectangle; n B32SectorFace; n_cursors x 2 f32; n_points x 3 f32
//   out: n_cursors B32RoomHover; u32 n_elements, n_selected; ceil(n_elements / 32) words
#include <cstdio>
#include <cstring>
#include <vector>

#include "b32_pick_words.h"
#include "b32_room_body.h"

namespace {

using b32::PickWords; using b32::pick_no_hit; using b32::pick_take; using b32::pick_fold; using b32::pick_winner;
constexpr uint32_t NONE = b32::PICK_NONE;

float qnan() { float f; std::memcpy(&f, &b32::PICK_QNAN, 4); return f; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t head[6]; B32Camera cam; float thr[2], rect[4];
    B32RoomGrid grid;
    if (std::fread(head, 4, 6, in) != 6 || std::fread(&cam, 4, 12, in) != 12 || std::fread(&grid, sizeof grid, 1, in) != 1 ||
        std::fread(thr, 4, 2, in) != 2 || std::fread(rect, 4, 4, in) != 4) return 3;
    const uint32_t w = head[0], h = head[1], n = head[2], nc = head[3], np = head[4];
    std::vector<B32SectorFace> faces(n);
    std::vector<float> cursors((size_t)nc * 2), points((size_t)np * 3);
    if (n && std::fread(faces.data(), sizeof(B32SectorFace), n, in) != n) return 3;
    if (nc && std::fread(cursors.data(), 8, nc, in) != nc) return 3;
    if (np && std::fread(points.data(), 12, np, in) != np) return 3;
    std::fclose(in);
    b32::ViewBlock v;
    b32::view_fill(v, cam, w, h, nullptr);

    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    for (uint32_t ci = 0; ci < nc; ++ci) {
        const B32RoomHoverParams prm{ cursors[2 * ci], cursors[2 * ci + 1], thr[0], thr[1] };
        PickWords gv = pick_no_hit(), ge = pick_no_hit(), gf = pick_no_hit();
        for (uint32_t e0 = 0; e0 < n; e0 += b32::PICK_CHUNK) {
            PickWords mv = pick_no_hit(), me = pick_no_hit(), mf = pick_no_hit();
            for (uint32_t i = e0; i < n && i < e0 + b32::PICK_CHUNK; ++i) {
                b32::RoomCandidates c;
                b32::room_candidates(v, grid, faces[i], prm, c);
                for (uint32_t k = 0; k < 4u; ++k) {
                    if ((c.vmask >> k) & 1u) pick_take(mv, c.vdepth[k], i * 4u + k);
                    if ((c.emask >> k) & 1u) pick_take(me, c.edepth[k], i * 4u + k);
                }
                if (c.face) pick_take(mf, c.fdepth, i);
            }
            pick_fold(gv, mv); pick_fold(ge, me); pick_fold(gf, mf);
        }
        B32RoomHover r{ NONE, NONE, 0.0f, 0.0f, NONE, NONE, 0.0f, 0.0f, NONE, 0.0f, { 0u, 0u } };
        uint32_t id; bool nan;
        b32::RoomQuad q;
        if (pick_winner(gv, id, nan)) {
            b32::room_project(v, grid, faces[id >> 2], q);
            r.vertex_rec = id >> 2; r.vertex_corner = id & 3u;
            (void)b32::room_vertex(q, (int)(id & 3u), prm.mx, prm.my, prm.vertex_threshold, r.vertex_dist, r.vertex_depth);
            if (nan) r.vertex_depth = qnan();
        }
        if (pick_winner(ge, id, nan)) {
            b32::room_project(v, grid, faces[id >> 2], q);
            r.edge_rec = id >> 2; r.edge_idx = id & 3u;
            (void)b32::room_edge(q, (int)(id & 3u), prm.mx, prm.my, prm.edge_threshold, r.edge_dist, r.edge_depth);
            if (nan) r.edge_depth = qnan();
        }
        if (pick_winner(gf, id, nan)) {
            b32::room_project(v, grid, faces[id], q);
            r.face_rec = id;
            (void)b32::room_face(q, prm.mx, prm.my, r.face_depth);
            if (nan) r.face_depth = qnan();
        }
        std::fwrite(&r, sizeof r, 1, out);
    }
    const uint32_t total = n + np;
    std::vector<uint32_t> words((total + 31u) / 32u, 0u);
    uint32_t selected = 0;
    for (uint32_t i = 0; i < total; ++i) {
        float p[3];
        if (i < n) b32::room_centre(grid, faces[i], p);
        else std::memcpy(p, points.data() + (size_t)(i - n) * 3, 12);
        if (b32::room_point_in_rect(v, p, rect[0], rect[1], rect[2], rect[3])) { words[i >> 5] |= 1u << (i & 31u); ++selected; }
    }
    const uint32_t bh[2] = { total, selected };
    std::fwrite(bh, 4, 2, out);
    if (!words.empty()) std::fwrite(words.data(), 4, words.size(), out);
    std::fclose(out);
    return 0;
}
