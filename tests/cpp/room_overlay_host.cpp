// room_overlay_host.cpp -- csrc/b32_room_overlay_body.h (the device code of b32_draw_room_overlay's arithmetic) compiled for the host, for
// tests/test_room_overlay.py.  No device, no library.  Every slot group goes through the function its lane calls, into the place
// room_overlay_layout gives it; the winner rule is b32_room_winner.h's.
//   usage: room_overlay_host <in> <out>
//   in : u32 width, height, n, has_materials; B32RoomOverlay; B32RoomGrid; 12 f32 camera (position, basis_x, basis_y, basis_z);
//        n B32SectorFace; n B32FaceMaterial (has_materials); n_vertices u32 keys; n_edges x 2 u32; n_faces u32; n_points x 3 f32
//   out: 8 u32 (first record of vertices, edges, hover, selected faces, selected edges, preview, points; total); 3 u64 drawn, dropped,
//        rejected; i32 winner; u32 pad; total B32Prim
#include <cstdio>
#include <vector>

#include "b32_room_overlay_body.h"

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return !n || std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    using namespace b32;
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t head[4]; B32RoomOverlay o; B32RoomGrid g; B32Camera cam;
    if (std::fread(head, 4, 4, in) != 4 || std::fread(&o, sizeof o, 1, in) != 1 || std::fread(&g, sizeof g, 1, in) != 1 || std::fread(&cam, 4, 12, in) != 12) return 3;
    const uint32_t w = head[0], h = head[1], n = head[2];
    std::vector<B32SectorFace> faces; std::vector<B32FaceMaterial> mats; std::vector<uint32_t> keys, edges, sel; std::vector<float> points;
    if (!get(in, faces, n) || !get(in, mats, head[3] ? n : 0) || !get(in, keys, o.n_vertices) || !get(in, edges, (size_t)o.n_edges * 2) ||
        !get(in, sel, o.n_faces) || !get(in, points, (size_t)o.n_points * 3)) return 3;
    std::fclose(in);
    ViewBlock v;
    view_fill(v, cam, w, h, nullptr);
    if (room_overlay_check(&o, keys.data(), edges.data(), sel.data(), points.data())) return 5;
    const RoomOverlayLayout l = room_overlay_layout(n, o);
    std::vector<B32Prim> out((size_t)l.total);
    const B32FaceMaterial* M = head[3] ? mats.data() : nullptr;
    const uint32_t sec = o.sections;
    unsigned long long counts[3] = { 0, 0, 0 };
    auto take = [&](uint32_t tally) { for (int k = 0; k < 3; ++k) counts[k] += (tally >> (10 * k)) & 1023u; };
    const B32RoomHover& hv = o.hover;
    const int winner = room_hover_winner(hv);

    if (sec & B32_ROOM_OVERLAY_VERTICES) {
        const uint32_t key = (winner == 0 && hv.vertex_rec < n) ? hv.vertex_rec * 4u + (hv.vertex_corner & 3u) : ROOM_OVERLAY_NONE;
        for (uint32_t p = 0; p <= o.n_vertices; ++p)
            take(room_overlay_vertex(v, g, faces.data(), n, keys.data(), o.n_vertices, o.primary_vertex, key, p, out.data() + l.vertices + p));
    }
    if (sec & B32_ROOM_OVERLAY_EDGES)
        for (uint32_t e = 0; e < o.n_edges; ++e) {
            B32Prim* q = out.data() + l.edges + e;
            *q = prim_noop();
            if (edges[2 * e] < n) take(room_overlay_thick_edge(v, g, faces[edges[2 * e]], edges[2 * e + 1] & 3u, ROOM_OVERLAY_SELECTED_VERTEX, q));
        }
    if (sec & B32_ROOM_OVERLAY_HOVER) {
        B32Prim* q = out.data() + l.hover;
        for (uint32_t j = 0; j < ROOM_OVERLAY_HOVER_SLOTS; ++j) q[j] = prim_noop();
        if (winner == 1 && hv.edge_rec < n) take(room_overlay_thick_edge(v, g, faces[hv.edge_rec], hv.edge_idx & 3u, ROOM_OVERLAY_HOVER_EDGE, q));
        const bool skipped = hv.face_rec >= o.skip_first && hv.face_rec - o.skip_first < o.skip_count;
        if (winner == 2 && hv.face_rec < n && !skipped) take(room_overlay_face(v, g, faces[hv.face_rec], M ? M + hv.face_rec : nullptr, ROOM_OVERLAY_HOVER_FACE, q + 1));
    }
    if (sec & B32_ROOM_OVERLAY_SELECTED) {
        for (uint32_t k = 0; k < o.n_faces; ++k) {
            B32Prim* q = out.data() + l.sel_faces + (size_t)k * ROOM_OVERLAY_FACE_SLOTS;
            if (sel[k] < n) take(room_overlay_face(v, g, faces[sel[k]], M ? M + sel[k] : nullptr, ROOM_OVERLAY_SELECT, q));
            else for (uint32_t j = 0; j < ROOM_OVERLAY_FACE_SLOTS; ++j) q[j] = prim_noop();
        }
        for (uint32_t e = 0; e < o.n_edges; ++e) {
            B32Prim* q = out.data() + l.sel_edges + e;
            if (edges[2 * e] < n) take(room_overlay_line_edge(v, g, faces[edges[2 * e]], edges[2 * e + 1] & 3u, ROOM_OVERLAY_SELECT, q));
            else *q = prim_noop();
        }
    }
    if (l.gate) {
        for (uint32_t r = 0; r < n; ++r)
            take(room_overlay_preview(v, g, faces[r], l.rect[0], l.rect[1], l.rect[2], l.rect[3], out.data() + l.preview + (size_t)r * ROOM_OVERLAY_PREVIEW_SLOTS));
        for (uint32_t j = 0; j < o.n_points; ++j)
            take(room_overlay_preview_point(v, points.data() + (size_t)j * 3, l.rect[0], l.rect[1], l.rect[2], l.rect[3],
                                            out.data() + l.points + (size_t)j * ROOM_OVERLAY_POINT_SLOTS));
    }

    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const uint32_t lay[8] = { (uint32_t)l.vertices, (uint32_t)l.edges, (uint32_t)l.hover, (uint32_t)l.sel_faces, (uint32_t)l.sel_edges,
                              (uint32_t)l.preview, (uint32_t)l.points, (uint32_t)l.total };
    std::fwrite(lay, 4, 8, f);
    std::fwrite(counts, 8, 3, f);
    const int32_t tail[2] = { winner, 0 };
    std::fwrite(tail, 4, 2, f);
    if (!out.empty()) std::fwrite(out.data(), sizeof(B32Prim), out.size(), f);
    std::fclose(f);
    return 0;
}
