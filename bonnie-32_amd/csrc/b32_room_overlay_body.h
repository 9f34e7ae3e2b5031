// b32_room_overlay_body.h -- the arithmetic of the world editor's room overlays (editor/viewport_3d.rs:4273-4658, :4862-5362) for one slot
// group: the selected / hovered vertex circles (:4273-4316), draw_edge_highlight (:4318-4402), the hovered edge and face (:4404-4658),
// draw_selection's SectorFace and Edge arms (:4862-5247) and the box-select preview (:5249-5362).  k_room_overlay (b32_room_overlay.hip)
// turns (resident records, materials, hover, lists, rectangle) into B32Prim records with these functions.  Every expression is a
// separately rounded f32 operation in the reference's order.  Not restated here: draw_3d_line is gizmo_item's B32_GIZMO_LINE
// (b32_gizmo_body.h); the cast, the 2^30 limit, the no-op and the circle and thick-line records are b32_prim_record.h's -- what a
// refused call means (a tally in 10-bit fields) is this file's.  The text also compiles for the host (B32_HD, b32_world_point.h), where tests/test_room_overlay.py
// runs it against a literal restatement, built with and without -ffp-contract=off.
//
// Where a record lies is a function of n, the B32RoomOverlay and the lists alone (room_overlay_layout): a call the reference does not
// make leaves the no-op record (a circle of radius -1) in its slot.
//   VERTICES  n_vertices + 1       the keys in ascending order, the hovered vertex at its rank among them
//   EDGES     n_edges              one B32_PRIM_THICK_LINE each
//   HOVER     1 + 6                the hovered edge's thick line, then the hovered face's lines
//   SELECTED  6 * n_faces + n_edges
//   PREVIEW   4 * n + 3 * n_points when the rectangle passes the gate of :5258, else nothing
// A corner is computed from the record where it lies with a run-time corner index (room_corner): no per-lane corner array.
#pragma once
#include "b32_room_body.h"
#include "b32_gizmo_body.h"
#include "b32_room_winner.h"

namespace b32 {

constexpr uint32_t ROOM_OVERLAY_NONE = 0xFFFFFFFFu;
constexpr uint32_t ROOM_OVERLAY_ALL = 31u;          // every B32_ROOM_OVERLAY_* bit
constexpr uint32_t ROOM_OVERLAY_HOVER_SLOTS = 7u, ROOM_OVERLAY_FACE_SLOTS = 6u, ROOM_OVERLAY_PREVIEW_SLOTS = 4u, ROOM_OVERLAY_POINT_SLOTS = 3u;

constexpr PrimColor ROOM_OVERLAY_SELECTED_VERTEX = { 100, 255, 100 }, ROOM_OVERLAY_HOVER_VERTEX = { 255, 200, 150 },
                    ROOM_OVERLAY_HOVER_EDGE = { 255, 200, 100 }, ROOM_OVERLAY_HOVER_FACE = { 150, 200, 255 },
                    ROOM_OVERLAY_SELECT = { 255, 200, 80 }, ROOM_OVERLAY_PREVIEW = { 100, 220, 255 };

// What a slot group adds to drawn / dropped / rejected: three 10-bit fields (a lane makes at most six calls, a wave 384)
B32_HD uint32_t room_overlay_tally(uint32_t which) { return 1u << (10u * which); }

// corner `kpos`'s place on the lattice with height H[k]
B32_HD void room_overlay_corner(const B32RoomGrid& g, const B32SectorFace& f, const float* H, float base_x, float base_z, uint32_t kpos, uint32_t k, float* p) {
    const uint32_t xs = (ROOM_XSEL >> (f.kind * 4u + kpos)) & 1u, zs = (ROOM_ZSEL >> (f.kind * 4u + kpos)) & 1u;
    p[0] = xs ? base_x + g.sector_size : base_x;
    p[1] = g.position[1] + H[k];
    p[2] = zs ? base_z + g.sector_size : base_z;
}

// draw_3d_line(fb, p0, p1, camera, color) into one record
B32_HD uint32_t room_overlay_line(const ViewBlock& v, const float* p0, const float* p1, PrimColor c, B32Prim* out) {
    B32GizmoItem it{};
    B32_UNROLL
    for (int k = 0; k < 3; ++k) { it.p0[k] = p0[k]; it.p1[k] = p1[k]; }
    it.r = c.r; it.g = c.g; it.b = c.b; it.blend = c.blend;
    it.kind = B32_GIZMO_LINE;
    return room_overlay_tally(gizmo_item(v, it, out));
}

// world_to_screen -> fb.draw_circle(fb_x as i32, fb_y as i32, radius, color), :4276-4313
B32_HD uint32_t room_overlay_circle(const ViewBlock& v, const float* p, int32_t radius, PrimColor c, B32Prim* out) {
    float sx, sy, z;
    if (!world_point(v, p, false, sx, sy, z)) return room_overlay_tally(1u);
    const int32_t x = as_i32(sx), y = as_i32(sy);
    if (prim_big(x) || prim_big(y)) return room_overlay_tally(2u);
    *out = prim_circle(B32_PRIM_CIRCLE, x, y, radius, c, 255u);
    return room_overlay_tally(0u);
}

// edge (e, (e + 1) % 4) of record f as draw_edge_highlight draws it, :4373-4384: both ends through world_to_screen, fb.draw_thick_line(.., 3, color)
B32_HD uint32_t room_overlay_thick_edge(const ViewBlock& v, const B32RoomGrid& g, const B32SectorFace& f, uint32_t e, PrimColor c, B32Prim* out) {
    float base_x, base_z, p0[3], p1[3];
    room_base(g, f, base_x, base_z);
    const uint32_t e1 = (e + 1u) & 3u;
    room_overlay_corner(g, f, f.heights, base_x, base_z, e, e, p0);
    room_overlay_corner(g, f, f.heights, base_x, base_z, e1, e1, p1);
    float sx0, sy0, sx1, sy1, z;
    const bool some0 = world_point(v, p0, false, sx0, sy0, z), some1 = world_point(v, p1, false, sx1, sy1, z);
    if (!some0 || !some1) return room_overlay_tally(1u);
    const int32_t x0 = as_i32(sx0), y0 = as_i32(sy0), x1 = as_i32(sx1), y1 = as_i32(sy1);
    if (prim_wide(x0, x1) || prim_wide(y0, y1)) return room_overlay_tally(2u);
    *out = prim_thick_line(x0, y0, x1, y1, 3, c, 255u);
    return room_overlay_tally(0u);
}

// draw_selection's Edge arm, :5229-5233: one draw_3d_line between corners e and (e + 1) % 4
B32_HD uint32_t room_overlay_line_edge(const ViewBlock& v, const B32RoomGrid& g, const B32SectorFace& f, uint32_t e, PrimColor c, B32Prim* out) {
    float base_x, base_z, p0[3], p1[3];
    room_base(g, f, base_x, base_z);
    const uint32_t e1 = (e + 1u) & 3u;
    room_overlay_corner(g, f, f.heights, base_x, base_z, e, e, p0);
    room_overlay_corner(g, f, f.heights, base_x, base_z, e1, e1, p1);
    return room_overlay_line(v, p0, p1, c, out);
}

// The lines of a hovered (:4493-4654) or selected (:4875-5046) face, six slots.  Two bits per corner index, slot j at bits 2 * j:
//   floor / ceiling, NwSe  1[0]-1[1]  1[1]-1[2]  2[2]-2[3]  2[3]-2[0]  1[0]-1[2]  2[0]-2[2]      (1: heights, 2: get_heights_2())
//   floor / ceiling, NeSw  1[0]-1[1]  1[0]-1[3]  2[1]-2[2]  2[2]-2[3]  1[1]-1[3]  2[1]-2[3]
//   wall                   p0-p1  p1-p2  p2-p3  p3-p0  p0-p2  (nothing)
constexpr uint32_t room_overlay_pack6(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e, uint32_t f) {
    return a | (b << 2) | (c << 4) | (d << 6) | (e << 8) | (f << 10);
}
constexpr uint32_t ROOM_OVERLAY_A_NWSE = room_overlay_pack6(0, 1, 2, 3, 0, 0), ROOM_OVERLAY_B_NWSE = room_overlay_pack6(1, 2, 3, 0, 2, 2),
                   ROOM_OVERLAY_A_NESW = room_overlay_pack6(0, 0, 1, 2, 1, 1), ROOM_OVERLAY_B_NESW = room_overlay_pack6(1, 3, 2, 3, 3, 3),
                   ROOM_OVERLAY_SECOND = 0x2Cu;     // slots 2, 3 and 5 read triangle 2's heights
// mat: the record's material, or nullptr (no table: the record's own heights and B32_SPLIT_NWSE, the reference's defaults)
B32_HD uint32_t room_overlay_face(const ViewBlock& v, const B32RoomGrid& g, const B32SectorFace& f, const B32FaceMaterial* mat, PrimColor c, B32Prim* out) {
    float base_x, base_z;
    room_base(g, f, base_x, base_z);
    const bool flat = f.kind < 2u;
    const bool nesw = flat && mat && mat->split_direction == B32_SPLIT_NESW;
    const float* H2 = (flat && mat && (mat->flags & B32_MAT_HAS_HEIGHTS_2)) ? mat->heights_2 : f.heights;
    const uint32_t A = nesw ? ROOM_OVERLAY_A_NESW : ROOM_OVERLAY_A_NWSE, B = nesw ? ROOM_OVERLAY_B_NESW : ROOM_OVERLAY_B_NWSE;
    uint32_t tally = 0u;
    for (uint32_t j = 0; j < ROOM_OVERLAY_FACE_SLOTS; ++j) {
        if (!flat && j == 5u) { out[j] = prim_noop(); continue; }
        const uint32_t ka = (A >> (2u * j)) & 3u, kb = (B >> (2u * j)) & 3u;
        const float* H = (flat && ((ROOM_OVERLAY_SECOND >> j) & 1u)) ? H2 : f.heights;
        float p0[3], p1[3];
        room_overlay_corner(g, f, H, base_x, base_z, ka, ka, p0);
        room_overlay_corner(g, f, H, base_x, base_z, kb, kb, p1);
        tally += room_overlay_line(v, p0, p1, c, out + j);
    }
    return tally;
}

// The preview of record f, :5267-5340, four slots: selected by its centre as k_room_box decides, then the outline from `heights` alone.
// WallSouth and WallWest: the preview's own (x0, z0, x1, z1) is the reverse of every other site (:5307, :5309), so corner k stands where
// corner k ^ 1 stands elsewhere, with its own height.
B32_HD uint32_t room_overlay_preview(const ViewBlock& v, const B32RoomGrid& g, const B32SectorFace& f, float rx0, float ry0, float rx1, float ry1, B32Prim* out) {
    for (uint32_t j = 0; j < ROOM_OVERLAY_PREVIEW_SLOTS; ++j) out[j] = prim_noop();
    float c[3];
    room_centre(g, f, c);
    if (!room_point_in_rect(v, c, rx0, ry0, rx1, ry1)) return 0u;
    float base_x, base_z;
    room_base(g, f, base_x, base_z);
    const uint32_t flip = (f.kind == 4u || f.kind == 5u) ? 1u : 0u;
    uint32_t tally = 0u;
    for (uint32_t j = 0; j < ROOM_OVERLAY_PREVIEW_SLOTS; ++j) {
        const uint32_t j1 = (j + 1u) & 3u;
        float p0[3], p1[3];
        room_overlay_corner(g, f, f.heights, base_x, base_z, j ^ flip, j, p0);
        room_overlay_corner(g, f, f.heights, base_x, base_z, j1 ^ flip, j1, p1);
        tally += room_overlay_line(v, p0, p1, ROOM_OVERLAY_PREVIEW, out + j);
    }
    return tally;
}

// The preview of an object position, :5341-5352, three slots: world_pos -+ Vec3(size, 0, 0) etc., component by component
B32_HD uint32_t room_overlay_preview_point(const ViewBlock& v, const float* p, float rx0, float ry0, float rx1, float ry1, B32Prim* out) {
    for (uint32_t j = 0; j < ROOM_OVERLAY_POINT_SLOTS; ++j) out[j] = prim_noop();
    if (!room_point_in_rect(v, p, rx0, ry0, rx1, ry1)) return 0u;
    const float size = 64.0f;
    uint32_t tally = 0u;
    for (uint32_t j = 0; j < ROOM_OVERLAY_POINT_SLOTS; ++j) {
        float p0[3], p1[3];
        B32_UNROLL
        for (uint32_t k = 0; k < 3u; ++k) {
            const float d = k == j ? size : 0.0f;
            p0[k] = p[k] - d; p1[k] = p[k] + d;
        }
        tally += room_overlay_line(v, p0, p1, ROOM_OVERLAY_PREVIEW, out + j);
    }
    return tally;
}

// Slot p of the VERTICES section (n_keys + 1 slots), :4275-4314: the selected keys in ascending order with the hovered vertex (hover_key,
// ROOM_OVERLAY_NONE when the hover's winner is not a vertex) at its rank among them -- the loop is over collect_room_vertices order, which
// is the keys' order, and the later circle wins a shared pixel.  A hovered vertex that is also selected is drawn as selected.
B32_HD uint32_t room_overlay_vertex(const ViewBlock& v, const B32RoomGrid& g, const B32SectorFace* faces, uint32_t n, const uint32_t* keys, uint32_t n_keys,
                                    uint32_t primary, uint32_t hover_key, uint32_t p, B32Prim* out) {
    *out = prim_noop();
    uint32_t lo = n_keys;
    if (hover_key != ROOM_OVERLAY_NONE) {           // the first key >= hover_key
        lo = 0u;
        uint32_t hi = n_keys;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (keys[mid] < hover_key) lo = mid + 1u; else hi = mid;
        }
    }
    uint32_t key;
    const bool hovered = p == lo;
    if (hovered) {
        if (hover_key == ROOM_OVERLAY_NONE || (lo < n_keys && keys[lo] == hover_key)) return 0u;
        key = hover_key;
    } else key = keys[p < lo ? p : p - 1u];
    const uint32_t rec = key >> 2, corner = key & 3u;
    if (rec >= n) return 0u;
    const B32SectorFace& f = faces[rec];
    float base_x, base_z, q[3];
    room_base(g, f, base_x, base_z);
    room_overlay_corner(g, f, f.heights, base_x, base_z, corner, corner, q);
    if (hovered) return room_overlay_circle(v, q, 4, ROOM_OVERLAY_HOVER_VERTEX, out);
    return room_overlay_circle(v, q, key == primary ? 5 : 4, ROOM_OVERLAY_SELECTED_VERTEX, out);
}

// ---- host: the argument rules of the struct and the lists (0: fine, else B32_E_ARG) ...
static inline int room_overlay_check(const B32RoomOverlay* o, const uint32_t* sel_vertices, const uint32_t* sel_edges, const uint32_t* sel_faces,
                                     const float* points_xyz) {
    if ((o->sections & ~ROOM_OVERLAY_ALL) || o->hover_source > 1u) return B32_E_ARG;
    if ((o->n_vertices && !sel_vertices) || (o->n_edges && !sel_edges) || (o->n_faces && !sel_faces) || (o->n_points && !points_xyz)) return B32_E_ARG;
    for (uint32_t i = 1; i < o->n_vertices; ++i) if (sel_vertices[i] <= sel_vertices[i - 1u]) return B32_E_ARG;
    for (uint32_t i = 0; i < o->n_edges; ++i) if (sel_edges[2u * (size_t)i + 1u] > 3u) return B32_E_ARG;
    if (o->hover_source == 0u && o->hover.edge_rec != ROOM_OVERLAY_NONE && o->hover.edge_idx > 3u) return B32_E_ARG;
    return B32_OK;
}
// ... and where the sections lie: first record of every part, the total, the rectangle as the reference passes it on (:5252-5258)
struct RoomOverlayLayout {
    uint64_t vertices, edges, hover, sel_faces, sel_edges, preview, points, total;
    float rect[4]; bool gate;
};
static inline RoomOverlayLayout room_overlay_layout(uint32_t n, const B32RoomOverlay& o) {
    RoomOverlayLayout l{};
    uint64_t at = 0;
    l.vertices = at; if (o.sections & B32_ROOM_OVERLAY_VERTICES) at += (uint64_t)o.n_vertices + 1u;
    l.edges = at; if (o.sections & B32_ROOM_OVERLAY_EDGES) at += o.n_edges;
    l.hover = at; if (o.sections & B32_ROOM_OVERLAY_HOVER) at += ROOM_OVERLAY_HOVER_SLOTS;
    l.sel_faces = at; if (o.sections & B32_ROOM_OVERLAY_SELECTED) at += (uint64_t)ROOM_OVERLAY_FACE_SLOTS * o.n_faces;
    l.sel_edges = at; if (o.sections & B32_ROOM_OVERLAY_SELECTED) at += o.n_edges;
    l.rect[0] = f32_min(o.x0, o.x1); l.rect[2] = f32_max(o.x0, o.x1);
    l.rect[1] = f32_min(o.y0, o.y1); l.rect[3] = f32_max(o.y0, o.y1);
    l.gate = (o.sections & B32_ROOM_OVERLAY_PREVIEW) && ((l.rect[2] - l.rect[0]) > 3.0f || (l.rect[3] - l.rect[1]) > 3.0f);
    l.preview = at; if (l.gate) at += (uint64_t)ROOM_OVERLAY_PREVIEW_SLOTS * n;
    l.points = at; if (l.gate) at += (uint64_t)ROOM_OVERLAY_POINT_SLOTS * o.n_points;
    l.total = at;
    return l;
}

}  // namespace b32
