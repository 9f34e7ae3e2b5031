// b32_room_body.h -- the arithmetic of the world editor's hover and rubber band over the current room's sector faces
// (find_hovered_elements, editor/viewport_3d.rs:7028-7336; find_selections_in_rect, :7512-7655) for ONE record of a b32_room: the four
// corners of a B32SectorFace on the sector lattice, their projection, the three candidate tests of a cursor and the centre the rubber
// band projects.  k_room_hover / k_room_hover_resolve / k_room_box (b32_room.hip) reduce what room_candidates / room_point_in_rect return.
// Every expression is a separately rounded f32 operation in the reference's order; the text also compiles for the host (B32_HD,
// b32_world_point.h), where tests/test_room_hover.py runs it against a literal restatement, built with and without -ffp-contract=off.
#pragma once
#if defined(__HIPCC__)
#include "b32_device.h"
#else
#include <math.h>
#include "b32_world_point.h"
#endif

namespace b32 {

// Corner k's (x, z) selectors per kind, bit k of nibble `kind`: 0 = base, 1 = base + S (viewport_3d.rs:6603-6657, :7099-7170, :7183-7279)
//   kind       0 Floor  1 Ceiling  2 North  3 East  4 South  5 West  6 NwSe  7 NeSw
//   x nibble   6        6          6        F       9        0       6       9
//   z nibble   C        C          0        6       F        9       6       6
constexpr uint32_t ROOM_XSEL = 0x9609F666u, ROOM_ZSEL = 0x669F60CCu;

B32_HD float room_sqrt(float x) {
#if defined(__HIPCC__)
    return __builtin_sqrtf(x);
#else
    return sqrtf(x);
#endif
}

// base_x / base_z of the record's sector: room.position + (g as f32) * SECTOR_SIZE, viewport_3d.rs:7074-7075
B32_HD void room_base(const B32RoomGrid& g, const B32SectorFace& f, float& base_x, float& base_z) {
    base_x = g.position[0] + (float)f.gx * g.sector_size;
    base_z = g.position[2] + (float)f.gz * g.sector_size;
}
// corner k (kind <= 7): (bx or bx + S, room_y + heights[k], bz or bz + S)
B32_HD void room_corner(const B32RoomGrid& g, const B32SectorFace& f, float base_x, float base_z, int k, float* p) {
    const uint32_t xs = (ROOM_XSEL >> (f.kind * 4u + (uint32_t)k)) & 1u, zs = (ROOM_ZSEL >> (f.kind * 4u + (uint32_t)k)) & 1u;
    p[0] = xs ? base_x + g.sector_size : base_x;
    p[1] = g.position[1] + f.heights[k];
    p[2] = zs ? base_z + g.sector_size : base_z;
}

// The record's four corners through world_to_screen_with_depth (math.rs:621-652), once: the three loops project the same corner with the
// same function, so one projection serves them all.
struct RoomQuad { bool some[4]; float sx[4], sy[4], d[4]; };
B32_HD void room_project(const ViewBlock& v, const B32RoomGrid& g, const B32SectorFace& f, RoomQuad& q) {
    float base_x, base_z;
    room_base(g, f, base_x, base_z);
    B32_UNROLL
    for (int k = 0; k < 4; ++k) {
        float p[3];
        room_corner(g, f, base_x, base_z, k, p);
        q.some[k] = world_point(v, p, false, q.sx[k], q.sy[k], q.d[k]);
    }
}

// ((mx - sx).powi(2) + (my - sy).powi(2)).sqrt(), viewport_3d.rs:7060
B32_HD float room_vertex_dist(float mx, float my, float sx, float sy) {
    const float dx = mx - sx, dy = my - sy;
    return room_sqrt(dx * dx + dy * dy);
}
// f32::clamp(0.0, 1.0): a NaN and -0.0 stay
B32_HD float room_clamp01(float t) {
    if (t < 0.0f) t = 0.0f;
    if (t > 1.0f) t = 1.0f;
    return t;
}
// point_to_segment_distance, math.rs:655-683
B32_HD float room_segment_dist(float px, float py, float x1, float y1, float x2, float y2) {
    const float dx = x2 - x1, dy = y2 - y1;
    const float len_sq = dx * dx + dy * dy;
    if (len_sq < 1e-6f) {
        const float pdx = px - x1, pdy = py - y1;
        return room_sqrt(pdx * pdx + pdy * pdy);
    }
    const float t = room_clamp01(((px - x1) * dx + (py - y1) * dy) / len_sq);
    const float closest_x = x1 + t * dx, closest_y = y1 + t * dy;
    const float dist_x = px - closest_x, dist_y = py - closest_y;
    return room_sqrt(dist_x * dist_x + dist_y * dist_y);
}
// interpolate_edge_depth, viewport_3d.rs:7411-7431
B32_HD float room_edge_depth(float mx, float my, float x0, float y0, float d0, float x1, float y1, float d1) {
    const float dx = x1 - x0, dy = y1 - y0;
    const float len_sq = dx * dx + dy * dy;
    if (len_sq < 0.0001f) return (d0 + d1) * 0.5f;
    const float t = room_clamp01(((mx - x0) * dx + (my - y0) * dy) / len_sq);
    return d0 + t * (d1 - d0);
}
// point_in_triangle_2d (math.rs:687-706) and interpolate_depth_in_triangle (viewport_3d.rs:7485-7508) for corners (a, b, c) of a quad, as
// pick_triangle_idx states them, without a cull: false = missed
B32_HD bool room_triangle(const RoomQuad& q, int a, int b, int c, float px, float py, float& depth) {
    const float x0 = q.sx[a], y0 = q.sy[a], x1 = q.sx[b], y1 = q.sy[b], x2 = q.sx[c], y2 = q.sy[c];
    const float d1 = (px - x1) * (y0 - y1) - (x0 - x1) * (py - y1);
    const float d2 = (px - x2) * (y1 - y2) - (x1 - x2) * (py - y2);
    const float d3 = (px - x0) * (y2 - y0) - (x2 - x0) * (py - y0);
    const bool has_neg = (d1 < 0.0f) || (d2 < 0.0f) || (d3 < 0.0f);
    const bool has_pos = (d1 > 0.0f) || (d2 > 0.0f) || (d3 > 0.0f);
    if (has_neg && has_pos) return false;
    const float area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
    if (fabsf(area) < 0.0001f) { depth = ((q.d[a] + q.d[b]) + q.d[c]) / 3.0f; return true; }
    const float w0 = ((x1 - px) * (y2 - py) - (x2 - px) * (y1 - py)) / area;
    const float w1 = ((x2 - px) * (y0 - py) - (x0 - px) * (y2 - py)) / area;
    const float w2 = (1.0f - w0) - w1;
    depth = (w0 * q.d[a] + w1 * q.d[b]) + w2 * q.d[c];
    return true;
}

// One corner as the vertex loop sees it (viewport_3d.rs:7050-7068): false = not a candidate
B32_HD bool room_vertex(const RoomQuad& q, int k, float mx, float my, float thr, float& dist, float& depth) {
    if (!q.some[k]) return false;
    dist = room_vertex_dist(mx, my, q.sx[k], q.sy[k]);
    depth = q.d[k];
    return dist < thr;
}
// Edge (k, (k + 1) % 4) as check_edge sees it (viewport_3d.rs:7078-7096), in its own orientation
B32_HD bool room_edge(const RoomQuad& q, int k, float mx, float my, float thr, float& dist, float& depth) {
    const int j = (k + 1) & 3;
    if (!q.some[k] || !q.some[j]) return false;
    dist = room_segment_dist(mx, my, q.sx[k], q.sy[k], q.sx[j], q.sy[j]);
    if (!(dist < thr)) return false;
    depth = room_edge_depth(mx, my, q.sx[k], q.sy[k], q.d[k], q.sx[j], q.sy[j], q.d[j]);
    return true;
}
// check_quad_hit_with_depth, viewport_3d.rs:7436-7481: all four corners project; (0, 1, 2), else (0, 2, 3)
B32_HD bool room_face(const RoomQuad& q, float mx, float my, float& depth) {
    if (!q.some[0] || !q.some[1] || !q.some[2] || !q.some[3]) return false;
    if (room_triangle(q, 0, 1, 2, mx, my, depth)) return true;
    return room_triangle(q, 0, 2, 3, mx, my, depth);
}

// What one record offers a cursor: bit k of vmask / emask = corner k / edge k is a candidate, with its distance and depth
struct RoomCandidates { uint32_t vmask, emask; bool face; float vdist[4], vdepth[4], edist[4], edepth[4], fdepth; };
B32_HD void room_candidates(const ViewBlock& v, const B32RoomGrid& g, const B32SectorFace& f, const B32RoomHoverParams& p, RoomCandidates& c) {
    RoomQuad q;
    room_project(v, g, f, q);
    c.vmask = 0u; c.emask = 0u;
    B32_UNROLL
    for (int k = 0; k < 4; ++k) {
        c.vdist[k] = c.vdepth[k] = c.edist[k] = c.edepth[k] = 0.0f;
        if (room_vertex(q, k, p.mx, p.my, p.vertex_threshold, c.vdist[k], c.vdepth[k])) c.vmask |= 1u << k;
        if (room_edge(q, k, p.mx, p.my, p.edge_threshold, c.edist[k], c.edepth[k])) c.emask |= 1u << k;
    }
    c.fdepth = 0.0f;
    c.face = room_face(q, p.mx, p.my, c.fdepth);
}

// The centre the rubber band projects for a record: face_center_in_rect / wall_center_in_rect, viewport_3d.rs:7597-7655
B32_HD void room_centre(const B32RoomGrid& g, const B32SectorFace& f, float* c) {
    float base_x, base_z;
    room_base(g, f, base_x, base_z);
    const float S = g.sector_size;
    const float avg = (((f.heights[0] + f.heights[1]) + f.heights[2]) + f.heights[3]) / 4.0f;
    c[1] = g.position[1] + avg;
    if (f.kind < 2u) { c[0] = base_x + S / 2.0f; c[2] = base_z + S / 2.0f; return; }
    float x0, z0, x1, z1;                                   // that function's own (x0, z0, x1, z1) per direction
    switch (f.kind) {
        case 2u: x0 = base_x; z0 = base_z; x1 = base_x + S; z1 = base_z; break;                  // North
        case 3u: x0 = base_x + S; z0 = base_z; x1 = base_x + S; z1 = base_z + S; break;          // East
        case 4u: x0 = base_x; z0 = base_z + S; x1 = base_x + S; z1 = base_z + S; break;          // South
        case 5u: x0 = base_x; z0 = base_z; x1 = base_x; z1 = base_z + S; break;                  // West
        case 6u: x0 = base_x; z0 = base_z; x1 = base_x + S; z1 = base_z + S; break;              // NwSe
        default: x0 = base_x + S; z0 = base_z; x1 = base_x; z1 = base_z + S; break;              // NeSw
    }
    c[0] = (x0 + x1) / 2.0f; c[2] = (z0 + z1) / 2.0f;
}
// world_to_screen (math.rs:503-534) of a point against the rectangle, inclusive; any NaN is false
B32_HD bool room_point_in_rect(const ViewBlock& v, const float* p, float x0, float y0, float x1, float y1) {
    float sx, sy, z;
    if (!world_point(v, p, false, sx, sy, z)) return false;
    return sx >= x0 && sx <= x1 && sy >= y0 && sy <= y1;
}

}  // namespace b32
