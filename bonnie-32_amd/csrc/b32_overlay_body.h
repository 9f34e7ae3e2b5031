// b32_overlay_body.h -- the arithmetic of the modeler's selection overlays (modeler/viewport.rs:1782-2247) for one element:
// draw_selected_object_brackets (:1782-1884), draw_mesh_selection_overlays (:1890-2105) and draw_box_selection_preview (:2108-2247).
// k_overlay_points and k_overlay_emit (b32_overlay.hip) turn (slot vertices, topology, hover result, selection, rectangle) into B32Prim
// records with these functions.  Every expression is a separately rounded f32 operation in the reference's order, `as i32` saturates
// and `as i32 + 1` wraps (a release build).  Not restated here: the casts, f32::min, the 2^30 limit, the no-op and the line and circle
// records are b32_prim_record.h's -- that a refused call is the no-op and nothing else is this file's.  The text also compiles for the
// host (B32_HD, b32_world_point.h), where tests/test_mesh_overlay.py runs it against a literal restatement, built with and without
// -ffp-contract=off.
//
// Where a record lies is a function of the topology, nv, the B32MeshOverlay and the selected list alone (overlay_layout): a call the
// reference does not make leaves the no-op record (a circle of radius -1) in its slot.
//   BRACKETS  24 (nv > 0)                         corner c = k / 3, direction k % 3
//   EDGES     nh                                  half-edge h
//   DOTS      nv                                  vertex i
//   HOVER     1 (vertex) + 3 (edge) + n + (n >= 4) (polygon of n positions; nothing for an index >= np)
//   SELECTED  n_selected | 4 * n_selected | sum of 2 * n + 1 over the listed polygons < np
//   PREVIEW   nv | 2 * ne (first half-edge of every edge, in loop order) | nh + np (polygon p at poly_start[p] + p)
#pragma once
#include "b32_prim_record.h"

namespace b32 {

constexpr uint32_t OVERLAY_NONE = 0xFFFFFFFFu;
constexpr uint32_t OVERLAY_ALL = 63u;               // every B32_OVERLAY_* bit
enum : uint32_t { OVERLAY_POLY_HOVER = 0u, OVERLAY_POLY_SELECTED = 1u, OVERLAY_POLY_PREVIEW = 2u };

// one vertex through world_to_screen_with_ortho[_depth], projected once (world_point is pure: the table's entry is what every one of the
// reference's repeated projections of that vertex gives)
struct OverlayPoint { float sx, sy, z; uint32_t some; };
// min / max of the slot's positions as orderable keys (overlay_key)
struct OverlayBounds { uint32_t mn[3], mx[3]; };
constexpr uint32_t OVERLAY_KEY_MIN0 = 0xFF7FFFFFu;  // overlay_key(f32::MAX): where the minima start
constexpr uint32_t OVERLAY_KEY_MAX0 = 0x00800000u;  // overlay_key(f32::MIN): where the maxima start

constexpr PrimColor OVERLAY_BRACKET_COLOR = { 0, 200, 230 }, OVERLAY_EDGE_COLOR = { 80, 80, 80 }, OVERLAY_DOT_COLOR = { 40, 40, 50 },
                    OVERLAY_HOVER_COLOR = { 255, 200, 150 }, OVERLAY_SELECT_COLOR = { 100, 180, 255 }, OVERLAY_PREVIEW_COLOR = { 255, 220, 100 };

// total order of the non-NaN f32 as u32, both zeros on one value (the hover's pick_orderable), and back (a zero comes back as +0.0)
B32_HD uint32_t overlay_key(float d) {
    uint32_t u = f32_bits(d);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
B32_HD float overlay_unkey(uint32_t k) { return bits_f32((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
// one position into the bounds: f32::min / f32::max ignore a NaN
B32_HD void overlay_bounds_take(OverlayBounds& b, const float* p) {
    for (int c = 0; c < 3; ++c) {
        if (p[c] != p[c]) continue;
        const uint32_t k = overlay_key(p[c]);
        if (k < b.mn[c]) b.mn[c] = k;
        if (k > b.mx[c]) b.mx[c] = k;
    }
}
constexpr OverlayBounds overlay_bounds_start() {   // (constexpr: host and device)
    return OverlayBounds{ { OVERLAY_KEY_MIN0, OVERLAY_KEY_MIN0, OVERLAY_KEY_MIN0 }, { OVERLAY_KEY_MAX0, OVERLAY_KEY_MAX0, OVERLAY_KEY_MAX0 } };
}

// fb.draw_line / draw_line_3d / draw_line_3d_alpha with cast ends; the no-op, and not a word, when an extent is too wide
B32_HD B32Prim overlay_line(uint32_t kind, int32_t x0, int32_t y0, int32_t x1, int32_t y1, float z0, float z1, PrimColor c, uint32_t alpha) {
    if (prim_wide(x0, x1) || prim_wide(y0, y1)) return prim_noop();
    return prim_line(kind, x0, y0, x1, y1, z0, z1, c, alpha);
}
// the 2-D line between two projected vertices, its ends moved by (ox, oy) in {0, 1} after the cast
B32_HD B32Prim overlay_seg(const OverlayPoint& e0, const OverlayPoint& e1, bool ox, bool oy, PrimColor c) {
    int32_t x0 = as_i32(e0.sx), y0 = as_i32(e0.sy), x1 = as_i32(e1.sx), y1 = as_i32(e1.sy);
    if (ox) { x0 = inc_wrap(x0); x1 = inc_wrap(x1); }
    if (oy) { y0 = inc_wrap(y0); y1 = inc_wrap(y1); }
    return overlay_line(B32_LINE_2D, x0, y0, x1, y1, 0.0f, 0.0f, c, 255u);
}
// fb.draw_circle[_alpha] at a projected point; the no-op when the centre is too big
B32_HD B32Prim overlay_circle(const OverlayPoint& e, int32_t radius, PrimColor c, uint32_t kind, uint32_t alpha) {
    const int32_t x = as_i32(e.sx), y = as_i32(e.sy);
    if (prim_big(x) || prim_big(y)) return prim_noop();
    return prim_circle(kind, x, y, radius, c, alpha);
}
// sx >= fb_x0 && sx <= fb_x1 && sy >= fb_y0 && sy <= fb_y1 (a NaN gives false); rect = x0, y0, x1, y1
B32_HD bool overlay_inside(float x, float y, const float* rect) { return x >= rect[0] && x <= rect[2] && y >= rect[1] && y <= rect[3]; }

B32_HD OverlayPoint overlay_point(const ViewBlock& a, const float* p) {
    OverlayPoint e; e.sx = 0.0f; e.sy = 0.0f; e.z = 0.0f;
    e.some = world_point(a, p, a.has_ortho != 0u, e.sx, e.sy, e.z) ? 1u : 0u;
    return e;
}

// ---- per element: what the lanes of k_overlay_points / k_overlay_emit write
// :1939-1954
B32_HD B32Prim overlay_dot(const OverlayPoint& e) {
    return e.some ? overlay_circle(e, 3, OVERLAY_DOT_COLOR, B32_PRIM_CIRCLE_ALPHA, 140u) : prim_noop();
}
// :2160-2178
B32_HD B32Prim overlay_preview_vertex(const OverlayPoint& e, const float* rect) {
    return (e.some && overlay_inside(e.sx, e.sy, rect)) ? overlay_circle(e, 6, OVERLAY_PREVIEW_COLOR, B32_PRIM_CIRCLE, 255u) : prim_noop();
}
// :1924-1935, one half-edge
B32_HD B32Prim overlay_edge(uint32_t v0, uint32_t v1, uint32_t nv, const OverlayPoint* tab) {
    if (v0 >= nv || v1 >= nv) return prim_noop();
    const OverlayPoint e0 = tab[v0], e1 = tab[v1];
    if (!e0.some || !e1.some) return prim_noop();
    return overlay_line(B32_LINE_3D_ALPHA, as_i32(e0.sx), as_i32(e0.sy), as_i32(e1.sx), as_i32(e1.sy), e0.z, e1.z, OVERLAY_EDGE_COLOR, 191u);
}
// :2183-2205, the first half-edge of its normalised edge: two records
B32_HD void overlay_preview_edge(uint32_t v0, uint32_t v1, uint32_t nv, const OverlayPoint* tab, const float* rect, B32Prim* out) {
    out[0] = prim_noop(); out[1] = prim_noop();
    if (v0 >= nv || v1 >= nv) return;
    const OverlayPoint e0 = tab[v0], e1 = tab[v1];
    if (!e0.some || !e1.some) return;
    const float mid_x = (e0.sx + e1.sx) / 2.0f, mid_y = (e0.sy + e1.sy) / 2.0f;
    if (!overlay_inside(mid_x, mid_y, rect)) return;
    out[0] = overlay_seg(e0, e1, false, false, OVERLAY_PREVIEW_COLOR);
    out[1] = overlay_seg(e0, e1, true, false, OVERLAY_PREVIEW_COLOR);
}
// :1960-1975, one record
B32_HD B32Prim overlay_hover_vertex(uint32_t v, uint32_t nv, const OverlayPoint* tab) {
    if (v >= nv || !tab[v].some) return prim_noop();
    return overlay_circle(tab[v], 5, OVERLAY_HOVER_COLOR, B32_PRIM_CIRCLE, 255u);
}
// :1980-1992, three records
B32_HD void overlay_hover_edge(uint32_t v0, uint32_t v1, uint32_t nv, const OverlayPoint* tab, B32Prim* out) {
    out[0] = prim_noop(); out[1] = prim_noop(); out[2] = prim_noop();
    if (v0 >= nv || v1 >= nv) return;
    const OverlayPoint e0 = tab[v0], e1 = tab[v1];
    if (!e0.some || !e1.some) return;
    out[0] = overlay_seg(e0, e1, false, false, OVERLAY_HOVER_COLOR);
    out[1] = overlay_seg(e0, e1, true, false, OVERLAY_HOVER_COLOR);
    out[2] = overlay_seg(e0, e1, false, true, OVERLAY_HOVER_COLOR);
}
// :2026-2041, one record
B32_HD B32Prim overlay_selected_vertex(uint32_t v, uint32_t nv, const OverlayPoint* tab) {
    if (v >= nv || !tab[v].some) return prim_noop();
    return overlay_circle(tab[v], 4, OVERLAY_SELECT_COLOR, B32_PRIM_CIRCLE, 255u);
}
// :2048-2061, four records; the pair as given
B32_HD void overlay_selected_edge(uint32_t v0, uint32_t v1, uint32_t nv, const OverlayPoint* tab, B32Prim* out) {
    for (int k = 0; k < 4; ++k) out[k] = prim_noop();
    if (v0 >= nv || v1 >= nv) return;
    const OverlayPoint e0 = tab[v0], e1 = tab[v1];
    if (!e0.some || !e1.some) return;
    out[0] = overlay_seg(e0, e1, false, false, OVERLAY_SELECT_COLOR);
    out[1] = overlay_seg(e0, e1, true, false, OVERLAY_SELECT_COLOR);
    out[2] = overlay_circle(e0, 3, OVERLAY_SELECT_COLOR, B32_PRIM_CIRCLE, 255u);
    out[3] = overlay_circle(e1, 3, OVERLAY_SELECT_COLOR, B32_PRIM_CIRCLE, 255u);
}

// records of a polygon of cnt positions
constexpr uint32_t overlay_polygon_slots(uint32_t mode, uint32_t cnt) {
    return mode == OVERLAY_POLY_HOVER ? cnt + (cnt >= 4u ? 1u : 0u) : (mode == OVERLAY_POLY_SELECTED ? 2u * cnt + 1u : cnt + 1u);
}
// One polygon (pv[0 .. cnt)) of the hovered face (:1997-2020), of the selected faces (:2068-2103) or of the face preview (:2210-2244)
// into its overlay_polygon_slots records at `out`.  The outline is streamed: the first, the third and the previous projected vertex are
// kept, prev -> cur is written as the walk goes and last -> first closes it; fewer than three projected vertices take it back.
// pos / stride: the slot's positions (floats between two vertices).
B32_HD void overlay_polygon(const ViewBlock& a, uint32_t mode, const uint32_t* pv, uint32_t cnt, const float* pos, uint32_t stride, uint32_t nv,
                            const OverlayPoint* tab, const float* rect, B32Prim* out) {
    const uint32_t slots = overlay_polygon_slots(mode, cnt);
    const PrimColor col = mode == OVERLAY_POLY_HOVER ? OVERLAY_HOVER_COLOR : (mode == OVERLAY_POLY_SELECTED ? OVERLAY_SELECT_COLOR : OVERLAY_PREVIEW_COLOR);
    uint32_t k = 0u, n = 0u;
    bool go = true;
    float acc[3] = { 0.0f, 0.0f, 0.0f };             // fold(Vec3::ZERO, |acc, p| acc + p) over get_pos(vi) != None
    uint32_t count = 0u;
    OverlayPoint centre; centre.sx = 0.0f; centre.sy = 0.0f; centre.z = 0.0f; centre.some = 0u;
    if (mode != OVERLAY_POLY_HOVER) {
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t vi = pv[j];
            if (vi >= nv) continue;
            const float* p = pos + (size_t)vi * stride;
            acc[0] = acc[0] + p[0]; acc[1] = acc[1] + p[1]; acc[2] = acc[2] + p[2];
            ++count;
        }
    }
    if (mode == OVERLAY_POLY_PREVIEW) {
        go = count != 0u;
        if (go) {
            const float inv = 1.0f / (float)count;
            const float c[3] = { acc[0] * inv, acc[1] * inv, acc[2] * inv };
            centre = overlay_point(a, c);
            go = centre.some != 0u && overlay_inside(centre.sx, centre.sy, rect);
        }
    }
    OverlayPoint first = centre, third = centre, prev = centre;
    if (go) {
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint32_t vi = pv[j];
            if (vi >= nv) continue;
            const OverlayPoint e = tab[vi];
            if (!e.some) continue;
            if (n == 0u) first = e;
            else {
                out[k++] = overlay_seg(prev, e, false, false, col);
                if (mode == OVERLAY_POLY_SELECTED) out[k++] = overlay_seg(prev, e, true, false, col);
            }
            if (n == 2u) third = e;
            prev = e; ++n;
        }
    }
    if (n >= 3u) {
        out[k++] = overlay_seg(prev, first, false, false, col);
        if (mode == OVERLAY_POLY_SELECTED) {
            out[k++] = overlay_seg(prev, first, true, false, col);
            const float inv = 1.0f / (float)n;      // n = screen_positions.len() (:2088)
            const float c[3] = { acc[0] * inv, acc[1] * inv, acc[2] * inv };
            centre = overlay_point(a, c);
            if (centre.some) out[k++] = overlay_circle(centre, 4, col, B32_PRIM_CIRCLE, 255u);
        } else if (mode == OVERLAY_POLY_PREVIEW) {
            out[k++] = overlay_circle(centre, 4, col, B32_PRIM_CIRCLE, 255u);
        } else if (n >= 4u) {
            out[k++] = overlay_seg(first, third, false, false, col);
        }
    } else {
        k = 0u;
    }
    for (; k < slots; ++k) out[k] = prim_noop();
}

// :1821-1883, bracket k (corner k / 3, direction k % 3) from the finished bounds
B32_HD B32Prim overlay_bracket(const ViewBlock& a, const OverlayBounds& b, uint32_t k) {
    float mn[3], mx[3];
    for (int c = 0; c < 3; ++c) { mn[c] = overlay_unkey(b.mn[c]) - 4.0f; mx[c] = overlay_unkey(b.mx[c]) + 4.0f; }
    const float size[3] = { mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2] };
    const float bracket_len = f32_min(f32_min(size[0], size[1]), size[2]) * 0.25f;
    const uint32_t ci = k / 3u, di = k % 3u;
    const bool hi[3] = { ci == 1u || ci == 2u || ci == 5u || ci == 6u, ci >= 4u, ci == 2u || ci == 3u || ci == 6u || ci == 7u };
    float corner[3], end[3];
    for (uint32_t c = 0; c < 3u; ++c) {
        corner[c] = hi[c] ? mx[c] : mn[c];
        const float dir = c != di ? 0.0f : (hi[c] ? -1.0f : 1.0f);
        end[c] = corner[c] + dir * bracket_len;
    }
    const OverlayPoint e0 = overlay_point(a, corner), e1 = overlay_point(a, end);
    if (!e0.some || !e1.some) return prim_noop();
    return overlay_line(B32_LINE_3D, as_i32(e0.sx), as_i32(e0.sy), as_i32(e1.sx), as_i32(e1.sy), e0.z, e1.z, OVERLAY_BRACKET_COLOR, 255u);
}

// ---- host: the struct's own argument rules (0: fine, else B32_E_ARG) ...
static inline int overlay_check(bool has_topology, const B32MeshOverlay* o, const uint32_t* selected) {
    if ((o->sections & ~OVERLAY_ALL) || o->select_kind > 3u || o->preview_mode > 2u || (o->n_selected && !selected)) return B32_E_ARG;
    const bool polygons = (o->sections & B32_OVERLAY_EDGES) || ((o->sections & B32_OVERLAY_HOVER) && o->hover_face != OVERLAY_NONE) ||
                          ((o->sections & B32_OVERLAY_SELECTED) && o->select_kind == 3u && o->n_selected) ||
                          ((o->sections & B32_OVERLAY_PREVIEW) && o->preview_mode != 0u);
    return (polygons && !has_topology) ? B32_E_ARG : B32_OK;
}
// ... and where the sections lie: first record of every section, and the total
struct OverlayLayout {
    uint64_t brackets, edges, dots, hover_vertex, hover_edge, hover_face, selected, preview, total;
    uint32_t hover_face_cnt;                        // positions of the hovered polygon (0: none or out of range)
};
// poly_start: the topology's host copy (nullptr: no topology -- the caller has checked that no section reads polygons); ne: its distinct
// edges; selected: the list (polygons: indices >= np take no records)
static inline OverlayLayout overlay_layout(const uint32_t* poly_start, uint32_t np, uint32_t nh, uint32_t ne, uint32_t nv, const B32MeshOverlay& o,
                                           const uint32_t* selected) {
    OverlayLayout l{};
    uint64_t at = 0;
    l.brackets = at; if ((o.sections & B32_OVERLAY_BRACKETS) && nv) at += 24u;
    l.edges = at; if (o.sections & B32_OVERLAY_EDGES) at += nh;
    l.dots = at; if (o.sections & B32_OVERLAY_DOTS) at += nv;
    l.hover_vertex = l.hover_edge = l.hover_face = at;
    if (o.sections & B32_OVERLAY_HOVER) {
        if (o.hover_vertex != OVERLAY_NONE) at += 1u;
        l.hover_edge = at;
        if (o.hover_edge_v0 != OVERLAY_NONE || o.hover_edge_v1 != OVERLAY_NONE) at += 3u;
        l.hover_face = at;
        if (o.hover_face != OVERLAY_NONE && poly_start && o.hover_face < np) {
            l.hover_face_cnt = poly_start[o.hover_face + 1u] - poly_start[o.hover_face];
            at += overlay_polygon_slots(OVERLAY_POLY_HOVER, l.hover_face_cnt);
        }
    }
    l.selected = at;
    if (o.sections & B32_OVERLAY_SELECTED) {
        if (o.select_kind == 1u) at += o.n_selected;
        else if (o.select_kind == 2u) at += 4ull * o.n_selected;
        else if (o.select_kind == 3u && poly_start)
            for (uint32_t i = 0; i < o.n_selected; ++i)
                if (selected[i] < np) at += overlay_polygon_slots(OVERLAY_POLY_SELECTED, poly_start[selected[i] + 1u] - poly_start[selected[i]]);
    }
    l.preview = at;
    if (o.sections & B32_OVERLAY_PREVIEW) {
        if (o.preview_mode == 0u) at += nv;
        else if (o.preview_mode == 1u) at += 2ull * ne;
        else at += (uint64_t)nh + np;
    }
    l.total = at;
    return l;
}

}  // namespace b32
