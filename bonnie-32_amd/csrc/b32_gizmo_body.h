// b32_gizmo_body.h -- the arithmetic of the world editor's overlay helpers (editor/viewport_3d.rs:5687-6357) for one item: the screen clip of
// draw_3d_line, the offsets of draw_3d_thick_line_depth, project_vertex of draw_filled_octahedron and a row's span of
// draw_filled_triangle_3d.  k_gizmo_project (b32_gizmo.hip) turns an item into its records with gizmo_item, GizmoPass (b32_prims.hip)
// decides a triangle's pixels with gizmo_tri_sort / gizmo_tri_row.  Every expression is a separately rounded f32 operation in the
// reference's order; the text also compiles for the host (B32_HD, b32_world_point.h), where tests/test_gizmos.py runs it against a
// literal restatement, built with and without -ffp-contract=off.
#pragma once
#if !defined(__HIPCC__)
#include <math.h>
#endif
#include "b32_prim_record.h"

namespace b32 {

constexpr uint32_t PRIM_TRIANGLE = 11u;             // the library-internal record kind of a filled triangle: (x0, y0), (x1, y1) and a third
                                                    // point whose x and y are the bit patterns of z0 and z1.  No entry takes it from the host.
B32_HD float gizmo_sqrt(float x) {
#if defined(__HIPCC__)
    return __builtin_sqrtf(x);
#else
    return sqrtf(x);
#endif
}

// records an item becomes: `size` parallel lines for a thick line of thickness > 1, else one (a no-op where nothing is drawn)
B32_HD uint32_t gizmo_record_count(uint32_t kind, int32_t size) { return (kind == B32_GIZMO_THICK_LINE_DEPTH && size > 1) ? (uint32_t)size : 1u; }

// clip_line_to_rect, viewport_3d.rs:5886-5955: false = None
B32_HD uint32_t gizmo_outcode(float x, float y, float xmin, float ymin, float xmax, float ymax) {
    uint32_t code = 0u;                             // INSIDE; LEFT 1, RIGHT 2, BOTTOM 4, TOP 8 (a NaN fails every comparison: 0)
    if (x < xmin) code |= 1u;
    else if (x >= xmax) code |= 2u;
    if (y < ymin) code |= 8u;
    else if (y >= ymax) code |= 4u;
    return code;
}
B32_HD bool gizmo_clip_line_to_rect(float& x0, float& y0, float& x1, float& y1, float xmin, float ymin, float xmax, float ymax) {
    uint32_t code0 = gizmo_outcode(x0, y0, xmin, ymin, xmax, ymax), code1 = gizmo_outcode(x1, y1, xmin, ymin, xmax, ymax);
    for (int round = 0; round < 16; ++round) {
        if ((code0 | code1) == 0u) return true;
        if ((code0 & code1) != 0u) return false;
        const uint32_t code_out = code0 != 0u ? code0 : code1;
        float x, y;
        if (code_out & 4u) {                        // BOTTOM
            x = x0 + (x1 - x0) * (ymax - 1.0f - y0) / (y1 - y0);
            y = ymax - 1.0f;
        } else if (code_out & 8u) {                 // TOP
            x = x0 + (x1 - x0) * (ymin - y0) / (y1 - y0);
            y = ymin;
        } else if (code_out & 2u) {                 // RIGHT
            y = y0 + (y1 - y0) * (xmax - 1.0f - x0) / (x1 - x0);
            x = xmax - 1.0f;
        } else {                                    // LEFT
            y = y0 + (y1 - y0) * (xmin - x0) / (x1 - x0);
            x = xmin;
        }
        if (code_out == code0) { x0 = x; y0 = y; code0 = gizmo_outcode(x0, y0, xmin, ymin, xmax, ymax); }
        else { x1 = x; y1 = y; code1 = gizmo_outcode(x1, y1, xmin, ymin, xmax, ymax); }
    }
    return false;                                   // failed to converge
}

// draw_3d_thick_line_depth's perpendicular, viewport_3d.rs:5763-5772 (false: len < 0.001), and the offset of line i, :5776-5778
B32_HD bool gizmo_thick_setup(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t thickness, float& px, float& py, float& half) {
    const float dx = (float)(x1 - x0), dy = (float)(y1 - y0);
    const float len = gizmo_sqrt(dx * dx + dy * dy);
    if (len < 0.001f) return false;
    half = (float)thickness * 0.5f;
    px = -dy / len * half;
    py = dx / len * half;
    return true;
}
B32_HD void gizmo_thick_offset(float px, float py, float half, int32_t i, int32_t& ox, int32_t& oy) {
    const float offset = (float)i - half + 0.5f;
    ox = as_i32(px * offset / half);
    oy = as_i32(py * offset / half);
}

// the editor's project_vertex, viewport_3d.rs:6239-6245: perspective_transform (math.rs:103-109), `cam.z < 0.1` -> None, project
// (math.rs:117-136), `as i32`
B32_HD bool gizmo_project_vertex(const ViewBlock& a, const float* p, int32_t& x, int32_t& y) {
    const float rel[3] = { p[0] - a.pos[0], p[1] - a.pos[1], p[2] - a.pos[2] };
    const float cam_x = world_dot(rel, a.bx), cam_y = world_dot(rel, a.by), cam_z = world_dot(rel, a.bz);
    if (cam_z < WORLD_NEAR) return false;
    const float denom = cam_z + 5.0f;               // ud = DISTANCE, us = ud - 1.0
    float sx = a.half_w, sy = a.half_h;
    if (!(fabsf(denom) < 0.001f)) {
        sx = (cam_x * 4.0f) / denom * a.vs + a.half_w;
        sy = (cam_y * 4.0f) / denom * a.vs + a.half_h;
    }
    x = as_i32(sx); y = as_i32(sy);
    return true;
}

// draw_filled_triangle_3d, viewport_3d.rs:6302-6357 (modeler/viewport.rs:4670-4721 is the same text).  The stable sort by y of
// three points (pts.sort_by: ties keep argument order) ...
B32_HD void gizmo_tri_sort(int32_t* x, int32_t* y) {
    auto swap = [&](int i, int j) { const int32_t tx = x[i], ty = y[i]; x[i] = x[j]; y[i] = y[j]; x[j] = tx; y[j] = ty; };
    if (y[1] < y[0]) swap(0, 1);
    if (y[2] < y[1]) { swap(1, 2); if (y[1] < y[0]) swap(0, 1); }
}
// ... and row y of the sorted triangle (y0 <= y <= y2, y2 != y0; coordinates below 2^30): false = the row is skipped, else the span is
// xa.max(0) ..= xb.min(w - 1)
B32_HD bool gizmo_tri_row(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t x2, int32_t y2, int32_t y, int32_t& xa, int32_t& xb) {
    const float total_height = (float)(y2 - y0);
    const bool second_half = y > y1 || y1 == y0;
    const float segment_height = second_half ? (float)(y2 - y1) : (float)(y1 - y0);
    if (segment_height == 0.0f) return false;
    const float alpha = (float)(y - y0) / total_height;
    const float beta = second_half ? (float)(y - y1) / segment_height : (float)(y - y0) / segment_height;
    float ax = (float)x0 + (float)(x2 - x0) * alpha;
    float bx = second_half ? (float)x1 + (float)(x2 - x1) * beta : (float)x0 + (float)(x1 - x0) * beta;
    if (ax > bx) { const float t = ax; ax = bx; bx = t; }
    xa = as_i32(ax); xb = as_i32(bx);
    return true;
}

// One item into its gizmo_record_count(kind, size) records at `out`, in the reference's call order; returns 0 drawn, 1 dropped (the
// reference draws nothing), 2 rejected (the reference's i32 arithmetic cannot carry it: prim_big, prim_wide).  The records carry the
// item's colour and alpha 0.
B32_HD uint32_t gizmo_item(const ViewBlock& a, const B32GizmoItem& it, B32Prim* out) {
    const uint32_t n_rec = gizmo_record_count(it.kind, it.size);
    for (uint32_t k = 0; k < n_rec; ++k) out[k] = prim_noop();
    const PrimColor col = { it.r, it.g, it.b, it.blend };

    if (it.kind <= B32_GIZMO_THICK_LINE_DEPTH) {
        float p0[3] = { it.p0[0], it.p0[1], it.p0[2] }, p1[3] = { it.p1[0], it.p1[1], it.p1[2] };
        if (!world_near_clip(a, p0, p1)) return 1u;     // viewport_3d.rs:5794-5816 and :5725-5747
        float sx0, sy0, cz0, sx1, sy1, cz1;
        if (!world_point(a, p0, false, sx0, sy0, cz0) || !world_point(a, p1, false, sx1, sy1, cz1)) return 1u;
        const bool flat = it.kind == B32_GIZMO_LINE;
        if (flat && !gizmo_clip_line_to_rect(sx0, sy0, sx1, sy1, 0.0f, 0.0f, a.half_w * 2.0f, a.half_h * 2.0f)) return 1u;
        const int32_t x0 = as_i32(sx0), y0 = as_i32(sy0), x1 = as_i32(sx1), y1 = as_i32(sy1);
        if (prim_wide(x0, x1) || prim_wide(y0, y1)) return 2u;
        B32Prim o = prim_line(flat ? B32_LINE_2D : B32_LINE_3D_OVERLAY, x0, y0, x1, y1, cz0, cz1, col, 0u);
        if (n_rec == 1u) {                          // draw_3d_line, draw_3d_line_depth; thickness <= 1
            out[0] = o;
            return 0u;
        }
        if (prim_big(x0) || prim_big(y0) || prim_big(x1) || prim_big(y1)) return 2u;
        float px, py, half;
        if (!gizmo_thick_setup(x0, y0, x1, y1, it.size, px, py, half)) return 1u;
        for (int32_t i = 0; i < it.size; ++i) {
            int32_t ox, oy;
            gizmo_thick_offset(px, py, half, i, ox, oy);
            o.x0 = x0 + ox; o.y0 = y0 + oy; o.x1 = x1 + ox; o.y1 = y1 + oy;
            out[i] = o;
        }
        return 0u;
    }
    if (it.kind == B32_GIZMO_POINT) {               // draw_3d_point, viewport_3d.rs:5958-5976
        float sx, sy, cz;
        if (!world_point(a, it.p0, false, sx, sy, cz)) return 1u;
        const int32_t x = as_i32(sx), y = as_i32(sy);
        if (prim_big(x) || prim_big(y)) return 2u;
        out[0] = prim_circle(B32_PRIM_CIRCLE, x, y, it.size, col, 0u);
        return 0u;
    }
    // the triangles: three projections, any None -> nothing
    int32_t x[3], y[3];
    const float* p[3] = { it.p0, it.p1, it.p2 };
    for (int k = 0; k < 3; ++k) {
        if (it.kind == B32_GIZMO_TRIANGLE) {
            if (!gizmo_project_vertex(a, p[k], x[k], y[k])) return 1u;
        } else {                                    // modeler/viewport.rs:4592-4607
            float sx, sy, cz;
            if (!world_point(a, p[k], a.has_ortho != 0u, sx, sy, cz)) return 1u;
            x[k] = as_i32(sx); y[k] = as_i32(sy);
        }
    }
    for (int k = 0; k < 3; ++k) if (prim_big(x[k]) || prim_big(y[k])) return 2u;
    if (y[0] == y[1] && y[1] == y[2]) return 1u;    // y2 == y0 after the sort
    B32Prim o = prim_line(PRIM_TRIANGLE, x[0], y[0], x[1], y[1], 0.0f, 0.0f, col, 0u);
    o.z0 = bits_f32((uint32_t)x[2]); o.z1 = bits_f32((uint32_t)y[2]);    // the third point
    out[0] = o;
    return 0u;
}

}  // namespace b32
