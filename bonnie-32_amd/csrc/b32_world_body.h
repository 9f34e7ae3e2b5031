// b32_world_body.h -- the arithmetic of b32_draw_world for one item: draw_3d_line_clipped (rasterizer/draw.rs:12-67) and the modeler's
// world_to_screen_with_ortho[_depth] + fb.draw_* calls (math.rs:538-617).  k_world_project (b32_world.hip) turns an item into its record
// with world_item.  Every expression is a separately rounded f32 operation in the reference's order (b32_world_point.h); what a record
// is, is b32_prim_record.h's.  The text also compiles for the host (B32_HD), where tests/test_world.py runs it against the literal
// restatement.
#pragma once
#include "b32_prim_record.h"

namespace b32 {

// One item into its record at `out`; returns 0 drawn, 1 dropped (the reference draws nothing: the no-op record), 2 rejected (what
// b32_draw_prims answers B32_E_UNSUPPORTED for: the no-op record too).  The record carries the item's size and mode whatever its kind.
B32_HD uint32_t world_item(const ViewBlock& v, const B32WorldItem& it, B32Prim* out) {
    *out = prim_noop();
    const bool circle = it.kind == B32_PRIM_CIRCLE || it.kind == B32_PRIM_CIRCLE_ALPHA;
    float p0[3] = { it.p0[0], it.p0[1], it.p0[2] }, p1[3] = { it.p1[0], it.p1[1], it.p1[2] };
    bool ortho = v.has_ortho != 0u;
    if (!circle && (it.flags & B32_WORLD_CLIP_NEAR)) {          // draw_3d_line_clipped: the projection after the clip takes no ortho
        ortho = false;
        if (!world_near_clip(v, p0, p1)) return 1u;
    }
    float sx0, sy0, cz0, sx1 = 0.0f, sy1 = 0.0f, cz1 = 0.0f;
    if (!world_point(v, p0, ortho, sx0, sy0, cz0)) return 1u;
    if (!circle && !world_point(v, p1, ortho, sx1, sy1, cz1)) return 1u;
    const int32_t x0 = as_i32(sx0), y0 = as_i32(sy0), x1 = as_i32(sx1), y1 = as_i32(sy1);
    if (circle ? (prim_big(x0) || prim_big(y0)) : (prim_wide(x0, x1) || prim_wide(y0, y1))) return 2u;
    const PrimColor col = { it.r, it.g, it.b, it.blend };
    B32Prim o = circle ? prim_circle(it.kind, x0, y0, it.size, col, it.alpha) : prim_line(it.kind, x0, y0, x1, y1, cz0, cz1, col, it.alpha);
    o.size = it.size; o.mode = it.mode;
    *out = o;
    return 0u;
}

}  // namespace b32
