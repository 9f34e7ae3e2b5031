// b32_prim_record.h -- the rules that decide what a B32Prim record is, once for every producer of records: k_world_project
// (b32_world_body.h), k_gizmo_project (b32_gizmo_body.h), the mesh overlay (b32_overlay_body.h), the room overlay
// (b32_room_overlay_body.h) and the host's check of caller-made records (b32_draw_lines / b32_draw_prims, b32_api.hip).  The reference's
// casts and f32 helpers, the limit of its i32 arithmetic, the record that draws nothing and the constructors of a circle, a line and a
// thick-line record.  The constructors fill records only: what an item beyond the limit MEANS (a silent no-op, outcome 2, a tally) is
// its caller's business -- the caller asks prim_big / prim_wide first.  The text compiles for the host too (B32_HD, b32_world_point.h).
#pragma once
#if defined(__HIPCC__)
#include "b32_device.h"
#else
#include "b32_world_point.h"
#endif

namespace b32 {

// Rust's `f as i32`: NaN -> 0, saturating, truncation toward zero
B32_HD int32_t as_i32(float f) {
#if defined(__HIPCC__)
    return f2i32_sat(f);
#else
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return (int32_t)f;
#endif
}
B32_HD int32_t inc_wrap(int32_t v) { return (int32_t)((uint32_t)v + 1u); }              // `+ 1` of a release build: wraps
// f32::min / f32::max: a NaN loses (constexpr: host and device -- the layouts call them from host code of the library)
constexpr float f32_min(float a, float b) { return a != a ? b : (b != b ? a : (b < a ? b : a)); }
constexpr float f32_max(float a, float b) { return a != a ? b : (b != b ? a : (b > a ? b : a)); }
B32_HD float bits_f32(uint32_t v) { float f; __builtin_memcpy(&f, &v, 4); return f; }
B32_HD uint32_t f32_bits(float f) { uint32_t v; __builtin_memcpy(&v, &f, 4); return v; }
// a record's depth: a NaN as the one quiet NaN (payloads are unspecified, and every NaN fails every depth test alike)
B32_HD float prim_depth(float z) { return z != z ? bits_f32(0x7FC00000u) : z; }

// What the reference's i32 arithmetic cannot carry (2 * err of a line, render.rs:735, 800; cy +- radius of a circle, :632-637;
// x0 + ox, y2 - y0 of the gizmos): a coordinate is too big, an extent v - u is too wide, when it reaches 2^30 (constexpr: b32_draw_lines
// and b32_draw_prims ask the same of caller-made records on the host).
constexpr long long PRIM_LIM = 1ll << 30;
constexpr bool prim_big(int32_t v) { return (long long)v >= PRIM_LIM || (long long)v <= -PRIM_LIM; }
constexpr bool prim_wide(int32_t u, int32_t v) { return (long long)v - u >= PRIM_LIM || (long long)v - u <= -PRIM_LIM; }

struct PrimColor { uint8_t r, g, b, blend = B32_BLEND_OPAQUE; };                      // RasterColor; three values: RasterColor::new

B32_HD B32Prim prim_noop() {                        // draws nothing: a circle of radius -1 (PrimPass::bounds)
    B32Prim o{};
    o.kind = B32_PRIM_CIRCLE; o.size = -1;
    return o;
}
// fb.draw_circle[_alpha](x, y, radius, colour)
B32_HD B32Prim prim_circle(uint32_t kind, int32_t x, int32_t y, int32_t radius, PrimColor c, uint32_t alpha) {
    B32Prim o{};
    o.x0 = x; o.y0 = y; o.size = radius;
    o.r = c.r; o.g = c.g; o.b = c.b; o.blend = c.blend;
    o.kind = (uint8_t)kind; o.alpha = (uint8_t)alpha;
    return o;
}
// fb.draw_line and its kin between cast ends; z0, z1 are kept by the depth kinds (draw_line_3d[_overlay / _alpha]) and 0 otherwise
B32_HD B32Prim prim_line(uint32_t kind, int32_t x0, int32_t y0, int32_t x1, int32_t y1, float z0, float z1, PrimColor c, uint32_t alpha) {
    B32Prim o{};
    const bool depth = kind >= B32_LINE_3D && kind <= B32_LINE_3D_ALPHA;
    o.x0 = x0; o.y0 = y0; o.x1 = x1; o.y1 = y1;
    o.z0 = depth ? prim_depth(z0) : 0.0f; o.z1 = depth ? prim_depth(z1) : 0.0f;
    o.r = c.r; o.g = c.g; o.b = c.b; o.blend = c.blend;
    o.kind = (uint8_t)kind; o.alpha = (uint8_t)alpha;
    return o;
}
// fb.draw_thick_line(x0, y0, x1, y1, thickness, colour)
B32_HD B32Prim prim_thick_line(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t thickness, PrimColor c, uint32_t alpha) {
    B32Prim o = prim_line(B32_PRIM_THICK_LINE, x0, y0, x1, y1, 0.0f, 0.0f, c, alpha);
    o.size = thickness;
    return o;
}

}  // namespace b32
