// b32_world_point.h -- the reference's world_to_screen family (math.rs:503-652) for one point, the near-plane clip of a world segment
// (draw.rs:19-42) and the camera block they read (ViewBlock, filled by view_fill), shared by everything that projects world positions
// on the device: the four producers of B32Prim records (b32_world_body.h, b32_gizmo_body.h, b32_overlay_body.h,
// b32_room_overlay_body.h -- what they share about the RECORDS is b32_prim_record.h), the pick, the hover and the box selections
// (b32_pick_body.h) and the room queries (b32_room_body.h).  f32, no contraction, the reference's order.  The text also compiles for the
// host (B32_HD): the tests build the *_body.h headers, which project through it, into host programs that fill the block with the same
// view_fill.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define B32_HD __device__ __forceinline__
#define B32_UNROLL _Pragma("unroll")
#else
#define B32_HD static inline
#define B32_UNROLL
#endif
#include <stdint.h>
#include "../../include/b32raster.h"

namespace b32 {

constexpr float WORLD_NEAR = 0.1f;                  // NEAR_PLANE, math.rs:155; the `cam_z <= 0.1` of math.rs:516, 560, 602, 634

// The camera block of a call: what world_point reads.  has_ortho == 0: perspective only, the ortho members stay zero.
struct ViewBlock {
    float pos[3], bx[3], by[3], bz[3];              // Camera
    float vs, half_w, half_h;                       // (min(w, h) as f32 / 2.0) * 0.75, w as f32 / 2.0, h as f32 / 2.0 (math.rs:524-531)
    float zoom, center_x, center_y; uint32_t has_ortho;
};
// ... of a camera over a w x h framebuffer; ortho == nullptr: perspective
static inline void view_fill(ViewBlock& v, const B32Camera& cam, uint32_t w, uint32_t h, const B32Ortho* ortho) {
    v = ViewBlock{};
    for (int k = 0; k < 3; ++k) { v.pos[k] = cam.position[k]; v.bx[k] = cam.basis_x[k]; v.by[k] = cam.basis_y[k]; v.bz[k] = cam.basis_z[k]; }
    v.vs = ((float)(w < h ? w : h) / 2.0f) * 0.75f;                         // math.rs:524-525, :642-643
    v.half_w = (float)w / 2.0f; v.half_h = (float)h / 2.0f;
    if (ortho) { v.has_ortho = 1u; v.zoom = ortho->zoom; v.center_x = ortho->center_x; v.center_y = ortho->center_y; }
}

// Vec3::dot, math.rs:23-25
B32_HD float world_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// world_to_screen[_with_depth] (ortho == false) and world_to_screen_with_ortho[_depth], math.rs:503-652: false = None
B32_HD bool world_point(const ViewBlock& a, const float* p, bool ortho, float& sx, float& sy, float& z) {
    const float rel[3] = { p[0] - a.pos[0], p[1] - a.pos[1], p[2] - a.pos[2] };
    const float cam_x = world_dot(rel, a.bx), cam_y = world_dot(rel, a.by), cam_z = world_dot(rel, a.bz);
    z = cam_z;
    if (ortho) {
        sx = (cam_x - a.center_x) * a.zoom + a.half_w;
        sy = -(cam_y - a.center_y) * a.zoom + a.half_h;
        return true;
    }
    if (cam_z <= WORLD_NEAR) return false;
    const float denom = cam_z + 5.0f;               // ud = 5.0, us = ud - 1.0
    sx = (cam_x * 4.0f / denom) * a.vs + a.half_w;
    sy = (cam_y * 4.0f / denom) * a.vs + a.half_h;
    return true;
}

// The near-plane clip of the segment p0 -> p1 in world space, draw.rs:19-42 (viewport_3d.rs:5725-5747 and :5794-5816 are the same text):
// false = both ends behind, nothing to draw; else the end behind the plane is moved onto it.  Whether the moved end still projects can
// hang on the last bit of p0 + (p1 - p0) * t.
B32_HD bool world_near_clip(const ViewBlock& a, float* p0, float* p1) {
    const float rel0[3] = { p0[0] - a.pos[0], p0[1] - a.pos[1], p0[2] - a.pos[2] };
    const float rel1[3] = { p1[0] - a.pos[0], p1[1] - a.pos[1], p1[2] - a.pos[2] };
    const float z0 = world_dot(rel0, a.bz), z1 = world_dot(rel1, a.bz);
    if (z0 <= WORLD_NEAR && z1 <= WORLD_NEAR) return false;
    if (z0 <= WORLD_NEAR || z1 <= WORLD_NEAR) {
        const float t = (WORLD_NEAR - z0) / (z1 - z0);
        float q[3];
        B32_UNROLL
        for (int k = 0; k < 3; ++k) q[k] = p0[k] + (p1[k] - p0[k]) * t;
        B32_UNROLL
        for (int k = 0; k < 3; ++k) { if (z0 <= WORLD_NEAR) p0[k] = q[k]; else p1[k] = q[k]; }
    }
    return true;
}

}  // namespace b32
