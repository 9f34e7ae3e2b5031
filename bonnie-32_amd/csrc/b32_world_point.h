// b32_world_point.h -- the reference's world_to_screen family (math.rs:503-652) for one point, and the camera block it reads (ViewBlock,
// filled by view_fill), shared by everything that projects world positions on the device: k_world_project (b32_world.hip),
// k_gizmo_project (b32_gizmo.hip), the overlay kernels (b32_overlay.hip), the pick, the hover and the box selections (b32_pick_body.h)
// and the room queries (b32_room_body.h).  f32, no contraction, the reference's order.  The text also compiles for the host (B32_HD):
// the tests build the *_body.h headers, which project through it, into host programs that fill the block with the same view_fill.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define B32_HD __device__ __forceinline__
#else
#define B32_HD static inline
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

}  // namespace b32
