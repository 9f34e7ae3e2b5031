// b32_world_point.h -- the reference's world_to_screen family (math.rs:503-652) for one point, shared by the kernels that project world
// positions on the device: k_world_project (b32_world.hip), k_gizmo_project (b32_gizmo.hip) and k_pick (b32_pick.hip).  f32, no
// contraction, the reference's order.  The text also compiles for the host (B32_HD; the camera block is whatever struct has WorldArgs's
// members): tests/test_gizmos.py builds b32_gizmo_body.h, which projects through it, into a host program.
#pragma once
#if defined(__HIPCC__)
#include "b32_device.h"
#define B32_HD __device__ __forceinline__
#else
#define B32_HD static inline
#endif

namespace b32 {

constexpr float WORLD_NEAR = 0.1f;                  // NEAR_PLANE, math.rs:155; the `cam_z <= 0.1` of math.rs:516, 560, 602, 634

// Vec3::dot, math.rs:23-25
B32_HD float world_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// world_to_screen[_with_depth] (ortho == false) and world_to_screen_with_ortho[_depth], math.rs:503-652: false = None
template <class A>
B32_HD bool world_point(const A& a, const float* p, bool ortho, float& sx, float& sy, float& z) {
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
