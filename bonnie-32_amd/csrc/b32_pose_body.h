// b32_pose_body.h -- the modeler's per-vertex skinning for one vertex: rotate_by_euler(v.pos, bone_rot) + bone_pos (modeler/state.rs:30-54;
// the draw, the box selection, the selection brackets and the hover of modeler/viewport.rs all evaluate this one expression) with the
// bone's cos / sin taken on the host (B32Bone).  k_pose (b32_pose.hip) runs it once per vertex and change of the bone table; the text
// also compiles for the host (B32_HD, b32_world_point.h), where tests/test_pose.py drives it vertex by vertex against the Python mirror,
// built with and without -ffp-contract=off.  Every expression is a separately rounded f32 operation in the reference's order.
#pragma once
#if defined(__HIPCC__)
#include "b32_device.h"
#define B32_HD __device__ __forceinline__
#else
#include <stdint.h>
#include "../../include/b32raster.h"
#define B32_HD static inline
#endif

namespace b32 {

// the rotating branch of rotate_by_euler, state.rs:43-53: X rotation first, then Z
B32_HD void pose_rotate(const B32Bone& bn, const float* v, float* out) {
    const float y1 = v[1] * bn.cos_x + v[2] * bn.sin_x;
    const float z1 = (-v[1]) * bn.sin_x + v[2] * bn.cos_x;
    const float x2 = v[0] * bn.cos_z + y1 * bn.sin_z;
    const float y2 = (-v[0]) * bn.sin_z + y1 * bn.cos_z;
    out[0] = x2; out[1] = y2; out[2] = z1;
}

// One vertex: rest = (position, normal), 6 floats; out likewise.  bone == nullptr is bone_transforms.get(idx) == None: the rest values
// as they are.  A bone whose rotation takes rotate_by_euler's early return only translates (x + bx: a -0.0 becomes +0.0) and leaves the
// normal alone.  The normal is rotated without the translation and not renormalised.
B32_HD void pose_vertex(const B32Bone* bone, const float* rest, float* out) {
    if (!bone) {
        for (int k = 0; k < 6; ++k) out[k] = rest[k];
        return;
    }
    const B32Bone& bn = *bone;
    if (bn.rotate == 0u) {
        out[0] = rest[0] + bn.pos[0]; out[1] = rest[1] + bn.pos[1]; out[2] = rest[2] + bn.pos[2];
        out[3] = rest[3]; out[4] = rest[4]; out[5] = rest[5];
        return;
    }
    float r[3];
    pose_rotate(bn, rest, r);
    out[0] = r[0] + bn.pos[0]; out[1] = r[1] + bn.pos[1]; out[2] = r[2] + bn.pos[2];
    pose_rotate(bn, rest + 3, out + 3);
}

}  // namespace b32
