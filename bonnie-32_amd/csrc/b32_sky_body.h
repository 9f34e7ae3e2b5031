// b32_sky_body.h -- what the two vertex kernels of the sky share (k_sky_project, b32_sky.hip; k_sky_place_project,
// b32_sky_resident.hip): the screen point of a vertex from its position RELATIVE to the camera.
#pragma once
#include "b32_device.h"

namespace b32 {

// perspective_transform (math.rs:103-109) + project (math.rs:117-136) into *out; behind the camera -> NaN marker (render.rs:99-103)
__device__ __forceinline__ void sky_screen_point(float rx, float ry, float rz, const B32Camera& cam, uint32_t width, uint32_t height, float2* __restrict__ out) {
    const float cx = rx * cam.basis_x[0] + ry * cam.basis_x[1] + rz * cam.basis_x[2];
    const float cy = rx * cam.basis_y[0] + ry * cam.basis_y[1] + rz * cam.basis_y[2];
    const float cz = rx * cam.basis_z[0] + ry * cam.basis_z[1] + rz * cam.basis_z[2];
    const float qnan = __uint_as_float(0x7FC00000u);
    if (cz <= 0.1f) { *out = make_float2(qnan, qnan); return; }
    const uint32_t mn = width < height ? width : height;
    const float vs = ((float)mn / 2.0f) * 0.75f;
    const float denom = cz + 5.0f;
    if (__builtin_fabsf(denom) < 0.001f) { *out = make_float2((float)width / 2.0f, (float)height / 2.0f); return; }
    *out = make_float2((cx * 4.0f) / denom * vs + ((float)width / 2.0f), (cy * 4.0f) / denom * vs + ((float)height / 2.0f));
}

}  // namespace b32
