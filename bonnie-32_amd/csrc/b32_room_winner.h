// b32_room_winner.h -- the closing rule of find_hovered_elements (editor/viewport_3d.rs:7283-7336) for one B32RoomHover, for host and
// device (B32_HD): b32_room_hover_winner (b32_room.hip) answers with it on the host, k_room_overlay (b32_room_overlay.hip) on the device
// for a hover that never left it.  Candidates are pushed as (depth, type) in the order vertex, edge, face; sort_by(partial_cmp, a NaN
// compares Equal) -- for so few elements the standard library's stable insertion sort, which is what this is; tolerance = closest * 0.01;
// the lowest type within the tolerance, else the closest one's type.  0 vertex, 1 edge, 2 face, -1 nothing.
#pragma once
#if defined(__HIPCC__)
#include "b32_device.h"
#else
#include <math.h>
#include "b32_world_point.h"
#endif
// (B32_HD is device-only under hipcc; this one function is also the host's b32_room_hover_winner)
#if defined(__HIPCC__)
#define B32_HD_BOTH __host__ __device__ __forceinline__
#else
#define B32_HD_BOTH static inline
#endif

namespace b32 {

B32_HD_BOTH int room_hover_winner(const B32RoomHover& h) {
    // (three scalars, not arrays, and no closure over them: the insertion sort of at most three elements written out, so that nothing is
    // indexed or addressed at run time and the device keeps it in registers)
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f; int t0 = -1, t1 = -1, t2 = -1; int n = 0;
    if (h.vertex_rec != 0xFFFFFFFFu) { d0 = h.vertex_depth; t0 = 0; n = 1; }
    if (h.edge_rec != 0xFFFFFFFFu) {
        const float d = h.edge_depth;
        if (n == 0) { d0 = d; t0 = 1; }
        else if (d < d0) { d1 = d0; t1 = t0; d0 = d; t0 = 1; }
        else { d1 = d; t1 = 1; }
        ++n;
    }
    if (h.face_rec != 0xFFFFFFFFu) {
        const float d = h.face_depth;
        if (n == 0) { d0 = d; t0 = 2; }
        else if (n == 1) {
            if (d < d0) { d1 = d0; t1 = t0; d0 = d; t0 = 2; } else { d1 = d; t1 = 2; }
        } else if (d < d1) {
            d2 = d1; t2 = t1;
            if (d < d0) { d1 = d0; t1 = t0; d0 = d; t0 = 2; } else { d1 = d; t1 = 2; }
        } else { d2 = d; t2 = 2; }
        ++n;
    }
    if (!n) return -1;
    const float closest = d0;
    const float tolerance = closest * 0.01f;
    int best = -1;
    if (fabsf(d0 - closest) < tolerance) best = t0;
    if (n > 1 && fabsf(d1 - closest) < tolerance && (best < 0 || t1 < best)) best = t1;
    if (n > 2 && fabsf(d2 - closest) < tolerance && (best < 0 || t2 < best)) best = t2;
    return best >= 0 ? best : t0;
}

}  // namespace b32
