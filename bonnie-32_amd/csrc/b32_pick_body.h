// b32_pick_body.h -- what b32_pick.hip (b32_pick_meshes) and b32_hover.hip (b32_hover_mesh, b32_box_select) share: the body of the
// reference's triangle loops for one triangle, the three minima that stand for "closest in loop order" and their reduction in a
// workgroup, and on the host the ring of device result buffers whose content leaves through a ticket.  See b32_pick.hip for the why.
#pragma once
#include "b32_host.h"
#include "b32_world_point.h"

namespace b32 {

constexpr uint32_t PICK_CHUNK = 1024;           // elements per workgroup: 256 lanes, four trips
constexpr uint32_t PICK_NONE = 0xFFFFFFFFu;
constexpr uint32_t PICK_QNAN = 0x7FC00000u;     // the one NaN a NaN depth is reported as (as b32_draw_world's records)

struct PickWords { unsigned long long key; uint32_t first, first_nan; };
// What the pick, the hover and the box selection hand their kernels in common.  The hover and the box selection (HoverArgs, BoxArgs in
// b32_hover.hip) use w, mx, my, cull and result, and keep their own element counts and words.
struct PickArgs {
    WorldArgs w;                                // camera and projection constants (items / out / counts unused)
    float mx, my; uint32_t cull;                // the cursor (unused by the box selection); back-face culling, for the hover "not SEE_THROUGH"
    uint32_t n;                                 // pick: entries of the table
    const PickItem* table;                      // pick: nullptr = the table is the kernel argument
    PickWords* words;                           // pick: n entries, all ones between two picks (the hover's are HoverArgs::words)
    unsigned char* result;                      // the call's device result buffer (pick_result_open), whose layout is the call's:
                                                //   pick   {int32 best; uint32 n; 8 bytes of padding} + n * sizeof(B32PickHit)
                                                //   hover  one B32HoverResult
                                                //   box    {uint32 n_elements; uint32 n_selected; 8 bytes of padding} + ceil(n_elements / 32) words
};

// total order of the non-NaN f32 as u32, both zeros on one value
__device__ __forceinline__ uint32_t pick_orderable(float d) {
    uint32_t u = __float_as_uint(d);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Vertex i (< it.nv) of an item: its local position, and the position the loops project -- placed (viewport_3d.rs:7716-7718) or, for
// the modeler without a placement, as it is.
__device__ __forceinline__ void pick_vertex(const PickItem& it, bool placed, uint32_t i, float* local, float* world) {
    const float* p = it.pos12 ? it.pos12 + (size_t)i * 3 : it.verts[i].pos;
    const float x = p[0], y = p[1], z = p[2];
    local[0] = x; local[1] = y; local[2] = z;
    if (placed) {
        const float rx = x * it.cos_f - z * it.sin_f;
        const float rz = x * it.sin_f + z * it.cos_f;
        world[0] = rx + it.wpos[0]; world[1] = y + it.wpos[1]; world[2] = rz + it.wpos[2];
    } else { world[0] = x; world[1] = y; world[2] = z; }
}

// The triangle (idx[0], idx[1], idx[2]) of an item through the body of the reference's loops: false = skipped or missed, true = hit
// with `depth`.
__device__ __forceinline__ bool pick_triangle_idx(const PickArgs& a, const PickItem& it, bool placed, const uint32_t* idx, float& depth) {
    if (idx[0] >= it.nv || idx[1] >= it.nv || idx[2] >= it.nv) return false;            // screen_verts.get(..) == None
    const bool ortho = a.w.has_ortho != 0u;
    float sx[3], sy[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float local[3], world[3];
        pick_vertex(it, placed, idx[k], local, world);
        if (!world_point(a.w, world, ortho, sx[k], sy[k], d[k])) return false;
    }
    const float px = a.mx, py = a.my;
    const float area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sx[2] - sx[0]) * (sy[1] - sy[0]);
    if (a.cull && area <= 0.0f) return false;                                           // modeler/viewport.rs:2571-2574 (a NaN area is kept)
    // point_in_triangle_2d, math.rs:687-706: sign(p, a, b) = (px - bx) * (ay - by) - (ax - bx) * (py - by)
    const float d1 = (px - sx[1]) * (sy[0] - sy[1]) - (sx[0] - sx[1]) * (py - sy[1]);
    const float d2 = (px - sx[2]) * (sy[1] - sy[2]) - (sx[1] - sx[2]) * (py - sy[2]);
    const float d3 = (px - sx[0]) * (sy[2] - sy[0]) - (sx[2] - sx[0]) * (py - sy[0]);
    const bool has_neg = (d1 < 0.0f) || (d2 < 0.0f) || (d3 < 0.0f);
    const bool has_pos = (d1 > 0.0f) || (d2 > 0.0f) || (d3 > 0.0f);
    if (has_neg && has_pos) return false;
    // interpolate_depth_in_triangle, viewport_3d.rs:7485-7508
    if (fabsf(area) < 0.0001f) { depth = ((d[0] + d[1]) + d[2]) / 3.0f; return true; }
    const float w0 = ((sx[1] - px) * (sy[2] - py) - (sx[2] - px) * (sy[1] - py)) / area;
    const float w1 = ((sx[2] - px) * (sy[0] - py) - (sx[0] - px) * (sy[2] - py)) / area;
    const float w2 = (1.0f - w0) - w1;
    depth = (w0 * d[0] + w1 * d[1]) + w2 * d[2];
    return true;
}
// Triangle t of an item's face list, placed.
__device__ __forceinline__ bool pick_triangle(const PickArgs& a, const PickItem& it, uint32_t t, float& depth) {
    const uint32_t* fv = it.faces[t].v;
    const uint32_t idx[3] = { fv[0], fv[1], fv[2] };
    return pick_triangle_idx(a, it, true, idx, depth);
}

// One hit into a lane's three minima; `id` is the triangle (k_pick, k_hover) or the item (k_pick_resolve).
__device__ __forceinline__ void pick_take(PickWords& m, float depth, uint32_t id) {
    m.first = min(m.first, id);
    if (depth != depth) m.first_nan = min(m.first_nan, id);
    else m.key = min(m.key, ((unsigned long long)pick_orderable(depth) << 32) | id);
}
// The workgroup's minima in thread 0 (256 lanes): shuffles in the wave, then the four waves through LDS.
__device__ __forceinline__ PickWords pick_reduce(PickWords m) {
    __shared__ PickWords part[4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        m.key = min(m.key, __shfl_xor(m.key, off));
        m.first = min(m.first, __shfl_xor(m.first, off));
        m.first_nan = min(m.first_nan, __shfl_xor(m.first_nan, off));
    }
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            m.key = min(m.key, part[k].key); m.first = min(m.first, part[k].first); m.first_nan = min(m.first_nan, part[k].first_nan);
        }
    }
    return m;
}
__device__ __forceinline__ PickWords pick_no_hit() { PickWords m; m.key = ~0ull; m.first = PICK_NONE; m.first_nan = PICK_NONE; return m; }

// camera, projection constants and cursor of a call (checked arguments)
static inline void pick_fill_args(PickArgs& a, const b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, float mx, float my, bool cull) {
    for (int k = 0; k < 3; ++k) { a.w.pos[k] = cam->position[k]; a.w.bx[k] = cam->basis_x[k]; a.w.by[k] = cam->basis_y[k]; a.w.bz[k] = cam->basis_z[k]; }
    a.w.vs = ((float)(c->width < c->height ? c->width : c->height) / 2.0f) * 0.75f;     // math.rs:642-643
    a.w.half_w = (float)c->width / 2.0f; a.w.half_h = (float)c->height / 2.0f;
    if (ortho) { a.w.has_ortho = 1u; a.w.zoom = ortho->zoom; a.w.center_x = ortho->center_x; a.w.center_y = ortho->center_y; }
    a.mx = mx; a.my = my; a.cull = cull ? 1u : 0u;
}

// The ticket (shared with b32_fb_download_async: at most DL_RING outstanding) and the device result buffer of a call: PICK_RING buffers in
// turn, each written again only behind the transfer that last read it.  The caller's kernels write `bytes` into *res on the stream.
static inline int pick_result_open(b32_ctx* c, size_t bytes, unsigned long long& t, hipEvent_t*& tev, uint32_t& k, unsigned char** res) {
    int rc;
    if ((rc = ticket_open(c, t, tev))) return rc;
    k = c->pick_slot;
    c->pick_slot = (k + 1) % b32_ctx::PICK_RING;
    if (!c->pick_left[k]) {
        HIPCHK(c, hipEventCreateWithFlags(&c->pick_left[k], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->pick_done[k], hipEventDisableTiming));
    } else if (bytes > c->pick_cap_res[k]) {
        HIPCHK(c, hipEventSynchronize(c->pick_left[k]));
    } else {
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->pick_left[k], 0));
    }
    if (bytes > c->pick_cap_res[k]) {
        if (c->pick_res[k]) HIPCHK(c, hipFree(c->pick_res[k]));
        c->pick_res[k] = nullptr; c->pick_cap_res[k] = 0;
        const size_t cap = bytes + bytes / 4 + 1024;
        HIPCHK(c, hipMalloc(&c->pick_res[k], cap));
        c->pick_cap_res[k] = cap;
    }
    *res = static_cast<unsigned char*>(c->pick_res[k]);
    return B32_OK;
}
// Delivery: the copy leaves on dl_stream behind the kernels enqueued so far, the ticket completes on it (as in b32_fb_download_async).
static inline int pick_result_deliver(b32_ctx* c, uint32_t k, size_t bytes, void* out, unsigned long long t, hipEvent_t* tev, uint64_t* ticket) {
    HIPCHK(c, hipEventRecord(c->pick_done[k], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->dl_stream, c->pick_done[k], 0));
    HIPCHK(c, hipMemcpyAsync(out, c->pick_res[k], bytes, hipMemcpyDeviceToHost, c->dl_stream));
    HIPCHK(c, hipEventRecord(c->pick_left[k], c->dl_stream));
    HIPCHK(c, hipEventRecord(*tev, c->dl_stream));
    c->dl_seq = t; *ticket = t;
    return B32_OK;
}
// the blocking forms' page-locked landing buffer
static inline int pick_host_ensure(b32_ctx* c, size_t bytes) {
    if (bytes <= c->pick_cap_host) return B32_OK;
    if (c->pick_host) HIPCHK(c, hipHostFree(c->pick_host));
    c->pick_host = nullptr; c->pick_cap_host = 0;
    const size_t cap = bytes + bytes / 4 + 1024;
    HIPCHK(c, hipHostMalloc(&c->pick_host, cap, hipHostMallocDefault));
    c->pick_cap_host = cap;
    return B32_OK;
}

}  // namespace b32
