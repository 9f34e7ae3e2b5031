// b32_pick_body.h -- what b32_pick.hip (b32_pick_meshes), b32_hover.hip (b32_hover_mesh, b32_box_select) and b32_room.hip (b32_room_hover,
// b32_room_box_select) share.  On the device: the body of the reference's triangle loops for one triangle, the reduction of the three
// minima (b32_pick_words.h) in a workgroup and their offer to memory, the bitmap tail of a box selection.  On the host: the ring of device
// result buffers whose content leaves through a ticket, and the blocking forms' landing buffer.  See b32_pick.hip for the why.
#pragma once
#include "b32_host.h"
#include "b32_pick_words.h"

namespace b32 {

// What the pick, the hover and the mesh box selection hand their kernels in common (PickArgs, HoverArgs, BoxArgs add their own).
struct QueryArgs {
    ViewBlock v;                                // camera and projection constants
    float mx, my; uint32_t cull;                // the cursor (unused by the box selection); back-face culling, for the hover "not SEE_THROUGH"
    unsigned char* result;                      // the call's device result buffer (pick_result_open), whose layout is the call's:
                                                //   pick   {int32 best; uint32 n; 8 bytes of padding} + n * sizeof(B32PickHit)
                                                //   hover  one B32HoverResult
                                                //   box    {uint32 n_elements; uint32 n_selected; 8 bytes of padding} + ceil(n_elements / 32) words
};
struct PickArgs {
    QueryArgs q;
    uint32_t n;                                 // entries of the table
    const PickItem* table;                      // nullptr = the table is the kernel argument
    PickWords* words;                           // n entries, all ones between two picks
};
constexpr size_t BOX_HEADER = 16;               // {uint32 n_elements; uint32 n_selected; 8 bytes of padding} in front of a box selection's words

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
__device__ __forceinline__ bool pick_triangle_idx(const QueryArgs& a, const PickItem& it, bool placed, const uint32_t* idx, float& depth) {
    if (idx[0] >= it.nv || idx[1] >= it.nv || idx[2] >= it.nv) return false;            // screen_verts.get(..) == None
    const bool ortho = a.v.has_ortho != 0u;
    float sx[3], sy[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float local[3], world[3];
        pick_vertex(it, placed, idx[k], local, world);
        if (!world_point(a.v, world, ortho, sx[k], sy[k], d[k])) return false;
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
__device__ __forceinline__ bool pick_triangle(const QueryArgs& a, const PickItem& it, uint32_t t, float& depth) {
    const uint32_t* fv = it.faces[t].v;
    const uint32_t idx[3] = { fv[0], fv[1], fv[2] };
    return pick_triangle_idx(a, it, true, idx, depth);
}

// The workgroup's minima in thread 0 (256 lanes): shuffles in the wave, then the four waves through LDS.
__device__ __forceinline__ PickWords pick_reduce(PickWords m) {
    __shared__ PickWords part[4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        PickWords o;
        o.key = __shfl_xor(m.key, off); o.first = __shfl_xor(m.first, off); o.first_nan = __shfl_xor(m.first_nan, off);
        pick_fold(m, o);
    }
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (int k = 1; k < 4; ++k) pick_fold(m, part[k]);
    }
    return m;
}
// A workgroup's minima offered to the words in memory: nothing without a hit, else at most one agent-scope atomic per word.
__device__ __forceinline__ void pick_offer(const PickWords& m, PickWords* w) {
    if (m.first == PICK_NONE) return;
    __hip_atomic_fetch_min(&w->first, m.first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (m.first_nan != PICK_NONE) __hip_atomic_fetch_min(&w->first_nan, m.first_nan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (m.key != ~0ull) __hip_atomic_fetch_min(&w->key, m.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The tail of a box selection's kernel (256 lanes, lane i decides element i; the lanes behind n_elements pass false): a wave's ballot is
// two words of the bitmap behind the header, its popcount is added to n_selected (zero when the kernel starts), lane 0 writes n_elements.
__device__ __forceinline__ void box_emit(unsigned char* result, uint32_t i, uint32_t n_elements, uint32_t nwords, bool sel) {
    const unsigned long long b = __ballot(sel);
    uint32_t* head = reinterpret_cast<uint32_t*>(result);
    if ((threadIdx.x & 63u) == 0u) {                                                     // (i is a multiple of 64 here)
        uint32_t* words = head + BOX_HEADER / 4;
        const uint32_t wd = i >> 5;
        if (wd < nwords) words[wd] = (uint32_t)b;
        if (wd + 1u < nwords) words[wd + 1u] = (uint32_t)(b >> 32);
        const uint32_t cnt = (uint32_t)__popcll(b);
        if (cnt) __hip_atomic_fetch_add(&head[1], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (i == 0u) head[0] = n_elements;
}

// camera, projection constants and cursor of a call (checked arguments)
static inline void query_fill(QueryArgs& a, const b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, float mx, float my, bool cull) {
    view_fill(a.v, *cam, c->width, c->height, ortho);
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
// A blocking form (checked arguments): the landing buffer, the async form into it (enqueue(out, &ticket)), the wait.  *landed: the
// result's `bytes`, valid until the next blocking form.
template <class Enqueue>
static inline int pick_blocking(b32_ctx* c, size_t bytes, const unsigned char** landed, Enqueue enqueue) {
    int rc;
    if ((rc = pick_host_ensure(c, bytes))) return rc;
    uint64_t t = 0;
    if ((rc = enqueue(c->pick_host, &t))) return rc;
    if ((rc = b32_ticket_wait(c, t))) return rc;
    *landed = static_cast<const unsigned char*>(c->pick_host);
    return B32_OK;
}

// A box selection's async form around its kernel: the result buffer into *result with the header zeroed on the stream, the caller's
// launch() (which reads *result), the delivery of header and words.
static inline size_t box_bytes(size_t nwords) { return BOX_HEADER + nwords * 4u; }
template <class Launch>
static inline int box_run(b32_ctx* c, uint32_t nwords, unsigned char** result, void* out, uint64_t* ticket, Launch launch) {
    unsigned long long t = 0; hipEvent_t* tev = nullptr; uint32_t k = 0;
    const size_t bytes = box_bytes(nwords);
    int rc;
    if ((rc = pick_result_open(c, bytes, t, tev, k, result))) return rc;
    HIPCHK(c, hipMemsetAsync(*result, 0, BOX_HEADER, c->stream));
    launch();
    HIPCHK(c, hipGetLastError());
    return pick_result_deliver(c, k, bytes, out, t, tev, ticket);
}
// ... and its blocking form's way out of the landing buffer (words: nullable)
static inline void box_landed(const unsigned char* h, size_t nwords, uint32_t* words, uint32_t* n_selected) {
    std::memcpy(n_selected, h + 4, 4);
    if (words && nwords) std::memcpy(words, h + BOX_HEADER, nwords * 4u);
}

}  // namespace b32
