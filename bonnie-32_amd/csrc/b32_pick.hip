// b32_pick.hip -- "what is under the cursor?" for placed resident meshes (b32_pick_meshes[_async]).
//
// Reference: check_mesh_hit (editor/viewport_3d.rs:7700-7756), called once per visible part of every enabled object of every room
// (:7344-7400), and the face branch of the modeler's find_hovered_element (modeler/viewport.rs:2544-2594).  Both rotate and translate
// every local vertex, project it (world_to_screen_with_depth / world_to_screen_with_ortho), test every triangle with
// point_in_triangle_2d (math.rs:687-706), interpolate a depth (interpolate_depth_in_triangle, viewport_3d.rs:7485-7508) and keep the
// closest hit with a strict `<` -- so the first of equal depths wins, and a NaN depth is kept when it comes first and ignored otherwise.
//
// GPU form: one launch for all items.  A table row (PickItem) names an item's vertices, faces and placement and its first workgroup; a
// workgroup takes PICK_CHUNK triangles of one item, one triangle per lane per trip, and evaluates the reference's expressions in the
// reference's order (f32, no contraction; world_point is the one k_world_project uses).  "Closest in loop order" without a sequential walk
// is three minima per item (PickWords):
//     key        min over the hits whose depth is not NaN of (orderable(depth) << 32 | tri): the smallest depth, the first of equal ones
//                (orderable: the sign-flip map, -0.0 mapped onto +0.0 first, so the two zeros tie as they do under `<`)
//     first      the smallest tri over all hits
//     first_nan  the smallest tri over the hits with a NaN depth
// first == first_nan: the first hit of the loop had a NaN depth and nothing replaced it; else the first hit was a number, every NaN after
// it was ignored and the answer is the key's.  Each minimum is reduced in the wave by shuffles, across the workgroup's four waves through
// LDS, and then costs at most one agent-scope atomic per word, workgroup and item -- from workgroups that had a hit only.
// k_pick_resolve (one workgroup, same stream) turns the words into B32PickHit records, recomputes the winning triangle's depth for its
// own bits (the key cannot tell -0.0 from +0.0), runs the loop over the items (viewport_3d.rs:7370: the same strict `<`, so the same three
// minima over (depth, item)) and re-arms the words.
#include "b32_host.h"
#include "b32_world_point.h"

namespace b32 {

constexpr uint32_t PICK_CHUNK = 1024;           // triangles per workgroup: 256 lanes, four trips
constexpr uint32_t PICK_SMALL = 32;             // tables of at most this many rows travel in the kernel argument (2048 bytes)
constexpr uint32_t PICK_MAX_ITEMS = 65535;
constexpr uint32_t PICK_NONE = 0xFFFFFFFFu;
constexpr uint32_t PICK_QNAN = 0x7FC00000u;     // the one NaN a NaN depth is reported as (as b32_draw_world's records)
constexpr size_t PICK_HEADER = 16;              // {int32 best; uint32 n; 8 bytes of padding} in front of the n B32PickHit

struct PickTable { PickItem r[PICK_SMALL]; };
struct PickWords { unsigned long long key; uint32_t first, first_nan; };
struct PickArgs {
    WorldArgs w;                                // camera and projection constants (items / out / counts unused)
    float mx, my; uint32_t cull, n;
    const PickItem* table;                      // nullptr: the table is the kernel argument
    PickWords* words;                           // n entries, all ones between two picks
    unsigned char* result;                      // PICK_HEADER + n * sizeof(B32PickHit)
};
static_assert(sizeof(PickItem) == 64 && sizeof(PickWords) == 16 && sizeof(B32PickHit) == 16 && sizeof(PickArgs) + sizeof(PickTable) <= 3072,
              "pick records / kernel argument size");

// total order of the non-NaN f32 as u32, both zeros on one value
__device__ __forceinline__ uint32_t pick_orderable(float d) {
    uint32_t u = __float_as_uint(d);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Triangle t of an item through the body of the reference's loops: false = skipped or missed, true = hit with `depth`.
__device__ __forceinline__ bool pick_triangle(const PickArgs& a, const PickItem& it, uint32_t t, float& depth) {
    const uint32_t* fv = it.faces[t].v;
    const uint32_t idx[3] = { fv[0], fv[1], fv[2] };
    if (idx[0] >= it.nv || idx[1] >= it.nv || idx[2] >= it.nv) return false;            // screen_verts.get(..) == None
    const bool ortho = a.w.has_ortho != 0u;
    float sx[3], sy[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* p = it.pos12 ? it.pos12 + (size_t)idx[k] * 3 : it.verts[idx[k]].pos;
        const float x = p[0], y = p[1], z = p[2];
        const float rx = x * it.cos_f - z * it.sin_f;                                   // viewport_3d.rs:7716-7718
        const float rz = x * it.sin_f + z * it.cos_f;
        const float world[3] = { rx + it.wpos[0], y + it.wpos[1], rz + it.wpos[2] };
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

// One hit into a lane's three minima; `id` is the triangle (k_pick) or the item (k_pick_resolve).
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

template <bool SMALL>
__global__ __launch_bounds__(256) void k_pick(PickArgs a, PickTable small) {
    const uint32_t wg = blockIdx.x;
    // the last row whose first workgroup is not behind this one (rows without triangles share their successor's number and lose to it)
    uint32_t item = 0;
    if (SMALL) {
        for (uint32_t i = 1; i < a.n; ++i) if (small.r[i].first_wg <= wg) item = i;
    } else {
        uint32_t lo = 0, hi = a.n;              // a.table[lo].first_wg <= wg < a.table[hi].first_wg
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (a.table[mid].first_wg <= wg) lo = mid; else hi = mid; }
        item = lo;
    }
    const PickItem it = SMALL ? small.r[item] : a.table[item];
    const uint32_t t0 = (wg - it.first_wg) * PICK_CHUNK;
    PickWords m = pick_no_hit();
#pragma unroll 1
    for (uint32_t trip = 0; trip < PICK_CHUNK / 256u; ++trip) {
        const uint32_t t = t0 + trip * 256u + threadIdx.x;
        float depth;
        if (t >= t0 && t < it.nf && pick_triangle(a, it, t, depth)) pick_take(m, depth, t);
    }
    m = pick_reduce(m);
    if (threadIdx.x == 0u && m.first != PICK_NONE) {
        PickWords* w = a.words + item;
        __hip_atomic_fetch_min(&w->first, m.first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (m.first_nan != PICK_NONE) __hip_atomic_fetch_min(&w->first_nan, m.first_nan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (m.key != ~0ull) __hip_atomic_fetch_min(&w->key, m.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool SMALL>
__global__ __launch_bounds__(256) void k_pick_resolve(PickArgs a, PickTable small) {
    B32PickHit* hits = reinterpret_cast<B32PickHit*>(a.result + PICK_HEADER);
    PickWords m = pick_no_hit();
    for (uint32_t i = threadIdx.x; i < a.n; i += 256u) {
        const PickWords w = a.words[i];
        a.words[i] = pick_no_hit();                                                      // armed for the next pick on this stream
        B32PickHit h; h.hit = 0u; h.tri = PICK_NONE; h.depth = 0.0f; h._pad = 0u;
        if (w.first != PICK_NONE) {
            h.hit = 1u;
            if (w.first == w.first_nan) { h.tri = w.first; h.depth = __uint_as_float(PICK_QNAN); }
            else {
                h.tri = (uint32_t)w.key;
                const PickItem it = SMALL ? small.r[i] : a.table[i];
                (void)pick_triangle(a, it, h.tri, h.depth);                              // the winner's own bits (the sign of a zero)
            }
            pick_take(m, h.depth, i);
        }
        hits[i] = h;
    }
    m = pick_reduce(m);
    if (threadIdx.x == 0u) {
        int32_t* head = reinterpret_cast<int32_t*>(a.result);
        head[0] = m.first == PICK_NONE ? -1 : (int32_t)(m.first == m.first_nan ? m.first : (uint32_t)m.key);
        head[1] = (int32_t)a.n; head[2] = 0; head[3] = 0;
    }
}

}  // namespace b32

// ------------------------------------------------------------------ host
namespace {

// The table of a pick (checked arguments): rows and the number of workgroups.  B32_E_UNSUPPORTED when the grid would not fit.
int pick_table(b32_scene* const* slots, const B32Placement* places, uint32_t n, std::vector<PickItem>& rows, uint32_t& groups) {
    rows.resize(n);
    unsigned long long wg = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const b32_scene* sl = slots[i];
        PickItem& r = rows[i];
        r = PickItem{};
        r.verts = sl->d_verts; r.faces = sl->d_faces; r.nv = sl->nv; r.nf = sl->nf;
        r.pos12 = (sl->pos_valid && sl->d_pos12) ? sl->d_pos12 : nullptr;
        r.cos_f = places[i].cos_f; r.sin_f = places[i].sin_f;
        for (int k = 0; k < 3; ++k) r.wpos[k] = places[i].world_pos[k];
        r.first_wg = (uint32_t)wg;
        wg += ((unsigned long long)sl->nf + PICK_CHUNK - 1u) / PICK_CHUNK;
        if (wg >= (1ull << 24)) return B32_E_UNSUPPORTED;                                 // (16 G triangles in one call)
    }
    groups = (uint32_t)wg;
    return B32_OK;
}

int pick_check(const b32_ctx* c, const B32Camera* cam, uint32_t flags, b32_scene* const* slots, const B32Placement* places, uint32_t n) {
    if (!c || !cam || (flags & ~B32_PICK_CULL_BACKFACES) || !c->width || !c->height) return B32_E_ARG;
    if (n > PICK_MAX_ITEMS) return B32_E_UNSUPPORTED;
    if (n && (!slots || !places)) return B32_E_ARG;
    for (uint32_t i = 0; i < n; ++i) if (!slots[i] || !slots[i]->have_scene) return B32_E_ARG;
    return B32_OK;
}

}  // namespace

extern "C" {

int b32_pick_meshes_async(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, float mx, float my, uint32_t flags,
                          b32_scene* const* slots, const B32Placement* places, uint32_t n, void* out, uint64_t* ticket) {
    { const int rc = pick_check(c, cam, flags, slots, places, n); if (rc) return rc; }
    if (!out || !ticket) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    std::vector<PickItem> rows;
    uint32_t groups = 0;
    int rc;
    if ((rc = pick_table(slots, places, n, rows, groups))) return rc;

    PickArgs a{};
    for (int k = 0; k < 3; ++k) { a.w.pos[k] = cam->position[k]; a.w.bx[k] = cam->basis_x[k]; a.w.by[k] = cam->basis_y[k]; a.w.bz[k] = cam->basis_z[k]; }
    a.w.vs = ((float)(c->width < c->height ? c->width : c->height) / 2.0f) * 0.75f;     // math.rs:642-643
    a.w.half_w = (float)c->width / 2.0f; a.w.half_h = (float)c->height / 2.0f;
    if (ortho) { a.w.has_ortho = 1u; a.w.zoom = ortho->zoom; a.w.center_x = ortho->center_x; a.w.center_y = ortho->center_y; }
    a.mx = mx; a.my = my; a.cull = (flags & B32_PICK_CULL_BACKFACES) ? 1u : 0u; a.n = n;

    // the words: all ones whenever no pick is running (allocated so; k_pick_resolve leaves them so)
    if ((size_t)n > c->pick_cap_words || !c->pick_words) {
        const size_t cap = (size_t)n + n / 4 + 64;
        if (c->pick_words) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(c->pick_words)); c->pick_words = nullptr; c->pick_cap_words = 0; }
        HIPCHK(c, hipMalloc(&c->pick_words, cap * sizeof(PickWords)));
        HIPCHK(c, hipMemsetAsync(c->pick_words, 0xFF, cap * sizeof(PickWords), c->stream));
        c->pick_cap_words = cap;
    }
    a.words = static_cast<PickWords*>(c->pick_words);

    // the ticket (shared with b32_fb_download_async: at most DL_RING outstanding) and the result buffer of this pick: PICK_RING device
    // buffers in turn, each written again only behind the transfer that last read it
    unsigned long long t = 0; hipEvent_t* tev = nullptr;
    if ((rc = ticket_open(c, t, tev))) return rc;
    const uint32_t k = c->pick_slot;
    c->pick_slot = (k + 1) % b32_ctx::PICK_RING;
    const size_t bytes = PICK_HEADER + (size_t)n * sizeof(B32PickHit);
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
    a.result = static_cast<unsigned char*>(c->pick_res[k]);

    const bool small = n <= PICK_SMALL;
    PickTable tab{};
    if (small) { for (uint32_t i = 0; i < n; ++i) tab.r[i] = rows[i]; }
    else {
        if ((rc = stage_records(c, c->pick_tab, rows.data(), n))) return rc;
        a.table = c->pick_tab.dev;
    }
    const bool timed = c->profile_level >= 1;
    if (timed) {
        for (hipEvent_t& e : c->pick_tev) if (!e) HIPCHK(c, hipEventCreate(&e));
        HIPCHK(c, hipEventRecord(c->pick_tev[0], c->stream));
    }
    if (groups) {
        if (small) hipLaunchKernelGGL(k_pick<true>, dim3(groups), dim3(256), 0, c->stream, a, tab);
        else hipLaunchKernelGGL(k_pick<false>, dim3(groups), dim3(256), 0, c->stream, a, tab);
    }
    if (small) hipLaunchKernelGGL(k_pick_resolve<true>, dim3(1), dim3(256), 0, c->stream, a, tab);
    else hipLaunchKernelGGL(k_pick_resolve<false>, dim3(1), dim3(256), 0, c->stream, a, tab);
    HIPCHK(c, hipGetLastError());
    if (timed) { HIPCHK(c, hipEventRecord(c->pick_tev[1], c->stream)); c->pick_timed = true; }
    // delivery: the copy leaves on dl_stream behind the resolve kernel, the ticket completes on it (as in b32_fb_download_async)
    HIPCHK(c, hipEventRecord(c->pick_done[k], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->dl_stream, c->pick_done[k], 0));
    HIPCHK(c, hipMemcpyAsync(out, c->pick_res[k], bytes, hipMemcpyDeviceToHost, c->dl_stream));
    HIPCHK(c, hipEventRecord(c->pick_left[k], c->dl_stream));
    HIPCHK(c, hipEventRecord(*tev, c->dl_stream));
    c->dl_seq = t; *ticket = t;
    return B32_OK;
}

int b32_pick_meshes(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, float mx, float my, uint32_t flags,
                    b32_scene* const* slots, const B32Placement* places, uint32_t n, B32PickHit* hits, int32_t* best) {
    { const int rc = pick_check(c, cam, flags, slots, places, n); if (rc) return rc; }
    if (!best) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    const size_t bytes = PICK_HEADER + (size_t)n * sizeof(B32PickHit);
    if (bytes > c->pick_cap_host) {
        if (c->pick_host) HIPCHK(c, hipHostFree(c->pick_host));
        c->pick_host = nullptr; c->pick_cap_host = 0;
        const size_t cap = bytes + bytes / 4 + 1024;
        HIPCHK(c, hipHostMalloc(&c->pick_host, cap, hipHostMallocDefault));
        c->pick_cap_host = cap;
    }
    uint64_t t = 0;
    int rc;
    if ((rc = b32_pick_meshes_async(c, cam, ortho, mx, my, flags, slots, places, n, c->pick_host, &t))) return rc;
    if ((rc = b32_ticket_wait(c, t))) return rc;
    const unsigned char* h = static_cast<const unsigned char*>(c->pick_host);
    std::memcpy(best, h, sizeof(int32_t));
    if (hits && n) std::memcpy(hits, h + PICK_HEADER, (size_t)n * sizeof(B32PickHit));
    return B32_OK;
}

}  // extern "C"
