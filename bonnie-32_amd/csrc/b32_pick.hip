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
#include "b32_pick_body.h"

namespace b32 {

constexpr uint32_t PICK_SMALL = 32;             // tables of at most this many rows travel in the kernel argument (2048 bytes)
constexpr uint32_t PICK_MAX_ITEMS = 65535;
constexpr size_t PICK_HEADER = 16;              // {int32 best; uint32 n; 8 bytes of padding} in front of the n B32PickHit

struct PickTable { PickItem r[PICK_SMALL]; };
static_assert(sizeof(PickItem) == 64 && sizeof(PickWords) == 16 && sizeof(B32PickHit) == 16 && sizeof(PickArgs) + sizeof(PickTable) <= 3072,
              "pick records / kernel argument size");

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
        if (t >= t0 && t < it.nf && pick_triangle(a.q, it, t, depth)) pick_take(m, depth, t);
    }
    m = pick_reduce(m);
    if (threadIdx.x == 0u) pick_offer(m, a.words + item);
}

template <bool SMALL>
__global__ __launch_bounds__(256) void k_pick_resolve(PickArgs a, PickTable small) {
    B32PickHit* hits = reinterpret_cast<B32PickHit*>(a.q.result + PICK_HEADER);
    PickWords m = pick_no_hit();
    for (uint32_t i = threadIdx.x; i < a.n; i += 256u) {
        const PickWords w = a.words[i];
        a.words[i] = pick_no_hit();                                                      // armed for the next pick on this stream
        B32PickHit h; h.hit = 0u; h.tri = PICK_NONE; h.depth = 0.0f; h._pad = 0u;
        bool nan;
        if (pick_winner(w, h.tri, nan)) {
            h.hit = 1u;
            if (nan) h.depth = __uint_as_float(PICK_QNAN);
            else {
                const PickItem it = SMALL ? small.r[i] : a.table[i];
                (void)pick_triangle(a.q, it, h.tri, h.depth);                            // the winner's own bits (the sign of a zero)
            }
            pick_take(m, h.depth, i);
        }
        hits[i] = h;
    }
    m = pick_reduce(m);
    if (threadIdx.x == 0u) {
        int32_t* head = reinterpret_cast<int32_t*>(a.q.result);
        uint32_t best; bool nan;
        head[0] = pick_winner(m, best, nan) ? (int32_t)best : -1;
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
        r.verts = sl->d_verts; r.faces = sl->d_faces; r.nv = sl->body_nv(); r.nf = sl->body_nf();       // (bone octahedra are drawn, never picked)
        r.pos12 = (sl->pos_valid && sl->d_pos12) ? sl->d_pos12 : nullptr;
        r.cos_f = places[i].cos_f; r.sin_f = places[i].sin_f;
        for (int k = 0; k < 3; ++k) r.wpos[k] = places[i].world_pos[k];
        r.first_wg = (uint32_t)wg;
        wg += ((unsigned long long)sl->body_nf() + PICK_CHUNK - 1u) / PICK_CHUNK;
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
    query_fill(a.q, c, cam, ortho, mx, my, (flags & B32_PICK_CULL_BACKFACES) != 0u);
    a.n = n;

    // the words: all ones whenever no pick is running (allocated so; k_pick_resolve leaves them so)
    if ((rc = armed_ensure(c, c->pick_words, (size_t)n * sizeof(PickWords), 0xFF))) return rc;
    a.words = static_cast<PickWords*>(c->pick_words.p);

    // the ticket and the result buffer of this pick (pick_result_open)
    unsigned long long t = 0; hipEvent_t* tev = nullptr; uint32_t k = 0;
    const size_t bytes = PICK_HEADER + (size_t)n * sizeof(B32PickHit);
    if ((rc = pick_result_open(c, bytes, t, tev, k, &a.q.result))) return rc;

    const bool small = n <= PICK_SMALL;
    PickTable tab{};
    if (small) { for (uint32_t i = 0; i < n; ++i) tab.r[i] = rows[i]; }
    else {
        if ((rc = stage_records(c, c->pick_tab, rows.data(), n))) return rc;
        a.table = c->pick_tab.dev;
    }
    const bool timed = c->profile_level >= 1;
    if (timed) HIPCHK(c, c->pick_timer.begin(c->stream));
    if (groups) {
        if (small) hipLaunchKernelGGL(k_pick<true>, dim3(groups), dim3(256), 0, c->stream, a, tab);
        else hipLaunchKernelGGL(k_pick<false>, dim3(groups), dim3(256), 0, c->stream, a, tab);
    }
    if (small) hipLaunchKernelGGL(k_pick_resolve<true>, dim3(1), dim3(256), 0, c->stream, a, tab);
    else hipLaunchKernelGGL(k_pick_resolve<false>, dim3(1), dim3(256), 0, c->stream, a, tab);
    HIPCHK(c, hipGetLastError());
    if (timed) HIPCHK(c, c->pick_timer.end(c->stream));
    return pick_result_deliver(c, k, bytes, out, t, tev, ticket);
}

int b32_pick_meshes(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, float mx, float my, uint32_t flags,
                    b32_scene* const* slots, const B32Placement* places, uint32_t n, B32PickHit* hits, int32_t* best) {
    { const int rc = pick_check(c, cam, flags, slots, places, n); if (rc) return rc; }
    if (!best) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    const unsigned char* h = nullptr;
    const int rc = pick_blocking(c, PICK_HEADER + (size_t)n * sizeof(B32PickHit), &h, [&](void* out, uint64_t* t) {
        return b32_pick_meshes_async(c, cam, ortho, mx, my, flags, slots, places, n, out, t); });
    if (rc) return rc;
    std::memcpy(best, h, sizeof(int32_t));
    if (hits && n) std::memcpy(hits, h + PICK_HEADER, (size_t)n * sizeof(B32PickHit));
    return B32_OK;
}

}  // extern "C"
