// b32_object_overlay.hip -- the world editor's object overlays made into B32Prim records on the device from resident asset parts
// (b32_draw_object_overlays), and a slot's bounds (b32_scene_bounds): k_scene_bounds, k_object_overlay, the host's record count.
//
// Reference: draw_asset_wireframe (editor/viewport_3d.rs:255-291) walks every polygon edge of every visible part of an asset per frame
// while the mouse moves; asset.bounds() (asset/asset.rs:288-312) walks every vertex of every part per selected object per frame before
// draw_rotated_bounding_box (viewport_3d.rs:7658-7697) draws twelve lines.  The parts are resident (slots, placed per draw), so the records
// are made where the vertices are.  The arithmetic is in b32_object_overlay_body.h; where a record lies is decided by the host
// (object_overlay_plan) from the half-edge counts and the item kinds, never from the camera.
//
// GPU form.
//   k_scene_bounds    the min / max of a slot's body positions as six unsigned keys (overlay_key: a monotone map, so the fold is a function
//                     of the SET of non-NaN values and runs in any order) in a 24-byte block that belongs to the slot.  A lane strides over
//                     the positions with six running keys; then shuffles in the wave, one LDS stage across the four waves, six atomics per
//                     WORKGROUP.  One launch per call however many slots are stale: blockIdx.y is the row of a table (stale slot ->
//                     positions, stride, nv, block).  The grid's x is sized from the largest nv and capped at 2 workgroups per CU: past
//                     that a workgroup takes several chunks of 256 and the atomics stop growing with nv; rows with fewer vertices let the
//                     surplus workgroups leave at once.  The block is armed (overlay_bounds_start) on the stream before the launch and stays
//                     valid until the slot's vertices move (SceneState::bounds_valid).
//   k_object_overlay  one lane per record, a workgroup inside exactly one row of the host's table: it finds the row from blockIdx.x by a
//                     binary search over first_wg -- addresses that depend on blockIdx alone, so the loads are scalar -- and runs
//                     object_overlay_lane.  A WIRE workgroup does 256 half-edges (two position loads, place, draw_3d_line_clipped, one
//                     record store); a box workgroup has 12 working lanes which fold the bounds blocks of the item's parts in keys, unkey,
//                     build their two corners by selection (no corner array) and run draw_3d_line.  Drawn / dropped / rejected: the
//                     shared counting tail (b32_item_kernels.h), one atomic per workgroup and counter.
// The records stay on the device: the ordered tile pass of b32_prims.hip reads them where this kernel wrote them.  No new record kind.
#include "b32_host.h"
#include "b32_item_kernels.h"
#include "b32_object_overlay_body.h"
#include "b32_pick_body.h"

namespace b32 {

static_assert(sizeof(HoverHalfEdge) == 16 && offsetof(HoverHalfEdge, v0) == 0 && offsetof(HoverHalfEdge, v1) == 4,
              "ObjectRow::he reads (v0, v1) as the first two of four words");
static_assert(sizeof(B32ObjectPart) == 24 && sizeof(B32ObjectItem) == 60 && offsetof(B32ObjectItem, box_min) == 28 && offsetof(B32ObjectItem, kind) == 56 &&
              sizeof(OverlayBounds) == 24 && sizeof(BoundsRow) == 24 && sizeof(ObjectOverlayArgs) <= 1024, "B32ObjectPart / B32ObjectItem layout");

// the blocks of the rows back at their start values, before k_scene_bounds on the stream
__global__ __launch_bounds__(64) void k_scene_bounds_arm(BoundsArgs a, uint32_t n_rows) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n_rows) return;
    OverlayBounds* o = a.rows ? a.rows[i].out : a.one.out;
    *o = overlay_bounds_start();
}

__global__ __launch_bounds__(256) void k_scene_bounds(BoundsArgs a) {
    __shared__ uint32_t part[4][6];
    const BoundsRow r = a.rows ? a.rows[blockIdx.y] : a.one;       // (uniform: scalar loads)
    if ((unsigned long long)blockIdx.x * 256u >= r.nv) return;      // (the whole workgroup: nothing of this row is left for it)
    OverlayBounds b = overlay_bounds_start();
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x; i < r.nv; i += (unsigned long long)gridDim.x * 256u) {
        const float* src = r.pos + i * r.stride;
        const float p[3] = { src[0], src[1], src[2] };
        overlay_bounds_take(b, p);
    }
    const uint32_t wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t lo = overlay_wave_min(b.mn[c]), hi = overlay_wave_max(b.mx[c]);
        if ((threadIdx.x & 63u) == 0u) { part[wave][c] = lo; part[wave][3 + c] = hi; }
    }
    __syncthreads();
    if (threadIdx.x < 6u) {
        const uint32_t c = threadIdx.x;
        const bool is_min = c < 3u;
        uint32_t k = part[0][c];
#pragma unroll
        for (int w = 1; w < 4; ++w) k = is_min ? min(k, part[w][c]) : max(k, part[w][c]);
        if (is_min) { if (k != OVERLAY_KEY_MIN0) __hip_atomic_fetch_min(&r.out->mn[c], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        else if (k != OVERLAY_KEY_MAX0) __hip_atomic_fetch_max(&r.out->mx[c - 3u], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// b32_scene_bounds' 32 bytes from the slot's finished block (behind k_scene_bounds on the stream)
__global__ __launch_bounds__(64) void k_scene_bounds_result(const OverlayBounds* block, uint32_t has_verts, uint32_t* out8) {
    if (threadIdx.x == 0u) object_bounds_result(*block, has_verts, out8);
}

__global__ __launch_bounds__(256) void k_object_overlay(ObjectOverlayArgs a) {
    uint32_t* tally = outcome_tally();
    const ObjectRow r = a.rows[object_row_of(a.rows, a.n_rows, blockIdx.x)];   // (uniform: scalar loads)
    const uint32_t which = object_overlay_lane(a.v, r, a.bounds, blockIdx.x - r.first_wg, threadIdx.x, a.out);
    // (every lane of the workgroup arrives here: no early return above)
    outcome_count(tally, a.counts, which);
}

void launch_scene_bounds(hipStream_t s, const BoundsArgs& a, uint32_t n_rows, uint32_t max_nv, int n_cu) {
    if (!n_rows) return;
    hipLaunchKernelGGL(k_scene_bounds_arm, dim3((n_rows + 63u) / 64u), dim3(64), 0, s, a, n_rows);
    if (!max_nv) return;                                            // (slots without vertices: the start values are the answer)
    const unsigned long long want = ((unsigned long long)max_nv + 255u) / 256u, cap = 2ull * (unsigned long long)(n_cu > 0 ? n_cu : 1);
    const uint32_t gx = (uint32_t)(want < cap ? want : cap);
    for (uint32_t first = 0; first < n_rows; first += 65535u) {     // (gridDim.y: one launch for up to 65535 stale slots)
        BoundsArgs b = a;
        if (b.rows) b.rows += first;
        const uint32_t gy = n_rows - first < 65535u ? n_rows - first : 65535u;
        hipLaunchKernelGGL(k_scene_bounds, dim3(gx, gy), dim3(256), 0, s, b);
    }
}

void launch_object_overlay(hipStream_t s, const ObjectOverlayArgs& a) {
    if (a.n_groups) hipLaunchKernelGGL(k_object_overlay, dim3(a.n_groups), dim3(256), 0, s, a);
}

}  // namespace b32

// What object_overlay_plan reads of the call's parts.  A NULL slot stays "does not hold its scene".
void object_part_views(const B32ObjectPart* parts, uint32_t n_parts, std::vector<ObjectPartView>& views) {
    views.assign(parts ? n_parts : 0u, ObjectPartView{});
    for (size_t p = 0; p < views.size(); ++p) {
        const b32_scene* sc = parts[p].slot;
        const b32_topology* t = parts[p].topology;
        ObjectPartView& v = views[p];
        v.holds_scene = sc && sc->have_scene;
        v.has_topology = t != nullptr;
        if (t) { v.he = reinterpret_cast<const uint32_t*>(t->he); v.nh = t->nh; }
        if (!v.holds_scene) continue;
        v.pos = slot_positions(sc, v.stride);
        v.nv = sc->body_nv();                         // (bone octahedra behind the mesh are neither drawn nor reduced)
        v.bounds = sc->d_bounds;
    }
}

// The slot's block exists (allocation only: nothing is enqueued, and the block says nothing until scene_bounds_run has filled it).
int scene_bounds_alloc(b32_ctx* c, b32_scene* sc) {
    if (sc->d_bounds) return B32_OK;
    sc->bounds_valid = false;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&sc->d_bounds), sizeof(OverlayBounds)));
    return B32_OK;
}
// One row of k_scene_bounds' table for a slot whose block exists.
void scene_bounds_row(const b32_scene* sc, BoundsRow* r) {
    r->pos = slot_positions(sc, r->stride);
    r->nv = sc->body_nv(); r->out = sc->d_bounds;
}
// The reductions of c->bounds_stale (each slot once, each with a block; d_rows: their rows on the device in that order, nullptr: one slot,
// its row by value) enqueued on the stream: the blocks armed, one launch, the slots' caches valid, the counter moved.
int scene_bounds_run(b32_ctx* c, const BoundsRow* d_rows) {
    const size_t n = c->bounds_stale.size();
    if (!n) return B32_OK;
    BoundsArgs a{};
    a.rows = d_rows;
    uint32_t max_nv = 0;
    for (const b32_scene* sc : c->bounds_stale) max_nv = std::max(max_nv, sc->body_nv());
    if (!d_rows) scene_bounds_row(c->bounds_stale[0], &a.one);
    launch_scene_bounds(c->stream, a, (uint32_t)n, max_nv, c->n_cu);
    HIPCHK(c, hipGetLastError());
    for (b32_scene* sc : c->bounds_stale) { sc->bounds_valid = true; ++c->bounds_reductions; }
    c->bounds_stale.clear();
    return B32_OK;
}

extern "C" int b32_object_overlay_record_count(const B32ObjectPart* parts, uint32_t n_parts, const B32ObjectItem* items, uint32_t n_items, uint64_t* n) {
    if (!n) return B32_E_ARG;
    std::vector<ObjectPartView> views;
    object_part_views(parts, n_parts, views);
    ObjectOverlayPlan plan;
    const int rc = object_overlay_plan(parts, views.data(), n_parts, items, n_items, false, plan);
    if (rc) return rc;
    *n = plan.total;
    return B32_OK;
}

extern "C" int b32_scene_bounds_async(b32_ctx* c, b32_scene* slot, void* out, uint64_t* ticket) {
    if (!c || !out || !ticket) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    if (!sc) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    int rc;
    if ((rc = scene_bounds_alloc(c, sc))) return rc;
    if (!sc->bounds_valid) {
        c->bounds_stale.assign(1, sc);
        if ((rc = scene_bounds_run(c, nullptr))) { c->bounds_stale.clear(); return rc; }
    }
    unsigned long long t = 0; hipEvent_t* tev = nullptr; uint32_t k = 0;
    unsigned char* res = nullptr;
    if ((rc = pick_result_open(c, 32, t, tev, k, &res))) return rc;
    hipLaunchKernelGGL(k_scene_bounds_result, dim3(1), dim3(64), 0, c->stream, sc->d_bounds, sc->body_nv() ? 1u : 0u, reinterpret_cast<uint32_t*>(res));
    HIPCHK(c, hipGetLastError());
    return pick_result_deliver(c, k, 32, out, t, tev, ticket);
}

extern "C" int b32_scene_bounds(b32_ctx* c, b32_scene* slot, float mn[3], float mx[3], uint32_t* has_verts) {
    if (!c || !mn || !mx || !has_verts || !scene_of(c, slot)) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    const unsigned char* h = nullptr;
    const int rc = pick_blocking(c, 32, &h, [&](void* landing, uint64_t* t) { return b32_scene_bounds_async(c, slot, landing, t); });
    if (rc) return rc;
    std::memcpy(mn, h, 12); std::memcpy(mx, h + 12, 12); std::memcpy(has_verts, h + 24, 4);
    return B32_OK;
}
