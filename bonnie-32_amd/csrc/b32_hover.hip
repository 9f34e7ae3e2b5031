// b32_hover.hip -- the modeler's hover and rubber-band selection for one resident mesh: b32_topology, b32_hover_mesh[_async],
// b32_box_select[_async].
//
// Reference: find_hovered_element (modeler/viewport.rs:2379-2601) asks on every mouse move which vertex, else which edge, else which
// face lies under the cursor; apply_box_selection (:1624-1779) projects the same vertices (or the polygons' centres) against a
// rectangle.  Both walk the modeler's n-gons, which the fan triangles of a scene slot cannot give back, so the polygons live in a
// b32_topology: per polygon position one half-edge (v[k], v[(k + 1) % n]) with the id of its normalised edge (Face::edges,
// mesh_editor.rs:92-95), and the fan triangles with their polygon (Face::triangulate, :99-112), both in the reference's loop order.
//
// GPU form of a hover.  The three loops are independent (the vertex loop does not read what the edge loop found), so all three are
// evaluated and reported; the caller masks (vertex, else edge, else face).
//   k_hover_front    (only with culling) one lane per polygon: the front pass (:2435-2473) sets bits of a vertex bitmap and of an edge
//                    bitmap with atomicOr.
//   k_hover          one launch over three ranges of work -- vertices, half-edges, fan triangles -- a workgroup inside exactly one of
//                    them, 1024 elements in four trips of 256 lanes, every expression a separately rounded f32 operation in the
//                    reference's order.  A candidate distance is neither NaN nor negative (`NaN < threshold` is false), so "smallest
//                    distance, first in loop order" is ONE 64-bit minimum of (distance bits << 32 | loop ordinal) and the key holds the
//                    winner's exact bits; the faces need the three minima of b32_pick.hip (a NaN depth sticks when it comes first).
//                    Reduced by shuffles and through LDS like k_pick; at most one agent-scope atomic per word and workgroup.
//   k_hover_resolve  one workgroup: writes the 32-byte result (the winning triangle's depth recomputed for the sign of a zero), re-arms
//                    the words and clears the bitmaps for the next call on the stream.
// k_box_select: one lane per vertex (mode 0) or polygon (mode 1); a wave's ballot is two words of the bitmap.
#include "b32_pick_body.h"

namespace b32 {

struct HoverWords { unsigned long long vkey, ekey; PickWords face; };
struct HoverArgs {
    QueryArgs q;                                // camera, cursor, cull = !SEE_THROUGH, result
    PickItem it;                                // the slot's vertices and the placement (faces / nf / first_wg unused)
    const HoverHalfEdge* he; const HoverFanTri* fan; const uint32_t* poly_start; const uint32_t* poly_verts;
    uint32_t np, nh, nt, placed;
    uint32_t mirror_axis; float mirror_thr, vthr, ethr;
    uint32_t gv, ge, vwords, ewords;            // workgroups of the vertex and of the half-edge range; words of the two bitmaps
    uint32_t *vbits, *ebits;
    HoverWords* words;
    const float* rest;                          // a rigged slot's rest stream (24 B per vertex: position, normal), else nullptr
};
struct BoxArgs {
    QueryArgs q; PickItem it;
    const uint32_t* poly_start; const uint32_t* poly_verts;
    uint32_t n, mode, placed, nwords;
    float x0, y0, x1, y1;
};
static_assert(sizeof(HoverWords) == 32 && sizeof(B32HoverResult) == 32 && sizeof(B32HoverParams) == 32 && sizeof(B32BoxParams) == 32 &&
              sizeof(HoverHalfEdge) == 16 && sizeof(HoverFanTri) == 16 && sizeof(HoverArgs) <= 1024, "hover records / kernel argument size");

// MirrorSettings::is_editable_side, modeler/state.rs:797-806 (a NaN coordinate or threshold fails)
__device__ __forceinline__ bool hover_editable(const HoverArgs& a, const float* local) {
    if (a.mirror_axis == 0u) return true;
    const float v = a.mirror_axis == 1u ? local[0] : (a.mirror_axis == 2u ? local[1] : local[2]);
    return v >= -a.mirror_thr;
}
// ... of vertex i, whose position in the slot is `local`: find_hovered_element tests the LOCAL position and projects the posed one
// (viewport.rs:2482-2486), and the local position of a rigged slot is in its rest stream.  RIG is a compile-time switch (a.rest != nullptr):
// the kernel of a slot without a rig is the text it was before there were rigs.
template <bool RIG>
__device__ __forceinline__ bool hover_editable_at(const HoverArgs& a, uint32_t i, const float* local) {
    if (!RIG) return hover_editable(a, local);
    if (a.mirror_axis == 0u) return true;
    return a.rest[(size_t)i * 6 + (a.mirror_axis - 1u)] >= -a.mirror_thr;       // (mirror_axis is 1, 2 or 3: checked by the entry)
}
// vertex i (< nv): its mirror test and its projection (world_to_screen_with_ortho, math.rs:538-575)
template <bool RIG>
__device__ __forceinline__ bool hover_screen(const HoverArgs& a, uint32_t i, bool mirror, float& sx, float& sy) {
    float local[3], world[3], z;
    pick_vertex(a.it, a.placed != 0u, i, local, world);
    if (mirror && !hover_editable_at<RIG>(a, i, local)) return false;
    return world_point(a.q.v, world, a.q.v.has_ortho != 0u, sx, sy, z);
}
__device__ __forceinline__ bool hover_bit(const uint32_t* bits, uint32_t i) { return ((bits[i >> 5] >> (i & 31u)) & 1u) != 0u; }

// viewport.rs:2435-2473
__global__ __launch_bounds__(256) void k_hover_front(HoverArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.np) return;
    const uint32_t s = a.poly_start[p], e = a.poly_start[p + 1u];
    if (e - s < 3u) return;
    float sx[3], sy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t i = a.poly_verts[s + k];
        if (i >= a.it.nv || !hover_screen<false>(a, i, false, sx[k], sy[k])) return;
    }
    const float area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sx[2] - sx[0]) * (sy[1] - sy[0]);
    if (!(area > 0.0f)) return;
    for (uint32_t j = s; j < e; ++j) {
        const uint32_t vi = a.poly_verts[j];
        if (vi < a.it.nv) atomicOr(&a.vbits[vi >> 5], 1u << (vi & 31u));
        const uint32_t ed = a.he[j].edge;
        atomicOr(&a.ebits[ed >> 5], 1u << (ed & 31u));
    }
}

// (mx - sx).powi(2) + (my - sy).powi(2)).sqrt(), viewport.rs:2497, :2611, :2621
__device__ __forceinline__ float hover_dist(float px, float py, float x, float y) {
    const float dx = px - x, dy = py - y;
    return sqrtf(dx * dx + dy * dy);
}
// point_to_line_distance, viewport.rs:2604-2622
__device__ __forceinline__ float hover_line_dist(float px, float py, float x0, float y0, float x1, float y1) {
    const float dx = x1 - x0, dy = y1 - y0;
    const float len_sq = dx * dx + dy * dy;
    if (len_sq < 0.001f) return hover_dist(px, py, x0, y0);
    float t = ((px - x0) * dx + (py - y0) * dy) / len_sq;
    if (t < 0.0f) t = 0.0f;                     // f32::clamp: a NaN and -0.0 stay
    if (t > 1.0f) t = 1.0f;
    const float proj_x = x0 + t * dx, proj_y = y0 + t * dy;
    return hover_dist(px, py, proj_x, proj_y);
}

template <bool RIG>
__global__ __launch_bounds__(256) void k_hover(HoverArgs a) {
    const uint32_t wg = blockIdx.x;
    const uint32_t range = wg < a.gv ? 0u : (wg < a.gv + a.ge ? 1u : 2u);
    const uint32_t e0 = (wg - (range == 0u ? 0u : (range == 1u ? a.gv : a.gv + a.ge))) * PICK_CHUNK;
    const uint32_t count = range == 0u ? a.it.nv : (range == 1u ? a.nh : a.nt);
    const bool cull = a.q.cull != 0u;
    PickWords m = pick_no_hit();                // vertices and half-edges use the key alone
#pragma unroll 1
    for (uint32_t trip = 0; trip < PICK_CHUNK / 256u; ++trip) {
        const uint32_t i = e0 + trip * 256u + threadIdx.x;
        if (i < e0 || i >= count) continue;
        if (range == 0u) {                      // viewport.rs:2475-2505
            if (cull && !hover_bit(a.vbits, i)) continue;
            float sx, sy;
            if (!hover_screen<RIG>(a, i, true, sx, sy)) continue;
            const float dist = hover_dist(a.q.mx, a.q.my, sx, sy);
            if (dist < a.vthr) m.key = min(m.key, ((unsigned long long)__float_as_uint(dist) << 32) | i);
        } else if (range == 1u) {               // viewport.rs:2507-2542
            const HoverHalfEdge h = a.he[i];
            if (cull && !hover_bit(a.ebits, h.edge)) continue;
            if (h.v0 >= a.it.nv || h.v1 >= a.it.nv) continue;
            float x0, y0, x1, y1;
            float l0[3], l1[3], w0[3], w1[3], z;
            pick_vertex(a.it, a.placed != 0u, h.v0, l0, w0);
            pick_vertex(a.it, a.placed != 0u, h.v1, l1, w1);
            if (!hover_editable_at<RIG>(a, h.v0, l0) || !hover_editable_at<RIG>(a, h.v1, l1)) continue;
            const bool ortho = a.q.v.has_ortho != 0u;
            if (!world_point(a.q.v, w0, ortho, x0, y0, z) || !world_point(a.q.v, w1, ortho, x1, y1, z)) continue;
            const float dist = hover_line_dist(a.q.mx, a.q.my, x0, y0, x1, y1);
            if (dist < a.ethr) m.key = min(m.key, ((unsigned long long)__float_as_uint(dist) << 32) | i);
        } else {                                // viewport.rs:2544-2594
            const HoverFanTri f = a.fan[i];
            const uint32_t s = a.poly_start[f.poly], e = a.poly_start[f.poly + 1u];
            bool editable = true;
            for (uint32_t j = s; j < e && editable; ++j) {
                const uint32_t vi = a.poly_verts[j];
                if (vi >= a.it.nv) { editable = false; break; }
                if (a.mirror_axis != 0u) {
                    float local[3], world[3];
                    pick_vertex(a.it, false, vi, local, world);
                    editable = hover_editable_at<RIG>(a, vi, local);
                }
            }
            float depth;
            if (editable && pick_triangle_idx(a.q, a.it, a.placed != 0u, f.v, depth)) pick_take(m, depth, i);
        }
    }
    m = pick_reduce(m);
    if (threadIdx.x == 0u) {
        if (range == 0u) { if (m.key != ~0ull) __hip_atomic_fetch_min(&a.words->vkey, m.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        else if (range == 1u) { if (m.key != ~0ull) __hip_atomic_fetch_min(&a.words->ekey, m.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        else pick_offer(m, &a.words->face);
    }
}

__global__ __launch_bounds__(256) void k_hover_resolve(HoverArgs a) {
    if (a.q.cull) {                                                                     // the bitmaps of the front pass: zero for the next call
        for (uint32_t i = threadIdx.x; i < a.vwords; i += 256u) a.vbits[i] = 0u;
        for (uint32_t i = threadIdx.x; i < a.ewords; i += 256u) a.ebits[i] = 0u;
    }
    if (threadIdx.x != 0u) return;
    const HoverWords w = *a.words;
    HoverWords armed; armed.vkey = ~0ull; armed.ekey = ~0ull; armed.face = pick_no_hit();
    *a.words = armed;
    B32HoverResult r;
    r.vertex = PICK_NONE; r.vertex_dist = 0.0f; r.edge_v0 = PICK_NONE; r.edge_v1 = PICK_NONE; r.edge_dist = 0.0f;
    r.face = PICK_NONE; r.face_depth = 0.0f; r._pad = 0u;
    if (w.vkey != ~0ull) { r.vertex = (uint32_t)w.vkey; r.vertex_dist = __uint_as_float((uint32_t)(w.vkey >> 32)); }
    if (w.ekey != ~0ull) {
        const HoverHalfEdge h = a.he[(uint32_t)w.ekey];
        r.edge_v0 = min(h.v0, h.v1); r.edge_v1 = max(h.v0, h.v1); r.edge_dist = __uint_as_float((uint32_t)(w.ekey >> 32));
    }
    uint32_t tri; bool nan;
    if (pick_winner(w.face, tri, nan)) {
        if (nan) r.face_depth = __uint_as_float(PICK_QNAN);
        else {
            const HoverFanTri f = a.fan[tri];
            (void)pick_triangle_idx(a.q, a.it, a.placed != 0u, f.v, r.face_depth);     // the winner's own bits (the sign of a zero)
        }
        r.face = a.fan[tri].poly;
    }
    *reinterpret_cast<B32HoverResult*>(a.q.result) = r;
}

// apply_box_selection, viewport.rs:1708-1726 (mode 0) and :1743-1766 (mode 1).  The header's n_selected is zero when the kernel starts.
__global__ __launch_bounds__(256) void k_box_select(BoxArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool sel = false;
    if (i < a.n) {
        float world[3]; bool some = true;
        if (a.mode == 0u) {
            float local[3];
            pick_vertex(a.it, a.placed != 0u, i, local, world);
        } else {
            const uint32_t s = a.poly_start[i], e = a.poly_start[i + 1u];
            float acc[3] = { 0.0f, 0.0f, 0.0f }; uint32_t cnt = 0;
            for (uint32_t j = s; j < e; ++j) {
                const uint32_t vi = a.poly_verts[j];
                if (vi >= a.it.nv) continue;                                            // filter_map: mesh.vertices.get(vi) == None
                float local[3], p[3];
                pick_vertex(a.it, a.placed != 0u, vi, local, p);
                acc[0] = acc[0] + p[0]; acc[1] = acc[1] + p[1]; acc[2] = acc[2] + p[2];
                ++cnt;
            }
            some = cnt != 0u;
            const float inv = 1.0f / (float)cnt;
            world[0] = acc[0] * inv; world[1] = acc[1] * inv; world[2] = acc[2] * inv;
        }
        float sx, sy, z;
        if (some && world_point(a.q.v, world, a.q.v.has_ortho != 0u, sx, sy, z))
            sel = sx >= a.x0 && sx <= a.x1 && sy >= a.y0 && sy <= a.y1;
    }
    box_emit(a.q.result, i, a.n, a.nwords, sel);
}

}  // namespace b32

// ------------------------------------------------------------------ host
namespace {

int hover_common_check(const b32_ctx* c, const B32Camera* cam, const b32_scene* slot) {
    if (!c || !cam || !slot || !slot->have_scene || !c->width || !c->height) return B32_E_ARG;
    return B32_OK;
}

void hover_item(PickItem& r, const b32_scene* sl, const B32Placement* place) {
    r = PickItem{};
    r.verts = sl->d_verts; r.nv = sl->body_nv();                                      // (bone octahedra are drawn, never hovered or selected)
    r.pos12 = (sl->pos_valid && sl->d_pos12) ? sl->d_pos12 : nullptr;
    if (place) { r.cos_f = place->cos_f; r.sin_f = place->sin_f; for (int k = 0; k < 3; ++k) r.wpos[k] = place->world_pos[k]; }
}

uint32_t hover_groups(uint32_t n) { return (uint32_t)(((unsigned long long)n + PICK_CHUNK - 1u) / PICK_CHUNK); }

}  // namespace

extern "C" {

int b32_topology_create(b32_ctx* c, const uint32_t* poly_start, uint32_t np, const uint32_t* poly_verts, b32_topology** out) {
    if (!c || !out) return B32_E_ARG;
    *out = nullptr;
    if (np && !poly_start) return B32_E_ARG;
    if (np == 0xFFFFFFFFu) return B32_E_UNSUPPORTED;
    if (np) {
        if (poly_start[0] != 0u) return B32_E_ARG;
        for (uint32_t p = 0; p < np; ++p) if (poly_start[p + 1] < poly_start[p]) return B32_E_ARG;
    }
    const uint32_t nh = np ? poly_start[np] : 0u;
    if (nh && !poly_verts) return B32_E_ARG;                                            // (empty polygons alone have no indices to read)
    (void)hipSetDevice(c->device);
    // half-edges in loop order, each with the id of its normalised edge (ids in the order of the sorted (min, max) pairs)
    std::vector<HoverHalfEdge> he(nh);
    std::vector<HoverFanTri> fan;
    std::vector<std::pair<unsigned long long, uint32_t>> keys(nh);
    for (uint32_t p = 0; p < np; ++p) {
        const uint32_t s = poly_start[p], n = poly_start[p + 1] - s;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t v0 = poly_verts[s + k], v1 = poly_verts[s + (k + 1u) % n];
            he[s + k] = HoverHalfEdge{ v0, v1, 0u, 0u };
            keys[s + k] = { ((unsigned long long)std::min(v0, v1) << 32) | std::max(v0, v1), s + k };
        }
        for (uint32_t k = 1; k + 1u < n; ++k) fan.push_back(HoverFanTri{ { poly_verts[s], poly_verts[s + k], poly_verts[s + k + 1u] }, p });
    }
    std::sort(keys.begin(), keys.end());
    uint32_t ne = 0;
    for (uint32_t j = 0; j < nh; ++j) {
        if (j && keys[j].first != keys[j - 1].first) ++ne;
        he[keys[j].second].edge = ne;
    }
    if (nh) ++ne;
    {   // the first half-edge of every edge in loop order (draw_box_selection_preview's HashSet, b32_overlay.hip)
        std::vector<uint8_t> seen(ne, 0);
        uint32_t rank = 0;
        for (uint32_t j = 0; j < nh; ++j) if (!seen[he[j].edge]) { seen[he[j].edge] = 1; he[j].first = ++rank; }
    }
    if (fan.size() >= 0xFFFFFFFFull) return B32_E_UNSUPPORTED;

    b32_topology* t = new b32_topology();
    t->np = np; t->nh = nh; t->nt = (uint32_t)fan.size(); t->ne = ne;
    if (np) t->h_poly_start.assign(poly_start, poly_start + (size_t)np + 1u); else t->h_poly_start.assign(1, 0u);
    const uint32_t zero = 0u;
    hipError_t e = hipSuccess;
    const auto up = [&](void** dst, const void* src, size_t bytes) {
        if (e != hipSuccess) return;
        e = hipMalloc(dst, bytes ? bytes : 4);
        if (e == hipSuccess && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
    };
    up(reinterpret_cast<void**>(&t->he), he.data(), (size_t)nh * sizeof(HoverHalfEdge));
    up(reinterpret_cast<void**>(&t->fan), fan.data(), fan.size() * sizeof(HoverFanTri));
    up(reinterpret_cast<void**>(&t->poly_start), np ? poly_start : &zero, ((size_t)np + 1u) * 4u);
    up(reinterpret_cast<void**>(&t->poly_verts), poly_verts, (size_t)nh * 4u);
    if (e != hipSuccess) {
        c->last_hip = (int)e;
        for (void* p : { (void*)t->he, (void*)t->fan, (void*)t->poly_start, (void*)t->poly_verts }) if (p) (void)hipFree(p);
        delete t;
        return B32_E_HIP;
    }
    *out = t;
    return B32_OK;
}

void b32_topology_destroy(b32_ctx* c, b32_topology* t) {
    if (!t) return;
    if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }     // (a hover that reads it may be in flight)
    for (void* p : { (void*)t->he, (void*)t->fan, (void*)t->poly_start, (void*)t->poly_verts }) if (p) (void)hipFree(p);
    delete t;
}

int b32_hover_mesh_async(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, b32_scene* slot, b32_topology* topo, const B32Placement* place,
                         const B32HoverParams* prm, void* out, uint64_t* ticket) {
    { const int rc = hover_common_check(c, cam, slot); if (rc) return rc; }
    if (!topo || !prm || (prm->flags & ~B32_HOVER_SEE_THROUGH) || prm->mirror_axis > 3u) return B32_E_ARG;
    if (!out || !ticket) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    int rc;
    HoverArgs a{};
    const bool cull = !(prm->flags & B32_HOVER_SEE_THROUGH);
    query_fill(a.q, c, cam, ortho, prm->mx, prm->my, cull);
    hover_item(a.it, slot, place);
    a.placed = place ? 1u : 0u;
    a.rest = slot->have_rig ? slot->d_rest : nullptr;
    a.he = topo->he; a.fan = topo->fan; a.poly_start = topo->poly_start; a.poly_verts = topo->poly_verts;
    a.np = topo->np; a.nh = topo->nh; a.nt = topo->nt;
    a.mirror_axis = prm->mirror_axis; a.mirror_thr = prm->mirror_threshold; a.vthr = prm->vertex_threshold; a.ethr = prm->edge_threshold;
    a.gv = hover_groups(a.it.nv); a.ge = hover_groups(a.nh);
    const uint32_t gf = hover_groups(a.nt);
    const unsigned long long groups = (unsigned long long)a.gv + a.ge + gf;
    if (groups >= (1ull << 31)) return B32_E_UNSUPPORTED;

    // the words: all ones whenever no hover is running (allocated so; k_hover_resolve leaves them so)
    if ((rc = armed_ensure(c, c->hover_words, sizeof(HoverWords), 0xFF))) return rc;
    a.words = static_cast<HoverWords*>(c->hover_words.p);
    // the bitmaps: all zero whenever no hover is running
    if (cull) {
        a.vwords = (uint32_t)(((unsigned long long)a.it.nv + 31u) / 32u); a.ewords = (uint32_t)(((unsigned long long)topo->ne + 31u) / 32u);
        if ((rc = armed_ensure(c, c->hover_bits, ((size_t)a.vwords + a.ewords) * 4u, 0))) return rc;
        a.vbits = static_cast<uint32_t*>(c->hover_bits.p); a.ebits = a.vbits + a.vwords;
    }

    unsigned long long t = 0; hipEvent_t* tev = nullptr; uint32_t k = 0;
    const size_t bytes = sizeof(B32HoverResult);
    if ((rc = pick_result_open(c, bytes, t, tev, k, &a.q.result))) return rc;
    const bool timed = c->profile_level >= 1;
    if (timed) HIPCHK(c, c->hover_timer.begin(c->stream));
    if (cull && a.np) hipLaunchKernelGGL(k_hover_front, dim3((a.np + 255u) / 256u), dim3(256), 0, c->stream, a);
    if (groups && a.rest) hipLaunchKernelGGL(k_hover<true>, dim3((uint32_t)groups), dim3(256), 0, c->stream, a);
    else if (groups) hipLaunchKernelGGL(k_hover<false>, dim3((uint32_t)groups), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_hover_resolve, dim3(1), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    if (timed) HIPCHK(c, c->hover_timer.end(c->stream));
    return pick_result_deliver(c, k, bytes, out, t, tev, ticket);
}

int b32_hover_mesh(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, b32_scene* slot, b32_topology* topo, const B32Placement* place,
                   const B32HoverParams* prm, B32HoverResult* out) {
    { const int rc = hover_common_check(c, cam, slot); if (rc) return rc; }
    if (!out) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    const unsigned char* h = nullptr;
    const int rc = pick_blocking(c, sizeof(B32HoverResult), &h, [&](void* landing, uint64_t* t) {
        return b32_hover_mesh_async(c, cam, ortho, slot, topo, place, prm, landing, t); });
    if (rc) return rc;
    std::memcpy(out, h, sizeof(B32HoverResult));
    return B32_OK;
}

int b32_box_select_async(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, b32_scene* slot, b32_topology* topo, const B32Placement* place,
                         const B32BoxParams* prm, void* out, uint64_t* ticket) {
    { const int rc = hover_common_check(c, cam, slot); if (rc) return rc; }
    if (!prm || prm->mode > B32_BOX_POLYGONS || (prm->mode == B32_BOX_POLYGONS && !topo) || !out || !ticket) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    BoxArgs a{};
    query_fill(a.q, c, cam, ortho, 0.0f, 0.0f, false);
    hover_item(a.it, slot, place);
    a.placed = place ? 1u : 0u;
    a.mode = prm->mode;
    if (a.mode == B32_BOX_POLYGONS) { a.n = topo->np; a.poly_start = topo->poly_start; a.poly_verts = topo->poly_verts; }
    else a.n = a.it.nv;
    a.nwords = (uint32_t)(((unsigned long long)a.n + 31u) / 32u);
    a.x0 = prm->x0; a.y0 = prm->y0; a.x1 = prm->x1; a.y1 = prm->y1;
    return box_run(c, a.nwords, &a.q.result, out, ticket, [&] {
        if (a.n) hipLaunchKernelGGL(k_box_select, dim3((uint32_t)(((unsigned long long)a.n + 255u) / 256u)), dim3(256), 0, c->stream, a); });
}

int b32_box_select(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, b32_scene* slot, b32_topology* topo, const B32Placement* place,
                   const B32BoxParams* prm, uint32_t* words, uint32_t* n_selected) {
    { const int rc = hover_common_check(c, cam, slot); if (rc) return rc; }
    if (!prm || prm->mode > B32_BOX_POLYGONS || (prm->mode == B32_BOX_POLYGONS && !topo) || !n_selected) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    const uint32_t n = prm->mode == B32_BOX_POLYGONS ? topo->np : slot->body_nv();
    const size_t nwords = (size_t)(((unsigned long long)n + 31u) / 32u);
    const unsigned char* h = nullptr;
    const int rc = pick_blocking(c, box_bytes(nwords), &h, [&](void* landing, uint64_t* t) {
        return b32_box_select_async(c, cam, ortho, slot, topo, place, prm, landing, t); });
    if (rc) return rc;
    box_landed(h, nwords, words, n_selected);
    return B32_OK;
}

}  // extern "C"
