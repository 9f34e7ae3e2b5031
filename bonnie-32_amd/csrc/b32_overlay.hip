// b32_overlay.hip -- the modeler's selection overlays made into B32Prim records on the device from a slot's resident vertices
// (b32_draw_mesh_overlay): k_overlay_points, k_overlay_emit and the host's record count.
//
// Reference: draw_selected_object_brackets (modeler/viewport.rs:1782-1884), draw_mesh_selection_overlays (:1890-2105) and
// draw_box_selection_preview (:2108-2247) start from the selected object's posed positions.  After b32_scene_pose those exist in the slot
// only, so the records are made where the vertices are.  The arithmetic is in b32_overlay_body.h; where a record lies is decided by the
// host (overlay_layout) from the topology, nv, the B32MeshOverlay and the selected list, never from the camera.
//
// GPU form.
//   k_overlay_points  one lane per vertex: the vertex is projected ONCE into a 16-byte table entry (sx, sy, camera z, projected).
//                     world_point is pure, so the entry is bit for bit what each of the reference's repeated projections of that vertex
//                     gives; the edge lanes would otherwise project every vertex about twice its valence times.  The lane also writes the
//                     vertex's dot record and its preview-vertex record, and feeds the brackets' bounds.
//                     The bounds: min starts at f32::MAX, max at f32::MIN, f32::min / f32::max ignore a NaN, so the result is the minimum /
//                     maximum of the non-NaN coordinates -- a function of the SET of values, not of the order of the walk.  The sign of a
//                     zero is the only thing an order could change, and it disappears in the margin (-0.0 - 4.0 == 0.0 - 4.0).  So the
//                     reduction runs as unsigned minima / maxima of a monotone key (overlay_key: the map the hover's minima use): shuffles
//                     in the wave, LDS across the waves, then ONE memory atomic per workgroup and component; a lane with a NaN takes no
//                     part.  It is never a serial walk.
//   k_overlay_emit    launched behind it on the stream, so the table and the bounds are complete.  One launch over six ranges of work, a
//                     workgroup inside exactly one of them (the section branch is workgroup-uniform, as k_hover's gv / ge ranges):
//                     half-edges (EDGES), half-edges (edge PREVIEW: only the first half-edge of an edge has records), the selected list,
//                     polygons (face PREVIEW), the hovered element, the brackets.  A polygon lane streams its vertices (overlay_polygon):
//                     no per-lane array, no scratch.  The brackets' workgroup reads the bounds with 24 lanes and arms them again for the
//                     next call on the stream.
// The records stay on the device: the ordered tile pass of b32_prims.hip reads them where these kernels wrote them.  No new record kind.
#include "b32_host.h"
#include "b32_item_kernels.h"
#include "b32_overlay_body.h"

namespace b32 {

static_assert(sizeof(OverlayPoint) == 16 && sizeof(OverlayBounds) == 24 && sizeof(B32MeshOverlay) == 48 && sizeof(OverlayArgs) <= 1024,
              "overlay records / kernel argument size");

__global__ __launch_bounds__(256) void k_overlay_points(OverlayArgs a) {
    __shared__ OverlayBounds wg;
    const bool brackets = (a.o.sections & B32_OVERLAY_BRACKETS) != 0u;
    if (brackets) {
        if (threadIdx.x < 3u) { wg.mn[threadIdx.x] = OVERLAY_KEY_MIN0; wg.mx[threadIdx.x] = OVERLAY_KEY_MAX0; }
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    OverlayBounds b = overlay_bounds_start();
    if (i < a.nv) {
        const float* src = a.pos + (size_t)i * a.stride;
        const float p[3] = { src[0], src[1], src[2] };
        const OverlayPoint e = overlay_point(a.v, p);
        a.tab[i] = e;
        if (a.o.sections & B32_OVERLAY_DOTS) a.out[a.at_dots + i] = overlay_dot(e);
        if ((a.o.sections & B32_OVERLAY_PREVIEW) && a.o.preview_mode == 0u) {
            const float rect[4] = { a.o.x0, a.o.y0, a.o.x1, a.o.y1 };
            a.out[a.at_preview + i] = overlay_preview_vertex(e, rect);
        }
        if (brackets) overlay_bounds_take(b, p);
    }
    if (!brackets) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t lo = overlay_wave_min(b.mn[c]), hi = overlay_wave_max(b.mx[c]);
        if ((threadIdx.x & 63u) == 0u) { atomicMin(&wg.mn[c], lo); atomicMax(&wg.mx[c], hi); }
    }
    __syncthreads();
    if (threadIdx.x < 3u) {
        const uint32_t c = threadIdx.x;
        if (wg.mn[c] != OVERLAY_KEY_MIN0) __hip_atomic_fetch_min(&a.bounds->mn[c], wg.mn[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (wg.mx[c] != OVERLAY_KEY_MAX0) __hip_atomic_fetch_max(&a.bounds->mx[c], wg.mx[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_overlay_emit(OverlayArgs a) {
    uint32_t wg = blockIdx.x;
    const OverlayPoint* tab = a.tab;
    const float rect[4] = { a.o.x0, a.o.y0, a.o.x1, a.o.y1 };
    B32Prim* out = a.out;
    if (wg < a.g_edges) {                           // :1924-1935
        const uint32_t h = wg * 256u + threadIdx.x;
        if (h >= a.nh) return;
        const HoverHalfEdge e = a.he[h];
        out[a.at_edges + h] = overlay_edge(e.v0, e.v1, a.nv, tab);
        return;
    }
    wg -= a.g_edges;
    if (wg < a.g_pedges) {                          // :2183-2205
        const uint32_t h = wg * 256u + threadIdx.x;
        if (h >= a.nh) return;
        const HoverHalfEdge e = a.he[h];
        if (e.first) overlay_preview_edge(e.v0, e.v1, a.nv, tab, rect, out + a.at_preview + 2u * (e.first - 1u));
        return;
    }
    wg -= a.g_pedges;
    if (wg < a.g_sel) {                             // :2025-2104
        const uint32_t i = wg * 256u + threadIdx.x;
        if (i >= a.n_sel) return;
        if (a.o.select_kind == 1u) {
            out[a.at_selected + i] = overlay_selected_vertex(a.selected[i], a.nv, tab);
        } else if (a.o.select_kind == 2u) {
            overlay_selected_edge(a.selected[2u * i], a.selected[2u * i + 1u], a.nv, tab, out + a.at_selected + 4u * i);
        } else {
            const uint32_t p = a.selected[2u * i], first = a.selected[2u * i + 1u];      // (p < np: the host left the others out)
            const uint32_t s = a.poly_start[p], e = a.poly_start[p + 1u];
            overlay_polygon(a.v, OVERLAY_POLY_SELECTED, a.poly_verts + s, e - s, a.pos, a.stride, a.nv, tab, rect, out + first);
        }
        return;
    }
    wg -= a.g_sel;
    if (wg < a.g_pfaces) {                          // :2210-2244
        const uint32_t p = wg * 256u + threadIdx.x;
        if (p >= a.np) return;
        const uint32_t s = a.poly_start[p], e = a.poly_start[p + 1u];
        overlay_polygon(a.v, OVERLAY_POLY_PREVIEW, a.poly_verts + s, e - s, a.pos, a.stride, a.nv, tab, rect, out + a.at_preview + s + p);
        return;
    }
    wg -= a.g_pfaces;
    if (wg < a.g_hover) {                           // :1960-2020: one lane per element
        if (threadIdx.x == 0u && a.o.hover_vertex != OVERLAY_NONE) out[a.at_hover_vertex] = overlay_hover_vertex(a.o.hover_vertex, a.nv, tab);
        if (threadIdx.x == 1u && (a.o.hover_edge_v0 != OVERLAY_NONE || a.o.hover_edge_v1 != OVERLAY_NONE))
            overlay_hover_edge(a.o.hover_edge_v0, a.o.hover_edge_v1, a.nv, tab, out + a.at_hover_edge);
        if (threadIdx.x == 2u && a.hover_face_cnt) {
            const uint32_t s = a.poly_start[a.o.hover_face];
            overlay_polygon(a.v, OVERLAY_POLY_HOVER, a.poly_verts + s, a.hover_face_cnt, a.pos, a.stride, a.nv, tab, rect, out + a.at_hover_face);
        }
        return;
    }
    // the brackets, :1821-1883: the bounds are complete (k_overlay_points ran before this kernel on the stream)
    const OverlayBounds b = *a.bounds;
    if (threadIdx.x < 24u) out[a.at_brackets + threadIdx.x] = overlay_bracket(a.v, b, threadIdx.x);
    __syncthreads();                                // every lane has read the bounds
    if (threadIdx.x < 3u) { a.bounds->mn[threadIdx.x] = OVERLAY_KEY_MIN0; a.bounds->mx[threadIdx.x] = OVERLAY_KEY_MAX0; }
}

void launch_overlay(hipStream_t s, const OverlayArgs& a) {
    if (a.nv) hipLaunchKernelGGL(k_overlay_points, dim3((uint32_t)(((unsigned long long)a.nv + 255u) / 256u)), dim3(256), 0, s, a);
    const unsigned long long groups = (unsigned long long)a.g_edges + a.g_pedges + a.g_sel + a.g_pfaces + a.g_hover + a.g_brackets;
    if (groups) hipLaunchKernelGGL(k_overlay_emit, dim3((uint32_t)groups), dim3(256), 0, s, a);
}

}  // namespace b32

extern "C" int b32_mesh_overlay_record_count(const b32_topology* t, uint32_t nv, const B32MeshOverlay* o, const uint32_t* selected, uint32_t* n) {
    if (!o || !n) return B32_E_ARG;
    { const int rc = overlay_check(t != nullptr, o, selected); if (rc) return rc; }
    const OverlayLayout l = overlay_layout(t ? t->h_poly_start.data() : nullptr, t ? t->np : 0u, t ? t->nh : 0u, t ? t->ne : 0u, nv, *o, selected);
    if (l.total > 0x7FFFFFFFull) return B32_E_UNSUPPORTED;
    *n = (uint32_t)l.total;
    return B32_OK;
}
