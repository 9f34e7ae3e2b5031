// b32_room_overlay.hip -- the world editor's room overlays made into B32Prim records on the device from a room's resident sector table
// (b32_draw_room_overlay): k_room_overlay and the host's record count.
//
// Reference: draw_viewport_3d draws the selected / hovered vertices (editor/viewport_3d.rs:4273-4316), the selected edges (:4318-4402), the
// hovered edge and face (:4404-4658), draw_selection (:4862-5247) and the box-select preview (:5249-5362) from the sector heights.  After
// b32_room_update those exist in the room only, and the hover of the same frame on the device only, so the records are made where both
// are.  The arithmetic is in b32_room_overlay_body.h; where a record lies is decided by the host (room_overlay_layout) from n, the
// B32RoomOverlay and the lists, never from the camera or the heights.
//
// GPU form: k_overlay_emit's.  One launch of 256-lane workgroups over seven ranges of work, a workgroup inside exactly one of them (the
// section branch is workgroup-uniform): VERTICES slots, EDGES pairs, the hover's two slot groups, SELECTED faces, SELECTED edges, PREVIEW
// records, PREVIEW points -- one lane per slot group (a face's six records, a record's four).  The arguments travel by value in the
// launch.  A lane reads its record where it lies in the room's table and computes a corner from it with a run-time corner index
// (room_corner's selectors): no per-lane corner array, no scratch (k_room_mesh's idiom).  The hover record is read by every lane at one
// address (hover_source 1: the room's device copy, filled behind k_room_hover_resolve on the stream) and the winner rule runs in the lane.
// Drawn / dropped / rejected: a lane's calls in three 10-bit fields of one word, through the shared counting tail (b32_item_kernels.h).
// The records stay on the device: the ordered tile pass of b32_prims.hip reads them where this kernel wrote them.  No new record kind.
#include "b32_host.h"
#include "b32_item_kernels.h"
#include "b32_room_overlay_body.h"

namespace b32 {

static_assert(sizeof(B32RoomOverlay) == 100 && offsetof(B32RoomOverlay, hover) == 8 && offsetof(B32RoomOverlay, primary_vertex) == 56 &&
              offsetof(B32RoomOverlay, x0) == 84 && sizeof(RoomOverlayArgs) <= 1024, "B32RoomOverlay layout / kernel argument size");

__global__ __launch_bounds__(256) void k_room_overlay(RoomOverlayArgs a) {
    uint32_t* tally = outcome_tally();
    uint32_t wg = blockIdx.x;
    const uint32_t i = threadIdx.x;
    B32Prim* out = a.out;
    uint32_t mine = 0u;                             // this lane's calls (room_overlay_tally)
    if (wg < a.g_vertices) {                        // :4273-4316
        const uint32_t p = wg * 256u + i;
        if (p <= a.o.n_vertices) {
            const B32RoomHover h = a.hover ? *a.hover : a.o.hover;
            const uint32_t hover_key = room_hover_winner(h) == 0 ? h.vertex_rec * 4u + (h.vertex_corner & 3u) : ROOM_OVERLAY_NONE;
            mine = room_overlay_vertex(a.v, a.grid, a.faces, a.n, a.lists, a.o.n_vertices, a.o.primary_vertex,
                                       (hover_key != ROOM_OVERLAY_NONE && h.vertex_rec < a.n) ? hover_key : ROOM_OVERLAY_NONE, p, out + a.at_vertices + p);
        }
    } else if ((wg -= a.g_vertices) < a.g_edges) {  // :4318-4402
        const uint32_t e = wg * 256u + i;
        if (e < a.o.n_edges) {
            const uint32_t rec = a.lists[a.l_edges + 2u * e], idx = a.lists[a.l_edges + 2u * e + 1u];
            B32Prim* o = out + a.at_edges + e;
            *o = prim_noop();
            if (rec < a.n) mine = room_overlay_thick_edge(a.v, a.grid, a.faces[rec], idx & 3u, ROOM_OVERLAY_SELECTED_VERTEX, o);
        }
    } else if ((wg -= a.g_edges) < a.g_hover) {     // :4404-4658: lane 0 the edge, lane 1 the face
        if (i < 2u) {
            const B32RoomHover h = a.hover ? *a.hover : a.o.hover;
            const int winner = room_hover_winner(h);
            B32Prim* o = out + a.at_hover;
            if (i == 0u) {
                *o = prim_noop();
                if (winner == 1 && h.edge_rec < a.n) mine = room_overlay_thick_edge(a.v, a.grid, a.faces[h.edge_rec], h.edge_idx & 3u, ROOM_OVERLAY_HOVER_EDGE, o);
            } else {
                const bool skipped = h.face_rec >= a.o.skip_first && h.face_rec - a.o.skip_first < a.o.skip_count;
                if (winner == 2 && h.face_rec < a.n && !skipped)
                    mine = room_overlay_face(a.v, a.grid, a.faces[h.face_rec], a.mats ? a.mats + h.face_rec : nullptr, ROOM_OVERLAY_HOVER_FACE, o + 1);
                else
                    for (uint32_t j = 0; j < ROOM_OVERLAY_FACE_SLOTS; ++j) o[1u + j] = prim_noop();
            }
        }
    } else if ((wg -= a.g_hover) < a.g_sel_faces) { // :4868-5047
        const uint32_t k = wg * 256u + i;
        if (k < a.o.n_faces) {
            const uint32_t rec = a.lists[a.l_faces + k];
            B32Prim* o = out + a.at_sel_faces + (size_t)k * ROOM_OVERLAY_FACE_SLOTS;
            if (rec < a.n) mine = room_overlay_face(a.v, a.grid, a.faces[rec], a.mats ? a.mats + rec : nullptr, ROOM_OVERLAY_SELECT, o);
            else for (uint32_t j = 0; j < ROOM_OVERLAY_FACE_SLOTS; ++j) o[j] = prim_noop();
        }
    } else if ((wg -= a.g_sel_faces) < a.g_sel_edges) {     // :5174-5236
        const uint32_t e = wg * 256u + i;
        if (e < a.o.n_edges) {
            const uint32_t rec = a.lists[a.l_edges + 2u * e], idx = a.lists[a.l_edges + 2u * e + 1u];
            B32Prim* o = out + a.at_sel_edges + e;
            if (rec < a.n) mine = room_overlay_line_edge(a.v, a.grid, a.faces[rec], idx & 3u, ROOM_OVERLAY_SELECT, o);
            else *o = prim_noop();
        }
    } else if ((wg -= a.g_sel_edges) < a.g_preview) {       // :5267-5340
        const uint32_t rec = wg * 256u + i;
        if (rec < a.n) mine = room_overlay_preview(a.v, a.grid, a.faces[rec], a.rect[0], a.rect[1], a.rect[2], a.rect[3], out + a.at_preview + (size_t)rec * ROOM_OVERLAY_PREVIEW_SLOTS);
    } else {                                        // :5341-5352
        wg -= a.g_preview;
        const uint32_t j = wg * 256u + i;
        if (j < a.o.n_points) {
            const uint32_t* w = a.lists + a.l_points + (size_t)j * 3u;
            const float p[3] = { __uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]) };
            mine = room_overlay_preview_point(a.v, p, a.rect[0], a.rect[1], a.rect[2], a.rect[3], out + a.at_points + (size_t)j * ROOM_OVERLAY_POINT_SLOTS);
        }
    }
    // (every lane of the workgroup arrives here: no early return above)
    outcome_count_packed(tally, a.counts, mine);
}

void launch_room_overlay(hipStream_t s, const RoomOverlayArgs& a) {
    const unsigned long long groups = (unsigned long long)a.g_vertices + a.g_edges + a.g_hover + a.g_sel_faces + a.g_sel_edges + a.g_preview + a.g_points;
    if (groups) hipLaunchKernelGGL(k_room_overlay, dim3((uint32_t)groups), dim3(256), 0, s, a);
}

}  // namespace b32

extern "C" int b32_room_overlay_record_count(const b32_room* room, const B32RoomOverlay* o, const uint32_t* sel_edges, const uint32_t* sel_faces, uint32_t* n) {
    if (!room || !o || !n) return B32_E_ARG;
    if ((o->sections & ~ROOM_OVERLAY_ALL) || o->hover_source > 1u || (o->n_edges && !sel_edges) || (o->n_faces && !sel_faces)) return B32_E_ARG;
    for (uint32_t i = 0; i < o->n_edges; ++i) if (sel_edges[2u * (size_t)i + 1u] > 3u) return B32_E_ARG;
    const RoomOverlayLayout l = room_overlay_layout(room->n, *o);
    if (l.total > 0x7FFFFFFFull) return B32_E_UNSUPPORTED;
    *n = (uint32_t)l.total;
    return B32_OK;
}
