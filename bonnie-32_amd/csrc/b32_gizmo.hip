// b32_gizmo.hip -- the world editor's overlay helpers projected into B32Prim records on the device (b32_draw_gizmos), and the items of
// draw_filled_octahedron.
//
// Reference: editor/viewport_3d.rs:5687-6357 -- draw_3d_line clips the projected f32 segment to the framebuffer (clip_line_to_rect, 16
// Cohen-Sutherland rounds) before it casts and walks; draw_3d_thick_line_depth draws `thickness` parallel overlay lines; draw_3d_point a
// circle; draw_filled_triangle_3d fills three projected points scan line by scan line.  The arithmetic is in b32_gizmo_body.h.
//
// GPU form: one lane per item, as k_world_project.  An item becomes one record, or `thickness` records for a thick line; where its first
// record lies depends on the kinds and sizes before it alone, so the host adds that up while it validates and copies the batch (GizmoRow)
// and the kernel needs no scan.  An item that draws nothing fills its place with circles of radius -1.  The records stay on the device:
// the ordered tile pass (GizmoPass, b32_prims.hip) reads them where this kernel wrote them.
#include "b32_gizmo_body.h"
#include "b32_item_kernels.h"

namespace b32 {

struct GizmoProject {
    using Args = GizmoArgs; using Row = GizmoRow;
    static constexpr uint32_t SMALL = GIZMO_SMALL;
    static __host__ __device__ uint32_t n(const GizmoArgs& a) { return a.w.n; }
    static __device__ const GizmoRow* rows(const GizmoArgs& a) { return a.rows; }
    // row i of the batch
    static __device__ __forceinline__ void item(const GizmoArgs& a, const GizmoRow& row, uint32_t, bool live) {
        uint32_t* tally = outcome_tally();
        uint32_t which = 3u;
        if (live) which = gizmo_item(a.w.v, row.it, a.w.out + row.first);
        outcome_count(tally, a.w.counts, which);
    }
};
// (4096 bytes is what a launch can carry; the pass's other batches stay under 2048, this one's rows are 52 bytes)
static_assert(sizeof(B32GizmoItem) == 48 && sizeof(GizmoRow) == 52 && sizeof(ItemBatch<GizmoProject>) + sizeof(GizmoArgs) <= 3072, "B32GizmoItem layout / kernel argument size");

__global__ __launch_bounds__(256) void k_gizmo_project_small(GizmoArgs a, ItemBatch<GizmoProject> batch) { item_small<GizmoProject>(a, batch); }
__global__ __launch_bounds__(256) void k_gizmo_project(GizmoArgs a) { item_large<GizmoProject>(a); }

void launch_gizmo_project(hipStream_t s, const GizmoArgs& a, const GizmoRow* small) {
    launch_items<GizmoProject>(s, k_gizmo_project_small, k_gizmo_project, a, small);
}

}  // namespace b32

// draw_filled_octahedron (viewport_3d.rs:6223-6292) as items, in call order.
extern "C" int b32_octahedron_items(const float center[3], float size, const uint8_t rgbb[4], B32GizmoItem out[20]) {
    if (!center || !rgbb || !out) return B32_E_ARG;
    const float cx = center[0], cy = center[1], cz = center[2];
    const float corner[6][3] = { { cx, cy + size, cz }, { cx, cy - size, cz }, { cx, cy, cz + size },          // top, bottom, front,
                                 { cx, cy, cz - size }, { cx - size, cy, cz }, { cx + size, cy, cz } };        // back, left, right
    enum { TOP, BOTTOM, FRONT, BACK, LEFT, RIGHT };
    static const uint8_t faces[8][3] = { { TOP, FRONT, RIGHT }, { TOP, RIGHT, BACK }, { TOP, BACK, LEFT }, { TOP, LEFT, FRONT },
                                         { BOTTOM, RIGHT, FRONT }, { BOTTOM, BACK, RIGHT }, { BOTTOM, LEFT, BACK }, { BOTTOM, FRONT, LEFT } };
    static const uint8_t edges[12][2] = { { TOP, FRONT }, { TOP, BACK }, { TOP, LEFT }, { TOP, RIGHT }, { BOTTOM, FRONT }, { BOTTOM, BACK },
                                          { BOTTOM, LEFT }, { BOTTOM, RIGHT }, { FRONT, RIGHT }, { RIGHT, BACK }, { BACK, LEFT }, { LEFT, FRONT } };
    auto put = [&](B32GizmoItem& it, int slot, int c) { float* p = slot == 0 ? it.p0 : slot == 1 ? it.p1 : it.p2; for (int k = 0; k < 3; ++k) p[k] = corner[c][k]; };
    for (int f = 0; f < 8; ++f) {
        B32GizmoItem it{};
        for (int k = 0; k < 3; ++k) put(it, k, faces[f][k]);
        it.r = rgbb[0]; it.g = rgbb[1]; it.b = rgbb[2]; it.blend = rgbb[3];
        it.kind = B32_GIZMO_TRIANGLE;
        out[f] = it;
    }
    for (int e = 0; e < 12; ++e) {
        B32GizmoItem it{};
        for (int k = 0; k < 2; ++k) put(it, k, edges[e][k]);
        it.r = (uint8_t)((uint16_t)rgbb[0] * 3 / 4); it.g = (uint8_t)((uint16_t)rgbb[1] * 3 / 4); it.b = (uint8_t)((uint16_t)rgbb[2] * 3 / 4);
        it.blend = B32_BLEND_OPAQUE;                // RasterColor::new
        it.kind = B32_GIZMO_LINE;
        out[8 + e] = it;
    }
    return B32_OK;
}
