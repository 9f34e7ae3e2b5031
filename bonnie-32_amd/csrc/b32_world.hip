// b32_world.hip -- world-space overlay items projected into B32Prim records on the device (b32_draw_world), and the floor grid's segments.
//
// Reference: every overlay starts from world positions.  draw_3d_line_clipped (rasterizer/draw.rs:12-67) clips a segment against the near
// plane in world space, projects both ends with world_to_screen (math.rs:503-534), casts with `as i32` and calls fb.draw_line; the modeler
// projects with world_to_screen_with_ortho[_depth] (math.rs:538-617) and calls draw_line_3d[_alpha] / draw_circle[_alpha].  Whether a
// clipped segment is drawn at all can hang on the last bit of p0 + (p1 - p0) * t: the clipped end is projected again and answers None when
// its camera z comes out <= 0.1.
//
// GPU form: one lane per item through world_item (b32_world_body.h: the reference's expressions in the reference's order).  Record i is
// written from item i, so the array order is the reference's call order; an item that draws nothing becomes the no-op record, which the
// tile pass skips (PrimPass::bounds).  The records stay on the device: the ordered tile pass of b32_prims.hip reads them where this
// kernel wrote them.
#include "b32_item_kernels.h"
#include "b32_world_body.h"
#include <cmath>

namespace b32 {

struct WorldProject {
    using Args = WorldArgs; using Row = B32WorldItem;
    static constexpr uint32_t SMALL = WORLD_SMALL;
    static __host__ __device__ uint32_t n(const WorldArgs& a) { return a.n; }
    static __device__ const B32WorldItem* rows(const WorldArgs& a) { return a.items; }
    static __device__ void item(const WorldArgs& a, const B32WorldItem& it, uint32_t i, bool live);
};
static_assert(sizeof(B32WorldItem) == 40 && sizeof(ItemBatch<WorldProject>) + sizeof(WorldArgs) <= 2048, "B32WorldItem layout / kernel argument size");

// item i of the batch (a lane without one works on a zeroed item and counts nothing)
__device__ __forceinline__ void WorldProject::item(const WorldArgs& a, const B32WorldItem& it, uint32_t i, bool live) {
    uint32_t* tally = outcome_tally();
    B32Prim o;
    const uint32_t which = world_item(a.v, it, &o);
    if (live) a.out[i] = o;
    outcome_count(tally, a.counts, live ? which : 3u);
}

__global__ __launch_bounds__(256) void k_world_project_small(WorldArgs a, ItemBatch<WorldProject> batch) { item_small<WorldProject>(a, batch); }
__global__ __launch_bounds__(256) void k_world_project(WorldArgs a) { item_large<WorldProject>(a); }

void launch_world_project(hipStream_t s, const WorldArgs& a, const B32WorldItem* small) {
    launch_items<WorldProject>(s, k_world_project_small, k_world_project, a, small);
}

}  // namespace b32

// draw_floor_grid's two while loops (draw.rs:81-135) as items, in call order.  An accumulation that does not advance is the reference's
// endless loop: found here, never by looping.
extern "C" int b32_floor_grid_items(float y, float spacing, float extent, const uint8_t grid_rgbb[4], const uint8_t x_axis_rgbb[4],
                                    const uint8_t z_axis_rgbb[4], B32WorldItem* out, uint32_t cap, uint32_t* n) {
    if (!n || !grid_rgbb || !x_axis_rgbb || !z_axis_rgbb) return B32_E_ARG;
    *n = 0;
    if (!std::isfinite(y) || !std::isfinite(spacing) || !std::isfinite(extent) || !(spacing > 0.0f)) return B32_E_ARG;
    constexpr uint32_t MAX_SEGMENTS = 1u << 20;
    const float segment_length = spacing;
    uint32_t count = 0;
    for (int pass = 0; pass < 2; ++pass) {                      // 0: X-parallel lines (fixed Z), 1: Z-parallel lines (fixed X)
        float u = -extent;                                      // the fixed coordinate
        while (u <= extent) {
            const bool axis = std::fabs(u) < 0.001f;
            const uint8_t* col = axis ? (pass == 0 ? z_axis_rgbb : x_axis_rgbb) : grid_rgbb;
            float v = -extent;
            while (v < extent) {
                const float v_end = std::fmin(v + segment_length, extent);
                if (count >= MAX_SEGMENTS) return B32_E_UNSUPPORTED;
                if (out && count < cap) {
                    B32WorldItem it{};
                    it.p0[0] = pass == 0 ? v : u; it.p0[1] = y; it.p0[2] = pass == 0 ? u : v;
                    it.p1[0] = pass == 0 ? v_end : u; it.p1[1] = y; it.p1[2] = pass == 0 ? u : v_end;
                    it.r = col[0]; it.g = col[1]; it.b = col[2]; it.blend = col[3];
                    it.kind = B32_LINE_2D; it.alpha = 255; it.flags = B32_WORLD_CLIP_NEAR;
                    out[count] = it;
                }
                ++count;
                const float next = v + segment_length;
                if (!(next > v)) return B32_E_ARG;
                v = next;
            }
            const float next = u + spacing;
            if (!(next > u)) return B32_E_ARG;
            u = next;
        }
    }
    *n = count;
    return B32_OK;
}
