// b32_lines.hip -- the reference Framebuffer's line family (draw_line, draw_line_alpha, draw_line_3d, draw_line_3d_overlay,
// draw_line_3d_alpha; render.rs:684-872) as one ordered pass: b32_draw_lines.
//
// Reference: each call walks its Bresenham line and, per on-screen pixel that passes the depth test (none for the 2-D kinds; `<`,
// `<=`, or `<=` against z * 0.995 for the 3-D ones), either replaces the pixel (set_pixel) or blends into it (set_pixel_alpha).
//
// GPU form: the ordered tile pass of b32_draw_pass.h with every entry walked (tile route: B32_ROUTE_LINE_TILES).  A line's box is the
// min / max of its end points, in i32; the player's cylinder (36 lines) is a small batch.
#include "b32_draw_pass.h"

namespace b32 {

struct LinePass {
    using Rec = B32Line;
    using Box = int;
    struct Areas {};
    static constexpr uint32_t SMALL = LINE_SMALL;
    __device__ static __forceinline__ bool bounds(const B32Line& l, int& x0, int& x1, int& y0, int& y1) {
        x0 = min(l.x0, l.x1); x1 = max(l.x0, l.x1); y0 = min(l.y0, l.y1); y1 = max(l.y0, l.y1);
        return true;
    }
    template <class S>
    __device__ static __forceinline__ bool entry(const B32Line& l, uint32_t i, const DrawTile&, S& sh) {
        draw_line_entry(l, sh.ce[i], sh.cop[i], sh.ccol[i]);
        return false;
    }
    __device__ static __forceinline__ uint32_t store(uint32_t o, uint32_t col, uint32_t c) {
        return (o & DOP_ALPHA) ? draw_blend_alpha(c, col, o >> 8) : col;        // set_pixel_alpha : set_pixel, render.rs:301-310
    }
};
using LineBatch = DrawBatch<B32Line, LINE_SMALL>;

__global__ void k_lines_bin(DrawArgs<B32Line> a) { draw_bin<LinePass>(a); }
template <bool SMALL>
__global__ __launch_bounds__(DRAW_THREADS) void k_lines_tile(DrawArgs<B32Line> a, LineBatch batch) { draw_tile<LinePass, SMALL>(a, batch); }

void launch_draw(hipStream_t s, const DrawArgs<B32Line>& a, const B32Line* small) {
    draw_launch(s, a, small, k_lines_bin, k_lines_tile<true>, k_lines_tile<false>);
}

}  // namespace b32
