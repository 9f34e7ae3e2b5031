// b32_prims.hip -- the rest of the reference Framebuffer's drawing methods (draw_circle, draw_circle_alpha, draw_line_blended,
// draw_thick_line, draw_rect, draw_filled_rect; render.rs:631-971) in one ordered pass with the line family: b32_draw_prims.
//
// Reference: every call writes its pixels one after another through set_pixel (replace, Color::to_bytes), set_pixel_alpha (integer
// blend, alpha 255) or set_pixel_blended (the PS1 blend by mode, render.rs:313-334).
//
// GPU form: the ordered tile pass of b32_draw_pass.h (tile route: B32_ROUTE_PRIM_TILES).  The bits of a pixel's mask come from two places:
//   * walked kinds (0..5, and a thick line of thickness <= 1, which is draw_line): eight lanes per primitive walk its Bresenham steps
//     inside the tile and atomicOr the bit into the pixel's LDS mask, as in the line pass;
//   * area kinds (circles, a thick line of thickness > 1, rectangles): decided pixel-major inside the fold -- every lane tests its own
//     pixels against the chunk's area primitives (no atomics).  A primitive's exact box (clipped to the tile) and, for a thick line,
//     its four f32 corners are computed once per chunk into LDS.  draw_rect's four opaque draw_line edges of one colour are exactly
//     the border of the normalised rectangle (a horizontal or vertical Bresenham line covers every pixel between its ends), so a
//     rectangle is one bit too.
// Binning and the scan's tile test use a conservative box per kind (PrimPass::bounds); the exact box decides only the pixels.
#include "b32_draw_pass.h"
#include "b32_fill_common.h"

namespace b32 {

using PrimBatch = DrawBatch<B32Prim, PRIM_SMALL>;
static_assert(sizeof(B32Prim) == 40 && sizeof(PrimBatch) <= 2048, "B32Prim layout / kernel argument size");

// an area primitive of the chunk: its exact box clipped to the tile (empty: bx0 > bx1), and per kind
//   circle: v = centre x, centre y, r * r;  rect: v = min_x, min_y, max_x, max_y;  thick line: q = the four corners (x, y)
struct PrimArea { int bx0, bx1, by0, by1; int v[4]; float q[8]; uint32_t kind; };

struct PrimPass {
    using Rec = B32Prim;
    using Box = long long;
    struct Areas { PrimArea ca[DRAW_CHUNK]; uint32_t careas; };
    static constexpr uint32_t SMALL = PRIM_SMALL;
    // 64-bit: the corners of a thick line reach 2^31 + 2^30.  A thick line's pixel centres lie within `half` of the segment; its f32
    // corners are rounded from integers up to 2^31 and the half-width (relative error 2^-24 each), hence the margin of
    // ((|coordinate| + thickness) >> 22) + 2.
    __device__ static __forceinline__ bool bounds(const B32Prim& p, long long& x0, long long& x1, long long& y0, long long& y1) {
        if (p.kind == B32_PRIM_CIRCLE || p.kind == B32_PRIM_CIRCLE_ALPHA) {
            if (p.size < 0) return false;
            x0 = (long long)p.x0 - p.size; x1 = (long long)p.x0 + p.size; y0 = (long long)p.y0 - p.size; y1 = (long long)p.y0 + p.size;
            return true;
        }
        x0 = min(p.x0, p.x1); x1 = max(p.x0, p.x1); y0 = min(p.y0, p.y1); y1 = max(p.y0, p.y1);
        if (p.kind == B32_PRIM_THICK_LINE && p.size > 1) {
            if (p.x0 == p.x1 && p.y0 == p.y1) return false;                 // len < 0.001
            const long long m = max(max(llabs((long long)p.x0), llabs((long long)p.x1)), max(llabs((long long)p.y0), llabs((long long)p.y1)));
            const long long pad = (long long)p.size / 2 + 2 + ((m + p.size) >> 22);
            x0 -= pad; x1 += pad; y0 -= pad; y1 += pad;
        }
        return true;
    }
    template <class S>
    __device__ static __forceinline__ bool entry(const B32Prim& p, uint32_t i, const DrawTile& t, S& sh) {
        if (p.kind <= B32_PRIM_LINE_BLENDED || (p.kind == B32_PRIM_THICK_LINE && p.size <= 1)) {
            draw_line_entry(p, sh.ce[i], sh.cop[i], sh.ccol[i]);
            if (p.kind == B32_PRIM_LINE_BLENDED && p.mode != B32_BLEND_OPAQUE) {
                sh.cop[i] |= DOP_PS1;
                sh.ccol[i] = (sh.ccol[i] & 0xFFFFFFu) | ((uint32_t)p.mode << 24);
            }
            return false;
        }
        PrimArea A{};
        A.kind = p.kind;
        int bx0, bx1, by0, by1;
        if (p.kind == B32_PRIM_CIRCLE || p.kind == B32_PRIM_CIRCLE_ALPHA) {           // render.rs:631-642, 670-681
            bx0 = p.x0 - p.size; bx1 = p.x0 + p.size; by0 = p.y0 - p.size; by1 = p.y0 + p.size;
            A.v[0] = p.x0; A.v[1] = p.y0; A.v[2] = p.size * p.size;
        } else if (p.kind == B32_PRIM_THICK_LINE) {                                     // render.rs:875-938, thickness > 1
            const float dx = (float)(p.x1 - p.x0), dy = (float)(p.y1 - p.y0);
            const float len = __builtin_sqrtf(dx * dx + dy * dy);
            const float half = (float)p.size * 0.5f;
            const float px = -dy / len * half, py = dx / len * half;
            const float fx0 = (float)p.x0, fy0 = (float)p.y0, fx1 = (float)p.x1, fy1 = (float)p.y1;
            A.q[0] = fx0 + px; A.q[1] = fy0 + py;
            A.q[2] = fx0 - px; A.q[3] = fy0 - py;
            A.q[4] = fx1 - px; A.q[5] = fy1 - py;
            A.q[6] = fx1 + px; A.q[7] = fy1 + py;
            float mnx = __builtin_inff(), mxx = -__builtin_inff(), mny = __builtin_inff(), mxy = -__builtin_inff();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                mnx = rmin(mnx, A.q[2 * k]); mxx = rmax(mxx, A.q[2 * k]);
                mny = rmin(mny, A.q[2 * k + 1]); mxy = rmax(mxy, A.q[2 * k + 1]);
            }
            bx0 = f2i32_sat(mnx); bx1 = f2i32_sat(mxx); by0 = f2i32_sat(mny); by1 = f2i32_sat(mxy);
            if (len < 0.001f) { bx0 = 1; bx1 = 0; }
        } else {                                                                       // draw_rect / draw_filled_rect, render.rs:941-971
            bx0 = min(p.x0, p.x1); bx1 = max(p.x0, p.x1); by0 = min(p.y0, p.y1); by1 = max(p.y0, p.y1);
            A.v[0] = bx0; A.v[1] = by0; A.v[2] = bx1; A.v[3] = by1;
        }
        A.bx0 = max(bx0, t.cx0); A.bx1 = min(bx1, t.cx1); A.by0 = max(by0, t.cy0); A.by1 = min(by1, t.cy1);
        sh.ca[i] = A;
        const bool blend = p.kind == B32_PRIM_CIRCLE_ALPHA;
        const uint32_t abyte = (blend || p.blend != B32_BLEND_ERASE) ? 255u : 0u;     // Color::to_bytes, types.rs:829-832
        sh.cop[i] = (blend ? DOP_ALPHA : 0u) | ((uint32_t)p.alpha << 8);
        sh.ccol[i] = (uint32_t)p.r | ((uint32_t)p.g << 8) | ((uint32_t)p.b << 16) | (abyte << 24);
        return true;
    }
    // the area kinds, pixel-major: column x, rows y0 + 4 r
    template <class S>
    __device__ static __forceinline__ void area_bits(const S& sh, uint32_t areas, int x, int y0, uint32_t* abits) {
        for (uint32_t am = areas; am; am &= am - 1u) {
            const uint32_t k = (uint32_t)__builtin_ctz(am);
            const PrimArea& A = sh.ca[k];
            if (x < A.bx0 || x > A.bx1) continue;
#pragma unroll
            for (uint32_t r = 0; r < DRAW_ROWS; ++r) {
                const int y = y0 + 4 * (int)r;
                if (y < A.by0 || y > A.by1) continue;
                bool hit;
                if (A.kind == B32_PRIM_CIRCLE || A.kind == B32_PRIM_CIRCLE_ALPHA) {
                    const int dx = x - A.v[0], dy = y - A.v[1];             // |dx|, |dy| <= radius <= 32767 inside the box: exact in i32
                    hit = dx * dx + dy * dy <= A.v[2];
                } else if (A.kind == B32_PRIM_THICK_LINE) {
                    const float p0 = (float)x + 0.5f, p1 = (float)y + 0.5f;
                    hit = true;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {                               // cross < 0.0: outside (-0.0 is inside)
                        const float ax = A.q[2 * e], ay = A.q[2 * e + 1], bx = A.q[(2 * e + 2) & 7], by = A.q[(2 * e + 3) & 7];
                        const float cross = (bx - ax) * (p1 - ay) - (by - ay) * (p0 - ax);
                        hit = hit && !(cross < 0.0f);
                    }
                } else if (A.kind == B32_PRIM_RECT) {
                    hit = x == A.v[0] || x == A.v[2] || y == A.v[1] || y == A.v[3];
                } else {
                    hit = true;
                }
                if (hit) abits[r] |= 1u << k;
            }
        }
    }
    __device__ static __forceinline__ uint32_t store(uint32_t o, uint32_t col, uint32_t c) {
        if (o & DOP_ALPHA) return draw_blend_alpha(c, col, (o >> 8) & 255u);
        if (o & DOP_PS1) return store8(c, col, 255u);                          // Color::blend(back opaque, mode)
        return col;                                                             // set_pixel, render.rs:301-310
    }
};

__global__ void k_prims_bin(DrawArgs<B32Prim> a) { draw_bin<PrimPass>(a); }
// (at most 128 VGPRs, four waves per SIMD: without the bound the small-batch form drifts to 136 and loses a wave)
template <bool SMALL>
__global__ __launch_bounds__(DRAW_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void k_prims_tile(DrawArgs<B32Prim> a, PrimBatch batch) { draw_tile<PrimPass, SMALL>(a, batch); }

void launch_draw(hipStream_t s, const DrawArgs<B32Prim>& a, const B32Prim* small) {
    draw_launch(s, a, small, k_prims_bin, k_prims_tile<true>, k_prims_tile<false>);
}

}  // namespace b32
