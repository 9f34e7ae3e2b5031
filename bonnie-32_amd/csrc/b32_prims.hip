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
#include "b32_gizmo_body.h"

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

// ---------------------------------------------------------------- the records of b32_draw_gizmos (b32_gizmo.hip)
// The same pass over the four record kinds k_gizmo_project writes -- B32_LINE_2D, B32_LINE_3D_OVERLAY (walked), B32_PRIM_CIRCLE and the
// library-internal filled triangle (areas) -- as kernels of its own: k_prims_tile sits right under its register bound and does not learn
// the triangle.  A triangle's row span depends on y alone (draw_filled_triangle_3d, viewport_3d.rs:6314-6345), so it is an area kind:
// every lane computes the span of each of its four rows (a wave's lanes share the row) and tests its column.  An area entry is the six
// sorted integers of a triangle or a circle's centre and r * r: 44 bytes against PrimArea's 84, which a triangle would not fit anyway.
struct GizmoArea { int bx0, bx1, by0, by1; int v[6]; uint32_t kind; };

struct GizmoPass : PrimPass {
    struct Areas { GizmoArea ca[DRAW_CHUNK]; uint32_t careas; };
    // The box of a triangle for binning and the scan's tile test: min and max of its three points, padded where f32 cannot hold the
    // coordinates -- ax = x0 as f32 + (x2 - x0) as f32 * alpha rounds three times, each by at most half an ulp of a magnitude below 2^31
    // (64), so beyond 2^24 a span can leave the integer box by up to 192 columns: the margin is ((largest |x|) >> 22) + 2.  Rows are exact.
    __device__ static __forceinline__ bool bounds(const B32Prim& p, long long& x0, long long& x1, long long& y0, long long& y1) {
        if (p.kind != PRIM_TRIANGLE) return PrimPass::bounds(p, x0, x1, y0, y1);
        const int x2 = (int)f32_bits(p.z0), y2 = (int)f32_bits(p.z1);
        x0 = min(min(p.x0, p.x1), x2); x1 = max(max(p.x0, p.x1), x2); y0 = min(min(p.y0, p.y1), y2); y1 = max(max(p.y0, p.y1), y2);
        const long long pad = (max(llabs(x0), llabs(x1)) >> 22) + 2;
        x0 -= pad; x1 += pad;
        return true;
    }
    template <class S>
    __device__ static __forceinline__ bool entry(const B32Prim& p, uint32_t i, const DrawTile& t, S& sh) {
        if (p.kind <= B32_LINE_3D_ALPHA) {
            draw_line_entry(p, sh.ce[i], sh.cop[i], sh.ccol[i]);
            return false;
        }
        GizmoArea A{};
        A.kind = p.kind;
        uint32_t abyte = p.blend != B32_BLEND_ERASE ? 255u : 0u;                      // Color::to_bytes, types.rs:829-832
        if (p.kind == PRIM_TRIANGLE) {                                                  // viewport_3d.rs:6302-6314
            int x[3] = { p.x0, p.x1, (int)f32_bits(p.z0) }, y[3] = { p.y0, p.y1, (int)f32_bits(p.z1) };
            gizmo_tri_sort(x, y);
            A.v[0] = x[0]; A.v[1] = y[0]; A.v[2] = x[1]; A.v[3] = y[1]; A.v[4] = x[2]; A.v[5] = y[2];
            A.bx0 = t.cx0; A.bx1 = t.cx1; A.by0 = max(y[0], t.cy0); A.by1 = min(y[2], t.cy1);
            if (y[2] == y[0]) { A.bx0 = 1; A.bx1 = 0; }
            abyte = 255u;                                                               // pixels[idx + 3] = 255, :6353
        } else {                                                                        // B32_PRIM_CIRCLE, render.rs:631-642
            A.bx0 = max(p.x0 - p.size, t.cx0); A.bx1 = min(p.x0 + p.size, t.cx1); A.by0 = max(p.y0 - p.size, t.cy0); A.by1 = min(p.y0 + p.size, t.cy1);
            A.v[0] = p.x0; A.v[1] = p.y0; A.v[2] = p.size * p.size;
        }
        sh.ca[i] = A;
        sh.cop[i] = 0u;
        sh.ccol[i] = (uint32_t)p.r | ((uint32_t)p.g << 8) | ((uint32_t)p.b << 16) | (abyte << 24);
        return true;
    }
    template <class S>
    __device__ static __forceinline__ void area_bits(const S& sh, uint32_t areas, int x, int y0, uint32_t* abits) {
        for (uint32_t am = areas; am; am &= am - 1u) {
            const uint32_t k = (uint32_t)__builtin_ctz(am);
            const GizmoArea& A = sh.ca[k];
            if (x < A.bx0 || x > A.bx1) continue;
#pragma unroll
            for (uint32_t r = 0; r < DRAW_ROWS; ++r) {
                const int y = y0 + 4 * (int)r;
                if (y < A.by0 || y > A.by1) continue;
                bool hit;
                if (A.kind == PRIM_TRIANGLE) {
                    int xa, xb;                                                        // (x is inside the frame: .max(0) / .min(w - 1) change nothing)
                    hit = gizmo_tri_row(A.v[0], A.v[1], A.v[2], A.v[3], A.v[4], A.v[5], y, xa, xb) && x >= xa && x <= xb;
                } else {
                    const int dx = x - A.v[0], dy = y - A.v[1];
                    hit = dx * dx + dy * dy <= A.v[2];
                }
                if (hit) abits[r] |= 1u << k;
            }
        }
    }
};

__global__ void k_gizmo_bin(DrawArgs<B32Prim> a) { draw_bin<GizmoPass>(a); }
__global__ __launch_bounds__(DRAW_THREADS) void k_gizmo_tile(DrawArgs<B32Prim> a, PrimBatch batch) { draw_tile<GizmoPass, false>(a, batch); }

// (the records are always on the device: k_gizmo_project wrote them)
void launch_draw_gizmo(hipStream_t s, const DrawArgs<B32Prim>& a, const B32Prim*) {
    const uint32_t ntiles = a.tiles_x * a.tiles_y;
    if (!a.n || !ntiles) return;
    if (a.counters) hipLaunchKernelGGL(k_gizmo_bin, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_gizmo_tile, dim3(ntiles), dim3(DRAW_THREADS), 0, s, a, PrimBatch{});
}

}  // namespace b32
