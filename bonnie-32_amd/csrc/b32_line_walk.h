// b32_line_walk.h -- the reference's Bresenham (draw_line / draw_line_3d_impl / draw_line_3d_alpha, render.rs:684-872) in closed form,
// shared by the wireframe phases (b32_wire.hip) and the Framebuffer line pass (b32_lines.hip).
#pragma once
#include "b32_device.h"

namespace b32 {

struct Edge { int32_t x0, y0, x1, y1; float z0, z1; };
// depth predicate of a walk: none (draw_line, draw_line_alpha), `z < zbuffer` (draw_line_3d), `z <= zbuffer` (draw_line_3d_overlay,
// draw_line_3d_alpha)
enum DepthOp : int { DEPTH_NONE = 0, DEPTH_LESS = 1, DEPTH_LESS_EQUAL = 2 };
__device__ __forceinline__ bool depth_passes(DepthOp op, float z, float zb) { return op == DEPTH_LESS ? z < zb : z <= zb; }

// Bresenham of draw_line / draw_line_3d_impl (render.rs:716-750, 771-817) in closed form.  With adx = |x1-x0|, ady = |y1-y0|,
// after i x-steps and j y-steps the error term is err = adx*(1+j) - ady*(1+i); the x-step condition 2*err >= -ady and the
// y-step condition 2*err <= adx give, for an x-major line (adx >= ady): x steps every iteration and
//   j(k) = floor((2*ady*k + adx) / (2*adx))      (round half up),
// and symmetrically for a y-major line i(k) = floor((2*adx*k + ady) / (2*ady)).  The depth parameter `step` advances by
// exactly 1.0 per iteration (saturating at 2^24 in f32).  tests/test_oracle_kats.py checks this against the literal loop.
// The walk proper: every pixel of the line inside [cx0, cx1] x [cy0, cy1] (inclusive, already inside the frame and the band) that
// passes the depth test goes to plot(x, y).  The closed form lets the walk start at the first step inside the rectangle's major-axis
// range; the minor coordinate is tested per pixel.
// steps of the line whose major coordinate lies inside the rectangle: [k_lo, k_hi] (false: none)
// (I: long long for any line, int for the ones edge_narrow() admits -- same values)
template <typename I>
__device__ __forceinline__ bool line_k_range_t(const Edge& e, I cx0, I cx1, I cy0, I cy1, I& k_lo, I& k_hi) {
    const I dx = (I)e.x1 - (I)e.x0, dy = (I)e.y1 - (I)e.y0;
    const I adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const bool xmajor = adx >= ady;
    const I N = xmajor ? adx : ady, m0 = xmajor ? (I)e.x0 : (I)e.y0, lo = xmajor ? cx0 : cy0, hi = xmajor ? cx1 : cy1;
    const int sm = xmajor ? (e.x0 < e.x1 ? 1 : -1) : (e.y0 < e.y1 ? 1 : -1);
    k_lo = 0; k_hi = N;
    if (sm > 0) { if (lo - m0 > k_lo) k_lo = lo - m0; if (hi - m0 < k_hi) k_hi = hi - m0; }
    else        { if (m0 - hi > k_lo) k_lo = m0 - hi; if (m0 - lo < k_hi) k_hi = m0 - lo; }
    return k_lo <= k_hi;
}
__device__ __forceinline__ bool line_k_range(const Edge& e, long long cx0, long long cx1, long long cy0, long long cy1, long long& k_lo, long long& k_hi) {
    return line_k_range_t<long long>(e, cx0, cx1, cy0, cy1, k_lo, k_hi);
}
// For a line edge_narrow() admits: the steps whose PIXEL lies inside the rectangle, both coordinates.  The minor coordinate after k steps
// is n0 + sn * j(k), j(k) = floor((2 * dmin * k + dmaj) / (2 * dmaj)), which never decreases: j(k) >= J  <=>  k >= ceil(dmaj * (2J - 1) /
// (2 * dmin)), so the steps with j(k) in [Ja, Jb] are an interval again.  Everything stays below 2^30.
// tests/test_oracle_kats.py::test_wire_tile_clip_closed_form_equals_literal_loop restates these lines in Python integers and compares
// them with the literal loop of render.rs:771-817 on 30 000 random lines and rectangles; the GPU parity tests compare whole frames.
__device__ __forceinline__ bool line_k_range_exact(const Edge& e, int cx0, int cx1, int cy0, int cy1, int& k_lo, int& k_hi) {
    if (!line_k_range_t<int>(e, cx0, cx1, cy0, cy1, k_lo, k_hi)) return false;
    const int dx = e.x1 - e.x0, dy = e.y1 - e.y0, adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const bool xmajor = adx >= ady;
    const int dmaj = xmajor ? adx : ady, dmin = xmajor ? ady : adx;
    const int n0 = xmajor ? e.y0 : e.x0, nlo = xmajor ? cy0 : cx0, nhi = xmajor ? cy1 : cx1;
    const bool up = xmajor ? e.y0 < e.y1 : e.x0 < e.x1;                  // sn > 0
    int ja = up ? nlo - n0 : n0 - nhi, jb = up ? nhi - n0 : n0 - nlo;   // the minor steps that put the pixel inside: j in [ja, jb]
    if (jb < 0 || ja > dmin) return false;
    ja = max(ja, 0); jb = min(jb, dmin);
    if (dmin > 0) {                                                      // (dmin == 0: j stays 0, every step qualifies)
        const uint32_t d = 2u * (uint32_t)dmin;
        if (ja >= 1) k_lo = max(k_lo, (int)(((uint32_t)dmaj * (uint32_t)(2 * ja - 1) + d - 1u) / d));
        k_hi = min(k_hi, (int)(((uint32_t)dmaj * (uint32_t)(2 * jb + 1) + d - 1u) / d) - 1);
    }
    return k_lo <= k_hi;
}
// steps k_a ... k_b of the line (a sub-range of line_k_range's).  I = the integer type of the walk: every line with extents below 2^14
// and start coordinates below 2^20 -- anything a sane mesh produces -- fits 32 bits (2 * dmin * k + dmaj < 2^29); the rest (coordinates
// up to 2^31 after the saturating `as i32`) walks in 64 bits.  Same values either way.
template <typename I, typename Depth, typename Plot>
__device__ __forceinline__ void walk_line_range_t(const Edge& e, DepthOp depth_op, I cx0, I cx1, I cy0, I cy1, I k_a, I k_b, Depth depth_at, Plot plot) {
    const I dx = (I)e.x1 - (I)e.x0, dy = (I)e.y1 - (I)e.y0;
    const I adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const I sx = e.x0 < e.x1 ? 1 : -1, sy = e.y0 < e.y1 ? 1 : -1;
    const I N = adx > ady ? adx : ady;
    const float total_steps = (float)(N > 1 ? N : 1);                   // dx.max((-dy).max(1)) as f32
    const bool xmajor = adx >= ady;
    const I m0 = xmajor ? (I)e.x0 : (I)e.y0;
    const I sm = xmajor ? sx : sy;
    const I dmin = xmajor ? ady : adx, dmaj = xmajor ? adx : ady;       // dmaj > 0 unless N == 0
    I j = 0, r = 0;                                                      // minor steps so far, remainder of the division
    if (dmaj > 0) { const I num = 2 * dmin * k_a + dmaj; j = num / (2 * dmaj); r = num - j * (2 * dmaj); }
    const I n0 = xmajor ? (I)e.y0 : (I)e.x0;
    const I sn = xmajor ? sy : sx;
    for (I k = k_a; k <= k_b; ++k) {
        const I maj = m0 + sm * k, mnr = n0 + sn * j;
        const I x = xmajor ? maj : mnr, y = xmajor ? mnr : maj;
        if (x >= cx0 && x <= cx1 && y >= cy0 && y <= cy1) {
            bool passes = true;
            if (depth_op != DEPTH_NONE) {
                const float step = (float)(k < (I)16777216 ? k : (I)16777216);
                const float t = step / total_steps;
                const float z = e.z0 + t * (e.z1 - e.z0);
                passes = depth_passes(depth_op, z, depth_at((uint32_t)x, (uint32_t)y));
            }
            if (passes) plot((uint32_t)x, (uint32_t)y);
        }
        r += 2 * dmin;
        if (dmaj > 0 && r >= 2 * dmaj) { r -= 2 * dmaj; ++j; }
    }
}
template <typename Depth, typename Plot>
__device__ __forceinline__ void walk_line_range(const Edge& e, DepthOp depth_op, long long cx0, long long cx1, long long cy0, long long cy1,
                                                long long k_a, long long k_b, Depth depth_at, Plot plot) {
    const long long adx = llabs((long long)e.x1 - e.x0), ady = llabs((long long)e.y1 - e.y0);
    const bool narrow = adx < 16384 && ady < 16384 && e.x0 > -1048576 && e.x0 < 1048576 && e.y0 > -1048576 && e.y0 < 1048576;
    if (narrow) walk_line_range_t<int>(e, depth_op, (int)cx0, (int)cx1, (int)cy0, (int)cy1, (int)k_a, (int)k_b, depth_at, plot);
    else walk_line_range_t<long long>(e, depth_op, cx0, cx1, cy0, cy1, k_a, k_b, depth_at, plot);
}
template <typename Depth, typename Plot>
__device__ __forceinline__ void walk_line(const Edge& e, DepthOp depth_op, long long cx0, long long cx1, long long cy0, long long cy1, Depth depth_at, Plot plot) {
    long long k_lo, k_hi;
    if (line_k_range(e, cx0, cx1, cy0, cy1, k_lo, k_hi)) walk_line_range(e, depth_op, cx0, cx1, cy0, cy1, k_lo, k_hi, depth_at, plot);
}
__device__ __forceinline__ uint32_t abs_diff(int p, int q) { return p < q ? (uint32_t)q - (uint32_t)p : (uint32_t)p - (uint32_t)q; }   // |p - q| of two i32, exact (< 2^32)
// Does the reference's i32 Bresenham state overflow (render.rs:742, 803)?  Extents of 2^30 and more: always refused.  Below that, with
// dmaj >= dmin the extents, `2 * err` reaches 3 * dmaj - 2 * dmin - r_min, where r_min = g = gcd(dmaj, dmin) if dmaj / g is odd and 0 if
// it is even (err after k steps is 1.5 * dmaj - dmin - r / 2, r = (2 * dmin * k + dmaj) mod (2 * dmaj); the reference restatement
// states the same rule, tests/test_wire_sheets.py compares both with the literal loop in a short word): a shallow
// line overflows from an extent of 2^31 / 3 on.  One multiply-subtract-compare for every line a mesh produces; the gcd only beyond it.
__device__ __forceinline__ bool edge_overflows(const Edge& e) {
    const uint32_t ax = abs_diff(e.x1, e.x0), ay = abs_diff(e.y1, e.y0);
    const uint32_t dmaj = ax > ay ? ax : ay, dmin = ax > ay ? ay : ax;
    if (dmaj >= (1u << 30)) return true;
    const uint32_t top = 3u * dmaj - 2u * dmin;                          // (< 3 * 2^30: fits)
    if (top < (1u << 31)) return false;
    uint32_t a = dmaj, b = dmin;
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    const uint32_t r_min = ((dmaj / a) & 1u) ? a : 0u;
    return ax >= ay ? top - r_min >= (1u << 31) : top - r_min > (1u << 31);        // (y-major: 2 * err is -(top - r): i32 holds -2^31)
}
// lines the tile kernel walks in 32-bit integers with the three-instruction depth parameter (the bounds of walk_line_range's `narrow`)
__device__ __forceinline__ bool edge_narrow(const Edge& e) {
    return abs_diff(e.x1, e.x0) < (uint32_t)WIRE_NARROW && abs_diff(e.y1, e.y0) < (uint32_t)WIRE_NARROW
        && e.x0 > -1048576 && e.x0 < 1048576 && e.y0 > -1048576 && e.y0 < 1048576;
}
}  // namespace b32
