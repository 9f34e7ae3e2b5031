// b32_prims.hip -- the rest of the reference Framebuffer's drawing methods (draw_circle, draw_circle_alpha, draw_line_blended,
// draw_thick_line, draw_rect, draw_filled_rect; render.rs:631-971) in one ordered pass with the line family: b32_draw_prims.
//
// Reference: every call writes its pixels one after another through set_pixel (replace, Color::to_bytes), set_pixel_alpha (integer
// blend, alpha 255) or set_pixel_blended (the PS1 blend by mode, render.rs:313-334).  Nothing here writes the z-buffer, so the depth
// tests of the 3-D line kinds do not depend on the order of the calls; the colour writes do.
//
// GPU form: the line pass's (b32_lines.hip, same tiles, chunks, routes and caps).  One 256-lane workgroup per 64 x LINE_TH tile takes
// the tile's primitives in array order, 32 at a time, and folds bit i of a pixel's mask into the colour it holds in a register.  The
// bits come from two places:
//   * walked kinds (0..5, and a thick line of thickness <= 1, which is draw_line): eight lanes per primitive walk its Bresenham steps
//     inside the tile (b32_line_walk.h) and atomicOr the bit into the pixel's LDS mask, as in the line pass;
//   * area kinds (circles, a thick line of thickness > 1, rectangles): decided pixel-major inside the fold -- every lane tests its own
//     pixels against the chunk's area primitives (no atomics).  A primitive's exact box (clipped to the tile) and, for a thick line,
//     its four f32 corners are computed once per chunk into LDS.  draw_rect's four opaque draw_line edges of one colour are exactly
//     the border of the normalised rectangle (a horizontal or vertical Bresenham line covers every pixel between its ends), so a
//     rectangle is one bit too.
// Binning and the scan's tile test use a conservative box per kind (prim_bounds); the exact box decides only the pixels.
#include "b32_line_walk.h"
#include "b32_fill_common.h"

namespace b32 {

constexpr uint32_t PRIM_THREADS = 256, PRIM_PX = 64 * LINE_TH;
constexpr uint32_t PRIM_CHUNK = 32;                 // primitives per fold (bits of a pixel's mask)
constexpr uint32_t PRIM_SEG = 8;                    // steps per lane of a walked kind (as LINE_SEG)
constexpr uint32_t PRIM_BIG_TILES = 64;
constexpr uint32_t PRIM_SORT_CAP = LINE_TILE_CAP + LINE_LONG_CAP;
static_assert(PRIM_CHUNK * PRIM_SEG == PRIM_THREADS && PRIM_SEG * PRIM_SEG >= 64, "one lane per segment of a chunk's walked kinds");
static_assert(PRIM_SORT_CAP >= PRIM_CHUNK + PRIM_THREADS && (PRIM_SORT_CAP & (PRIM_SORT_CAP - 1)) == 0, "scan buffer / bitonic sort");
static_assert(sizeof(B32Prim) == 40 && sizeof(PrimBatch) <= 2048, "B32Prim layout / kernel argument size");

// the op word of a chunk entry: depth predicate (bits 0-1) | store op (bits 2-3) | alpha (bits 8-15)
constexpr uint32_t POP_ALPHA = 4u;                  // set_pixel_alpha, render.rs:646-667
constexpr uint32_t POP_PS1 = 8u;                    // set_pixel_blended, render.rs:313-334 (mode in the colour word's top byte)

__device__ __forceinline__ uint32_t* prim_long_counter(const PrimArgs& a, uint32_t parity) { return a.counters + (size_t)parity * FILL_PAD; }
__device__ __forceinline__ uint32_t* prim_counter(const PrimArgs& a, uint32_t tile) { return a.counters + (size_t)(2u + tile) * FILL_PAD; }

__device__ __forceinline__ bool prim_walked(const B32Prim& p) {
    return p.kind <= B32_PRIM_LINE_BLENDED || (p.kind == B32_PRIM_THICK_LINE && p.size <= 1);
}
// A box holding every pixel the primitive can write (inclusive, not clipped); false: it writes none.  64-bit: the corners of a thick
// line reach 2^31 + 2^30.  A thick line's pixel centres lie within `half` of the segment; its f32 corners are rounded from integers up to
// 2^31 and the half-width (relative error 2^-24 each), hence the margin of ((|coordinate| + thickness) >> 22) + 2.
__device__ __forceinline__ bool prim_bounds(const B32Prim& p, long long& x0, long long& x1, long long& y0, long long& y1) {
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

__global__ void k_prims_bin(PrimArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    long long x0, x1, y0, y1;
    if (!prim_bounds(a.prims[i], x0, x1, y0, y1)) return;
    x0 = max(x0, 0ll); x1 = min(x1, (long long)a.width - 1); y0 = max(y0, (long long)a.band_y0); y1 = min(y1, (long long)a.band_y1 - 1);
    if (x0 > x1 || y0 > y1) return;
    const uint32_t tx0 = (uint32_t)x0 >> 6, tx1 = (uint32_t)x1 >> 6;
    const uint32_t ty0 = ((uint32_t)y0 - a.band_y0) / LINE_TH, ty1 = ((uint32_t)y1 - a.band_y0) / LINE_TH;
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > PRIM_BIG_TILES) {
        const uint32_t pos = atomicAdd(prim_long_counter(a, a.parity), 1u);
        if (pos < LINE_LONG_CAP) a.long_list[pos] = i;
        return;
    }
    for (uint32_t ty = ty0; ty <= ty1; ++ty)
        for (uint32_t tx = tx0; tx <= tx1; ++tx) {
            const uint32_t tile = ty * a.tiles_x + tx;
            const uint32_t pos = atomicAdd(prim_counter(a, tile), 1u);
            if (pos < LINE_TILE_CAP) a.lists[(size_t)tile * LINE_TILE_CAP + pos] = i;
        }
}

// an area primitive of the chunk: its exact box clipped to the tile (empty: bx0 > bx1), and per kind
//   circle: v = centre x, centre y, r * r;  rect: v = min_x, min_y, max_x, max_y;  thick line: q = the four corners (x, y)
struct PrimArea { int bx0, bx1, by0, by1; int v[4]; float q[8]; uint32_t kind; };

template <bool SMALL>
__global__ __launch_bounds__(PRIM_THREADS) void k_prims_tile(PrimArgs a, PrimBatch batch) {
    __shared__ B32Prim sp[SMALL ? PRIM_SMALL : 1];      // a small batch, out of the kernel argument
    __shared__ uint32_t ids[PRIM_SORT_CAP];              // primitive ids in array order (scan: at most PRIM_CHUNK - 1 + PRIM_THREADS pending)
    __shared__ float zt[PRIM_PX];                        // Framebuffer::zbuffer of the tile (read only)
    __shared__ uint32_t mask[PRIM_PX];                   // bit i: walked primitive i of the chunk passes at this pixel
    __shared__ Edge ce[PRIM_CHUNK];                      // the chunk's walked kinds (the 3D_ALPHA kind with its depths biased)
    __shared__ PrimArea ca[PRIM_CHUNK];                  // ... and its area kinds
    __shared__ uint32_t cop[PRIM_CHUNK], ccol[PRIM_CHUNK];
    __shared__ uint32_t wcnt[PRIM_THREADS / 64];
    __shared__ uint32_t careas;                          // bit i: entry i of the chunk is an area kind
    const uint32_t tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t txi = tile % a.tiles_x, tyi = tile / a.tiles_x, x_lo = txi * 64u, y_top = a.band_y0 + tyi * LINE_TH;
    // the tile's rectangle inside the frame and the band (non-empty: a tile of the grid)
    const int cx0 = (int)x_lo, cx1 = (int)min(x_lo + 63u, a.width - 1u), cy0 = (int)y_top, cy1 = (int)min(y_top + LINE_TH - 1u, a.band_y1 - 1u);

    if (SMALL) {
        if (tid < a.n) sp[tid] = batch.p[tid];
        __syncthreads();
    }
    auto prim_at = [&](uint32_t i) -> B32Prim { return SMALL ? sp[i] : a.prims[i]; };
    auto touches = [&](const B32Prim& p) {
        long long x0, x1, y0, y1;
        return prim_bounds(p, x0, x1, y0, y1) && max(x0, (long long)cx0) <= min(x1, (long long)cx1) && max(y0, (long long)cy0) <= min(y1, (long long)cy1);
    };

    uint32_t cur[PRIM_PX / PRIM_THREADS];                // the colour of pixels tid + 256 r, from the first chunk on
    uint32_t touched = 0;                                // bit r: pixel tid + 256 r was written
    bool loaded = false;                                 // (uniform) colours and depths read
    auto process_chunk = [&](const uint32_t* cid, uint32_t m) {
        bool area = false;
        if (tid < m) {
            const B32Prim p = prim_at(cid[tid]);
            const uint32_t abyte = p.blend != B32_BLEND_ERASE ? 255u : 0u;                 // Color::to_bytes, types.rs:829-832
            const uint32_t rgb = (uint32_t)p.r | ((uint32_t)p.g << 8) | ((uint32_t)p.b << 16);
            if (prim_walked(p)) {
                const bool biased = p.kind == B32_LINE_3D_ALPHA;
                const float z0 = biased ? p.z0 * 0.995f : p.z0, z1 = biased ? p.z1 * 0.995f : p.z1;    // DEPTH_BIAS, render.rs:826-828
                ce[tid] = Edge{ p.x0, p.y0, p.x1, p.y1, z0, z1 };
                const uint32_t depth = p.kind == B32_LINE_3D ? DEPTH_LESS
                                     : (p.kind == B32_LINE_3D_OVERLAY || p.kind == B32_LINE_3D_ALPHA) ? DEPTH_LESS_EQUAL : DEPTH_NONE;
                const bool blend = p.kind == B32_LINE_2D_ALPHA || p.kind == B32_LINE_3D_ALPHA;
                const bool ps1 = p.kind == B32_PRIM_LINE_BLENDED && p.mode != B32_BLEND_OPAQUE;
                cop[tid] = depth | (blend ? POP_ALPHA : ps1 ? POP_PS1 : 0u) | ((uint32_t)p.alpha << 8);
                ccol[tid] = rgb | ((ps1 ? (uint32_t)p.mode : blend ? 255u : abyte) << 24);
            } else {
                area = true;
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
                A.bx0 = max(bx0, cx0); A.bx1 = min(bx1, cx1); A.by0 = max(by0, cy0); A.by1 = min(by1, cy1);
                ca[tid] = A;
                const bool blend = p.kind == B32_PRIM_CIRCLE_ALPHA;
                cop[tid] = (blend ? POP_ALPHA : 0u) | ((uint32_t)p.alpha << 8);
                ccol[tid] = rgb | ((blend ? 255u : abyte) << 24);
            }
        }
        if (wave == 0) {
            const uint32_t bal = (uint32_t)__ballot(area);                  // (the chunk's entries are lanes 0..31 of wave 0)
            if (lane == 0) careas = bal;
        }
        if (!loaded) {
            loaded = true;
#pragma unroll
            for (uint32_t r = 0; r < PRIM_PX / PRIM_THREADS; ++r) {
                const uint32_t p = tid + r * PRIM_THREADS, x = x_lo + (p & 63u), y = y_top + (p >> 6);
                const bool in = (int)x <= cx1 && (int)y <= cy1;
                cur[r] = in ? a.fb[(size_t)y * a.width + x] : 0u;
                zt[p] = (in && a.zbuf) ? a.zbuf[(size_t)y * a.width + x] : 3.40282347e+38f;
                mask[p] = 0u;
            }
        }
        __syncthreads();
        const uint32_t areas = careas;
        const uint32_t i = tid / PRIM_SEG, q = tid % PRIM_SEG;
        if (i < m && !(areas & (1u << i))) {
            const Edge e = ce[i];
            const DepthOp op = (DepthOp)(cop[i] & 3u);
            const uint32_t bit = 1u << i;
            auto depth_at = [&](uint32_t x, uint32_t y) { return zt[(y - y_top) * 64u + (x - x_lo)]; };
            auto plot = [&](uint32_t x, uint32_t y) { atomicOr(&mask[(y - y_top) * 64u + (x - x_lo)], bit); };
            if (edge_narrow(e)) {
                int k_lo, k_hi;
                if (line_k_range_exact(e, cx0, cx1, cy0, cy1, k_lo, k_hi)) {
                    const int ka = k_lo + (int)(q * PRIM_SEG), kb = min(ka + (int)PRIM_SEG - 1, k_hi);
                    if (ka <= kb) walk_line_range_t<int>(e, op, cx0, cx1, cy0, cy1, ka, kb, depth_at, plot);
                }
            } else {
                long long k_lo, k_hi;                                   // (major axis only: at most 64 steps, the minor one tested per pixel)
                if (line_k_range(e, cx0, cx1, cy0, cy1, k_lo, k_hi)) {
                    const long long ka = k_lo + (long long)(q * PRIM_SEG), kb = min(ka + (long long)PRIM_SEG - 1, k_hi);
                    if (ka <= kb) walk_line_range_t<long long>(e, op, cx0, cx1, cy0, cy1, ka, kb, depth_at, plot);
                }
            }
        }
        __syncthreads();
        const int x = (int)(x_lo + (tid & 63u));                        // this lane's pixels: one column, rows (tid >> 6) + 4 r of the tile
        uint32_t abits[PRIM_PX / PRIM_THREADS] = {};
        for (uint32_t am = areas; am; am &= am - 1u) {                  // the area kinds, pixel-major
            const uint32_t k = (uint32_t)__builtin_ctz(am);
            const PrimArea& A = ca[k];
            if (x < A.bx0 || x > A.bx1) continue;
#pragma unroll
            for (uint32_t r = 0; r < PRIM_PX / PRIM_THREADS; ++r) {
                const int y = (int)(y_top + (tid >> 6) + 4u * r);
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
#pragma unroll
        for (uint32_t r = 0; r < PRIM_PX / PRIM_THREADS; ++r) {
            const uint32_t p = tid + r * PRIM_THREADS;
            const uint32_t walked = mask[p];
            uint32_t bits = walked | abits[r];
            if (!bits) continue;
            if (walked) mask[p] = 0u;
            touched |= 1u << r;
            uint32_t c = cur[r];
            while (bits) {
                const uint32_t k = (uint32_t)__builtin_ctz(bits);
                bits &= bits - 1u;
                const uint32_t o = cop[k], col = ccol[k];
                if (o & POP_ALPHA) {                                    // set_pixel_alpha, render.rs:646-667
                    const uint32_t al = (o >> 8) & 255u, inv = 255u - al;
                    const uint32_t rr = ((col & 255u) * al + (c & 255u) * inv) / 255u;
                    const uint32_t gg = (((col >> 8) & 255u) * al + ((c >> 8) & 255u) * inv) / 255u;
                    const uint32_t bb = (((col >> 16) & 255u) * al + ((c >> 16) & 255u) * inv) / 255u;
                    c = rr | (gg << 8) | (bb << 16) | 0xFF000000u;
                } else if (o & POP_PS1) {                               // set_pixel_blended: Color::blend(back opaque, mode), render.rs:313-334
                    c = store8(c, col, 255u);
                } else {
                    c = col;                                            // set_pixel, render.rs:301-310
                }
            }
            cur[r] = c;
        }
        __syncthreads();                                                // (the next chunk overwrites ce / ca / cop / ccol / careas)
    };
    // appends the primitives base + tid that `take` to ids[at...] in array order; returns how many the workgroup appended
    auto append_ordered = [&](bool take, uint32_t id, uint32_t at) -> uint32_t {
        const unsigned long long bal = __ballot(take);
        const uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = at, total = 0;
        for (uint32_t w = 0; w < PRIM_THREADS / 64; ++w) { if (w < wave) off += wcnt[w]; total += wcnt[w]; }
        if (take) ids[off + before] = id;
        __syncthreads();
        return total;
    };

    bool scan = SMALL || !a.counters;
    if (!scan) {
        const uint32_t cnt = *prim_counter(a, tile), long_n = *prim_long_counter(a, a.parity);
        __syncthreads();                                                // (everyone has read the counters)
        if (tid == 0) *prim_counter(a, tile) = 0u;                      // zero again for the next binned batch
        if (tid == 0 && tile == 0) *prim_long_counter(a, a.parity ^ 1u) = 0u;   // (the previous binned batch's, done: the next batch's now)
        scan = cnt > LINE_TILE_CAP || long_n > LINE_LONG_CAP;
        if (!scan) {
            for (uint32_t k = tid; k < cnt; k += PRIM_THREADS) ids[k] = a.lists[(size_t)tile * LINE_TILE_CAP + k];
            uint32_t m = cnt;
            for (uint32_t base = 0; base < long_n; base += PRIM_THREADS) {
                const uint32_t k = base + tid;
                const uint32_t id = k < long_n ? a.long_list[k] : 0u;
                m += append_ordered(k < long_n && touches(a.prims[id]), id, m);
            }
            if (m == 0) return;
            uint32_t P = 2;
            while (P < m) P <<= 1;
            for (uint32_t k = m + tid; k < P; k += PRIM_THREADS) ids[k] = 0xFFFFFFFFu;
            __syncthreads();
            for (uint32_t k = 2; k <= P; k <<= 1)                           // bitonic sort, ascending
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    for (uint32_t t = tid; t < P; t += PRIM_THREADS) {
                        const uint32_t u = t ^ j;
                        if (u > t) {
                            const uint32_t x = ids[t], y = ids[u];
                            if ((x > y) == ((t & k) == 0)) { ids[t] = y; ids[u] = x; }
                        }
                    }
                    __syncthreads();
                }
            for (uint32_t done = 0; done < m; done += PRIM_CHUNK) process_chunk(ids + done, min(PRIM_CHUNK, m - done));
        }
    }
    if (scan) {
        uint32_t pend = 0;                                              // ids[0, pend): taken, not yet drawn (fewer than a chunk)
        for (uint32_t base = 0; base < a.n; base += PRIM_THREADS) {
            const uint32_t k = base + tid;
            const uint32_t total = pend + append_ordered(k < a.n && touches(prim_at(k)), k, pend);
            uint32_t done = 0;
            for (; total - done >= PRIM_CHUNK; done += PRIM_CHUNK) process_chunk(ids + done, PRIM_CHUNK);
            pend = total - done;
            if (done && pend) {                                         // the rest to the front
                const uint32_t v = tid < pend ? ids[done + tid] : 0u;
                __syncthreads();
                if (tid < pend) ids[tid] = v;
                __syncthreads();
            }
        }
        if (pend) process_chunk(ids, pend);
    }
    if (!loaded) return;
#pragma unroll
    for (uint32_t r = 0; r < PRIM_PX / PRIM_THREADS; ++r) {
        if (!(touched & (1u << r))) continue;
        const uint32_t p = tid + r * PRIM_THREADS;
        a.fb[(size_t)(y_top + (p >> 6)) * a.width + x_lo + (p & 63u)] = cur[r];
    }
}

void launch_prims(hipStream_t s, const PrimArgs& a, const B32Prim* small) {
    const uint32_t ntiles = a.tiles_x * a.tiles_y;
    if (!a.n || !ntiles) return;
    PrimBatch batch;
    if (small) {
        for (uint32_t i = 0; i < a.n && i < PRIM_SMALL; ++i) batch.p[i] = small[i];
        hipLaunchKernelGGL(k_prims_tile<true>, dim3(ntiles), dim3(PRIM_THREADS), 0, s, a, batch);
        return;
    }
    if (a.counters) hipLaunchKernelGGL(k_prims_bin, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_prims_tile<false>, dim3(ntiles), dim3(PRIM_THREADS), 0, s, a, batch);
}

}  // namespace b32
