// b32_lines.hip -- the reference Framebuffer's line family (draw_line, draw_line_alpha, draw_line_3d, draw_line_3d_overlay,
// draw_line_3d_alpha; render.rs:684-872) as one ordered pass: b32_draw_lines.
//
// Reference: each call walks its Bresenham line and, per on-screen pixel that passes the depth test (none for the 2-D kinds; `<`,
// `<=`, or `<=` against z * 0.995 for the 3-D ones), either replaces the pixel (set_pixel) or blends into it (set_pixel_alpha).  Lines
// never write the z-buffer, so every depth test is independent of the order of the calls; the colour writes are not -- a later
// opaque line hides an earlier one, and a blend reads what the lines before it left.
//
// GPU form: one 256-lane workgroup per 64 x LINE_TH tile of the band.  The tile's lines are taken in array order, 32 at a time: eight
// lanes per line walk its steps inside the tile (the closed form of b32_line_walk.h starts a walk at any step) and set bit i of the
// pixel's LDS mask when the pixel passes line i's depth test; then every pixel folds its set bits lowest first into its colour, which
// stays in a register from the first chunk to the last.  The tile is written once.  Which lines a tile takes:
//   * scan: the tile tests every line of the batch against its box, in order (ballot compaction keeps the order).  Batches of at most
//     LINE_SMALL lines (the player's cylinder: 36) travel in the kernel argument and always take it -- one launch, no copy;
//   * tile route (B32_ROUTE_LINE_TILES, larger batches): k_lines_bin appends every line to the list of each tile its clipped box
//     touches (a line whose box covers more than LINE_BIG_TILES tiles goes to one shared list instead), and k_lines_tile puts the
//     tile's list plus the shared lines that touch the tile back in array order with a bitonic sort in LDS (ids are unique).  A tile
//     whose list overflowed, or every tile when the shared list did, scans the whole batch as above: exact, only slower.
#include "b32_line_walk.h"

namespace b32 {

constexpr uint32_t LINE_THREADS = 256, LINE_PX = 64 * LINE_TH;
constexpr uint32_t LINE_CHUNK = 32;                 // lines per fold (bits of a pixel's mask)
constexpr uint32_t LINE_SEG = 8;                    // steps per lane: 8 lanes cover the at most 64 steps of a line inside a tile
constexpr uint32_t LINE_BIG_TILES = 64;
constexpr uint32_t LINE_SORT_CAP = LINE_TILE_CAP + LINE_LONG_CAP;
static_assert(LINE_CHUNK * LINE_SEG == LINE_THREADS && LINE_SEG * LINE_SEG >= 64, "one lane per segment of a chunk's lines");
static_assert(LINE_SORT_CAP >= LINE_CHUNK + LINE_THREADS && (LINE_SORT_CAP & (LINE_SORT_CAP - 1)) == 0, "scan buffer / bitonic sort");

// the op word of a chunk entry: depth predicate | blend flag | alpha
constexpr uint32_t LOP_BLEND = 4u;

// (the two long-list counters first, then one per tile: where they lie does not depend on the tile grid of the batch)
__device__ __forceinline__ uint32_t* line_long_counter(const LineArgs& a, uint32_t parity) { return a.counters + (size_t)parity * FILL_PAD; }
__device__ __forceinline__ uint32_t* line_counter(const LineArgs& a, uint32_t tile) { return a.counters + (size_t)(2u + tile) * FILL_PAD; }

struct LineBox { int cx0, cx1, cy0, cy1; };
// the line's box clipped to the frame and the band (every pixel the walk can touch lies inside it); false: empty
__device__ __forceinline__ bool line_box(const LineArgs& a, const B32Line& l, LineBox& b) {
    b.cx0 = max(min(l.x0, l.x1), 0); b.cx1 = min(max(l.x0, l.x1), (int)a.width - 1);
    b.cy0 = max(min(l.y0, l.y1), (int)a.band_y0); b.cy1 = min(max(l.y0, l.y1), (int)a.band_y1 - 1);
    return b.cx0 <= b.cx1 && b.cy0 <= b.cy1;
}

__global__ void k_lines_bin(LineArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const B32Line l = a.lines[i];
    LineBox b;
    if (!line_box(a, l, b)) return;
    const uint32_t tx0 = (uint32_t)b.cx0 >> 6, tx1 = (uint32_t)b.cx1 >> 6;
    const uint32_t ty0 = ((uint32_t)b.cy0 - a.band_y0) / LINE_TH, ty1 = ((uint32_t)b.cy1 - a.band_y0) / LINE_TH;
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > LINE_BIG_TILES) {
        const uint32_t pos = atomicAdd(line_long_counter(a, a.parity), 1u);
        if (pos < LINE_LONG_CAP) a.long_list[pos] = i;
        return;
    }
    for (uint32_t ty = ty0; ty <= ty1; ++ty)
        for (uint32_t tx = tx0; tx <= tx1; ++tx) {
            const uint32_t tile = ty * a.tiles_x + tx;
            const uint32_t pos = atomicAdd(line_counter(a, tile), 1u);
            if (pos < LINE_TILE_CAP) a.lists[(size_t)tile * LINE_TILE_CAP + pos] = i;
        }
}

template <bool SMALL>
__global__ __launch_bounds__(LINE_THREADS) void k_lines_tile(LineArgs a, LineBatch batch) {
    __shared__ B32Line sl[SMALL ? LINE_SMALL : 1];       // a small batch, out of the kernel argument
    __shared__ uint32_t ids[LINE_SORT_CAP];              // line ids in array order (scan: at most LINE_CHUNK - 1 + LINE_THREADS pending)
    __shared__ float zt[LINE_PX];                        // Framebuffer::zbuffer of the tile (read only)
    __shared__ uint32_t mask[LINE_PX];                   // bit i: line i of the chunk passes at this pixel
    __shared__ Edge ce[LINE_CHUNK];                      // the chunk's lines (the 3D_ALPHA kind with its depths biased)
    __shared__ uint32_t cop[LINE_CHUNK], ccol[LINE_CHUNK];
    __shared__ uint32_t wcnt[LINE_THREADS / 64];
    const uint32_t tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t txi = tile % a.tiles_x, tyi = tile / a.tiles_x, x_lo = txi * 64u, y_top = a.band_y0 + tyi * LINE_TH;
    // the tile's rectangle inside the frame and the band (non-empty: a tile of the grid)
    const int cx0 = (int)x_lo, cx1 = (int)min(x_lo + 63u, a.width - 1u), cy0 = (int)y_top, cy1 = (int)min(y_top + LINE_TH - 1u, a.band_y1 - 1u);

    if (SMALL) {
        if (tid < a.n) sl[tid] = batch.l[tid];
        __syncthreads();
    }
    auto line_at = [&](uint32_t i) -> B32Line { return SMALL ? sl[i] : a.lines[i]; };
    auto touches = [&](const B32Line& l) {
        return max(min(l.x0, l.x1), cx0) <= min(max(l.x0, l.x1), cx1) && max(min(l.y0, l.y1), cy0) <= min(max(l.y0, l.y1), cy1);
    };

    uint32_t cur[LINE_PX / LINE_THREADS];                // the colour of pixels tid + 256 r, from the first chunk on
    uint32_t touched = 0;                                // bit r: pixel tid + 256 r was written
    bool loaded = false;                                 // (uniform) colours and depths read
    auto process_chunk = [&](const uint32_t* cid, uint32_t m) {
        if (tid < m) {
            const B32Line l = line_at(cid[tid]);
            const bool biased = l.kind == B32_LINE_3D_ALPHA;
            const float z0 = biased ? l.z0 * 0.995f : l.z0, z1 = biased ? l.z1 * 0.995f : l.z1;    // DEPTH_BIAS, render.rs:826-828
            ce[tid] = Edge{ l.x0, l.y0, l.x1, l.y1, z0, z1 };
            const uint32_t depth = l.kind == B32_LINE_3D ? DEPTH_LESS : l.kind >= B32_LINE_3D_OVERLAY ? DEPTH_LESS_EQUAL : DEPTH_NONE;
            const bool blend = l.kind == B32_LINE_2D_ALPHA || l.kind == B32_LINE_3D_ALPHA;
            cop[tid] = depth | (blend ? LOP_BLEND : 0u) | ((uint32_t)l.alpha << 8);
            const uint32_t alpha_byte = (blend || l.blend != B32_BLEND_ERASE) ? 255u : 0u;                 // Color::to_bytes, types.rs:829-832
            ccol[tid] = (uint32_t)l.r | ((uint32_t)l.g << 8) | ((uint32_t)l.b << 16) | (alpha_byte << 24);
        }
        if (!loaded) {
            loaded = true;
#pragma unroll
            for (uint32_t r = 0; r < LINE_PX / LINE_THREADS; ++r) {
                const uint32_t p = tid + r * LINE_THREADS, x = x_lo + (p & 63u), y = y_top + (p >> 6);
                const bool in = (int)x <= cx1 && (int)y <= cy1;
                cur[r] = in ? a.fb[(size_t)y * a.width + x] : 0u;
                zt[p] = (in && a.zbuf) ? a.zbuf[(size_t)y * a.width + x] : 3.40282347e+38f;
                mask[p] = 0u;
            }
        }
        __syncthreads();
        const uint32_t i = tid / LINE_SEG, q = tid % LINE_SEG;
        if (i < m) {
            const Edge e = ce[i];
            const DepthOp op = (DepthOp)(cop[i] & 3u);
            const uint32_t bit = 1u << i;
            auto depth_at = [&](uint32_t x, uint32_t y) { return zt[(y - y_top) * 64u + (x - x_lo)]; };
            auto plot = [&](uint32_t x, uint32_t y) { atomicOr(&mask[(y - y_top) * 64u + (x - x_lo)], bit); };
            if (edge_narrow(e)) {
                int k_lo, k_hi;
                if (line_k_range_exact(e, cx0, cx1, cy0, cy1, k_lo, k_hi)) {
                    const int ka = k_lo + (int)(q * LINE_SEG), kb = min(ka + (int)LINE_SEG - 1, k_hi);
                    if (ka <= kb) walk_line_range_t<int>(e, op, cx0, cx1, cy0, cy1, ka, kb, depth_at, plot);
                }
            } else {
                long long k_lo, k_hi;                                   // (major axis only: at most 64 steps, the minor one tested per pixel)
                if (line_k_range(e, cx0, cx1, cy0, cy1, k_lo, k_hi)) {
                    const long long ka = k_lo + (long long)(q * LINE_SEG), kb = min(ka + (long long)LINE_SEG - 1, k_hi);
                    if (ka <= kb) walk_line_range_t<long long>(e, op, cx0, cx1, cy0, cy1, ka, kb, depth_at, plot);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < LINE_PX / LINE_THREADS; ++r) {
            const uint32_t p = tid + r * LINE_THREADS;
            uint32_t bits = mask[p];
            if (!bits) continue;
            mask[p] = 0u;
            touched |= 1u << r;
            uint32_t c = cur[r];
            while (bits) {
                const uint32_t k = (uint32_t)__builtin_ctz(bits);
                bits &= bits - 1u;
                const uint32_t o = cop[k], col = ccol[k];
                if (o & LOP_BLEND) {                                    // set_pixel_alpha, render.rs:646-667
                    const uint32_t al = o >> 8, inv = 255u - al;
                    const uint32_t rr = ((col & 255u) * al + (c & 255u) * inv) / 255u;
                    const uint32_t gg = (((col >> 8) & 255u) * al + ((c >> 8) & 255u) * inv) / 255u;
                    const uint32_t bb = (((col >> 16) & 255u) * al + ((c >> 16) & 255u) * inv) / 255u;
                    c = rr | (gg << 8) | (bb << 16) | 0xFF000000u;
                } else {
                    c = col;                                            // set_pixel, render.rs:301-310
                }
            }
            cur[r] = c;
        }
        __syncthreads();                                                // (the next chunk overwrites ce / cop / ccol)
    };
    // appends the lines base + tid that `take` to ids[at...] in array order; returns how many the workgroup appended
    auto append_ordered = [&](bool take, uint32_t id, uint32_t at) -> uint32_t {
        const unsigned long long bal = __ballot(take);
        const uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = at, total = 0;
        for (uint32_t w = 0; w < LINE_THREADS / 64; ++w) { if (w < wave) off += wcnt[w]; total += wcnt[w]; }
        if (take) ids[off + before] = id;
        __syncthreads();
        return total;
    };

    bool scan = SMALL || !a.counters;
    if (!scan) {
        const uint32_t cnt = *line_counter(a, tile), long_n = *line_long_counter(a, a.parity);
        __syncthreads();                                                // (everyone has read the counters)
        if (tid == 0) *line_counter(a, tile) = 0u;                      // zero again for the next binned batch
        if (tid == 0 && tile == 0) *line_long_counter(a, a.parity ^ 1u) = 0u;   // (the previous binned batch's, done: the next batch's now)
        scan = cnt > LINE_TILE_CAP || long_n > LINE_LONG_CAP;
        if (!scan) {
            for (uint32_t k = tid; k < cnt; k += LINE_THREADS) ids[k] = a.lists[(size_t)tile * LINE_TILE_CAP + k];
            uint32_t m = cnt;
            for (uint32_t base = 0; base < long_n; base += LINE_THREADS) {
                const uint32_t k = base + tid;
                const uint32_t id = k < long_n ? a.long_list[k] : 0u;
                m += append_ordered(k < long_n && touches(a.lines[id]), id, m);
            }
            if (m == 0) return;
            uint32_t P = 2;
            while (P < m) P <<= 1;
            for (uint32_t k = m + tid; k < P; k += LINE_THREADS) ids[k] = 0xFFFFFFFFu;
            __syncthreads();
            for (uint32_t k = 2; k <= P; k <<= 1)                           // bitonic sort, ascending
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    for (uint32_t t = tid; t < P; t += LINE_THREADS) {
                        const uint32_t u = t ^ j;
                        if (u > t) {
                            const uint32_t x = ids[t], y = ids[u];
                            if ((x > y) == ((t & k) == 0)) { ids[t] = y; ids[u] = x; }
                        }
                    }
                    __syncthreads();
                }
            for (uint32_t done = 0; done < m; done += LINE_CHUNK) process_chunk(ids + done, min(LINE_CHUNK, m - done));
        }
    }
    if (scan) {
        uint32_t pend = 0;                                              // ids[0, pend): taken, not yet drawn (fewer than a chunk)
        for (uint32_t base = 0; base < a.n; base += LINE_THREADS) {
            const uint32_t k = base + tid;
            const uint32_t total = pend + append_ordered(k < a.n && touches(line_at(k)), k, pend);
            uint32_t done = 0;
            for (; total - done >= LINE_CHUNK; done += LINE_CHUNK) process_chunk(ids + done, LINE_CHUNK);
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
    for (uint32_t r = 0; r < LINE_PX / LINE_THREADS; ++r) {
        if (!(touched & (1u << r))) continue;
        const uint32_t p = tid + r * LINE_THREADS;
        a.fb[(size_t)(y_top + (p >> 6)) * a.width + x_lo + (p & 63u)] = cur[r];
    }
}

void launch_lines(hipStream_t s, const LineArgs& a, const B32Line* small) {
    const uint32_t ntiles = a.tiles_x * a.tiles_y;
    if (!a.n || !ntiles) return;
    LineBatch batch;
    if (small) {
        for (uint32_t i = 0; i < a.n && i < LINE_SMALL; ++i) batch.l[i] = small[i];
        hipLaunchKernelGGL(k_lines_tile<true>, dim3(ntiles), dim3(LINE_THREADS), 0, s, a, batch);
        return;
    }
    if (a.counters) hipLaunchKernelGGL(k_lines_bin, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_lines_tile<false>, dim3(ntiles), dim3(LINE_THREADS), 0, s, a, batch);
}

}  // namespace b32
