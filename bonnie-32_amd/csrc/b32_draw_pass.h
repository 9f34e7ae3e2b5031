// b32_draw_pass.h -- the ordered tile pass behind b32_draw_lines (b32_lines.hip) and b32_draw_prims (b32_prims.hip).
//
// Reference: every Framebuffer drawing call writes its pixels one after another, each either replacing the pixel or blending into it.
// None of them writes the z-buffer, so every depth test is independent of the order of the calls; the colour writes are not -- a later
// opaque record hides an earlier one, and a blend reads what the records before it left.
//
// GPU form: one 256-lane workgroup per 64 x LINE_TH tile of the band.  The tile's records are taken in array order, 32 at a time (a
// chunk): eight lanes per walked record walk its Bresenham steps inside the tile (the closed form of b32_line_walk.h starts a walk at
// any step) and set bit i of the pixel's LDS mask when the pixel passes record i's depth test; a pass may add bits of its own per pixel
// (the area kinds of the primitive pass); then every pixel folds its set bits lowest first into its colour, which stays in a register
// from the first chunk to the last.  The tile is written once.  Which records a tile takes:
//   * scan: the tile tests every record of the batch against its box, in order (ballot compaction keeps the order).  Batches of at most
//     Pass::SMALL records travel in the kernel argument and always take it -- one launch, no copy;
//   * tile route (larger batches): draw_bin appends every record to the list of each tile its clipped box touches (a record whose box
//     covers more than DRAW_BIG_TILES tiles goes to one shared list instead), and draw_tile puts the tile's list plus the shared records
//     that touch the tile back in array order with a bitonic sort in LDS (ids are unique).  A tile whose list overflowed, or every tile
//     when the shared list did, scans the whole batch as above: exact, only slower.
//
// A pass is a struct of static __device__ functions:
//   Rec, SMALL      the record type and its small-batch size
//   Box             the integer type of a record's box (int where min / max of the coordinates is the box, long long where it is padded)
//   Areas           LDS for per-pixel bits beside the walked ones: an empty struct, or one with `uint32_t careas` (bit i: entry i of
//                   the chunk is not walked) plus whatever entry() and area_bits() share
//   bounds(r, x0, x1, y0, y1)          a box holding every pixel the record can write (inclusive, not clipped); false: it writes none
//   entry(r, i, tile, sh)              sets up chunk entry i (sh.ce / cop / ccol, or the pass's own); true: not walked
//   area_bits(sh, areas, x, y0, bits)  (only with Areas) ORs bit k into bits[r] where entry k of `areas` covers pixel (x, y0 + 4 r)
//   store(op, col, c)                  the pixel after entry (op, col) is written over colour c
#pragma once
#include <type_traits>
#include "b32_line_walk.h"

namespace b32 {

constexpr uint32_t DRAW_THREADS = 256, DRAW_PX = 64 * LINE_TH, DRAW_ROWS = DRAW_PX / DRAW_THREADS;   // a lane's pixels: tid + 256 r
constexpr uint32_t DRAW_CHUNK = 32;                 // records per fold (bits of a pixel's mask)
constexpr uint32_t DRAW_SEG = 8;                    // steps per lane: 8 lanes cover the at most 64 steps of a walk inside a tile
constexpr uint32_t DRAW_BIG_TILES = 64;
constexpr uint32_t DRAW_SORT_CAP = LINE_TILE_CAP + LINE_LONG_CAP;
static_assert(DRAW_CHUNK * DRAW_SEG == DRAW_THREADS && DRAW_SEG * DRAW_SEG >= 64, "one lane per segment of a chunk's walked records");
static_assert(DRAW_SORT_CAP >= DRAW_CHUNK + DRAW_THREADS && (DRAW_SORT_CAP & (DRAW_SORT_CAP - 1)) == 0, "scan buffer / bitonic sort");

// the op word of a chunk entry: depth predicate (bits 0-1) | store op (bits 2-3) | alpha (bits 8-15)
constexpr uint32_t DOP_ALPHA = 4u;                  // set_pixel_alpha, render.rs:646-667
constexpr uint32_t DOP_PS1 = 8u;                    // set_pixel_blended, render.rs:313-334 (mode in the colour word's top byte)

// (the two long-list counters first, then one per tile: where they lie does not depend on the tile grid of the batch)
template <class A> __device__ __forceinline__ uint32_t* draw_long_counter(const A& a, uint32_t parity) { return a.counters + (size_t)parity * FILL_PAD; }
template <class A> __device__ __forceinline__ uint32_t* draw_counter(const A& a, uint32_t tile) { return a.counters + (size_t)(2u + tile) * FILL_PAD; }

// set_pixel_alpha, render.rs:646-667
__device__ __forceinline__ uint32_t draw_blend_alpha(uint32_t c, uint32_t col, uint32_t al) {
    const uint32_t inv = 255u - al;
    const uint32_t rr = ((col & 255u) * al + (c & 255u) * inv) / 255u;
    const uint32_t gg = (((col >> 8) & 255u) * al + ((c >> 8) & 255u) * inv) / 255u;
    const uint32_t bb = (((col >> 16) & 255u) * al + ((c >> 16) & 255u) * inv) / 255u;
    return rr | (gg << 8) | (bb << 16) | 0xFF000000u;
}

// a walked entry of the line family (kinds 0..4, B32_LINE_*; any other kind: no depth test, replace): edge, op word, colour word
template <class Rec>
__device__ __forceinline__ void draw_line_entry(const Rec& l, Edge& e, uint32_t& op, uint32_t& col) {
    const bool biased = l.kind == B32_LINE_3D_ALPHA;
    const float z0 = biased ? l.z0 * 0.995f : l.z0, z1 = biased ? l.z1 * 0.995f : l.z1;    // DEPTH_BIAS, render.rs:826-828
    e = Edge{ l.x0, l.y0, l.x1, l.y1, z0, z1 };
    const uint32_t depth = l.kind == B32_LINE_3D ? DEPTH_LESS
                         : (l.kind == B32_LINE_3D_OVERLAY || l.kind == B32_LINE_3D_ALPHA) ? DEPTH_LESS_EQUAL : DEPTH_NONE;
    const bool blend = l.kind == B32_LINE_2D_ALPHA || l.kind == B32_LINE_3D_ALPHA;
    op = depth | (blend ? DOP_ALPHA : 0u) | ((uint32_t)l.alpha << 8);
    const uint32_t alpha_byte = (blend || l.blend != B32_BLEND_ERASE) ? 255u : 0u;         // Color::to_bytes, types.rs:829-832
    col = (uint32_t)l.r | ((uint32_t)l.g << 8) | ((uint32_t)l.b << 16) | (alpha_byte << 24);
}

// the tile route's binning: one lane per record
template <class Pass>
__device__ __forceinline__ void draw_bin(const DrawArgs<typename Pass::Rec>& a) {
    using Box = typename Pass::Box;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    Box x0, x1, y0, y1;
    if (!Pass::bounds(a.recs[i], x0, x1, y0, y1)) return;
    // clipped to the frame and the band (every pixel the record can touch lies inside it)
    x0 = max(x0, (Box)0); x1 = min(x1, (Box)a.width - 1); y0 = max(y0, (Box)a.band_y0); y1 = min(y1, (Box)a.band_y1 - 1);
    if (x0 > x1 || y0 > y1) return;
    const uint32_t tx0 = (uint32_t)x0 >> 6, tx1 = (uint32_t)x1 >> 6;
    const uint32_t ty0 = ((uint32_t)y0 - a.band_y0) / LINE_TH, ty1 = ((uint32_t)y1 - a.band_y0) / LINE_TH;
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > DRAW_BIG_TILES) {
        const uint32_t pos = atomicAdd(draw_long_counter(a, a.parity), 1u);
        if (pos < LINE_LONG_CAP) a.long_list[pos] = i;
        return;
    }
    for (uint32_t ty = ty0; ty <= ty1; ++ty)
        for (uint32_t tx = tx0; tx <= tx1; ++tx) {
            const uint32_t tile = ty * a.tiles_x + tx;
            const uint32_t pos = atomicAdd(draw_counter(a, tile), 1u);
            if (pos < LINE_TILE_CAP) a.lists[(size_t)tile * LINE_TILE_CAP + pos] = i;
        }
}

// the tile's rectangle inside the frame and the band (non-empty: a tile of the grid)
struct DrawTile { int cx0, cx1, cy0, cy1; };

// LDS of one tile workgroup
template <class Pass, bool SMALL>
struct DrawShared : Pass::Areas {
    typename Pass::Rec small[SMALL ? Pass::SMALL : 1];   // a small batch, out of the kernel argument
    uint32_t ids[DRAW_SORT_CAP];                         // record ids in array order (scan: at most DRAW_CHUNK - 1 + DRAW_THREADS pending)
    float zt[DRAW_PX];                                   // Framebuffer::zbuffer of the tile (read only)
    uint32_t mask[DRAW_PX];                              // bit i: walked entry i of the chunk passes at this pixel
    Edge ce[DRAW_CHUNK];                                 // the chunk's walked entries (the 3D_ALPHA kind with its depths biased)
    uint32_t cop[DRAW_CHUNK], ccol[DRAW_CHUNK];
    uint32_t wcnt[DRAW_THREADS / 64];
};

template <class Pass, bool SMALL>
__device__ __forceinline__ void draw_tile(const DrawArgs<typename Pass::Rec>& a, const DrawBatch<typename Pass::Rec, Pass::SMALL>& batch) {
    using Rec = typename Pass::Rec;
    using Box = typename Pass::Box;
    constexpr bool AREAS = !std::is_empty<typename Pass::Areas>::value;
    __shared__ DrawShared<Pass, SMALL> sh;
    const uint32_t tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t txi = tile % a.tiles_x, tyi = tile / a.tiles_x, x_lo = txi * 64u, y_top = a.band_y0 + tyi * LINE_TH;
    const int cx0 = (int)x_lo, cx1 = (int)min(x_lo + 63u, a.width - 1u), cy0 = (int)y_top, cy1 = (int)min(y_top + LINE_TH - 1u, a.band_y1 - 1u);

    if (SMALL) {
        if (tid < a.n) sh.small[tid] = batch.r[tid];
        __syncthreads();
    }
    auto rec_at = [&](uint32_t i) -> Rec { return SMALL ? sh.small[i] : a.recs[i]; };
    auto touches = [&](const Rec& r) {
        Box x0, x1, y0, y1;
        return Pass::bounds(r, x0, x1, y0, y1) && max(x0, (Box)cx0) <= min(x1, (Box)cx1) && max(y0, (Box)cy0) <= min(y1, (Box)cy1);
    };

    uint32_t cur[DRAW_ROWS];                             // the colour of pixels tid + 256 r, from the first chunk on
    uint32_t touched = 0;                                // bit r: pixel tid + 256 r was written
    bool loaded = false;                                 // (uniform) colours and depths read
    auto process_chunk = [&](const uint32_t* cid, uint32_t m) {
        bool area = false;
        if (tid < m) area = Pass::entry(rec_at(cid[tid]), tid, DrawTile{ cx0, cx1, cy0, cy1 }, sh);
        if constexpr (AREAS) {
            if (wave == 0) {
                const uint32_t bal = (uint32_t)__ballot(area);                  // (the chunk's entries are lanes 0..31 of wave 0)
                if (lane == 0) sh.careas = bal;
            }
        }
        if (!loaded) {
            loaded = true;
#pragma unroll
            for (uint32_t r = 0; r < DRAW_ROWS; ++r) {
                const uint32_t p = tid + r * DRAW_THREADS, x = x_lo + (p & 63u), y = y_top + (p >> 6);
                const bool in = (int)x <= cx1 && (int)y <= cy1;
                cur[r] = in ? a.fb[(size_t)y * a.width + x] : 0u;
                sh.zt[p] = (in && a.zbuf) ? a.zbuf[(size_t)y * a.width + x] : 3.40282347e+38f;
                sh.mask[p] = 0u;
            }
        }
        __syncthreads();
        uint32_t areas = 0u;
        if constexpr (AREAS) areas = sh.careas;
        const uint32_t i = tid / DRAW_SEG, q = tid % DRAW_SEG;
        if (i < m && !(areas & (1u << i))) {
            const Edge e = sh.ce[i];
            const DepthOp op = (DepthOp)(sh.cop[i] & 3u);
            const uint32_t bit = 1u << i;
            auto depth_at = [&](uint32_t x, uint32_t y) { return sh.zt[(y - y_top) * 64u + (x - x_lo)]; };
            auto plot = [&](uint32_t x, uint32_t y) { atomicOr(&sh.mask[(y - y_top) * 64u + (x - x_lo)], bit); };
            if (edge_narrow(e)) {
                int k_lo, k_hi;
                if (line_k_range_exact(e, cx0, cx1, cy0, cy1, k_lo, k_hi)) {
                    const int ka = k_lo + (int)(q * DRAW_SEG), kb = min(ka + (int)DRAW_SEG - 1, k_hi);
                    if (ka <= kb) walk_line_range_t<int>(e, op, cx0, cx1, cy0, cy1, ka, kb, depth_at, plot);
                }
            } else {
                long long k_lo, k_hi;                                   // (major axis only: at most 64 steps, the minor one tested per pixel)
                if (line_k_range(e, cx0, cx1, cy0, cy1, k_lo, k_hi)) {
                    const long long ka = k_lo + (long long)(q * DRAW_SEG), kb = min(ka + (long long)DRAW_SEG - 1, k_hi);
                    if (ka <= kb) walk_line_range_t<long long>(e, op, cx0, cx1, cy0, cy1, ka, kb, depth_at, plot);
                }
            }
        }
        __syncthreads();
        uint32_t abits[DRAW_ROWS] = {};
        // this lane's pixels: one column, rows (tid >> 6) + 4 r of the tile
        if constexpr (AREAS) Pass::area_bits(sh, areas, (int)(x_lo + (tid & 63u)), (int)(y_top + (tid >> 6)), abits);
#pragma unroll
        for (uint32_t r = 0; r < DRAW_ROWS; ++r) {
            const uint32_t p = tid + r * DRAW_THREADS;
            const uint32_t walked = sh.mask[p];
            uint32_t bits = walked | abits[r];
            if (!bits) continue;
            if (walked) sh.mask[p] = 0u;
            touched |= 1u << r;
            uint32_t c = cur[r];
            while (bits) {
                const uint32_t k = (uint32_t)__builtin_ctz(bits);
                bits &= bits - 1u;
                c = Pass::store(sh.cop[k], sh.ccol[k], c);
            }
            cur[r] = c;
        }
        __syncthreads();                                                // (the next chunk overwrites the entries)
    };
    // appends the records base + tid that `take` to ids[at...] in array order; returns how many the workgroup appended
    auto append_ordered = [&](bool take, uint32_t id, uint32_t at) -> uint32_t {
        const unsigned long long bal = __ballot(take);
        const uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) sh.wcnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = at, total = 0;
        for (uint32_t w = 0; w < DRAW_THREADS / 64; ++w) { if (w < wave) off += sh.wcnt[w]; total += sh.wcnt[w]; }
        if (take) sh.ids[off + before] = id;
        __syncthreads();
        return total;
    };

    bool scan = SMALL || !a.counters;
    if (!scan) {
        const uint32_t cnt = *draw_counter(a, tile), long_n = *draw_long_counter(a, a.parity);
        __syncthreads();                                                // (everyone has read the counters)
        if (tid == 0) *draw_counter(a, tile) = 0u;                      // zero again for the next binned batch
        if (tid == 0 && tile == 0) *draw_long_counter(a, a.parity ^ 1u) = 0u;   // (the previous binned batch's, done: the next batch's now)
        scan = cnt > LINE_TILE_CAP || long_n > LINE_LONG_CAP;
        if (!scan) {
            for (uint32_t k = tid; k < cnt; k += DRAW_THREADS) sh.ids[k] = a.lists[(size_t)tile * LINE_TILE_CAP + k];
            uint32_t m = cnt;
            for (uint32_t base = 0; base < long_n; base += DRAW_THREADS) {
                const uint32_t k = base + tid;
                const uint32_t id = k < long_n ? a.long_list[k] : 0u;
                m += append_ordered(k < long_n && touches(a.recs[id]), id, m);
            }
            if (m == 0) return;
            uint32_t P = 2;
            while (P < m) P <<= 1;
            for (uint32_t k = m + tid; k < P; k += DRAW_THREADS) sh.ids[k] = 0xFFFFFFFFu;
            __syncthreads();
            for (uint32_t k = 2; k <= P; k <<= 1)                           // bitonic sort, ascending
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    for (uint32_t t = tid; t < P; t += DRAW_THREADS) {
                        const uint32_t u = t ^ j;
                        if (u > t) {
                            const uint32_t x = sh.ids[t], y = sh.ids[u];
                            if ((x > y) == ((t & k) == 0)) { sh.ids[t] = y; sh.ids[u] = x; }
                        }
                    }
                    __syncthreads();
                }
            for (uint32_t done = 0; done < m; done += DRAW_CHUNK) process_chunk(sh.ids + done, min(DRAW_CHUNK, m - done));
        }
    }
    if (scan) {
        uint32_t pend = 0;                                              // ids[0, pend): taken, not yet drawn (fewer than a chunk)
        for (uint32_t base = 0; base < a.n; base += DRAW_THREADS) {
            const uint32_t k = base + tid;
            const uint32_t total = pend + append_ordered(k < a.n && touches(rec_at(k)), k, pend);
            uint32_t done = 0;
            for (; total - done >= DRAW_CHUNK; done += DRAW_CHUNK) process_chunk(sh.ids + done, DRAW_CHUNK);
            pend = total - done;
            if (done && pend) {                                         // the rest to the front
                const uint32_t v = tid < pend ? sh.ids[done + tid] : 0u;
                __syncthreads();
                if (tid < pend) sh.ids[tid] = v;
                __syncthreads();
            }
        }
        if (pend) process_chunk(sh.ids, pend);
    }
    if (!loaded) return;
#pragma unroll
    for (uint32_t r = 0; r < DRAW_ROWS; ++r) {
        if (!(touched & (1u << r))) continue;
        const uint32_t p = tid + r * DRAW_THREADS;
        a.fb[(size_t)(y_top + (p >> 6)) * a.width + x_lo + (p & 63u)] = cur[r];
    }
}

// small != nullptr: a.n <= N records passed by value, one launch; else the bin kernel (tile route only) and the tile kernel
template <class Rec, uint32_t N>
void draw_launch(hipStream_t s, const DrawArgs<Rec>& a, const Rec* small, void (*bin)(DrawArgs<Rec>),
                 void (*tile_small)(DrawArgs<Rec>, DrawBatch<Rec, N>), void (*tile_large)(DrawArgs<Rec>, DrawBatch<Rec, N>)) {
    const uint32_t ntiles = a.tiles_x * a.tiles_y;
    if (!a.n || !ntiles) return;
    DrawBatch<Rec, N> batch;
    if (small) {
        for (uint32_t i = 0; i < a.n && i < N; ++i) batch.r[i] = small[i];
        hipLaunchKernelGGL(tile_small, dim3(ntiles), dim3(DRAW_THREADS), 0, s, a, batch);
        return;
    }
    if (a.counters) hipLaunchKernelGGL(bin, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tile_large, dim3(ntiles), dim3(DRAW_THREADS), 0, s, a, batch);
}

}  // namespace b32
