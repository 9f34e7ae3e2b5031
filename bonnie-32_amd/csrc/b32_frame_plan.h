// b32_frame_plan.h -- the decisions of one frame's plan as pure functions of plain integers and bools: the cut tile grid, the cursor
// gate's threshold, which hand-over joins the setup kernel to the fill, whether the next frame may take the second frame set, whether
// the fused kernel is the kernel that runs, its workgroup form, and the two patiences of the spin kernels.  enqueue_frame
// (b32_frame.hip) and launch_fill (b32_fill.hip) take every one of them from here and spell none of them again.  Nothing of HIP is
// included: tests/cpp/frame_plan_host.cpp compiles this text for the host and compares it with the expressions it replaced.
#pragma once
#include <cstdint>

namespace b32 {

// ------------------------------------------------------------------ patiences of the spin kernels (10 ns ticks of the wall clock)
// k_gate, k_join and the fill that polls its own hand-over give up after PATIENCE_TICKS and raise the sticky error bit: 2 s, a last
// resort -- queues of an oversubscribed GPU are time-sliced in milliseconds.  After a b32_debug_inject the signal is known not to come:
// 2 ms, then the error.
constexpr uint32_t PATIENCE_TICKS = 200000000u;
constexpr uint32_t PATIENCE_INJECTED_TICKS = 200000u;

// ------------------------------------------------------------------ cut tile grid
constexpr uint32_t PLAN_TILE_H = 64;          // the uncut tile's rows (TILE_H, b32_device.h)
struct TileGrid { uint32_t tile_h, tile_yb, tiles_y; };
// Too few 64x64 tiles to fill the GPU (narrow multi-GPU band, PS1-sized frame): tiles of 32, 16 or 8 rows multiply the parallelism of
// the fused kernel.  An empty band keeps the uncut grid (no rows).
inline TileGrid plan_cut_grid(uint32_t tiles_x, uint32_t band_y0, uint32_t band_y1, uint32_t n_cu, uint32_t min_tile_h) {
    uint32_t th = PLAN_TILE_H;
    if (band_y1 <= band_y0) return { th, (band_y0 / th) * th, 0u };
    // 64 -> 32 rows below two tiles per CU, 32 -> 16 -> 8 rows below one tile per CU (measured: a 240-row band of C3 prefers 320 tiles
    // of 32 rows to 600 of 16; C2's 20 tiles prefer 150 of 8 rows -- 0.039 ms against 0.051 with 75 of 16 rows, 0.049 with 300 of 4)
    while (th > min_tile_h && tiles_x * ((band_y1 + th - 1) / th - band_y0 / th) < (th == PLAN_TILE_H ? 2u : 1u) * n_cu &&
           (band_y1 - band_y0) / (th / 2) + 2 <= 255 /* tile rows must fit the packed spans */) th /= 2;
    const uint32_t yb = (band_y0 / th) * th;
    return { th, yb, (band_y1 - yb + th - 1) / th };
}

// ------------------------------------------------------------------ cursor gate (b32_set_pipeline_gate)
// How far the tile cursor of the polled fill (`tiles` tiles, `groups` workgroups) must have got before the next setup kernel starts.
// The fused kernel's workgroups take their next tile from the cursor after the coverage of the current one: the cursor passes
// tiles - groups when the last tile is handed out, and every fetch beyond that is a workgroup that found the queue empty and has only
// the shading of its last tile left, i.e. is about to free its place on a CU.  Up to 1000 the setting counts those fetches (1: the last
// tile has been handed out, 1000: every workgroup but one has come back); above 1000 it is a share of the tiles handed out before.
inline uint32_t plan_gate_need(uint32_t gate_permille, uint32_t tiles, uint32_t groups) {
    if (!gate_permille || !tiles) return 0u;
    const uint32_t pre = tiles > groups ? tiles - groups : 0u;      // cursor value when the last tile is handed out
    return gate_permille > 1000u ? (uint32_t)((uint64_t)(gate_permille - 1000u) * pre / 1000u)
                                 : pre + (uint32_t)((uint64_t)(gate_permille - 1u) * groups / 1000u);
}

// ------------------------------------------------------------------ the fused kernel is the kernel that runs
// The frame's tile lists are the sort-free path's (prio64), something solid is drawn (no wireframe_overlay) and the frame is not an
// ordered walk of whole lists: launch_fill then launches the fused coverage + shading kernel.  Everything that hangs on that kernel --
// the polled hand-over, the start word the next frame's gate waits for, its deferral to k_blend, the folded clear, the LDS atlas and
// span coverage counters, the tile count remembered for the cursor gate -- asks this and nothing else.
inline bool plan_fused(bool prio64, bool wire_front, bool ordered_all) { return prio64 && !wire_front && !ordered_all; }

// The fused kernel's workgroup form: 16 waves per tile while every tile can have a CU of its own, else 8 waves, two workgroups per CU
// (with more tiles than CUs the 8-wave form is faster -- a 960-row band of C3, 600 tiles: 0.112 -> 0.086 ms; 480 rows: 0.086 -> 0.067;
// 240 rows: 0.067 -> 0.057).  fill_args sizes the LDS index atlas for this form and launch_fill launches it (FillArgs::wide).
inline bool plan_wide(uint32_t ntiles, uint32_t n_cu, bool narrow_only) { return ntiles <= n_cu && !narrow_only; }

// ------------------------------------------------------------------ two frames in flight: may the NEXT frame take the other frame set
// Only large meshes on the direct-binning route: the frames of small ones are launch-latency bound and the cross-stream events cost
// them more than the overlap returns -- a 12-room console frame 0.72 ms against 0.65; keyed routes have binning launches behind k_setup:
// one stream.
// ... and a frame whose fused kernel has no more tiles than workgroup slots has no tail to fill: the cross-stream waits (~10 us
// between two kernels) then cost more than the overlap returns (C2, 100 k triangles at 320x240: 0.052 against 0.048 ms).  The merged
// runs of a batched frame are the exception: their kernels leave most of the GPU idle anyway (75 tiles for 256 CUs).
// Round 6: with the flag / join kernel pair (no cross-stream event: ~5 us instead of ~12) frames WITHOUT a tail pay too when their two
// kernels are of comparable length -- C2, 100 k triangles at 320x240: setup 15.7 + fill 21.9 us, 0.0375 -> 0.0339 ms per frame --
// but only on that hand-over (the small-mesh route keeps the event: C1 0.0235 -> 0.0281), i.e. while the caller's stream and the side
// stream have different priorities (unknown before the first pipelined frame of a stream: tried once, then decided): `join_small`.
// The same for the frames of a screen band (one rank of a sharded frame: 240 rows of C4 are 320 tiles of 32 rows) -- round 5 had measured
// them with the event (N = 8 band 0.067 -> 0.071: no); with the kernel pair the weak series' N = 8 point goes 0.054 -> 0.042 ms per rank.
inline bool plan_pipe_hint(bool direct_bin, uint32_t ntiles, uint32_t n_cu, bool batched, bool join_small) {
    return direct_bin && (ntiles > 2u * n_cu || batched || join_small);
}

// ------------------------------------------------------------------ setup -> fill hand-over of a pipelined frame
enum class HandOver {
    None,         // not pipelined: setup and fill are on one stream
    Poll,         // k_flag_poll behind the setup kernel; the fused kernel polls the word itself (FillArgs::join_seq)
    FlagJoin,     // k_flag behind the setup kernel on the side stream, k_join in front of the fill on the main stream
    Event         // cross-stream event (ev_setup)
};
struct HandOverIn {
    bool pipelined;       // the setup kernel runs on the side stream (after the pipe_hint correction: such a frame is direct-binned)
    bool batched;         // a merged run of a batched frame
    bool join_ok;         // the caller's stream and the side stream have different priorities: they never share a hardware queue
    bool direct_bin, wire_front, ordered_all;
    uint32_t ntiles, n_cu;
    bool narrow_only;     // B32_ROUTE_WIDE_GROUPS is off
};
// Poll -- the merged draws of a batched frame: their fills are few 16-wave workgroups (at most 5 / 8 of the CUs: the setup kernel they
// may have to spin for keeps the rest of the GPU), the setup kernel of draw k + 1 has normally finished beside draw k's fill and blend
// pass, and what the cross-stream event cost the main stream per draw (6.5 us between k_blend's end and the next fill's start:
// tools/console_trace.sh) was most of what there was to save in a console frame.
// FlagJoin -- no cross-stream event on the fill's path: see k_flag / k_join.  The merged runs of a batched frame keep the event: their
// kernels are so short that the two extra launches cost what the barrier packet did -- console frame 0.268-0.275 against 0.264-0.265 ms.
// Streams of different priorities never share a hardware queue (the runtime pools its queues by priority); two streams of ONE priority
// may, and k_join in front of k_flag in the same queue would wait for its patience: those keep the event (!join_ok).
inline HandOver plan_hand_over(const HandOverIn& in) {
    if (!in.pipelined) return HandOver::None;
    // (a direct-binned frame's tile lists are the sort-free path's: its fill is the fused kernel unless the frame draws nothing solid)
    if (in.batched && in.join_ok && plan_fused(in.direct_bin, in.wire_front, in.ordered_all) && in.ntiles && 8u * in.ntiles <= 5u * in.n_cu &&
        !in.narrow_only)
        return HandOver::Poll;
    if (in.direct_bin && in.join_ok && !in.batched) return HandOver::FlagJoin;
    return HandOver::Event;
}

}  // namespace b32
