// frame_plan_host.cpp -- csrc/b32_frame_plan.h compiled for the host (tests/test_frame_plan.py builds and runs this).
//   (a) the documented cases of each decision, as literals;
//   (b) every decision against the expressions it replaced: the old_* functions below are the text of enqueue_frame, plan_route, frame_params
//       and fill_args (b32_frame.hip) and of launch_fill (b32_fill.hip) at commit 1d989c2, the parent of the change that introduced the
//       header, over small stand-ins for the context and the frame parameters -- compared over a grid of inputs, every combination.
// Prints one "cases <decision> <count>" line per grid and "ok"; the first difference is printed and the exit status is 1.
#include "b32_frame_plan.h"

#include <cstdio>
#include <initializer_list>

using namespace b32;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// ---------------------------------------------------------------- the parent's text (1d989c2)
namespace parent {
constexpr uint32_t TILE_H = 64;
constexpr int B32_MIN_TILE_H = 8;
constexpr uint32_t B32_ROUTE_WIDE_GROUPS = 16;
struct Ctx {
    uint32_t band_y0, band_y1; int n_cu; uint32_t gate_permille; uint32_t route_off;
    bool pipelined, frame_batched, join_ok, pipe_hint; int join_stream;
};
struct Fp { uint32_t tiles_x, tile_h, tile_yb, tiles_y; };
struct Route { bool direct_bin, want_inline, ordered_all, prio64; };

// frame_params (the uncut grid), then plan_route's cut for a sort-free frame with B32_ROUTE_CUT_TILES on
static void old_cut_grid(const Ctx* c, Fp& fp) {
    fp.tile_h = TILE_H;
    fp.tile_yb = (c->band_y0 / TILE_H) * TILE_H;
    fp.tiles_y = c->band_y1 > c->band_y0 ? (c->band_y1 - fp.tile_yb + TILE_H - 1) / TILE_H : 0;
    if (c->band_y1 > c->band_y0) {
        uint32_t th = TILE_H;
        while (th > (uint32_t)B32_MIN_TILE_H && fp.tiles_x * ((c->band_y1 + th - 1) / th - c->band_y0 / th) < (th == TILE_H ? 2u : 1u) * (uint32_t)c->n_cu &&
               (c->band_y1 - c->band_y0) / (th / 2) + 2 <= 255 /* tile rows must fit the packed spans */) th /= 2;
        fp.tile_h = th;
        fp.tile_yb = (c->band_y0 / th) * th;
        fp.tiles_y = (c->band_y1 - fp.tile_yb + th - 1) / th;
    }
}
// enqueue_frame, the cursor gate (alt[0].d_ctrl present)
static uint32_t old_gate_need(const Ctx* c, uint32_t polled_tiles, uint32_t polled_groups) {
    uint32_t gate_need = 0;
    if (c->gate_permille && polled_tiles) {
        const uint32_t groups = polled_groups, tiles = polled_tiles;
        const uint32_t pre = tiles > groups ? tiles - groups : 0u;      // cursor value when the last tile is handed out
        const uint32_t need = c->gate_permille > 1000u ? (uint32_t)((uint64_t)(c->gate_permille - 1000u) * pre / 1000u)
                                                       : pre + (uint32_t)((uint64_t)(c->gate_permille - 1u) * groups / 1000u);
        gate_need = need;
    }
    return gate_need;
}
// enqueue_frame from the pipe_hint to the hand-over: 0 none, 1 polled, 2 flag / join, 3 event.  c->pipelined comes in as the rotation left it.
static int old_hand_over(Ctx* c, const Route& r, const Fp& fp, bool wire_front) {
    const int s = 1;
    const uint32_t ntiles = fp.tiles_x * fp.tiles_y;
    const bool join_small = !c->frame_batched && (c->join_stream != s || c->join_ok);
    c->pipe_hint = r.direct_bin && (ntiles > 2u * (uint32_t)c->n_cu || c->frame_batched || join_small);
    if (!c->pipe_hint) c->pipelined = false;
    const bool poll_batched = c->pipelined && c->frame_batched && c->join_ok && (r.direct_bin || r.want_inline) && !wire_front && !r.ordered_all &&
                              ntiles && 8u * ntiles <= 5u * (uint32_t)c->n_cu && !(c->route_off & B32_ROUTE_WIDE_GROUPS);
    if (poll_batched) {
        return 1;
    } else if (c->pipelined && r.direct_bin && c->join_ok && !c->frame_batched) {
        return 2;
    } else if (c->pipelined) {
        return 3;
    }
    return 0;
}
// enqueue_frame: "the fused kernel is the kernel that runs", as the start-loss injection, start_defer, the clear fold, the two route counters
// and last_cover_tiles spelled it
static bool old_fused(const Route& r, bool wire_front) { return r.prio64 && !wire_front && !r.ordered_all; }
// launch_fill: the same decision by its order of early returns.  0 nothing, 1 event only, 2 ordered walk, 3 fused kernel, 4 keyed kernels
struct FillArgsBits { uint32_t skip_solid, ordered_all, prio64, narrow_only; };
static int old_launch_fill(const FillArgsBits& a, uint32_t ntiles) {
    if (ntiles == 0) return 0;
    if (a.skip_solid) return 1;
    if (a.ordered_all) return 2;
    if (a.prio64) return 3;
    return 4;
}
// the workgroup form, in fill_args (for the atlas room) and in launch_fill (for the kernel)
static bool old_wide_fill_args(const Ctx* c, const Fp& fp) {
    const bool wide = fp.tiles_x * fp.tiles_y <= (uint32_t)c->n_cu && !(c->route_off & B32_ROUTE_WIDE_GROUPS);
    return wide;
}
static bool old_wide_launch_fill(const FillArgsBits& a, uint32_t ntiles, int n_cu) {
    const bool wide = ntiles <= (uint32_t)n_cu && !a.narrow_only;
    return wide;
}
}  // namespace parent

// ---------------------------------------------------------------- (a) documented cases
static void documented_cases() {
    const uint32_t CU = 256, MIN_H = 8;
    TileGrid g = plan_cut_grid(40, 0, 240, CU, MIN_H);
    CHECK(g.tile_h == 32 && g.tile_yb == 0 && g.tiles_y == 8, "%u %u %u", g.tile_h, g.tile_yb, g.tiles_y);      // 320 tiles of 32 rows
    g = plan_cut_grid(40, 240, 480, CU, MIN_H);
    CHECK(g.tile_h == 32 && g.tile_yb == 224 && g.tiles_y == 8, "%u %u %u", g.tile_h, g.tile_yb, g.tiles_y);
    g = plan_cut_grid(5, 0, 240, CU, MIN_H);
    CHECK(g.tile_h == 8 && g.tiles_y == 30, "%u %u %u", g.tile_h, g.tile_yb, g.tiles_y);                          // 150 tiles of 8 rows
    g = plan_cut_grid(40, 0, 1920, CU, MIN_H);
    CHECK(g.tile_h == 64 && g.tiles_y == 30, "%u %u %u", g.tile_h, g.tile_yb, g.tiles_y);
    g = plan_cut_grid(40, 100, 100, CU, MIN_H);
    CHECK(g.tile_h == 64 && g.tile_yb == 64 && g.tiles_y == 0, "%u %u %u", g.tile_h, g.tile_yb, g.tiles_y);      // an empty band is left at 64

    CHECK(plan_gate_need(1, 1200, 512) == 688, "%u", plan_gate_need(1, 1200, 512));
    CHECK(plan_gate_need(1000, 1200, 512) == 1199, "%u", plan_gate_need(1000, 1200, 512));
    CHECK(plan_gate_need(1150, 1200, 512) == 103, "%u", plan_gate_need(1150, 1200, 512));
    CHECK(plan_gate_need(1001, 1200, 512) == 0, "%u", plan_gate_need(1001, 1200, 512));
    CHECK(plan_gate_need(0, 1200, 512) == 0, "%u", plan_gate_need(0, 1200, 512));
    CHECK(plan_gate_need(500, 20, 20) == 9, "%u", plan_gate_need(500, 20, 20));                                   // 499 * 20 / 1000

    HandOverIn in{};
    in.n_cu = CU; in.ntiles = 160;
    CHECK(plan_hand_over(in) == HandOver::None, "not pipelined");
    in.pipelined = in.batched = in.join_ok = in.direct_bin = true;
    CHECK(plan_hand_over(in) == HandOver::Poll, "8 * 160 == 5 * 256: the last tile count that polls");
    in.ntiles = 161;
    CHECK(plan_hand_over(in) == HandOver::Event, "a batched frame never takes the flag / join pair");
    in.ntiles = 160;
    for (int k = 0; k < 4; ++k) {          // Poll is refused by each of these
        HandOverIn x = in;
        if (k == 0) x.wire_front = true;
        if (k == 1) x.ordered_all = true;
        if (k == 2) x.ntiles = 0;
        if (k == 3) x.narrow_only = true;
        CHECK(plan_hand_over(x) == HandOver::Event, "refusal %d", k);
    }
    in.batched = false;
    CHECK(plan_hand_over(in) == HandOver::FlagJoin, "not batched, join_ok, direct_bin");
    in.join_ok = false;
    CHECK(plan_hand_over(in) == HandOver::Event, "streams of one priority keep the event");

    CHECK(PATIENCE_TICKS == 200000000u && PATIENCE_INJECTED_TICKS == 200000u, "2 s and 2 ms in 10 ns ticks");
}

// ---------------------------------------------------------------- (b) against the parent, exhaustively
static const uint32_t NTILES[] = { 0, 1, 160, 161, 256, 257, 512, 513, 1200 };
static const int N_CU[] = { 1, 104, 256 };
static const uint32_t PERMILLE[] = { 0, 1, 500, 1000, 1001, 1150, 2000 };
static const uint32_t BANDS[][2] = { { 0, 1 }, { 0, 240 }, { 240, 480 }, { 7, 9 }, { 0, 1920 }, { 1000, 1064 } };
static const uint32_t TILES_X[] = { 1, 5, 40 };

static void against_the_parent() {
    unsigned long n = 0;
    for (const auto& band : BANDS) for (uint32_t tx : TILES_X) for (int cu : N_CU) {
        parent::Ctx c{}; c.band_y0 = band[0]; c.band_y1 = band[1]; c.n_cu = cu;
        parent::Fp fp{}; fp.tiles_x = tx;
        parent::old_cut_grid(&c, fp);
        const TileGrid g = plan_cut_grid(tx, band[0], band[1], (uint32_t)cu, (uint32_t)parent::B32_MIN_TILE_H);
        CHECK(g.tile_h == fp.tile_h && g.tile_yb == fp.tile_yb && g.tiles_y == fp.tiles_y, "band %u..%u tiles_x %u n_cu %d: %u %u %u against %u %u %u",
              band[0], band[1], tx, cu, g.tile_h, g.tile_yb, g.tiles_y, fp.tile_h, fp.tile_yb, fp.tiles_y);
        ++n;
    }
    std::printf("cases cut_grid %lu\n", n);

    n = 0;
    for (uint32_t p : PERMILLE) for (uint32_t tiles : NTILES) for (int cu : N_CU) {
        const uint32_t groups = tiles < 2u * (uint32_t)cu ? tiles : 2u * (uint32_t)cu;      // (what remember_cover notes for such a fill)
        parent::Ctx c{}; c.gate_permille = p;
        const uint32_t want = parent::old_gate_need(&c, tiles, groups), got = plan_gate_need(p, tiles, groups);
        CHECK(got == want, "permille %u tiles %u groups %u: %u against %u", p, tiles, groups, got, want);
        ++n;
    }
    std::printf("cases gate %lu\n", n);

    // the hand-over and the pipe_hint: nine bools, every combination
    n = 0;
    for (unsigned bits = 0; bits < 512; ++bits) for (uint32_t ntiles : NTILES) for (int cu : N_CU) {
        const bool rotated = bits & 1, batched = bits & 2, join_ok = bits & 4, join_fresh = bits & 8, direct_bin = bits & 16, want_inline = bits & 32,
                   wire_front = bits & 64, ordered_all = bits & 128, narrow = bits & 256;
        parent::Ctx c{}; c.n_cu = cu; c.pipelined = rotated; c.frame_batched = batched; c.join_ok = join_ok; c.join_stream = join_fresh ? 0 : 1;
        c.route_off = narrow ? parent::B32_ROUTE_WIDE_GROUPS : 0u;
        parent::Route r{}; r.direct_bin = direct_bin; r.want_inline = want_inline; r.ordered_all = ordered_all;
        parent::Fp fp{}; fp.tiles_x = 1; fp.tiles_y = ntiles;
        const int want = parent::old_hand_over(&c, r, fp, wire_front);
        // the new text of plan_pipeline (b32_frame.hip)
        const bool join_small = !batched && (join_fresh || join_ok);
        const bool hint = plan_pipe_hint(direct_bin, ntiles, (uint32_t)cu, batched, join_small);
        const bool pipelined = rotated && hint;
        const HandOver got = plan_hand_over({ pipelined, batched, join_ok, direct_bin, wire_front, ordered_all, ntiles, (uint32_t)cu, narrow });
        CHECK(hint == c.pipe_hint && pipelined == c.pipelined, "pipe_hint: bits %u ntiles %u n_cu %d", bits, ntiles, cu);
        CHECK((int)got == want, "hand-over: bits %u ntiles %u n_cu %d: %d against %d", bits, ntiles, cu, (int)got, want);
        ++n;
    }
    std::printf("cases hand_over %lu\n", n);

    n = 0;
    for (unsigned bits = 0; bits < 8; ++bits) for (uint32_t ntiles : NTILES) {
        const bool prio64 = bits & 1, wire_front = bits & 2, ordered_all = bits & 4;
        parent::Route r{}; r.prio64 = prio64; r.ordered_all = ordered_all;
        const parent::FillArgsBits a{ wire_front ? 1u : 0u, ordered_all ? 1u : 0u, prio64 ? 1u : 0u, 0u };
        const bool got = plan_fused(prio64, wire_front, ordered_all);
        CHECK(got == parent::old_fused(r, wire_front), "fused: bits %u", bits);
        CHECK((got && ntiles) == (parent::old_launch_fill(a, ntiles) == 3), "launch_fill's order of returns: bits %u ntiles %u", bits, ntiles);
        ++n;
    }
    std::printf("cases fused %lu\n", n);

    n = 0;
    for (uint32_t ntiles : NTILES) for (int cu : N_CU) for (int narrow = 0; narrow < 2; ++narrow) {
        parent::Ctx c{}; c.n_cu = cu; c.route_off = narrow ? parent::B32_ROUTE_WIDE_GROUPS : 0u;
        parent::Fp fp{}; fp.tiles_x = 1; fp.tiles_y = ntiles;
        const parent::FillArgsBits a{ 0u, 0u, 1u, narrow ? 1u : 0u };
        const bool got = plan_wide(ntiles, (uint32_t)cu, narrow != 0);
        CHECK(got == parent::old_wide_fill_args(&c, fp) && got == parent::old_wide_launch_fill(a, ntiles, cu), "wide: ntiles %u n_cu %d narrow %d", ntiles, cu, narrow);
        ++n;
    }
    std::printf("cases wide %lu\n", n);
}

int main() {
    documented_cases();
    against_the_parent();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
