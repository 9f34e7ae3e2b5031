// b32_pick_words.h -- the three minima that stand for "closest in loop order" (see b32_pick.hip for the why): what a lane takes, how two
// sets fold and how a finished set names its winner.  Shared by the pick, the hover and the room hover (b32_pick_body.h holds what they
// share on the device and in the library).  The text also compiles for the host (B32_HD, b32_world_point.h): tests/cpp/room_host.cpp
// drives b32_room_body.h's candidates through it.
#pragma once
#include "b32_world_point.h"

namespace b32 {

constexpr uint32_t PICK_CHUNK = 1024;           // elements per workgroup: 256 lanes, four trips
constexpr uint32_t PICK_NONE = 0xFFFFFFFFu;
constexpr uint32_t PICK_QNAN = 0x7FC00000u;     // the one NaN a NaN depth is reported as (as b32_draw_world's records)

struct PickWords { unsigned long long key; uint32_t first, first_nan; };
B32_HD PickWords pick_no_hit() { PickWords m; m.key = ~0ull; m.first = PICK_NONE; m.first_nan = PICK_NONE; return m; }

B32_HD uint32_t pick_min(uint32_t a, uint32_t b) { return b < a ? b : a; }
B32_HD unsigned long long pick_min(unsigned long long a, unsigned long long b) { return b < a ? b : a; }

// total order of the non-NaN f32 as u32, both zeros on one value
B32_HD uint32_t pick_orderable(float d) {
    uint32_t u; __builtin_memcpy(&u, &d, 4);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// One hit into a lane's three minima; `id` is the triangle (k_pick, k_hover), the item (k_pick_resolve) or the record's element (k_room_hover).
B32_HD void pick_take(PickWords& m, float depth, uint32_t id) {
    m.first = pick_min(m.first, id);
    if (depth != depth) m.first_nan = pick_min(m.first_nan, id);
    else m.key = pick_min(m.key, ((unsigned long long)pick_orderable(depth) << 32) | id);
}
// Another set's minima into this one: another lane's, another wave's, another workgroup's.
B32_HD void pick_fold(PickWords& into, const PickWords& m) {
    into.key = pick_min(into.key, m.key); into.first = pick_min(into.first, m.first); into.first_nan = pick_min(into.first_nan, m.first_nan);
}
// The winner of a finished set: false = none; nan = the first hit's depth was a NaN (it stuck), else the key's id
B32_HD bool pick_winner(const PickWords& w, uint32_t& id, bool& nan) {
    if (w.first == PICK_NONE) return false;
    nan = w.first == w.first_nan;
    id = nan ? w.first : (uint32_t)w.key;
    return true;
}

}  // namespace b32
