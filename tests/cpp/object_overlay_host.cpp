// object_overlay_host.cpp -- csrc/b32_object_overlay_body.h (the device code of b32_draw_object_overlays' arithmetic, and the host's plan of
// rows) compiled for the host, for tests/test_object_overlay.py.  No device, no library.  The batch goes through object_overlay_plan as the
// producer calls it (count only, then with rows); every workgroup of the plan finds its row with object_row_of and every one of its 256
// lanes runs object_overlay_lane, as k_object_overlay does; a part's bounds block is folded with overlay_bounds_take as k_scene_bounds'
// lanes do (two running blocks, even and odd vertices, joined in keys).
//   usage: object_overlay_host <in> <out>
//   in : u32 width, height, n_parts, n_items; 12 f32 camera (position, basis_x, basis_y, basis_z);
//        per part: u32 flags, _pad, slot (0: NULL, 1: holds its scene, 2: does not), has_topology, nh, nv, stride; nh x 2 u32 (v0, v1);
//        nv x stride f32 (the position in front); then n_items B32ObjectItem
//   out: i32 rc, u32 rows, u64 total, u64 groups, 3 u64 drawn / dropped / rejected; n_parts x 8 u32 (b32_scene_bounds' 32 bytes of each
//        part); total B32Prim.  rc != 0: the first four only.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "b32_object_overlay_body.h"

struct Part { uint32_t head[7]; std::vector<uint32_t> he; std::vector<float> pos; b32::OverlayBounds bounds; };

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return !n || std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    using namespace b32;
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t head[4]; B32Camera cam;
    if (std::fread(head, 4, 4, in) != 4 || std::fread(&cam, 4, 12, in) != 12) return 3;
    const uint32_t w = head[0], h = head[1], n_parts = head[2], n_items = head[3];
    std::vector<Part> P(n_parts);
    for (Part& p : P) {
        if (std::fread(p.head, 4, 7, in) != 7) return 3;
        std::vector<uint32_t> pairs;
        if (!get(in, pairs, (size_t)p.head[4] * 2) || !get(in, p.pos, (size_t)p.head[5] * p.head[6])) return 3;
        p.he.assign((size_t)p.head[4] * 4, 0u);                     // four words per half-edge, (v0, v1) in front
        for (size_t k = 0; k < p.head[4]; ++k) { p.he[4 * k] = pairs[2 * k]; p.he[4 * k + 1] = pairs[2 * k + 1]; p.he[4 * k + 2] = 0xDEADu; p.he[4 * k + 3] = 0xBEEFu; }
        OverlayBounds even = overlay_bounds_start(), odd = overlay_bounds_start();
        for (uint32_t i = 0; i < p.head[5]; ++i) overlay_bounds_take((i & 1u) ? odd : even, p.pos.data() + (size_t)i * p.head[6]);
        p.bounds = overlay_bounds_start();
        object_bounds_fold(p.bounds, odd); object_bounds_fold(p.bounds, even);
    }
    std::vector<B32ObjectItem> items;
    if (!get(in, items, n_items)) return 3;
    std::fclose(in);

    std::vector<B32ObjectPart> parts(n_parts);
    std::vector<ObjectPartView> views(n_parts);
    for (uint32_t k = 0; k < n_parts; ++k) {
        const Part& p = P[k];
        // (the plan never reads through a slot or a topology: any non-null address stands for one)
        parts[k].slot = p.head[2] ? reinterpret_cast<b32_scene*>(&P[k]) : nullptr;
        parts[k].topology = p.head[3] ? reinterpret_cast<b32_topology*>(&P[k]) : nullptr;
        parts[k].flags = p.head[0]; parts[k]._pad = p.head[1];
        ObjectPartView& v = views[k];
        v.holds_scene = p.head[2] == 1u; v.has_topology = p.head[3] != 0u;
        v.he = p.he.data(); v.nh = p.head[4];
        v.pos = p.pos.data(); v.stride = p.head[6]; v.nv = p.head[5];
        v.bounds = &p.bounds;
    }
    ObjectOverlayPlan count, plan;
    int rc = object_overlay_plan(parts.data(), views.data(), n_parts, items.data(), n_items, false, count);
    if (!rc) rc = object_overlay_plan(parts.data(), views.data(), n_parts, items.data(), n_items, true, plan);
    if (!rc && (plan.total != count.total || plan.groups != count.groups || !count.rows.empty())) return 6;

    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const int32_t rc32 = rc; const uint32_t n_rows = (uint32_t)plan.rows.size();
    const uint64_t tg[2] = { rc ? 0 : plan.total, rc ? 0 : plan.groups };
    std::fwrite(&rc32, 4, 1, f); std::fwrite(&n_rows, 4, 1, f); std::fwrite(tg, 8, 2, f);
    if (rc) { std::fclose(f); return 0; }

    ViewBlock v;
    view_fill(v, cam, w, h, nullptr);
    std::vector<B32Prim> out((size_t)plan.total);
    for (B32Prim& o : out) { o = B32Prim{}; o.kind = 0xEE; }        // (a place no lane writes stays visible)
    unsigned long long counts[3] = { 0, 0, 0 };
    for (uint64_t wg = 0; wg < plan.groups; ++wg) {
        const uint32_t r = object_row_of(plan.rows.data(), n_rows, (uint32_t)wg);
        const ObjectRow& row = plan.rows[r];
        for (uint32_t lane = 0; lane < OBJECT_LANES; ++lane) {
            const uint32_t which = object_overlay_lane(v, row, plan.bounds.data(), (uint32_t)wg - row.first_wg, lane, out.data());
            if (which < 3u) ++counts[which];
        }
    }
    std::fwrite(counts, 8, 3, f);
    for (const Part& p : P) {
        uint32_t res[8];
        object_bounds_result(p.bounds, p.head[5] ? 1u : 0u, res);
        std::fwrite(res, 4, 8, f);
    }
    if (!out.empty()) std::fwrite(out.data(), sizeof(B32Prim), out.size(), f);
    std::fclose(f);
    return 0;
}
