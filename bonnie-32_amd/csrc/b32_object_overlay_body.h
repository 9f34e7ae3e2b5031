// b32_object_overlay_body.h -- the arithmetic of the world editor's object overlays for one record: draw_asset_wireframe
// (editor/viewport_3d.rs:255-291), Asset::bounds (asset/asset.rs:288-312) and draw_rotated_bounding_box (viewport_3d.rs:7658-7697).
// k_object_overlay (b32_object_overlay.hip) turns (rows, resident positions, half-edges, bounds keys) into B32Prim records with
// object_overlay_lane; k_scene_bounds folds a slot's positions with overlay_bounds_take.  Every expression is a separately rounded f32
// operation in the reference's order.  Not restated here: draw_3d_line_clipped is world_item's B32_LINE_2D with B32_WORLD_CLIP_NEAR
// (b32_world_body.h), draw_3d_line is gizmo_item's B32_GIZMO_LINE (b32_gizmo_body.h), the keys of the bounds are overlay_key / overlay_unkey /
// overlay_bounds_take (b32_overlay_body.h), the no-op and the 2^30 limit are b32_prim_record.h's.  The text also compiles for the host
// (B32_HD, b32_world_point.h), where tests/test_object_overlay.py runs it against a literal restatement, built with and without
// -ffp-contract=off, and tests/cpp/object_overlay_host.cpp walks the plan and the lanes under the sanitizers.
//
// Where a record lies is a function of the parts' half-edge counts and the item kinds alone (object_overlay_plan): a call the reference
// does not make leaves the no-op record (a circle of radius -1) in its slot.
//   WIRE      the sum of nh over the item's visible parts, in part order then loop order
//   BOX_MESH  12, the edges of :7688-7692
//   BOX       12
// The host lays out ROWS: one per (WIRE item, visible part with half-edges), one per box.  A workgroup of 256 lanes serves exactly one
// row; a row knows its first record and its first workgroup.
#pragma once
#include <vector>
#include "b32_world_body.h"
#include "b32_gizmo_body.h"
#include "b32_overlay_body.h"

namespace b32 {

constexpr uint32_t OBJECT_BOX_SLOTS = 12u, OBJECT_LANES = 256u;
constexpr uint32_t OBJECT_NO_CALL = 3u;             // a lane's outcome when it stands for no call of the reference (counts nothing)
constexpr uint32_t OBJECT_HAS_VERTS = 0x100u;       // ObjectRow::kind: some part of a BOX_MESH item has vertices (has_verts, asset.rs:293)

// One row of the call's table, as it lies on the device.
struct ObjectRow {
    const uint32_t* he;                             // WIRE: the part's half-edges, four words each, (v0, v1) in front (HoverHalfEdge)
    const float* pos;                               // WIRE: the slot's positions, `stride` floats between two vertices
    uint32_t nh, nv, stride;
    uint32_t first_rec, first_wg;                   // the row's first record and first workgroup
    uint32_t first_bound, n_bounds;                 // BOX_MESH: the item's parts in the call's table of bounds blocks
    uint32_t kind;                                  // B32_OBJECT_*, | OBJECT_HAS_VERTS
    B32Placement place;
    float box_min[3], box_max[3];                   // BOX
    uint8_t r, g, b, blend;
};
static_assert(sizeof(ObjectRow) == 96 && sizeof(ObjectRow) % 8 == 0, "ObjectRow travels in a run of words with pointers behind it");

// :276-285 and :7681-7685 (the same text): rotate about Y by the facing, then translate
B32_HD void object_place(const B32Placement& pl, const float* p, float* q) {
    q[0] = (p[0] * pl.cos_f - p[2] * pl.sin_f) + pl.world_pos[0];
    q[1] = p[1] + pl.world_pos[1];
    q[2] = (p[0] * pl.sin_f + p[2] * pl.cos_f) + pl.world_pos[2];
}

// draw_asset_wireframe's half-edge (v0, v1), :271-287, into one record; returns 0 drawn, 1 dropped, 2 rejected.  An index >= nv: the
// no-op, dropped (the reference panics)
B32_HD uint32_t object_wire_edge(const ViewBlock& v, const B32Placement& pl, const float* pos, uint32_t stride, uint32_t nv, uint32_t v0, uint32_t v1,
                                 PrimColor c, B32Prim* out) {
    if (v0 >= nv || v1 >= nv) { *out = prim_noop(); return 1u; }
    const float* a = pos + (size_t)v0 * stride;
    const float* b = pos + (size_t)v1 * stride;
    const float l0[3] = { a[0], a[1], a[2] }, l1[3] = { b[0], b[1], b[2] };
    B32WorldItem it{};
    object_place(pl, l0, it.p0);
    object_place(pl, l1, it.p1);
    it.r = c.r; it.g = c.g; it.b = c.b; it.blend = c.blend;
    it.kind = B32_LINE_2D; it.alpha = 255u; it.flags = B32_WORLD_CLIP_NEAR;
    return world_item(v, it, out);
}

// corner k of :7669-7678 from min / max: x is max for k % 4 in {1, 2}, y for k >= 4, z for k % 4 in {2, 3}
B32_HD void object_box_corner(const float* mn, const float* mx, uint32_t k, float* c) {
    const uint32_t q = k & 3u;
    c[0] = (q == 1u || q == 2u) ? mx[0] : mn[0];
    c[1] = k >= 4u ? mx[1] : mn[1];
    c[2] = q >= 2u ? mx[2] : mn[2];
}
// edge e of :7688-7692 as its two corner indices: bottom (e, (e + 1) % 4), top the same + 4, verticals (e - 8, e - 4)
B32_HD void object_box_edge_corners(uint32_t e, uint32_t& a, uint32_t& b) {
    if (e < 8u) { const uint32_t base = e & 4u; a = base + (e & 3u); b = base + ((e + 1u) & 3u); }
    else { a = e - 8u; b = e - 4u; }
}
// draw_rotated_bounding_box's edge e, :7681-7695, into one record
B32_HD uint32_t object_box_edge(const ViewBlock& v, const B32Placement& pl, const float* mn, const float* mx, uint32_t e, PrimColor c, B32Prim* out) {
    uint32_t ka, kb;
    object_box_edge_corners(e, ka, kb);
    float ca[3], cb[3];
    object_box_corner(mn, mx, ka, ca);
    object_box_corner(mn, mx, kb, cb);
    B32GizmoItem it{};
    object_place(pl, ca, it.p0);
    object_place(pl, cb, it.p1);
    it.r = c.r; it.g = c.g; it.b = c.b; it.blend = c.blend;
    it.kind = B32_GIZMO_LINE;
    return gizmo_item(v, it, out);
}

// Asset::bounds over the parts' finished blocks, asset.rs:291-304: the minimum of minima and the maximum of maxima, in keys (exact and
// order-free); a block still at its start values (no vertex, or only NaN) changes nothing
B32_HD void object_bounds_fold(OverlayBounds& b, const OverlayBounds& part) {
    B32_UNROLL
    for (int c = 0; c < 3; ++c) {
        if (part.mn[c] < b.mn[c]) b.mn[c] = part.mn[c];
        if (part.mx[c] > b.mx[c]) b.mx[c] = part.mx[c];
    }
}

// Lane `lane` of workgroup `wg` of row r: its record, and what it adds to drawn / dropped / rejected (OBJECT_NO_CALL: nothing).
// bounds: the call's table of bounds blocks (BOX_MESH)
B32_HD uint32_t object_overlay_lane(const ViewBlock& v, const ObjectRow& r, const OverlayBounds* const* bounds, uint32_t wg, uint32_t lane, B32Prim* out) {
    const PrimColor col = { r.r, r.g, r.b, r.blend };
    const uint32_t kind = r.kind & 0xFFu;
    if (kind == B32_OBJECT_WIRE) {
        const uint64_t h = (uint64_t)wg * OBJECT_LANES + lane;
        if (h >= r.nh) return OBJECT_NO_CALL;
        const uint32_t* e = r.he + 4u * h;
        return object_wire_edge(v, r.place, r.pos, r.stride, r.nv, e[0], e[1], col, out + r.first_rec + h);
    }
    if (lane >= OBJECT_BOX_SLOTS) return OBJECT_NO_CALL;
    B32Prim* o = out + r.first_rec + lane;
    float mn[3], mx[3];
    if (kind == B32_OBJECT_BOX_MESH) {
        if (!(r.kind & OBJECT_HAS_VERTS)) {         // bounds() is None: no call at all; the item counts once, as dropped
            *o = prim_noop();
            return lane == 0u ? 1u : OBJECT_NO_CALL;
        }
        OverlayBounds b = overlay_bounds_start();
        for (uint32_t k = 0; k < r.n_bounds; ++k) object_bounds_fold(b, *bounds[r.first_bound + k]);
        B32_UNROLL
        for (int c = 0; c < 3; ++c) { mn[c] = overlay_unkey(b.mn[c]); mx[c] = overlay_unkey(b.mx[c]); }
    } else {
        B32_UNROLL
        for (int c = 0; c < 3; ++c) { mn[c] = r.box_min[c]; mx[c] = r.box_max[c]; }
    }
    return object_box_edge(v, r.place, mn, mx, lane, col, o);
}

// b32_scene_bounds' 32 bytes from a finished block: min[3], max[3], has_verts, padding
B32_HD void object_bounds_result(const OverlayBounds& b, uint32_t has_verts, uint32_t* out8) {
    B32_UNROLL
    for (int c = 0; c < 3; ++c) { out8[c] = f32_bits(overlay_unkey(b.mn[c])); out8[3 + c] = f32_bits(overlay_unkey(b.mx[c])); }
    out8[6] = has_verts; out8[7] = 0u;
}

// ---- host: what the plan reads of a part -- the producer fills it from (slot, topology), a test from plain arrays ...
struct ObjectPartView {
    bool holds_scene, has_topology;
    const uint32_t* he; uint32_t nh;                // the topology's half-edges on the device
    const float* pos; uint32_t stride, nv;          // the slot's body positions on the device
    const OverlayBounds* bounds;                    // the slot's bounds block (nullptr while no BOX_MESH item reads it)
};
// ... and what a checked batch becomes: the rows in record order, the table of bounds blocks of the BOX_MESH rows, the record count,
// the workgroups, and the parts (indices into the table) some BOX_MESH item reads, each once
struct ObjectOverlayPlan {
    std::vector<ObjectRow> rows; std::vector<const OverlayBounds*> bounds; std::vector<uint32_t> bound_parts;
    uint64_t total = 0, groups = 0;
};
// The argument rules (0: fine, B32_E_ARG, B32_E_UNSUPPORTED past 2^31 - 1 records) and the layout.  with_rows == false: count only (no view
// needs pointers).  Nothing is read through a view's pointers.
static inline int object_overlay_plan(const B32ObjectPart* parts, const ObjectPartView* views, uint32_t n_parts, const B32ObjectItem* items,
                                      uint32_t n_items, bool with_rows, ObjectOverlayPlan& plan) {
    plan.rows.clear(); plan.bounds.clear(); plan.bound_parts.clear(); plan.total = 0; plan.groups = 0;
    if ((n_parts && (!parts || !views)) || (n_items && !items)) return B32_E_ARG;
    for (uint32_t p = 0; p < n_parts; ++p)
        if (!parts[p].slot || !views[p].holds_scene || (parts[p].flags & ~B32_OBJECT_PART_HIDDEN) || parts[p]._pad) return B32_E_ARG;
    std::vector<uint8_t> listed(with_rows ? n_parts : 0u, 0);
    for (uint32_t i = 0; i < n_items; ++i) {
        const B32ObjectItem& it = items[i];
        if (it.kind > B32_OBJECT_BOX || it._pad[0] || it._pad[1] || it._pad[2]) return B32_E_ARG;
        if (it.first_part > n_parts || it.n_parts > n_parts - it.first_part) return B32_E_ARG;
        ObjectRow r{};
        r.kind = it.kind; r.place = it.place;
        r.r = it.r; r.g = it.g; r.b = it.b; r.blend = it.blend;
        if (it.kind == B32_OBJECT_WIRE) {
            for (uint32_t p = it.first_part; p < it.first_part + it.n_parts; ++p) {
                if (parts[p].flags & B32_OBJECT_PART_HIDDEN) continue;
                if (!views[p].has_topology) return B32_E_ARG;
                const uint32_t nh = views[p].nh;
                if (!nh) continue;
                if (with_rows) {
                    r.he = views[p].he; r.pos = views[p].pos; r.nh = nh; r.nv = views[p].nv; r.stride = views[p].stride;
                    r.first_rec = (uint32_t)plan.total; r.first_wg = (uint32_t)plan.groups;
                    plan.rows.push_back(r);
                }
                plan.total += nh;
                plan.groups += ((uint64_t)nh + OBJECT_LANES - 1u) / OBJECT_LANES;
                if (plan.total > 0x7FFFFFFFull) return B32_E_UNSUPPORTED;
            }
            continue;
        }
        if (with_rows) {
            if (it.kind == B32_OBJECT_BOX_MESH) {
                r.first_bound = (uint32_t)plan.bounds.size(); r.n_bounds = it.n_parts;
                for (uint32_t p = it.first_part; p < it.first_part + it.n_parts; ++p) {
                    if (views[p].nv) r.kind |= OBJECT_HAS_VERTS;
                    plan.bounds.push_back(views[p].bounds);
                    if (!listed[p]) { listed[p] = 1; plan.bound_parts.push_back(p); }
                }
            } else {
                for (int c = 0; c < 3; ++c) { r.box_min[c] = it.box_min[c]; r.box_max[c] = it.box_max[c]; }
            }
            r.first_rec = (uint32_t)plan.total; r.first_wg = (uint32_t)plan.groups;
            plan.rows.push_back(r);
        }
        plan.total += OBJECT_BOX_SLOTS;
        plan.groups += 1u;
        if (plan.total > 0x7FFFFFFFull) return B32_E_UNSUPPORTED;
    }
    return B32_OK;
}
// the row that workgroup `wg` serves: the last one whose first workgroup is not behind it (rows have at least one workgroup each, so
// first_wg rises strictly)
B32_HD uint32_t object_row_of(const ObjectRow* rows, uint32_t n_rows, uint32_t wg) {
    uint32_t lo = 0u, hi = n_rows;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (rows[mid].first_wg <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace b32
