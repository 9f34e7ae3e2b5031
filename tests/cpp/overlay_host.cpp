// overlay_host.cpp -- csrc/b32_overlay_body.h (the device code of b32_draw_mesh_overlay's arithmetic) compiled for the host, for
// tests/test_mesh_overlay.py.  No device, no library.  Every element goes through the function its lane calls, into the place
// overlay_layout gives it; the bounds are reduced through the same keys.
//   usage: overlay_host <in> <out>
//   in : u32 width, height, has_ortho, nv, np, nh, n_sel_words; B32MeshOverlay; 12 f32 camera (position, basis_x, basis_y, basis_z);
//        3 f32 ortho (zoom, center_x, center_y); nv x 3 f32 positions; np + 1 u32 poly_start; nh u32 poly_verts; n_sel_words u32 selected
//   out: 9 u32 (first record of brackets, edges, dots, hover vertex, hover edge, hover face, selected, preview; total); total B32Prim
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "b32_overlay_body.h"

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return !n || std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    using namespace b32;
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t head[7]; B32MeshOverlay o; B32Camera cam; B32Ortho ortho;
    if (std::fread(head, 4, 7, in) != 7 || std::fread(&o, sizeof o, 1, in) != 1 || std::fread(&cam, 4, 12, in) != 12 || std::fread(&ortho, 4, 3, in) != 3) return 3;
    const uint32_t w = head[0], h = head[1], nv = head[3], np = head[4], nh = head[5], nsel = head[6];
    std::vector<float> pos; std::vector<uint32_t> ps, pv, sel;
    if (!get(in, pos, (size_t)nv * 3) || !get(in, ps, (size_t)np + 1) || !get(in, pv, nh) || !get(in, sel, nsel)) return 3;
    std::fclose(in);
    ViewBlock a;
    view_fill(a, cam, w, h, head[2] ? &ortho : nullptr);
    if (overlay_check(true, &o, sel.data())) return 5;

    // the half-edges as b32_topology_create derives them
    struct HE { uint32_t v0, v1, edge, first; };
    std::vector<HE> he(nh);
    std::vector<std::pair<unsigned long long, uint32_t>> keys(nh);
    for (uint32_t p = 0; p < np; ++p) {
        const uint32_t s = ps[p], n = ps[p + 1] - s;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t v0 = pv[s + k], v1 = pv[s + (k + 1u) % n];
            he[s + k] = HE{ v0, v1, 0u, 0u };
            keys[s + k] = { ((unsigned long long)std::min(v0, v1) << 32) | std::max(v0, v1), s + k };
        }
    }
    std::sort(keys.begin(), keys.end());
    uint32_t ne = 0;
    for (uint32_t j = 0; j < nh; ++j) { if (j && keys[j].first != keys[j - 1].first) ++ne; he[keys[j].second].edge = ne; }
    if (nh) ++ne;
    { std::vector<uint8_t> seen(ne, 0); uint32_t rank = 0; for (uint32_t j = 0; j < nh; ++j) if (!seen[he[j].edge]) { seen[he[j].edge] = 1; he[j].first = ++rank; } }

    const OverlayLayout l = overlay_layout(ps.data(), np, nh, ne, nv, o, sel.data());
    std::vector<B32Prim> out((size_t)l.total);
    const float rect[4] = { o.x0, o.y0, o.x1, o.y1 };
    const uint32_t sec = o.sections;

    // k_overlay_points
    std::vector<OverlayPoint> tab(nv);
    OverlayBounds b = overlay_bounds_start();
    for (uint32_t i = 0; i < nv; ++i) {
        const float* p = pos.data() + (size_t)i * 3;
        tab[i] = overlay_point(a, p);
        if (sec & B32_OVERLAY_DOTS) out[l.dots + i] = overlay_dot(tab[i]);
        if ((sec & B32_OVERLAY_PREVIEW) && o.preview_mode == 0u) out[l.preview + i] = overlay_preview_vertex(tab[i], rect);
        if (sec & B32_OVERLAY_BRACKETS) overlay_bounds_take(b, p);
    }
    // k_overlay_emit
    if (sec & B32_OVERLAY_EDGES) for (uint32_t j = 0; j < nh; ++j) out[l.edges + j] = overlay_edge(he[j].v0, he[j].v1, nv, tab.data());
    if ((sec & B32_OVERLAY_PREVIEW) && o.preview_mode == 1u)
        for (uint32_t j = 0; j < nh; ++j) if (he[j].first) overlay_preview_edge(he[j].v0, he[j].v1, nv, tab.data(), rect, out.data() + l.preview + 2u * (he[j].first - 1u));
    if ((sec & B32_OVERLAY_SELECTED) && o.n_selected) {
        uint64_t at = l.selected;
        for (uint32_t i = 0; i < o.n_selected; ++i) {
            if (o.select_kind == 1u) out[l.selected + i] = overlay_selected_vertex(sel[i], nv, tab.data());
            else if (o.select_kind == 2u) overlay_selected_edge(sel[2 * i], sel[2 * i + 1], nv, tab.data(), out.data() + l.selected + 4u * i);
            else if (o.select_kind == 3u && sel[i] < np) {
                const uint32_t s = ps[sel[i]], n = ps[sel[i] + 1] - s;
                overlay_polygon(a, OVERLAY_POLY_SELECTED, pv.data() + s, n, pos.data(), 3u, nv, tab.data(), rect, out.data() + at);
                at += overlay_polygon_slots(OVERLAY_POLY_SELECTED, n);
            }
        }
    }
    if ((sec & B32_OVERLAY_PREVIEW) && o.preview_mode == 2u)
        for (uint32_t p = 0; p < np; ++p)
            overlay_polygon(a, OVERLAY_POLY_PREVIEW, pv.data() + ps[p], ps[p + 1] - ps[p], pos.data(), 3u, nv, tab.data(), rect, out.data() + l.preview + ps[p] + p);
    if (sec & B32_OVERLAY_HOVER) {
        if (o.hover_vertex != OVERLAY_NONE) out[l.hover_vertex] = overlay_hover_vertex(o.hover_vertex, nv, tab.data());
        if (o.hover_edge_v0 != OVERLAY_NONE || o.hover_edge_v1 != OVERLAY_NONE) overlay_hover_edge(o.hover_edge_v0, o.hover_edge_v1, nv, tab.data(), out.data() + l.hover_edge);
        if (l.hover_face_cnt)
            overlay_polygon(a, OVERLAY_POLY_HOVER, pv.data() + ps[o.hover_face], l.hover_face_cnt, pos.data(), 3u, nv, tab.data(), rect, out.data() + l.hover_face);
    }
    if ((sec & B32_OVERLAY_BRACKETS) && nv) for (uint32_t k = 0; k < 24u; ++k) out[l.brackets + k] = overlay_bracket(a, b, k);

    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const uint32_t lay[9] = { (uint32_t)l.brackets, (uint32_t)l.edges, (uint32_t)l.dots, (uint32_t)l.hover_vertex, (uint32_t)l.hover_edge,
                              (uint32_t)l.hover_face, (uint32_t)l.selected, (uint32_t)l.preview, (uint32_t)l.total };
    std::fwrite(lay, 4, 9, f);
    if (!out.empty()) std::fwrite(out.data(), sizeof(B32Prim), out.size(), f);
    std::fclose(f);
    return 0;
}
