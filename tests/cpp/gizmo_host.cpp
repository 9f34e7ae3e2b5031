// gizmo_host.cpp -- csrc/b32_gizmo_body.h (the device code of b32_draw_gizmos' arithmetic) compiled for the host, for
// tests/test_gizmos.py.  No device, no library.
//   usage: gizmo_host <in> <out>
//   in : u32 width, height, has_ortho, n; 12 f32 camera (position, basis_x, basis_y, basis_z); 3 f32 ortho (zoom, center_x, center_y);
//        n B32GizmoItem
//   out: u32 n_records, n_span_rows; u64 drawn, dropped, rejected; n u32 (0 drawn, 1 dropped, 2 rejected); n_records B32Prim;
//        n_span_rows x 4 i32 (record index, y, x_start, x_end) -- every row of every triangle record that is not skipped, rows
//        y0.max(0) ..= y2.min(h - 1), x_start = (ax as i32).max(0), x_end = (bx as i32).min(w - 1) (x_start > x_end: an empty row)
#include <cstdio>
#include <vector>

#include "b32_gizmo_body.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t head[4]; B32Camera cam; B32Ortho ortho;
    if (std::fread(head, 4, 4, in) != 4 || std::fread(&cam, 4, 12, in) != 12 || std::fread(&ortho, 4, 3, in) != 3) return 3;
    const uint32_t w = head[0], h = head[1], n = head[3];
    std::vector<B32GizmoItem> items(n);
    if (n && std::fread(items.data(), sizeof(B32GizmoItem), n, in) != n) return 3;
    std::fclose(in);
    b32::ViewBlock a;
    b32::view_fill(a, cam, w, h, head[2] ? &ortho : nullptr);

    std::vector<B32Prim> recs;
    std::vector<uint32_t> which(n);
    unsigned long long counts[3] = { 0, 0, 0 };
    for (uint32_t i = 0; i < n; ++i) {
        const size_t first = recs.size();
        recs.resize(first + b32::gizmo_record_count(items[i].kind, items[i].size));
        which[i] = b32::gizmo_item(a, items[i], recs.data() + first);
        ++counts[which[i]];
    }
    std::vector<int32_t> spans;
    for (size_t r = 0; r < recs.size(); ++r) {
        const B32Prim& p = recs[r];
        if (p.kind != b32::PRIM_TRIANGLE) continue;
        int32_t x[3] = { p.x0, p.x1, (int32_t)b32::f32_bits(p.z0) }, y[3] = { p.y0, p.y1, (int32_t)b32::f32_bits(p.z1) };
        b32::gizmo_tri_sort(x, y);
        if (y[2] == y[0]) continue;
        const int32_t ya = y[0] > 0 ? y[0] : 0, yb = y[2] < (int32_t)h - 1 ? y[2] : (int32_t)h - 1;
        for (int32_t yy = ya; yy <= yb; ++yy) {
            int32_t xa, xb;
            if (!b32::gizmo_tri_row(x[0], y[0], x[1], y[1], x[2], y[2], yy, xa, xb)) continue;
            spans.push_back((int32_t)r); spans.push_back(yy);
            spans.push_back(xa > 0 ? xa : 0); spans.push_back(xb < (int32_t)w - 1 ? xb : (int32_t)w - 1);
        }
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    const uint32_t oh[2] = { (uint32_t)recs.size(), (uint32_t)(spans.size() / 4) };
    std::fwrite(oh, 4, 2, out); std::fwrite(counts, 8, 3, out);
    if (n) std::fwrite(which.data(), 4, n, out);
    if (!recs.empty()) std::fwrite(recs.data(), sizeof(B32Prim), recs.size(), out);
    if (!spans.empty()) std::fwrite(spans.data(), 4, spans.size(), out);
    std::fclose(out);
    return 0;
}
