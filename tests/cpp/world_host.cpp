// world_host.cpp -- csrc/b32_world_body.h (the device code of b32_draw_world's arithmetic) compiled for the host, for
// tests/test_world.py.  No device, no library.
//   usage: world_host <in> <out>
//   in : u32 width, height, has_ortho, n; 12 f32 camera (position, basis_x, basis_y, basis_z); 3 f32 ortho (zoom, center_x, center_y);
//        n B32WorldItem
//   out: u64 drawn, dropped, rejected; n u32 (0 drawn, 1 dropped, 2 rejected); n B32Prim
#include <cstdio>
#include <vector>

#include "b32_world_body.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    uint32_t head[4]; B32Camera cam; B32Ortho ortho;
    if (std::fread(head, 4, 4, in) != 4 || std::fread(&cam, 4, 12, in) != 12 || std::fread(&ortho, 4, 3, in) != 3) return 3;
    const uint32_t w = head[0], h = head[1], n = head[3];
    std::vector<B32WorldItem> items(n);
    if (n && std::fread(items.data(), sizeof(B32WorldItem), n, in) != n) return 3;
    std::fclose(in);
    b32::ViewBlock a;
    b32::view_fill(a, cam, w, h, head[2] ? &ortho : nullptr);

    std::vector<B32Prim> recs(n);
    std::vector<uint32_t> which(n);
    unsigned long long counts[3] = { 0, 0, 0 };
    for (uint32_t i = 0; i < n; ++i) {
        which[i] = b32::world_item(a, items[i], &recs[i]);
        ++counts[which[i]];
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 4;
    std::fwrite(counts, 8, 3, out);
    if (n) { std::fwrite(which.data(), 4, n, out); std::fwrite(recs.data(), sizeof(B32Prim), n, out); }
    std::fclose(out);
    return 0;
}
