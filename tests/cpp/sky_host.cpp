// The console loop with a sky through the C++ host mirror (b32::Sky, b32::FrameSky, b32::FrameLoop::submit(.., &sky)):
//   sky_host <out.rgba> <sky.bin> <scene.b32scene>
// sky.bin: uint32 nv, nf, n_stars, n_frames; float size; nv B32SkyVertex (the offsets); nf x 3 uint32; n_stars B32Star; n_frames x 12
// floats (a camera per frame: position, basis_x, basis_y, basis_z).  The scene file gives the framebuffer, the clear colour, the
// settings and one mesh.  Every frame is clear -> sky -> stars -> mesh -> delivered by ticket, the presenter one frame behind; the
// delivered frames are written one after another.
#include <cstdio>
#include <fstream>
#include <vector>

#include "scenefile.hpp"

template <class T>
static bool read_n(std::ifstream& in, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || (bool)in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: sky_host OUT SKY SCENE\n"); return 2; }
    try {
        std::ifstream in(argv[2], std::ios::binary);
        uint32_t head[4]; float size = 0.0f;
        if (!in.read(reinterpret_cast<char*>(head), sizeof(head)) || !in.read(reinterpret_cast<char*>(&size), sizeof(size))) return 3;
        std::vector<B32SkyVertex> offsets; std::vector<uint32_t> faces; std::vector<B32Star> stars; std::vector<float> cams;
        if (!read_n(in, offsets, head[0]) || !read_n(in, faces, (size_t)head[1] * 3) || !read_n(in, stars, head[2]) || !read_n(in, cams, (size_t)head[3] * 12)) return 3;
        const b32::SceneFile sc = b32::read_scene(argv[3]);
        b32::Framebuffer fb(sc.width, sc.height);
        b32::ResidentMesh mesh(fb, sc.vertices, sc.faces, sc.textures);
        const std::vector<std::pair<const b32::ResidentMesh*, b32::MeshParams>> frame{ { &mesh, b32::MeshParams{ sc.settings.ambient, sc.settings.backface_cull, false, sc.fog } } };
        b32::RasterSettings base = sc.settings;
        base.backface_wireframe = false;
        b32::Sky sky(fb, offsets, faces);
        b32::FrameSky fs; fs.sky = &sky; fs.stars = stars; fs.size = size;
        std::ofstream out(argv[1], std::ios::binary);
        const size_t bytes = (size_t)sc.width * sc.height * 4;
        unsigned presented = 0;
        {
            b32::FrameLoop loop(fb);
            uint64_t prev = 0;
            for (uint32_t i = 0; i < head[3]; ++i) {
                const float* c = &cams[(size_t)i * 12];
                const b32::Camera cam{ { c[0], c[1], c[2] }, { c[3], c[4], c[5] }, { c[6], c[7], c[8] }, { c[9], c[10], c[11] } };
                const uint64_t t = loop.submit(sc.clear, frame, cam, base, nullptr, nullptr, &fs);
                if (prev) { out.write(reinterpret_cast<const char*>(loop.wait(prev)), (std::streamsize)bytes); ++presented; }
                prev = t;
            }
            if (prev) { out.write(reinterpret_cast<const char*>(loop.wait(prev)), (std::streamsize)bytes); ++presented; }
            loop.finish();
        }
        std::printf("presented_frames %u\n", presented);
    } catch (const b32::Error& e) {
        std::fprintf(stderr, "b32::Error %d: %s\n", e.code, e.what());
        return 10;
    }
    return 0;
}
