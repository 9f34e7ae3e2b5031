// csrc/b32_mirror_body.h built for the host: the mirror-editing mesh of b32_scene_build_mirror, output by output, exactly as one lane of
// k_mirror_mesh computes it (tests/test_mirror.py drives it; also built with -fsanitize=address,undefined).
//   mirror_host IN OUT   IN:  uint32 bv, bf, rigged, n_bones; B32Mirror; bv B32Vertex; bf B32Face; rigged: bv x 6 floats (the rest stream), bv
//                             uint16 bone indices (padded to a multiple of 4 bytes), n_bones B32Bone
//                        OUT: int32 rc of the argument rules; rc == 0: uint32 nv_out, nf_out, the vertices, the faces
//   mirror_host          no arguments: the argument rules and the source mapping at counts a buffer could not hold, up to 2^32 - 1
#include "b32_mirror_body.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace b32;

static bool read_all(const char* path, std::vector<unsigned char>& blob) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    blob.resize((size_t)n);
    const bool ok = n == 0 || fread(blob.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "mirror_host: %s failed (line %d)\n", #cond, __LINE__); return 1; } } while (0)

static B32Mirror mk(uint32_t axis, uint32_t v0, uint32_t vc, uint32_t f0, uint32_t fc) {
    B32Mirror m{};
    m.axis = axis; m.dim = B32_MIRROR_DIM; m.v_first = v0; m.v_count = vc; m.f_first = f0; m.f_count = fc;
    return m;
}

static int self_check() {
    const uint32_t MAXU = 0xFFFFFFFFu;
    uint32_t nv = 7, nf = 7;
    B32Mirror m = mk(1, 0, 0, 0, 0);
    EXPECT(mirror_counts(0, 0, &m, &nv, &nf) == B32_OK && nv == 0 && nf == 0);
    EXPECT(mirror_counts(5, 5, nullptr, &nv, &nf) == B32_E_ARG);
    m = mk(0, 0, 0, 0, 0); EXPECT(mirror_counts(5, 5, &m, &nv, &nf) == B32_E_ARG);
    m = mk(4, 0, 0, 0, 0); EXPECT(mirror_counts(5, 5, &m, &nv, &nf) == B32_E_ARG);
    m = mk(3, 2, 4, 0, 0); EXPECT(mirror_counts(5, 5, &m, &nv, &nf) == B32_E_ARG);
    m = mk(3, 2, 3, 1, 5); EXPECT(mirror_counts(5, 5, &m, &nv, &nf) == B32_E_ARG);
    m = mk(3, MAXU, 2, 0, 0); EXPECT(mirror_counts(MAXU, 5, &m, &nv, &nf) == B32_E_ARG);          // (the sum wraps in 32 bits)
    m = mk(2, 2, 3, 1, 4); EXPECT(mirror_counts(5, 5, &m, &nv, &nf) == B32_OK && nv == 8 && nf == 9);
    EXPECT(mirror_counts(5, 5, &m, nullptr, nullptr) == B32_OK);
    EXPECT(nv == 8 && nf == 9);
    // counts past 2^32 - 1
    m = mk(1, MAXU - 1, 1, 0, 0); EXPECT(mirror_counts(MAXU, 0, &m, &nv, &nf) == B32_E_UNSUPPORTED && nv == 8 && nf == 9);
    m = mk(1, 0, 0, 0, 1); EXPECT(mirror_counts(0, MAXU, &m, &nv, &nf) == B32_E_UNSUPPORTED);
    m = mk(1, 0, 0x80000000u, 0, 0x80000000u); EXPECT(mirror_counts(0x80000000u, 0x80000000u, &m, &nv, &nf) == B32_E_UNSUPPORTED);
    m = mk(1, 0, 0x7FFFFFFFu, 0, 0x7FFFFFFFu);    // (one vertex and one face behind the ranges: the last outputs, 2^32 - 2, are shifted ones)
    EXPECT(mirror_counts(0x80000000u, 0x80000000u, &m, &nv, &nf) == B32_OK && nv == MAXU && nf == MAXU);
    // the mapping at those counts: every output has a source inside the body, at the seams of the three regions
    {
        const uint32_t bv = 0x80000000u, c = m.v_count, v_end = m.v_first + c;
        const uint32_t probes[] = { 0u, 1u, v_end - 1u, v_end, v_end + 1u, v_end + c - 1u, v_end + c, MAXU - 1u };
        for (uint32_t i : probes) {
            bool twin;
            const uint32_t s = mirror_vertex_source(m, i, twin);
            EXPECT(s < bv);
            EXPECT(twin == (i >= v_end && i < v_end + c));
            EXPECT(s == (i < v_end ? i : i - c));
        }
        const uint32_t bf = 0x80000000u, f0 = m.f_first, fc = m.f_count;
        const uint32_t fprobes[] = { 0u, f0, f0 + 1u, f0 + 2u, f0 + 2u * fc - 2u, f0 + 2u * fc - 1u, f0 + 2u * fc, MAXU - 1u };
        for (uint32_t j : fprobes) {
            uint32_t kind;
            const uint32_t s = mirror_face_source(m, j, kind);
            EXPECT(s < bf);
            if (j < f0) EXPECT(kind == MIRROR_FACE_COPY && s == j);
            else if (j < f0 + 2u * fc) EXPECT(s == f0 + (j - f0) / 2u && kind == (((j - f0) & 1u) ? MIRROR_FACE_TWIN : MIRROR_FACE_COPY));
            else EXPECT(kind == MIRROR_FACE_SHIFTED && s == j - fc);
        }
    }
    // the wrap of a twin's indices
    {
        const uint32_t src[5] = { MAXU, 1u, 0xFFFFFFF0u, 9u, 0x00FF0201u };
        uint32_t out[5];
        mirror_face(src, MIRROR_FACE_TWIN, 0x20u, out);
        EXPECT(out[0] == 0x1Fu && out[1] == 0x10u && out[2] == 0x21u && out[3] == 9u && out[4] == 0x00FF0201u);
        mirror_face(src, MIRROR_FACE_SHIFTED, 0x20u, out);
        EXPECT(out[0] == 0x1Fu && out[1] == 0x21u && out[2] == 0x10u);
        mirror_face(src, MIRROR_FACE_COPY, 0x20u, out);
        EXPECT(out[0] == MAXU && out[1] == 1u && out[2] == 0xFFFFFFF0u);
    }
    EXPECT(mirror_dim(180, B32_MIRROR_DIM) == 153 && mirror_dim(255, B32_MIRROR_DIM) == 216 && mirror_dim(1, B32_MIRROR_DIM) == 0);
    EXPECT(mirror_flip(0u) == 0x80000000u && mirror_flip(0x80000000u) == 0u && mirror_flip(0x7FC12345u) == 0xFFC12345u);
    printf("ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return self_check();
    if (argc != 3) { fprintf(stderr, "usage: mirror_host [IN OUT]\n"); return 2; }
    std::vector<unsigned char> blob;
    if (!read_all(argv[1], blob) || blob.size() < 16 + sizeof(B32Mirror)) return 2;
    uint32_t head[4];
    memcpy(head, blob.data(), 16);
    const uint32_t bv = head[0], bf = head[1], rigged = head[2], n_bones = head[3];
    B32Mirror m;
    memcpy(&m, blob.data() + 16, sizeof(m));
    size_t at = 16 + sizeof(m);
    std::vector<uint32_t> verts((size_t)bv * 9), faces((size_t)bf * 5), rest;
    std::vector<uint16_t> bone_of;
    std::vector<B32Bone> bones(n_bones);
    const size_t need = at + verts.size() * 4 + faces.size() * 4 + (rigged ? (size_t)bv * 24 + (((size_t)bv * 2 + 3) & ~(size_t)3) + (size_t)n_bones * sizeof(B32Bone) : 0);
    if (blob.size() != need || n_bones > B32_MAX_BONES) return 2;
    if (!verts.empty()) memcpy(verts.data(), blob.data() + at, verts.size() * 4);
    at += verts.size() * 4;
    if (!faces.empty()) memcpy(faces.data(), blob.data() + at, faces.size() * 4);
    at += faces.size() * 4;
    if (rigged) {
        rest.resize((size_t)bv * 6); bone_of.resize(bv);
        if (bv) memcpy(rest.data(), blob.data() + at, rest.size() * 4);
        at += rest.size() * 4;
        if (bv) memcpy(bone_of.data(), blob.data() + at, (size_t)bv * 2);
        at += ((size_t)bv * 2 + 3) & ~(size_t)3;
        if (n_bones) memcpy(bones.data(), blob.data() + at, (size_t)n_bones * sizeof(B32Bone));
    }
    uint32_t nv = 0, nf = 0;
    const int32_t rc = mirror_counts(bv, bf, &m, &nv, &nf);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(&rc, 4, 1, out);
    if (rc == B32_OK) {
        std::vector<uint32_t> ov((size_t)nv * 9), of((size_t)nf * 5);
        for (uint32_t t = 0; t < nv; ++t) {     // lane t of k_mirror_mesh, the vertex
            bool twin;
            const uint32_t s = mirror_vertex_source(m, t, twin);
            if (s >= bv) { fclose(out); return 3; }
            const uint32_t* w = verts.data() + (size_t)s * 9;
            uint32_t* d = ov.data() + (size_t)t * 9;
            if (!twin) { for (int k = 0; k < 9; ++k) d[k] = w[k]; continue; }
            uint32_t local[6] = { w[0], w[1], w[2], w[5], w[6], w[7] };
            const B32Bone* bone = nullptr;
            if (rigged) {
                for (int k = 0; k < 6; ++k) local[k] = rest[(size_t)s * 6 + k];
                if (bone_of[s] < n_bones) bone = &bones[bone_of[s]];
            }
            mirror_twin_vertex(w, local, m.axis, m.dim, bone, d);
        }
        for (uint32_t t = 0; t < nf; ++t) {     // ... and the face
            uint32_t kind;
            const uint32_t s = mirror_face_source(m, t, kind);
            if (s >= bf) { fclose(out); return 3; }
            mirror_face(faces.data() + (size_t)s * 5, kind, m.v_count, of.data() + (size_t)t * 5);
        }
        fwrite(&nv, 4, 1, out); fwrite(&nf, 4, 1, out);
        if (!ov.empty()) fwrite(ov.data(), 4, ov.size(), out);
        if (!of.empty()) fwrite(of.data(), 4, of.size(), out);
    }
    fclose(out);
    return 0;
}
