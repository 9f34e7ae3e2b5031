// b32_patch_body.h -- what ONE lane of the in-place edits of a resident scene does (b32_scene_patch_vertices / _faces / _texels /
// _indexed; the kernels and the host side are in b32_patch.hip).  The reference edits a mesh on the host every frame while the user drags
// -- positions (modeler/viewport.rs:95, :373), uv (modeler/layout.rs:3732-3902), editor_alpha (viewport.rs:1295), face flags, atlas indices
// (modeler/mesh_editor.rs:647) and CLUT entries (texture/user_texture.rs:337) -- and hands the whole mesh to the rasterizer again.  Here the
// mesh stays resident and a record per edited element is scattered into it.  The text also compiles for the host (B32_HD,
// b32_pose_body.h), where tests/test_scene_patch.py drives it lane by lane against the Python mirrors.
#pragma once
#include "b32_pose_body.h"
#include <string.h>

namespace b32 {

constexpr uint32_t PATCH_VERTEX_WORDS = 10;     // B32VertexPatch: index, then the 9 dwords of a B32Vertex
constexpr uint32_t PATCH_FACE_WORDS = 6;        // B32FacePatch: index, then the 5 dwords of a B32Face
constexpr uint32_t PATCH_CLUT_ENTRIES = 256;    // the CLUT in front of a staged index rectangle: 256 Color15, zero behind the palette

B32_HD float patch_as_float(uint32_t u) {
#if defined(__HIPCC__)
    return __uint_as_float(u);
#else
    float f; memcpy(&f, &u, 4); return f;
#endif
}
B32_HD uint32_t patch_as_bits(float f) {
#if defined(__HIPCC__)
    return __float_as_uint(f);
#else
    uint32_t u; memcpy(&u, &f, 4); return u;
#endif
}

// The bone a vertex is posed with: none for an index at or past the table (B32_BONE_NONE included), as in k_pose.
B32_HD bool patch_has_bone(uint32_t bone_of, uint32_t n_bones) { return bone_of < n_bones; }

// One vertex record.  The whole B32Vertex is written, as whole dwords.  rest == nullptr: a slot without a rig, the record is the vertex.
// Else the record is in REST space: position and normal go into the rest stream (6 dwords per vertex) and the vertex gets them posed by
// `bone` (nullptr: the rest bits, bone_transforms.get(idx) == None) with pose_vertex, the pose pass's own function.
B32_HD void patch_vertex(const uint32_t* rec, uint32_t* verts, uint32_t* rest, const B32Bone* bone) {
    const uint32_t i = rec[0];
    uint32_t w[9];
    for (int k = 0; k < 9; ++k) w[k] = rec[1 + k];
    if (rest) {
        uint32_t* r = rest + (size_t)i * 6;
        r[0] = w[0]; r[1] = w[1]; r[2] = w[2]; r[3] = w[5]; r[4] = w[6]; r[5] = w[7];
        if (bone) {
            float in[6], out[6];
            in[0] = patch_as_float(w[0]); in[1] = patch_as_float(w[1]); in[2] = patch_as_float(w[2]);
            in[3] = patch_as_float(w[5]); in[4] = patch_as_float(w[6]); in[5] = patch_as_float(w[7]);
            pose_vertex(bone, in, out);
            w[0] = patch_as_bits(out[0]); w[1] = patch_as_bits(out[1]); w[2] = patch_as_bits(out[2]);
            w[5] = patch_as_bits(out[3]); w[6] = patch_as_bits(out[4]); w[7] = patch_as_bits(out[5]);
        }
    }
    uint32_t* v = verts + (size_t)i * 9;
    for (int k = 0; k < 9; ++k) v[k] = w[k];
}

// One face record: the whole B32Face, padding byte included, as a fresh upload copies it.
B32_HD void patch_face(const uint32_t* rec, uint32_t* faces) {
    uint32_t* f = faces + (size_t)rec[0] * 5;
    for (int k = 0; k < 5; ++k) f[k] = rec[1 + k];
}

// A rectangle [x, x + w) x [y, y + h) of a texture tex_w texels wide whose first texel is texel `offset` of the pool.  Lane t owns texel
// (x + t % w, y + t / w): adjacent lanes write adjacent texels of one row.  The staged source is packed, w elements per row.  Only
// texels inside the rectangle are written, so the pool's padding behind a texture and the next texture's first texel are never touched.
struct PatchRect { uint32_t x, y, w, h, tex_w, offset; };
B32_HD uint32_t patch_texel_in_texture(const PatchRect& r, uint32_t t) {
    const uint32_t row = t / r.w, col = t - row * r.w;
    return (r.y + row) * r.tex_w + r.x + col;
}
template <class Texel>
B32_HD void patch_texel(const PatchRect& r, uint32_t t, const Texel* src, Texel* pool) {
    pool[r.offset + patch_texel_in_texture(r, t)] = src[t];
}
// Clut::lookup (types.rs:390-397): an index past the palette is 0x0000
B32_HD uint16_t patch_lookup(const uint16_t* clut, uint32_t clut_len, uint32_t index) { return index < clut_len ? clut[index] : (uint16_t)0; }
// ... expanded into the pool; kept_idx != nullptr: the slot keeps its index atlas (one texture), which gets the index byte too
B32_HD void patch_indexed_texel(const PatchRect& r, uint32_t t, const uint8_t* idx, const uint16_t* clut, uint32_t clut_len, uint16_t* pool, uint8_t* kept_idx) {
    const uint32_t at = patch_texel_in_texture(r, t);
    const uint32_t k = idx[t];
    pool[r.offset + at] = patch_lookup(clut, clut_len, k);
    if (kept_idx) kept_idx[at] = (uint8_t)k;
}
// entry t < PATCH_CLUT_ENTRIES of the kept CLUT on a whole-texture patch: zero behind a shorter palette, as the upload leaves it
B32_HD void patch_kept_clut(uint32_t t, const uint16_t* clut, uint32_t clut_len, uint16_t* kept) { kept[t] = patch_lookup(clut, clut_len, t); }

// host only: the caller's rectangle (rows `stride` elements apart) packed to w elements per row on its way into the pinned ring
static inline void patch_pack_rect(const void* src, uint32_t stride, uint32_t w, uint32_t h, uint32_t elem_bytes, void* dst) {
    for (uint32_t row = 0; row < h; ++row)
        memcpy(static_cast<unsigned char*>(dst) + (size_t)row * w * elem_bytes, static_cast<const unsigned char*>(src) + (size_t)row * stride * elem_bytes, (size_t)w * elem_bytes);
}

}  // namespace b32
