// b32_mirror_body.h -- the modeler's mirror editing for ONE output element: where an output vertex or face of the mirrored mesh comes from,
// and what a twin is (b32_scene_build_mirror; the kernel and the host side are in b32_mirror.hip).  Reference: with MirrorSettings enabled
// (modeler/state.rs:777-850) the draw appends, behind the selected object's nv vertices, nv twins -- mirrored in LOCAL space
// (mirror_position, mirror_normal), then put through the vertex's bone, colour (base_color as f32 * 0.85) as u8 -- and behind EACH of the
// object's triangles its twin with reversed winding (mirror_offset + v0, + v2, + v1); every later object's vertices shift by nv
// (modeler/viewport.rs:1209-1311).  The rule is positional: it never looks at an index value.  The text also compiles for the host (B32_HD,
// b32_pose_body.h), where tests/test_mirror.py and tests/cpp/mirror_host.cpp drive it output by output.  The bone arithmetic is
// pose_vertex's and is not restated.
#pragma once
#include "b32_pose_body.h"
#include <string.h>

namespace b32 {

constexpr uint32_t MIRROR_SIGN = 0x80000000u;

B32_HD float mirror_as_float(uint32_t u) {
#if defined(__HIPCC__)
    return __uint_as_float(u);
#else
    float f; memcpy(&f, &u, 4); return f;
#endif
}
B32_HD uint32_t mirror_as_bits(float f) {
#if defined(__HIPCC__)
    return __float_as_uint(f);
#else
    uint32_t u; memcpy(&u, &f, 4); return u;
#endif
}

// ---- the source of an output.  c = v_count twins stand behind the range's last vertex; the range's faces alternate with their twins.
// Output vertex i: source vertex and whether the output is that vertex's twin.
B32_HD uint32_t mirror_vertex_source(const B32Mirror& m, uint32_t i, bool& twin) {
    const uint32_t v_end = m.v_first + m.v_count;
    twin = i >= v_end && i - v_end < m.v_count;
    return i < v_end ? i : i - m.v_count;
}
// Output face j: source face and what becomes of it.
enum MirrorFaceKind : uint32_t { MIRROR_FACE_COPY = 0, MIRROR_FACE_TWIN = 1, MIRROR_FACE_SHIFTED = 2 };
B32_HD uint32_t mirror_face_source(const B32Mirror& m, uint32_t j, uint32_t& kind) {
    if (j < m.f_first) { kind = MIRROR_FACE_COPY; return j; }
    const uint32_t k = j - m.f_first;
    if ((k >> 1) < m.f_count) { kind = (k & 1u) ? MIRROR_FACE_TWIN : MIRROR_FACE_COPY; return m.f_first + (k >> 1); }
    kind = MIRROR_FACE_SHIFTED;
    return j - m.f_count;
}

// ---- a twin
// Rust's -x on the bits: -0.0 <-> +0.0, a NaN keeps its payload (not 0 - x)
B32_HD uint32_t mirror_flip(uint32_t bits) { return bits ^ MIRROR_SIGN; }
// (ch as f32 * dim) as u8: one f32 product, then Rust's saturating cast (NaN -> 0)
B32_HD uint32_t mirror_dim(uint32_t ch, float dim) {
    const float f = (float)ch * dim;
    if (!(f > 0.0f)) return 0u;
    if (f >= 255.0f) return 255u;
    return (uint32_t)f;
}
// The twin of the vertex whose 9 dwords are `src`.  local: its LOCAL position and normal as 6 dwords (the rest stream of a rigged slot,
// else words 0..2 and 5..7 of src).  bone == nullptr: bone_transforms.get(idx) == None, or a slot without a rig: the mirrored bits.
B32_HD void mirror_twin_vertex(const uint32_t* src, const uint32_t* local, uint32_t axis, float dim, const B32Bone* bone, uint32_t* out) {
    uint32_t l[6];
    for (int k = 0; k < 6; ++k) l[k] = local[k];
    const uint32_t a = axis - 1u;               // (1 X, 2 Y, 3 Z: validated by the host)
    for (uint32_t k = 0; k < 3u; ++k)
        if (k == a) { l[k] = mirror_flip(l[k]); l[3 + k] = mirror_flip(l[3 + k]); }
    if (bone) {
        float in[6], posed[6];
        for (int k = 0; k < 6; ++k) in[k] = mirror_as_float(l[k]);
        pose_vertex(bone, in, posed);
        for (int k = 0; k < 6; ++k) l[k] = mirror_as_bits(posed[k]);
    }
    out[0] = l[0]; out[1] = l[1]; out[2] = l[2];
    out[3] = src[3]; out[4] = src[4];
    out[5] = l[3]; out[6] = l[4]; out[7] = l[5];
    const uint32_t rgba = src[8];               // r | g << 8 | b << 16 | blend << 24; Color::new sets BlendMode::Opaque (types.rs:773-775)
    out[8] = mirror_dim(rgba & 255u, dim) | (mirror_dim((rgba >> 8) & 255u, dim) << 8) | (mirror_dim((rgba >> 16) & 255u, dim) << 16) |
             ((uint32_t)B32_BLEND_OPAQUE << 24);
}
// Output face of `kind` from the 5 dwords of its source: indices by wrapping u32 adds of c = v_count, the other eight bytes copied.
B32_HD void mirror_face(const uint32_t* src, uint32_t kind, uint32_t c, uint32_t* out) {
    const uint32_t add = kind == MIRROR_FACE_COPY ? 0u : c;
    const bool swap = kind == MIRROR_FACE_TWIN;
    out[0] = src[0] + add;
    out[1] = (swap ? src[2] : src[1]) + add;
    out[2] = (swap ? src[1] : src[2]) + add;
    out[3] = src[3]; out[4] = src[4];
}

// ---- host only: the argument rules of b32_scene_build_mirror / b32_mirror_counts for a body of nv vertices and nf faces
static inline int mirror_counts(uint32_t nv, uint32_t nf, const B32Mirror* m, uint32_t* nv_out, uint32_t* nf_out) {
    if (!m || m->axis < 1u || m->axis > 3u) return B32_E_ARG;
    if ((uint64_t)m->v_first + m->v_count > nv || (uint64_t)m->f_first + m->f_count > nf) return B32_E_ARG;
    const uint64_t v = (uint64_t)nv + m->v_count, f = (uint64_t)nf + m->f_count;
    if (v > 0xFFFFFFFFull || f > 0xFFFFFFFFull) return B32_E_UNSUPPORTED;
    if (nv_out) *nv_out = (uint32_t)v;
    if (nf_out) *nf_out = (uint32_t)f;
    return B32_OK;
}

}  // namespace b32
