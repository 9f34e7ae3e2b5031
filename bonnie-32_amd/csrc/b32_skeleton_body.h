// b32_skeleton_body.h -- the modeler's bone octahedra (modeler/skeleton.rs:412-477 skeleton_to_triangles, :534-562
// skeleton_to_triangles_from_bones, :565-660 generate_bone_octahedron, :257-270 compute_perpendicular_axes) and the tip of a bone
// (modeler/state.rs:2629-2638 get_bone_tip_position) for ONE bone: its tip, whether it is drawn, its colour and alpha, and the 6 vertices
// and 8 faces of its octahedron.  k_skeleton_mesh (b32_skeleton.hip) writes one vertex or face per lane; the host side of
// b32_scene_build_skeleton, b32_skeleton_counts and b32_skeleton_items run the tip, the liveness and the colour rule from this same text
// (SKEL_HD is host and device under hipcc).  The text also compiles without hipcc, where tests/cpp/skeleton_host.cpp drives it bone by
// bone against a literal restatement, built with and without -ffp-contract=off.  Every expression is a separately rounded f32 operation
// in the reference's order; libm stays with the caller (B32SkelBone carries cos / sin, as B32Bone and B32Placement do).
// One departure from the reference's bits, the room mesh's: a float of a vertex that is a NaN is written as 0x7FC00000 (skel_canon).
#pragma once
#if defined(__HIPCC__)
#include "b32_device.h"
#define SKEL_HD __host__ __device__ __forceinline__
#else
#include <stdint.h>
#include "../../include/b32raster.h"
#define SKEL_HD static inline
#endif

namespace b32 {

// the literals of the reference (tests/golden/skeleton_constants.json has them as data, taken from its text)
constexpr float SKEL_DEGENERATE = 0.001f;       // skeleton.rs:577  length < 0.001: no octahedron
constexpr float SKEL_UP_LIMIT = 0.9f;           // skeleton.rs:259  dir.y.abs() < 0.9: up = +Y, else +X
constexpr float SKEL_RING_AT = 0.2f;            // skeleton.rs:590  the ring sits 20 % along the bone
constexpr float SKEL_DEFAULT_WIDTH = 40.0f;     // state.rs:343     RigBone::DEFAULT_WIDTH (the creation preview's width)
constexpr uint32_t SKEL_DIM_ALPHA = 30u;        // skeleton.rs:432  non-selected bones while a bone is selected
constexpr uint32_t SKEL_MAX_OCTS = B32_MAX_BONES + 1u;      // every bone and the creation preview
constexpr uint32_t SKEL_OCT_VERTS = 6u, SKEL_OCT_FACES = 8u, SKEL_OCT_ELEMS = 14u;

// bone colours, skeleton.rs:13-39, as r | g << 8 | b << 16
enum SkelColour : uint32_t { SKEL_COL_DEFAULT = 0, SKEL_COL_SELECTED, SKEL_COL_HOVERED, SKEL_COL_TIP_HOVERED, SKEL_COL_ROOT, SKEL_COL_CREATING, SKEL_COL_HIERARCHY_LINE };
SKEL_HD uint32_t skel_colour(uint32_t which) {
    switch (which) {
        case SKEL_COL_SELECTED: return 80u | 255u << 8 | 80u << 16;
        case SKEL_COL_HOVERED: return 100u | 180u << 8 | 255u << 16;
        case SKEL_COL_TIP_HOVERED: return 255u | 180u << 8 | 80u << 16;
        case SKEL_COL_ROOT: return 255u | 220u << 8 | 100u << 16;
        case SKEL_COL_CREATING: return 255u | 150u << 8 | 50u << 16;
        case SKEL_COL_HIERARCHY_LINE: return 100u | 100u << 8 | 100u << 16;
        default: return 200u | 200u << 8 | 200u << 16;
    }
}

// One octahedron as the kernel takes it: generate_bone_octahedron's arguments.  32 bytes.
struct SkelOct { float base[3]; float tip[3]; float width; uint8_t r, g, b, alpha; };
static_assert(sizeof(SkelOct) == 32 && sizeof(B32SkelBone) == 40 && sizeof(B32SkeletonStyle) == 44, "SkelOct / B32SkelBone / B32SkeletonStyle layout");

SKEL_HD float skel_sqrt(float x) { return __builtin_sqrtf(x); }
SKEL_HD float skel_canon(float x) { return x != x ? __builtin_nanf("") : x; }
// Vec3::len, math.rs:23-37: dot = (x*x + y*y) + z*z
SKEL_HD float skel_len(const float* v) { return skel_sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
// Vec3::normalize, math.rs:39-49: ZERO when len == 0.0, else three divisions
SKEL_HD void skel_normalize(const float* v, float* out) {
    const float l = skel_len(v);
    if (l == 0.0f) { out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; return; }
    out[0] = v[0] / l; out[1] = v[1] / l; out[2] = v[2] / l;
}
// cross, skeleton.rs:273-279
SKEL_HD void skel_cross(const float* a, const float* b, float* out) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// get_bone_tip_position, state.rs:2629-2638: base + Vec3(sin_z*cos_x, cos_z*cos_x, -sin_x).normalize() * length
SKEL_HD void skel_tip(const B32SkelBone& bn, float* tip) {
    const float d[3] = { bn.sin_z * bn.cos_x, bn.cos_z * bn.cos_x, -bn.sin_x };
    float n[3];
    skel_normalize(d, n);
    tip[0] = bn.pos[0] + n[0] * bn.length; tip[1] = bn.pos[1] + n[1] * bn.length; tip[2] = bn.pos[2] + n[2] * bn.length;
}
// skeleton.rs:575-579: (tip - base).len() < 0.001 draws nothing (a NaN length is not < and is drawn)
SKEL_HD bool skel_live(const float* base, const float* tip) {
    const float d[3] = { tip[0] - base[0], tip[1] - base[1], tip[2] - base[2] };
    return !(skel_len(d) < SKEL_DEGENERATE);
}

// Colour and alpha of bone i (skeleton.rs:430-454; mode 1: :546-550).  Priority selected > tip-hovered > hovered > root > default;
// while a bone is selected every other bone gets editor_alpha.min(30).
SKEL_HD void skel_bone_style(const B32SkeletonStyle& st, uint32_t i, bool root, uint32_t& rgb, uint32_t& alpha) {
    const uint32_t plain = skel_colour(root ? SKEL_COL_ROOT : SKEL_COL_DEFAULT);
    alpha = st.editor_alpha;
    if (st.mode != 0u) { rgb = plain; return; }
    const bool selected = st.selected_bone >= 0 && (uint32_t)st.selected_bone == i;
    if (selected) rgb = skel_colour(SKEL_COL_SELECTED);
    else if (st.hovered_tip >= 0 && (uint32_t)st.hovered_tip == i) rgb = skel_colour(SKEL_COL_TIP_HOVERED);
    else if (st.hovered_bone >= 0 && (uint32_t)st.hovered_bone == i) rgb = skel_colour(SKEL_COL_HOVERED);
    else rgb = plain;
    if (st.selected_bone >= 0 && !selected && alpha > SKEL_DIM_ALPHA) alpha = SKEL_DIM_ALPHA;
}
// The octahedron of bone i of a table, or of the creation preview: false when generate_bone_octahedron returns early.
SKEL_HD bool skel_bone_oct(const B32SkelBone& bn, const B32SkeletonStyle& st, uint32_t i, SkelOct& o) {
    for (int k = 0; k < 3; ++k) o.base[k] = bn.pos[k];
    skel_tip(bn, o.tip);
    o.width = bn.width;
    uint32_t rgb, alpha;
    skel_bone_style(st, i, bn.parent == B32_BONE_NONE, rgb, alpha);
    o.r = (uint8_t)(rgb & 255u); o.g = (uint8_t)((rgb >> 8) & 255u); o.b = (uint8_t)((rgb >> 16) & 255u); o.alpha = (uint8_t)alpha;
    return skel_live(o.base, o.tip);
}
SKEL_HD bool skel_preview_oct(const B32SkeletonStyle& st, SkelOct& o) {
    if (st.mode != 0u || !st.has_preview) return false;
    for (int k = 0; k < 3; ++k) { o.base[k] = st.preview_start[k]; o.tip[k] = st.preview_end[k]; }
    o.width = SKEL_DEFAULT_WIDTH;
    const uint32_t rgb = skel_colour(SKEL_COL_CREATING);
    o.r = (uint8_t)(rgb & 255u); o.g = (uint8_t)((rgb >> 8) & 255u); o.b = (uint8_t)((rgb >> 16) & 255u); o.alpha = 255u;
    return skel_live(o.base, o.tip);
}

// Vertex k (0 base, 1 tip, 2..5 ring) of an octahedron, skeleton.rs:575-630
SKEL_HD void skel_vertex(const SkelOct& o, uint32_t k, B32Vertex& v) {
    const float direction[3] = { o.tip[0] - o.base[0], o.tip[1] - o.base[1], o.tip[2] - o.base[2] };
    const float length = skel_len(direction);
    const float inv = 1.0f / length;
    const float dn[3] = { direction[0] * inv, direction[1] * inv, direction[2] * inv };
    float p[3], n[3];
    if (k == 0u) {
        for (int j = 0; j < 3; ++j) { p[j] = o.base[j]; n[j] = dn[j] * -1.0f; }
    } else if (k == 1u) {
        for (int j = 0; j < 3; ++j) { p[j] = o.tip[j]; n[j] = dn[j]; }
    } else {
        // compute_perpendicular_axes, skeleton.rs:257-270
        const bool y_up = __builtin_fabsf(dn[1]) < SKEL_UP_LIMIT;
        const float up[3] = { y_up ? 0.0f : 1.0f, y_up ? 1.0f : 0.0f, 0.0f };
        float c[3], perp[3];
        skel_cross(dn, up, c);
        skel_normalize(c, perp);                                // perp1
        if (k & 1u) {                                           // ring[1] and ring[3] use perp2 = cross(dir, perp1).normalize()
            skel_cross(dn, perp, c);
            skel_normalize(c, perp);
        }
        const float along = length * SKEL_RING_AT;
        float centre[3], d[3];
        for (int j = 0; j < 3; ++j) {
            centre[j] = o.base[j] + dn[j] * along;
            const float w = perp[j] * o.width;
            p[j] = k < 4u ? centre[j] + w : centre[j] - w;      // ring: + perp1, + perp2, - perp1, - perp2
            d[j] = p[j] - centre[j];
        }
        skel_normalize(d, n);
    }
    for (int j = 0; j < 3; ++j) { v.pos[j] = skel_canon(p[j]); v.normal[j] = skel_canon(n[j]); }
    v.uv[0] = 0.0f; v.uv[1] = 0.0f;
    v.r = o.r; v.g = o.g; v.b = o.b; v.blend = B32_BLEND_OPAQUE;
}
// Face k (0..3 the base pyramid, 4..7 the tip pyramid with the ring reversed), skeleton.rs:632-659; first_vertex = v_start
SKEL_HD void skel_face(const SkelOct& o, uint32_t k, uint32_t first_vertex, B32Face& f) {
    const uint32_t i = k & 3u, next = (i + 1u) & 3u;
    if (k < 4u) { f.v[0] = first_vertex; f.v[1] = first_vertex + 2u + i; f.v[2] = first_vertex + 2u + next; }
    else { f.v[0] = first_vertex + 1u; f.v[1] = first_vertex + 2u + next; f.v[2] = first_vertex + 2u + i; }
    f.texture_id = B32_NO_TEXTURE;
    f.black_transparent = 0; f.blend_mode = B32_BLEND_OPAQUE; f.editor_alpha = o.alpha; f._pad = 0;
}

}  // namespace b32
