// b32_room_mesh_body.h -- the arithmetic of Room::to_render_data_with_textures (world/geometry.rs:2839-3352) for ONE output vertex or
// face of ONE record of a b32_room: what add_horizontal_face_to_render_data (:2906-3048), add_wall_to_render_data (:3051-3231) and
// add_diagonal_wall_to_render_data (:3235-3352) push, as a function of the record (B32SectorFace), its material (B32FaceMaterial), the
// grid and the place inside the record alone.  k_room_mesh (b32_room.hip) runs one lane per vertex slot.  Every expression is a
// separately rounded f32 operation in the reference's order; the text also compiles for the host (B32_HD), where
// tests/test_room_mesh.py runs it against a literal restatement and the golden room scenes, built with -ffp-contract=off.
//
// Where a record's output lies depends on (kind, normal_mode) alone: sides = 2 for Both, else 1.
//   floor / ceiling  6 * sides vertices, 2 * sides faces: triangle 1 front, triangle 1 back, triangle 2 front, triangle 2 back (those that
//                    are rendered); vertex slot s is corner s % 3 of rendered triangle s / 3, face k is rendered triangle k
//   wall             4 * sides vertices, 2 * sides faces: front, then back; vertex slot s is corner s % 4 of side s / 4, faces 2 * side
//                    and 2 * side + 1 are that side's
// One departure from the reference's bits: the sign and payload of a NaN are the machine's (inf - inf is 0xFFC00000 on x86 and 0x7FC00000
// here), so every float of a vertex that is a NaN is written as 0x7FC00000 (room_mesh_canon), as the room hover reports its NaN depths.
#pragma once
#include "b32_room_body.h"

namespace b32 {

constexpr uint32_t ROOM_MESH_SLOTS = 12u;       // vertex slots per record: a floor or ceiling with Both

// (constexpr: host and device -- the room's prefix sums are made on the host)
constexpr uint32_t room_mesh_sides(uint32_t normal_mode) { return normal_mode == B32_NORMAL_BOTH ? 2u : 1u; }
constexpr uint32_t room_mesh_vertex_count(uint32_t kind, uint32_t normal_mode) { return (kind < 2u ? 6u : 4u) * room_mesh_sides(normal_mode); }
constexpr uint32_t room_mesh_face_count(uint32_t normal_mode) { return 2u * room_mesh_sides(normal_mode); }
B32_HD float room_mesh_canon(float x) { return x != x ? __builtin_nanf("") : x; }

// Vec3::cross, then Vec3::normalize with its `l == 0.0 -> ZERO` return (math.rs:27-49); back: scale(-1.0), a zero becomes a negative zero
B32_HD void room_mesh_normal(const float* a, const float* b, bool back, float* n) {
    const float x = a[1] * b[2] - a[2] * b[1];
    const float y = a[2] * b[0] - a[0] * b[2];
    const float z = a[0] * b[1] - a[1] * b[0];
    const float l = room_sqrt((x * x + y * y) + z * z);
    if (l == 0.0f) { n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f; }
    else { n[0] = x / l; n[1] = y / l; n[2] = z / l; }
    if (back) { n[0] = n[0] * -1.0f; n[1] = n[1] * -1.0f; n[2] = n[2] * -1.0f; }
}

// add_horizontal_face_to_render_data: vertex slot `slot` < 6 * sides
B32_HD void room_mesh_horizontal_vertex(const B32RoomGrid& g, const B32SectorFace& f, const B32FaceMaterial& m, uint32_t slot, B32Vertex& v) {
    const uint32_t sides = room_mesh_sides(m.normal_mode);
    const uint32_t t = slot / 3u, j = slot - t * 3u;
    const bool second = t >= sides;                                                      // triangle 2
    const bool back = m.normal_mode == B32_NORMAL_BACK || (m.normal_mode == B32_NORMAL_BOTH && (t & 1u));
    const bool is_floor = f.kind == 0u;
    // SplitDirection::triangle_1_corners / triangle_2_corners: NwSe (0, 1, 2) (0, 2, 3); NeSw (0, 1, 3) (1, 2, 3)
    uint32_t c;
    if (m.split_direction == B32_SPLIT_NWSE) c = second ? (j ? j + 1u : 0u) : j;
    else c = second ? j + 1u : (j == 2u ? 3u : j);
    const float* H = (second && (m.flags & B32_MAT_HAS_HEIGHTS_2)) ? m.heights_2 : f.heights;
    const float S = g.sector_size, py = g.position[1];
    float bx, bz;
    room_base(g, f, bx, bz);
    const bool east = c == 1u || c == 2u, south = c >= 2u;                               // NW, NE, SE, SW
    v.pos[0] = room_mesh_canon(east ? bx + S : bx);
    v.pos[1] = room_mesh_canon(py + H[c]);
    v.pos[2] = room_mesh_canon(south ? bz + S : bz);
    {   // edges corners[1] - corners[0] and corners[3] - corners[0] of the triangle's own corner set (:2991-3007)
        const float y0 = py + H[0];
        const float e1[3] = { (bx + S) - bx, (py + H[1]) - y0, bz - bz };
        const float e2[3] = { bx - bx, (py + H[3]) - y0, (bz + S) - bz };
        float n[3];
        if (is_floor) room_mesh_normal(e2, e1, back, n);
        else room_mesh_normal(e1, e2, back, n);
        v.normal[0] = room_mesh_canon(n[0]); v.normal[1] = room_mesh_canon(n[1]); v.normal[2] = room_mesh_canon(n[2]);
    }
    {   // uvs_1 / uvs_2 (:2949-2975): triangle 2 without an override has triangle 1's when the widths are equal
        const bool first = !second || (!(m.flags & B32_MAT_HAS_UV_2) && m.tex_width == m.tex_width_2);
        const bool has = (m.flags & (first ? B32_MAT_HAS_UV : B32_MAT_HAS_UV_2)) != 0;
        float tu, tv;
        if (has) { const float* uv = first ? m.uv[c] : m.uv_2[c]; tu = uv[0]; tv = uv[1]; }
        else {
            const float s = 32.0f / (float)(first ? m.tex_width : m.tex_width_2);
            const float uo = (float)f.gx * s, vo = (float)f.gz * s;
            tu = east ? uo + s : uo; tv = south ? vo + s : vo;
        }
        v.uv[0] = room_mesh_canon(tu); v.uv[1] = room_mesh_canon(tv);
    }
    const uint8_t* col = second ? m.colors_2[c] : m.colors[c];
    v.r = col[0]; v.g = col[1]; v.b = col[2]; v.blend = col[3];
}

// add_wall_to_render_data (kinds 2..5) / add_diagonal_wall_to_render_data (6, 7): vertex slot `slot` < 4 * sides
B32_HD void room_mesh_wall_vertex(const B32RoomGrid& g, const B32SectorFace& f, const B32FaceMaterial& m, uint32_t slot, B32Vertex& v) {
    const uint32_t side = slot >> 2, i = slot & 3u;
    const bool back = m.normal_mode == B32_NORMAL_BACK || side != 0u;
    float bx, bz;
    room_base(g, f, bx, bz);
    // a diagonal's corners come in its own reversed order (:3256-3280): corner i is the hover's corner i ^ 1, height included
    float p[3];
    room_corner(g, f, bx, bz, (int)(f.kind >= 6u ? (i ^ 1u) : i), p);
    v.pos[0] = room_mesh_canon(p[0]); v.pos[1] = room_mesh_canon(p[1]); v.pos[2] = room_mesh_canon(p[2]);
    const float d = 1.0f / room_sqrt(2.0f);
    float nx, nz;
    switch (f.kind) {
        case 2u: nx = 0.0f; nz = 1.0f; break;                                            // North
        case 3u: nx = -1.0f; nz = 0.0f; break;                                           // East
        case 4u: nx = 0.0f; nz = -1.0f; break;                                           // South
        case 5u: nx = 1.0f; nz = 0.0f; break;                                            // West
        case 6u: nx = d; nz = -d; break;                                                 // NwSe
        default: nx = d; nz = d; break;                                                  // NeSw
    }
    float ny = 0.0f;
    if (back) { nx = nx * -1.0f; ny = ny * -1.0f; nz = nz * -1.0f; }
    v.normal[0] = nx; v.normal[1] = ny; v.normal[2] = nz;
    const float s = 32.0f / (float)m.tex_width;
    const bool has = (m.flags & B32_MAT_HAS_UV) != 0;
    float tu, tv;
    if (has) { tu = m.uv[i][0]; tv = m.uv[i][1]; }
    else {
        const float u = (float)((f.kind == 3u || f.kind == 5u) ? f.gz : f.gx) * s;       // East and West tile along z
        tu = (i == 1u || i == 2u) ? u + s : u;
        tv = i < 2u ? s : 0.0f;
    }
    if (m.uv_projection == B32_UV_PROJECTED) tv = ((-(g.position[1] + f.heights[i])) / g.sector_size) * s;   // (heights[i]: not the corner's)
    v.uv[0] = room_mesh_canon(tu); v.uv[1] = room_mesh_canon(tv);
    v.r = m.colors[i][0]; v.g = m.colors[i][1]; v.b = m.colors[i][2]; v.blend = m.colors[i][3];
}

B32_HD void room_mesh_vertex(const B32RoomGrid& g, const B32SectorFace& f, const B32FaceMaterial& m, uint32_t slot, B32Vertex& v) {
    if (f.kind < 2u) room_mesh_horizontal_vertex(g, f, m, slot, v);
    else room_mesh_wall_vertex(g, f, m, slot, v);
}

// Face k < 2 * sides of the record; first_vertex: vertices.len() in front of the record
B32_HD void room_mesh_face(const B32SectorFace& f, const B32FaceMaterial& m, uint32_t k, uint32_t first_vertex, B32Face& o) {
    if (f.kind < 2u) {
        const bool second = k >= room_mesh_sides(m.normal_mode);
        const bool back = m.normal_mode == B32_NORMAL_BACK || (m.normal_mode == B32_NORMAL_BOTH && (k & 1u));
        const bool is_floor = f.kind == 0u;
        const bool flip = back ? is_floor : !is_floor;
        const uint32_t b = first_vertex + 3u * k;
        o.v[0] = b; o.v[1] = flip ? b + 2u : b + 1u; o.v[2] = flip ? b + 1u : b + 2u;
        o.texture_id = second ? m.texture_id_2 : m.texture_id;
    } else {
        const uint32_t side = k >> 1, w = k & 1u;
        const bool back = m.normal_mode == B32_NORMAL_BACK || side != 0u;
        const uint32_t b = first_vertex + 4u * side;
        o.v[0] = b; o.v[1] = back ? b + 1u + w : b + 2u + w; o.v[2] = back ? b + 2u + w : b + 1u + w;
        o.texture_id = m.texture_id;
    }
    o.black_transparent = m.black_transparent ? 1 : 0;
    o.blend_mode = m.blend_mode;
    o.editor_alpha = 255;
    o._pad = 0;
}

}  // namespace b32
