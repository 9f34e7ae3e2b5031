// b32_room.hip -- the world editor's hover and rubber band over the current room's sector faces: b32_room, b32_room_hover[_async],
// b32_room_box_select[_async], b32_room_hover_winner.
//
// Reference: find_hovered_elements (editor/viewport_3d.rs:7028-7336) asks on every mouse move which sector vertex, edge or face is under
// the cursor, each loop keeping the candidate of SMALLEST CAMERA DEPTH (the modeler's b32_hover_mesh keeps the smallest distance);
// find_selections_in_rect (:7512-7594) projects every face's centre and every object's position against a rectangle.  Both walk the
// sector grid itself -- per face four heights on a lattice -- which a b32_room holds as one 24-byte record per face in the reference's
// loop order; the arithmetic of one record is b32_room_body.h.
//
// GPU form of a hover.  "None yet, or strictly smaller depth" in loop order is the rule of b32_pick.hip's three minima, once per loop.
//   k_room_hover          one lane per record, 1024 records per workgroup in four trips of 256 lanes; a lane projects its four corners
//                         once and offers its vertices, edges and face to three sets of minima, which are reduced one after the other
//                         (pick_reduce's LDS scratch is one array: a barrier between two reductions); at most one agent-scope atomic
//                         per word and workgroup.
//   k_room_hover_resolve  one workgroup: decodes the three sets, recomputes the winners' distance and depth from their records (exact
//                         bits, the sign of a zero), writes the 48-byte result and re-arms the words for the next call on the stream.
// k_room_box: one lane per element (records, then points); a wave's ballot is two words of the bitmap, as in k_box_select.
//
// The room's render mesh (b32_room_set_materials, b32_room_update_materials, b32_room_build_mesh): Room::to_render_data_with_textures
// (world/geometry.rs:2839-3352) from the resident records and one B32FaceMaterial per record; the arithmetic of one vertex and one face
// is b32_room_mesh_body.h.  Where a record's output lies depends on (kind, normal_mode) alone, which the room keeps on the host with the
// prefix sums of the counts; the sums are uploaded in stream order whenever a kind or a mode changes, no scan runs on the device.
//   k_room_mesh           one lane per vertex slot, 12 slots per record (a floor or ceiling with Both), surplus slots idle: consecutive
//                         lanes write consecutive B32Vertex records; the first 2 or 4 slots also write the record's faces.  A lane reads
//                         record and material where they lie (the corner index is divergent: no private copy, no scratch) and never reads
//                         the slot's vertices.  Lane 0 writes the slot's device-side face count.
#include "b32_pick_body.h"
#include "b32_room_mesh_body.h"
#include "b32_room_winner.h"

namespace b32 {

struct RoomWords { PickWords vertex, edge, face; };
struct RoomHoverArgs {
    ViewBlock v; B32RoomGrid grid; B32RoomHoverParams prm;      // (v: perspective only, has_ortho == 0)
    const B32SectorFace* faces; uint32_t n;
    RoomWords* words;
    unsigned char* result;                      // one B32RoomHover
};
struct RoomBoxArgs {
    ViewBlock v; B32RoomGrid grid;
    const B32SectorFace* faces; const float* points;
    uint32_t n, n_points, nwords;
    float x0, y0, x1, y1;
    unsigned char* result;                      // the header and the words
};
struct RoomMeshArgs {
    B32RoomGrid grid;
    const B32SectorFace* faces; const B32FaceMaterial* mats; const uint2* first;
    B32Vertex* verts; B32Face* out_faces; uint32_t* consts;
    uint32_t n, nv, nf;
};
static_assert(sizeof(B32SectorFace) == 24 && sizeof(B32RoomGrid) == 16 && sizeof(B32RoomHoverParams) == 16 && sizeof(B32RoomHover) == 48 &&
              sizeof(RoomWords) == 48, "room records");
static_assert(sizeof(B32FaceMaterial) == 136 && offsetof(B32FaceMaterial, uv) == 16 && offsetof(B32FaceMaterial, uv_2) == 48 &&
              offsetof(B32FaceMaterial, colors) == 80 && offsetof(B32FaceMaterial, colors_2) == 96 && offsetof(B32FaceMaterial, heights_2) == 112 &&
              offsetof(B32FaceMaterial, normal_mode) == 128 && offsetof(B32FaceMaterial, flags) == 133 && sizeof(B32Face) == 20, "room mesh records");

__global__ __launch_bounds__(256) void k_room_hover(RoomHoverArgs a) {
    const uint32_t e0 = blockIdx.x * PICK_CHUNK;
    PickWords mv = pick_no_hit(), me = pick_no_hit(), mf = pick_no_hit();
#pragma unroll 1
    for (uint32_t trip = 0; trip < PICK_CHUNK / 256u; ++trip) {
        const uint32_t i = e0 + trip * 256u + threadIdx.x;
        if (i >= a.n) continue;
        const B32SectorFace f = a.faces[i];
        RoomCandidates c;
        room_candidates(a.v, a.grid, f, a.prm, c);
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if ((c.vmask >> k) & 1u) pick_take(mv, c.vdepth[k], i * 4u + k);
            if ((c.emask >> k) & 1u) pick_take(me, c.edepth[k], i * 4u + k);
        }
        if (c.face) pick_take(mf, c.fdepth, i);
    }
    mv = pick_reduce(mv);
    __syncthreads();                            // thread 0 has read the scratch before the next reduction writes it
    me = pick_reduce(me);
    __syncthreads();
    mf = pick_reduce(mf);
    if (threadIdx.x == 0u) {
        pick_offer(mv, &a.words->vertex);
        pick_offer(me, &a.words->edge);
        pick_offer(mf, &a.words->face);
    }
}

__global__ __launch_bounds__(64) void k_room_hover_resolve(RoomHoverArgs a) {
    if (threadIdx.x != 0u) return;
    const RoomWords w = *a.words;
    RoomWords armed; armed.vertex = pick_no_hit(); armed.edge = pick_no_hit(); armed.face = pick_no_hit();
    *a.words = armed;
    B32RoomHover r;
    r.vertex_rec = PICK_NONE; r.vertex_corner = PICK_NONE; r.vertex_dist = 0.0f; r.vertex_depth = 0.0f;
    r.edge_rec = PICK_NONE; r.edge_idx = PICK_NONE; r.edge_dist = 0.0f; r.edge_depth = 0.0f;
    r.face_rec = PICK_NONE; r.face_depth = 0.0f; r._pad[0] = 0u; r._pad[1] = 0u;
    uint32_t id; bool nan;
    if (pick_winner(w.vertex, id, nan) && (id >> 2) < a.n) {
        RoomQuad q;
        room_project(a.v, a.grid, a.faces[id >> 2], q);
        r.vertex_rec = id >> 2; r.vertex_corner = id & 3u;
#pragma unroll
        for (int k = 0; k < 4; ++k)             // (constant indices: the quad stays in registers)
            if ((uint32_t)k == (id & 3u)) (void)room_vertex(q, k, a.prm.mx, a.prm.my, a.prm.vertex_threshold, r.vertex_dist, r.vertex_depth);
        if (nan) r.vertex_depth = __uint_as_float(PICK_QNAN);
    }
    if (pick_winner(w.edge, id, nan) && (id >> 2) < a.n) {
        RoomQuad q;
        room_project(a.v, a.grid, a.faces[id >> 2], q);
        r.edge_rec = id >> 2; r.edge_idx = id & 3u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((uint32_t)k == (id & 3u)) (void)room_edge(q, k, a.prm.mx, a.prm.my, a.prm.edge_threshold, r.edge_dist, r.edge_depth);
        if (nan) r.edge_depth = __uint_as_float(PICK_QNAN);
    }
    if (pick_winner(w.face, id, nan) && id < a.n) {
        RoomQuad q;
        room_project(a.v, a.grid, a.faces[id], q);
        r.face_rec = id;
        (void)room_face(q, a.prm.mx, a.prm.my, r.face_depth);
        if (nan) r.face_depth = __uint_as_float(PICK_QNAN);
    }
    *reinterpret_cast<B32RoomHover*>(a.result) = r;
}

// find_selections_in_rect, viewport_3d.rs:7512-7594.  The header's n_selected is zero when the kernel starts.
__global__ __launch_bounds__(256) void k_room_box(RoomBoxArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t total = a.n + a.n_points;
    bool sel = false;
    if (i < total) {
        float p[3];
        if (i < a.n) room_centre(a.grid, a.faces[i], p);
        else { const float* s = a.points + (size_t)(i - a.n) * 3; p[0] = s[0]; p[1] = s[1]; p[2] = s[2]; }
        sel = room_point_in_rect(a.v, p, a.x0, a.y0, a.x1, a.y1);
    }
    box_emit(a.result, i, total, a.nwords, sel);
}

// Room::to_render_data_with_textures: lane t is vertex slot t % 12 of record t / 12 (12 * n <= 12 * 2^24).  The stores are guarded by the
// counts the host allocated for, whatever the tables say.
__global__ __launch_bounds__(256) void k_room_mesh(RoomMeshArgs a) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t == 0u) { a.consts[0] = a.nf; a.consts[1] = 0u; a.consts[2] = 0u; a.consts[3] = 0u; }      // (h_consts of an upload)
    const uint32_t rec = t / ROOM_MESH_SLOTS, slot = t - rec * ROOM_MESH_SLOTS;
    if (rec >= a.n) return;
    const B32SectorFace& f = a.faces[rec];
    const B32FaceMaterial& m = a.mats[rec];
    const uint2 at = a.first[rec];
    const uint32_t kind = f.kind, mode = m.normal_mode;
    if (slot < room_mesh_vertex_count(kind, mode) && at.x + slot < a.nv) {
        B32Vertex v;
        room_mesh_vertex(a.grid, f, m, slot, v);
        a.verts[at.x + slot] = v;
    }
    if (slot < room_mesh_face_count(mode) && at.y + slot < a.nf) {
        B32Face o;
        room_mesh_face(f, m, slot, at.x, o);
        a.out_faces[at.y + slot] = o;
    }
}

}  // namespace b32

// ------------------------------------------------------------------ host
namespace {

bool room_kinds_ok(const B32SectorFace* faces, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) if (faces[i].kind > 7u) return false;
    return true;
}

bool room_materials_ok(const B32FaceMaterial* m, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        if (m[i].normal_mode > B32_NORMAL_BACK || m[i].split_direction > B32_SPLIT_NESW || m[i].uv_projection > B32_UV_PROJECTED || m[i].blend_mode > B32_BLEND_ERASE) return false;
    return true;
}
// The prefix sums from record `from` on (entry i: vertices and faces in front of record i; entry n: the mesh's counts), and their upload
// in stream order.
int room_mesh_layout(b32_ctx* c, b32_room* r, uint32_t from) {
    for (uint32_t i = from; i < r->n; ++i) {
        const uint2 at = r->h_first[i];
        r->h_first[i + 1] = make_uint2(at.x + room_mesh_vertex_count(r->h_kind[i], r->h_mode[i]), at.y + room_mesh_face_count(r->h_mode[i]));
    }
    if (from < r->n) HIPCHK(c, hipMemcpyAsync(r->first + from, r->h_first.data() + from, (size_t)(r->n - from) * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
    return B32_OK;
}
// What the host keeps of materials [first, first + count); returns the first record whose normal_mode changed (n: none)
uint32_t room_materials_keep(b32_room* r, uint32_t first, uint32_t count, const B32FaceMaterial* m) {
    uint32_t changed = r->n;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t k = first + i;
        const uint32_t faces = room_mesh_face_count(r->h_mode[k]);
        if (r->have_mats && r->h_blend[k] != B32_BLEND_OPAQUE) r->own_blend_faces -= faces;
        if (r->h_mode[k] != m[i].normal_mode && changed == r->n) changed = k;
        r->h_mode[k] = m[i].normal_mode; r->h_blend[k] = m[i].blend_mode;
        r->h_tex[2 * (size_t)k] = m[i].texture_id; r->h_tex[2 * (size_t)k + 1] = m[i].texture_id_2;
        if (m[i].blend_mode != B32_BLEND_OPAQUE) r->own_blend_faces += room_mesh_face_count(m[i].normal_mode);
    }
    return changed;
}

int room_common_check(const b32_ctx* c, const B32Camera* cam, const b32_room* room) {
    if (!c || !cam || !room || !c->width || !c->height) return B32_E_ARG;
    return B32_OK;
}

}  // namespace

extern "C" {

int b32_room_create(b32_ctx* c, const B32RoomGrid* grid, const B32SectorFace* faces, uint32_t n, b32_room** out) {
    if (!c || !out) return B32_E_ARG;
    *out = nullptr;
    if (!grid || (n && !faces)) return B32_E_ARG;
    if (n > B32_ROOM_MAX_FACES) return B32_E_UNSUPPORTED;
    if (!room_kinds_ok(faces, n)) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    b32_room* r = new b32_room();
    r->n = n; r->grid = *grid;
    r->h_kind.resize(n);
    for (uint32_t i = 0; i < n; ++i) r->h_kind[i] = faces[i].kind;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&r->faces), n ? (size_t)n * sizeof(B32SectorFace) : 4);
    if (e == hipSuccess && n) e = hipMemcpyAsync(r->faces, faces, (size_t)n * sizeof(B32SectorFace), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
        c->last_hip = (int)e;
        if (r->faces) (void)hipFree(r->faces);
        delete r;
        return B32_E_HIP;
    }
    *out = r;
    return B32_OK;
}

int b32_room_update(b32_ctx* c, b32_room* room, const B32RoomGrid* grid, uint32_t first, uint32_t count, const B32SectorFace* faces) {
    if (!c || !room || (count && !faces)) return B32_E_ARG;
    if ((unsigned long long)first + count > room->n) return B32_E_ARG;
    if (!room_kinds_ok(faces, count)) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    if (count) HIPCHK(c, hipMemcpyAsync(room->faces + first, faces, (size_t)count * sizeof(B32SectorFace), hipMemcpyHostToDevice, c->stream));
    if (grid) room->grid = *grid;
    uint32_t changed = room->n;                 // a kind that changes moves every later record's place in the render mesh
    for (uint32_t i = 0; i < count; ++i) {
        if (room->h_kind[first + i] != faces[i].kind && changed == room->n) changed = first + i;
        room->h_kind[first + i] = faces[i].kind;
    }
    if (room->have_mats && changed < room->n) return room_mesh_layout(c, room, changed);
    return B32_OK;
}

int b32_room_set_materials(b32_ctx* c, b32_room* room, const B32FaceMaterial* m) {
    if (!c || !room || (room->n && !m)) return B32_E_ARG;
    if (!room_materials_ok(m, room->n)) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    const uint32_t n = room->n;
    if (!room->mats) {
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&room->mats), n ? (size_t)n * sizeof(B32FaceMaterial) : 8));
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&room->first), n ? (size_t)n * sizeof(uint2) : 8));
        room->h_mode.assign(n, 0); room->h_blend.assign(n, 0); room->h_tex.assign(2 * (size_t)n, 0); room->h_first.assign((size_t)n + 1, make_uint2(0, 0));
    }
    if (n) HIPCHK(c, hipMemcpyAsync(room->mats, m, (size_t)n * sizeof(B32FaceMaterial), hipMemcpyHostToDevice, c->stream));
    room->have_mats = false; room->own_blend_faces = 0;
    (void)room_materials_keep(room, 0, n, m);
    room->have_mats = true;
    return room_mesh_layout(c, room, 0);
}

int b32_room_update_materials(b32_ctx* c, b32_room* room, uint32_t first, uint32_t count, const B32FaceMaterial* m) {
    if (!c || !room || !room->have_mats || (count && !m)) return B32_E_ARG;
    if ((unsigned long long)first + count > room->n) return B32_E_ARG;
    if (!room_materials_ok(m, count)) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    if (count) HIPCHK(c, hipMemcpyAsync(room->mats + first, m, (size_t)count * sizeof(B32FaceMaterial), hipMemcpyHostToDevice, c->stream));
    const uint32_t changed = room_materials_keep(room, first, count, m);
    if (changed < room->n) return room_mesh_layout(c, room, changed);
    return B32_OK;
}

int b32_room_mesh_counts(const b32_room* room, uint32_t* nv, uint32_t* nf) {
    if (!room || !room->have_mats || !nv || !nf) return B32_E_ARG;
    *nv = room->h_first[room->n].x; *nf = room->h_first[room->n].y;
    return B32_OK;
}

// Another mesh in the slot, like an upload's (geometry_replaced); the ordering argument is the pose's.
int b32_room_build_mesh(b32_ctx* c, b32_room* room, b32_scene* slot) {
    if (!c || !room || !room->have_mats) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    if (!sc) return B32_E_ARG;
    { const int rcs = edit_begin(c); if (rcs) return rcs; }
    const uint32_t n = room->n, nv = room->h_first[n].x, nf = room->h_first[n].y;
    int rc;
    if ((rc = ensure(c, sc->d_verts, sc->cap_verts, (size_t)nv + 1))) return rc;
    if ((rc = ensure(c, sc->d_faces, sc->cap_faces, (size_t)nf + 1))) return rc;
    if (!sc->d_consts) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&sc->d_consts), 16 * sizeof(uint32_t)));
    // the face tally from the room's own tables (the faces exist on the device only): editor_alpha is 255, so a face's own part is its
    // blend mode; a texture's blend mode adds to it
    FaceTally tally;
    tally.own = tally.any = room->own_blend_faces;
    if (sc->tex_blend_any) {
        tally.any = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t sides = room_mesh_sides(room->h_mode[i]);
            const bool own = room->h_blend[i] != B32_BLEND_OPAQUE, flat = room->h_kind[i] < 2u;
            tally.any += (own || tex_blends(sc, room->h_tex[2 * (size_t)i])) ? sides : 0u;
            tally.any += (own || tex_blends(sc, room->h_tex[2 * (size_t)i + (flat ? 1 : 0)])) ? sides : 0u;
        }
    }
    const bool same_nf = sc->nf == nf;
    sc->nv = nv; sc->nf = nf;
    if ((rc = ensure_work(c, nf))) return rc;
    geometry_replaced(*sc, edit_words(c), same_nf, blend_fresh(tally, *sc, sc->fmt8, sc->tex_blend_any, sc->blend_texels8));
    RoomMeshArgs a{};
    a.grid = room->grid; a.faces = room->faces; a.mats = room->mats; a.first = room->first;
    a.verts = sc->d_verts; a.out_faces = sc->d_faces; a.consts = sc->d_consts;
    a.n = n; a.nv = nv; a.nf = nf;
    const uint32_t groups = (uint32_t)(((unsigned long long)n * ROOM_MESH_SLOTS + 255u) / 256u);
    hipLaunchKernelGGL(k_room_mesh, dim3(groups ? groups : 1u), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    return B32_OK;
}

void b32_room_destroy(b32_ctx* c, b32_room* room) {
    if (!room) return;
    if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }     // (a hover that reads it may be in flight)
    for (void* p : { (void*)room->faces, (void*)room->mats, (void*)room->first, room->d_hover }) if (p) (void)hipFree(p);
    delete room;
}

int b32_room_hover_async(b32_ctx* c, const B32Camera* cam, b32_room* room, const B32RoomHoverParams* prm, void* out, uint64_t* ticket) {
    { const int rc = room_common_check(c, cam, room); if (rc) return rc; }
    if (!prm || !out || !ticket) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    int rc;
    RoomHoverArgs a{};
    view_fill(a.v, *cam, c->width, c->height, nullptr);
    a.grid = room->grid; a.prm = *prm; a.faces = room->faces; a.n = room->n;
    // the words: all ones whenever no room hover is running (allocated so; k_room_hover_resolve leaves them so)
    if ((rc = armed_ensure(c, c->room_words, sizeof(RoomWords), 0xFF))) return rc;
    a.words = static_cast<RoomWords*>(c->room_words.p);
    unsigned long long t = 0; hipEvent_t* tev = nullptr; uint32_t k = 0;
    const size_t bytes = sizeof(B32RoomHover);
    if ((rc = pick_result_open(c, bytes, t, tev, k, &a.result))) return rc;
    const uint32_t groups = (a.n + PICK_CHUNK - 1u) / PICK_CHUNK;                       // (n <= 2^24)
    if (groups) hipLaunchKernelGGL(k_room_hover, dim3(groups), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_room_hover_resolve, dim3(1), dim3(64), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    // the room's own copy of the result, for b32_draw_room_overlay's hover_source 1: behind the resolve kernel on the stream
    if (!room->d_hover) HIPCHK(c, hipMalloc(&room->d_hover, sizeof(B32RoomHover)));
    HIPCHK(c, hipMemcpyAsync(room->d_hover, a.result, sizeof(B32RoomHover), hipMemcpyDeviceToDevice, c->stream));
    room->have_hover = true;
    return pick_result_deliver(c, k, bytes, out, t, tev, ticket);
}

int b32_room_hover(b32_ctx* c, const B32Camera* cam, b32_room* room, const B32RoomHoverParams* prm, B32RoomHover* out) {
    { const int rc = room_common_check(c, cam, room); if (rc) return rc; }
    if (!prm || !out) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    const unsigned char* h = nullptr;
    const int rc = pick_blocking(c, sizeof(B32RoomHover), &h, [&](void* landing, uint64_t* t) {
        return b32_room_hover_async(c, cam, room, prm, landing, t); });
    if (rc) return rc;
    std::memcpy(out, h, sizeof(B32RoomHover));
    return B32_OK;
}

// viewport_3d.rs:7283-7336: the one text of the rule is room_hover_winner (b32_room_winner.h), which the room overlay runs on the device.
int b32_room_hover_winner(const B32RoomHover* h) { return h ? room_hover_winner(*h) : -1; }

int b32_room_box_select_async(b32_ctx* c, const B32Camera* cam, b32_room* room, float x0, float y0, float x1, float y1, const float* points_xyz,
                              uint32_t n_points, void* out, uint64_t* ticket) {
    { const int rc = room_common_check(c, cam, room); if (rc) return rc; }
    if ((n_points && !points_xyz) || !out || !ticket) return B32_E_ARG;
    if ((unsigned long long)room->n + n_points >= (1ull << 32)) return B32_E_UNSUPPORTED;
    (void)hipSetDevice(c->device);
    int rc;
    RoomBoxArgs a{};
    view_fill(a.v, *cam, c->width, c->height, nullptr);
    a.grid = room->grid; a.faces = room->faces; a.n = room->n; a.n_points = n_points;
    a.x0 = x0; a.y0 = y0; a.x1 = x1; a.y1 = y1;
    const uint32_t total = a.n + n_points;
    a.nwords = (uint32_t)(((unsigned long long)total + 31u) / 32u);
    if (n_points) {                             // the points: copied before return, ordered on the stream behind the last call that read them
        const size_t bytes = (size_t)n_points * 3u * sizeof(float);
        if ((rc = armed_ensure(c, c->room_points, bytes, -1))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->room_points.p, points_xyz, bytes, hipMemcpyHostToDevice, c->stream));
        a.points = static_cast<const float*>(c->room_points.p);
    }
    return box_run(c, a.nwords, &a.result, out, ticket, [&] {
        if (total) hipLaunchKernelGGL(k_room_box, dim3((uint32_t)(((unsigned long long)total + 255u) / 256u)), dim3(256), 0, c->stream, a); });
}

int b32_room_box_select(b32_ctx* c, const B32Camera* cam, b32_room* room, float x0, float y0, float x1, float y1, const float* points_xyz,
                        uint32_t n_points, uint32_t* words, uint32_t* n_selected) {
    { const int rc = room_common_check(c, cam, room); if (rc) return rc; }
    if ((n_points && !points_xyz) || !n_selected) return B32_E_ARG;
    if ((unsigned long long)room->n + n_points >= (1ull << 32)) return B32_E_UNSUPPORTED;
    (void)hipSetDevice(c->device);
    const size_t nwords = (size_t)(((unsigned long long)room->n + n_points + 31u) / 32u);
    const unsigned char* h = nullptr;
    const int rc = pick_blocking(c, box_bytes(nwords), &h, [&](void* landing, uint64_t* t) {
        return b32_room_box_select_async(c, cam, room, x0, y0, x1, y1, points_xyz, n_points, landing, t); });
    if (rc) return rc;
    box_landed(h, nwords, words, n_selected);
    return B32_OK;
}

}  // extern "C"
