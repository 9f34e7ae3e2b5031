// b32_patch.hip -- a resident scene edited in place: b32_scene_patch_vertices / _faces / _texels / _indexed and b32_scene_read_texels.
//
// Reference: the modeler changes its mesh on the host every frame while the user drags -- the move / rotate / scale tools write the
// selected vertices' positions (modeler/viewport.rs:95, :373), the UV editor writes uv (modeler/layout.rs:3732-3902), the opacity slider
// editor_alpha of an object's faces (viewport.rs:1295), the face panel blend_mode and black_transparent, paint mode atlas indices
// (modeler/mesh_editor.rs:647), the palette panel one CLUT entry (texture/user_texture.rs:337) -- and then hands the whole mesh and the
// re-expanded atlas to the rasterizer again (viewport.rs:1180-1183).  Here only the edited elements travel.
//
// GPU form.  The records (or the packed rectangle) go through a pinned ring to a device buffer on the context's stream (the caller may
// reuse its arrays at once) and ONE kernel scatters them; a lane's work is in b32_patch_body.h.  No LDS, no atomics, no scratch.
//   k_patch_vertices  one lane per record, whole dwords.  On a rigged slot the record is in rest space: the lane writes the rest stream and
//                     poses the vertex with the slot's current bone table, which travels by value in the kernel argument like k_pose's.
//                     A lane's bone index is divergent and a divergent index into the argument block would become a private copy of the
//                     table (scratch), so the wave takes its distinct bone indices one at a time (readfirstlane): the index is then
//                     uniform and the bone is read with scalar loads.  A drag's vertices share a handful of bones.
//   k_patch_faces     one lane per record, whole dwords.
//   k_patch_texels<T> one lane per texel of the rectangle, adjacent lanes adjacent texels of one row.
//   k_patch_indexed   ditto, through Clut::lookup; also the kept index bytes and, for a whole texture, the kept CLUT.
// Ordering against the side stream is b32_scene_pose's (b32_scene.hip); what an edit does to the slot's derived state
// is stated in b32_scene_state.h.
#include "b32_host.h"
#include "b32_patch_body.h"

namespace b32 {

struct PatchTable { B32Bone b[B32_MAX_BONES]; };
struct PatchVertArgs {
    const uint32_t* recs;           // n x PATCH_VERTEX_WORDS
    uint32_t* verts;
    uint32_t* rest;                 // nullptr: the slot has no rig
    const uint16_t* bone_of;
    uint32_t n, n_bones;            // n_bones <= B32_MAX_BONES
};
static_assert(sizeof(B32VertexPatch) == 4 * PATCH_VERTEX_WORDS && offsetof(B32VertexPatch, v) == 4, "B32VertexPatch layout");
static_assert(sizeof(B32FacePatch) == 4 * PATCH_FACE_WORDS && offsetof(B32FacePatch, f) == 4, "B32FacePatch layout");
static_assert(sizeof(B32Vertex) == 36 && sizeof(B32Face) == 20 && sizeof(B32Bone) == 32, "B32Vertex / B32Face / B32Bone layout");
static_assert(sizeof(PatchTable) + sizeof(PatchVertArgs) <= 3072, "kernel argument size");
static_assert(PATCH_CLUT_ENTRIES * 2 == ATLAS_CLUT_BYTES, "the staged CLUT is the kept one's size");

__global__ __launch_bounds__(256) void k_patch_vertices(PatchVertArgs a, PatchTable table) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= a.n) return;
    const uint32_t* rec = a.recs + (size_t)t * PATCH_VERTEX_WORDS;
    const uint32_t b = a.rest ? (uint32_t)a.bone_of[rec[0]] : B32_BONE_NONE;
    if (!a.rest || !patch_has_bone(b, a.n_bones)) {
        patch_vertex(rec, a.verts, a.rest, nullptr);
        return;
    }
    for (bool done = false; !done;) {
        const uint32_t k = __builtin_amdgcn_readfirstlane(b);
        if (b == k) {
            const B32Bone bn = table.b[k];
            patch_vertex(rec, a.verts, a.rest, &bn);
            done = true;
        }
    }
}

__global__ __launch_bounds__(256) void k_patch_faces(const uint32_t* recs, uint32_t n, uint32_t* faces) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < n) patch_face(recs + (size_t)t * PATCH_FACE_WORDS, faces);
}

template <class Texel>
__global__ __launch_bounds__(256) void k_patch_texels(PatchRect r, const Texel* src, Texel* pool) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < r.w * r.h) patch_texel(r, t, src, pool);
}

__global__ __launch_bounds__(256) void k_patch_indexed(PatchRect r, const uint16_t* clut, uint32_t clut_len, uint16_t* pool, uint8_t* atlas, uint32_t write_clut) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < r.w * r.h)
        patch_indexed_texel(r, t, reinterpret_cast<const uint8_t*>(clut + PATCH_CLUT_ENTRIES), clut, clut_len, pool, atlas ? atlas + ATLAS_CLUT_BYTES : nullptr);
    if (write_clut && t < PATCH_CLUT_ENTRIES) patch_kept_clut(t, clut, clut_len, reinterpret_cast<uint16_t*>(atlas));
}

static dim3 patch_grid(uint32_t lanes) { return dim3((uint32_t)(((unsigned long long)lanes + 255u) / 256u)); }

void launch_patch_vertices(hipStream_t s, const uint32_t* recs, uint32_t n, B32Vertex* verts, float* rest, const uint16_t* bone_of, const B32Bone* bones, uint32_t n_bones) {
    if (!n) return;
    if (n_bones > B32_MAX_BONES) n_bones = B32_MAX_BONES;
    PatchVertArgs a{ recs, reinterpret_cast<uint32_t*>(verts), reinterpret_cast<uint32_t*>(rest), bone_of, n, rest ? n_bones : 0u };
    PatchTable t{};
    for (uint32_t k = 0; k < a.n_bones; ++k) t.b[k] = bones[k];
    hipLaunchKernelGGL(k_patch_vertices, patch_grid(n), dim3(256), 0, s, a, t);
}
void launch_patch_faces(hipStream_t s, const uint32_t* recs, uint32_t n, B32Face* faces) {
    if (!n) return;
    hipLaunchKernelGGL(k_patch_faces, patch_grid(n), dim3(256), 0, s, recs, n, reinterpret_cast<uint32_t*>(faces));
}
void launch_patch_texels(hipStream_t s, const PatchRect& r, const void* src, uint16_t* pool15, uint32_t* pool32) {
    if (!r.w || !r.h) return;
    if (pool32) hipLaunchKernelGGL(k_patch_texels<uint32_t>, patch_grid(r.w * r.h), dim3(256), 0, s, r, static_cast<const uint32_t*>(src), pool32);
    else hipLaunchKernelGGL(k_patch_texels<uint16_t>, patch_grid(r.w * r.h), dim3(256), 0, s, r, static_cast<const uint16_t*>(src), pool15);
}
void launch_patch_indexed(hipStream_t s, const PatchRect& r, const void* src, uint32_t clut_len, uint16_t* pool15, uint8_t* atlas, bool write_clut) {
    if (!r.w || !r.h) return;
    const uint32_t lanes = std::max(r.w * r.h, write_clut ? PATCH_CLUT_ENTRIES : 0u);
    hipLaunchKernelGGL(k_patch_indexed, patch_grid(lanes), dim3(256), 0, s, r, static_cast<const uint16_t*>(src), clut_len, pool15, atlas, write_clut ? 1u : 0u);
}

}  // namespace b32

// ------------------------------------------------------------------ the host side
// The body's faces on the host and their tally: fetched once after the geometry was replaced (ONE host synchronisation).  Shared with
// b32_scene_build_mirror (b32_mirror.hip), which tallies the built mesh from it.
extern "C" int patch_fetch_faces(b32_ctx* c, b32_scene* sc) {
    if (sc->h_faces_valid) return B32_OK;
    const uint32_t bf = sc->body_nf();
    sc->h_faces.resize(bf);
    if (bf) {
        HIPCHK(c, hipMemcpyAsync(sc->h_faces.data(), sc->d_faces, (size_t)bf * sizeof(B32Face), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    sc->tally = tally_faces(sc->h_faces.data(), bf, [sc](uint32_t t) { return tex_blends(sc, t); });
    sc->h_faces_valid = true;
    return B32_OK;
}
namespace {

// stage_records (b32_host.h) for a payload the caller assembles in place: `fill` writes n dwords into the pinned ring slot.
template <class Fill>
int patch_stage(b32_ctx* c, uint32_t n, Fill fill) {
    Staged<uint32_t>& ps = c->patch;
    const uint32_t k = ps.slot;
    ps.slot = (k + 1) % LINE_RING;
    if (ps.ev[k]) HIPCHK(c, hipEventSynchronize(ps.ev[k]));
    else HIPCHK(c, hipEventCreateWithFlags(&ps.ev[k], hipEventDisableTiming));
    if (ps.cap_host[k] < n) {
        if (ps.host[k]) HIPCHK(c, hipHostFree(ps.host[k]));
        ps.host[k] = nullptr; ps.cap_host[k] = 0;
        const size_t cap = (size_t)n + n / 4 + 64;
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&ps.host[k]), cap * sizeof(uint32_t), hipHostMallocDefault));
        ps.cap_host[k] = cap;
    }
    fill(ps.host[k]);
    int rc;
    if ((rc = ensure(c, ps.dev, ps.cap_dev, (size_t)n))) return rc;
    HIPCHK(c, hipMemcpyAsync(ps.dev, ps.host[k], (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(ps.ev[k], c->stream));
    return B32_OK;
}

SlotBlend patch_tally_blend(const b32_scene* sc) {   // the slot's blend bookkeeping as its (patched) tally has it
    return tally_slot(sc->tally, *sc, sc->fmt8, sc->tex_blend_any, sc->blend_texels8, sc->tail_v != 0 || sc->tail_f != 0);
}

bool patch_texel_blends8(uint32_t color) {      // b32_scene_upload_rgba: a texel that is neither Opaque nor Erase
    const uint32_t b = color >> 24;
    return b != B32_BLEND_OPAQUE && b != B32_BLEND_ERASE;
}
// The Color pool of an 8-bit-colour scene on the host and how many of its texels blend: fetched once after an upload (ONE host
// synchronisation), because whether ANY texel blends decides the scene's walk (blend8) and a patch can remove the last one.
int patch_fetch_texels32(b32_ctx* c, b32_scene* sc) {
    if (sc->h_texels32_valid) return B32_OK;
    sc->h_texels32.resize(sc->pool_texels);
    if (sc->pool_texels) {
        HIPCHK(c, hipMemcpyAsync(sc->h_texels32.data(), sc->d_texels32, (size_t)sc->pool_texels * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    size_t n = 0;
    for (const TexDesc& d : sc->h_tex)
        for (size_t k = 0, e = (size_t)d.width * d.height; k < e; ++k) n += patch_texel_blends8(sc->h_texels32[d.offset + k]) ? 1u : 0u;
    sc->blend_texel_count = n;
    sc->h_texels32_valid = true;
    return B32_OK;
}

// the checks b32_scene_patch_texels, _indexed and b32_scene_read_texels share; *empty: nothing to do (B32_OK)
int patch_rect_check(const b32_scene* sc, uint32_t tex, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const void* data, uint32_t stride, bool* empty) {
    *empty = false;
    if (tex >= sc->nt || tex >= sc->h_tex.size()) return B32_E_ARG;
    if (!w || !h) { *empty = true; return B32_OK; }
    if (!data || stride < w || !patch_rect_ok(x, y, w, h, sc->h_tex[tex].width, sc->h_tex[tex].height)) return B32_E_ARG;
    return B32_OK;
}

}  // namespace

extern "C" {

int b32_scene_patch_vertices(b32_ctx* c, b32_scene* slot, const B32VertexPatch* recs, uint32_t n) {
    if (!c) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    if (!sc) return B32_E_ARG;
    if (!n) return B32_OK;
    if (!recs || !patch_records_ok(recs, sizeof(B32VertexPatch), n, sc->body_nv())) return B32_E_ARG;
    if ((unsigned long long)n * PATCH_VERTEX_WORDS > 0xFFFFFFFFull) return B32_E_UNSUPPORTED;
    { const int rcs = edit_begin(c); if (rcs) return rcs; }
    const uint32_t words = n * PATCH_VERTEX_WORDS;
    { const int rc = patch_stage(c, words, [&](uint32_t* dst) { std::memcpy(dst, recs, (size_t)words * 4); }); if (rc) return rc; }
    const bool rigged = sc->have_rig;
    launch_patch_vertices(c->stream, c->patch.dev, n, sc->d_verts, rigged ? sc->d_rest : nullptr, sc->d_bone_of, sc->h_bones.data(), rigged ? (uint32_t)sc->h_bones.size() : 0u);
    HIPCHK(c, hipGetLastError());
    vertices_moved(*sc, edit_words(c));
    return B32_OK;
}

int b32_scene_patch_faces(b32_ctx* c, b32_scene* slot, const B32FacePatch* recs, uint32_t n) {
    if (!c) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    if (!sc) return B32_E_ARG;
    if (!n) return B32_OK;
    if (!recs || !patch_records_ok(recs, sizeof(B32FacePatch), n, sc->body_nf())) return B32_E_ARG;
    { const int rcs = edit_begin(c); if (rcs) return rcs; }
    int rc;
    if ((rc = patch_fetch_faces(c, sc))) return rc;      // (the first face patch after an upload synchronises once; later ones do not)
    const uint32_t words = n * PATCH_FACE_WORDS;
    if ((rc = patch_stage(c, words, [&](uint32_t* dst) { std::memcpy(dst, recs, (size_t)words * 4); }))) return rc;
    launch_patch_faces(c->stream, c->patch.dev, n, sc->d_faces);
    HIPCHK(c, hipGetLastError());
    const auto blends = [sc](uint32_t t) { return tex_blends(sc, t); };
    for (uint32_t k = 0; k < n; ++k) {
        B32Face& f = sc->h_faces[recs[k].index];
        tally_face(sc->tally, f, false, blends);
        f = recs[k].f;
        tally_face(sc->tally, f, true, blends);
    }
    faces_edited(*sc, edit_words(c), patch_tally_blend(sc));
    return B32_OK;
}

int b32_scene_patch_texels(b32_ctx* c, b32_scene* slot, uint32_t tex, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const void* texels, uint32_t stride) {
    if (!c) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    if (!sc) return B32_E_ARG;
    bool empty;
    { const int rc = patch_rect_check(sc, tex, x, y, w, h, texels, stride, &empty); if (rc || empty) return rc; }
    { const int rcs = edit_begin(c); if (rcs) return rcs; }
    int rc;
    const TexDesc& d = sc->h_tex[tex];
    const uint32_t elem = sc->fmt8 ? 4u : 2u;
    const uint32_t words = (uint32_t)(((size_t)w * h * elem + 3) / 4);
    if (sc->fmt8 && (rc = patch_fetch_texels32(c, sc))) return rc;
    if ((rc = patch_stage(c, words, [&](uint32_t* dst) { dst[words - 1] = 0; patch_pack_rect(texels, stride, w, h, elem, dst); }))) return rc;
    const PatchRect r{ x, y, w, h, d.width, d.offset };
    launch_patch_texels(c->stream, r, c->patch.dev, sc->fmt8 ? nullptr : sc->d_texels, sc->fmt8 ? sc->d_texels32 : nullptr);
    HIPCHK(c, hipGetLastError());
    if (sc->fmt8) {                                      // does any texel blend now?  (blend_texels8 -> blend8: blend_fresh)
        const uint32_t* src = static_cast<const uint32_t*>(texels);
        for (uint32_t row = 0; row < h; ++row)
            for (uint32_t col = 0; col < w; ++col) {
                uint32_t& old = sc->h_texels32[(size_t)d.offset + (size_t)(y + row) * d.width + x + col];
                uint32_t now;
                std::memcpy(&now, reinterpret_cast<const unsigned char*>(src) + ((size_t)row * stride + col) * 4, 4);
                sc->blend_texel_count += (patch_texel_blends8(now) ? 1 : 0);
                sc->blend_texel_count -= (patch_texel_blends8(old) ? 1 : 0);
                old = now;
            }
        const bool blend_texels = sc->blend_texel_count != 0;
        if (blend_texels != sc->blend_texels8) {
            if ((rc = patch_fetch_faces(c, sc))) return rc;
            sc->blend_texels8 = blend_texels;
            set_blend(*sc, patch_tally_blend(sc));
        }
    }
    texels_rewritten(*sc, edit_words(c), false);        // (expanded texels have no index: the fill reads the pool from now on)
    return B32_OK;
}

int b32_scene_patch_indexed(b32_ctx* c, b32_scene* slot, uint32_t tex, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const uint8_t* indices, uint32_t stride,
                            const uint16_t* clut, uint32_t clut_len) {
    if (!c) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    if (!sc || sc->fmt8) return B32_E_ARG;
    bool empty;
    { const int rc = patch_rect_check(sc, tex, x, y, w, h, indices, stride, &empty); if (rc) return rc; }
    if (clut_len && !clut) return B32_E_ARG;
    if (empty) return B32_OK;
    { const int rcs = edit_begin(c); if (rcs) return rcs; }
    const TexDesc& d = sc->h_tex[tex];
    const uint32_t kept_entries = std::min(clut_len, PATCH_CLUT_ENTRIES);       // (an index is a byte: entries past 256 are never looked up)
    const uint32_t clut_words = PATCH_CLUT_ENTRIES / 2, words = clut_words + (uint32_t)(((size_t)w * h + 3) / 4);
    uint16_t padded[PATCH_CLUT_ENTRIES] = {};
    if (kept_entries) std::memcpy(padded, clut, (size_t)kept_entries * 2);
    int rc;
    if ((rc = patch_stage(c, words, [&](uint32_t* dst) {
            dst[words - 1] = 0;
            std::memcpy(dst, padded, sizeof(padded));
            patch_pack_rect(indices, stride, w, h, 1, dst + clut_words);
        }))) return rc;
    // the kept index atlas (one texture, B32_ROUTE_LDS_ATLAS) follows the patch while its CLUT stays the pool's: a whole-texture patch
    // brings its own, a partial one must come with the kept one or the atlas is dropped
    const bool whole = x == 0 && y == 0 && w == d.width && h == d.height;
    bool keep = sc->atlas_idx_bytes != 0 && sc->h_clut.size() == PATCH_CLUT_ENTRIES;
    if (keep && !whole && std::memcmp(sc->h_clut.data(), padded, sizeof(padded)) != 0) keep = false;
    if (keep && whole) std::memcpy(sc->h_clut.data(), padded, sizeof(padded));
    const PatchRect r{ x, y, w, h, d.width, d.offset };
    launch_patch_indexed(c->stream, r, c->patch.dev, kept_entries, sc->d_texels, keep ? sc->d_atlas0 : nullptr, keep && whole);
    HIPCHK(c, hipGetLastError());
    texels_rewritten(*sc, edit_words(c), keep);
    return B32_OK;
}

int b32_scene_read_texels(b32_ctx* c, b32_scene* slot, uint32_t tex, void* out) {
    if (!c) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    if (!sc || tex >= sc->nt || tex >= sc->h_tex.size()) return B32_E_ARG;
    const TexDesc& d = sc->h_tex[tex];
    const size_t n = (size_t)d.width * d.height;
    if (!n) return B32_OK;
    if (!out) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    const void* src = sc->fmt8 ? static_cast<const void*>(sc->d_texels32 + d.offset) : static_cast<const void*>(sc->d_texels + d.offset);
    HIPCHK(c, hipMemcpyAsync(out, src, n * (sc->fmt8 ? 4u : 2u), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}

}  // extern "C"
