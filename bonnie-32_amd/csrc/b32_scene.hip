// b32_scene.hip -- the C ABI, part 2: host -> device uploads (the drop-in calls' staged arena, resident scenes with Texture15 / Texture /
// index atlas + CLUT), scene slots, and the synchronous drop-in calls render_mesh[_15] / render_scene[_15].
#include "b32_host.h"
#include "b32_skeleton_body.h"

extern "C" {
// ------------------------------------------------------------------ scene upload
// Host -> device copy of an upload.  Inside a drop-in call (stage_active) the bytes are packed into the pinned arena and moved later
// by one kernel (stage_flush); a copy that does not fit, or any other caller, takes the stream's ordinary async copy.  The arena copy
// rounds the length up to 16 B: every destination has at least 15 B of slack (ensure() allocates one element more than asked for, texel
// offsets are multiples of 16 B).
int h2d(b32_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!bytes) return B32_OK;
    c->side_dirty = true;
    const size_t padded = (bytes + 15) & ~(size_t)15;
    if (c->stage_active && c->stage_segs.count < 16 && c->stage_used + padded <= c->stage_cap && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        std::memcpy(c->stage_host + c->stage_used, src, bytes);
        const uint32_t k = c->stage_segs.count++;
        c->stage_segs.dst[k] = dst; c->stage_segs.src_off[k] = (uint32_t)c->stage_used; c->stage_segs.n16[k] = (uint32_t)(padded >> 4);
        c->stage_used += padded;
        return B32_OK;
    }
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return B32_OK;
}
static_assert(sizeof(Ctrl) == 64 && sizeof(Stamps) == 64, "Ctrl and Stamps are read back through a 128-byte slot of the pinned arena");
bool stage_ensure(b32_ctx* c) {
    if (!c->stage_host && !c->stage_failed) {
        void* h = nullptr;
        c->stage_failed = true;
        if (hipHostMalloc(&h, STAGE_BYTES, hipHostMallocDefault) == hipSuccess) {
            void* d = nullptr;
            if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess && d) {
                c->stage_host = static_cast<unsigned char*>(h); c->stage_dev = d; c->stage_cap = STAGE_CTRL_OFF; c->stage_failed = false;
            } else (void)hipHostFree(h);
        }
        (void)hipGetLastError();
    }
    return c->stage_host != nullptr;
}
static void stage_begin(b32_ctx* c) {
    (void)hipSetDevice(c->device);
    stage_ensure(c);
    c->stage_used = 0; c->stage_segs.count = 0;
    c->stage_active = c->stage_host != nullptr;
}
static void stage_flush(b32_ctx* c) {        // enqueue the one copy kernel (ordered before the frame's kernels on the same stream)
    if (c->stage_active && c->stage_segs.count) launch_upload(c->stream, c->stage_dev, c->stage_segs);
    c->stage_active = false; c->stage_segs.count = 0; c->stage_used = 0;
}

// per-face work buffers of the current frame set for a mesh of nf faces
int ensure_work(b32_ctx* c, uint32_t nf) {
    int rc;
    if ((size_t)nf + 1 > c->cap_work || !c->cur.crecs) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const size_t n = (size_t)nf + nf / 4 + 16;
        if ((rc = ensure_plain(c, c->cur.keys0, n))) return rc;
        if ((rc = ensure_plain(c, c->vals[0], n))) return rc;
        if ((rc = ensure_plain(c, c->keys1, n))) return rc;
        if ((rc = ensure_plain(c, c->vals[1], n))) return rc;
        if ((rc = ensure_plain(c, c->cur.crecs, n))) return rc;
        if ((rc = ensure_plain(c, c->cur.srecs, n))) return rc;
        if ((rc = ensure_plain(c, c->cur.xrecs, n))) return rc;
        if ((rc = ensure_plain(c, c->counts, n))) return rc;
        if ((rc = ensure_plain(c, c->cur.spans, n))) return rc;
        if ((rc = ensure_plain(c, c->cur.face_of, n))) return rc;
        c->bin_blocks = (uint32_t)((n + 4095) / 4096);
        c->partial_blocks = (uint32_t)((n + 255) / 256);
        if ((rc = ensure_plain(c, c->cur.partials, (size_t)c->partial_blocks * 8 + 8))) return rc;
        if ((rc = ensure_plain(c, c->block_sums, (size_t)c->bin_blocks + 1))) return rc;
        c->cap_work = c->cur.cap_work = n;
    }
    return B32_OK;
}

// What the three uploads end with, behind their texel walk (the textures are laid out: the face tally asks them): vertices and faces to
// the device, the slot's derived state (geometry_replaced), and the slot holds a scene again.
static int upload_geometry(b32_ctx* c, const B32Vertex* v, uint32_t nv, const B32Face* f, uint32_t nf, bool fmt8) {
    if ((nv && !v) || (nf && !f)) return B32_E_ARG;
    b32_scene& sc = c->scene;
    int rc;
    if ((rc = ensure(c, sc.d_verts, sc.cap_verts, (size_t)nv + 1))) return rc;
    if ((rc = ensure(c, sc.d_faces, sc.cap_faces, (size_t)nf + 1))) return rc;
    const FaceTally tally = tally_faces(f, nf, [&sc](uint32_t t) { return tex_blends(&sc, t); });
    if ((rc = h2d(c, sc.d_verts, v, (size_t)nv * sizeof(B32Vertex)))) return rc;
    if ((rc = h2d(c, sc.d_faces, f, (size_t)nf * sizeof(B32Face)))) return rc;
    const bool same_nf = sc.nf == nf;
    sc.nv = nv; sc.nf = nf;
    if ((rc = ensure_work(c, nf))) return rc;
    geometry_replaced(sc, edit_words(c), same_nf, blend_fresh(tally, sc, fmt8, sc.tex_blend_any, sc.blend_texels8));
    c->h_consts[0] = nf;
    if (!sc.d_consts) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&sc.d_consts), 16 * sizeof(uint32_t)));   // (swapped away with a scene)
    if ((rc = h2d(c, sc.d_consts, c->h_consts, sizeof(c->h_consts)))) return rc;
    // the caller may reuse its host buffers as soon as an upload call returns; the drop-in render calls return only after
    // b32_frame_finish has synchronised the stream, so they skip this extra round trip
    if (!c->defer_upload_sync) HIPCHK(c, hipStreamSynchronize(c->stream));
    sc.fmt8 = fmt8;
    sc.have_scene = true;
    return B32_OK;
}

// CHEAP coverage is worth it while skipped winners are rare: textures with at most 1/cheap_den skippable texels (b32_set_cheap_threshold).  Measured on the C3
// geometry with 1 transparent CLUT entry out of K (tools/cheap_threshold.py): EXACT coverage (skip mask in LDS) 0.233 ms whatever the
// texture; CHEAP 0.19 ms at K = 256, 0.220 at 64, 0.246 at 32, 0.307 at 16, 0.46 at 8.  (b32_set_cheap_threshold: that tool's switch.)

static int layout_textures(b32_ctx* c, uint32_t nt, const uint32_t* w, const uint32_t* h, const uint32_t* blend, size_t* total, bool rgba = false) {
    pool_replaced(c->scene);                         // (first: a layout that fails half-way leaves nothing that describes the old pool)
    if (nt > 65534) return B32_E_UNSUPPORTED;        // the surface record holds the texture slot in 16 bits
    c->scene.h_tex.resize(nt);
    c->scene.tex_blend_any = false;
    size_t off = 0;
    for (uint32_t i = 0; i < nt; ++i) {
        if (w[i] > 65535 || h[i] > 65535) return B32_E_ARG;
        if (blend[i] != B32_BLEND_OPAQUE) c->scene.tex_blend_any = true;
        c->scene.h_tex[i] = { w[i], h[i], blend[i], (uint32_t)off };
        off += ((size_t)w[i] * h[i] + 7) & ~(size_t)7;
        if (off > 0x7FFFFFFFull) return B32_E_ARG;
    }
    *total = off + 8;
    c->scene.pool_texels = (uint32_t)off;
    int rc;
    if ((rc = ensure(c, c->scene.d_texmask, c->scene.cap_texmask, off / 32 + 4))) return rc;
    if (rgba) { if ((rc = ensure(c, c->scene.d_texels32, c->scene.cap_texels32, *total))) return rc; }
    else if ((rc = ensure(c, c->scene.d_texels, c->scene.cap_texels, *total))) return rc;
    if ((rc = ensure(c, c->scene.d_tex, c->scene.cap_tex, (size_t)nt + 1))) return rc;
    if ((rc = h2d(c, c->scene.d_tex, c->scene.h_tex.data(), nt * sizeof(TexDesc)))) return rc;
    c->scene.nt = nt;
    return B32_OK;
}

// 64-bit content hash, four independent lanes of 8-byte words (about memcpy speed; the tail bytes go through a padded word)
static uint64_t hash_bytes(const void* data, size_t n) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    const uint64_t K1 = 0x9E3779B185EBCA87ull, K2 = 0xC2B2AE3D27D4EB4Full;
    uint64_t h[4] = { K1 ^ n, K2 + n, K1 * 3 + n, K2 * 5 ^ n };
    auto round = [&](uint64_t acc, uint64_t x) { acc += x * K2; acc = (acc << 31) | (acc >> 33); return acc * K1; };
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        uint64_t w[4];
        std::memcpy(w, p + i, 32);
        h[0] = round(h[0], w[0]); h[1] = round(h[1], w[1]); h[2] = round(h[2], w[2]); h[3] = round(h[3], w[3]);
    }
    uint64_t tail[4] = { 0, 0, 0, 0 };
    if (i < n) { std::memcpy(tail, p + i, n - i); for (int k = 0; k < 4; ++k) h[k] = round(h[k], tail[k]); }
    uint64_t r = ((h[0] << 1) | (h[0] >> 63)) ^ ((h[1] << 7) | (h[1] >> 57)) ^ ((h[2] << 12) | (h[2] >> 52)) ^ ((h[3] << 18) | (h[3] >> 46));
    r ^= r >> 33; r *= K2; r ^= r >> 29; r *= K1; r ^= r >> 32;
    return r;
}

// What the three uploads begin with: the resident scene is being replaced (it holds none until upload_geometry has finished), and the
// textures' dimensions and blend modes as layout_textures takes them.  A texture without texels -- pixels.is_empty() -- samples as
// TRANSPARENT and takes no room in the pool.
namespace {
struct TexDims {
    std::vector<uint32_t> w, h, bl;
    void set(uint32_t i, uint32_t width, uint32_t height, uint32_t blend, bool has_texels) { w[i] = has_texels ? width : 0u; h[i] = has_texels ? height : 0u; bl[i] = blend; }
};
}
static int upload_begin(b32_ctx* c, const void* tex, uint32_t nt, TexDims& d) {
    if (!c || (nt && !tex)) return B32_E_ARG;
    { const int rc = edit_begin(c); if (rc) return rc; }
    c->scene.have_scene = false;
    d.w.resize(nt); d.h.resize(nt); d.bl.resize(nt);
    return B32_OK;
}

int b32_scene_upload(b32_ctx* c, const B32Vertex* v, uint32_t nv, const B32Face* f, uint32_t nf, const B32Texture15* tex, uint32_t nt) {
    TexDims d;
    { const int rcb = upload_begin(c, tex, nt, d); if (rcb) return rcb; }
    for (uint32_t i = 0; i < nt; ++i) d.set(i, tex[i].width, tex[i].height, tex[i].blend_mode, tex[i].pixels != nullptr);
    const std::vector<uint32_t>&w = d.w, &h = d.h, &bl = d.bl;
    // texture cache: the same set as the pool holds (pointer, size, blend mode, content hash of every texture)?
    std::vector<TexSig> sig(nt);
    for (uint32_t i = 0; i < nt; ++i) sig[i] = { tex[i].pixels, w[i], h[i], bl[i], hash_bytes(tex[i].pixels, (size_t)w[i] * h[i] * 2) };
    bool hit = c->scene.tex_sig_valid && !(c->route_off & B32_ROUTE_TEX_CACHE) && c->scene.tex_sig.size() == nt && c->scene.nt == nt && c->scene.d_texels && c->scene.d_tex;
    for (uint32_t i = 0; hit && i < nt; ++i) {
        const TexSig& o = c->scene.tex_sig[i];
        hit = o.ptr == sig[i].ptr && o.w == sig[i].w && o.h == sig[i].h && o.blend == sig[i].blend && o.hash == sig[i].hash;
    }
    int rc;
    if (!hit) {
        size_t total = 0;
        rc = layout_textures(c, nt, w.data(), h.data(), bl.data(), &total);
        if (rc) return rc;
        c->scene.cheap_ok = true;
        for (uint32_t i = 0; i < nt; ++i) {
            const size_t n = (size_t)w[i] * h[i];
            if ((rc = h2d(c, c->scene.d_texels + c->scene.h_tex[i].offset, tex[i].pixels, n * 2))) return rc;
            size_t skippable = 0;                                               // texels the black_transparent rule can skip
            const uint16_t* px = tex[i].pixels;
            for (size_t k = 0; k < n; ++k) skippable += (px[k] & 0x7FFF) == 0;
            if (n == 0 || skippable * c->cheap_den > n) c->scene.cheap_ok = false;
        }
        c->scene.tex_sig.swap(sig); c->scene.tex_sig_valid = true;
    }
    return upload_geometry(c, v, nv, f, nf, false);
}

int b32_scene_upload_rgba(b32_ctx* c, const B32Vertex* v, uint32_t nv, const B32Face* f, uint32_t nf, const B32Texture* tex, uint32_t nt) {
    TexDims d;
    { const int rcb = upload_begin(c, tex, nt, d); if (rcb) return rcb; }
    for (uint32_t i = 0; i < nt; ++i) d.set(i, tex[i].width, tex[i].height, tex[i].blend_mode, tex[i].pixels != nullptr);
    const std::vector<uint32_t>&w = d.w, &h = d.h;
    size_t total = 0;
    int rc = layout_textures(c, nt, w.data(), h.data(), d.bl.data(), &total, true);
    if (rc) return rc;
    c->scene.cheap_ok = true;
    bool blend_texels = false;
    for (uint32_t i = 0; i < nt; ++i) {
        const size_t n = (size_t)w[i] * h[i];
        if ((rc = h2d(c, c->scene.d_texels32 + c->scene.h_tex[i].offset, tex[i].pixels, n * 4))) return rc;
        size_t skippable = 0;                                               // Erase texels: the fragment is skipped (render.rs:1348)
        for (size_t k = 0; k < n; ++k) {
            const uint8_t b = tex[i].pixels[k * 4 + 3];
            skippable += b == B32_BLEND_ERASE;
            blend_texels |= b != B32_BLEND_OPAQUE && b != B32_BLEND_ERASE;
        }
        if (n == 0 || skippable * c->cheap_den > n) c->scene.cheap_ok = false;
    }
    c->scene.blend_texels8 = blend_texels;
    return upload_geometry(c, v, nv, f, nf, true);
}

int b32_scene_upload_indexed(b32_ctx* c, const B32Vertex* v, uint32_t nv, const B32Face* f, uint32_t nf, const B32IndexedTexture* tex, uint32_t nt) {
    TexDims d;
    { const int rcb = upload_begin(c, tex, nt, d); if (rcb) return rcb; }
    for (uint32_t i = 0; i < nt; ++i) d.set(i, tex[i].width, tex[i].height, tex[i].blend_mode, tex[i].indices && tex[i].clut);
    const std::vector<uint32_t>&w = d.w, &h = d.h;
    size_t total = 0;
    int rc = layout_textures(c, nt, w.data(), h.data(), d.bl.data(), &total);
    if (rc) return rc;
    c->scene.cheap_ok = true;
    for (uint32_t i = 0; i < nt; ++i) {
        const size_t n = (size_t)w[i] * h[i];
        if (!n) { c->scene.cheap_ok = false; continue; }
        // the expansion kernel also counts the texels the black_transparent rule can skip (no walk over the texels on the host)
        uint8_t* d_idx = nullptr; uint16_t* d_clut = nullptr; uint32_t* d_cnt = nullptr;
        Scratch tmp(c);
        // ONE texture with at most 256 palette entries: index bytes and CLUT stay on the device behind each other -- 256 Color15 entries
        // (zero behind the palette, which is what Clut::lookup returns for an index past it, types.rs:390-397), then the indices -- so that
        // the fused kernel can stage them in LDS (B32_ROUTE_LDS_ATLAS); the expansion below reads the same copies
        const bool keep = nt == 1 && tex[i].clut_len <= 256u && n <= (160u << 10);
        if (keep) {
            if ((rc = ensure(c, c->scene.d_atlas0, c->scene.cap_atlas0, (size_t)ATLAS_CLUT_BYTES + n + 32))) return rc;
            HIPCHK(c, hipMemsetAsync(c->scene.d_atlas0, 0, ATLAS_CLUT_BYTES, c->stream));
            if ((rc = h2d(c, c->scene.d_atlas0, tex[i].clut, (size_t)tex[i].clut_len * 2))) return rc;
            if ((rc = h2d(c, c->scene.d_atlas0 + ATLAS_CLUT_BYTES, tex[i].indices, n))) return rc;
            HIPCHK(c, hipMemsetAsync(c->scene.d_atlas0 + ATLAS_CLUT_BYTES + n, 0, 32, c->stream));      // (the staging copy reads whole 16-byte quads)
            d_clut = reinterpret_cast<uint16_t*>(c->scene.d_atlas0); d_idx = c->scene.d_atlas0 + ATLAS_CLUT_BYTES;
            c->scene.atlas_idx_bytes = (uint32_t)n;
            c->scene.h_clut.assign(ATLAS_CLUT_BYTES / 2, 0);                                            // (what b32_scene_patch_indexed compares a partial patch's CLUT with)
            std::copy(tex[i].clut, tex[i].clut + tex[i].clut_len, c->scene.h_clut.begin());
        } else {
            if ((rc = tmp.upload(tex[i].indices, n, &d_idx))) return rc;
            if ((rc = tmp.upload(tex[i].clut, (size_t)tex[i].clut_len, &d_clut))) return rc;
        }
        if ((rc = tmp.alloc(&d_cnt, 1))) return rc;
        HIPCHK(c, hipMemsetAsync(d_cnt, 0, 4, c->stream));
        launch_expand_indexed(c->stream, d_idx, (uint32_t)n, d_clut, tex[i].clut_len, c->scene.d_texels + c->scene.h_tex[i].offset, d_cnt);
        uint32_t skippable = 0;
        HIPCHK(c, hipMemcpyAsync(&skippable, d_cnt, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if ((size_t)skippable * c->cheap_den > n) c->scene.cheap_ok = false;
    }
    return upload_geometry(c, v, nv, f, nf, false);
}

// ------------------------------------------------------------------ scene slots (several resident scenes per context)
int b32_scene_create(b32_ctx* c, b32_scene** out) {
    if (!c || !out) return B32_E_ARG;
    *out = new b32_scene();
    return B32_OK;
}
void b32_scene_destroy(b32_ctx* c, b32_scene* sl) {
    if (!c || !sl) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    sl->release();
    delete sl;
}
int b32_scene_swap(b32_ctx* c, b32_scene* sl) {
    if (!c || !sl) return B32_E_ARG;
    // a pending frame of the outgoing scene that may have to be redrawn (pair overflow, long transparent lists) is settled first:
    // the redraw needs that scene.  Frames of small meshes never redraw and stay in flight.
    // Its error, if any, is the frame's error: kept for the b32_frame_finish that ends the frame (the exchange itself goes ahead).
    { const int rc = settle_pending(c); if (rc) return rc; }
    std::swap(c->scene, *sl);
    return B32_OK;
}

// ------------------------------------------------------------------ bones (b32_pose.hip has the kernels and the why)
int b32_scene_set_rig(b32_ctx* c, b32_scene* slot, const uint16_t* bone_of_vertex) {
    if (!c) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    const uint32_t nv = sc ? sc->body_nv() : 0u;        // (bone octahedra behind the mesh are not skinned: bone_index None)
    if (!sc || (nv && !bone_of_vertex)) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    int rc;
    sc->have_rig = false;
    sc->h_bones.clear();                                 // (until the next pose the vertices are the rest ones: a patch copies)
    if ((rc = ensure(c, sc->d_rest, sc->cap_rest, (size_t)nv * 6 + 1))) return rc;
    if ((rc = ensure(c, sc->d_bone_of, sc->cap_bone_of, (size_t)nv + 1))) return rc;
    // (on the stream: behind the upload or the pose that wrote the vertices, in front of the next pose)
    launch_pose_rest(c->stream, sc->d_verts, nv, sc->d_rest);
    HIPCHK(c, hipGetLastError());
    if (nv) HIPCHK(c, hipMemcpyAsync(sc->d_bone_of, bone_of_vertex, (size_t)nv * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // the caller may reuse its array (once per rig, like an upload)
    sc->have_rig = true;
    return B32_OK;
}
// Order against the side stream (DESIGN.md section 7d has the full argument).  Two kernels read a scene's vertices or what was derived
// from them there: k_setup of a pipelined frame (the vertices) and the early k_wire_bin (the wire list k_setup wrote, not the vertices).
// enqueue_frame's hand_over step, the call right behind launch_setup, makes the main stream wait for that k_setup -- by ev_setup, by
// k_join, or by the fused kernel that polls the hand-over itself (where the event cannot be recorded it drains the side stream before it
// returns the error) -- and its wire_phases step launches the wire kernels, which wait for k_wire_bin (ev_wbin or the polled word), on
// the main stream; no return lies between launch_setup and hand_over.  So everything on the side stream that a pose could overtake is in front of main-stream work enqueued
// earlier, and the pose, enqueued on the main stream, needs no event of its own.  The other direction is side_dirty: the next pipelined
// k_setup waits for the main stream as it stands after the pose.
int b32_scene_pose(b32_ctx* c, b32_scene* slot, const B32Bone* bones, uint32_t n_bones) {
    if (!c) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    if (!sc || !sc->have_rig || (n_bones && !bones)) return B32_E_ARG;
    if (n_bones > B32_MAX_BONES) return B32_E_UNSUPPORTED;
    { const int rc = edit_begin(c); if (rc) return rc; }
    launch_pose(c->stream, sc->d_rest, sc->d_bone_of, sc->d_verts, sc->body_nv(), bones, n_bones);
    HIPCHK(c, hipGetLastError());
    sc->h_bones.assign(bones, bones + n_bones);          // (b32_scene_patch_vertices poses a patched rest vertex with it)
    vertices_moved(*sc, edit_words(c));
    return B32_OK;
}
// ------------------------------------------------------------------ the bone octahedra (b32_skeleton.hip has the kernel and the why)
// The drawn octahedra of a table, in order, the creation preview last: where liveness is decided, once (b32_skeleton_body.h).
static uint32_t skeleton_octs(const B32SkelBone* bones, uint32_t n_bones, const B32SkeletonStyle& st, SkelOct* octs) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_bones; ++i) if (skel_bone_oct(bones[i], st, i, octs[n])) ++n;
    if (skel_preview_oct(st, octs[n])) ++n;
    return n;
}
static int skeleton_check(const B32SkelBone* bones, uint32_t n_bones, const B32SkeletonStyle* st) {
    if (!st || (n_bones && !bones) || st->mode > 1u) return B32_E_ARG;
    return n_bones > B32_MAX_BONES ? B32_E_UNSUPPORTED : B32_OK;
}
int b32_skeleton_counts(const B32SkelBone* bones, uint32_t n_bones, const B32SkeletonStyle* style, uint32_t* n_vertices, uint32_t* n_faces) {
    { const int rc = skeleton_check(bones, n_bones, style); if (rc) return rc; }
    SkelOct octs[SKEL_MAX_OCTS];
    const uint32_t n = skeleton_octs(bones, n_bones, *style, octs);
    if (n_vertices) *n_vertices = n * SKEL_OCT_VERTS;
    if (n_faces) *n_faces = n * SKEL_OCT_FACES;
    return B32_OK;
}
// Ordering against the side stream is b32_scene_pose's (above); the slot's derived state is tail_rebuilt's.
int b32_scene_build_skeleton(b32_ctx* c, b32_scene* slot, const B32SkelBone* bones, uint32_t n_bones, const B32SkeletonStyle* style) {
    if (!c) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    if (!sc) return B32_E_ARG;
    { const int rc = skeleton_check(bones, n_bones, style); if (rc) return rc; }
    SkelOct octs[SKEL_MAX_OCTS];
    const uint32_t n_octs = skeleton_octs(bones, n_bones, *style, octs);
    { const int rc = edit_begin(c); if (rc) return rc; }
    const uint32_t bv = sc->body_nv(), bf = sc->body_nf(), nv = bv + n_octs * SKEL_OCT_VERTS, nf = bf + n_octs * SKEL_OCT_FACES;
    int rc;
    if ((rc = ensure_keep(c, sc->d_verts, sc->cap_verts, (size_t)nv + 1, bv))) return rc;
    if ((rc = ensure_keep(c, sc->d_faces, sc->cap_faces, (size_t)nf + 1, bf))) return rc;
    if (!sc->d_consts) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&sc->d_consts), 16 * sizeof(uint32_t)));
    uint32_t tail_blend_faces = 0;                       // the face rule for the tail: editor_alpha < 255 is all an octahedron blends by
    for (uint32_t k = 0; k < n_octs; ++k) tail_blend_faces += octs[k].alpha < 255 ? SKEL_OCT_FACES : 0u;
    if ((rc = ensure_work(c, nf))) return rc;
    launch_skeleton_mesh(c->stream, octs, n_octs, sc->d_verts, bv, sc->d_faces, bf, sc->d_consts);
    HIPCHK(c, hipGetLastError());
    const bool same_nf = sc->nf == nf;
    sc->nv = nv; sc->nf = nf;
    tail_rebuilt(*sc, edit_words(c), same_nf, nv - bv, nf - bf, tail_blend_faces, sc->fmt8);
    return B32_OK;
}
int b32_skeleton_items(const B32SkelBone* bones, uint32_t n_bones, const B32SkeletonStyle* style, B32WorldItem* out, uint32_t cap, uint32_t* n_out) {
    if (!n_out) return B32_E_ARG;
    *n_out = 0;
    { const int rc = skeleton_check(bones, n_bones, style); if (rc) return rc; }
    uint32_t count = 0;
    const auto put = [&](const B32WorldItem& it) { if (out && count < cap) out[count] = it; ++count; };
    const auto colour = [](B32WorldItem& it, uint32_t r, uint32_t g, uint32_t b) { it.r = (uint8_t)r; it.g = (uint8_t)g; it.b = (uint8_t)b; it.blend = B32_BLEND_OPAQUE; it.alpha = 255; };
    for (uint32_t i = 0; i < n_bones; ++i) {                    // draw_skeleton, skeleton.rs:70-79
        const uint32_t parent = bones[i].parent;
        if (parent == B32_BONE_NONE) continue;
        B32WorldItem it{};
        for (int k = 0; k < 3; ++k) { it.p0[k] = parent < n_bones ? bones[parent].pos[k] : 0.0f; it.p1[k] = bones[i].pos[k]; }
        const uint32_t rgb = skel_colour(SKEL_COL_HIERARCHY_LINE);
        colour(it, rgb & 255u, (rgb >> 8) & 255u, (rgb >> 16) & 255u);
        it.kind = B32_LINE_2D; it.flags = B32_WORLD_CLIP_NEAR;
        put(it);
    }
    for (uint32_t i = 0; i < n_bones; ++i) {                    // draw_bone_dots, skeleton.rs:110-143: the tip, then the base
        const bool tip_hovered = style->hovered_tip >= 0 && (uint32_t)style->hovered_tip == i;
        const bool hovered = style->hovered_bone >= 0 && (uint32_t)style->hovered_bone == i;
        const bool selected = style->selected_bone >= 0 && (uint32_t)style->selected_bone == i;
        B32WorldItem tip{}, base{};
        skel_tip(bones[i], tip.p0);
        tip.kind = B32_PRIM_CIRCLE; tip.size = tip_hovered ? 11 : (selected ? 8 : 5);
        if (tip_hovered) colour(tip, 255, 180, 80); else if (selected) colour(tip, 80, 255, 80); else colour(tip, 220, 220, 230);
        put(tip);
        for (int k = 0; k < 3; ++k) base.p0[k] = bones[i].pos[k];
        base.kind = B32_PRIM_CIRCLE; base.size = hovered ? 11 : (selected ? 8 : 5);
        if (hovered) colour(base, 100, 180, 255); else if (selected) colour(base, 80, 255, 80); else colour(base, 150, 150, 160);
        put(base);
    }
    *n_out = count;
    return B32_OK;
}
int b32_scene_read_vertices(b32_ctx* c, b32_scene* slot, uint32_t first, uint32_t count, B32Vertex* out) {
    if (!c) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    if (!sc || (count && !out) || (unsigned long long)first + count > sc->nv) return B32_E_ARG;
    if (!count) return B32_OK;
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipMemcpyAsync(out, sc->d_verts + first, (size_t)count * sizeof(B32Vertex), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}
int b32_scene_read_faces(b32_ctx* c, b32_scene* slot, uint32_t first, uint32_t count, B32Face* out) {
    if (!c) return B32_E_ARG;
    b32_scene* sc = scene_of(c, slot);
    if (!sc || (count && !out) || (unsigned long long)first + count > sc->nf) return B32_E_ARG;
    if (!count) return B32_OK;
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipMemcpyAsync(out, sc->d_faces + first, (size_t)count * sizeof(B32Face), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}

// RasterTimings of a synchronous call: the per-phase split comes from the device-side phase clock (b32_frame_finish); the wall time of
// the whole call is reported as draw_ms only for an empty mesh, where no kernel ran.
static void wall_timing(b32_ctx* c, B32Timings* out, std::chrono::steady_clock::time_point t0) {
    if (!out || c->profile_level >= 2 || out->draw_ms > 0.0f || out->cull_ms > 0.0f) return;      // (the device phase clock filled them)
    out->draw_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
int b32_render_scene_15(b32_ctx* c, const B32Camera* cam, const B32Settings* st, const B32Fog* fog, B32Timings* out) {
    if (!c) return B32_E_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = b32_render_scene_15_async(c, cam, st, fog);
    if (rc == B32_OK) rc = b32_frame_finish(c, out);
    if (rc == B32_OK) wall_timing(c, out, t0);
    return rc;
}

int b32_render_scene(b32_ctx* c, const B32Camera* cam, const B32Settings* st, B32Timings* out) {
    if (!c) return B32_E_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = b32_render_scene_async(c, cam, st);
    if (rc == B32_OK) rc = b32_frame_finish(c, out);
    if (rc == B32_OK) wall_timing(c, out, t0);
    return rc;
}

int b32_render_mesh(b32_ctx* c, const B32Vertex* v, uint32_t nv, const B32Face* f, uint32_t nf, const B32Texture* tex, uint32_t nt,
                    const B32Camera* cam, const B32Settings* st, B32Timings* out) {
    if (!c || !cam || !st || !c->fb) return B32_E_ARG;
    int rc = validate_settings(st);
    if (rc) return rc;
    c->defer_upload_sync = true;
    stage_begin(c);
    rc = b32_scene_upload_rgba(c, v, nv, f, nf, tex, nt);
    stage_flush(c);
    c->defer_upload_sync = false;
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    rc = b32_render_scene(c, cam, st, out);
    if (rc != B32_OK) (void)hipStreamSynchronize(c->stream);      // the caller's buffers must be free of pending copies on every exit
    return rc;
}

int b32_render_mesh_15(b32_ctx* c, const B32Vertex* v, uint32_t nv, const B32Face* f, uint32_t nf, const B32Texture15* tex, uint32_t nt,
                       const B32Camera* cam, const B32Settings* st, const B32Fog* fog, B32Timings* out) {
    if (!c || !cam || !st || !c->fb) return B32_E_ARG;
    int rc = validate_settings(st);
    if (rc) return rc;
    c->defer_upload_sync = true;
    stage_begin(c);
    rc = b32_scene_upload(c, v, nv, f, nf, tex, nt);
    stage_flush(c);
    c->defer_upload_sync = false;
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    rc = b32_render_scene_15(c, cam, st, fog, out);
    if (rc != B32_OK) (void)hipStreamSynchronize(c->stream);      // the caller's buffers must be free of pending copies on every exit
    return rc;
}

}  // extern "C"
