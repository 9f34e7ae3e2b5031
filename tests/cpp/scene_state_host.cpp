// scene_state_host.cpp -- the rules of csrc/b32_scene_state.h against what the eleven writers of a resident scene assigned by hand before
// the rules existed, in a program of its own for a build with the address and undefined-behaviour sanitizers.  Every writer is carried
// twice: `old_*` is the earlier code's assignments as literal statements on one SceneState, `new_*` is the call the library makes now on
// a second one.  Every sequence of four writers (11^4) is walked several times with parameters drawn from their edge values -- the face
// count the same or another, a tail or none, translucent bones or none, RGB555 or 8-bit colour, blending textures or none, a texture
// cache hit, a kept index atlas -- and with a "frames were drawn, host copies fetched, a rig set" step in between that makes everything
// valid again.  After every step the two states and the two context words must be equal field by field.  A merged mesh lives in a slot of
// its own that only build_merged and the frames write (b32_batch.hip), so it is a second pair of states here as well.
// Prints "ok" and returns 0, or says which sequence, step and field differed.
#include <cstdio>
#include "b32_scene_state.h"

using namespace b32;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {       // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return n ? (uint32_t)(z % n) : 0u;
}
static bool coin() { return rnd(2) != 0; }

struct Words { unsigned long long gen_counter = 0; bool side_dirty = true; };
// What a slot holds beside the derived state and both versions of a writer read or write alike.
struct Content { uint32_t nf = 0; bool fmt8 = false, tex_blend_any = false, blend_texels8 = false; FaceTally tally; };
// One step's parameters, drawn once and given to both versions.
struct Params {
    uint32_t nf; FaceTally tally; bool tex_blends, blend_texels, hit, keep_atlas; uint32_t n_octs, dim_octs;
    bool members_may_blend; uint32_t members_blend_faces;
};
static Params draw(const Content& k, const SceneState& st, bool cached_upload) {
    Params p{};
    p.tex_blends = coin();
    p.hit = cached_upload && st.tex_sig_valid && coin();    // (the cache can only hit while it is valid, and then the textures are the pool's)
    if (p.hit) p.tex_blends = k.tex_blend_any;
    p.nf = coin() ? k.nf : 8u + rnd(3) * 9000u;
    p.tally.own = coin() ? 0u : 1u + rnd(3);
    p.tally.any = p.tally.own + (p.tex_blends && coin() ? 2u : 0u);
    p.tally.alpha = p.tally.own && coin() ? 1u : 0u;
    p.blend_texels = coin(); p.keep_atlas = coin();
    p.n_octs = coin() ? 0u : 1u + rnd(2); p.dim_octs = p.n_octs && coin() ? 1u : 0u;
    p.members_may_blend = coin(); p.members_blend_faces = p.members_may_blend ? 5u : 0u;
    return p;
}

// ---------------------------------------------------------------- the earlier code, statement by statement
static SlotBlend old_tally_slot(const FaceTally& body, const SlotBlend& cur, bool fmt8, bool any_texture_blends, bool blend_texels8, bool has_tail) {
    SlotBlend s = cur;
    const uint32_t tail_faces = has_tail ? cur.blend_faces - cur.body_blend_faces : 0u;
    const uint32_t faces = body.any;
    const bool may_blend = fmt8 ? false : (body.own != 0 || any_texture_blends);
    const bool blend8 = fmt8 ? (blend_texels8 || body.alpha != 0) : cur.blend8;
    if (has_tail) {
        s.body_blend_faces = faces; s.body_may_blend = may_blend; s.body_blend8 = fmt8 ? blend8 : cur.body_blend8;
        s.blend_faces = faces + tail_faces;
        if (fmt8) s.blend8 = blend8 || tail_faces != 0;
        else s.may_blend = may_blend || tail_faces != 0;
    } else {
        s.blend_faces = faces; s.may_blend = may_blend; s.blend8 = blend8;
    }
    return s;
}
static void old_apply_tally(SceneState& o, const Content& k) {
    const SlotBlend cur{ o.may_blend, o.blend8, o.blend_faces, o.body_may_blend, o.body_blend8, o.body_blend_faces };
    const SlotBlend s = old_tally_slot(k.tally, cur, k.fmt8, k.tex_blend_any, k.blend_texels8, o.tail_v != 0 || o.tail_f != 0);
    o.may_blend = s.may_blend; o.blend8 = s.blend8; o.blend_faces = s.blend_faces;
    o.body_may_blend = s.body_may_blend; o.body_blend8 = s.body_blend8; o.body_blend_faces = s.body_blend_faces;
}
static void old_layout_textures(SceneState& o) {
    o.atlas_idx_bytes = 0;
    o.h_texels32_valid = false;
    o.mask_dirty = true;
}
static void old_upload_geometry(SceneState& o, Words& w, const Content& k, const Params& p) {
    o.may_blend = p.tally.own != 0; o.blend_faces = p.tally.any;
    w.side_dirty = true;                                    // (h2d)
    if (k.nf != p.nf) { o.direct_cap_opaque = 0; o.direct_ntiles = 0; o.direct_ok = true; }
    o.have_rig = false;
    o.tail_v = 0; o.tail_f = 0;
    o.h_faces_valid = false;
    o.local_sort_ok = true;
    o.pos_valid = false; o.lit_valid = false; o.band_frames = 0;
    o.gen = ++w.gen_counter;
}
static void old_upload(SceneState& o, Words& w, const Content& k, const Params& p) {
    if (!p.hit) {
        o.tex_sig_valid = false;
        old_layout_textures(o);
        o.tex_sig_valid = true;
    }
    old_upload_geometry(o, w, k, p);
    if (p.tex_blends) o.may_blend = true;
}
static void old_upload_rgba(SceneState& o, Words& w, const Content& k, const Params& p) {
    o.tex_sig_valid = false;
    old_layout_textures(o);
    old_upload_geometry(o, w, k, p);
    o.blend8 = p.blend_texels || p.tally.alpha != 0;
    o.may_blend = false;
}
static void old_upload_indexed(SceneState& o, Words& w, const Content& k, const Params& p) {
    o.tex_sig_valid = false;
    old_layout_textures(o);
    if (p.keep_atlas) o.atlas_idx_bytes = 4096;
    old_upload_geometry(o, w, k, p);
    if (p.tex_blends) o.may_blend = true;
}
static void old_room_build_mesh(SceneState& o, Words& w, const Content& k, const Params& p) {      // (p.tally: own faces, with the textures', alpha 0)
    o.blend_faces = p.tally.any;
    if (k.fmt8) { o.may_blend = false; o.blend8 = k.blend_texels8; }
    else o.may_blend = p.tally.own != 0 || k.tex_blend_any;
    if (k.nf != p.nf) { o.direct_cap_opaque = 0; o.direct_ntiles = 0; o.direct_ok = true; }
    o.have_rig = false;
    o.tail_v = 0; o.tail_f = 0;
    o.h_faces_valid = false;
    o.local_sort_ok = true;
    o.pos_valid = false; o.lit_valid = false; o.band_frames = 0;
    o.gen = ++w.gen_counter;
    w.side_dirty = true;
}
static void old_build_merged(SceneState& m, Words& w, const Params& p) {
    m.may_blend = false; m.blend_faces = 0;
    m.may_blend |= p.members_may_blend; m.blend_faces += p.members_blend_faces;
    m.mask_dirty = true;
    m.blend8 = false; m.local_sort_ok = true;
    m.direct_cap_opaque = 0; m.direct_ntiles = 0; m.direct_ok = true; m.pos_valid = false; m.lit_valid = false; m.band_frames = 0;
    m.tex_sig_valid = false; m.gen = ++w.gen_counter;
    w.side_dirty = true;
}
static void old_pose(SceneState& o, Words& w) {
    w.side_dirty = true;
    o.pos_valid = false; o.lit_valid = false;
    o.gen = ++w.gen_counter;
}
static void old_build_skeleton(SceneState& o, Words& w, const Content& k, uint32_t nf, uint32_t tail_v, uint32_t tail_f, uint32_t nb) {
    if (!o.tail_v && !o.tail_f) { o.body_blend_faces = o.blend_faces; o.body_may_blend = o.may_blend; o.body_blend8 = o.blend8; }
    o.blend_faces = o.body_blend_faces + nb;
    if (k.fmt8) o.blend8 = o.body_blend8 || nb != 0;
    else o.may_blend = o.body_may_blend || nb != 0;
    if (k.nf != nf) { o.direct_cap_opaque = 0; o.direct_ntiles = 0; o.direct_ok = true; }
    o.tail_v = tail_v; o.tail_f = tail_f;
    o.pos_valid = false; o.lit_valid = false;
    w.side_dirty = true;
    o.gen = ++w.gen_counter;
}
static void old_patch_changed(SceneState& o, Words& w) {
    w.side_dirty = true;
    o.gen = ++w.gen_counter;
}
static void old_patch_vertices(SceneState& o, Words& w) {
    o.pos_valid = false; o.lit_valid = false;
    old_patch_changed(o, w);
}
static void old_patch_faces(SceneState& o, Words& w, const Content& k) {       // (k.tally: the patched tally; the fetch made the host copy valid)
    o.h_faces_valid = true;
    old_apply_tally(o, k);
    old_patch_changed(o, w);
}
static void old_patch_texels(SceneState& o, Words& w, const Content& k, bool blend_texels_flipped) {
    if (k.fmt8) o.h_texels32_valid = true;
    if (blend_texels_flipped) { o.h_faces_valid = true; old_apply_tally(o, k); }
    o.atlas_idx_bytes = 0;
    o.mask_dirty = true; o.tex_sig_valid = false;
    old_patch_changed(o, w);
}
static void old_patch_indexed(SceneState& o, Words& w, bool clut_kept, bool whole, bool same_clut) {
    bool keep = o.atlas_idx_bytes != 0 && clut_kept;
    if (o.atlas_idx_bytes && !keep) o.atlas_idx_bytes = 0;
    if (keep && !whole && !same_clut) { o.atlas_idx_bytes = 0; keep = false; }
    o.mask_dirty = true; o.tex_sig_valid = false;
    old_patch_changed(o, w);
}

// ---------------------------------------------------------------- the comparison
static const char* differ(const SceneState& a, const SceneState& b, const Words& wa, const Words& wb) {
#define SAME(f) if (a.f != b.f) return #f
    SAME(may_blend); SAME(blend8); SAME(blend_faces); SAME(body_may_blend); SAME(body_blend8); SAME(body_blend_faces);
    SAME(pos_valid); SAME(lit_valid); SAME(band_frames); SAME(direct_cap_opaque); SAME(direct_ntiles); SAME(direct_ok); SAME(local_sort_ok);
    SAME(gen); SAME(have_rig); SAME(tail_v); SAME(tail_f); SAME(h_faces_valid); SAME(h_texels32_valid); SAME(mask_dirty); SAME(tex_sig_valid);
    SAME(atlas_idx_bytes);
#undef SAME
    if (wa.gen_counter != wb.gen_counter) return "gen_counter";
    if (wa.side_dirty != wb.side_dirty) return "side_dirty";
    return nullptr;
}
// Frames were drawn: everything a frame makes valid or learns (frame_positions, the mask rebuild, the direct-binning sizing and overflow
// handling, the side stream's wait).
static void frames_drawn(SceneState& s, Words& w, uint32_t bits) {
    s.pos_valid = true; s.lit_valid = (bits & 1u) != 0; s.band_frames += 2;
    s.direct_cap_opaque = 777; s.direct_ntiles = 300; s.direct_ok = (bits & 2u) != 0; s.local_sort_ok = (bits & 4u) != 0;
    s.mask_dirty = false;
    w.side_dirty = false;
}
// ... and what the calls between two edits make valid on a slot: b32_scene_set_rig, patch_fetch_faces / _texels32.
static void slot_settled(SceneState& s, bool fmt8, uint32_t bits) {
    s.have_rig = (bits & 8u) != 0; s.h_faces_valid = (bits & 16u) != 0; s.h_texels32_valid = fmt8 && (bits & 32u) != 0;
}

enum Writer { UPLOAD, UPLOAD_RGBA, UPLOAD_INDEXED, ROOM_BUILD_MESH, BUILD_MERGED, POSE, BUILD_SKELETON, PATCH_VERTICES, PATCH_FACES, PATCH_TEXELS,
              PATCH_INDEXED, N_WRITERS };

struct World {
    SceneState o, n, mo, mn;            // the slot and the merged mesh, earlier code and rules
    Words wo, wn;
    Content k;
};

static void step(World& W, int writer) {
    const Params p = draw(W.k, W.o, writer == UPLOAD);             // (only b32_scene_upload has the texture cache)
    const EditWords ew{ W.wn.gen_counter, W.wn.side_dirty };
    Content& k = W.k;
    switch (writer) {
    case UPLOAD: case UPLOAD_RGBA: case UPLOAD_INDEXED: {
        const bool fmt8 = writer == UPLOAD_RGBA;
        if (writer == UPLOAD) old_upload(W.o, W.wo, k, p);
        else if (writer == UPLOAD_RGBA) old_upload_rgba(W.o, W.wo, k, p);
        else old_upload_indexed(W.o, W.wo, k, p);
        if (!p.hit) {                                       // layout_textures and the format's own middle
            pool_replaced(W.n);
            k.tex_blend_any = p.tex_blends;
            if (writer == UPLOAD) W.n.tex_sig_valid = true;
            if (writer == UPLOAD_INDEXED && p.keep_atlas) W.n.atlas_idx_bytes = 4096;
        }
        if (fmt8) k.blend_texels8 = p.blend_texels;
        geometry_replaced(W.n, ew, k.nf == p.nf, blend_fresh(p.tally, W.n, fmt8, k.tex_blend_any, k.blend_texels8));
        k.nf = p.nf; k.fmt8 = fmt8; k.tally = p.tally;
        break;
    }
    case ROOM_BUILD_MESH: {
        Params q = p;
        q.tally.alpha = 0;                                  // (a room's faces have editor_alpha 255)
        if (!k.tex_blend_any) q.tally.any = q.tally.own;
        old_room_build_mesh(W.o, W.wo, k, q);
        geometry_replaced(W.n, ew, k.nf == q.nf, blend_fresh(q.tally, W.n, k.fmt8, k.tex_blend_any, k.blend_texels8));
        k.nf = q.nf; k.tally = q.tally;
        break;
    }
    case BUILD_MERGED: {
        old_build_merged(W.mo, W.wo, p);
        SlotBlend blend = W.mn;
        blend.may_blend = p.members_may_blend; blend.blend8 = false; blend.blend_faces = p.members_blend_faces;
        pool_replaced(W.mn);
        geometry_replaced(W.mn, ew, false, blend);
        break;
    }
    case POSE:
        old_pose(W.o, W.wo);
        vertices_moved(W.n, ew);
        break;
    case BUILD_SKELETON: {
        const uint32_t body_nf = k.nf - W.o.tail_f, nf = body_nf + p.n_octs * 8u;
        old_build_skeleton(W.o, W.wo, k, nf, p.n_octs * 6u, p.n_octs * 8u, p.dim_octs * 8u);
        tail_rebuilt(W.n, ew, k.nf == nf, p.n_octs * 6u, p.n_octs * 8u, p.dim_octs * 8u, k.fmt8);
        k.nf = nf;
        break;
    }
    case PATCH_VERTICES:
        old_patch_vertices(W.o, W.wo);
        vertices_moved(W.n, ew);
        break;
    case PATCH_FACES: {
        k.tally = p.tally;
        if (!k.tex_blend_any) k.tally.any = k.tally.own;
        old_patch_faces(W.o, W.wo, k);
        W.n.h_faces_valid = true;                           // (patch_fetch_faces)
        faces_edited(W.n, ew, tally_slot(k.tally, W.n, k.fmt8, k.tex_blend_any, k.blend_texels8, W.n.tail_v != 0 || W.n.tail_f != 0));
        break;
    }
    case PATCH_TEXELS: {
        const bool flipped = k.fmt8 && p.blend_texels != k.blend_texels8;
        if (flipped) k.blend_texels8 = p.blend_texels;
        old_patch_texels(W.o, W.wo, k, flipped);
        if (k.fmt8) W.n.h_texels32_valid = true;            // (patch_fetch_texels32)
        if (flipped) {
            W.n.h_faces_valid = true;
            set_blend(W.n, tally_slot(k.tally, W.n, k.fmt8, k.tex_blend_any, k.blend_texels8, W.n.tail_v != 0 || W.n.tail_f != 0));
        }
        texels_rewritten(W.n, ew, false);
        break;
    }
    case PATCH_INDEXED: {
        if (k.fmt8) break;                                  // (refused: B32_E_ARG, nothing changes)
        const bool clut_kept = p.keep_atlas, whole = p.blend_texels, same_clut = p.members_may_blend;
        old_patch_indexed(W.o, W.wo, clut_kept, whole, same_clut);
        bool keep = W.n.atlas_idx_bytes != 0 && clut_kept;
        if (keep && !whole && !same_clut) keep = false;
        texels_rewritten(W.n, ew, keep);
        break;
    }
    }
}

int main() {
    unsigned long long steps = 0;
    for (int seq = 0; seq < N_WRITERS * N_WRITERS * N_WRITERS * N_WRITERS; ++seq)
        for (int round = 0; round < 12; ++round) {
            World W;
            int code = seq;
            for (int s = 0; s < 4; ++s, code /= N_WRITERS) {
                step(W, code % N_WRITERS);
                ++steps;
                const char* bad = differ(W.o, W.n, W.wo, W.wn);
                if (!bad) bad = differ(W.mo, W.mn, W.wo, W.wn);
                if (bad) { std::printf("sequence %d round %d step %d (writer %d): %s differs\n", seq, round, s, code % N_WRITERS, bad); return 1; }
                if (coin()) {
                    const uint32_t bits = rnd(64);
                    frames_drawn(W.o, W.wo, bits); frames_drawn(W.n, W.wn, bits);
                    slot_settled(W.o, W.k.fmt8, bits); slot_settled(W.n, W.k.fmt8, bits);
                    if (coin()) { frames_drawn(W.mo, W.wo, bits); frames_drawn(W.mn, W.wn, bits); }
                }
            }
        }
    std::printf("ok (%llu steps)\n", steps);
    return 0;
}
