// b32_patch_tally.h -- host only: what the in-place edits of a resident scene (b32_patch.hip) decide on the host, in a form a stand-alone
// program can include (tests/cpp/patch_tally_host.cpp, built with the sanitizers): the record rules of b32_scene_patch_* and the blend
// bookkeeping upload_geometry, b32_scene_upload_rgba and b32_scene_build_skeleton (b32_scene.hip) derive from a slot's faces, kept
// incrementally while faces are patched.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/b32raster.h"

namespace b32 {

// Records of `rec_bytes` each whose first dword is the element's index: strictly ascending and below `limit` (a parallel scatter has
// no "last one wins").
inline bool patch_records_ok(const void* recs, size_t rec_bytes, uint32_t n, uint32_t limit) {
    const unsigned char* p = static_cast<const unsigned char*>(recs);
    uint32_t prev = 0;
    for (uint32_t k = 0; k < n; ++k) {
        uint32_t i;
        memcpy(&i, p + (size_t)k * rec_bytes, 4);
        if (i >= limit || (k && i <= prev)) return false;
        prev = i;
    }
    return true;
}
// A non-empty rectangle [x, x + w) x [y, y + h) inside a texture of tex_w x tex_h texels.
inline bool patch_rect_ok(uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t tex_w, uint32_t tex_h) {
    return w && h && (uint64_t)x + w <= tex_w && (uint64_t)y + h <= tex_h;
}

// upload_geometry's face loop as three counters over the BODY's faces:
//   own    faces whose own blend mode or editor alpha puts them in the transparent pass (may_blend)
//   any    ... counting the faces a texture's blend mode puts there too (blend_faces; render.rs:2403-2415)
//   alpha  faces with editor_alpha < 255 (b32_scene_upload_rgba: blend8)
struct FaceTally { uint32_t own = 0, any = 0, alpha = 0; };
// tex_blends(t): texture t resolves and its blend mode is not Opaque (the caller knows the slot's textures)
template <class TexBlends>
inline void tally_face(FaceTally& t, const B32Face& f, bool add, TexBlends tex_blends) {
    const bool own = f.blend_mode != B32_BLEND_OPAQUE || f.editor_alpha < 255;
    const bool any = own || (f.texture_id != B32_NO_TEXTURE && tex_blends(f.texture_id));
    const uint32_t d = add ? 1u : 0xFFFFFFFFu;
    if (own) t.own += d;
    if (any) t.any += d;
    if (f.editor_alpha < 255) t.alpha += d;
}
template <class TexBlends>
inline FaceTally tally_faces(const B32Face* f, uint32_t nf, TexBlends tex_blends) {
    FaceTally t;
    for (uint32_t i = 0; i < nf; ++i) tally_face(t, f[i], true, tex_blends);
    return t;
}

// The slot's blend bookkeeping (b32_scene: may_blend, blend8, blend_faces and the body_* copies kept while there is a tail).
struct SlotBlend {
    bool may_blend, blend8; uint32_t blend_faces;
    bool body_may_blend, body_blend8; uint32_t body_blend_faces;
};
// ... as a fresh upload of the body's faces, followed by the same b32_scene_build_skeleton, leaves it.  `cur` is what the slot holds
// now: an RGB555 upload leaves blend8 alone and an 8-bit-colour one sets may_blend = false; the tail's part is the difference between
// the slot's and the body's face count.
inline SlotBlend tally_slot(const FaceTally& body, const SlotBlend& cur, bool fmt8, bool any_texture_blends, bool blend_texels8, bool has_tail) {
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

}  // namespace b32
