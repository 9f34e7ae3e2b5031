// b32_patch_tally.h -- host only, in a form a stand-alone program can include (tests/cpp/patch_tally_host.cpp, built with the sanitizers):
// the record rules of b32_scene_patch_* and the blend rule -- what a slot's faces, textures and tail say about its transparent pass.
// Every writer of a slot (b32_scene_state.h) takes its blend bookkeeping from here: an upload counts the faces once (tally_faces), a face
// patch keeps the count incrementally (tally_face), the room mesh counts from its own tables.
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

// The face rule as three counters over the BODY's faces:
//   own    faces whose own blend mode or editor alpha puts them in the transparent pass (may_blend)
//   any    ... counting the faces a texture's blend mode puts there too (blend_faces; render.rs:2403-2415)
//   alpha  faces with editor_alpha < 255 (the 8-bit path's blend8)
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

// The slot's blend bookkeeping (b32::SceneState inherits it): may_blend, blend8 and blend_faces of the whole slot, and the same three of
// the body alone, which mean something only while there is a tail.
struct SlotBlend {
    bool may_blend = true;              // some face / texture can produce a transparent-pass surface (render.rs:2403-2415)
    bool blend8 = false;                // 8-bit path: some texel blends or some face has editor_alpha < 255 -> ordered walk
    uint32_t blend_faces = 0;           // faces that their own blend mode / editor alpha or their texture's blend mode puts in the transparent pass
    bool body_may_blend = false, body_blend8 = false; uint32_t body_blend_faces = 0;
};
// THE blend rule: what a mesh without a tail whose faces count `body` leaves.  `cur` is what the slot holds now: an RGB555 mesh leaves
// blend8 alone, an 8-bit-colour one sets may_blend = false, and neither touches the body_* copies.
inline SlotBlend blend_fresh(const FaceTally& body, const SlotBlend& cur, bool fmt8, bool any_texture_blends, bool blend_texels8) {
    SlotBlend s = cur;
    s.blend_faces = body.any;
    s.may_blend = fmt8 ? false : (body.own != 0 || any_texture_blends);
    if (fmt8) s.blend8 = blend_texels8 || body.alpha != 0;
    return s;
}
// ... and a tail behind it (b32_scene_build_skeleton) with tail_faces transparent-pass faces: s.body_* hold the body's three, the slot's
// are body + tail.  An octahedron blends by editor_alpha alone: blend8 on the 8-bit path, may_blend on the RGB555 one.
inline SlotBlend blend_with_tail(SlotBlend s, uint32_t tail_faces, bool fmt8) {
    s.blend_faces = s.body_blend_faces + tail_faces;
    if (fmt8) s.blend8 = s.body_blend8 || tail_faces != 0;
    else s.may_blend = s.body_may_blend || tail_faces != 0;
    return s;
}
inline SlotBlend blend_save_body(SlotBlend s) {     // the first tail of a mesh: what the slot holds is the body's
    s.body_may_blend = s.may_blend; s.body_blend8 = s.blend8; s.body_blend_faces = s.blend_faces;
    return s;
}
// The slot after its body's faces were edited: as a fresh upload of them, followed by the same b32_scene_build_skeleton, leaves it.  The
// tail's part is the difference between the slot's and the body's face count.
inline SlotBlend tally_slot(const FaceTally& body, const SlotBlend& cur, bool fmt8, bool any_texture_blends, bool blend_texels8, bool has_tail) {
    if (!has_tail) return blend_fresh(body, cur, fmt8, any_texture_blends, blend_texels8);
    const SlotBlend held{ cur.body_may_blend, cur.body_blend8, cur.body_blend_faces };
    const SlotBlend b = blend_fresh(body, held, fmt8, any_texture_blends, blend_texels8);    // the rule on the body's three ...
    SlotBlend s = cur;
    s.body_may_blend = b.may_blend; s.body_blend8 = b.blend8; s.body_blend_faces = b.blend_faces;
    return blend_with_tail(s, cur.blend_faces - cur.body_blend_faces, fmt8);                 // ... and the same tail on top again
}

}  // namespace b32
