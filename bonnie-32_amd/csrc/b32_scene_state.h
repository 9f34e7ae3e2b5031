// b32_scene_state.h -- host only (plain C++17, nothing of HIP; tests/cpp/scene_state_host.cpp walks it under the sanitizers): the state
// of a resident scene that is DERIVED from its vertices, faces and texels, and what each kind of edit does to it.  b32_scene (b32_host.h)
// inherits SceneState; every writer of a slot ends in ONE of the functions below and assigns none of these fields itself.  What makes a
// field valid again stays with the code that does the work: frame_positions (pos_valid, lit_valid, band_frames), the mask rebuild
// (mask_dirty), the direct-binning sizing and overflow handling of a frame (direct_*, local_sort_ok), patch_fetch_* (h_*_valid),
// b32_scene_set_rig (have_rig), the texture cache and the index atlas of the uploads (tex_sig_valid, atlas_idx_bytes), scene_bounds_ensure
// (bounds_valid: b32_draw_object_overlays, b32_scene_bounds, b32_object_overlay.hip).
#pragma once
#include "b32_patch_tally.h"

namespace b32 {

struct SceneState : SlotBlend {         // (the blend bookkeeping: b32_patch_tally.h)
    // packed vertex streams of a mesh too large for the in-kernel list collection (frame_positions): positions, the lit stream behind
    // them, and the frames drawn since the mesh arrived
    bool pos_valid = false, lit_valid = false; uint32_t band_frames = 0;
    bool bounds_valid = false;          // the slot's min / max keys (b32_scene::d_bounds) are those of the BODY's vertices as they are now
    // direct binning (DirectBin, b32_device.h): what the scene's frames taught about its tile regions
    uint32_t direct_cap_opaque = 0;     // opaque entries per tile region (0: sized from the mesh on first use)
    uint32_t direct_ntiles = 0;         // the tile grid that size belongs to (another grid: sized again)
    bool direct_ok = true;              // false: the regions would not fit (one tile's list too long) -> counting sort
    bool local_sort_ok = true;          // no tile list of this scene has exceeded the LDS sort capacity so far
    unsigned long long gen = 0;         // identity of the scene's content: the key of the merged-run cache (b32_batch.hip)
    bool have_rig = false;              // b32_scene_set_rig: the rest stream and the bone indices belong to these vertices
    uint32_t tail_v = 0, tail_f = 0;    // the bone octahedra: the last tail_v vertices and tail_f faces (b32_scene_build_skeleton)
    bool h_faces_valid = false;         // the host copy of the body's faces and its tally are current (patch_fetch_faces)
    bool h_texels32_valid = false;      // ... and that of an 8-bit-colour pool (patch_fetch_texels32)
    bool mask_dirty = true;             // the skip mask of the texel pool has to be rebuilt
    bool tex_sig_valid = false;         // the drop-in calls' texture cache describes the pool
    uint32_t atlas_idx_bytes = 0;       // the kept index atlas mirrors the pool (0: no atlas; the fill reads the pool)
};

// The two words of the context an edit touches.
struct EditWords {
    unsigned long long& gen_counter;    // the last content number given out
    bool& side_dirty;                   // something k_setup reads was written on the main stream since the side stream last waited for it
};

inline void set_blend(SceneState& st, const SlotBlend& b) { static_cast<SlotBlend&>(st) = b; }

// Every edit ends here: a merged run that holds the slot is rebuilt, the next pipelined k_setup waits for the main stream.
inline void content_changed(SceneState& st, EditWords w) {
    st.gen = ++w.gen_counter;
    w.side_dirty = true;
}

// Pose, vertex patch: the same mesh with vertices elsewhere.  The packed streams are packed again by the next frame; band_frames stays
// (the mesh has been drawn before: frame_positions need not wait for a second frame), and so does everything learnt about the faces.
// The bounds of the body are reduced again by the next call that reads them; uploads, room build and merged meshes end here too, so
// this is the one place that clears them.
inline void vertices_moved(SceneState& st, EditWords w) {
    st.pos_valid = false; st.lit_valid = false;
    st.bounds_valid = false;
    content_changed(st, w);
}

// Face patch: `b` is the tally's verdict (tally_slot).  Vertices, face count and host copies stay as they are.
inline void faces_edited(SceneState& st, EditWords w, const SlotBlend& b) {
    set_blend(st, b);
    content_changed(st, w);
}

// (another face count: tile regions sized afresh.  With the same count what an overflowing frame taught stays -- the per-frame drop-in
// call uploads the same mesh again and again)
inline void regions_forgotten(SceneState& st) { st.direct_cap_opaque = 0; st.direct_ntiles = 0; st.direct_ok = true; }

// b32_scene_build_skeleton: the body stays, tail_v vertices / tail_f faces behind it are written anew, tail_blend_faces of them for the
// transparent pass.  band_frames, local_sort_ok, the rig, the host copy of the BODY's faces and the BODY's bounds (no body vertex moves,
// and a grown vertex buffer receives the body by a copy) are the body's business and stay.
inline void tail_rebuilt(SceneState& st, EditWords w, bool same_nf, uint32_t tail_v, uint32_t tail_f, uint32_t tail_blend_faces, bool fmt8) {
    const bool first = !st.tail_v && !st.tail_f;
    const bool bounds = st.bounds_valid;
    set_blend(st, blend_with_tail(first ? blend_save_body(st) : st, tail_blend_faces, fmt8));
    if (!same_nf) regions_forgotten(st);
    st.tail_v = tail_v; st.tail_f = tail_f;
    vertices_moved(st, w);
    st.bounds_valid = bounds;
}

// Uploads, b32_room_build_mesh, a merged mesh: another mesh stands in the slot.  Whatever belonged to the old vertices and faces goes: rig,
// tail, the host copy of the faces, the verdict on the LDS sort, the frame count.  keep_regions: see regions_forgotten (a merged mesh
// never keeps them: its members' sum says nothing about which faces they are).
inline void geometry_replaced(SceneState& st, EditWords w, bool keep_regions, const SlotBlend& b) {
    if (!keep_regions) regions_forgotten(st);
    st.have_rig = false;
    st.tail_v = 0; st.tail_f = 0;
    st.h_faces_valid = false;
    st.local_sort_ok = true;
    st.band_frames = 0;
    set_blend(st, b);
    vertices_moved(st, w);
}

// What every rewrite of texels kills: the skip mask and the texture cache; the index atlas unless the writer patched it too.
inline void texel_caches_stale(SceneState& st, bool atlas_follows) {
    st.mask_dirty = true; st.tex_sig_valid = false;
    if (!atlas_follows) st.atlas_idx_bytes = 0;
}
// Texel patches: the pool is edited in place.  The host copy of an 8-bit-colour pool is edited with it and stays valid.
inline void texels_rewritten(SceneState& st, EditWords w, bool atlas_follows) {
    texel_caches_stale(st, atlas_follows);
    content_changed(st, w);
}
// layout_textures, a merged mesh: the pool is laid out anew, so the host copy goes too.  Not an edit of its own: the geometry_replaced
// of the same call ends it (one content number per upload).
inline void pool_replaced(SceneState& st) {
    st.h_texels32_valid = false;
    texel_caches_stale(st, false);
}

}  // namespace b32
