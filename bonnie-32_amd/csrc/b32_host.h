// b32_host.h -- what the translation units of the C ABI share: an uploaded scene (b32_scene), a frame set (FrameSet), the context that
// holds one resident scene and up to three frame sets as members of those types (b32_ctx), the allocation helpers, and the handful of
// functions one unit calls in another.  A buffer of a scene or of a frame set is named in ONE free list, the struct's release().
// Internal: nothing here is part of include/b32raster.h.
//   b32_api.hip    context, stream, framebuffer calls, test taps and switches
//   b32_scene.hip  uploads (drop-in and resident), scene slots, the synchronous drop-in calls
//   b32_frame.hip  one frame: route, enqueue, two / three frames in flight, b32_frame_finish
//   b32_batch.hip  b32_frame_begin / _add_scene / _end (merged runs)
#pragma once
#include "b32_device.h"
#include "b32_frame_plan.h"
#include "b32_scene_state.h"
#include <algorithm>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <vector>

using namespace b32;
#ifndef B32_MIN_TILE_H
#define B32_MIN_TILE_H 8
#endif

namespace {
constexpr int EV_RING = 64;     // frames of per-phase events kept between two b32_frame_finish calls
constexpr int EV_PER_FRAME = 6; // start | setup | sort | bin | cover | shade+blend
}

// Everything k_setup WRITES for one frame and the fill kernels read: a context owns two or three of these so that the setup kernel of
// frame i + 1 can run on a second stream beside the fill of frame i (see pipeline_begin).  b32_ctx::cur is the set of the frame being
// enqueued; b32_ctx::alt holds the other ones, oldest first (rotate_sets exchanges whole structs).
// cap_work is the element count the per-face buffers of THIS set were allocated for and travels with them.  b32_ctx::cap_work is what
// the mesh needs (it also sizes the per-face buffers all sets share): ensure_work brings `cur` to it, pipeline_ensure -- which runs before
// every rotate_sets -- brings each `alt` in use to it, so the set a frame is enqueued on always has cap_work == b32_ctx::cap_work.
struct FrameSet {
    uint32_t* keys0 = nullptr; CovRec* crecs = nullptr; ShadeRec* srecs = nullptr; AuxRec* xrecs = nullptr;     // painter's keys, per-face records (b32_device.h)
    uint32_t* spans = nullptr; uint32_t* partials = nullptr; size_t cap_work = 0;
    uint32_t* face_of = nullptr;        // record slot -> face id (k_setup packs each wave's survivors to the front of its 64 slots)
    float* shades = nullptr; size_t cap_shades = 0;
    // direct binning (DirectBin, b32_device.h): k_setup appends to fixed tile regions; the regions grow when a frame overflowed one
    uint32_t* direct_lists = nullptr; size_t cap_direct = 0;
    uint32_t* tile_fill = nullptr; size_t cap_tile_fill = 0;      // FILL_PAD words per tile, zero between frames
    WireTri* wire = nullptr; size_t cap_wire = 0;           // (frames with wireframe phases: k_setup writes the wire list, the wire kernels behind the fill read it)
    uint32_t *wire_fill = nullptr, *wire_lists = nullptr; size_t cap_wire_tiles = 0;   // (... and its tile lists, WireArgs: binned beside the previous frame's fill)
    unsigned long long wire_grid = 0;                                                   // tile grid the (self-resetting) counters belong to
    Ctrl* d_ctrl = nullptr;
    hipEvent_t ev_setup = nullptr;                         // k_setup finished (side stream)
    bool in_flight = false;                                  // a frame was enqueued on this set since the last b32_frame_finish
    // Frees the buffers and leaves the set empty (the caller has drained both streams).  The control block, the event and in_flight
    // survive: pipeline_ensure re-sizes a set that stays in use; b32_destroy releases those two for all three sets.
    void release() {
        for (void* p : { (void*)keys0, (void*)crecs, (void*)srecs, (void*)xrecs, (void*)spans, (void*)face_of, (void*)partials, (void*)shades,
                         (void*)direct_lists, (void*)tile_fill, (void*)wire, (void*)wire_fill, (void*)wire_lists }) if (p) (void)hipFree(p);
        FrameSet e; e.d_ctrl = d_ctrl; e.ev_setup = ev_setup; e.in_flight = in_flight;
        *this = e;
    }
};

// Host records on their way to the device: a batch too large for a kernel argument is copied into a pinned ring slot (the caller may reuse
// its array at once) and from there to `dev` on the stream (stage_records); a slot is written again LINE_RING batches later, after its copy
// has left (normally long ago).
constexpr uint32_t LINE_RING = 4;
template <class Rec>
struct Staged {
    Rec* host[LINE_RING] = {}; size_t cap_host[LINE_RING] = {}; hipEvent_t ev[LINE_RING] = {}; uint32_t slot = 0;
    Rec* dev = nullptr; size_t cap_dev = 0;
    void release() {
        for (uint32_t k = 0; k < LINE_RING; ++k) { if (ev[k]) (void)hipEventDestroy(ev[k]); if (host[k]) (void)hipHostFree(host[k]); }
        if (dev) (void)hipFree(dev);
    }
};
// What one ordered tile pass (b32_draw_pass.h) keeps in the context: its staged records, and counters / lists / long_list of the tile
// route (DrawArgs).
template <class Rec>
struct DrawPassState : Staged<Rec> {
    uint32_t *counters = nullptr, *lists = nullptr, *long_list = nullptr; size_t cap_tiles = 0; uint32_t parity = 0;
    unsigned long long tile_batches = 0, scan_batches = 0;
    void release() {
        Staged<Rec>::release();
        for (void* p : { (void*)counters, (void*)lists, (void*)long_list }) if (p) (void)hipFree(p);
    }
};

// Texture cache of the drop-in calls ("texture upload may be cached by (ptr,len,hash) but must be semantically per-call"):
// what the texel pool currently holds -- per texture the caller's pointer, its dimensions, blend mode and a 64-bit hash of its
// content.  A call that passes the same set again (the reference's callers pass the same Texture15 slice every frame) skips the
// texel copies and the skippable-texel count; any change of pointer, size or content re-uploads.
struct TexSig { const void* ptr; uint32_t w, h, blend; uint64_t hash; };

// Everything that belongs to ONE uploaded scene: b32_ctx::scene is the resident one, a slot of b32_scene_swap (or a merged mesh of a
// batched frame) another; b32_scene_swap exchanges whole structs.  What is per context (the routes' switches, h_consts, last_direct,
// epoch, the frame sets) is not here.
struct b32_scene : b32::SceneState {    // (SceneState, b32_scene_state.h: what is derived from the content below and dies when it changes)
    B32Vertex* d_verts = nullptr; size_t cap_verts = 0;
    B32Face* d_faces = nullptr; size_t cap_faces = 0;
    uint16_t* d_texels = nullptr; size_t cap_texels = 0;
    uint32_t* d_texels32 = nullptr; size_t cap_texels32 = 0;   // 8-bit-colour path: Color texels
    TexDesc* d_tex = nullptr; size_t cap_tex = 0;
    std::vector<TexDesc> h_tex;
    uint32_t* d_consts = nullptr;       // (h_consts on the device: the face count the first radix pass reads)
    uint8_t* d_atlas0 = nullptr; size_t cap_atlas0 = 0;       // indexed upload of ONE texture: CLUT (512 B) + index bytes (atlas_idx_bytes), kept for the LDS route
    uint32_t* d_texmask = nullptr; size_t cap_texmask = 0;       // skip mask of the texel pool (FillArgs.texmask), rebuilt when the pool changes (mask_dirty)
    uint32_t pool_texels = 0;
    uint32_t nv = 0, nf = 0, nt = 0;
    bool have_scene = false;
    bool fmt8 = false;                  // uploaded by b32_scene_upload_rgba (render_mesh path)
    bool blend_texels8 = false;         // 8-bit path: some texel blends (the texels' part of blend8, which stays when b32_room_build_mesh replaces the faces)
    bool cheap_ok = false;              // every texture has few skippable texels: CHEAP coverage + repair is profitable
    bool tex_blend_any = false;         // some texture has a blend mode other than Opaque
    // packed vertex streams of a resident mesh (k_pack_streams: nv positions of 12 B, then nv (u, v, rgba) of 12 B; pos_valid, lit_valid):
    // built on the second frame of an uploaded mesh too large for the in-kernel list collection
    float* d_pos12 = nullptr; size_t cap_pos12 = 0;
    // min / max of the BODY's positions as six orderable keys (OverlayBounds, b32_overlay_body.h; bounds_valid): reduced on the device by the
    // first b32_draw_object_overlays / b32_scene_bounds that reads them after the vertices moved (scene_bounds_ensure); allocated on first use
    OverlayBounds* d_bounds = nullptr;
    std::vector<TexSig> tex_sig;        // (tex_sig_valid)
    // bones (b32_scene_set_rig, have_rig): the rest stream (nv positions and normals, 24 B each) k_pose starts from, and a bone index per
    // vertex.  Part of the scene's content: swapped with it; the buffers stay for the next rig when the geometry is replaced
    float* d_rest = nullptr; size_t cap_rest = 0; uint16_t* d_bone_of = nullptr; size_t cap_bone_of = 0;
    // the bone octahedra (b32_scene_build_skeleton): the last tail_v of the nv vertices and the last tail_f of the nf faces.  Everything
    // that draws reads nv / nf; what the reference does to mesh objects only (rig, pose, hover, box selection, pick, selection overlays)
    // reads body_nv() / body_nf().
    // in-place edits (b32_scene_patch_*, b32_patch.hip): what they need of the slot on the host.  h_bones: the table of the last
    // b32_scene_pose (empty before the first one and after b32_scene_set_rig), with which a patched rest vertex is posed.  h_faces: the
    // body's faces, fetched by the first face patch after the geometry was replaced (one synchronisation) and kept up to date, and
    // their tally.  h_texels32: the Color pool of an 8-bit-colour scene, fetched by its first texel patch, and how many of its texels
    // blend (blend_texels8).  h_clut: the kept CLUT of an index atlas (atlas_idx_bytes != 0), 256 entries
    std::vector<B32Bone> h_bones;
    std::vector<B32Face> h_faces; b32::FaceTally tally;
    std::vector<uint32_t> h_texels32; size_t blend_texel_count = 0;
    std::vector<uint16_t> h_clut;
    uint32_t body_nv() const { return nv - tail_v; }
    uint32_t body_nf() const { return nf - tail_f; }
    // The only list of a scene's device buffers (the caller has drained the streams that use them).
    void release() {
        for (void* p : { (void*)d_verts, (void*)d_faces, (void*)d_texels, (void*)d_texels32, (void*)d_tex, (void*)d_consts, (void*)d_texmask,
                         (void*)d_pos12, (void*)d_atlas0, (void*)d_rest, (void*)d_bone_of, (void*)d_bounds }) if (p) (void)hipFree(p);
    }
};

// The modeler's polygons over a slot's vertices (b32_topology_create, b32_hover.hip).
struct b32_topology {
    b32::HoverHalfEdge* he = nullptr;           // nh half-edges in loop order (half-edge h sits at position h of poly_verts)
    b32::HoverFanTri* fan = nullptr;            // nt fan triangles in loop order
    uint32_t* poly_start = nullptr;             // np + 1
    uint32_t* poly_verts = nullptr;             // nh
    uint32_t np = 0, nh = 0, nt = 0, ne = 0;    // polygons, half-edges, fan triangles, distinct normalised edges
    std::vector<uint32_t> h_poly_start;         // np + 1 on the host: where the overlay's records lie (overlay_layout)
};

// The world editor's current room (b32_room_create, b32_room.hip): one record per sector face on the device.
struct b32_room {
    B32SectorFace* faces = nullptr;             // n records on the device
    uint32_t n = 0;
    B32RoomGrid grid{};                         // travels in the kernel argument: an update is ordered by the launch that follows it
    // the render mesh: materials and per record {first vertex, first face} on the device; on the host what decides where a record's
    // output lies (kind, normal_mode) and which faces can blend (blend_mode, the two texture ids), and the prefix sums (n + 1 entries)
    B32FaceMaterial* mats = nullptr; uint2* first = nullptr; bool have_mats = false;
    std::vector<uint8_t> h_kind, h_mode, h_blend; std::vector<uint32_t> h_tex; std::vector<uint2> h_first;
    uint32_t own_blend_faces = 0;               // faces whose own blend mode puts them in the transparent pass
    // the 48 bytes of the room's last b32_room_hover[_async], copied on the stream behind k_room_hover_resolve: what
    // b32_draw_room_overlay reads with hover_source 1
    void* d_hover = nullptr; bool have_hover = false;
};

// A resident sky (b32_sky_create, b32_api.hip): the offsets generate_mesh adds to the camera position, with their colours, and the faces.
struct b32_sky {
    b32_ctx* owner = nullptr;                   // the context it was created on: every other one answers B32_E_ARG
    B32SkyVertex* verts = nullptr; uint32_t* faces = nullptr; uint32_t nv = 0, nf = 0;
    float2* proj = nullptr;                     // nv projected points: written by every b32_render_sky, sized at create
    Staged<B32SkyVertex> ring;                  // b32_sky_update's pinned ring (its copies land in `verts`; ring.dev stays empty)
};

// Device words that stay armed between two calls (armed_ensure).
struct ArmedWords { void* p = nullptr; size_t cap = 0; };
// HIP events around the kernels of the last call of its kind enqueued while profiling was on (b32_last_kernel_times); created on first use.
struct EventPair {
    hipEvent_t ev[2] = {}; bool timed = false;
    hipError_t begin(hipStream_t s) {
        for (hipEvent_t& e : ev) if (!e) { const hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return r; }
        return hipEventRecord(ev[0], s);
    }
    hipError_t end(hipStream_t s) { const hipError_t r = hipEventRecord(ev[1], s); if (r == hipSuccess) timed = true; return r; }
    bool elapsed(float* ms) const { return timed && hipEventSynchronize(ev[1]) == hipSuccess && hipEventElapsedTime(ms, ev[0], ev[1]) == hipSuccess; }   // (waits)
    void destroy() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

struct b32_ctx {
    int device = 0;
    int n_cu = 256;
    int last_hip = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    // two frames in flight: the setup kernel of the next frame on `side` beside the fill of the current one on `stream`
    hipStream_t side = nullptr; hipEvent_t ev_main = nullptr, ev_wbin = nullptr;     // (ev_wbin: a pipelined frame's k_wire_bin finished on the side stream)
    FrameSet cur;                        // the frame set of the frame being enqueued
    FrameSet alt[2];                     // the other frame sets, oldest first (allocated on first use; alt[1] only with three sets)
    uint32_t n_sets_user = 0;            // what b32_set_pipeline_depth asked for (0: the library's own choice, see auto_depth in b32_api.hip)
    uint32_t n_sets = 2;                 // b32_set_pipeline_depth: 2 = setup(i+1) beside fill(i); 3 = setup(i+2) beside fill(i), so that the
                                         // setup kernel a fill waits for ended a whole fill ago (fills back to back; measured slower: the two
                                         // kernels then share the CUs all the time and the frame is bound by their summed VALU work)
    bool side_dirty = true;              // something k_setup reads was written on `stream` since the side stream last waited for it
    hipStream_t join_stream = nullptr; bool join_ok = false;   // k_flag / k_join instead of an event: only while `stream` and `side` have DIFFERENT priorities (then they never share a hardware queue); checked per main stream
    uint32_t gate_permille = 0;          // b32_set_pipeline_gate: hold the next setup kernel until the previous fill's tile cursor has got this far (0: only until that fill has started -- the frame sets' order, k_gate)
    uint32_t wire_seq = 0;               // WireArgs::epoch of the last frame with wireframe phases (never 0)
    bool start_lost = false;             // fault injection: the last fused kernel was told not to publish its start (the next start gate waits 2 ms only)
    uint32_t join_seq = 0;               // FillArgs::join_seq of the last polled hand-over (never 0)
    uint32_t fill_seq = 0;               // FillArgs::start_seq of the last fused kernel launched (never 0)
    bool pipe_hint = true;               // the previous frame's route could use the second frame set
    struct CoverOf { const Ctrl* ctrl; uint32_t tiles, groups, seq; } cover_of[3] = {};   // the last fused kernel of each frame set (keyed by its control block; tiles 0: the set's last
                                                                                      // frame had none), written by remember_cover: the gate polls the cursor of the frame n_sets - 1 back
    bool pipelined = false;              // the frame being enqueued runs its k_setup on the side stream
    unsigned long long pipelined_frames = 0;
    unsigned long long flag_join_frames = 0, event_join_frames = 0, poll_join_frames = 0;    // ... handed over to the fill by k_flag / k_join, or by a cross-stream event
    uint32_t inject = 0;                 // b32_debug_inject: fault injection for the tests of the failure paths

    // framebuffer
    uint32_t width = 0, height = 0;
    uint32_t* fb_own = nullptr; size_t fb_own_px = 0;
    uint32_t* fb = nullptr; bool fb_external = false;
    uint32_t band_y0 = 0, band_y1 = 0; bool band_set = false;
    float* zbuf = nullptr; size_t cap_zbuf = 0; bool zbuf_valid = false;   // Framebuffer::zbuffer; !valid == every entry f32::MAX

    // multi-GPU band exchange (b32_gather.hip): mappings of the root's framebuffer / epoch words (band rank), or the root's own epoch words
    void* band_fb_ipc = nullptr; uint32_t* band_sync_own = nullptr; uint32_t* band_sync = nullptr;      // (band_sync_own: inside fb_own's tail)
    uint32_t band_rank = 0; bool band_attached = false;

    b32_scene scene;                    // the resident scene (b32_scene_swap exchanges it with a slot)
    int count_fragments = 0;            // 1: exact fragment-store count every frame (EXACT coverage); instrumentation, off by default
    bool last_exact = false;            // the last frame ran EXACT coverage in painter's mode (B32Timings.fragments is exact)

    // per-face work buffers shared by all frame sets (the keyed routes' sort and binning: launches on the main stream only)
    size_t cap_work = 0;                // elements the resident mesh needs: these buffers' size and every frame set's in use (see FrameSet)
    uint32_t *keys1 = nullptr, *vals[2] = { nullptr, nullptr };   // (keys1: the radix passes' second key buffer beside cur.keys0)
    uint32_t* counts = nullptr; uint32_t* block_sums = nullptr; uint32_t bin_blocks = 0;
    uint32_t* tile_mid = nullptr; size_t cap_tile_mid = 0;
    bool last_local_sort = false;       // the last frame took the fast path (draw order not materialised)
    uint32_t route_off = 0;             // b32_set_routes: B32_ROUTE_* bits switched off (tests keep the older pipelines covered with it)
    uint32_t cheap_den = 64;            // b32_set_cheap_threshold
    // pairs
    size_t cap_pairs = 0;
    uint32_t* inline_lists = nullptr; size_t cap_inline = 0;      // small meshes: one list region per tile, filled inside k_cover
    bool last_direct = false;           // the last frame took the direct-binning route
    uint32_t epoch = 0;                 // DirectBin / FillArgs::epoch of the last direct-binned frame (never 0).  Both per context: not part of a scene slot
    // Framebuffer::clear deferred (b32_fb_clear): applied by the next frame's fused kernel when that frame takes the sort-free path in
    // painter's mode on the same band, else by a clear launch before whatever touches the framebuffer next (flush_clear)
    bool clear_pending = false; uint32_t clear_rgba = 0, clear_y0 = 0, clear_y1 = 0;
    unsigned long long routes[8] = {};                            // b32_route_count
    unsigned long long lds_atlas_frames = 0;
    uint32_t *pkeys[2] = { nullptr, nullptr }, *pvals[2] = { nullptr, nullptr };
    // sort scratch
    uint32_t* block_hist = nullptr; uint32_t hist_blocks = 0; uint32_t* digit_total = nullptr;
    uint32_t partial_blocks = 0;
    // tiles
    uint32_t* ranges = nullptr; size_t cap_ranges = 0;
    uint32_t* vis = nullptr; size_t cap_vis = 0;
    // wireframe phases (allocated on first use; the wire list and its tile lists belong to the frame set)
    uint32_t *wire_owner = nullptr, *wire_first = nullptr; size_t cap_wire_table = 0;
    unsigned long long wire_tile_frames = 0;
    DrawPassState<B32Line> lines;                                 // b32_draw_lines
    DrawPassState<B32Prim> prims;                                 // b32_draw_prims
    // b32_draw_world: the items' pinned ring and device copy (the projected records are written into prims.dev and drawn as a primitive
    // batch); drawn / dropped / rejected on the device; HIP events around the last projection kernel enqueued while profiling was on
    // (b32_last_kernel_times "world_project")
    Staged<B32WorldItem> world;
    Staged<B32Star> stars;                                        // b32_draw_stars: the pinned ring and device copy of a batch of more than STAR_SMALL stars
    Staged<uint32_t> patch;                                       // b32_scene_patch_*: the records' (or the rectangle's) pinned ring and device copy, in dwords
    ArmedWords world_counts;
    unsigned long long world_tile_batches = 0, world_scan_batches = 0;
    EventPair world_timer;
    // b32_draw_gizmos: the rows' pinned ring and device copy (as `world`), the rows of the batch being validated, the entry's own counts
    Staged<GizmoRow> gizmo; std::vector<GizmoRow> gizmo_rows;
    ArmedWords gizmo_counts;
    unsigned long long span_cover_frames = 0;                     // frames whose opaque coverage used exact row intervals (B32_ROUTE_SPAN_COVER)
    // control
    Ctrl h_ctrl{}; Stamps h_stamps{};          // host copies of the frame set's control block (FrameSet::d_ctrl: Ctrl followed by Stamps)
    uint32_t h_consts[4] = { 0, 0, 0, 0 };   // staging for scene.d_consts (outlives the async copy)
    bool defer_upload_sync = false;            // drop-in calls: the frame's own synchronisation covers the uploads
    // staged upload of the drop-in calls (see UploadSegs): the caller's slices are packed into a pinned arena on the host and one
    // kernel moves them; active only inside b32_render_mesh[_15], which always synchronise before they return
    unsigned char* stage_host = nullptr; void* stage_dev = nullptr; size_t stage_cap = 0, stage_used = 0;
    bool stage_active = false, stage_failed = false; UploadSegs stage_segs{};
    B32Light* d_lights = nullptr; size_t cap_lights = 0; std::vector<B32Light> h_lights;

    // batched frame (b32_frame_begin / _add_scene / _end): per-mesh rows of the frame being enqueued (kept for a redraw), the recording
    // between begin and end, and the merged meshes built so far (reused while their members' contents stay the same)
    bool frame_batched = false; MeshTable frame_table{};
    bool frame_placed = false; PlaceTable frame_places{};      // placements of the frame being enqueued (row 0: a draw on its own), kept for a redraw like the rows
    struct BatchEntry { b32_scene* slot; MeshRow row; bool wire; bool placed; B32Placement place; };
    struct MergedRun { std::vector<b32_scene*> members; std::vector<unsigned long long> gens; b32_scene* merged = nullptr; unsigned long long used = 0; };
    bool batch_open = false; B32Camera batch_cam{}; B32Settings batch_st{}; std::vector<B32Light> batch_lights; std::vector<BatchEntry> batch;
    std::vector<MergedRun> merged_runs; unsigned long long batch_clock = 0, gen_counter = 0;
    unsigned long long batch_stats[4] = {};      // merged draws, sequential draws, merged meshes built, frames
    // last enqueued frame (for redraw after a pair overflow)
    bool frame_pending = false;
    bool pending_superseded = false;    // safe mode: a b32_fb_clear of the whole band was issued behind the pending frame -- every pixel (and depth) that frame
                                        // drew is overwritten, so the NEXT frame may be enqueued without settling it (a redraw of it could not be seen)
    bool pending_may_redraw = false;    // the pending frame took a path that can overflow its buffers (not the small-mesh path)
    bool deep_async = false;            // b32_set_async_depth(1): large-scene frames are enqueued back to back, a dropped one is reported
    bool redrawing = false;             // enqueue_frame is repeating the pending frame (k_setup must not count it as lost)
    int deferred_rc = 0;                // error of a frame that b32_scene_swap had to settle: reported by the next b32_frame_finish
    B32Timings settled_tm{}; bool settled_valid = false;   // ... and its counters, for a b32_frame_finish that finds no later frame pending
    B32Camera last_cam{}; B32Settings last_settings{}; B32Fog last_fog{}; bool last_has_fog = false;

    // asynchronous framebuffer downloads (b32_fb_download_async): ticket t completes with event dl_ev[t % DL_RING]
    static constexpr uint32_t DL_RING = 8;
    hipEvent_t dl_ev[DL_RING] = {}; unsigned long long dl_seq = 0;
    // ... through a device-side snapshot: the frame is copied to dl_stage[t % 2] on the context's stream (microseconds) and leaves for the host
    // from there on dl_stream, so that the NEXT frame's kernels do not wait for the PCIe transfer
    hipStream_t dl_stream = nullptr; hipEvent_t dl_snap[2] = {}; uint32_t* dl_stage[2] = {}; size_t dl_stage_px = 0;
    // b32_pick_meshes[_async] (b32_pick.hip): the three minima per item (all ones between two picks), the table of a pick too large for
    // the kernel argument, PICK_RING device result buffers in turn (pick_done: the resolve kernel wrote it, main stream; pick_left: its
    // transfer has left, dl_stream), the blocking form's page-locked landing buffer, HIP events around the last pick enqueued while
    // profiling was on (b32_last_kernel_times "pick")
    static constexpr uint32_t PICK_RING = 4;
    ArmedWords pick_words;
    Staged<PickItem> pick_tab;
    void* pick_res[PICK_RING] = {}; size_t pick_cap_res[PICK_RING] = {}; hipEvent_t pick_done[PICK_RING] = {}, pick_left[PICK_RING] = {}; uint32_t pick_slot = 0;
    void* pick_host = nullptr; size_t pick_cap_host = 0;
    EventPair pick_timer;
    // b32_hover_mesh / b32_box_select[_async] (b32_hover.hip): the front pass's vertex bitmap and, behind it, its edge bitmap (all zero
    // between two calls), the minima of a hover (HoverWords, all ones between two calls), HIP events around the last hover enqueued while
    // profiling was on (b32_last_kernel_times "hover").  Results leave through the pick's ring of result buffers.
    ArmedWords hover_bits, hover_words;
    EventPair hover_timer;
    // b32_room_hover / b32_room_box_select[_async] (b32_room.hip): the three sets of minima of a room hover (all ones between two calls) and
    // the device copy of a box selection's points.  Results leave through the pick's ring of result buffers.
    ArmedWords room_words, room_points;
    // b32_draw_mesh_overlay (b32_overlay.hip): the projected vertices of the call being enqueued, the bounds' keys (armed between two
    // calls), the selected list's pinned ring and device copy (as `world`)
    uint4* overlay_tab = nullptr; size_t overlay_cap_tab = 0;     // (16 bytes per vertex: OverlayPoint)
    void* overlay_bounds = nullptr;
    Staged<uint32_t> overlay_sel; std::vector<uint32_t> overlay_pairs;
    // b32_draw_object_overlays / b32_scene_bounds (b32_object_overlay.hip): the slots whose bounds the call being enqueued reduces, and how
    // many reductions were launched since the context was created (b32_route_count 20).  The rows travel in overlay_pairs / overlay_sel.
    std::vector<b32_scene*> bounds_stale; unsigned long long bounds_reductions = 0;
    // profiling
    int profile_level = 0;
    uint32_t prof_stride = 1, prof_seq = 0;      // b32_set_profiling_stride: events on every prof_stride-th frame only
    hipEvent_t ev[EV_RING][EV_PER_FRAME] = {};
    bool ev_created = false;
    uint32_t ev_frames = 0;             // frames recorded since the last finish
    float phase_ms[5] = { 0, 0, 0, 0, 0 }; // averages of the last finished batch: setup, sort, bin, cover, shade
    uint32_t phase_frames = 0;
    int phase_level = 0;                // profiling level those averages were taken at
    std::vector<B32Light> keep_lights;  // private copy of the last frame's lights (redraw after overflow)
};

#define HIPCHK(ctx, expr)                                                 \
    do {                                                                  \
        hipError_t _e = (expr);                                           \
        if (_e != hipSuccess) { (ctx)->last_hip = (int)_e; return B32_E_HIP; } \
    } while (0)

template <typename T>
static int ensure(b32_ctx* c, T*& p, size_t& cap, size_t need) {
    if (need <= cap && p) return B32_OK;
    c->side_dirty = true;
    if (p) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(p)); p = nullptr; cap = 0; }
    size_t n = need + need / 4 + 16;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)));
    cap = n;
    return B32_OK;
}
// ensure() for a buffer whose first `keep` elements stay (b32_scene_build_skeleton: the body in front of a growing tail): the new
// allocation is filled by a copy on the device, on the stream behind whatever wrote the old one, and the old one is freed after the one
// synchronisation
template <typename T>
static int ensure_keep(b32_ctx* c, T*& p, size_t& cap, size_t need, size_t keep) {
    if (need <= cap && p) return B32_OK;
    c->side_dirty = true;
    const size_t n = need + need / 4 + 16;
    T* q = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&q), n * sizeof(T)));
    T* old = p;
    if (old) {
        hipError_t e = keep ? hipMemcpyAsync(q, old, keep * sizeof(T), hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { (void)hipFree(q); c->last_hip = (int)e; return B32_E_HIP; }
    }
    p = q; cap = n;                                     // (the slot owns the new buffer before the old one goes: a failing free leaves nothing dangling)
    if (old) HIPCHK(c, hipFree(old));
    return B32_OK;
}
// Device words that stay armed between two calls (all ones, all zero: `fill`, a byte; < 0: no fill): at least `bytes` of them, allocated
// on first use and filled on the context's stream; growing waits for the stream before it frees.  Unlike ensure() it leaves side_dirty
// alone: nothing on the side stream reads these.
static int armed_ensure(b32_ctx* c, ArmedWords& w, size_t bytes, int fill) {
    if (w.p && bytes <= w.cap) return B32_OK;
    if (w.p) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(w.p)); w.p = nullptr; w.cap = 0; }
    const size_t cap = bytes + bytes / 4 + 64;
    HIPCHK(c, hipMalloc(&w.p, cap));
    w.cap = cap;
    if (fill >= 0) HIPCHK(c, hipMemsetAsync(w.p, fill, cap, c->stream));
    return B32_OK;
}
template <typename T>
static int ensure_plain(b32_ctx* c, T*& p, size_t count) {   // exact-size (re)allocation without capacity tracking
    c->side_dirty = true;
    if (p) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(p)); p = nullptr; }
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
    return B32_OK;
}

// Stage the records: a batch is copied into a pinned ring slot of `ps` (the caller may reuse its array at once) and from there on the
// stream to `dst` (device memory of the caller's, n records of room: b32_sky_update), or to ps.dev (dst == nullptr, grown to the batch).
template <class Rec>
static int stage_records(b32_ctx* c, Staged<Rec>& ps, const Rec* recs, uint32_t n, Rec* dst = nullptr) {
    const uint32_t k = ps.slot;
    ps.slot = (k + 1) % LINE_RING;
    if (ps.ev[k]) HIPCHK(c, hipEventSynchronize(ps.ev[k]));
    else HIPCHK(c, hipEventCreateWithFlags(&ps.ev[k], hipEventDisableTiming));
    if (ps.cap_host[k] < n) {
        if (ps.host[k]) HIPCHK(c, hipHostFree(ps.host[k]));
        ps.host[k] = nullptr; ps.cap_host[k] = 0;
        const size_t cap = (size_t)n + n / 4 + 64;
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&ps.host[k]), cap * sizeof(Rec), hipHostMallocDefault));
        ps.cap_host[k] = cap;
    }
    std::memcpy(ps.host[k], recs, (size_t)n * sizeof(Rec));
    int rc;
    if (!dst && (rc = ensure(c, ps.dev, ps.cap_dev, (size_t)n))) return rc;
    HIPCHK(c, hipMemcpyAsync(dst ? dst : ps.dev, ps.host[k], (size_t)n * sizeof(Rec), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(ps.ev[k], c->stream));
    return B32_OK;
}

// Scratch device allocations of ONE API call (sky / stars / present / taps): released on every exit path, error returns included,
// after the stream has drained.
struct Scratch {
    b32_ctx* c;
    std::vector<void*> ptrs;
    explicit Scratch(b32_ctx* ctx) : c(ctx) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        if (ptrs.empty()) return;
        (void)hipStreamSynchronize(c->stream);
        for (void* q : ptrs) (void)hipFree(q);
    }
    template <typename T>
    int alloc(T** out, size_t count) {
        void* q = nullptr;
        *out = nullptr;
        HIPCHK(c, hipMalloc(&q, (count ? count : 1) * sizeof(T)));
        ptrs.push_back(q);
        *out = static_cast<T*>(q);
        return B32_OK;
    }
    template <typename T>
    int upload(const T* host, size_t n, T** dev) {       // scratch copy of a small per-call input
        int rc = alloc(dev, n);
        if (rc || !n) return rc;
        HIPCHK(c, hipMemcpyAsync(*dev, host, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
        return B32_OK;
    }
};

// pinned host arena of the drop-in calls (stage_ensure, b32_scene.hip): packed uploads, and the frame's Ctrl + Stamps on the way back
constexpr size_t STAGE_BYTES = (size_t)1 << 20, STAGE_CTRL_OFF = STAGE_BYTES - 128;   // the last 128 B receive the frame's Ctrl + Stamps

// ---- shared between the units (defined in the file named); C linkage like the ABI around them, but not exported
#define B32_INTERNAL __attribute__((visibility("hidden")))
extern "C" {
B32_INTERNAL int settle_pending(b32_ctx* c);                                      // b32_api.hip
B32_INTERNAL int flush_clear(b32_ctx* c);                                         // b32_api.hip
// The next ticket (b32_fb_download_async, b32_pick_meshes_async, b32_hover_mesh_async, b32_box_select_async): its number and its event, created on first use, else waited for when
// it still belongs to the ticket DL_RING tickets ago; the transfer stream exists afterwards.  The caller records *ev on dl_stream and
// then sets dl_seq = t.
B32_INTERNAL int ticket_open(b32_ctx* c, unsigned long long& t, hipEvent_t*& ev); // b32_api.hip
B32_INTERNAL int apply_depth_auto(b32_ctx* c);                                    // b32_api.hip (b32_set_pipeline_depth(ctx, 0): the depth the library picks)
constexpr size_t FB_TAIL_BYTES = 8192;      // behind the pixels of a library-owned framebuffer: the epoch words of the band exchange (b32_gather.hip)
B32_INTERNAL void band_close_any(b32_ctx* c);                                    // b32_gather.hip
B32_INTERNAL int h2d(b32_ctx* c, void* dst, const void* src, size_t bytes);       // b32_scene.hip
B32_INTERNAL bool stage_ensure(b32_ctx* c);                                       // b32_scene.hip
B32_INTERNAL int ensure_work(b32_ctx* c, uint32_t nf);                            // b32_scene.hip
B32_INTERNAL int patch_fetch_faces(b32_ctx* c, b32_scene* sc);                    // b32_patch.hip (the body's faces on the host and their tally)
B32_INTERNAL int validate_settings(const B32Settings* st);                        // b32_frame.hip
B32_INTERNAL int enqueue_frame(b32_ctx* c, const B32Camera* cam, const B32Settings* st, const B32Fog* fog);            // b32_frame.hip
// (place: the placement of a draw on its own, or NULL; a merged run -- frame_batched -- has set frame_placed / frame_places itself)
B32_INTERNAL int render_scene_async_any(b32_ctx* c, const B32Camera* cam, const B32Settings* st, const B32Fog* fog, const B32Placement* place);   // b32_frame.hip
}
// b32_object_overlay.hip, for ObjectOverlayProducer (b32_api.hip): what object_overlay_plan reads of the call's parts; a slot's bounds
// block allocated (nothing enqueued); its row of k_scene_bounds' table; the reductions of c->bounds_stale enqueued (d_rows: their rows on
// the device in that order, nullptr: one slot, its row by value) -- the blocks armed, one launch, the caches valid, the counter moved
namespace b32 { struct ObjectPartView; }
B32_INTERNAL void object_part_views(const B32ObjectPart* parts, uint32_t n_parts, std::vector<b32::ObjectPartView>& views);
B32_INTERNAL int scene_bounds_alloc(b32_ctx* c, b32_scene* sc);
B32_INTERNAL void scene_bounds_row(const b32_scene* sc, b32::BoundsRow* r);
B32_INTERNAL int scene_bounds_run(b32_ctx* c, const b32::BoundsRow* d_rows);

// ---- editing a resident scene (the rules: b32_scene_state.h)
// The slot a call names (NULL: the resident scene), if it holds a scene.
static inline b32_scene* scene_of(b32_ctx* c, b32_scene* slot) {
    b32_scene* sc = slot ? slot : &c->scene;
    return sc->have_scene ? sc : nullptr;
}
// A slot's positions as the overlays read them on the device: the packed stream while it is current, else the B32Vertex array; `stride`
// floats between two vertices.
static inline const float* slot_positions(const b32_scene* sc, uint32_t& stride) {
    const bool packed = sc->pos_valid && sc->d_pos12;
    stride = packed ? 3u : (uint32_t)(sizeof(B32Vertex) / sizeof(float));
    return packed ? sc->d_pos12 : reinterpret_cast<const float*>(sc->d_verts);
}
// Entering an edit.  A pending frame that may still be redrawn (overflowed tile regions / pair buffers) is redrawn from the RESIDENT
// vertices, faces and texels: it is settled before any of them changes, or the redraw would draw the edited scene in its place.
static inline int edit_begin(b32_ctx* c) {
    (void)hipSetDevice(c->device);
    return settle_pending(c);
}
static inline b32::EditWords edit_words(b32_ctx* c) { return { c->gen_counter, c->side_dirty }; }
// tex_blends(t) of the tally (b32_patch_tally.h): texture t of the slot resolves and its blend mode is not Opaque.
static inline bool tex_blends(const b32_scene* sc, uint32_t t) {
    return t < sc->nt && t < sc->h_tex.size() && sc->h_tex[t].blend_mode != B32_BLEND_OPAQUE;
}
