// b32_api.hip -- the C ABI of include/b32raster.h, part 1: context, stream, device-resident framebuffer, test taps and switches.
// (Scene uploads: b32_scene.hip; frames: b32_frame.hip; batched frames: b32_batch.hip; shared declarations: b32_host.h.)
#include "b32_host.h"
#include "b32_overlay_body.h"
#include "b32_room_overlay_body.h"
#include "b32_object_overlay_body.h"

extern "C" {

const char* b32_strerror(int code) {
    switch (code) {
        case B32_OK: return "ok";
        case B32_E_ARG: return "invalid argument";
        case B32_E_INDEX: return "face references a vertex index out of range";
        case B32_E_NAN_KEY: return "NaN painter's-sort key";
        case B32_E_HIP: return "HIP runtime error";
        case B32_E_UNSUPPORTED: return "setting outside the supported hot-path scope";
        case B32_E_NO_DEVICE: return "no HIP device (the rasterizer has no CPU fallback)";
        case B32_E_FRAME_DROPPED: return "an earlier frame in flight ran out of buffer space and drew nothing (deep asynchronous mode)";
        case B32_E_BAND_TIMEOUT: return "a band exchange wait gave up: another rank did not publish / release its frame in time (the frame may hold stale rows)";
        default: return "unknown error";
    }
}

int b32_create(int device, b32_ctx** out) {
    if (!out) return B32_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return B32_E_NO_DEVICE;
    b32_ctx* c = new b32_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete c; return B32_E_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) { delete c; return B32_E_HIP; }
    c->stream = c->own_stream;
    if (hipMalloc(reinterpret_cast<void**>(&c->cur.d_ctrl), sizeof(Ctrl) + sizeof(Stamps) + sizeof(Events)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->scene.d_consts), 16 * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&c->digit_total), 4096 * sizeof(uint32_t)) != hipSuccess) { delete c; return B32_E_HIP; }
    if (hipMemset(c->cur.d_ctrl, 0, sizeof(Ctrl) + sizeof(Stamps) + sizeof(Events)) != hipSuccess) { delete c; return B32_E_HIP; }     // (`sticky` is never reset by a frame)
    *out = c;
    return B32_OK;
}

void b32_destroy(b32_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    band_close_any(c);
    if (c->side) (void)hipStreamSynchronize(c->side);
    c->scene.release();
    for (auto& r : c->merged_runs) if (r.merged) { r.merged->release(); delete r.merged; }
    for (FrameSet* a : { &c->cur, &c->alt[0], &c->alt[1] }) {
        a->release();
        if (a->d_ctrl) (void)hipFree(a->d_ctrl);
        if (a->ev_setup) (void)hipEventDestroy(a->ev_setup);
    }
    // the context's own buffers: what all frame sets and scenes share
    for (void* p : { (void*)c->fb_own, (void*)c->zbuf, (void*)c->keys1, (void*)c->vals[0], (void*)c->vals[1], (void*)c->counts, (void*)c->block_sums,
                     (void*)c->pkeys[0], (void*)c->pkeys[1], (void*)c->pvals[0], (void*)c->pvals[1], (void*)c->block_hist, (void*)c->digit_total,
                     (void*)c->ranges, (void*)c->vis, (void*)c->tile_mid, (void*)c->inline_lists, (void*)c->wire_owner, (void*)c->wire_first,
                     (void*)c->d_lights }) if (p) (void)hipFree(p);
    for (hipEvent_t e : { c->ev_main, c->ev_wbin }) if (e) (void)hipEventDestroy(e);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->ev_created) for (auto& fr : c->ev) for (auto& e : fr) if (e) (void)hipEventDestroy(e);
    c->lines.release(); c->prims.release(); c->world.release(); c->gizmo.release(); c->patch.release(); c->stars.release();
    for (ArmedWords* w : { &c->world_counts, &c->gizmo_counts, &c->pick_words, &c->hover_bits, &c->hover_words, &c->room_words, &c->room_points })
        if (w->p) (void)hipFree(w->p);
    for (EventPair* t : { &c->world_timer, &c->pick_timer, &c->hover_timer }) t->destroy();
    c->pick_tab.release();
    if (c->pick_host) (void)hipHostFree(c->pick_host);
    c->overlay_sel.release();
    if (c->overlay_tab) (void)hipFree(c->overlay_tab);
    if (c->overlay_bounds) (void)hipFree(c->overlay_bounds);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->stage_host) (void)hipHostFree(c->stage_host);
    for (hipEvent_t e : c->dl_ev) if (e) (void)hipEventDestroy(e);
    if (c->dl_stream) { (void)hipStreamSynchronize(c->dl_stream); (void)hipStreamDestroy(c->dl_stream); }
    for (hipEvent_t e : c->dl_snap) if (e) (void)hipEventDestroy(e);
    for (uint32_t* q : c->dl_stage) if (q) (void)hipFree(q);
    for (uint32_t k = 0; k < b32_ctx::PICK_RING; ++k) {                     // (behind dl_stream's last transfer)
        if (c->pick_res[k]) (void)hipFree(c->pick_res[k]);
        for (hipEvent_t e : { c->pick_done[k], c->pick_left[k] }) if (e) (void)hipEventDestroy(e);
    }
    delete c;
}

int b32_last_hip_error(const b32_ctx* c) { return c ? c->last_hip : 0; }
#ifndef B32_SRC_DIGEST
#define B32_SRC_DIGEST "unknown-digest!!"
#endif
// (the marker in front lets build.py read the digest from the file without loading it)
static const char g_build_digest[] = "B32-SRC-DIGEST:" B32_SRC_DIGEST;
const char* b32_build_digest(void) { return g_build_digest + 15; }

// A pending frame that may still need a redraw (pair overflow, long transparent lists) is settled before anything reads or rebinds
// the framebuffer, so that no caller ever sees the cleared frame of an aborted attempt.  Its error, if any, is the frame's error: kept
// for the b32_frame_finish that ends the frame, and so are its counters.
int settle_pending(b32_ctx* c) {
    if (!c->frame_pending || !c->pending_may_redraw) return B32_OK;
    B32Timings tm;
    const int rc = b32_frame_finish(c, &tm);
    if (rc == B32_E_HIP || rc == B32_E_ARG) return rc;
    if (rc && !c->deferred_rc) c->deferred_rc = rc;
    if (!rc) { c->settled_tm = tm; c->settled_valid = true; }     // "its counters are those of the most recent frame": this one, unless another follows
    return B32_OK;
}

// The deferred Framebuffer::clear as launches of its own: before anything but the sort-free frame reads or writes the framebuffer.
int flush_clear(b32_ctx* c) {
    if (!c->clear_pending) return B32_OK;
    c->clear_pending = false;
    if (!c->fb || c->clear_y1 <= c->clear_y0) return B32_OK;
    launch_clear(c->stream, c->fb + (size_t)c->clear_y0 * c->width, (size_t)c->width * (c->clear_y1 - c->clear_y0), c->clear_rgba);
    if (c->zbuf && c->zbuf_valid && (size_t)c->width * c->height <= c->cap_zbuf)        // self.zbuffer[i] = f32::MAX, render.rs:43
        launch_clear(c->stream, reinterpret_cast<uint32_t*>(c->zbuf) + (size_t)c->clear_y0 * c->width, (size_t)c->width * (c->clear_y1 - c->clear_y0), 0x7F7FFFFFu);
    HIPCHK(c, hipGetLastError());
    return B32_OK;
}

int b32_set_stream(b32_ctx* c, void* s) {
    if (!c) return B32_E_ARG;
    { const int rc = settle_pending(c); if (rc) return rc; }
    { const int rc = flush_clear(c); if (rc) return rc; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stream = s ? reinterpret_cast<hipStream_t>(s) : c->own_stream;
    c->side_dirty = true;
    return B32_OK;
}
int b32_synchronize(b32_ctx* c) {
    if (!c) return B32_E_ARG;
    { const int rc = flush_clear(c); if (rc) return rc; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}

// ------------------------------------------------------------------ framebuffer
static int fb_set_dims(b32_ctx* c, uint32_t w, uint32_t h) {
    c->width = w; c->height = h;
    if (!c->band_set) { c->band_y0 = 0; c->band_y1 = h; }
    else { if (c->band_y1 > h) c->band_y1 = h; if (c->band_y0 > c->band_y1) c->band_y0 = c->band_y1; }
    return c->n_sets_user ? B32_OK : apply_depth_auto(c);       // (the band's share of the frame decides the library's own pipeline depth)
}
static int fb_resize_any(b32_ctx* c, uint32_t w, uint32_t h, bool always_new) {
    if (!c || w == 0 || h == 0 || w > 16384 || h > 16384) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    { const int rc = settle_pending(c); if (rc) return rc; }
    { const int rcf = flush_clear(c); if (rcf) return rcf; }
    if (c->fb_external) { c->fb_external = false; c->fb = nullptr; c->width = c->height = 0; }
    if (!always_new && c->fb && c->width == w && c->height == h) return B32_OK;          // Framebuffer::resize: no-op on equal dims
    // an exported framebuffer that changes size (or is made anew) is no longer the one the ranks mapped: the epoch words sit behind the
    // pixels at an offset that depends on the size, and the old mapping may be freed below -- the root must b32_band_export again
    // (until then b32_band_wait / _release / _status return B32_E_ARG instead of touching pixels or freed memory)
    if (c->band_sync_own) { c->band_sync_own = nullptr; if (c->band_rank == 0) c->band_sync = nullptr; }
    const size_t px = (size_t)w * h;
    if (px > c->fb_own_px || !c->fb_own) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->fb_own) HIPCHK(c, hipFree(c->fb_own));
        c->fb_own = nullptr;
        c->band_sync_own = nullptr;                                          // (the epoch words of an exported framebuffer lived in the old allocation)
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->fb_own), px * 4 + 4096 + FB_TAIL_BYTES));
        c->fb_own_px = px;
    }
    c->fb = c->fb_own;
    c->band_set = false;
    c->zbuf_valid = false;                                                  // vec![f32::MAX; w*h], render.rs:22,32
    { const int rcd = fb_set_dims(c, w, h); if (rcd) return rcd; }
    HIPCHK(c, hipMemsetAsync(c->fb, 0, px * 4, c->stream));                // vec![0; w*h*4], render.rs:18-33
    return B32_OK;
}
int b32_fb_resize(b32_ctx* c, uint32_t w, uint32_t h) { return fb_resize_any(c, w, h, false); }   // Framebuffer::resize, render.rs:27-34
int b32_fb_new(b32_ctx* c, uint32_t w, uint32_t h) { return fb_resize_any(c, w, h, true); }       // Framebuffer::new, render.rs:18-25
int b32_fb_bind_device(b32_ctx* c, void* dptr, uint32_t w, uint32_t h) {
    if (!c) return B32_E_ARG;
    { const int rc = settle_pending(c); if (rc) return rc; }
    { const int rcf = flush_clear(c); if (rcf) return rcf; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!dptr) { c->fb_external = false; c->fb = nullptr; c->width = c->height = 0; return B32_OK; }
    if (w == 0 || h == 0 || w > 16384 || h > 16384 || (reinterpret_cast<uintptr_t>(dptr) & 15)) return B32_E_ARG;
    c->fb = reinterpret_cast<uint32_t*>(dptr); c->fb_external = true;
    c->band_set = false;
    c->zbuf_valid = false;
    return fb_set_dims(c, w, h);
}
int b32_fb_size(const b32_ctx* c, uint32_t* w, uint32_t* h) {
    if (!c) return B32_E_ARG;
    if (w) *w = c->width;
    if (h) *h = c->height;
    return B32_OK;
}
int b32_set_band(b32_ctx* c, uint32_t y0, uint32_t y1) {
    if (!c || !c->fb || y0 > y1 || y1 > c->height) return B32_E_ARG;
    { const int rcs = settle_pending(c); if (rcs) return rcs; }       // (a redraw of the pending frame belongs to the band it was enqueued for)
    { const int rcf = flush_clear(c); if (rcf) return rcf; }          // (a deferred clear belongs to the rows of the band it was issued for)
    c->band_y0 = y0; c->band_y1 = y1; c->band_set = !(y0 == 0 && y1 == c->height);
    if (!c->n_sets_user) return apply_depth_auto(c);        // (a narrow band runs three frame sets: b32_set_pipeline_depth)
    return B32_OK;
}
// (safe mode) a pending large-scene frame that may still need a redraw is settled before anything else WRITES the framebuffer too:
// redrawn after a clear or a sky pass it would put its pixels on top of them
static int settle_before_write(b32_ctx* c) { return c->deep_async ? B32_OK : settle_pending(c); }

int b32_fb_clear(b32_ctx* c, uint8_t r, uint8_t g, uint8_t b, uint8_t blend) {
    if (!c || !c->fb) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    // Safe mode settles a pending large-scene frame before anything writes the framebuffer -- except here: this clear covers every row the
    // pending frame can have drawn (its band; a band change settles) and resets their depths, so whether that frame was dropped or not
    // can no longer be seen.  It is marked superseded instead, and the draw that follows is enqueued behind it like in deep mode (the
    // setup kernel of the new frame beside the fill of the old one): the reference's loop -- clear, draw, clear, draw -- runs without a
    // host synchronisation per frame in the library's DEFAULT mode too.  Anything that reads the framebuffer in between still settles.
    // Only for a framebuffer that can be read through this library alone (every such read settles): memory the caller bound
    // (b32_fb_bind_device: a torch tensor, an RCCL gather) or shares with other ranks (b32_band_export / _import / _attach) is read behind
    // the library's back -- there the pending frame is settled here as before, so that an overflowing first frame is redrawn and its
    // capacities grow instead of every later frame of a clear / draw loop overflowing the same way unseen.
    const bool only_ours = !c->fb_external && !c->band_sync && !c->band_sync_own;
    if (!c->deep_async && c->frame_pending && c->pending_may_redraw && only_ours) c->pending_superseded = true;
    else { const int rc = settle_before_write(c); if (rc) return rc; }
    const uint32_t a = blend == B32_BLEND_ERASE ? 0u : 255u;               // Color::to_bytes, types.rs:829-832
    const uint32_t rgba = r | (g << 8) | (b << 16) | (a << 24);
    // with a screen band set (multi-GPU sharding) only the rows this rank owns are cleared: the others belong to other ranks.
    // The clear is DEFERRED: the frame that follows folds it into its fused kernel (no clear launch, uncovered pixels written once);
    // anything else that touches the framebuffer first turns it into the launches it replaces (flush_clear).  An earlier deferred
    // clear of the same rows is dead (fully overwritten); of other rows, it is flushed.
    if (c->clear_pending && (c->clear_y0 != c->band_y0 || c->clear_y1 != c->band_y1)) { const int rc = flush_clear(c); if (rc) return rc; }
    c->clear_pending = true; c->clear_rgba = rgba; c->clear_y0 = c->band_y0; c->clear_y1 = c->band_y1;
    return B32_OK;
}
int b32_fb_clear_gradient(b32_ctx* c, uint8_t r0, uint8_t g0, uint8_t b0, uint8_t blend0, uint8_t r1, uint8_t g1, uint8_t b1, uint8_t blend1) {
    if (!c || !c->fb) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    { const int rc = settle_before_write(c); if (rc) return rc; }
    { const int rcf = flush_clear(c); if (rcf) return rcf; }
    const bool z = c->zbuf && c->zbuf_valid && (size_t)c->width * c->height <= c->cap_zbuf;
    launch_clear_gradient(c->stream, c->fb, z ? c->zbuf : nullptr, c->width, c->height, c->band_y0, c->band_y1,
                          r0 | (g0 << 8) | (b0 << 16) | ((uint32_t)blend0 << 24), r1 | (g1 << 8) | (b1 << 16) | ((uint32_t)blend1 << 24));
    HIPCHK(c, hipGetLastError());
    return B32_OK;
}
int b32_fb_clear_transparent(b32_ctx* c) { return b32_fb_clear(c, 0, 0, 0, B32_BLEND_ERASE); }    // [0,0,0,0] + zbuffer = f32::MAX

int b32_render_skybox_mesh(b32_ctx* c, const B32SkyVertex* v, uint32_t nv, const uint32_t* faces, uint32_t nf, const B32Camera* cam) {
    if (!c || !c->fb || !cam || (nv && !v) || (nf && !faces)) return B32_E_ARG;
    if (!nv || !nf) return B32_OK;
    (void)hipSetDevice(c->device);
    { const int rcs = settle_before_write(c); if (rcs) return rcs; }
    { const int rcf = flush_clear(c); if (rcf) return rcf; }
    for (size_t i = 0; i < (size_t)3 * nf; ++i) if (faces[i] >= nv) return B32_E_INDEX;    // projected[face[k]] index panic
    B32SkyVertex* dv = nullptr; uint32_t* df = nullptr; float2* dp = nullptr;
    Scratch tmp(c);
    int rc;
    if ((rc = tmp.upload(v, (size_t)nv, &dv))) return rc;
    if ((rc = tmp.upload(faces, (size_t)nf * 3, &df))) return rc;
    if ((rc = tmp.alloc(&dp, (size_t)nv))) return rc;
    launch_sky(c->stream, dv, nv, df, nf, *cam, dp, c->fb, c->width, c->height, c->band_y0, c->band_y1);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}
int b32_draw_star_diamonds(b32_ctx* c, const int32_t* cx, const int32_t* cy, const uint8_t* rgb, uint32_t n, float size) {
    if (!c || !c->fb || (n && (!cx || !cy || !rgb))) return B32_E_ARG;
    if (!n) return B32_OK;
    (void)hipSetDevice(c->device);
    { const int rcs = settle_before_write(c); if (rcs) return rcs; }
    { const int rcf = flush_clear(c); if (rcf) return rcf; }
    int32_t *dx = nullptr, *dy = nullptr; uint8_t* dc = nullptr;
    Scratch tmp(c);
    int rc;
    if ((rc = tmp.upload(cx, (size_t)n, &dx))) return rc;
    if ((rc = tmp.upload(cy, (size_t)n, &dy))) return rc;
    if ((rc = tmp.upload(rgb, (size_t)n * 3, &dc))) return rc;
    launch_stars(c->stream, dx, dy, dc, n, size, c->fb, c->width, c->height, c->band_y0, c->band_y1);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}
}  // extern "C"

// The ordered tile pass (b32_draw_pass.h) on the stream, in three steps that b32_draw_lines / b32_draw_prims (records from the host:
// draw_pass) and the record producers (records a kernel wrote on the device: produce_draw) put together.

// Before a pass: a pending frame settled (safe mode), a deferred clear flushed.
static int draw_enter(b32_ctx* c) {
    (void)hipSetDevice(c->device);
    { const int rcs = settle_before_write(c); if (rcs) return rcs; }
    return flush_clear(c);
}
// What every launch of a pass over the (non-empty) band needs.
template <class Rec>
static DrawArgs<Rec> draw_args(b32_ctx* c, uint32_t n) {
    DrawArgs<Rec> a{};
    a.n = n; a.fb = c->fb;
    a.zbuf = (c->zbuf && c->zbuf_valid && (size_t)c->width * c->height <= c->cap_zbuf) ? c->zbuf : nullptr;
    a.width = c->width; a.band_y0 = c->band_y0; a.band_y1 = c->band_y1;
    a.tiles_x = (c->width + 63u) / 64u; a.tiles_y = (c->band_y1 - c->band_y0 + LINE_TH - 1u) / LINE_TH;
    return a;
}
// Bin and draw records that are already on the device (a.recs, behind whatever wrote them on the stream): the tile route if `tiles` and
// `route` is not switched off, else every tile scans the whole batch.  *tiled (nullable): which of the two it was.
template <class Rec>
static int draw_resident(b32_ctx* c, DrawPassState<Rec>& ps, DrawArgs<Rec>& a, bool tiles, uint32_t route, bool* tiled = nullptr,
                         void (*launch)(hipStream_t, const DrawArgs<Rec>&, const Rec*) = nullptr) {
    const size_t ntiles = (size_t)a.tiles_x * a.tiles_y;
    const bool binned = tiles && !(c->route_off & route);
    if (tiled) *tiled = binned;
    if (binned) {
        if (ntiles > ps.cap_tiles || !ps.counters) {                       // (zero between batches: every tile kernel zeroes its own counter)
            const size_t cap = ntiles + ntiles / 4 + 16;
            if (ps.counters) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(ps.counters)); HIPCHK(c, hipFree(ps.lists)); }
            ps.counters = ps.lists = nullptr; ps.cap_tiles = 0;
            HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&ps.counters), (cap + 2) * FILL_PAD * sizeof(uint32_t)));
            HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&ps.lists), cap * LINE_TILE_CAP * sizeof(uint32_t)));
            HIPCHK(c, hipMemsetAsync(ps.counters, 0, (cap + 2) * FILL_PAD * sizeof(uint32_t), c->stream));
            ps.cap_tiles = cap;
        }
        if (!ps.long_list) HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&ps.long_list), LINE_LONG_CAP * sizeof(uint32_t)));
        a.counters = ps.counters; a.lists = ps.lists; a.long_list = ps.long_list; a.parity = ps.parity;
        ps.parity ^= 1u;
        ++ps.tile_batches;
    } else {
        ++ps.scan_batches;
    }
    if (launch) launch(c->stream, a, nullptr);                             // (the pass's kernels for other record kinds: GizmoPass)
    else launch_draw(c->stream, a, nullptr);
    HIPCHK(c, hipGetLastError());
    return B32_OK;
}

// A validated batch of host records through the pass, in array order.  A batch of at most `small_n` records travels in the kernel
// argument; a larger one is staged, and takes the tile route unless `route` is switched off.
template <class Rec>
static int draw_pass(b32_ctx* c, DrawPassState<Rec>& ps, const Rec* recs, uint32_t n, uint32_t small_n, uint32_t route) {
    if (!n) return B32_OK;
    { const int rc = draw_enter(c); if (rc) return rc; }
    if (c->band_y1 <= c->band_y0) return B32_OK;
    DrawArgs<Rec> a = draw_args<Rec>(c, n);
    if (n <= small_n) {
        launch_draw(c->stream, a, recs);
        HIPCHK(c, hipGetLastError());
        ++ps.scan_batches;
        return B32_OK;
    }
    { const int rc = stage_records(c, ps, recs, n); if (rc) return rc; }
    a.recs = ps.dev;
    return draw_resident(c, ps, a, true, route);
}

// ------------------------------------------------------------------ record producers
// Six features turn caller input into B32Prim records on the device -- in the primitive pass's record buffer, so the records never visit
// the host -- and hand them to the ordered tile pass: world items, the editor's gizmos, the modeler's mesh overlays, the world editor's
// room and object overlays, and the sky's star sprites.  Each also has a stage tap (b32_*_project_batch) that runs the same kernel into scratch memory and copies the records to
// the host.  A producer is a struct that holds the call's arguments and states only what is its own:
//   prepare(c, w, h)         everything that can fail on the arguments alone: the whole batch checked, the records laid out and counted
//                            (`total`), the args block `a` filled but for device pointers, the host rows to put on the device (`rows`,
//                            `n_rows`; none: nullptr, 0).  Enqueues nothing.
//   bind(c, out, in, tap)    the output, the rows on the device (nullptr: none, or they travel in the kernel argument) and the producer's
//                            private device state into `a`; tap != nullptr: per-call state from the tap's scratch, not from the context
//   launch(s, small)         the producer's kernels (small != nullptr: the rows by value, where the producer has such a kernel: SMALL > 0)
// and, for a draw: staged(c), its pinned ring; pass, the pass's launcher (nullptr: launch_draw); timer(c), events around the launch while
// profiling is on; routed(c, tiled), its own route counters.  produce_draw and produce_tap below are the only two sequences.
template <class ArgsT, class RowT, uint32_t SMALL_N>
struct Producer {
    using Args = ArgsT; using Row = RowT;
    static constexpr uint32_t SMALL = SMALL_N;
    Args a{}; const Row* rows = nullptr; uint32_t n_rows = 0; uint64_t total = 0;
    static constexpr void (*pass)(hipStream_t, const DrawArgs<B32Prim>&, const B32Prim*) = nullptr;
    static EventPair* timer(b32_ctx*) { return nullptr; }
    static void routed(b32_ctx*, bool) {}
};
// An entry's drawn / dropped / rejected on the device (zero on first use; the kernels add to them) as a kernel's `counts`.
static int counts_bind(b32_ctx* c, ArmedWords& w, unsigned long long*& counts) {
    const int rc = armed_ensure(c, w, 3 * sizeof(unsigned long long), 0);
    counts = static_cast<unsigned long long*>(w.p);
    return rc;
}
static int counts_read(b32_ctx* c, const ArmedWords& w, uint64_t* drawn, uint64_t* dropped, uint64_t* rejected) {
    if (!drawn || !dropped || !rejected) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    unsigned long long h[3] = { 0, 0, 0 };
    if (w.p) HIPCHK(c, hipMemcpyAsync(h, w.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *drawn = h[0]; *dropped = h[1]; *rejected = h[2];
    return B32_OK;
}

// World-space items (b32_world.hip; draw.rs:12-67, math.rs:503-652): record i from item i.
struct WorldProducer : Producer<WorldArgs, B32WorldItem, WORLD_SMALL> {
    const B32Camera* cam; const B32Ortho* ortho; const B32WorldItem* items; uint32_t n;
    int prepare(b32_ctx*, uint32_t w, uint32_t h) {
        for (uint32_t i = 0; i < n; ++i) {
            const B32WorldItem& it = items[i];
            const bool circle = it.kind == B32_PRIM_CIRCLE || it.kind == B32_PRIM_CIRCLE_ALPHA;
            if (it.kind > B32_PRIM_THICK_LINE || (it.flags & ~B32_WORLD_CLIP_NEAR) || (circle && it.flags) ||
                (it.kind == B32_PRIM_LINE_BLENDED && it.mode > B32_BLEND_ERASE)) return B32_E_ARG;
            if (circle && std::llabs((long long)it.size) > 32767) return B32_E_UNSUPPORTED;      // r * r (render.rs:632)
        }
        a.n = n;
        view_fill(a.v, *cam, w, h, ortho);
        rows = items; n_rows = n; total = n;
        return B32_OK;
    }
    int bind(b32_ctx* c, B32Prim* out, const B32WorldItem* in, Scratch*) {
        a.out = out; a.items = in;
        return counts_bind(c, c->world_counts, a.counts);
    }
    void launch(hipStream_t s, const B32WorldItem* small) const { launch_world_project(s, a, small); }
    static Staged<B32WorldItem>& staged(b32_ctx* c) { return c->world; }
    static EventPair* timer(b32_ctx* c) { return &c->world_timer; }         // (b32_last_kernel_times "world_project")
    static void routed(b32_ctx* c, bool tiled) { ++(tiled ? c->world_tile_batches : c->world_scan_batches); }
};

// The editor's overlay helpers (b32_gizmo.hip; viewport_3d.rs:5687-6357): the rows are the items with the index of their first record (a
// thick line becomes `thickness` records), drawn by the pass's GizmoPass kernels.
struct GizmoProducer : Producer<GizmoArgs, GizmoRow, GIZMO_SMALL> {
    const B32Camera* cam; const B32Ortho* ortho; const B32GizmoItem* items; uint32_t n;
    GizmoRow few[GIZMO_SMALL];                                                // (a small batch's rows: no allocation)
    int prepare(b32_ctx* c, uint32_t w, uint32_t h) {
        GizmoRow* r = few;
        if (n > GIZMO_SMALL) { c->gizmo_rows.resize(n); r = c->gizmo_rows.data(); }
        for (uint32_t i = 0; i < n; ++i) {
            const B32GizmoItem& it = items[i];
            if (it.kind > B32_GIZMO_TRIANGLE_VIEW || it._pad[0] || it._pad[1] || it._pad[2] ||
                (it.kind == B32_GIZMO_THICK_LINE_DEPTH && it.size > B32_GIZMO_MAX_THICKNESS)) return B32_E_ARG;
            if (it.kind == B32_GIZMO_POINT && std::llabs((long long)it.size) > 32767) return B32_E_UNSUPPORTED;    // r * r (render.rs:632)
            r[i].it = it; r[i].first = (uint32_t)total;
            total += (it.kind == B32_GIZMO_THICK_LINE_DEPTH && it.size > 1) ? (uint32_t)it.size : 1u;
        }
        if (total > 0x7FFFFFFFull) return B32_E_UNSUPPORTED;
        a.w.n = n;
        view_fill(a.w.v, *cam, w, h, ortho);
        rows = r; n_rows = n;
        return B32_OK;
    }
    int bind(b32_ctx* c, B32Prim* out, const GizmoRow* in, Scratch*) {
        a.w.out = out; a.rows = in;
        return counts_bind(c, c->gizmo_counts, a.w.counts);
    }
    void launch(hipStream_t s, const GizmoRow* small) const { launch_gizmo_project(s, a, small); }
    static Staged<GizmoRow>& staged(b32_ctx* c) { return c->gizmo; }
    static constexpr auto pass = launch_draw_gizmo;
};

// ------------------------------------------------------------------ the modeler's selection overlays (b32_overlay.hip)
// the bounds' keys: armed whenever no overlay is running (allocated so; k_overlay_emit leaves them so)
static int overlay_bounds(b32_ctx* c, OverlayArgs& a) {
    if (!c->overlay_bounds) {
        static const OverlayBounds armed = overlay_bounds_start();
        HIPCHK(c, hipMalloc(&c->overlay_bounds, sizeof(OverlayBounds)));
        HIPCHK(c, hipMemcpyAsync(c->overlay_bounds, &armed, sizeof(OverlayBounds), hipMemcpyHostToDevice, c->stream));
    }
    a.bounds = static_cast<OverlayBounds*>(c->overlay_bounds);
    return B32_OK;
}

// (modeler/viewport.rs:1782-2247) Made into records by k_overlay_points / k_overlay_emit from the slot's vertices as they are on the
// device.  The rows are the selected list to upload: the list as given, or c->overlay_pairs for polygons.
struct MeshOverlayProducer : Producer<OverlayArgs, uint32_t, 0> {
    const B32Camera* cam; const B32Ortho* ortho; const b32_scene* slot; const b32_topology* topo; const B32MeshOverlay* o; const uint32_t* selected;
    int prepare(b32_ctx* c, uint32_t w, uint32_t h);
    int bind(b32_ctx* c, B32Prim* out, const uint32_t* in, Scratch* tap) {    // the point table and the bounds
        int rc;
        a.out = out; a.selected = in;
        if (tap) { if ((rc = tap->alloc(&a.tab, (size_t)a.nv))) return rc; }
        else {
            if ((rc = ensure(c, c->overlay_tab, c->overlay_cap_tab, (size_t)a.nv))) return rc;
            a.tab = reinterpret_cast<OverlayPoint*>(c->overlay_tab);
        }
        return overlay_bounds(c, a);
    }
    void launch(hipStream_t s, const uint32_t*) const { launch_overlay(s, a); }
    static Staged<uint32_t>& staged(b32_ctx* c) { return c->overlay_sel; }
};
int MeshOverlayProducer::prepare(b32_ctx* c, uint32_t w, uint32_t h) {
    if (!cam || !slot || !o || !w || !h || !slot->have_scene) return B32_E_ARG;
    { const int rc = overlay_check(topo != nullptr, o, selected); if (rc) return rc; }
    const uint32_t np = topo ? topo->np : 0u, nh = topo ? topo->nh : 0u;
    const OverlayLayout l = overlay_layout(topo ? topo->h_poly_start.data() : nullptr, np, nh, topo ? topo->ne : 0u, slot->body_nv(), *o, selected);
    total = l.total;
    if (l.total > 0x7FFFFFFFull) return B32_E_UNSUPPORTED;
    view_fill(a.v, *cam, w, h, ortho);
    a.pos = slot_positions(slot, a.stride);
    a.nv = slot->body_nv();                            // (bone octahedra behind the mesh get no brackets and no dots)
    if (topo) { a.he = topo->he; a.poly_start = topo->poly_start; a.poly_verts = topo->poly_verts; a.np = np; a.nh = nh; }
    a.o = *o;
    a.at_brackets = (uint32_t)l.brackets; a.at_edges = (uint32_t)l.edges; a.at_dots = (uint32_t)l.dots;
    a.at_hover_vertex = (uint32_t)l.hover_vertex; a.at_hover_edge = (uint32_t)l.hover_edge; a.at_hover_face = (uint32_t)l.hover_face;
    a.at_selected = (uint32_t)l.selected; a.at_preview = (uint32_t)l.preview;
    a.hover_face_cnt = l.hover_face_cnt;
    const uint32_t sec = o->sections;
    const auto groups = [](uint32_t n) { return (uint32_t)(((unsigned long long)n + 255u) / 256u); };
    if (sec & B32_OVERLAY_EDGES) a.g_edges = groups(nh);
    if ((sec & B32_OVERLAY_PREVIEW) && o->preview_mode == 1u) a.g_pedges = groups(nh);
    if ((sec & B32_OVERLAY_PREVIEW) && o->preview_mode == 2u) a.g_pfaces = groups(np);
    if ((sec & B32_OVERLAY_SELECTED) && o->select_kind && o->n_selected) {
        if (o->select_kind == 3u) {                                                   // (polygon, first record) pairs of the polygons that exist
            c->overlay_pairs.clear();
            uint64_t at = l.selected;
            for (uint32_t i = 0; i < o->n_selected; ++i) {
                const uint32_t p = selected[i];
                if (p >= np) continue;
                c->overlay_pairs.push_back(p); c->overlay_pairs.push_back((uint32_t)at);
                at += overlay_polygon_slots(OVERLAY_POLY_SELECTED, topo->h_poly_start[p + 1u] - topo->h_poly_start[p]);
            }
            a.n_sel = (uint32_t)(c->overlay_pairs.size() / 2u);
            rows = c->overlay_pairs.data(); n_rows = (uint32_t)c->overlay_pairs.size();
        } else {
            if (o->select_kind == 2u && o->n_selected > 0x7FFFFFFFu) return B32_E_UNSUPPORTED;
            a.n_sel = o->n_selected;
            rows = selected; n_rows = o->select_kind == 2u ? 2u * o->n_selected : o->n_selected;
        }
        a.g_sel = groups(a.n_sel);
    }
    if ((sec & B32_OVERLAY_HOVER) && (o->hover_vertex != OVERLAY_NONE || o->hover_edge_v0 != OVERLAY_NONE || o->hover_edge_v1 != OVERLAY_NONE || l.hover_face_cnt))
        a.g_hover = 1u;
    if ((sec & B32_OVERLAY_BRACKETS) && a.nv) a.g_brackets = 1u;
    if ((unsigned long long)a.g_edges + a.g_pedges + a.g_sel + a.g_pfaces + 2u >= (1ull << 31)) return B32_E_UNSUPPORTED;
    return B32_OK;
}

// ------------------------------------------------------------------ the world editor's room overlays (b32_room_overlay.hip)
// (viewport_3d.rs:4273-4658, :4862-5362) Made into records by k_room_overlay from the room's records (and its last hover) as they are on
// the device.  The rows are the call's lists as one run of words in c->overlay_pairs: keys, edge pairs, faces, the points' bits.  Adds
// into the gizmo entry's counters (b32_gizmo_counts).
struct RoomOverlayProducer : Producer<RoomOverlayArgs, uint32_t, 0> {
    const B32Camera* cam; const b32_room* room; const B32RoomOverlay* o;
    const uint32_t *sel_vertices, *sel_edges, *sel_faces; const float* points_xyz;
    int prepare(b32_ctx* c, uint32_t w, uint32_t h);
    int bind(b32_ctx* c, B32Prim* out, const uint32_t* in, Scratch*) {
        a.out = out; a.lists = in;
        return counts_bind(c, c->gizmo_counts, a.counts);
    }
    void launch(hipStream_t s, const uint32_t*) const { launch_room_overlay(s, a); }
    static Staged<uint32_t>& staged(b32_ctx* c) { return c->overlay_sel; }
};
int RoomOverlayProducer::prepare(b32_ctx* c, uint32_t w, uint32_t h) {
    if (!cam || !room || !o || !w || !h) return B32_E_ARG;
    { const int rc = room_overlay_check(o, sel_vertices, sel_edges, sel_faces, points_xyz); if (rc) return rc; }
    if (o->hover_source == 1u && !room->have_hover) return B32_E_ARG;
    const RoomOverlayLayout l = room_overlay_layout(room->n, *o);
    total = l.total;
    if (l.total > 0x7FFFFFFFull) return B32_E_UNSUPPORTED;
    const uint64_t words = (uint64_t)o->n_vertices + 2ull * o->n_edges + o->n_faces + 3ull * o->n_points;
    if (words > 0x7FFFFFFFull) return B32_E_UNSUPPORTED;
    view_fill(a.v, *cam, w, h, nullptr);
    a.grid = room->grid; a.faces = room->faces; a.mats = room->have_mats ? room->mats : nullptr; a.n = room->n;
    a.hover = o->hover_source == 1u ? static_cast<const B32RoomHover*>(room->d_hover) : nullptr;
    a.o = *o;
    for (int k = 0; k < 4; ++k) a.rect[k] = l.rect[k];
    a.at_vertices = (uint32_t)l.vertices; a.at_edges = (uint32_t)l.edges; a.at_hover = (uint32_t)l.hover; a.at_sel_faces = (uint32_t)l.sel_faces;
    a.at_sel_edges = (uint32_t)l.sel_edges; a.at_preview = (uint32_t)l.preview; a.at_points = (uint32_t)l.points;
    a.l_edges = o->n_vertices; a.l_faces = a.l_edges + 2u * o->n_edges; a.l_points = a.l_faces + o->n_faces;
    std::vector<uint32_t>& lw = c->overlay_pairs;
    lw.resize((size_t)words);
    if (o->n_vertices) std::memcpy(lw.data(), sel_vertices, (size_t)o->n_vertices * 4u);
    if (o->n_edges) std::memcpy(lw.data() + a.l_edges, sel_edges, (size_t)o->n_edges * 8u);
    if (o->n_faces) std::memcpy(lw.data() + a.l_faces, sel_faces, (size_t)o->n_faces * 4u);
    if (o->n_points) std::memcpy(lw.data() + a.l_points, points_xyz, (size_t)o->n_points * 12u);
    const uint32_t sec = o->sections;
    const auto groups = [](uint64_t n) { return (uint32_t)((n + 255u) / 256u); };
    if (sec & B32_ROOM_OVERLAY_VERTICES) a.g_vertices = groups((uint64_t)o->n_vertices + 1u);
    if (sec & B32_ROOM_OVERLAY_EDGES) a.g_edges = groups(o->n_edges);
    if (sec & B32_ROOM_OVERLAY_HOVER) a.g_hover = 1u;
    if (sec & B32_ROOM_OVERLAY_SELECTED) { a.g_sel_faces = groups(o->n_faces); a.g_sel_edges = groups(o->n_edges); }
    if (l.gate) { a.g_preview = groups(room->n); a.g_points = groups(o->n_points); }
    rows = lw.data(); n_rows = (uint32_t)lw.size();
    return B32_OK;
}

// ------------------------------------------------------------------ the world editor's object overlays (b32_object_overlay.hip)
// (viewport_3d.rs:255-291, :7658-7697, asset.rs:288-312) Made into records by k_object_overlay from the parts' vertices and half-edges as
// they are on the device.  The rows are one run of words in c->overlay_pairs: the ObjectRows, the table of bounds blocks of the BOX_MESH
// rows, then k_scene_bounds' rows for the slots whose bounds are stale (c->bounds_stale) -- reduced in bind, in front of the kernel, into
// the slot's own block for the draw and for the tap alike.  Adds into the gizmo entry's counters (b32_gizmo_counts).
struct ObjectOverlayProducer : Producer<ObjectOverlayArgs, uint32_t, 0> {
    const B32Camera* cam; const B32ObjectPart* parts; uint32_t n_parts; const B32ObjectItem* items; uint32_t n_items;
    uint32_t w_bounds = 0, w_stale = 0;                                       // first word of the second and of the third table
    int prepare(b32_ctx* c, uint32_t w, uint32_t h);
    int bind(b32_ctx* c, B32Prim* out, const uint32_t* in, Scratch*) {
        a.out = out;
        a.rows = reinterpret_cast<const ObjectRow*>(in);
        a.bounds = reinterpret_cast<const OverlayBounds* const*>(in + w_bounds);
        { const int rc = scene_bounds_run(c, reinterpret_cast<const BoundsRow*>(in + w_stale)); if (rc) return rc; }
        return counts_bind(c, c->gizmo_counts, a.counts);
    }
    void launch(hipStream_t s, const uint32_t*) const { launch_object_overlay(s, a); }
    static Staged<uint32_t>& staged(b32_ctx* c) { return c->overlay_sel; }
};
int ObjectOverlayProducer::prepare(b32_ctx* c, uint32_t w, uint32_t h) {
    if (!cam || !w || !h) return B32_E_ARG;
    c->bounds_stale.clear();
    std::vector<ObjectPartView> views;
    object_part_views(parts, n_parts, views);
    ObjectOverlayPlan plan;
    int rc;
    if ((rc = object_overlay_plan(parts, views.data(), n_parts, items, n_items, false, plan))) return rc;      // the whole batch checked
    total = plan.total;
    if (!total) return B32_OK;
    (void)hipSetDevice(c->device);
    for (uint32_t i = 0; i < n_items; ++i) {                                // the blocks BOX_MESH reads exist (allocation only)
        if (items[i].kind != B32_OBJECT_BOX_MESH) continue;
        for (uint32_t p = items[i].first_part; p < items[i].first_part + items[i].n_parts; ++p) {
            if ((rc = scene_bounds_alloc(c, parts[p].slot))) return rc;
            views[p].bounds = parts[p].slot->d_bounds;
        }
    }
    if ((rc = object_overlay_plan(parts, views.data(), n_parts, items, n_items, true, plan))) return rc;
    for (uint32_t p : plan.bound_parts) {                                   // each stale slot once
        b32_scene* sc = parts[p].slot;
        if (!sc->bounds_valid && std::find(c->bounds_stale.begin(), c->bounds_stale.end(), sc) == c->bounds_stale.end()) c->bounds_stale.push_back(sc);
    }
    constexpr size_t ROW_W = sizeof(ObjectRow) / 4u, PTR_W = sizeof(void*) / 4u, STALE_W = sizeof(BoundsRow) / 4u;
    const size_t n_r = plan.rows.size(), n_b = plan.bounds.size(), n_s = c->bounds_stale.size();
    const size_t words = n_r * ROW_W + n_b * PTR_W + n_s * STALE_W;
    if (words > 0x7FFFFFFFull || plan.groups > 0x7FFFFFFFull) return B32_E_UNSUPPORTED;
    std::vector<uint32_t>& lw = c->overlay_pairs;
    lw.resize(words);
    std::memcpy(lw.data(), plan.rows.data(), n_r * sizeof(ObjectRow));
    w_bounds = (uint32_t)(n_r * ROW_W);
    if (n_b) std::memcpy(lw.data() + w_bounds, plan.bounds.data(), n_b * sizeof(void*));
    w_stale = w_bounds + (uint32_t)(n_b * PTR_W);
    for (size_t k = 0; k < n_s; ++k) {
        BoundsRow br{};
        scene_bounds_row(c->bounds_stale[k], &br);
        std::memcpy(lw.data() + w_stale + k * STALE_W, &br, sizeof(BoundsRow));
    }
    view_fill(a.v, *cam, w, h, nullptr);
    a.n_rows = (uint32_t)n_r; a.n_groups = (uint32_t)plan.groups;
    rows = lw.data(); n_rows = (uint32_t)words;
    return B32_OK;
}

// ------------------------------------------------------------------ the star sprites (b32_sky_resident.hip)
// (render.rs:206-237) Made into 1x1 filled rectangles by k_star_records: star i's 1, 5 or 9 records at i * per.  The rows are the stars.
struct StarProducer : Producer<StarArgs, B32Star, STAR_SMALL> {
    const B32Star* stars; uint32_t n; float size;
    int prepare(b32_ctx*, uint32_t, uint32_t) {
        if (n > STAR_MAX) return B32_E_UNSUPPORTED;
        a.n = n; a.per = star_per(size);
        rows = stars; n_rows = n; total = (uint64_t)n * a.per;
        return B32_OK;
    }
    int bind(b32_ctx*, B32Prim* out, const B32Star* in, Scratch*) { a.out = out; a.stars = in; return B32_OK; }
    void launch(hipStream_t s, const B32Star* small) const { launch_star_records(s, a, small); }
    static Staged<B32Star>& staged(b32_ctx* c) { return c->stars; }
};

// Where a producer's rows travel: by value in the kernel argument when it has such a kernel and the batch is small (no staging copy, no
// pinned-ring slot), else on the device.
template <class P> static bool rows_by_value(const P& p) { return P::SMALL && p.n_rows <= P::SMALL; }

// A producer's records drawn.  The batch is validated before anything is enqueued and before a pending frame is settled; a batch without
// records settles and flushes nothing; an empty band returns behind draw_enter without running the producer's kernel (no records, no
// counts).  The records go into c->prims.dev and are binned and drawn from there like any other primitive batch: the tile route when
// there are more than PRIM_SMALL of them.
template <class P>
static int produce_draw(b32_ctx* c, P& p) {
    int rc;
    if ((rc = p.prepare(c, c->width, c->height))) return rc;
    if (!p.total) return B32_OK;
    if ((rc = draw_enter(c))) return rc;                                    // (sets the device)
    if (c->band_y1 <= c->band_y0) return B32_OK;
    if ((rc = ensure(c, c->prims.dev, c->prims.cap_dev, (size_t)p.total))) return rc;
    const bool by_value = rows_by_value(p);
    const typename P::Row* d_rows = nullptr;
    if (!by_value && p.n_rows) {
        if ((rc = stage_records(c, P::staged(c), p.rows, p.n_rows))) return rc;
        d_rows = P::staged(c).dev;
    }
    if ((rc = p.bind(c, c->prims.dev, d_rows, nullptr))) return rc;
    EventPair* timer = c->profile_level >= 1 ? P::timer(c) : nullptr;
    if (timer) HIPCHK(c, timer->begin(c->stream));
    p.launch(c->stream, by_value ? p.rows : nullptr);
    HIPCHK(c, hipGetLastError());
    if (timer) HIPCHK(c, timer->end(c->stream));
    DrawArgs<B32Prim> d = draw_args<B32Prim>(c, (uint32_t)p.total);
    d.recs = c->prims.dev;
    bool tiled = false;
    if ((rc = draw_resident(c, c->prims, d, p.total > PRIM_SMALL, B32_ROUTE_PRIM_TILES, &tiled, P::pass))) return rc;
    P::routed(c, tiled);
    return B32_OK;
}
// A producer's records for a w x h framebuffer copied to the host (stage tap): the same kernel in the same launch form as the draw's,
// into scratch memory.  Needs no framebuffer, ignores the band, and always runs the kernel (the counters move).
template <class P>
static int produce_tap(b32_ctx* c, P& p, uint32_t w, uint32_t h, B32Prim* out, uint32_t cap, uint32_t* n_records) {
    int rc;
    if ((rc = p.prepare(c, w, h))) return rc;
    if (p.total > cap || (p.total && !out)) return B32_E_ARG;
    if (n_records) *n_records = (uint32_t)p.total;
    if (!p.total) return B32_OK;
    (void)hipSetDevice(c->device);
    const bool by_value = rows_by_value(p);
    B32Prim* d_out = nullptr; typename P::Row* d_rows = nullptr;
    Scratch tmp(c);
    if ((rc = tmp.alloc(&d_out, (size_t)p.total))) return rc;
    if (!by_value && p.n_rows && (rc = tmp.upload(p.rows, (size_t)p.n_rows, &d_rows))) return rc;
    if ((rc = p.bind(c, d_out, d_rows, &tmp))) return rc;
    p.launch(c->stream, by_value ? p.rows : nullptr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_out, (size_t)p.total * sizeof(B32Prim), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}

extern "C" {

// The line family of Framebuffer (render.rs:684-872), b32_lines.hip.
int b32_draw_lines(b32_ctx* c, const B32Line* lines, uint32_t n) {
    if (!c || !c->fb || (n && !lines)) return B32_E_ARG;
    for (uint32_t i = 0; i < n; ++i) {                                      // the whole batch, before anything is drawn
        const B32Line& l = lines[i];
        if (l.kind > B32_LINE_3D_ALPHA) return B32_E_ARG;
        if (prim_wide(l.x0, l.x1) || prim_wide(l.y0, l.y1)) return B32_E_UNSUPPORTED;   // 2 * err overflows i32 (render.rs:735, 800)
    }
    return draw_pass(c, c->lines, lines, n, LINE_SMALL, B32_ROUTE_LINE_TILES);
}
// The rest of Framebuffer's drawing methods (render.rs:631-971) and the line family, b32_prims.hip.
int b32_draw_prims(b32_ctx* c, const B32Prim* prims, uint32_t n) {
    if (!c || !c->fb || (n && !prims)) return B32_E_ARG;
    for (uint32_t i = 0; i < n; ++i) {                                      // the whole batch, before anything is drawn
        const B32Prim& p = prims[i];
        if (p.kind > B32_PRIM_FILLED_RECT || (p.kind == B32_PRIM_LINE_BLENDED && p.mode > B32_BLEND_ERASE)) return B32_E_ARG;
        if (p.kind == B32_PRIM_CIRCLE || p.kind == B32_PRIM_CIRCLE_ALPHA) {
            // r * r, dx * dx + dy * dy and cy +- radius stay inside i32 (render.rs:632-637)
            if (std::llabs((long long)p.size) > 32767 || prim_big(p.x0) || prim_big(p.y0)) return B32_E_UNSUPPORTED;
        } else if (p.kind != B32_PRIM_FILLED_RECT) {
            if (prim_wide(p.x0, p.x1) || prim_wide(p.y0, p.y1)) return B32_E_UNSUPPORTED;   // 2 * err overflows i32 (render.rs:735, 800)
        }
    }
    return draw_pass(c, c->prims, prims, n, PRIM_SMALL, B32_ROUTE_PRIM_TILES);
}
// The record producers (above): each a draw and its stage tap.
int b32_draw_world(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, const B32WorldItem* items, uint32_t n) {
    if (!c || !c->fb || !cam || (n && !items)) return B32_E_ARG;
    WorldProducer p{ {}, cam, ortho, items, n };
    return produce_draw(c, p);
}
int b32_draw_floor_grid(b32_ctx* c, const B32Camera* cam, float y, float spacing, float extent,
                        const uint8_t grid_rgbb[4], const uint8_t x_axis_rgbb[4], const uint8_t z_axis_rgbb[4]) {
    if (!c || !c->fb || !cam) return B32_E_ARG;
    uint32_t n = 0;
    int rc;
    if ((rc = b32_floor_grid_items(y, spacing, extent, grid_rgbb, x_axis_rgbb, z_axis_rgbb, nullptr, 0, &n))) return rc;
    std::vector<B32WorldItem> items(n);
    if ((rc = b32_floor_grid_items(y, spacing, extent, grid_rgbb, x_axis_rgbb, z_axis_rgbb, items.data(), n, &n))) return rc;
    return b32_draw_world(c, cam, nullptr, items.data(), n);
}
int b32_world_project_batch(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, const B32WorldItem* items, uint32_t n,
                            uint32_t w, uint32_t h, B32Prim* out) {
    if (!c || !cam || (n && (!items || !out)) || w == 0 || h == 0 || w > 16384 || h > 16384) return B32_E_ARG;
    WorldProducer p{ {}, cam, ortho, items, n };
    return produce_tap(c, p, w, h, out, n, nullptr);
}
int b32_world_counts(b32_ctx* c, uint64_t* drawn, uint64_t* dropped, uint64_t* rejected) {
    return c ? counts_read(c, c->world_counts, drawn, dropped, rejected) : B32_E_ARG;
}
int b32_draw_gizmos(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, const B32GizmoItem* items, uint32_t n) {
    if (!c || !c->fb || !cam || (n && !items)) return B32_E_ARG;
    GizmoProducer p{ {}, cam, ortho, items, n };
    return produce_draw(c, p);
}
int b32_gizmo_project_batch(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, const B32GizmoItem* items, uint32_t n,
                            uint32_t w, uint32_t h, B32Prim* out, uint32_t cap, uint32_t* n_records) {
    if (!c || !cam || !n_records || (n && !items) || w == 0 || h == 0 || w > 16384 || h > 16384) return B32_E_ARG;
    GizmoProducer p{ {}, cam, ortho, items, n };
    return produce_tap(c, p, w, h, out, cap, n_records);
}
int b32_gizmo_counts(b32_ctx* c, uint64_t* drawn, uint64_t* dropped, uint64_t* rejected) {
    return c ? counts_read(c, c->gizmo_counts, drawn, dropped, rejected) : B32_E_ARG;
}
int b32_draw_mesh_overlay(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, b32_scene* slot, b32_topology* topo, const B32MeshOverlay* o,
                          const uint32_t* selected) {
    if (!c || !c->fb) return B32_E_ARG;
    MeshOverlayProducer p{ {}, cam, ortho, slot, topo, o, selected };
    return produce_draw(c, p);
}
int b32_mesh_overlay_project_batch(b32_ctx* c, const B32Camera* cam, const B32Ortho* ortho, b32_scene* slot, b32_topology* topo,
                                   const B32MeshOverlay* o, const uint32_t* selected, uint32_t w, uint32_t h, B32Prim* out, uint32_t cap,
                                   uint32_t* n_records) {
    if (!c || !n_records || w > 16384 || h > 16384) return B32_E_ARG;
    MeshOverlayProducer p{ {}, cam, ortho, slot, topo, o, selected };
    return produce_tap(c, p, w, h, out, cap, n_records);
}
int b32_draw_room_overlay(b32_ctx* c, const B32Camera* cam, b32_room* room, const B32RoomOverlay* o, const uint32_t* sel_vertices,
                          const uint32_t* sel_edges, const uint32_t* sel_faces, const float* points_xyz) {
    if (!c || !c->fb) return B32_E_ARG;
    RoomOverlayProducer p{ {}, cam, room, o, sel_vertices, sel_edges, sel_faces, points_xyz };
    return produce_draw(c, p);
}
int b32_room_overlay_project_batch(b32_ctx* c, const B32Camera* cam, b32_room* room, const B32RoomOverlay* o, const uint32_t* sel_vertices,
                                   const uint32_t* sel_edges, const uint32_t* sel_faces, const float* points_xyz, uint32_t w, uint32_t h,
                                   B32Prim* out, uint32_t cap, uint32_t* n_records) {
    if (!c || !n_records || w > 16384 || h > 16384) return B32_E_ARG;
    RoomOverlayProducer p{ {}, cam, room, o, sel_vertices, sel_edges, sel_faces, points_xyz };
    return produce_tap(c, p, w, h, out, cap, n_records);
}
int b32_draw_object_overlays(b32_ctx* c, const B32Camera* cam, const B32ObjectPart* parts, uint32_t n_parts, const B32ObjectItem* items,
                             uint32_t n_items) {
    if (!c || !c->fb) return B32_E_ARG;
    ObjectOverlayProducer p{ {}, cam, parts, n_parts, items, n_items };
    return produce_draw(c, p);
}
int b32_object_overlay_project_batch(b32_ctx* c, const B32Camera* cam, const B32ObjectPart* parts, uint32_t n_parts, const B32ObjectItem* items,
                                     uint32_t n_items, uint32_t w, uint32_t h, B32Prim* out, uint32_t cap, uint32_t* n_records) {
    if (!c || !n_records || w > 16384 || h > 16384) return B32_E_ARG;
    ObjectOverlayProducer p{ {}, cam, parts, n_parts, items, n_items };
    return produce_tap(c, p, w, h, out, cap, n_records);
}
int b32_draw_stars(b32_ctx* c, const B32Star* stars, uint32_t n, float size) {
    if (!c || !c->fb || (n && !stars)) return B32_E_ARG;
    StarProducer p{ {}, stars, n, size };
    return produce_draw(c, p);
}
int b32_star_record_count(uint32_t n, float size, uint64_t* records) {
    if (!records) return B32_E_ARG;
    *records = (uint64_t)n * star_per(size);
    return B32_OK;
}
int b32_star_records_batch(b32_ctx* c, const B32Star* stars, uint32_t n, float size, B32Prim* out, uint32_t cap, uint32_t* n_records) {
    if (!c || !n_records || (n && !stars)) return B32_E_ARG;
    StarProducer p{ {}, stars, n, size };
    return produce_tap(c, p, 1, 1, out, cap, n_records);
}

// ------------------------------------------------------------------ the resident sky (k_sky_place_project, b32_sky_resident.hip)
int b32_sky_create(b32_ctx* c, const B32SkyVertex* offsets, uint32_t nv, const uint32_t* faces, uint32_t nf, b32_sky** out) {
    if (!c || !out || (nv && !offsets) || (nf && !faces)) return B32_E_ARG;
    for (size_t i = 0; i < (size_t)3 * nf; ++i) if (faces[i] >= nv) return B32_E_INDEX;    // projected[face[k]] index panic
    (void)hipSetDevice(c->device);
    b32_sky* s = new b32_sky();
    s->owner = c; s->nv = nv; s->nf = nf;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->verts), nv ? (size_t)nv * sizeof(B32SkyVertex) : 16);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->faces), nf ? (size_t)nf * 3 * sizeof(uint32_t) : 16);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->proj), nv ? (size_t)nv * sizeof(float2) : 16);
    if (e == hipSuccess && nv) e = hipMemcpyAsync(s->verts, offsets, (size_t)nv * sizeof(B32SkyVertex), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && nf) e = hipMemcpyAsync(s->faces, faces, (size_t)nf * 3 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);                   // (the caller's arrays are free again; once per level, not per frame)
    if (e != hipSuccess) {
        c->last_hip = (int)e;
        for (void* p : { (void*)s->verts, (void*)s->faces, (void*)s->proj }) if (p) (void)hipFree(p);
        delete s;
        return B32_E_HIP;
    }
    *out = s;
    return B32_OK;
}
void b32_sky_destroy(b32_ctx* c, b32_sky* sky) {
    if (!sky) return;
    if (c) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }     // (a render that reads it may be in flight)
    sky->ring.release();
    for (void* p : { (void*)sky->verts, (void*)sky->faces, (void*)sky->proj }) if (p) (void)hipFree(p);
    delete sky;
}
int b32_sky_update(b32_ctx* c, b32_sky* sky, uint32_t first, uint32_t count, const B32SkyVertex* verts) {
    if (!c || !sky || sky->owner != c || (count && !verts)) return B32_E_ARG;
    if ((unsigned long long)first + count > sky->nv) return B32_E_ARG;
    if (!count) return B32_OK;
    (void)hipSetDevice(c->device);
    return stage_records(c, sky->ring, verts, count, sky->verts + first);
}
int b32_render_sky(b32_ctx* c, b32_sky* sky, const B32Camera* cam) {
    if (!c || !c->fb || !sky || sky->owner != c || !cam) return B32_E_ARG;
    if (!sky->nv || !sky->nf) return B32_OK;
    { const int rc = draw_enter(c); if (rc) return rc; }
    if (c->band_y1 <= c->band_y0) return B32_OK;
    launch_sky_place_project(c->stream, sky->verts, sky->nv, *cam, c->width, c->height, sky->proj);
    launch_sky_fill(c->stream, sky->verts, sky->nv, sky->faces, sky->nf, sky->proj, c->fb, c->width, c->height, c->band_y0, c->band_y1);
    HIPCHK(c, hipGetLastError());
    return B32_OK;
}
int b32_sky_project_batch(b32_ctx* c, b32_sky* sky, const B32Camera* cam, uint32_t w, uint32_t h, float* xy) {
    if (!c || !sky || sky->owner != c || !cam || w == 0 || h == 0 || w > 16384 || h > 16384 || (sky->nv && !xy)) return B32_E_ARG;
    if (!sky->nv) return B32_OK;
    (void)hipSetDevice(c->device);
    float2* dp = nullptr;
    Scratch tmp(c);
    int rc;
    if ((rc = tmp.alloc(&dp, (size_t)sky->nv))) return rc;
    launch_sky_place_project(c->stream, sky->verts, sky->nv, *cam, w, h, dp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(xy, dp, (size_t)sky->nv * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}
int b32_present_nearest(b32_ctx* c, uint32_t dw, uint32_t dh, uint8_t* out) {
    if (!c || !c->fb || !out || !dw || !dh || dw > 32768 || dh > 32768) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    { const int rc = settle_pending(c); if (rc) return rc; }
    { const int rcf = flush_clear(c); if (rcf) return rcf; }
    uint32_t* dd = nullptr;
    Scratch tmp(c);
    int rc;
    if ((rc = tmp.alloc(&dd, (size_t)dw * dh))) return rc;
    launch_upscale_nearest(c->stream, c->fb, c->width, c->height, dd, dw, dh);
    HIPCHK(c, hipMemcpyAsync(out, dd, (size_t)dw * dh * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}
int b32_fb_upload(b32_ctx* c, const uint8_t* rgba) {
    if (!c || !c->fb || !rgba) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    { const int rc = settle_pending(c); if (rc) return rc; }
    { const int rcf = flush_clear(c); if (rcf) return rcf; }
    HIPCHK(c, hipMemcpyAsync(c->fb, rgba, (size_t)c->width * c->height * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}
int b32_zbuffer_download(b32_ctx* c, float* z) {
    if (!c || !c->fb || !z) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    { const int rc = settle_pending(c); if (rc) return rc; }
    { const int rcf = flush_clear(c); if (rcf) return rcf; }
    const size_t px = (size_t)c->width * c->height;
    if (!c->zbuf || !c->zbuf_valid) { HIPCHK(c, hipStreamSynchronize(c->stream)); for (size_t i = 0; i < px; ++i) z[i] = 3.40282347e+38f; return B32_OK; }
    HIPCHK(c, hipMemcpyAsync(z, c->zbuf, px * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}
int b32_zbuffer_upload(b32_ctx* c, const float* z) {
    if (!c || !c->fb || !z) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    { const int rc = settle_pending(c); if (rc) return rc; }
    { const int rcf = flush_clear(c); if (rcf) return rcf; }
    const size_t px = (size_t)c->width * c->height;
    int rc;
    if (px > c->cap_zbuf || !c->zbuf) { if ((rc = ensure_plain(c, c->zbuf, px + 64))) return rc; c->cap_zbuf = px; }
    HIPCHK(c, hipMemcpyAsync(c->zbuf, z, px * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->zbuf_valid = true;
    return B32_OK;
}
int b32_fb_download(b32_ctx* c, uint8_t* rgba) {
    if (!c || !c->fb || !rgba) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    { const int rc = settle_pending(c); if (rc) return rc; }
    { const int rcf = flush_clear(c); if (rcf) return rcf; }
    HIPCHK(c, hipMemcpyAsync(rgba, c->fb, (size_t)c->width * c->height * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}

// The presenter's copy without a host round trip per frame: the reference hands fb.pixels to the screen EVERY frame
// (game/renderer.rs:179-214); here the copy engine moves the frame into page-locked caller memory behind everything enqueued so far and
// a ticket tells when it has landed, so the host can enqueue frame i + 1 while frame i is drawn and copied.
void* b32_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void b32_host_free(void* p) { if (p) (void)hipHostFree(p); }
int ticket_open(b32_ctx* c, unsigned long long& t, hipEvent_t*& ev) {
    t = c->dl_seq + 1;
    ev = &c->dl_ev[t % b32_ctx::DL_RING];
    if (!*ev) HIPCHK(c, hipEventCreateWithFlags(ev, hipEventDisableTiming));
    else if (t > b32_ctx::DL_RING) HIPCHK(c, hipEventSynchronize(*ev));      // (the ticket that used this event, DL_RING tickets ago)
    if (!c->dl_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->dl_stream, hipStreamNonBlocking));
        for (hipEvent_t& e : c->dl_snap) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    return B32_OK;
}
int b32_fb_download_async(b32_ctx* c, uint8_t* rgba, uint64_t* ticket) {
    if (!c || !c->fb || !rgba || !ticket) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    // (safe mode: a pending frame that may still need a redraw is settled first, as b32_fb_download does -- the frames of small meshes, what
    // a console frame is made of, never are; deep mode never blocks the host: a dropped frame is reported by b32_frame_finish)
    if (!c->deep_async) { const int rc = settle_pending(c); if (rc) return rc; }
    { const int rcf = flush_clear(c); if (rcf) return rcf; }
    unsigned long long t = 0; hipEvent_t* tev = nullptr;
    { const int rct = ticket_open(c, t, tev); if (rct) return rct; }
    hipEvent_t& ev = *tev;
    const size_t px = (size_t)c->width * c->height;
    // a snapshot on the device first (two staging buffers, alternating): the frames that follow overwrite the framebuffer while the
    // snapshot crosses PCIe on a stream of its own
    if (px > c->dl_stage_px) {
        HIPCHK(c, hipStreamSynchronize(c->dl_stream));
        for (uint32_t*& q : c->dl_stage) { if (q) HIPCHK(c, hipFree(q)); q = nullptr; HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&q), px * 4)); }
        c->dl_stage_px = px;
    }
    const int k = (int)(t & 1u);
    // (the staging buffer's previous reader -- a download with a ticket of this parity, so t - 2 or earlier -- must have left: the main stream
    // waits for ticket t - 2, a download or a pick, behind which dl_stream has nothing older; normally long done)
    if (t > 2) HIPCHK(c, hipStreamWaitEvent(c->stream, c->dl_ev[(t - 2) % b32_ctx::DL_RING], 0));
    HIPCHK(c, hipMemcpyAsync(c->dl_stage[k], c->fb, px * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->dl_snap[k], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->dl_stream, c->dl_snap[k], 0));
    HIPCHK(c, hipMemcpyAsync(rgba, c->dl_stage[k], px * 4, hipMemcpyDeviceToHost, c->dl_stream));
    HIPCHK(c, hipEventRecord(ev, c->dl_stream));
    c->dl_seq = t; *ticket = t;
    return B32_OK;
}
int b32_ticket_poll(b32_ctx* c, uint64_t ticket, int* done) {
    if (!c || !done || ticket == 0 || ticket > c->dl_seq) return B32_E_ARG;
    *done = 1;
    if (ticket + b32_ctx::DL_RING <= c->dl_seq) return B32_OK;               // (its event has been reused: it completed long ago)
    const hipError_t e = hipEventQuery(c->dl_ev[ticket % b32_ctx::DL_RING]);
    if (e == hipErrorNotReady) { *done = 0; (void)hipGetLastError(); return B32_OK; }
    if (e != hipSuccess) { c->last_hip = (int)e; return B32_E_HIP; }
    return B32_OK;
}
int b32_ticket_wait(b32_ctx* c, uint64_t ticket) {
    if (!c || ticket == 0 || ticket > c->dl_seq) return B32_E_ARG;
    if (ticket + b32_ctx::DL_RING <= c->dl_seq) return B32_OK;
    HIPCHK(c, hipEventSynchronize(c->dl_ev[ticket % b32_ctx::DL_RING]));
    return B32_OK;
}

// ------------------------------------------------------------------ stage taps
int b32_project_fixed_batch(b32_ctx* c, const float* pos, uint32_t n, const B32Camera* cam, uint32_t w, uint32_t h,
                            int32_t* sx, int32_t* sy, float* z) {
    if (!c || !cam || (n && (!pos || !sx || !sy || !z))) return B32_E_ARG;
    if (!n) return B32_OK;
    (void)hipSetDevice(c->device);
    float* d_pos = nullptr; int32_t *d_sx = nullptr, *d_sy = nullptr; float* d_z = nullptr;
    Scratch tmp(c);
    int rc;
    if ((rc = tmp.upload(pos, (size_t)n * 3, &d_pos))) return rc;
    if ((rc = tmp.alloc(&d_sx, (size_t)n))) return rc;
    if ((rc = tmp.alloc(&d_sy, (size_t)n))) return rc;
    if ((rc = tmp.alloc(&d_z, (size_t)n))) return rc;
    launch_project_fixed(c->stream, d_pos, n, *cam, w, h, d_sx, d_sy, d_z);
    HIPCHK(c, hipMemcpyAsync(sx, d_sx, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sy, d_sy, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(z, d_z, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}

int b32_last_draw_order(b32_ctx* c, uint32_t* face_idx, uint32_t cap, uint32_t* n) {
    if (!c || !n || c->frame_pending) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    const uint32_t cnt = c->h_ctrl.n_visible;
    *n = cnt;
    if (c->last_local_sort && cnt) {     // the fast path never builds the global order: sort k_setup's keys now (tap only)
        const SortScratch sc{ c->block_hist, c->hist_blocks, c->digit_total };
        hipStream_t s = c->stream;
        launch_radix_pass(s, c->cur.keys0, nullptr, c->keys1, c->vals[1], c->scene.d_consts, c->scene.nf, 0, 8, sc);
        launch_radix_pass(s, c->keys1, c->vals[1], c->cur.keys0, c->vals[0], &c->cur.d_ctrl->n_visible, c->scene.nf, 8, 8, sc);
        launch_radix_pass(s, c->cur.keys0, c->vals[0], c->keys1, c->vals[1], &c->cur.d_ctrl->n_visible, c->scene.nf, 16, 8, sc);
        launch_radix_pass(s, c->keys1, c->vals[1], c->cur.keys0, c->vals[0], &c->cur.d_ctrl->n_visible, c->scene.nf, 24, 8, sc);
        c->last_local_sort = false;
    }
    const uint32_t m = cnt < cap ? cnt : cap;
    if (m && face_idx) {
        // the device works on record slots (k_setup packs each wave's survivors to the front of its 64 slots): back to face ids
        std::vector<uint32_t> fo(c->scene.nf);
        HIPCHK(c, hipMemcpyAsync(face_idx, c->vals[0], (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(fo.data(), c->cur.face_of, (size_t)c->scene.nf * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint32_t i = 0; i < m; ++i) face_idx[i] = face_idx[i] < c->scene.nf ? fo[face_idx[i]] : 0xFFFFFFFFu;
    }
    return B32_OK;
}

int b32_last_surface_shading(b32_ctx* c, uint32_t* face_idx, float* shades, uint32_t* colors, uint32_t cap, uint32_t* n, uint32_t* n_shaded) {
    if (!c || !n || !n_shaded || c->frame_pending || c->frame_batched || c->band_set || !c->scene.have_scene) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    const uint32_t nf = c->scene.nf, cnt = c->h_ctrl.n_visible;
    const bool lit = c->last_settings.shading != B32_SHADE_NONE;
    *n = 0; *n_shaded = 0;
    if (!nf || !cnt) return B32_OK;
    // the frame set must be the one that mesh's frame wrote (a slot swapped out since then is another mesh: refused, not read past its end)
    if (cnt > nf || nf > c->cur.cap_work || !c->cur.face_of || !c->cur.srecs || !c->cur.keys0 || !c->vals[0]) return B32_E_ARG;
    if (lit && (!c->cur.shades || nf > c->cur.cap_shades)) return B32_E_ARG;
    // which record slots hold a surface: the fast path leaves k_setup's keys as they were written (KEY_INVALID behind each wave's
    // survivors); a frame with a global sort has sorted over them and left the slots, in draw order, where b32_last_draw_order reads them
    std::vector<uint32_t> live(c->last_local_sort ? nf : cnt), fo(nf);
    std::vector<ShadeRec> sr(nf);
    std::vector<float> sh(lit ? (size_t)nf * 9 : 0);
    HIPCHK(c, hipMemcpyAsync(live.data(), c->last_local_sort ? c->cur.keys0 : c->vals[0], live.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(fo.data(), c->cur.face_of, (size_t)nf * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sr.data(), c->cur.srecs, (size_t)nf * sizeof(ShadeRec), hipMemcpyDeviceToHost, c->stream));
    if (lit) HIPCHK(c, hipMemcpyAsync(sh.data(), c->cur.shades, sh.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> slots;
    slots.reserve(cnt);
    if (c->last_local_sort) { for (uint32_t s = 0; s < nf; ++s) if (live[s] != KEY_INVALID) slots.push_back(s); }
    else { slots = live; std::sort(slots.begin(), slots.end()); }
    if (slots.size() != cnt || slots.back() >= nf) return B32_E_ARG;
    *n = cnt; *n_shaded = lit ? cnt : 0;
    for (uint32_t i = 0; i < cnt && i < cap; ++i) {          // (slots ascend with the face id: k_setup packs each wave's survivors in order)
        const uint32_t s = slots[i];
        if (face_idx) face_idx[i] = fo[s];
        if (colors) { colors[i * 3] = sr[s].pk0 & 0xFFFFFFu; colors[i * 3 + 1] = sr[s].pk1 & 0xFFFFFFu; colors[i * 3 + 2] = sr[s].pk2 & 0xFFFFFFu; }
        if (shades && lit) std::memcpy(shades + (size_t)i * 9, sh.data() + (size_t)s * 9, 9 * sizeof(float));
    }
    return B32_OK;
}

int b32_selftest_f32(b32_ctx* c, int op, const float* a, const float* b, const float* cc, float* out, uint32_t n) {
    if (!c || !a || !b || !cc || !out) return B32_E_ARG;
    if (!n) return B32_OK;
    (void)hipSetDevice(c->device);
    float* d[4] = { nullptr, nullptr, nullptr, nullptr };
    Scratch tmp(c);
    int rc;
    if ((rc = tmp.upload(a, (size_t)n, &d[0]))) return rc;
    if ((rc = tmp.upload(b, (size_t)n, &d[1]))) return rc;
    if ((rc = tmp.upload(cc, (size_t)n, &d[2]))) return rc;
    if ((rc = tmp.alloc(&d[3], (size_t)n))) return rc;
    launch_selftest(c->stream, op, d[0], d[1], d[2], d[3], n);
    HIPCHK(c, hipMemcpyAsync(out, d[3], (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return B32_OK;
}

int b32_device_constants(b32_ctx* c, const char** names, uint32_t* bits, uint8_t* is_f32, uint32_t cap, uint32_t* count,
                         uint8_t* unr_table257, int32_t* dither16) {
    if (!c) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    struct Entry { const char* name; uint8_t f; };
#define B32_K_F 1
#define B32_K_I 0
#define B32_K_ENTRY(name, kind, v) { name, B32_K_##kind },
    static const Entry kEntries[] = { B32_CONSTANTS(B32_K_ENTRY) };
#undef B32_K_ENTRY
#undef B32_K_F
#undef B32_K_I
    constexpr uint32_t N = sizeof(kEntries) / sizeof(kEntries[0]);
    if (count) *count = N;
    uint32_t* d_bits = nullptr; uint8_t* d_unr = nullptr; int32_t* d_dither = nullptr;
    Scratch tmp(c);
    int rc;
    if ((rc = tmp.alloc(&d_bits, (size_t)N))) return rc;
    if ((rc = tmp.alloc(&d_unr, (size_t)K::UNR_ENTRIES))) return rc;
    if ((rc = tmp.alloc(&d_dither, (size_t)16))) return rc;
    launch_constants(c->stream, d_bits, d_unr, d_dither);
    std::vector<uint32_t> h(N);
    HIPCHK(c, hipMemcpyAsync(h.data(), d_bits, N * 4, hipMemcpyDeviceToHost, c->stream));
    if (unr_table257) HIPCHK(c, hipMemcpyAsync(unr_table257, d_unr, K::UNR_ENTRIES, hipMemcpyDeviceToHost, c->stream));
    if (dither16) HIPCHK(c, hipMemcpyAsync(dither16, d_dither, 16 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < N && i < cap; ++i) {
        if (names) names[i] = kEntries[i].name;
        if (bits) bits[i] = h[i];
        if (is_f32) is_f32[i] = kEntries[i].f;
    }
    return B32_OK;
}

int b32_last_kernel_times(b32_ctx* c, const char** names, float* ms, uint32_t cap) {
    if (!c || !names || !ms) return 0;
    static const char* const kNames[5] = { "setup", "sort", "bin", "cover", "shade" };
    uint32_t k = 0;
    for (int p = 0; c->phase_frames && p < 5 && k < cap; ++p) {
        if (p != 3 && c->phase_level < 2) continue;
        names[k] = kNames[p]; ms[k] = c->phase_ms[p]; ++k;
    }
    // the kernels of the last b32_draw_world (its projection), b32_pick_meshes[_async] (pick and resolve) and b32_hover_mesh[_async]
    // enqueued while profiling was on (waits for them)
    const struct { const char* name; const EventPair* pair; } timers[3] = { { "world_project", &c->world_timer }, { "pick", &c->pick_timer }, { "hover", &c->hover_timer } };
    for (const auto& t : timers) {
        float t_ms = 0.0f;
        if (k < cap && t.pair->elapsed(&t_ms)) { names[k] = t.name; ms[k] = t_ms; ++k; }
    }
    return (int)k;
}

}  // extern "C"

// 0 = no events, 1 = events around k_fill, 2 = events around every phase.
extern "C" int b32_set_fragment_counting(b32_ctx* c, int on) {
    if (!c) return B32_E_ARG;
    c->count_fragments = on ? 1 : 0;
    return B32_OK;
}
extern "C" unsigned long long b32_route_count(const b32_ctx* c, int which) {
    if (c && which == 7) return c->pipelined_frames;
    if (c && which == 8) return c->lds_atlas_frames;
    if (c && which == 9) return c->wire_tile_frames;
    if (c && which == 10) return c->span_cover_frames;
    if (c && which == 11) return c->flag_join_frames;
    if (c && which == 12) return c->event_join_frames;
    if (c && which == 13) return c->poll_join_frames;
    if (c && which == 14) return c->lines.tile_batches;
    if (c && which == 15) return c->lines.scan_batches;
    if (c && which == 16) return c->prims.tile_batches;
    if (c && which == 17) return c->prims.scan_batches;
    if (c && which == 18) return c->world_tile_batches;
    if (c && which == 19) return c->world_scan_batches;
    if (c && which == 20) return c->bounds_reductions;
    return (c && which >= 0 && which < 8) ? c->routes[which] : 0ull;
}
extern "C" int b32_set_async_depth(b32_ctx* c, int deep) {
    if (!c) return B32_E_ARG;
    if (!deep) { const int rc = settle_pending(c); if (rc) return rc; }
    c->deep_async = deep != 0;
    return B32_OK;
}
extern "C" int b32_set_profiling(b32_ctx* c, int level) {
    if (!c) return B32_E_ARG;
    c->profile_level = level < 0 ? 0 : (level > 2 ? 2 : level);
    if (!c->profile_level) c->hover_timer.timed = c->world_timer.timed = false;     // (b32_last_kernel_times no longer reports "hover", "world_project")
    c->prof_seq = 0;
    if (c->profile_level >= 1 && !c->ev_created) {      // (here, not in the first profiled frame: 384 hipEventCreate calls are ~0.2 ms of host time)
        (void)hipSetDevice(c->device);
        for (auto& fr : c->ev) for (auto& e : fr) HIPCHK(c, hipEventCreate(&e));
        c->ev_created = true;
    }
    return B32_OK;
}
extern "C" int b32_set_routes(b32_ctx* c, uint32_t off_mask) {
    if (!c) return B32_E_ARG;
    const int rc = settle_pending(c);
    if (rc) return rc;
    c->route_off = off_mask;
    return B32_OK;
}
extern "C" int b32_set_cheap_threshold(b32_ctx* c, uint32_t den) {
    if (!c || den == 0) return B32_E_ARG;
    c->cheap_den = den;          // (applies to the textures uploaded from now on:
    c->scene.tex_sig_valid = false;    //  the next upload re-counts the skippable texels even if the pool already holds the same textures)
    return B32_OK;
}
extern "C" int b32_set_pipeline_gate(b32_ctx* c, uint32_t permille) {
    if (!c || permille > 2000u) return B32_E_ARG;
    c->gate_permille = permille;
    return B32_OK;
}
extern "C" int b32_last_shader_clock(const b32_ctx* c, float* ghz, float* fill_ms) {
    if (!c || !ghz) return B32_E_ARG;
    *ghz = 0.0f; if (fill_ms) *fill_ms = 0.0f;
    const unsigned long long* t = c->h_stamps.t;                      // of the last frame b32_frame_finish read back
    if (!t[ST_FILL] || !t[ST_CLKW] || t[ST_CLKW] <= t[ST_FILL] || t[ST_CLK1] <= t[ST_CLK0]) return B32_OK;      // (no fused kernel in that frame)
    const double ns = (double)(t[ST_CLKW] - t[ST_FILL]) * 10.0;       // wall_clock64: 100 MHz
    *ghz = (float)((double)(t[ST_CLK1] - t[ST_CLK0]) / ns);
    if (fill_ms) *fill_ms = (float)(ns * 1e-6);
    return B32_OK;
}
extern "C" int b32_transparent_counts(const b32_ctx* c, uint32_t* host_bound, uint32_t* device_last) {
    if (!c || !host_bound || !device_last) return B32_E_ARG;
    *host_bound = c->scene.blend_faces; *device_last = c->h_ctrl.n_transparent;
    return B32_OK;
}
// The depth the library picks itself (b32_set_pipeline_depth(ctx, 0), the default): two frame sets, three for a NARROW band -- at most a sixth
// of the frame's rows, one rank of a frame sharded over six or more GPUs.  Such a rank still transforms the whole mesh and its frame is
// bound by the setup kernel, not by the fill: with three sets the setup kernels run back to back on the side stream instead of each waiting
// for the previous frame's fill to start (240 rows of C3, 1 of 8 ranks: 0.040 -> 0.034-0.035 ms per frame; 480 rows: the same either way; 960
// rows and the whole frame: two sets are faster -- profiles/r06_band_depth.txt).
static uint32_t auto_depth(const b32_ctx* c) {
    return (c->band_set && c->height && (uint64_t)(c->band_y1 - c->band_y0) * 6u <= c->height) ? 3u : 2u;
}
static int apply_depth(b32_ctx* c, uint32_t sets) {
    if (sets == c->n_sets) return B32_OK;
    (void)hipSetDevice(c->device);
    // everything in flight ends first: the ring's order (alt[0] oldest) only means something for one depth
    const int rc = b32_frame_finish(c, nullptr);
    if (rc == B32_E_HIP || rc == B32_E_ARG) return rc;
    if (rc && !c->deferred_rc) c->deferred_rc = rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->side) HIPCHK(c, hipStreamSynchronize(c->side));
    c->n_sets = sets;
    return B32_OK;
}
extern "C" int b32_set_pipeline_depth(b32_ctx* c, uint32_t sets) {
    if (!c || sets == 1u || sets > 3u) return B32_E_ARG;
    c->n_sets_user = sets;
    return apply_depth(c, sets ? sets : auto_depth(c));
}
extern "C" int apply_depth_auto(b32_ctx* c) { return apply_depth(c, auto_depth(c)); }
extern "C" int b32_debug_inject(b32_ctx* c, uint32_t what) {
    if (!c || (what & ~3u)) return B32_E_ARG;
    c->inject |= what;
    return B32_OK;
}
extern "C" int b32_set_profiling_stride(b32_ctx* c, uint32_t every) {
    if (!c) return B32_E_ARG;
    c->prof_stride = every ? every : 1u;
    c->prof_seq = 0;
    return B32_OK;
}
