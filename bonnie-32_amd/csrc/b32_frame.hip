// b32_frame.hip -- the C ABI, part 3: one frame.  Route selection, enqueue (k_setup -> fill [-> k_blend] [-> wireframe kernels]) without a
// host round trip, two or three frames in flight, and b32_frame_finish -- the only host readback (error flags, triangles_drawn, fragment
// count, overflow -> grow and redraw).
#include "b32_host.h"

// ------------------------------------------------------------------ two frames in flight
// The fused fill kernel leaves most CUs idle in its last fifth (the tile queue's tail), and k_setup of the NEXT frame needs nothing
// from it: with two frame sets (everything k_setup writes, FrameSet) the setup kernel of frame i + 1 runs on a second stream beside the
// fill of frame i.  Orders kept by events: setup(i) -> fill(i) (ev_setup; or the k_flag / k_join kernels), fill(i) -> setup(i + 2) on the same set
// (round 6: on the device, k_gate waits for fill(i + 1) to have STARTED; an event only where that frame launched no fused kernel), and
// anything enqueued on the main stream that k_setup reads (uploads, packed streams, light lists, list-space memsets) -> the next
// setup (ev_main, only when `side_dirty`).  The main stream always waits for the frame's setup before enqueue_frame returns, so a
// synchronisation of the main stream still covers everything this context has in flight.
static void swap_with(b32_ctx* c, FrameSet& a) { std::swap(c->cur, a); }
// The frame being enqueued takes the OLDEST set; afterwards alt[n_sets - 2] is the previous frame's set and alt[0] the set of the frame
// n_sets - 1 back -- the one whose fill the new frame's setup kernel is meant to run beside (its tile cursor is what the gate polls).
static void rotate_sets(b32_ctx* c) {
    swap_with(c, c->alt[0]);                                   // current <- oldest; alt[0] <- previous frame's
    if (c->n_sets == 3) std::swap(c->alt[0], c->alt[1]);        // alt[0] <- two frames back, alt[1] <- previous frame's
}
static void unrotate_sets(b32_ctx* c) {      // (an enqueue that failed between rotate_sets and its launches)
    if (c->n_sets == 3) std::swap(c->alt[0], c->alt[1]);
    swap_with(c, c->alt[0]);
}
// side stream, events and the other sets' per-face buffers (sized like the current set's)
static int pipeline_ensure(b32_ctx* c) {
    if (!c->side) {
        // lowest priority: while the fill kernel has workgroups to place, they go first; the setup kernel takes what is left
        int prio_least = 0, prio_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        HIPCHK(c, hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, prio_least));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_wbin, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->cur.ev_setup, hipEventDisableTiming));
        for (FrameSet& a : c->alt) HIPCHK(c, hipEventCreateWithFlags(&a.ev_setup, hipEventDisableTiming));
        // the fills of the frames enqueued before the side stream existed end before this point of the main stream, which the first setup
        // kernel on the side stream waits for (side_dirty)
        c->side_dirty = true;
    }
    for (uint32_t k = 0; k + 1 < c->n_sets; ++k) {
        FrameSet& a = c->alt[k];
        if (!a.d_ctrl) {
            HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&a.d_ctrl), sizeof(Ctrl) + sizeof(Stamps) + sizeof(Events)));
            HIPCHK(c, hipMemsetAsync(a.d_ctrl, 0, sizeof(Ctrl) + sizeof(Stamps) + sizeof(Events), c->stream));
            c->side_dirty = true;
        }
        if (a.cap_work < c->cap_work || !a.crecs) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            a.release();
            const size_t n = c->cap_work;
            int rc;
            if ((rc = ensure_plain(c, a.keys0, n))) return rc;
            if ((rc = ensure_plain(c, a.crecs, n))) return rc;
            if ((rc = ensure_plain(c, a.srecs, n))) return rc;
            if ((rc = ensure_plain(c, a.xrecs, n))) return rc;
            if ((rc = ensure_plain(c, a.spans, n))) return rc;
            if ((rc = ensure_plain(c, a.face_of, n))) return rc;
            if ((rc = ensure_plain(c, a.partials, (size_t)((n + 255) / 256) * 8 + 8))) return rc;
            a.cap_work = n;
        }
    }
    return B32_OK;
}

extern "C" {
// ------------------------------------------------------------------ frame
int validate_settings(const B32Settings* st) {
    if (st->shading > B32_SHADE_GOURAUD) return B32_E_ARG;
    if (st->n_lights && !st->lights) return B32_E_ARG;
    if (st->shading != B32_SHADE_NONE)
        for (uint32_t i = 0; i < st->n_lights; ++i)
            if (st->lights[i].enabled && st->lights[i].type > B32_LIGHT_SPOT) return B32_E_ARG;                 // not a LightType
    return B32_OK;
}

static uint32_t bits_for(uint32_t n_keys) { uint32_t b = 1; while ((1ull << b) < n_keys) ++b; return b; }

// ------------------------------------------------------------------ one frame = the pieces below, in order (enqueue_frame)
// The frame's plan: which pipeline it takes (every route produces the same framebuffer: tests run every scene through several of them)
// and what the steps of enqueue_frame pass to each other.  The decisions themselves are b32_frame_plan.h's.
struct FramePlan {
    bool wire_back = false, wire_front = false;      // the wireframe phases of this frame (render.rs:2577, 2603)
    // ---- the route (plan_route)
    bool with_class = false;     // the scene can have a transparent pass: tile lists are split by class
    bool ordered_all = false;    // ordered walk of whole tile lists instead of the overwrite pass (x-ray; 8-bit path with blending texels)
    bool want_prio64 = false;    // sort-free fused path (painter's or z-buffer mode)
    bool exact_cov = false;      // EXACT coverage: texel rule per fragment (exact store counting, textures with many skippable texels)
    bool local_sort = false;     // keyed fast path: per-tile LDS sort instead of the global painter's sort
    bool want_inline = false;    // small mesh: the fused kernel's workgroups collect their own tile lists
    bool direct_bin = false;     // large mesh: k_setup appends to fixed tile regions (DirectBin)
    bool inline_bin = false, prio64 = false;     // the tile lists the fill reads (inline / direct binning: known from the route; span binning: once it ran)
    uint32_t list_stride = 0;    // entries per tile region (inline / direct binning)
    DirectBin db{};
    uint32_t ntiles = 0;         // of the grid plan_route left in FrameParams
    bool fused = false, wide = false;                // plan_fused / plan_wide: asked once, here (set_prio64, plan_pipeline); FillArgs carries them to launch_fill
    void set_prio64(bool on) { prio64 = on; fused = plan_fused(prio64, wire_front, ordered_all); }
    // ---- two frames in flight (plan_pipeline, order_side_stream, hand_over)
    HandOver hand_over_kind = HandOver::None;
    hipStream_t setup_stream = nullptr;              // the side stream of a pipelined frame, else the context's
    uint32_t poll_seq = 0, poll_patience = 0;        // FillArgs::join_seq / join_patience of a polled hand-over
    uint32_t start_seq = 0;                          // the start word this frame's fused kernel was meant to publish
    // ---- wireframe phases (wire_args, hand_over, wire_phases)
    bool wire_on = false, wire_binned = false, wire_polled = false;
    WireArgs wa{};
    // ---- the rest
    const float *pos12 = nullptr, *attr12 = nullptr; // packed vertex streams (frame_positions)
    bool prof_all = false, prof_fill = false;        // profiling level 2 / >= 1 on this frame
    hipEvent_t* ev = nullptr;                        // its row of events
    int pair_buf = 0;                                // the pair buffer that holds the keyed routes' grouped lists (bin_keyed)
};

// The frame sets between rotate_sets and the frame's first launch into the set it rotated to: every return in between -- the ones inside
// HIPCHK too -- puts the sets back (the pending frame stays the current set's) and the frame is not pipelined.  Dismissed immediately
// before launch_setup: from there on the frame is in flight in that set and no return may unrotate.
struct SetsGuard {
    b32_ctx* c; bool armed = false;
    explicit SetsGuard(b32_ctx* ctx) : c(ctx) {}
    SetsGuard(const SetsGuard&) = delete;
    SetsGuard& operator=(const SetsGuard&) = delete;
    void rotate() { rotate_sets(c); armed = true; }
    void dismiss() { armed = false; }
    ~SetsGuard() { if (armed) { unrotate_sets(c); c->pipelined = false; } }
};

static FrameParams frame_params(const b32_ctx* c, const B32Camera* cam, const B32Settings* st, const B32Fog* fog, bool wire_any) {
    FrameParams fp{};
    fp.cam = *cam;
    fp.width = c->width; fp.height = c->height;
    fp.band_y0 = c->band_y0; fp.band_y1 = c->band_y1;
    fp.tiles_x = (c->width + TILE_W - 1) / TILE_W;
    fp.tile_h = TILE_H;
    fp.tile_yb = (c->band_y0 / TILE_H) * TILE_H;
    fp.tiles_y = c->band_y1 > c->band_y0 ? (c->band_y1 - fp.tile_yb + TILE_H - 1) / TILE_H : 0;
    fp.nv = c->scene.nv; fp.nf = c->scene.nf; fp.nt = c->scene.nt;
    fp.n_lights = st->shading != B32_SHADE_NONE ? st->n_lights : 0;
    fp.ambient = st->ambient;
    fp.affine = st->affine_textures; fp.shading = st->shading; fp.backface_cull = st->backface_cull;
    fp.dithering = st->dithering; fp.fixed_point = st->use_fixed_point; fp.has_fog = fog ? 1 : 0; fp.zmode = st->use_zbuffer ? 1 : 0;
    if (fog) fp.fog = *fog;
    fp.camfx = make_camfx_any(*cam, c->width, c->height);
    fp.fmt8 = c->scene.fmt8 ? 1 : 0;
    fp.ortho = st->has_ortho ? 1 : 0; fp.xray = st->xray_mode ? 1 : 0;
    fp.ortho_zoom = st->ortho_zoom; fp.ortho_cx = st->ortho_center_x; fp.ortho_cy = st->ortho_center_y;
    fp.wire_collect = wire_any ? 1 : 0;
    fp.band_only = 0;
    fp.redraw = c->redrawing ? 1 : 0;
    fp.tex_blend_any = c->scene.tex_blend_any ? 1 : 0;
    fp.batched = c->frame_batched ? 1 : 0;
    fp.placed = c->frame_placed ? 1 : 0;
    return fp;
}

// lights: up to LIGHTS_INLINE travel by value in k_setup's arguments (a light change costs no copy and no synchronisation: the
// per-room light lists of a multi-mesh frame stay asynchronous); longer lists go through a device buffer, refreshed -- with a
// synchronisation -- only when they differ from the copy it holds
static int frame_lights(b32_ctx* c, const B32Settings* st, FrameParams& fp, LightSet& lset) {
    int rc;
    if (fp.n_lights && fp.n_lights <= LIGHTS_INLINE) {
        memcpy(lset.l, st->lights, fp.n_lights * sizeof(B32Light));
        fp.lights_inline = 1;
    } else if (fp.n_lights) {
        bool same = c->h_lights.size() == fp.n_lights && memcmp(c->h_lights.data(), st->lights, fp.n_lights * sizeof(B32Light)) == 0;
        if (!same) {
            if ((rc = ensure(c, c->d_lights, c->cap_lights, (size_t)fp.n_lights))) return rc;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipMemcpy(c->d_lights, st->lights, fp.n_lights * sizeof(B32Light), hipMemcpyHostToDevice));
            c->side_dirty = true;
            c->h_lights.assign(st->lights, st->lights + fp.n_lights);
        }
    }
    if (fp.shading != B32_SHADE_NONE && (!c->cur.shades || c->cur.cap_shades < c->cap_work)) {
        if (c->cur.shades) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(c->cur.shades)); c->cur.shades = nullptr; }
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&c->cur.shades), c->cap_work * 9 * sizeof(float)));
        c->cur.cap_shades = c->cap_work;
    }
    return B32_OK;
}

// work buffers every route may need, sized for the uncut 64x64 tile grid (the sort-free path may cut tiles to a quarter of the height:
// 4 x as many list ranges)
static int frame_buffers(b32_ctx* c, const FrameParams& fp, bool wire_back) {
    hipStream_t s = c->stream;
    const uint32_t ntiles = fp.tiles_x * fp.tiles_y;
    int rc;
    // pair buffers: start at 2 pairs per face + one per tile; b32_frame_finish grows them on overflow
    if (c->cap_pairs == 0 || !c->pkeys[0]) {
        const size_t n = (size_t)c->scene.nf * 2 + ntiles + 1024;
        for (int i = 0; i < 2; ++i) { if ((rc = ensure_plain(c, c->pkeys[i], n))) return rc; if ((rc = ensure_plain(c, c->pvals[i], n))) return rc; }
        c->cap_pairs = n;
    }
    const uint32_t need_blocks = std::max((uint32_t)((std::max(c->cap_pairs, c->cap_work) + SORT_TILE - 1) / SORT_TILE) + 1,
                                          (uint32_t)(c->cap_work / 1024 + 2));          // span counting sort: >= 1024 faces per block
    if (need_blocks > c->hist_blocks || !c->block_hist) {
        if ((rc = ensure_plain(c, c->block_hist, (size_t)4096 * need_blocks))) return rc;
        c->hist_blocks = need_blocks;
    }
    const size_t need_ranges = (size_t)4 * ntiles + 4 * fp.tiles_x + 2;      // list ranges: 2 per tile (tile, class), x 4 for cut tiles
    if (need_ranges > c->cap_ranges || !c->ranges) {
        if ((rc = ensure_plain(c, c->ranges, need_ranges + 64))) return rc;
        c->cap_ranges = need_ranges + 64;
    }
    if (need_ranges > c->cap_tile_mid || !c->tile_mid) {
        if ((rc = ensure_plain(c, c->tile_mid, need_ranges + 64))) return rc;
        c->cap_tile_mid = need_ranges + 64;
    }
    if (c->scene.mask_dirty && c->scene.pool_texels) {      // (after the drop-in call's staged copy kernel on the same stream: the texels are there)
        launch_build_mask(s, c->scene.fmt8 ? nullptr : c->scene.d_texels, c->scene.fmt8 ? c->scene.d_texels32 : nullptr, c->scene.pool_texels, c->scene.d_texmask);
        c->scene.mask_dirty = false;
    }
    if (fp.zmode) {          // Framebuffer::zbuffer (render.rs:12): allocated on first use, f32::MAX until drawn into
        const size_t px = (size_t)c->width * c->height;
        if (px > c->cap_zbuf || !c->zbuf) { if ((rc = ensure_plain(c, c->zbuf, px + 64))) return rc; c->cap_zbuf = px; c->zbuf_valid = false; }
        if (!c->zbuf_valid) { launch_clear(s, reinterpret_cast<uint32_t*>(c->zbuf), px, 0x7F7FFFFFu); c->zbuf_valid = true; }
    }
    if ((size_t)c->width * c->height > c->cap_vis || !c->vis) {
        if ((rc = ensure_plain(c, c->vis, (size_t)c->width * c->height * 2 + 64))) return rc;    // two words per pixel (prio64 coverage)
        c->cap_vis = (size_t)c->width * c->height;
    }
    if (fp.wire_collect && c->scene.nf) {
        if ((size_t)c->scene.nf > c->cur.cap_wire || !c->cur.wire) { if ((rc = ensure_plain(c, c->cur.wire, (size_t)c->scene.nf + 16))) return rc; c->cur.cap_wire = c->scene.nf; }
        size_t slots = 1024;
        while (slots < (size_t)c->scene.nf * 6) slots <<= 1;                        // load factor <= 0.5 with all 3*nf edges distinct
        if (wire_back && (slots > c->cap_wire_table || !c->wire_owner)) {
            if ((rc = ensure_plain(c, c->wire_owner, slots))) return rc;
            if ((rc = ensure_plain(c, c->wire_first, slots))) return rc;
            c->cap_wire_table = slots;
        }
        // tile route: one counter and one list region per 64 x 16 wire tile (WIRE_TH rows) of the band (+ the overflow flag and the big-edge count)
        if (!(c->route_off & B32_ROUTE_WIRE_TILES) && c->band_y1 > c->band_y0) {
            const size_t wt = (size_t)fp.tiles_x * ((c->band_y1 - (c->band_y0 / WIRE_TH) * WIRE_TH + WIRE_TH - 1) / WIRE_TH);
            if (wt > c->cur.cap_wire_tiles || !c->cur.wire_fill) {
                if ((rc = ensure_plain(c, c->cur.wire_fill, (wt + 2) * FILL_PAD + 64))) return rc;
                if ((rc = ensure_plain(c, c->cur.wire_lists, wt * WIRE_TILE_CAP + 64))) return rc;
                c->cur.cap_wire_tiles = wt; c->cur.wire_grid = 0;
            }
            // (the counters are zero between frames: k_wire_tile re-zeroes what k_wire_bin counted; a new allocation or another tile grid
            // -- resize, band change -- starts from a cleared array)
            const unsigned long long grid = ((unsigned long long)c->width << 40) ^ ((unsigned long long)c->band_y0 << 20) ^ c->band_y1;
            if (grid != c->cur.wire_grid) {
                HIPCHK(c, hipMemsetAsync(c->cur.wire_fill, 0, ((c->cur.cap_wire_tiles + 2) * FILL_PAD + 64) * sizeof(uint32_t), s));
                c->cur.wire_grid = grid; c->side_dirty = true;          // (a pipelined frame bins on the side stream: behind this memset)
            }
        }
    }
    return B32_OK;
}

// Route selection.  May cut the tile grid (fp.tile_h / tile_yb / tiles_y) and prepares the direct binning's regions.
static int plan_route(b32_ctx* c, FrameParams& fp, const SortScratch& sc, FramePlan& r) {
    const bool wire_front = r.wire_front;
    int rc;
    // z-buffer frames without a transparent pass take the sort-free fused path too (depth is the priority); otherwise z-buffer
    // mode applies depth + skip rule per fragment (EXACT coverage)
    // (a transparent pass rides along: its entries are split off at binning time and sorted per tile by k_blend)
    r.with_class = c->scene.may_blend && !c->scene.fmt8;
    const bool spans_ok = !(c->route_off & B32_ROUTE_SORT_FREE) && c->scene.local_sort_ok && bin_spans_applicable(fp, sc, r.with_class);
    r.ordered_all = c->scene.fmt8 ? c->scene.blend8 : (fp.xray != 0);
    // sort-free path: painter's or z-buffer mode (orthographic keys use all 32 bits -> class pass -> general path)
    r.want_prio64 = spans_ok && !fp.ortho && !r.ordered_all;
    // too few 64x64 tiles to fill the GPU (narrow multi-GPU band, PS1-sized frame): tiles of 32 or 16 rows multiply the parallelism
    // of the fused kernel.  Only the sort-free path knows about them (its k_blend included); the keyed kernels keep 64 rows.
    if (r.want_prio64 && !(c->route_off & B32_ROUTE_CUT_TILES)) {
        static_assert(PLAN_TILE_H == (uint32_t)TILE_H, "b32_frame_plan.h cuts the tiles of b32_device.h");
        const TileGrid g = plan_cut_grid(fp.tiles_x, c->band_y0, c->band_y1, (uint32_t)c->n_cu, (uint32_t)B32_MIN_TILE_H);
        fp.tile_h = g.tile_h; fp.tile_yb = g.tile_yb; fp.tiles_y = g.tiles_y;
    }
    const uint32_t ntiles = r.ntiles = fp.tiles_x * fp.tiles_y;
    // EXACT coverage = texel rule per fragment: exact store counting, textures with many skippable texels; the keyed z-buffer kernel
    // is EXACT by construction
    r.exact_cov = c->count_fragments || !c->scene.cheap_ok || (fp.zmode && !r.want_prio64);
    // the sorted fast path reads the class from bit 31 of the depth key and has no ordered opaque walk: not for ortho / x-ray frames
    r.local_sort = !r.exact_cov && c->scene.local_sort_ok && !fp.ortho && !r.ordered_all && !fp.zmode;
    fp.band_only = (r.want_prio64 && c->band_set) ? 1 : 0;   // other ranks own the other rows: their surfaces' records are never read here
    // small mesh (what the reference's callers submit per room / asset part): no binning launch, the
    // fused kernel's workgroups collect their own tile lists from the spans (needs one list region of nf entries per tile)
    // (with a transparent pass only up to 2048 faces: no tile's transparent list can then exceed what k_blend sorts in LDS)
    r.list_stride = (c->scene.nf + 31u) & ~31u;
    r.want_inline = r.want_prio64 && !wire_front && c->scene.nf <= (r.with_class ? 2048u : 8192u) && (size_t)ntiles * r.list_stride <= ((size_t)4 << 20) &&
                    !(c->route_off & B32_ROUTE_INLINE_BIN);
    // larger meshes: no binning launch either -- k_setup appends every surviving face to fixed-size tile regions (DirectBin)
    if (c->scene.direct_ntiles != ntiles) { c->scene.direct_ntiles = ntiles; c->scene.direct_cap_opaque = 0; c->scene.direct_ok = true; }   // another tile grid (resize, band)
    if (r.want_prio64 && !r.want_inline && !wire_front && c->scene.direct_ok && !(c->route_off & B32_ROUTE_DIRECT_BIN) && ntiles) {
        // first guess: three times the mean list of a mesh whose every face is drawn and touches one tile; a frame that overflows
        // reports its longest list and is redrawn with regions a quarter above it (b32_frame_finish)
        if (!c->scene.direct_cap_opaque) c->scene.direct_cap_opaque = std::max<uint32_t>(512u, (uint32_t)std::min<uint64_t>((uint64_t)3 * c->scene.nf / ntiles + 64, 1u << 24));
        // a mesh of moderate size gets regions that hold ALL its faces (at most 32 MB of list space): such a frame can never overflow a
        // region, needs no redraw, and may stay in flight across scene swaps and further frames like a small mesh's
        if (c->scene.nf <= 65536u && (uint64_t)ntiles * (c->scene.nf + (r.with_class ? BLEND_SORT_CAP : 0u)) <= (8u << 20)) c->scene.direct_cap_opaque = std::max(c->scene.direct_cap_opaque, c->scene.nf);
        const uint32_t cap_o = (c->scene.direct_cap_opaque + 31u) & ~31u;
        const uint32_t region = cap_o + (r.with_class ? BLEND_SORT_CAP : 0u);
        const size_t need = (size_t)ntiles * region + 64;
        if (need <= ((size_t)1 << 28)) {                            // 1 GB of list space at most; beyond that the compact counting sort
            if (need > c->cur.cap_direct || !c->cur.direct_lists) {
                if ((rc = ensure_plain(c, c->cur.direct_lists, need + need / 8))) return rc;
                c->cur.cap_direct = need + need / 8;
            }
            const size_t need_fill = (size_t)ntiles * FILL_PAD + 64;
            if (need_fill > c->cur.cap_tile_fill || !c->cur.tile_fill) {
                if ((rc = ensure_plain(c, c->cur.tile_fill, need_fill * 2))) return rc;
                c->cur.cap_tile_fill = need_fill * 2;
                HIPCHK(c, hipMemsetAsync(c->cur.tile_fill, 0, c->cur.cap_tile_fill * sizeof(uint32_t), c->stream));   // zero from here on: k_cover re-zeroes what k_setup counted
                c->side_dirty = true;
            }
            if (++c->epoch == 0) c->epoch = 1;
            r.db.fill = c->cur.tile_fill; r.db.lists = c->cur.direct_lists; r.db.region = region; r.db.cap_opaque = cap_o;
            r.db.cap_transparent = r.with_class ? BLEND_SORT_CAP : 0u; r.db.with_class = r.with_class ? 1u : 0u; r.db.epoch = c->epoch;
            r.direct_bin = true;
            r.list_stride = region;
        } else c->scene.direct_ok = false;
    }
    // (the small mesh's list regions: allocated here, in front of every launch of the frame -- growing them synchronises the stream and
    // frees the old buffer, which must not happen between a frame's setup kernel and its fill)
    if (!r.direct_bin && r.want_inline) {
        const size_t need = (size_t)ntiles * r.list_stride + 64;
        if (need > c->cap_inline) {
            if ((rc = ensure_plain(c, c->inline_lists, need + need / 2))) return rc;
            c->cap_inline = need + need / 2;
        }
        r.inline_bin = true;
    }
    r.set_prio64(r.direct_bin || r.inline_bin);        // (a span-binned frame: decided when the binning has run, tile_lists)
    return B32_OK;
}

// frames of a mesh that stays (second frame on) and is too large for the in-kernel list collection: k_setup culls and bins every face
// from packed positions and reads the packed (u, v, rgba) only of the faces it draws (on a band-sharded frame: that reach this rank's rows)
static int frame_positions(b32_ctx* c, const FrameParams& fp, const float*& pos12, const float*& attr12) {
    int rc;
    pos12 = attr12 = nullptr;
    if (c->scene.nv && c->scene.nf > 8192u && !(c->route_off & B32_ROUTE_PACKED_STREAMS)) {
        // streams per vertex, one behind the other: 12 B positions, 12 B (u, v, rgba) and -- only once the mesh has been drawn with a
        // shading pass -- 24 B (u, v, rgba, normal) for lit frames (floats: 3 + 3 [+ 6] per vertex)
        const bool want_lit = fp.shading != B32_SHADE_NONE;
        if ((!c->scene.pos_valid || (want_lit && !c->scene.lit_valid)) && c->scene.band_frames >= 1) {
            const bool with_lit = want_lit || c->scene.lit_valid;
            const size_t need = (size_t)c->scene.nv * (with_lit ? 12 : 6);
            if (need > c->scene.cap_pos12 || !c->scene.d_pos12) {
                if ((rc = ensure_plain(c, c->scene.d_pos12, need + 16))) return rc;
                c->scene.cap_pos12 = need;
            }
            launch_pack_streams(c->stream, c->scene.d_verts, c->scene.nv, c->scene.d_pos12, c->scene.d_pos12 + (size_t)c->scene.nv * 3, with_lit);
            c->scene.pos_valid = true; c->scene.lit_valid = with_lit; c->side_dirty = true;
        }
        c->scene.band_frames++;
        if (c->scene.pos_valid && (!want_lit || c->scene.lit_valid)) { pos12 = c->scene.d_pos12; attr12 = c->scene.d_pos12 + (size_t)c->scene.nv * 3; }
    }
    return B32_OK;
}

// The keyed pipelines (no sort-free path for this frame): pairs keyed by (tile, class), grouped by radix passes; returns the pair buffer
// that holds the grouped lists (FramePlan::pair_buf).  ev_bin: event to record when the binning proper starts (profiling level 2), or nullptr.
static int bin_keyed(b32_ctx* c, const FrameParams& fp, FramePlan& r, const SortScratch& sc, hipEvent_t ev_bin) {
    hipStream_t s = c->stream;
    const uint32_t ntiles = r.ntiles;
    int& cur = r.pair_buf;
    cur = 0;
    if (r.local_sort) {
        // fast path: no global depth sort.  Pairs are emitted in face order from k_setup's spans; k_cover sorts every tile
        // list by depth key in LDS (stable, so ties keep face order).
        if (ev_bin) HIPCHK(c, hipEventRecord(ev_bin, s));
        launch_bin_faces(s, fp, c->cur.spans, c->cur.keys0, c->cur.partials, c->cur.d_ctrl, c->pkeys[0], c->pvals[0], (uint32_t)c->cap_pairs, 0);
    } else {
        // painter's order: 4 stable passes over the 32-bit key; pass 1 also compacts away culled faces and its scan kernel
        // reduces k_setup's counters into Ctrl (n_visible feeds the later passes).
        RadixExtra ex1; ex1.post_ctrl = c->cur.d_ctrl; ex1.partials = c->cur.partials; ex1.npart = (c->scene.nf + 255) / 256;
        launch_radix_pass(s, c->cur.keys0, nullptr, c->keys1, c->vals[1], c->scene.d_consts, c->scene.nf, 0, 8, sc, ex1);
        launch_radix_pass(s, c->keys1, c->vals[1], c->cur.keys0, c->vals[0], &c->cur.d_ctrl->n_visible, c->scene.nf, 8, 8, sc);
        launch_radix_pass(s, c->cur.keys0, c->vals[0], c->keys1, c->vals[1], &c->cur.d_ctrl->n_visible, c->scene.nf, 16, 8, sc);
        launch_radix_pass(s, c->keys1, c->vals[1], c->cur.keys0, c->vals[0], &c->cur.d_ctrl->n_visible, c->scene.nf, 24, 8, sc);
        if (fp.ortho) {      // 32-bit depth keys: the opaque/transparent partition is a fifth stable pass on the class
            launch_class_keys(s, c->cur.crecs, c->vals[0], &c->cur.d_ctrl->n_visible, c->scene.nf, c->cur.keys0);
            launch_radix_pass(s, c->cur.keys0, c->vals[0], c->keys1, c->vals[1], &c->cur.d_ctrl->n_visible, c->scene.nf, 0, 8, sc);
            HIPCHK(c, hipMemcpyAsync(c->vals[0], c->vals[1], (size_t)c->scene.nf * 4, hipMemcpyDeviceToDevice, s));
        }
        if (ev_bin) HIPCHK(c, hipEventRecord(ev_bin, s));
        launch_bin(s, fp, c->cur.spans, c->vals[0], c->cur.d_ctrl, c->counts, c->block_sums, c->bin_blocks, c->pkeys[0], c->pvals[0], (uint32_t)c->cap_pairs);
    }
    const uint32_t n_sort_keys = r.local_sort ? ntiles : 2 * ntiles;          // the fast path groups by tile only
    const uint32_t kb = bits_for(n_sort_keys ? n_sort_keys : 1);
    if (kb <= 8 || kb > 12) {
        for (uint32_t shift = 0; shift < kb; shift += 8) {
            launch_radix_pass(s, c->pkeys[cur], c->pvals[cur], c->pkeys[cur ^ 1], c->pvals[cur ^ 1], &c->cur.d_ctrl->n_pairs, (uint32_t)c->cap_pairs, (int)shift, 8, sc);
            cur ^= 1;
        }
        launch_tile_ranges(s, c->pkeys[cur], c->cur.d_ctrl, (uint32_t)c->cap_pairs, c->ranges, n_sort_keys);
    } else {    // up to 2048 tiles: one pass groups every (tile, class) list and its digit bases are the list ranges
        RadixExtra exr; exr.ranges_out = c->ranges; exr.n_ranges = n_sort_keys + 1;
        launch_radix_pass(s, c->pkeys[cur], c->pvals[cur], c->pkeys[cur ^ 1], c->pvals[cur ^ 1], &c->cur.d_ctrl->n_pairs, (uint32_t)c->cap_pairs, 0, kb <= 11 ? 11 : 12, sc, exr);
        cur ^= 1;
    }
    return B32_OK;
}

static FillArgs fill_args(const b32_ctx* c, const FrameParams& fp, const FramePlan& r) {
    FillArgs fa{};
    fa.fp = fp; fa.crecs = c->cur.crecs; fa.srecs = c->cur.srecs; fa.xrecs = c->cur.xrecs; fa.shades = c->cur.shades; fa.pair_vals = c->pvals[r.pair_buf]; fa.ranges = c->ranges;
    fa.keys = c->cur.keys0; fa.local_sort = r.local_sort ? 1u : 0u; fa.tile_keys_only = (r.local_sort || r.prio64) ? 1u : 0u; fa.tile_mid = c->tile_mid;
    fa.tex = c->scene.d_tex; fa.texels = c->scene.d_texels; fa.fb = c->fb; fa.vis = c->vis; fa.zbuf = c->zbuf; fa.ctrl = c->cur.d_ctrl;
    fa.tex0 = c->scene.nt ? c->scene.h_tex[0] : TexDesc{ 0, 0, 0, 0 };
    fa.lds_tex_texels = 0;
    if (c->scene.nt == 1 && r.exact_cov) {                     // (CHEAP coverage: one texel fetch per output pixel, served by L1/L2)
        const size_t n = (size_t)c->scene.h_tex[0].width * c->scene.h_tex[0].height;
        if (n > 0 && n * 2 <= fill_lds_tex_budget()) fa.lds_tex_texels = (uint32_t)n;
    }
    fa.exact_coverage = r.exact_cov ? 1u : 0u;
    fa.may_blend = c->scene.may_blend ? 1u : 0u;
    fa.skip_solid = r.wire_front ? 1u : 0u;
    fa.texels32 = c->scene.d_texels32;
    fa.ordered_all = r.ordered_all ? 1u : 0u;
    fa.fused = r.fused ? 1u : 0u;
    fa.wide = r.wide ? 1u : 0u;
    fa.texmask = c->scene.d_texmask;
    { const uint32_t words = c->scene.pool_texels / 32 + 2; fa.mask_lds_words = (c->scene.pool_texels && words <= MASK_LDS_MAX_WORDS) ? words : 0u; }
    fa.inline_bin = r.inline_bin ? 1u : 0u; fa.list_stride = r.list_stride; fa.spans = c->cur.spans; fa.partials = c->cur.partials;
    if (r.inline_bin) fa.pair_vals = c->inline_lists;
    fa.direct_bin = r.direct_bin ? 1u : 0u; fa.tile_fill = c->cur.tile_fill; fa.epoch = c->epoch;
    if (r.direct_bin) fa.pair_vals = c->cur.direct_lists;
    fa.gather_blend = (r.prio64 && r.with_class) ? 1u : 0u;
    fa.stagger = (c->route_off & B32_ROUTE_STAGGER) ? 0u : 1u;       // (launch_fill decides whether the frame qualifies)
    fa.span_cover = (r.prio64 && !r.exact_cov && !fp.zmode && !(c->route_off & B32_ROUTE_SPAN_COVER)) ? 1u : 0u;
    // index atlas + CLUT sampled from LDS: the fused kernel with one indexed texture, when they fit beside the tile planes of the
    // workgroup form launch_fill is told to launch (16 waves, one workgroup per CU: ~84 KB; two 8-wave workgroups per CU: ~6 KB)
    fa.atlas0 = c->scene.d_atlas0; fa.atlas_idx_bytes = 0;
    if (r.prio64 && !c->scene.fmt8 && c->scene.nt == 1 && c->scene.atlas_idx_bytes && !(c->route_off & B32_ROUTE_LDS_ATLAS) &&
        c->scene.atlas_idx_bytes + ATLAS_CLUT_BYTES + 16u <= fill_lds_atlas_room(r.wide))
        fa.atlas_idx_bytes = c->scene.atlas_idx_bytes;
    if (c->scene.fmt8) fa.fp.xray = 0;                        // render_mesh: x-ray only changes culling; its stores keep their own depth tests
    return fa;
}

// ------------------------------------------------------------------ the steps of enqueue_frame, in the order it calls them
// Two frames in flight: when an earlier frame of this context is still pending, this frame of a large mesh takes the OTHER frame set
// and (if it ends up on the direct-binning route) its setup kernel runs on the side stream, beside that frame's fill.
static int choose_frame_set(b32_ctx* c, const FramePlan& r, SetsGuard& sets) {
    c->pipelined = false;
    // (pipe_hint: whether the previous frame's route qualified -- a frame that will not, e.g. every frame of a PS1-sized target, skips
    // the set swap and its event as well: 0.030 -> 0.028 ms on 20 k triangles at 320x240)
    const uint32_t pipe_min_faces = 2048u;
    // (not on the legacy default stream -- hipStreamLegacy, what torch's default stream maps to: it synchronises implicitly with every
    // blocking stream, and recording / waiting cross-stream events on that handle crashed the runtime, found when safe mode began to
    // leave superseded frames in flight)
    if (!(c->frame_pending && c->pipe_hint && !c->redrawing && !r.prof_all && c->scene.nf > pipe_min_faces && !(c->route_off & B32_ROUTE_PIPELINE) &&
          c->stream != hipStreamLegacy))
        return B32_OK;
    int rc;
    if ((rc = pipeline_ensure(c))) return rc;
    sets.rotate();
    c->pipelined = true;
    if (c->join_stream != c->stream) {
        // Streams of different priorities never share a hardware queue (the runtime pools its queues by priority); two streams of ONE
        // priority may, and k_join in front of k_flag in the same queue would wait for its patience: those keep the event.
        int pm = 0, ps = 0;
        c->join_ok = hipStreamGetPriority(c->stream, &pm) == hipSuccess && hipStreamGetPriority(c->side, &ps) == hipSuccess && pm != ps;
        c->join_stream = c->stream;
    }
    return B32_OK;
}

// the frame's row of profiling events (created on first use)
static int profiling_row(b32_ctx* c, FramePlan& r) {
    if (!r.prof_fill) return B32_OK;
    if (!c->ev_created) {
        for (auto& fr : c->ev) for (auto& e : fr) if (hipEventCreate(&e) != hipSuccess) return B32_E_HIP;
        c->ev_created = true;
    }
    r.ev = c->ev[c->ev_frames % EV_RING];
    return B32_OK;
}

// What follows from the route for the two frame sets: whether the NEXT frame may rotate (pipe_hint), whether this one keeps the side
// stream, its hand-over, and the fused kernel's workgroup form.  What b32_frame_finish needs to know about the route is noted here too.
static void plan_pipeline(b32_ctx* c, const FrameParams& fp, FramePlan& r) {
    const bool join_small = !c->frame_batched && (c->join_stream != c->stream || c->join_ok);
    c->pipe_hint = plan_pipe_hint(r.direct_bin, r.ntiles, (uint32_t)c->n_cu, c->frame_batched, join_small);
    if (!c->pipe_hint) c->pipelined = false;       // (the frame keeps the set it rotated to -- the route's regions are that set's -- but runs on the main stream)
    c->last_local_sort = r.local_sort || r.want_prio64;                         // the global draw order is not materialised
    c->last_exact = r.ordered_all ? true : (r.exact_cov && !fp.zmode);          // the ordered walk counts every store it performs
    c->last_direct = r.direct_bin;
    const bool narrow_only = (c->route_off & B32_ROUTE_WIDE_GROUPS) != 0;
    r.wide = plan_wide(r.ntiles, (uint32_t)c->n_cu, narrow_only);
    r.hand_over_kind = plan_hand_over({ c->pipelined, c->frame_batched, c->join_ok, r.direct_bin, r.wire_front, r.ordered_all, r.ntiles, (uint32_t)c->n_cu, narrow_only });
}

// an empty mesh launches no setup kernel: the control block it would have reset (all but `sticky`)
static int reset_ctrl_of_empty_frame(b32_ctx* c) {
    if (c->scene.nf) return B32_OK;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemsetAsync(c->cur.d_ctrl, 0, offsetof(Ctrl, sticky), s));
    HIPCHK(c, hipMemsetAsync(&c->cur.d_ctrl->fragments, 0, sizeof(unsigned long long), s));
    HIPCHK(c, hipMemsetAsync(c->cur.d_ctrl + 1, 0, sizeof(Stamps), s));          // (and the phase clock: b32_last_shader_clock of an empty frame is 0, not the frame before's)
    return B32_OK;
}

// A pipelined frame's setup kernel runs on the side stream: behind whatever the main stream wrote that it reads (side_dirty), behind the
// last reader of the frame set it writes (start gate, or an event), and -- b32_set_pipeline_gate -- behind the tail of the fill in front.
static int order_side_stream(b32_ctx* c, FramePlan& r) {
    hipStream_t s = c->stream;
    r.setup_stream = s;
    if (!c->pipelined) return B32_OK;
    if (c->side_dirty) { HIPCHK(c, hipEventRecord(c->ev_main, s)); HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_main, 0)); c->side_dirty = false; }
    r.setup_stream = c->side;
    c->pipelined_frames++;
    uint32_t polled_tiles = 0, polled_groups = 0, polled_seq = 0;       // the fused kernel of the frame whose cursor the gate polls (alt[0]: n_sets - 1 frames back)
    for (const auto& co : c->cover_of) if (co.ctrl && co.ctrl == c->alt[0].d_ctrl) { polled_tiles = co.tiles; polled_groups = co.groups; polled_seq = co.seq; }
    // The set this frame's setup kernel writes was last read by the fill n_sets frames back.  That fill lies in front of alt[0]'s on the main
    // stream: when alt[0]'s frame launched a fused kernel, "it has started" orders the two on the device (k_gate, no event on the main
    // stream); else the side stream waits for the main stream as it stands now.
    const bool start_gate = polled_tiles && polled_seq && c->alt[0].d_ctrl;
    if (!start_gate) { HIPCHK(c, hipEventRecord(c->ev_main, s)); HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_main, 0)); }
    const uint32_t gate_need = c->alt[0].d_ctrl ? plan_gate_need(c->gate_permille, polled_tiles, polled_groups) : 0u;
    // (b32_debug_inject(ctx, 2): the fill in front did not publish its start -- this gate's patience is 2 ms, then the error)
    const uint32_t start_patience = c->start_lost ? PATIENCE_INJECTED_TICKS : PATIENCE_TICKS;
    c->start_lost = false;                               // (one gate only, whichever way this frame is ordered)
    if (gate_need || start_gate) launch_gate(c->side, c->alt[0].d_ctrl, gate_need, 30000u /* 300 us */, start_gate ? polled_seq : 0u, c->cur.d_ctrl, start_patience);      // alt[0]: the frame n_sets - 1 back (rotate_sets)
    return B32_OK;
}

// the wire kernels' arguments: known before the setup kernel is launched -- a pipelined frame bins its wire list on the side stream
static void wire_args(b32_ctx* c, const FrameParams& fp, FramePlan& r) {
    r.wire_on = fp.wire_collect && c->scene.nf;
    if (!r.wire_on) return;
    WireArgs& wa = r.wa;
    wa.tris = c->cur.wire; wa.nf = c->scene.nf; wa.table_owner = c->wire_owner; wa.table_first = c->wire_first;
    wa.table_mask = c->cap_wire_table ? (uint32_t)(c->cap_wire_table - 1) : 0;
    wa.fb = c->fb; wa.zbuf = (c->zbuf && c->zbuf_valid) ? c->zbuf : nullptr;
    wa.width = c->width; wa.height = c->height; wa.band_y0 = c->band_y0; wa.band_y1 = c->band_y1; wa.ctrl = c->cur.d_ctrl;
    if (++c->wire_seq == 0) c->wire_seq = 1;
    wa.epoch = c->wire_seq;
    if (!(c->route_off & B32_ROUTE_WIRE_TILES) && c->cur.wire_fill && c->band_y1 > c->band_y0) {
        wa.tile_yb = (c->band_y0 / WIRE_TH) * WIRE_TH; wa.tiles_x = (c->width + TILE_W - 1) / TILE_W;
        wa.tiles_y = (c->band_y1 - wa.tile_yb + WIRE_TH - 1) / WIRE_TH;
        if ((size_t)wa.tiles_x * wa.tiles_y <= c->cur.cap_wire_tiles) { wa.tile_fill = c->cur.wire_fill; wa.tile_lists = c->cur.wire_lists; c->wire_tile_frames++; }
    }
}

// the setup kernel's arguments: the resident scene, the frame's lights and tables, and the frame set it writes
static SetupArgs setup_args(const b32_ctx* c, const FrameParams& fp, const FramePlan& r, const LightSet& lset) {
    SetupArgs a{};
    a.fp = fp; a.lset = lset; a.mtab = c->frame_table; a.ptab = c->frame_places;
    SetupBuffers& b = a.buf;
    b.verts = c->scene.d_verts; b.faces = c->scene.d_faces; b.tex = c->scene.d_tex; b.lights = c->d_lights;
    b.recs = RecArrays{ c->cur.crecs, c->cur.srecs, c->cur.xrecs }; b.db = r.db;
    b.shades = c->cur.shades; b.keys = c->cur.keys0;
    b.spans = r.direct_bin ? nullptr : c->cur.spans;      // (direct binning: nobody reads the spans)
    b.partials = c->cur.partials; b.ctrl = c->cur.d_ctrl; b.wire = c->cur.wire;
    b.pos12 = r.pos12; b.attr12 = r.attr12; b.face_of = c->cur.face_of;
    return a;
}

// b32_debug_inject(ctx, 1): the next hand-over's flag carries another value and whoever waits for it has a patience of 2 ms -- the "setup
// kernel never arrived" path.  Taken by one hand-over.
static bool take_lost_flag(b32_ctx* c) {
    const bool lose_flag = (c->inject & 1u) != 0;
    c->inject &= ~1u;
    return lose_flag;
}

// The main stream is made to wait for the setup kernel just launched on the side stream, by the hand-over the plan chose (the decision and
// its measurements: plan_hand_over).  Then the early wire binning, on the side stream behind the setup kernel: the fill does not wait for it.
// On return everything this frame has on the side stream lies in front of main-stream work.
static int hand_over(b32_ctx* c, FramePlan& r) {
    hipStream_t s = c->stream;
    if (r.hand_over_kind == HandOver::Poll) {          // the fused kernel polls the word itself (FillArgs::join_seq)
        const bool lose_flag = take_lost_flag(c);
        if (++c->join_seq == 0) c->join_seq = 1;
        launch_flag_poll(c->side, c->cur.d_ctrl, lose_flag ? c->join_seq ^ 0x40000000u : c->join_seq);
        r.poll_seq = c->join_seq; r.poll_patience = lose_flag ? PATIENCE_INJECTED_TICKS : PATIENCE_TICKS;
        c->flag_join_frames++; c->poll_join_frames++;
    } else if (r.hand_over_kind == HandOver::FlagJoin) {
        const bool lose_flag = take_lost_flag(c);
        launch_flag(c->side, c->cur.d_ctrl, lose_flag ? c->epoch ^ 0x40000000u : c->epoch);
        launch_join(s, c->cur.d_ctrl, c->epoch, lose_flag ? PATIENCE_INJECTED_TICKS : PATIENCE_TICKS);
        c->flag_join_frames++;
    } else if (r.hand_over_kind == HandOver::Event) {
        hipError_t e1 = hipEventRecord(c->cur.ev_setup, c->side);
        if (e1 == hipSuccess) e1 = hipStreamWaitEvent(s, c->cur.ev_setup, 0);
        // (the setup kernel is in flight and nothing orders the main stream behind it: wait for it here)
        if (e1 != hipSuccess) { (void)hipStreamSynchronize(c->side); c->last_hip = (int)e1; return B32_E_HIP; }
        c->event_join_frames++;
    }
    if (c->pipelined && r.wire_on && r.wa.tile_fill) {       // (behind ev_setup: the fill does not wait for the binning)
        launch_wire_bin(c->side, r.wa, r.wire_back, r.wire_front, true);
        // (back-face edges: the first wire kernel on the main stream, k_wire_table_clear, looks at Events::wbin_done itself -- no event
        // for the main stream to wait for; the overlay alone has no such kernel in front of k_wire_tile and keeps the event)
        if (r.wire_back) { launch_flag_wbin(c->side, c->cur.d_ctrl, r.wa.epoch); r.wire_polled = true; }
        else HIPCHK(c, hipEventRecord(c->ev_wbin, c->side));
        r.wire_binned = true;
    }
    c->cur.in_flight = true;
    if (r.prof_all) HIPCHK(c, hipEventRecord(r.ev[1], s));
    return B32_OK;
}

// The tile lists the fill reads.  Direct and inline binning launch nothing here (k_setup and the fused kernel build them); a sort-free frame
// that is neither bins its spans with a counting sort, and falls back to the keyed pipelines when that does not apply.
static int tile_lists(b32_ctx* c, const FrameParams& fp, const SortScratch& sc, FramePlan& r) {
    hipStream_t s = c->stream;
    int rc;
    if (r.prof_all && r.want_prio64) HIPCHK(c, hipEventRecord(r.ev[2], s));
    if (r.want_prio64 && !r.prio64)
        r.set_prio64(launch_bin_spans(s, fp, c->cur.spans, r.with_class ? c->cur.keys0 : nullptr, c->cur.partials, c->cur.d_ctrl, sc, (uint32_t)c->cap_pairs, c->ranges,
                                      c->tile_mid, BLEND_SORT_CAP, c->pvals[0]));
    if (!r.prio64 && (rc = bin_keyed(c, fp, r, sc, r.prof_all ? r.ev[2] : nullptr))) return rc;
    c->routes[r.direct_bin ? 0 : r.inline_bin ? 1 : r.prio64 ? 2 : 3]++;
    // (direct binning with regions that hold the whole mesh, and no more faces that can be transparent than k_blend sorts per tile:
    // nothing can overflow)
    const bool direct_safe = r.direct_bin && r.db.cap_opaque >= c->scene.nf && (!r.with_class || c->scene.blend_faces <= BLEND_SORT_CAP);
    c->pending_may_redraw = !(r.inline_bin || direct_safe);
    if (r.prof_fill) HIPCHK(c, hipEventRecord(r.ev[3], s));
    return B32_OK;
}

// coverage, shading, transparent pass: the fill's arguments, the words it publishes and polls, a deferred clear, the launch
static int fill(b32_ctx* c, const FrameParams& fp, FramePlan& r) {
    const bool fused = r.fused;
    int rc;
    FillArgs fa = fill_args(c, fp, r);
    if (++c->fill_seq == 0) c->fill_seq = 1;
    fa.start_seq = r.start_seq = c->fill_seq;
    fa.join_seq = r.poll_seq; fa.join_patience = r.poll_patience;
    if ((c->inject & 2u) && fused && r.ntiles) { c->inject &= ~2u; fa.start_seq = 0; c->start_lost = true; }    // (fault injection: see b32_debug_inject)
    // Which kernel of the frame says "started": the fused kernel -- or, when the frame has a transparent pass, that pass (k_blend, the next
    // kernel on the main stream).  The next frame's setup kernel is released by that word, i.e. it then runs beside the blend kernel and the
    // fill has the GPU to itself: C3 with 10 % transparent faces 0.227 -> 0.192 ms per frame, the same in z-buffer mode 0.264 -> 0.222 (the fill
    // is the kernel that suffers from company: 97 us beside a setup kernel, 82 alone; k_blend 127 either way).  The wire tile kernel of
    // default() in that role: 0.284 -> 0.331 -- its setup kernel is the long one and then starts too late; not done.
    // Only frames that fill the GPU (more tiles than workgroup slots): a console-sized draw leaves most CUs idle anyway and its setup kernel is
    // a chain of round trips that wants to start as early as it may (12-room console frame with the deferral: 0.171 -> 0.213 ms).
    fa.start_defer = (fused && r.ntiles > 2u * (uint32_t)c->n_cu && fa.gather_blend) ? 1u : 0u;
    // a deferred Framebuffer::clear: folded into this frame's fused kernel when that kernel is the one that runs, the frame has no
    // depth buffer to reset and the clear was issued for this very band; else the clear launches go first
    if (c->clear_pending) {
        // (a frame with a depth buffer to reset: only in z-buffer mode, where the fused kernel owns the depth buffer too -- it seeds its
        // winners with f32::MAX instead of reading the buffer and writes f32::MAX where nothing is drawn)
        const bool has_z = c->zbuf && c->zbuf_valid;
        if (fused && (!has_z || fp.zmode) && c->scene.nf && r.ntiles && c->clear_y0 == c->band_y0 && c->clear_y1 == c->band_y1) {
            fa.clear_on = 1; fa.clear_rgba = c->clear_rgba; fa.clear_depth = (has_z && fp.zmode) ? 1u : 0u; c->clear_pending = false;
        } else if ((rc = flush_clear(c))) return rc;
    }
    if (fa.atlas_idx_bytes && fused) c->lds_atlas_frames++;
    if (fa.span_cover && fused) c->span_cover_frames++;
    launch_fill(c->stream, fa, c->n_cu, r.prof_fill ? r.ev[4] : nullptr);
    return B32_OK;
}

// the wireframe phases on the main stream (behind the early binning of a pipelined frame), and the end of the frame's profiling row
static int wire_phases(b32_ctx* c, FramePlan& r) {
    hipStream_t s = c->stream;
    if (r.wire_on && r.wire_binned && !r.wire_polled) HIPCHK(c, hipStreamWaitEvent(s, c->ev_wbin, 0));
    if (r.wire_on) launch_wire(s, r.wa, r.wire_back, r.wire_front, r.wire_binned, r.wire_polled ? c->cur.d_ctrl : nullptr, r.wa.epoch);
    if (r.prof_all) HIPCHK(c, hipEventRecord(r.ev[5], s));
    if (r.prof_fill) c->ev_frames++;
    return B32_OK;
}

// What the gates of the frames that follow need to know about this frame's fused kernel, per frame set (keyed by its control block): its
// tile count (0: it launched none), its workgroups, the start word it was meant to publish.
static void remember_cover(b32_ctx* c, const FramePlan& r) {
    const uint32_t tiles = r.fused ? r.ntiles : 0u;
    b32_ctx::CoverOf* slot = &c->cover_of[0];
    for (auto& co : c->cover_of) { if (co.ctrl == c->cur.d_ctrl) { slot = &co; break; } if (!co.ctrl) slot = &co; }
    *slot = { c->cur.d_ctrl, tiles, std::min<uint32_t>(r.ntiles, (uint32_t)c->n_cu * 2u), tiles ? r.start_seq : 0u };
}

// One frame on the GPU: called by the drop-in calls, the resident scenes, every draw of a batched frame and every redraw.
int enqueue_frame(b32_ctx* c, const B32Camera* cam, const B32Settings* st, const B32Fog* fog) {
    FramePlan r;
    r.wire_back = st->backface_cull && st->backface_wireframe;      // render.rs:2577
    r.wire_front = st->wireframe_overlay != 0;                       // render.rs:2603 (an empty list draws nothing either way)
    FrameParams fp = frame_params(c, cam, st, fog, r.wire_back || r.wire_front);
    LightSet lset{};
    r.prof_fill = c->profile_level >= 1 && (c->prof_seq++ % c->prof_stride) == 0;
    r.prof_all = r.prof_fill && c->profile_level >= 2;
    int rc;
    // ---- everything that can fail without a trace: buffers, the plan, the stream order.  A return in here puts the frame sets back.
    SetsGuard sets(c);
    if ((rc = choose_frame_set(c, r, sets))) return rc;
    if ((rc = frame_lights(c, st, fp, lset))) return rc;
    if ((rc = frame_buffers(c, fp, r.wire_back))) return rc;
    if ((rc = profiling_row(c, r))) return rc;
    const SortScratch sc{ c->block_hist, c->hist_blocks, c->digit_total };
    if ((rc = plan_route(c, fp, sc, r))) return rc;
    plan_pipeline(c, fp, r);
    if ((rc = reset_ctrl_of_empty_frame(c))) return rc;
    if ((rc = frame_positions(c, fp, r.pos12, r.attr12))) return rc;
    if ((rc = order_side_stream(c, r))) return rc;
    wire_args(c, fp, r);
    if (r.prof_all) HIPCHK(c, hipEventRecord(r.ev[0], c->stream));
    // ---- transform, cull, setup (+ tile binning of large meshes): from here on the frame is in flight in the set it rotated to
    sets.dismiss();
    launch_setup(r.setup_stream, setup_args(c, fp, r, lset));
    if ((rc = hand_over(c, r))) return rc;
    if ((rc = tile_lists(c, fp, sc, r))) return rc;
    if ((rc = fill(c, fp, r))) return rc;
    if ((rc = wire_phases(c, r))) return rc;
    remember_cover(c, r);
    HIPCHK(c, hipGetLastError());
    return B32_OK;
}

int b32_render_scene_15_async(b32_ctx* c, const B32Camera* cam, const B32Settings* st, const B32Fog* fog) {
    if (!c || c->scene.fmt8) return B32_E_ARG;                 // the resident scene holds Texture (8-bit) texels: use b32_render_scene
    c->frame_batched = false;
    return render_scene_async_any(c, cam, st, fog, nullptr);
}
int b32_render_scene_async(b32_ctx* c, const B32Camera* cam, const B32Settings* st) {
    if (!c || !c->scene.fmt8) return B32_E_ARG;
    c->frame_batched = false;
    return render_scene_async_any(c, cam, st, nullptr, nullptr);
}
// the resident scene on its own, placed: render_asset_parts' two branches (scene.rs:163-169) behind one entry
int b32_render_scene_15_placed_async(b32_ctx* c, const B32Camera* cam, const B32Settings* st, const B32Fog* fog, const B32Placement* place) {
    if (!c) return B32_E_ARG;
    c->frame_batched = false;
    return render_scene_async_any(c, cam, st, c->scene.fmt8 ? nullptr : fog, place);      // (render_mesh takes no fog)
}
int render_scene_async_any(b32_ctx* c, const B32Camera* cam, const B32Settings* st, const B32Fog* fog, const B32Placement* place) {
    if (!c || !cam || !st || !c->fb || !c->scene.have_scene) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    int rc = validate_settings(st);
    if (rc) return rc;
    // keep a private copy of the lights so a redraw after overflow does not dereference a dead caller pointer
    // (safe mode) a pending frame that may still need a redraw is settled before the next one overwrites its control block
    // (... unless a clear of the whole band has superseded it: b32_fb_clear)
    if (!c->deep_async && !(c->pending_superseded && c->clear_pending) && (rc = settle_pending(c))) return rc;
    c->pending_superseded = false;
    // (behind the settle: a redraw of the pending frame above used the placement THAT frame was enqueued with)
    if (!c->frame_batched) { c->frame_placed = place != nullptr; if (place) c->frame_places.p[0] = *place; }
    c->last_cam = *cam; c->last_settings = *st; c->last_has_fog = fog != nullptr;
    if (fog) c->last_fog = *fog;
    c->keep_lights.assign(st->lights, st->lights + (st->lights ? st->n_lights : 0));
    c->last_settings.lights = c->keep_lights.empty() ? nullptr : c->keep_lights.data();
    rc = enqueue_frame(c, cam, &c->last_settings, fog);
    if (rc == B32_OK) c->frame_pending = true;
    return rc;
}

static void collect_events(b32_ctx* c) {
    c->phase_frames = 0;
    for (float& p : c->phase_ms) p = 0;
    if (!c->ev_created || c->ev_frames == 0 || c->profile_level < 1) { c->ev_frames = 0; return; }
    const uint32_t n = c->ev_frames < (uint32_t)EV_RING ? c->ev_frames : (uint32_t)EV_RING;
    for (uint32_t i = 0; i < n; ++i) {
        float ms = 0;
        if (c->profile_level >= 2) {
            for (int p = 0; p < 3; ++p) if (hipEventElapsedTime(&ms, c->ev[i][p], c->ev[i][p + 1]) == hipSuccess) c->phase_ms[p] += ms;
            if (hipEventElapsedTime(&ms, c->ev[i][4], c->ev[i][5]) == hipSuccess) c->phase_ms[4] += ms;
        }
        if (hipEventElapsedTime(&ms, c->ev[i][3], c->ev[i][4]) == hipSuccess) c->phase_ms[3] += ms;     // the coverage kernel alone
    }
    for (float& p : c->phase_ms) p /= (float)n;
    c->phase_frames = n;
    c->phase_level = c->profile_level;
    c->ev_frames = 0;
}

// The pending frame drew nothing (it reported what it ran out of): the same frame again, counted under b32_route_count(route_index).
static int redraw_pending(b32_ctx* c, int route_index) {
    c->routes[route_index]++;
    c->ev_frames = 0;                                  // the aborted frame must not enter the phase averages
    c->redrawing = true;
    const int rc = enqueue_frame(c, &c->last_cam, &c->last_settings, c->last_has_fog ? &c->last_fog : nullptr);
    c->redrawing = false;
    return rc;
}

int b32_frame_finish(b32_ctx* c, B32Timings* out) {
    if (!c) return B32_E_ARG;
    (void)hipSetDevice(c->device);
    if (out) memset(out, 0, sizeof(*out));
    // A clear issued after the frame's draw (deep mode: safe mode settled the frame before it recorded the clear) stays deferred until
    // the frame has been settled: a redraw below must land UNDER that clear, not on top of it, and must not fold it either.
    const bool later_clear = c->frame_pending && c->clear_pending;
    const uint32_t lc_rgba = c->clear_rgba, lc_y0 = c->clear_y0, lc_y1 = c->clear_y1;
    if (later_clear) c->clear_pending = false;
    struct ClearAfter {      // re-arms and flushes the later clear on every exit path
        b32_ctx* c; bool on; uint32_t rgba, y0, y1;
        ~ClearAfter() { if (on) { c->clear_pending = true; c->clear_rgba = rgba; c->clear_y0 = y0; c->clear_y1 = y1; (void)flush_clear(c); (void)hipStreamSynchronize(c->stream); } }
    } clear_after{ c, later_clear, lc_rgba, lc_y0, lc_y1 };
    // A superseded frame (safe mode, b32_fb_clear) whose clear has ALREADY been executed -- something flushed it without settling:
    // b32_synchronize -- must not be redrawn: its pixels would land on top of that clear.  It is retired instead: its counters and
    // errors are read, the capacities it asked for are granted to the frames that follow, nothing is enqueued.
    const bool no_redraw = c->frame_pending && c->pending_superseded && !later_clear;
    if (!later_clear) { const int rcf = flush_clear(c); if (rcf) return rcf; }
    if (!c->frame_pending) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const int d = c->deferred_rc; c->deferred_rc = 0;
        if (out && c->settled_valid && !d) *out = c->settled_tm;      // the most recent frame was settled early (settle_pending): its counters
        c->settled_valid = false;
        return d;
    }
    c->settled_valid = false;                                        // (a later frame is pending: the counters are its own)
    for (int attempt = 0; attempt < 5; ++attempt) {
        // the frame's counters come back through the pinned arena (one small kernel writing host memory) rather than an SDMA copy:
        // ~5 us of stream time less per synchronous frame
        if (stage_ensure(c)) {
            launch_ctrl_out(c->stream, c->cur.d_ctrl, static_cast<unsigned char*>(c->stage_dev) + STAGE_CTRL_OFF);
            HIPCHK(c, hipStreamSynchronize(c->stream));
            std::memcpy(&c->h_ctrl, c->stage_host + STAGE_CTRL_OFF, sizeof(Ctrl));
            std::memcpy(&c->h_stamps, c->stage_host + STAGE_CTRL_OFF + sizeof(Ctrl), sizeof(Stamps));
        } else {
            unsigned char tmp[sizeof(Ctrl) + sizeof(Stamps)];
            HIPCHK(c, hipMemcpyAsync(tmp, c->cur.d_ctrl, sizeof(tmp), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            std::memcpy(&c->h_ctrl, tmp, sizeof(Ctrl)); std::memcpy(&c->h_stamps, tmp + sizeof(Ctrl), sizeof(Stamps));
            c->h_stamps.t[ST_END] = 0;
        }
        if ((c->h_ctrl.need_global_sort & 2u) && c->last_direct) {
            // direct binning: a tile region was too small and nothing was drawn; redraw this frame with regions a quarter above the
            // longest list it reported (enqueue_frame falls back to the compact counting sort if those would not fit)
            c->scene.direct_cap_opaque = c->h_ctrl.list_demand + c->h_ctrl.list_demand / 4 + 64;
            if (no_redraw) break;
            const int rc = redraw_pending(c, 4);
            if (rc) return rc;
            continue;
        }
        if ((c->h_ctrl.need_global_sort & 1u) && c->scene.local_sort_ok) {
            // a tile list was longer than the LDS sort handles: nothing was drawn; redraw this frame (and the following ones of
            // this scene) with the global depth sort
            c->scene.local_sort_ok = false;
            if (no_redraw) break;
            const int rc = redraw_pending(c, 5);
            if (rc) return rc;
            continue;
        }
        if (!c->h_ctrl.pairs_overflow) break;
        // the fill aborted before touching the framebuffer: grow the pair buffers and redraw the same frame
        const size_t n = (size_t)c->h_ctrl.pairs_overflow + c->h_ctrl.pairs_overflow / 4 + 1024;
        int rc;
        for (int i = 0; i < 2; ++i) { if ((rc = ensure_plain(c, c->pkeys[i], n))) return rc; if ((rc = ensure_plain(c, c->pvals[i], n))) return rc; }
        c->cap_pairs = n;
        if (no_redraw) break;
        if ((rc = redraw_pending(c, 6))) return rc;
    }
    c->frame_pending = false;
    c->pending_superseded = false;
    c->cur.in_flight = false;
    collect_events(c);
    uint32_t sticky = c->h_ctrl.sticky;                        // errors of every frame enqueued since the last finish
    if (sticky) HIPCHK(c, hipMemsetAsync(&c->cur.d_ctrl->sticky, 0, sizeof(uint32_t), c->stream));
    if (sticky) c->side_dirty = true;                           // (the next setup kernel on the side stream reads that word: after the memset)
    for (FrameSet& o : c->alt) if (o.in_flight && o.d_ctrl) {
        // several frames in flight: the frames of the other sets since the last finish -- their sticky errors, and each set's last frame,
        // which no later k_setup of that set has looked at: dropped (it ran out of list space and drew nothing) means lost
        Ctrl other;
        HIPCHK(c, hipMemcpy(&other, o.d_ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost));      // (the main stream has drained)
        o.in_flight = false;
        uint32_t st2 = other.sticky;
        if (other.pairs_overflow || other.need_global_sort) st2 += 0x100u;
        if (other.sticky) HIPCHK(c, hipMemsetAsync(&o.d_ctrl->sticky, 0, sizeof(uint32_t), c->stream));
        if (other.pairs_overflow || other.need_global_sort) {      // (not again at the next finish)
            HIPCHK(c, hipMemsetAsync(&o.d_ctrl->pairs_overflow, 0, sizeof(uint32_t), c->stream));
            HIPCHK(c, hipMemsetAsync(&o.d_ctrl->need_global_sort, 0, sizeof(uint32_t), c->stream));
        }
        if (other.sticky || other.pairs_overflow || other.need_global_sort) c->side_dirty = true;
        sticky = (sticky | (st2 & 0xFFu)) + (st2 & ~0xFFu);
    }
    if (c->deferred_rc) { const int d = c->deferred_rc; c->deferred_rc = 0; return d; }     // (an earlier mesh of this frame, settled by a swap)
    if (c->h_ctrl.pairs_overflow && !no_redraw) return B32_E_HIP;
    // deep asynchronous mode: an earlier frame was lost (the last one is good).  (Safe mode only ever leaves a frame behind when a clear of
    // the whole band has overwritten whatever it drew: nothing observable was lost.)
    // (a framebuffer that is read behind the library's back -- caller-bound or shared with other ranks -- is never superseded; should a
    // dropped frame be counted there all the same, it is reported)
    if ((sticky >> 8) && (c->deep_async || c->fb_external || c->band_sync)) return B32_E_FRAME_DROPPED;
    if (c->h_ctrl.err_index || (sticky & 1u)) return B32_E_INDEX;
    if (c->h_ctrl.abort || (sticky & 2u)) return B32_E_NAN_KEY;
    if (sticky & 8u) {                                         // (k_join gave up on a setup kernel: internal.  Whatever that kernel left in the tile
        // counters of its frame set -- it may have finished late, or not at all -- is cleared once both streams have drained, so that the
        // frames that follow bin into empty lists again)
        if (c->side) HIPCHK(c, hipStreamSynchronize(c->side));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->cur.tile_fill) HIPCHK(c, hipMemsetAsync(c->cur.tile_fill, 0, c->cur.cap_tile_fill * sizeof(uint32_t), c->stream));
        for (FrameSet& o : c->alt) if (o.tile_fill) HIPCHK(c, hipMemsetAsync(o.tile_fill, 0, o.cap_tile_fill * sizeof(uint32_t), c->stream));
        c->side_dirty = true;
        return B32_E_HIP;
    }
    if (sticky & 16u) return B32_E_BAND_TIMEOUT;               // (b32_band_wait / _wait_all / _acquire gave up on another rank's epoch word)
    if (c->h_ctrl.wire_overflow || (sticky & 4u)) return B32_E_UNSUPPORTED;     // an edge >= 2^30 px long: i32 overflow in the reference's Bresenham
    if (out) {
        out->triangles_drawn = c->h_ctrl.n_visible;
        out->fragments = c->last_exact ? c->h_ctrl.fragments : 0;     // exact only with fragment counting on, painter's mode
        out->tile_pairs = c->h_ctrl.n_pairs;
        // RasterTimings phases of the most recent frame from the device-side phase clock (10 ns ticks): the reference's TRANSFORM, FOG and
        // CULL / SETUP stages are ONE fused kernel here (reported as cull_ms, transform_ms = fog_ms = 0), its sort is the tile binning,
        // its draw loop the fill kernels, its wireframe phase the line kernels.  With b32_set_profiling(2) the HIP-event averages over
        // the finished batch of frames take their place.
        const unsigned long long* t = c->h_stamps.t;
        const unsigned long long t_end = t[ST_END] ? t[ST_END] : 0ull;
        if (c->scene.nf && t[ST_SETUP] && t[ST_FILL] >= t[ST_SETUP]) {
            const unsigned long long t_bin = t[ST_BIN] ? t[ST_BIN] : t[ST_FILL];
            const unsigned long long t_fill_end = t[ST_WIRE] ? t[ST_WIRE] : t_end;
            out->cull_ms = (float)(t_bin - t[ST_SETUP]) * 1e-5f;
            out->sort_ms = (float)(t[ST_FILL] - t_bin) * 1e-5f;
            if (t_fill_end >= t[ST_FILL]) out->draw_ms = (float)(t_fill_end - t[ST_FILL]) * 1e-5f;
            if (t[ST_WIRE] && t_end >= t[ST_WIRE]) out->wireframe_ms = (float)(t_end - t[ST_WIRE]) * 1e-5f;
        }
        if (c->phase_frames && c->phase_level >= 2) {
            out->cull_ms = c->phase_ms[0];
            out->sort_ms = c->phase_ms[1];
            out->draw_ms = c->phase_ms[2] + c->phase_ms[3] + c->phase_ms[4];
        }
    }
    return B32_OK;
}

}  // extern "C"
