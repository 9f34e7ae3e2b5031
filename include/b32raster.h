/*
 * b32raster.h — C ABI of the MI355X-native bonnie-32 rasterizer hot path.
 *
 * This is the drop-in boundary for the reference's `render_mesh_15`
 * (reference: src/rasterizer/render.rs:2302-2310, re-exported at
 * src/rasterizer/mod.rs:63) and the `Framebuffer` it draws into
 * (render.rs:10-45).  The reference has no FFI seam today; these entry points
 * are exactly what a Rust `extern "C"` block for that path would bind (see
 * INTEGRATION.md for the Rust-side stub).
 *
 * Plain pointers and sizes only; no torch / HIP types in any signature
 * (streams and device pointers travel as `void*`).
 *
 * The same POD structs are consumed by the CPU oracle (oracle/b32_oracle.c),
 * which is test infrastructure and never linked into the product library.
 */
#ifndef B32RASTER_H
#define B32RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (reference behaviour in brackets) ---------------------- */
#define B32_OK             0
#define B32_E_ARG         -1  /* null pointer / zero-size framebuffer                      */
#define B32_E_INDEX       -2  /* face.v* >= nv            [index panic, render.rs:2375-2377] */
#define B32_E_NAN_KEY     -3  /* NaN painter's key        [unwrap panic, render.rs:2531]     */
#define B32_E_HIP         -4  /* HIP runtime failure (b32_last_hip_error has the code)      */
#define B32_E_UNSUPPORTED -5  /* a wireframe edge whose Bresenham state overflows i32 in the reference: every extent >= 2^30 px, and below that
                                  every edge with 3 * dmaj - 2 * dmin - r_min >= 2^31 (dmaj >= dmin its extents; r_min = gcd(dmaj, dmin) if
                                  dmaj / gcd is odd, else 0; a y-major edge has one value more of room) -- a shallow edge from 2^31 / 3 =
                                  715 827 883 px on; Framebuffer lines and primitives: >= 2^30; more than 65534 textures */
#define B32_E_NO_DEVICE   -6  /* no gfx950 device / kernels missing: the product path never falls back to CPU   */
#define B32_E_FRAME_DROPPED -7 /* deep asynchronous mode only (b32_set_async_depth): an EARLIER frame in flight ran out of buffer
                                  space and drew nothing (its framebuffer kept the cleared / previous contents); the most recent
                                  frame has been redrawn correctly */
#define B32_E_BAND_TIMEOUT -8  /* multi-GPU band exchange: a b32_band_wait / _wait_all / _acquire since the last b32_frame_finish gave up
                                  on another rank's epoch word (the frame may hold that rank's rows of an older frame) */

/* ---- enums mirrored as integers ------------------------------------------ */
/* BlendMode, types.rs:1380-1388 */
#define B32_BLEND_OPAQUE      0
#define B32_BLEND_AVERAGE     1
#define B32_BLEND_ADD         2
#define B32_BLEND_SUBTRACT    3
#define B32_BLEND_ADD_QUARTER 4
#define B32_BLEND_ERASE       5
/* ShadingMode, types.rs:1289-1294 */
#define B32_SHADE_NONE    0
#define B32_SHADE_FLAT    1
#define B32_SHADE_GOURAUD 2
/* LightType, types.rs:1297-1304 */
#define B32_LIGHT_DIRECTIONAL 0
#define B32_LIGHT_POINT       1
#define B32_LIGHT_SPOT        2   /* render.rs:1038-1058; f32::acos as the `libm` crate (musl acosf.c) computes it -- the reference's wasm32 target */

#define B32_NO_TEXTURE 0xFFFFFFFFu

/* ---- POD mirrors of the reference API types ------------------------------ */

/* Vertex, types.rs:947-959.  36 B.  (bone_index is editor-only and not part of the record: b32_scene_set_rig takes it as an array of its own.) */
typedef struct B32Vertex {
    float   pos[3];
    float   uv[2];
    float   normal[3];
    uint8_t r, g, b, blend;      /* Color{r,g,b,blend}, types.rs:721-726 */
} B32Vertex;

/* Face, types.rs:984-1002. 20 B. texture_id: Option<usize> -> B32_NO_TEXTURE = None. */
typedef struct B32Face {
    uint32_t v[3];
    uint32_t texture_id;
    uint8_t  black_transparent;
    uint8_t  blend_mode;
    uint8_t  editor_alpha;
    uint8_t  _pad;
} B32Face;

/* Texture15, types.rs:532-539. `pixels` is a HOST pointer to width*height Color15 (u16). */
typedef struct B32Texture15 {
    uint32_t        width, height;
    uint32_t        blend_mode;
    uint32_t        _pad;
    const uint16_t* pixels;
} B32Texture15;

/* Texture, types.rs:1166-1176 (the 8-bit-colour path): `pixels` is a HOST pointer to width*height Color values, 4 bytes
 * each = r, g, b, blend (Color{r,g,b,blend: BlendMode}, types.rs:721-726; blend == B32_BLEND_ERASE is a transparent texel). */
typedef struct B32Texture {
    uint32_t       width, height;
    uint32_t       blend_mode;
    uint32_t       _pad;
    const uint8_t* pixels;
} B32Texture;

/* IndexedAtlas + Clut (modeler/mesh_editor.rs:594-682, types.rs:390-397): one byte per texel for
 * both 4- and 8-bit depths; out-of-range index -> 0x0000.  Expanded with Clut::lookup semantics
 * exactly as IndexedAtlas::to_texture15 does before the rasterizer sees it (scene.rs:164). */
typedef struct B32IndexedTexture {
    uint32_t        width, height;
    uint32_t        blend_mode;
    uint32_t        clut_len;     /* 16 or 256 */
    const uint8_t*  indices;      /* HOST pointer, width*height */
    const uint16_t* clut;         /* HOST pointer, clut_len Color15 */
} B32IndexedTexture;

/* Camera, camera.rs:9-18: basis vectors are inputs (sin/cos stay on the host). */
typedef struct B32Camera {
    float position[3];
    float basis_x[3];
    float basis_y[3];
    float basis_z[3];
} B32Camera;

/* Light, types.rs:1306-1314 */
typedef struct B32Light {
    uint32_t type;
    float    position[3];
    float    direction[3];
    float    radius;
    float    angle;
    float    intensity;
    uint8_t  r, g, b, enabled;
} B32Light;

/* RasterSettings, types.rs:1392-1428 (low_resolution / stretch_to_fill are presentation-only). */
typedef struct B32Settings {
    uint8_t affine_textures;
    uint8_t use_zbuffer;
    uint8_t shading;
    uint8_t backface_cull;
    uint8_t backface_wireframe;
    uint8_t dithering;
    uint8_t wireframe_overlay;
    uint8_t use_rgb555;
    uint8_t use_fixed_point;
    uint8_t xray_mode;
    uint8_t has_ortho;           /* ortho_projection.is_some() */
    uint8_t _pad;
    float   ambient;
    float   ortho_zoom, ortho_center_x, ortho_center_y;
    uint32_t        n_lights;
    const B32Light* lights;      /* HOST pointer */
} B32Settings;

/* fog: Option<(f32,f32,f32,Color)> of render_mesh_15 (render.rs:2309); NULL pointer = None. */
typedef struct B32Fog {
    float   start, falloff, cull_distance;
    uint8_t r, g, b, blend;
} B32Fog;

/* RasterTimings, types.rs:1499-1514, plus the exact fragment-store count used for Mpixels/s. */
typedef struct B32Timings {
    float    transform_ms, fog_ms, cull_ms, sort_ms, draw_ms, wireframe_ms;
    uint32_t triangles_drawn;    /* opaque.len()+transparent.len(), render.rs:2545 */
    uint32_t tile_pairs;         /* (surface, 64x64 tile) pairs binned this frame (work unit of the coverage kernel) */
    uint64_t fragments;          /* pixel stores reached in rasterize_triangle_15 (render.rs:1671-1702) */
} B32Timings;

typedef struct b32_ctx b32_ctx;

/* ---- context -------------------------------------------------------------- */
/* One ctx = one device = one caller thread at a time.  Fails with B32_E_NO_DEVICE when no HIP
 * device is visible; there is no CPU fallback. */
int         b32_create(int device, b32_ctx** out);
void        b32_destroy(b32_ctx* ctx);
const char* b32_strerror(int code);
int         b32_last_hip_error(const b32_ctx* ctx);
/* Digest (16 hex digits) of the sources and compiler flags this library was built from (bonnie-32_amd/build.py: csrc_digest; no
 * reference counterpart).  bench.py and __graft_entry__.smoke() refuse to run a library whose digest is not the source tree's. */
const char* b32_build_digest(void);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream); NULL = the ctx's own non-blocking stream.  The legacy default
 * stream is not NULL here: pass hipStreamLegacy ((hipStream_t)1) for it (torch reports its default stream as handle 0). */
int         b32_set_stream(b32_ctx* ctx, void* hip_stream);
int         b32_synchronize(b32_ctx* ctx);

/* ---- Framebuffer (render.rs:10-45) --------------------------------------- */
int b32_fb_resize(b32_ctx* ctx, uint32_t width, uint32_t height);           /* Framebuffer::resize :27-34: zero-filled on change, no-op on equal dimensions */
int b32_fb_new(b32_ctx* ctx, uint32_t width, uint32_t height);              /* Framebuffer::new :18-25: ALWAYS zero pixels and an f32::MAX z-buffer */
/* Framebuffer::clear :36-45 (rows of the band only when b32_set_band is active).  The clear is deferred inside the library: the draw
 * that follows folds it into its fused kernel when it can (painter's mode, no depth buffer allocated, same band) -- the frame then has
 * no clear launch and pixels nobody draws are written once -- and every other call that reads or writes the framebuffer, changes the
 * band, the binding or the stream, b32_synchronize and b32_frame_finish first turn it into the launches it stands for.  Through this
 * API the deferral is unobservable; code that reads a caller-bound device buffer (b32_fb_bind_device) DIRECTLY sees the clear after
 * the next draw, b32_synchronize or b32_frame_finish, in stream order. */
int b32_fb_clear(b32_ctx* ctx, uint8_t r, uint8_t g, uint8_t b, uint8_t blend);
int b32_fb_upload(b32_ctx* ctx, const uint8_t* rgba);                        /* host fb.pixels -> device */
int b32_fb_download(b32_ctx* ctx, uint8_t* rgba);                            /* device -> host fb.pixels */
/* The presenter's copy WITHOUT a host round trip per frame.  The reference hands fb.pixels to the screen every frame
 * (game/renderer.rs:179-214); b32_fb_download blocks the host until the frame is there.  b32_fb_download_async only ENQUEUES the copy --
 * behind everything enqueued on the context so far (a deferred clear is flushed; in safe mode a pending frame that may still need a
 * redraw is settled first, which frames of small meshes never do) -- into page-locked memory of the caller, and hands out a ticket:
 *     frame i:   b32_fb_clear; b32_frame_submit(...) or the draws; b32_fb_download_async(ctx, pinned[i & 1], &ticket[i & 1]);
 *                b32_ticket_wait(ctx, ticket[(i - 1) & 1]);   present pinned[(i - 1) & 1]      (frame i is being drawn meanwhile)
 * b32_ticket_poll never blocks (*done = 0 / 1); b32_ticket_wait blocks until the copy has landed.  At most 8 tickets are outstanding per
 * context: a ninth download first waits for the oldest.  `rgba` must stay valid until its ticket is done; memory from b32_host_alloc
 * (page-locked; NULL when it cannot be had) keeps the copy asynchronous, pageable memory works but may block the call.
 * Errors of the frames are reported by b32_frame_finish as ever. */
void* b32_host_alloc(size_t bytes);
void b32_host_free(void* p);
int b32_fb_download_async(b32_ctx* ctx, uint8_t* rgba, uint64_t* ticket);
int b32_ticket_poll(b32_ctx* ctx, uint64_t ticket, int* done);
int b32_ticket_wait(b32_ctx* ctx, uint64_t ticket);
/* Framebuffer::zbuffer (render.rs:12), used when settings.use_zbuffer: f32 per pixel, f32::MAX after new/resize/clear. */
int b32_zbuffer_download(b32_ctx* ctx, float* z);
int b32_zbuffer_upload(b32_ctx* ctx, const float* z);
/* Draw into caller-owned DEVICE memory (width*height*4 B, e.g. a torch uint8 tensor) instead of the
 * ctx-owned buffer; pass NULL to return to the ctx-owned buffer. */
int b32_fb_bind_device(b32_ctx* ctx, void* device_rgba, uint32_t width, uint32_t height);
int b32_fb_size(const b32_ctx* ctx, uint32_t* width, uint32_t* height);
/* Multi-GPU screen-band sharding: only rows [y0,y1) are filled by this ctx (default = whole frame). */
int b32_set_band(b32_ctx* ctx, uint32_t y0, uint32_t y1);

/* ---- render_mesh_15 (render.rs:2302-2638) -------------------------------- */
/* Drop-in form: host slices in, framebuffer stays device resident (read-modify-write).
 * Texture cache: the texel pool of the previous call is reused when every texture has the same host pointer, dimensions, blend mode and
 * 64-bit content hash (the texels are re-hashed on every call, so an in-place edit is seen); an edit that collides in the hash (2^-64
 * per edit, non-cryptographic) would draw stale texels -- b32_set_routes(B32_ROUTE_TEX_CACHE) uploads the texels on every call. */
int b32_render_mesh_15(b32_ctx* ctx,
                       const B32Vertex* vertices, uint32_t nv,
                       const B32Face* faces, uint32_t nf,
                       const B32Texture15* textures, uint32_t nt,
                       const B32Camera* camera, const B32Settings* settings,
                       const B32Fog* fog /* nullable */,
                       B32Timings* out /* nullable */);

/* Resident form (scene.rs:112-261 step-before): upload a mesh once, draw it many times. */
int b32_scene_upload(b32_ctx* ctx,
                     const B32Vertex* vertices, uint32_t nv,
                     const B32Face* faces, uint32_t nf,
                     const B32Texture15* textures, uint32_t nt);
/* Same, textures given as index atlas + CLUT; the expansion (Clut::lookup) runs on the device. */
int b32_scene_upload_indexed(b32_ctx* ctx,
                             const B32Vertex* vertices, uint32_t nv,
                             const B32Face* faces, uint32_t nf,
                             const B32IndexedTexture* textures, uint32_t nt);
int b32_render_scene_15(b32_ctx* ctx,
                        const B32Camera* camera, const B32Settings* settings,
                        const B32Fog* fog /* nullable */,
                        B32Timings* out /* nullable */);
/* Asynchronous draw of the resident scene: enqueue only, no host sync, no timings. Errors and counters
 * of the most recent frame are collected by b32_frame_finish (which synchronizes the stream). */
int b32_render_scene_15_async(b32_ctx* ctx,
                              const B32Camera* camera, const B32Settings* settings,
                              const B32Fog* fog /* nullable */);
int b32_frame_finish(b32_ctx* ctx, B32Timings* out /* nullable */);
/* How many frames of a LARGE scene (more than 8192 faces, or more than 2048 with a transparent pass) may be in flight.  Such a
 * frame can run out of tile-list space (the setup kernel bins it into fixed tile regions sized from the mesh; a region overflows when
 * far more of the mesh lands in one screen tile than the mean) or need the global depth sort; it then draws nothing and must be
 * redrawn by the host.
 *   deep = 0 (default): safe.  Enqueueing another frame, or any call that reads, writes or rebinds the framebuffer (b32_fb_download,
 *            b32_zbuffer_download, b32_fb_upload, b32_fb_clear*, b32_render_skybox_mesh, b32_draw_star_diamonds, b32_draw_lines,
 *            b32_draw_prims, b32_render_sky, b32_draw_stars, b32_fb_bind_device,
 *            b32_set_stream, b32_present_nearest, b32_scene_upload*, b32_scene_swap, b32_set_band), first settles the pending frame (one host synchronisation, redraw if needed): no
 *            frame is ever lost, and none is redrawn on top of a later clear.  One exception that cannot be observed (round 5): a
 *            b32_fb_clear of the whole band behind a pending frame overwrites every pixel and depth that frame can have drawn, so the
 *            frame is marked superseded instead of settled and the draw that follows is enqueued behind it like in deep mode -- the
 *            reference's loop (clear, draw, clear, draw; game/renderer.rs:91-95) runs without a host synchronisation per frame in
 *            this default mode too.  Any call that READS the framebuffer in between still settles; errors of a superseded frame are
 *            still reported by the next b32_frame_finish.  The exception applies only to a framebuffer nobody can read behind the
 *            library's back: the library's own allocation (b32_fb_new / _resize), not exported to other ranks.  With caller-bound memory
 *            (b32_fb_bind_device) or a framebuffer shared by b32_band_export / _import / _attach the clear settles the pending frame as
 *            every other write does.  A superseded frame whose clear has meanwhile been executed (b32_synchronize) is never redrawn.
 *   deep = 1: throughput.  Frames are enqueued back to back with no host synchronisation (bench.py and the tools that call
 *            b32_set_async_depth(ctx, 1): static camera, capacities settled by a warm-up frame).  Only the most recent frame can be redrawn; if an earlier one was dropped,
 *            b32_frame_finish reports B32_E_FRAME_DROPPED -- never silently.  Consumers outside the library that read the bound
 *            framebuffer between two frames (an RCCL gather on the same stream) must accept that contract.  A b32_fb_clear issued
 *            after a draw is applied after that draw even when b32_frame_finish has to redraw it.
 * Frames of small meshes never overflow and are always enqueued without synchronisation. */
int b32_set_async_depth(b32_ctx* ctx, int deep);
/* Which internal route the frames of this context took since it was created (tests assert that the route they target really ran;
 * no reference counterpart).  which: 0 frames binned by the setup kernel into fixed tile regions (large meshes), 1 frames whose tile
 * lists were collected inside the fill kernel (small meshes), 2 frames binned by the counting-sort launches, 3 frames through the
 * keyed pipeline (global depth sort), 4 frames redrawn because a tile region overflowed, 5 frames redrawn through the global depth
 * sort, 6 frames redrawn after a pair-buffer overflow, 7 frames whose setup kernel ran on the second stream beside the previous frame's
 * fill (two frames in flight), 8 frames whose fused kernel sampled the 4/8-bit index atlas + CLUT from LDS (B32_ROUTE_LDS_ATLAS),
 * 9 frames whose wireframe phases went through the tile route (B32_ROUTE_WIRE_TILES), 10 frames whose opaque coverage was decided by
 * exact row intervals (B32_ROUTE_SPAN_COVER), 11 pipelined frames whose setup kernel was handed over to the fill by the flag / join kernel
 * pair, 12 by a cross-stream event (main and side stream of one priority), 13 those of 11 whose fused kernel polled the flag itself (the merged
 * draws of a batched frame: no launch and no event in front of the fill), 14 b32_draw_lines batches binned to tiles (B32_ROUTE_LINE_TILES),
 * 15 b32_draw_lines batches in which every tile scanned the whole batch in order (small batches, or the route switched off), 16 b32_draw_prims
 * batches binned to tiles (B32_ROUTE_PRIM_TILES), 17 b32_draw_prims batches in which every tile scanned the whole batch in order
 * (b32_draw_world batches count under 16 / 17 too: they are primitive batches), 18 b32_draw_world batches binned to tiles, 19 b32_draw_world
 * batches in which every tile scanned the whole batch, 20 reductions of a slot's bounds launched by b32_draw_object_overlays, its stage tap
 * and b32_scene_bounds (one per slot whose vertices changed since its last one).
 * Unknown `which` or null ctx: 0. */
unsigned long long b32_route_count(const b32_ctx* ctx, int which);
/* Switch internal routes OFF for the frames enqueued from now on (no reference counterpart: the results are identical on every route;
 * the tests use it to keep the older pipelines covered, the timing tools to compare routes).  off_mask = 0 restores the default. */
#define B32_ROUTE_SORT_FREE   1u   /* the fused sort-free kernel -> keyed pipelines (global painter's sort / per-tile LDS sort)    */
#define B32_ROUTE_CUT_TILES   2u   /* tiles of 32 / 16 rows when a frame has few 64x64 tiles                                      */
#define B32_ROUTE_INLINE_BIN  4u   /* small meshes: tile lists collected inside the fill kernel -> binning launches                */
#define B32_ROUTE_DIRECT_BIN  8u   /* large meshes: binning inside the setup kernel -> counting-sort launches                      */
#define B32_ROUTE_WIDE_GROUPS 16u  /* 16-wave workgroups of the fused kernel when tiles are few -> always 8 waves                  */
#define B32_ROUTE_PACKED_STREAMS 32u /* resident large meshes: packed position / attribute streams for the setup kernel -> B32Vertex array */
#define B32_ROUTE_TEX_CACHE   128u /* drop-in calls: texture cache by (pointer, size, blend mode, 64-bit content hash) -> texels uploaded on every call */
#define B32_ROUTE_BATCH       256u /* b32_frame_end: runs of commuting meshes drawn as one merged mesh -> one draw per mesh           */
#define B32_ROUTE_LDS_ATLAS   512u /* one indexed texture (b32_scene_upload_indexed): index atlas + CLUT staged in LDS by every workgroup of the fused
                                    * kernel and looked up per shaded pixel (Clut::lookup, types.rs:390-397) whenever they fit beside the tile planes
                                    * -> expanded Color15 texels fetched from global memory                                          */
#define B32_ROUTE_WIRE_TILES  1024u /* wireframe phases (render.rs:2574-2635): edges binned to 64x16 tiles, first occurrences found in an LDS table per tile,
                                    * lines walked into an LDS bit plane -> one global first-occurrence table + one lane per whole line        */
#define B32_ROUTE_SPAN_COVER  2048u /* sort-free CHEAP painter's coverage: for surfaces with integer vertices, |area| <= 8192 and edges <= 512 px the reference's
                                    * toleranced inside test (render.rs:1536-1542) equals the closed integer triangle, so every row's passing pixels are one
                                    * interval with integer-quotient ends -- no per-pixel test; other surfaces keep the per-pixel form -> per-pixel form for all */
#define B32_ROUTE_STAGGER     4096u /* fused kernel, frames with more tiles than workgroup slots: the second workgroup of every CU starts 4 us late (the two then
                                    * run coverage against shading instead of in step) -> all workgroups start together */
#define B32_ROUTE_LINE_TILES  8192u /* b32_draw_lines, batches of more than 64 lines: line ids binned to 64x16 tiles, each tile's list put in order in LDS
                                    * (a tile whose list overflows scans the whole batch) -> every tile scans the whole batch in order */
#define B32_ROUTE_PRIM_TILES 16384u /* b32_draw_prims, batches of more than 48 primitives: the same tile route as B32_ROUTE_LINE_TILES, binned by a conservative
                                    * box per kind -> every tile scans the whole batch in order */
#define B32_ROUTE_PIPELINE    64u  /* setup kernel of the next frame on a second stream beside the fill of the current one -> one stream */
int b32_set_routes(b32_ctx* ctx, uint32_t off_mask);
/* CHEAP coverage (inside test only, texel rule applied to the winner) is used while every texture has at most 1/den skippable texels
 * (default 64); applies to textures uploaded after the call.  den = 0: B32_E_ARG. */
int b32_set_cheap_threshold(b32_ctx* ctx, uint32_t den);

/* Several resident scenes per context (scene.rs:112-261 draws room after room, asset part after asset part, onto one
 * framebuffer every frame): a slot owns one uploaded scene's device buffers.  b32_scene_swap exchanges the context's current
 * resident scene with the slot's content (either side may be empty), so
 *     upload A; swap(sA);  upload B; swap(sB);                                 -- once
 *     clear;  swap(sA); render_async; swap(sA);  swap(sB); render_async; swap(sB);  frame_finish      -- every frame
 * draws both meshes with no upload and no host synchronisation between them.  Errors of ANY frame enqueued since the last
 * b32_frame_finish are reported by it (B32_E_INDEX / B32_E_NAN_KEY / B32_E_UNSUPPORTED; as in the reference, the failing mesh
 * draws nothing); its counters are those of the most recent frame.  A pending frame of a large scene (more than 8192 faces, or
 * more than 2048 with a transparent pass: it may need a redraw with grown buffers) is finished by b32_scene_swap before the exchange; an error of that frame is kept and
 * reported by the b32_frame_finish that ends the frame, and when no later frame is pending then, its counters are that frame's too. */
typedef struct b32_scene b32_scene;
int b32_scene_create(b32_ctx* ctx, b32_scene** out);
void b32_scene_destroy(b32_ctx* ctx, b32_scene* slot);
int b32_scene_swap(b32_ctx* ctx, b32_scene* slot);

/* ---- bones: a rigged resident mesh posed on the device from a per-frame bone table ------------------------------------------------
 * The modeler skins per vertex on the host, four times per frame -- the draw (modeler/viewport.rs:1196-1240), the box selection
 * (:1677-1694), the selection brackets (:1796-1810) and the hover (:2401-2421) -- always with
 *     posed = rotate_by_euler(v.pos, bone_rot) + bone_pos          (modeler/state.rs:30-54)
 * where (bone_pos, bone_rot) = get_bone_world_transform(v.bone_index.or(obj.default_bone_index)) (state.rs:2585-2614).  Here the mesh stays
 * resident and is posed ONCE per change of the bone table, into the slot's own vertices: the draw, the wireframe, b32_hover_mesh,
 * b32_box_select and b32_pick_meshes then read posed vertices like any others, and none of their kernels skins.
 *
 * B32Bone is get_bone_world_transform(i) with libm kept on the host (like the camera basis and B32Placement): cos / sin of
 * bone_rot.x.to_radians() and bone_rot.z.to_radians(), and `rotate` = 0 where rotate_by_euler takes its early return
 * (|rot.x| < 0.001 && |rot.z| < 0.001, in degrees) -- the reference then returns v as it is, it does not multiply by cos(0).
 *
 * b32_scene_set_rig   makes the scene of `slot` (NULL: the context's resident scene) a rigged one.  It copies the scene's CURRENT positions
 *     and normals, on the device, into a rest stream (24 B per vertex) and uploads bone_of_vertex (nv entries; the caller has resolved
 *     v.bone_index.or(obj.default_bone_index); B32_BONE_NONE = no bone).  Mirror editing's twins (viewport.rs:1250-1266: mirrored in local space
 *     before the bone) are built from this rig into a derived slot by b32_scene_build_mirror, below.  The rig is part of the scene's
 *     content: it travels with b32_scene_swap, and any b32_scene_upload* into that scene drops it.  A second call replaces the indices and
 *     takes a NEW rest snapshot of whatever the vertices are at that moment -- after a pose, the posed ones (pose with n_bones = 0 first to
 *     get the uploaded vertices back).  The caller may reuse bone_of_vertex when the call returns.
 * b32_scene_pose      enqueues one kernel on the context's stream, one lane per vertex, always from the rest stream (poses never
 *     accumulate).  With b = bone_of_vertex[i]:
 *       b >= n_bones (B32_BONE_NONE included; bone_transforms.get(idx) == None): position and normal are the rest bits;
 *       bones[b].rotate == 0: pos = rest_pos + bone_pos component-wise (a -0.0 becomes +0.0), the normal is the rest bits;
 *       otherwise, for v = position and, without the translation, for the normal:
 *           y1 = v.y*cos_x + v.z*sin_x      z1 = (-v.y)*sin_x + v.z*cos_x
 *           x2 = v.x*cos_z + y1*sin_z       y2 = (-v.x)*sin_z + y1*cos_z
 *           pos = (x2 + bx, y2 + by, z1 + bz)        normal = (x2, y2, z1)   (not renormalised)
 *     every operation a separately rounded f32 operation in this order, no fused multiply-add.  uv and colour are untouched; n_bones == 0
 *     restores the rest vertices bit for bit.  The table is copied by the call (the caller may reuse it at once).  The call performs no
 *     host synchronisation for small meshes; like b32_scene_upload it first settles a pending frame of a large scene that may still be
 *     redrawn (from the vertices as they were).  It touches neither framebuffer nor z-buffer and flushes no deferred clear.  What the
 *     scene's frames taught the context (tile region sizes, sort route) stays, as for placements; the packed streams of a mesh with more
 *     than 8192 faces are packed again by the next frame.  The scene's content counts as changed: a cached merged run of
 *     b32_frame_add_scene that contains the slot is rebuilt by the next batched frame (one build with its host synchronisation per pose,
 *     b32_batch_count(ctx, 2) grows by one) -- a mesh that is posed every frame is better drawn on its own, as the modeler does.
 *   A B32Placement on top of a pose is pose first, placement second (in k_setup, k_pick, k_hover as before).  The reference has no such
 *   combination: the modeler has bones and no placements, the world editor placements and no bones.
 *   b32_hover_mesh on a rigged slot tests the mirror plane on the REST position (find_hovered_element tests the local position,
 *   viewport.rs:2482-2486, and projects the posed one); box selection and picking have no mirror test.
 * b32_scene_read_vertices   blocking: vertices first .. first + count of the scene as they are on the device now (posed, if posed).
 * Errors: NULL context, a slot (or context) without a scene, set_rig with NULL indices and nv > 0, pose without a rig or with NULL bones
 * and n_bones > 0, read_vertices with NULL out and count > 0 or first + count > nv -> B32_E_ARG; n_bones > B32_MAX_BONES ->
 * B32_E_UNSUPPORTED. */
typedef struct B32Bone {            /* 32 bytes: get_bone_world_transform(i) with libm kept on the host */
    float pos[3];                   /* bone_pos */
    float cos_x, sin_x, cos_z, sin_z;   /* of bone_rot.x / .z .to_radians(); read only when rotate != 0 */
    uint32_t rotate;                /* 0: rotate_by_euler's early return (|rot.x| < 0.001 && |rot.z| < 0.001, degrees) */
} B32Bone;
#define B32_BONE_NONE 0xFFFFu
#define B32_MAX_BONES 64u
int b32_scene_set_rig(b32_ctx* ctx, b32_scene* slot /* NULL: the context's resident scene */, const uint16_t* bone_of_vertex /* nv entries */);
int b32_scene_pose(b32_ctx* ctx, b32_scene* slot /* NULL: ditto */, const B32Bone* bones, uint32_t n_bones);
int b32_scene_read_vertices(b32_ctx* ctx, b32_scene* slot /* NULL: ditto */, uint32_t first, uint32_t count, B32Vertex* out);  /* blocking */

/* ---- the bone octahedra: a mesh tail built on the device from the bone table -------------------------------------------------------
 * The modeler draws ONE combined mesh per frame: every object's faces and, while bones are shown, the eight faces per bone of
 * skeleton_to_triangles (modeler/skeleton.rs:412-477, :565-660), appended before its single render_mesh_15 / render_mesh call
 * (modeler/viewport.rs:1196-1395).  Painter's order, the order of equal keys and the editor-alpha blend run over that one list, so a
 * skeleton drawn as a second mesh is another frame.  Here a slot's geometry is a BODY -- what an upload or b32_room_build_mesh left --
 * plus a TAIL: 6 vertices and 8 faces per drawn bone, in bone order, the creation preview last, written by one kernel from the table.
 *
 * B32SkelBone is what the reference reads per bone, libm kept on the host: pos = get_bone_world_transform(i).0; cos / sin of the WORLD
 * rotation's .x / .z .to_radians() (always read: get_bone_tip_position has no early return); length; width = display_width() as the
 * host resolved it (state.rs:369-375); parent: B32_BONE_NONE marks a root (only the colour depends on it here; b32_skeleton_items reads
 * the parent's position, (0, 0, 0) for an index >= n as get_bone_world_transform answers out of range).
 * B32SkeletonStyle is the editor state: selected_bone / hovered_bone / hovered_tip (negative: none), editor_alpha, mode 0 =
 * skeleton_to_triangles, mode 1 = skeleton_to_triangles_from_bones (root / default colours only, editor_alpha on every bone, no
 * preview); has_preview with preview_start / preview_end = bone_creation (colour `creating`, alpha 255, width DEFAULT_WIDTH = 40).
 *
 * Per bone, every operation a separately rounded f32 operation in the reference's order (csrc/b32_skeleton_body.h):
 *     tip = pos + Vec3(sin_z*cos_x, cos_z*cos_x, -sin_x).normalize() * length      (state.rs:2629-2638)
 *   Vec3::normalize (math.rs:39-49) is ZERO for len == 0.0, else three divisions by len = sqrt((x*x + y*y) + z*z).
 *   direction = tip - pos; length = direction.len(); length < 0.001 -> nothing (a NaN is not < and is drawn).
 *   dir_norm = direction * (1.0 / length); up = +Y while |dir_norm.y| < 0.9, else +X; perp1 = cross(dir_norm, up).normalize(),
 *   perp2 = cross(dir_norm, perp1).normalize(); ring_center = pos + dir_norm * (length * 0.2); ring = center + perp1*w, + perp2*w,
 *   - perp1*w, - perp2*w.  Vertices: base (normal dir_norm * -1.0), tip (dir_norm), the ring ((ring[i] - center).normalize()); uv (0, 0),
 *   the bone's colour.  Faces: (0, 2+i, 2+next) for i = 0..3, then (1, 2+next, 2+i); no texture, Opaque, black_transparent 0,
 *   editor_alpha = the bone's alpha.  Colour: selected > tip-hovered > hovered > root > default; while a bone is selected every other bone
 *   has alpha editor_alpha.min(30).  One departure from the reference's bits: a float that is a NaN is written as 0x7FC00000.
 *
 * b32_scene_build_skeleton   replaces the tail of `slot` (NULL: the context's resident scene).  The host copies the table, computes each
 *     tip and decides liveness there, once, with the text above; the drawn octahedra travel by value in the launch, in order, so the
 *     device never decides a second time where an octahedron lies.  One kernel on the context's stream: one workgroup of 64 lanes per
 *     drawn octahedron (at most 65 workgroups), of which 14 lanes work, one per output element (6 vertices, 8 faces), and 50 idle -- the
 *     octahedron's record is then read from the kernel argument by the workgroup's index, with scalar loads.  No upload and no host
 *     synchronisation unless the slot's buffers must grow (then the body is kept by a copy on the device and the stream is waited for
 *     once).  Face indices are absolute: the first tail vertex is the body's vertex count.
 *     n_bones == 0 without a preview removes the tail.  An empty body (nv == nf == 0) is legal: the model browser's skeleton mesh.
 *     Like b32_scene_pose it first settles a pending frame that may still be redrawn, and the scene's content counts as changed.
 *     Works for RGB555 and 8-bit-colour scenes; a tail face with alpha < 255 is a transparent-pass face like an uploaded one.
 *   The tail is DRAWN and never QUERIED.  Frames, merged runs of b32_frame_add_scene, placed draws, the wireframe phases and b32_last_*
 *   see body + tail; b32_scene_read_vertices / _read_faces read body + tail.  b32_scene_set_rig, b32_scene_pose, b32_hover_mesh,
 *   b32_box_select (its result size too), b32_pick_meshes and b32_draw_mesh_overlay / _project_batch see the BODY only: the reference
 *   skins, hovers, selects and overlays mesh objects, and skeleton vertices have bone_index None.  A pose after a build leaves the tail's
 *   bits alone and a build after a pose the body's.  Any b32_scene_upload* or b32_room_build_mesh into the slot drops the tail, as it
 *   drops the rig; b32_scene_swap carries it.
 * b32_skeleton_counts   host only: the tail's vertex and face counts for this table and style (6 and 8 per drawn octahedron).
 * b32_skeleton_items    host only, like b32_floor_grid_items: the calls of draw_skeleton (skeleton.rs:70-79: per bone with a parent one
 *     B32_LINE_2D item with B32_WORLD_CLIP_NEAR from the parent's position to the bone's, colour (100, 100, 100)) followed by those of
 *     draw_bone_dots (:110-143: per bone the tip circle, then the base circle; radius 11 / 8 / 5 and colour by tip-hovered / selected /
 *     neither, resp. hovered / selected / neither), for b32_draw_world.  The tip is the octahedron's tip vertex, bit for bit.  *n_out = the
 *     number of items; at most `cap` are written (out may be NULL).
 * Errors: NULL context or style, a slot (or context) without a scene, NULL bones with n_bones > 0, mode > 1 -> B32_E_ARG;
 * n_bones > B32_MAX_BONES -> B32_E_UNSUPPORTED. */
typedef struct B32SkelBone {        /* 40 bytes */
    float pos[3];                   /* get_bone_world_transform(i).0 */
    float cos_x, sin_x, cos_z, sin_z;   /* of the world rotation's .x / .z .to_radians() */
    float length;
    float width;                    /* display_width() */
    uint32_t parent;                /* B32_BONE_NONE: a root */
} B32SkelBone;
typedef struct B32SkeletonStyle {   /* 44 bytes */
    int32_t selected_bone, hovered_bone, hovered_tip;     /* negative: none */
    uint32_t mode;                  /* 0: skeleton_to_triangles; 1: skeleton_to_triangles_from_bones */
    uint8_t editor_alpha;
    uint8_t has_preview;            /* mode 0: bone_creation is Some */
    uint8_t _pad[2];
    float preview_start[3], preview_end[3];
} B32SkeletonStyle;
int b32_scene_build_skeleton(b32_ctx* ctx, b32_scene* slot /* NULL: the context's resident scene */, const B32SkelBone* bones, uint32_t n_bones,
                             const B32SkeletonStyle* style);
int b32_skeleton_counts(const B32SkelBone* bones, uint32_t n_bones, const B32SkeletonStyle* style, uint32_t* n_vertices, uint32_t* n_faces);
struct B32WorldItem;
int b32_skeleton_items(const B32SkelBone* bones, uint32_t n_bones, const B32SkeletonStyle* style, struct B32WorldItem* out, uint32_t cap,
                       uint32_t* n_out);

/* ---- editing a resident scene in place: vertices, faces, texels and palette -----------------------------------------------------------
 * The modeler changes its mesh every frame while the user drags: the move / rotate / scale tools write the selected vertices' positions
 * (modeler/viewport.rs:95, :373), the UV editor uv (modeler/layout.rs:3732-3902), the opacity slider editor_alpha of an object's faces
 * (viewport.rs:1295), the face panel blend_mode and black_transparent, paint mode atlas indices (modeler/mesh_editor.rs:647), the palette
 * panel one CLUT entry (texture/user_texture.rs:337).  These calls change a resident scene where it lies instead of uploading it again.
 *
 * The contract: after any sequence of patches the slot is indistinguishable -- every frame, query, read-back, error and counter -- from a
 * slot into which the patched arrays were uploaded afresh, followed by the same b32_scene_set_rig, b32_scene_pose with the slot's last
 * bone table and the same b32_scene_build_skeleton.  Two exceptions, both about speed and never a result: whether the scene's textures
 * count as having few skippable texels (decided by the upload, b32_set_cheap_threshold) keeps its value, and the tile-region sizes the
 * slot's frames have learnt stay.
 *
 * Common rules.  `index` values are strictly ascending within one call (a parallel scatter has no "last one wins") and below the BODY's
 * vertex / face count: the tail of bone octahedra is never patched and stays bit for bit.  A rectangle [x, x + w) x [y, y + h) lies inside
 * texture `tex`; the caller's rows are `stride` elements apart (stride >= w).  Anything else is B32_E_ARG, and a failed call changes
 * nothing.  n == 0, w == 0 or h == 0 is B32_OK and changes nothing.  The records travel through a pinned ring: the caller may reuse its
 * arrays when the call returns.  Every call enqueues one copy and one kernel on the context's stream and performs no host synchronisation
 * (the two documented exceptions below fetch a host copy ONCE per upload); like b32_scene_pose it first settles a pending frame that may
 * still be redrawn, and the scene's content counts as changed (a merged run of b32_frame_add_scene that holds the slot is rebuilt).
 *
 * b32_scene_patch_vertices   one lane per record writes the whole B32Vertex.  On a rigged slot the record is in REST (local) space, where
 *     the modeler edits: position and normal go into the rest stream, and the vertex gets them posed with the table of the slot's last
 *     b32_scene_pose (before the first pose, after a pose with n_bones = 0 and after b32_scene_set_rig: copied), by the pose pass's own
 *     arithmetic.  Later poses start from the patched rest vertex.
 * b32_scene_patch_faces      one lane per record writes the whole B32Face.  Which faces can reach the transparent pass is host
 *     bookkeeping derived from ALL faces (editor_alpha, blend_mode, the texture's blend mode); it comes out as a fresh upload's would, the
 *     transitions to and from "no face blends" included.  This needs the old faces: the FIRST face patch after an upload or
 *     b32_room_build_mesh copies the body's faces to the host (one host synchronisation); later ones are incremental and do not
 *     synchronise.  Vertex indices are not validated: as after an upload, one out of range is the frame's B32_E_INDEX.
 * b32_scene_patch_texels     the rectangle into the texel pool: Color15 (uint16_t) for an RGB555 scene, 4-byte Color for a scene of
 *     b32_scene_upload_rgba.  The skip mask is rebuilt by the next frame.  On an 8-bit-colour scene whether ANY texel blends decides the
 *     walk; to know when the last one goes, the first texel patch after an upload copies the pool to the host (one host synchronisation).
 * b32_scene_patch_indexed    indices[] looked up in clut[] (Clut::lookup: an index at or past clut_len is 0x0000) into the pool of an
 *     RGB555 scene (B32_E_ARG on an 8-bit-colour one).  A scene of b32_scene_upload_indexed with ONE texture keeps its index atlas and CLUT
 *     for the fill (B32_ROUTE_LDS_ATLAS): the patch writes the kept indices too; a whole-texture patch also replaces the kept CLUT (zero
 *     behind a shorter one) -- a palette-only change is a whole-texture patch; a partial patch whose CLUT, zero-padded to 256 entries,
 *     differs from the kept one drops the kept atlas, and so does b32_scene_patch_texels (expanded texels have no index): the fill then
 *     reads the pool.
 * b32_scene_read_texels      blocking: the expanded pool texels of one texture (width * height elements), as they are on the device now.
 * Out of scope: vertex / face / texture counts and texture sizes (an upload), connectivity (an upload plus b32_topology_create), rooms
 * (b32_room_update*). */
typedef struct B32VertexPatch { uint32_t index; B32Vertex v; } B32VertexPatch;   /* 40 bytes */
typedef struct B32FacePatch   { uint32_t index; B32Face   f; } B32FacePatch;     /* 24 bytes */
int b32_scene_patch_vertices(b32_ctx* ctx, b32_scene* slot /* NULL: the context's resident scene */, const B32VertexPatch* recs, uint32_t n);
int b32_scene_patch_faces(b32_ctx* ctx, b32_scene* slot /* NULL: ditto */, const B32FacePatch* recs, uint32_t n);
int b32_scene_patch_texels(b32_ctx* ctx, b32_scene* slot /* NULL: ditto */, uint32_t tex, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                           const void* texels, uint32_t stride);
int b32_scene_patch_indexed(b32_ctx* ctx, b32_scene* slot /* NULL: ditto */, uint32_t tex, uint32_t x, uint32_t y, uint32_t w, uint32_t h,
                            const uint8_t* indices, uint32_t stride, const uint16_t* clut, uint32_t clut_len);
int b32_scene_read_texels(b32_ctx* ctx, b32_scene* slot /* NULL: ditto */, uint32_t tex, void* out);  /* blocking */

/* ---- mirror editing: the mirrored half built on the device into a derived slot ----------------------------------------------------------
 * With MirrorSettings enabled (modeler/state.rs:777-850; the default for symmetric characters) the modeler draws another mesh than it
 * edits (modeler/viewport.rs:1209-1311): behind the selected object's vertices it appends their twins -- mirrored in LOCAL space
 * (mirror_position, mirror_normal), then put through the vertex's bone, colour (base_color as f32 * 0.85) as u8 -- behind EACH of the
 * object's triangles that triangle's twin with reversed winding, and every later object's vertices shift.  The interleaving matters: equal
 * sort keys in painter's mode and equal depths in z-buffer mode are decided by face order, so twins drawn behind all body faces are
 * another frame.  Here `src` keeps the combined mesh -- pose, patch, b32_hover_mesh, b32_box_select and the overlays keep addressing it --
 * and b32_scene_build_mirror writes the mesh the reference would have assembled from src's BODY into `dst`, which the frame draws:
 *     patch_vertices(src) -> pose(src) -> build_mirror(src, dst) -> build_skeleton(dst) -> draw dst -> hover(src) -> overlay(src)
 *
 * The rule, by output position (it never looks at an index value).  c = v_count, v_end = v_first + v_count, f_end = f_first + f_count,
 * bv / bf = src's body counts.
 *   Vertices, bv + c: output i < v_end is src's vertex i bit for bit (posed, if src is posed); outputs v_end .. v_end + c are the twins of
 *   vertices v_first .. v_end; output i + c is src's vertex i for i >= v_end.
 *   A twin starts from the LOCAL position and normal -- src's rest stream when src is rigged, else its vertex as it is.  The component of
 *   `axis` gets its sign BIT flipped in both (Rust's -x: -0.0 <-> +0.0, a NaN keeps its payload; not 0 - x).  On a rigged src the twin is
 *   then posed by the pose pass's own arithmetic with the bone of the SOURCE vertex and the table of src's last b32_scene_pose (before the
 *   first pose and after a pose with n_bones = 0: the mirrored rest bits), exactly as b32_scene_patch_vertices poses.  uv is copied as
 *   bits; r, g, b are each (ch as f32 * dim) as u8 with Rust's saturating cast (NaN -> 0); blend is B32_BLEND_OPAQUE (Color::new,
 *   types.rs:773-775).
 *   Faces, bf + f_count: output j < f_first is face j; face j of the range goes to f_first + 2 * (j - f_first) and its twin to the next
 *   place with v = (v0 + c, v2 + c, v1 + c), the other eight bytes copied; face j >= f_end goes to j + f_count with all three indices
 *   + c.  The adds wrap (u32).  Indices are never validated: one out of range is the frame's B32_E_INDEX, as after an upload.
 *   v_count == 0 && f_count == 0 is legal: dst becomes a copy of src's body.
 *
 * b32_scene_build_mirror   ONE kernel on the context's stream, one lane per output element; no upload.  State is b32_room_build_mesh's:
 *     dst must hold an uploaded scene, its textures stay, its geometry is replaced, its rig and tail go (call b32_scene_build_skeleton on
 *     dst afterwards, as after a room build), its content counts as changed.  dst's transparent-pass bookkeeping comes out as a fresh
 *     upload of the built arrays with dst's textures leaves it.  Works for RGB555 and 8-bit-colour dst; src's pixel format is irrelevant.
 *     src is read only: its bits, rig, tail, content number, bounds cache, merged runs and query answers stay as they are.
 *     No host synchronisation, with two exceptions: the FIRST build after src's upload (or room build) copies src's body faces to the
 *     host once, as the first b32_scene_patch_faces does (face patches of src keep the copy current); and a growth of dst's buffers.
 *     Like b32_scene_pose it first settles a pending frame that may still be redrawn.
 * b32_mirror_counts        host only: the built mesh's counts for a body of nv vertices and nf faces.
 * Errors (nothing is enqueued, dst is untouched): NULL context or struct, src == dst (also through NULL), either slot without a scene, axis
 * not 1..3, v_first + v_count > bv, f_first + f_count > bf -> B32_E_ARG; an output count past 2^32 - 1 -> B32_E_UNSUPPORTED.
 * Out of scope: apply_mirror (mesh_editor.rs:1909; connectivity changes: an upload), constrain_to_plane (the host's edit), keeping dst's
 * tail across a build. */
#define B32_MIRROR_DIM 0.85f
typedef struct B32Mirror {          /* 32 bytes */
    uint32_t axis;                  /* 1 X, 2 Y, 3 Z (B32HoverParams' mirror_axis without the 0) */
    float    dim;                   /* the reference's 0.85 (viewport.rs:1273): B32_MIRROR_DIM */
    uint32_t v_first, v_count;      /* the selected object's vertices inside src's BODY */
    uint32_t f_first, f_count;      /* ... and its faces */
    uint32_t _pad[2];
} B32Mirror;
int b32_scene_build_mirror(b32_ctx* ctx, b32_scene* src /* NULL: the context's resident scene */, b32_scene* dst /* NULL: ditto */,
                           const B32Mirror* mirror);
int b32_mirror_counts(uint32_t nv, uint32_t nf, const B32Mirror* mirror, uint32_t* nv_out, uint32_t* nf_out);   /* host only */

/* ---- a frame of several meshes (scene.rs:112-261) -------------------------------------------------------------------------------
 * The console's render step is one render_mesh_15 call per room and per asset part onto the same framebuffer, with ONE camera and
 * light list per frame and per-mesh ambient, fog (per room, scene.rs:189-205) and backface culling (per part: double_sided,
 * scene.rs:133-137).  These three calls take that sequence -- the meshes resident in scene slots -- and produce the framebuffer (and
 * depth buffer) the sequential calls produce, bit for bit, but draw every run of meshes whose draws commute as ONE merged mesh (one
 * setup + fill kernel pair instead of one per mesh; a 12-room 320x240 frame is launch-latency bound otherwise):
 *   z-buffer mode with RGB555 output: runs of meshes, each run ended by the first mesh that has a transparent pass (semi-transparent
 *   faces blend against what was drawn before them, so that mesh keeps its place); painter's mode, the 8-bit-colour path, x-ray,
 *   orthographic views and wireframe phases: mesh by mesh, exactly as b32_render_scene_15_async would.
 * b32_frame_begin copies camera, settings and lights; b32_frame_add_scene appends a slot (which must HOLD its scene: not swapped into
 * the context) with its per-mesh parameters (NULL: the base settings' ambient and backface flags, no fog); b32_frame_end enqueues the
 * frame; b32_frame_finish reports errors as for any asynchronous frame.  Difference to the sequential calls in the ERROR case only: a
 * vertex index out of range or a NaN sort key in one mesh of a merged run (the reference panics there) leaves the whole run undrawn.
 * At most 32 meshes are merged into one draw; longer runs are split.  Merged meshes are cached per context while the member slots'
 * contents stay the same (any b32_scene_upload* into a member rebuilds).
 * What a member keeps of its own inside a run (pinned by tests/test_run_sheets.py): a texture id at or above the member's OWN texture
 * count is no texture (the face is untextured and opaque, whatever the next member's texture 0 is), a vertex index at or above its OWN
 * vertex count is the index error above; a depth tie between members goes to the earlier member, then to the earlier face, as the
 * sequential strict `z <` gives it.  Where a run ends: "has a transparent pass" is the host's bound -- a face with a blend mode or
 * editor_alpha < 255, or ANY texture of the slot with a blend mode, used by a face or not -- so such a slot ends its run even when the
 * device classifies nothing as transparent; an 8-bit-colour slot, a slot with a wireframe phase (base backface_wireframe and its own
 * backface_cull) and a slot without faces are drawn on their own and end the run in front of them; a run of one is a draw on its own.
 * A slot that does not hold its scene makes b32_frame_end return B32_E_ARG: the runs in front of it are enqueued, nothing behind it is,
 * and the context stays usable.  The cache holds 64 merged meshes and reuses the least recently used one; the same slots in another
 * order are another run. */
typedef struct B32MeshParams {
    float   ambient;
    uint8_t backface_cull, backface_wireframe, has_fog, _pad;
    B32Fog  fog;
} B32MeshParams;
int b32_frame_begin(b32_ctx* ctx, const B32Camera* camera, const B32Settings* base_settings);
int b32_frame_add_scene(b32_ctx* ctx, b32_scene* slot, const B32MeshParams* params /* nullable */);
int b32_frame_end(b32_ctx* ctx);
/* The same frame in ONE call: begin, n x add_scene (params[i], or the base settings' values when params is NULL), end. */
int b32_frame_submit(b32_ctx* ctx, const B32Camera* camera, const B32Settings* base_settings, b32_scene* const* slots,
                     const B32MeshParams* params /* nullable */, uint32_t n);
/* which: 0 merged draws, 1 mesh-by-mesh draws, 2 merged meshes built, 3 frames ended -- since the context was created (tests). */
unsigned long long b32_batch_count(const b32_ctx* ctx, int which);

/* ---- placed draws: facing and world offset per draw (render_asset_parts, scene.rs:112-171) ----------------------------------------
 * The reference never draws a placed object from world-space vertices: per part, per object and per frame it rotates the asset's LOCAL
 * vertices about Y by the object's facing, translates them by its world position (scene.rs:140-156) and only then calls render_mesh_15 /
 * render_mesh.  A B32Placement carries exactly that to the setup kernel, which applies it to the three vertices a lane has loaded, so a
 * resident mesh can move, turn and be drawn any number of times per frame without an upload:
 *     rx = x * cos_f - z * sin_f        rz = x * sin_f + z * cos_f
 *     pos    = (rx + wx, y + wy, rz + wz)
 *     normal = (nx * cos_f - nz * sin_f, ny, nx * sin_f + nz * cos_f)      (not renormalised; uv and colour unchanged)
 * every operation a separately rounded f32 operation in this order, no fused multiply-add.  The placed position is "the vertex" for
 * everything downstream (fixed-point snap, camera space, near test, fog, painter's key, light positions), the placed normal is what
 * flat and Gouraud lighting see.  cos_f / sin_f come from the caller (libm stays on the host, like the camera basis).  The reference
 * skips the transform altogether when neither facing nor position exceeds 0.0001 (has_transform, scene.rs:125) and then uses the local
 * vertices as they are -- it does not multiply by 1 and add 0: pass place = NULL for that case; NULL means "draw exactly as the
 * entry without a placement".  Nothing is validated about the numbers: a placement that produces a NaN sort key is reported as
 * B32_E_NAN_KEY by b32_frame_finish, like the reference's panic.
 *   b32_frame_add_scene_placed   b32_frame_add_scene with a placement for this draw.  The same slot may be added any number of times
 *                                in one frame, each time with its own placement (one upload, twenty crates).  The merged mesh of a run
 *                                does not depend on the placements: frames that differ only in them reuse it (b32_batch_count(ctx, 2)
 *                                stays constant).  Run splitting, the 32-mesh limit, the error semantics of merged runs and the
 *                                asynchronous modes are those of b32_frame_add_scene; a frame that has to be redrawn (grown buffers)
 *                                is redrawn with the placements it had.
 *   b32_frame_submit_placed      the whole table in one call: places[i] is read only where has_place[i] != 0; places == NULL or
 *                                has_place == NULL: no mesh is placed (b32_frame_submit).
 *   b32_render_scene_15_placed_async   the context's resident scene on its own, placed: RGB555 scenes like b32_render_scene_15_async,
 *                                8-bit-colour scenes (b32_scene_upload_rgba) like b32_render_scene_async (fog is ignored there: render_mesh
 *                                has none). */
typedef struct B32Placement {
    float cos_f, sin_f;          /* facing.cos(), facing.sin(), scene.rs:123-124 */
    float world_pos[3];          /* obj.world_position(room), scene.rs:248 */
} B32Placement;                  /* 20 bytes */
int b32_frame_add_scene_placed(b32_ctx* ctx, b32_scene* slot, const B32MeshParams* params /* nullable */, const B32Placement* place /* nullable */);
int b32_frame_submit_placed(b32_ctx* ctx, const B32Camera* camera, const B32Settings* base_settings, b32_scene* const* slots,
                            const B32MeshParams* params /* nullable */, const B32Placement* places /* nullable: n entries */,
                            const uint8_t* has_place /* nullable: n bytes */, uint32_t n);
int b32_render_scene_15_placed_async(b32_ctx* ctx, const B32Camera* camera, const B32Settings* settings, const B32Fog* fog /* nullable */,
                                     const B32Placement* place /* nullable */);

/* ---- picking: which placed resident mesh, and which of its triangles, lies under the cursor ----------------------------------------------
 * check_mesh_hit (editor/viewport_3d.rs:7700-7756; called per visible part of every enabled object, :7344-7400) and the face branch of the
 * modeler's find_hovered_element (modeler/viewport.rs:2544-2594) walk every triangle of meshes this library already holds.  An item is one
 * (slot, placement) pair; for the cursor (mx, my) in framebuffer coordinates the device runs, per item,
 *     closest = None
 *     for t in 0..nf, in face order:
 *         a vertex index >= nv                          -> skip (screen_verts.get(..) is None: no error)
 *         P_k = (x*cos_f - z*sin_f + wx, y + wy, x*sin_f + z*cos_f + wz)      the placement is ALWAYS applied (no has_transform shortcut)
 *         (sx_k, sy_k, d_k) = world_to_screen_with_depth(P_k) (ortho == NULL, math.rs:621-652) or
 *                             world_to_screen_with_ortho_depth(P_k, ortho) (math.rs:580-617); any None -> skip
 *         area = (sx1 - sx0)*(sy2 - sy0) - (sx2 - sx0)*(sy1 - sy0);  B32_PICK_CULL_BACKFACES and area <= 0.0 -> skip (a NaN area is kept)
 *         !point_in_triangle_2d(mx, my, ...) (math.rs:687-706) -> skip
 *         depth = interpolate_depth_in_triangle(...) (viewport_3d.rs:7485-7508)
 *         if closest is None or depth < closest.depth: closest = (depth, t)
 * and then, over the items in array order (viewport_3d.rs:7370),
 *         if closest_i is Some and (best is None or closest_i.depth < best.depth): best = i
 * with every expression an f32 operation in the reference's order (no contraction, Vec3::dot = (x*ox + y*oy) + z*oz).  The strict `<`
 * decides everything and its consequences are reproduced: among equal depths (-0.0 == +0.0) the first in loop order wins and its own
 * depth bits are reported; a hit with a NaN depth is taken when it is the first hit and then never replaced, and ignored after a number
 * (a face (i, i, i) is hit from every cursor; a face with a NaN vertex passes the near test and is "inside" for every cursor).  One
 * departure, as in b32_draw_world: a NaN depth is reported as the one quiet NaN 0x7FC00000.
 * The framebuffer size is the context's (b32_fb_size); a band (b32_set_band) is ignored.  Slots must HOLD their scene, as for
 * b32_frame_add_scene; the same slot may appear any number of times.  A NULL or empty slot, NULL places with n > 0, an unknown flag or a
 * zero-size framebuffer -> B32_E_ARG; n > 65535 -> B32_E_UNSUPPORTED; n == 0 -> *best = -1.  Nothing about the numbers is validated.
 * The work is enqueued on the context's stream behind the uploads into the slots.  It neither reads nor writes the framebuffer or the
 * z-buffer, flushes no deferred clear, settles or supersedes no pending frame and changes no b32_batch_count.
 * b32_pick_meshes_async performs no host synchronisation: it delivers 16 + 16 * n bytes -- {int32 best; uint32 n; 8 bytes of padding},
 * then n B32PickHit -- into the caller's memory (preferably from b32_host_alloc) and completes through the tickets of
 * b32_fb_download_async (b32_ticket_poll / _wait; the same limit of 8 outstanding).  b32_pick_meshes is the asynchronous form followed
 * by a wait on its own ticket only. */
typedef struct B32PickHit { uint32_t hit; uint32_t tri; float depth; uint32_t _pad; } B32PickHit;   /* 16 bytes; hit == 0: tri = 0xFFFFFFFF, depth = 0 */
#define B32_PICK_CULL_BACKFACES 1u
struct B32Ortho;                 /* OrthoProjection: defined with the world-space overlays below */
int b32_pick_meshes(b32_ctx* ctx, const B32Camera* camera, const struct B32Ortho* ortho /* nullable */, float mx, float my, uint32_t flags,
                    b32_scene* const* slots, const B32Placement* places /* n entries, required */, uint32_t n,
                    B32PickHit* hits /* n entries, nullable */, int32_t* best /* -1: nothing hit */);
int b32_pick_meshes_async(b32_ctx* ctx, const B32Camera* camera, const struct B32Ortho* ortho /* nullable */, float mx, float my, uint32_t flags,
                          b32_scene* const* slots, const B32Placement* places /* n entries, required */, uint32_t n,
                          void* out /* 16 + 16 * n bytes */, uint64_t* ticket);

/* ---- hover and box selection: which vertex, else edge, else face of ONE resident mesh lies under the cursor ------------------------------
 * find_hovered_element (modeler/viewport.rs:2379-2601) and apply_box_selection (modeler/viewport.rs:1624-1779) walk the modeler's n-gons;
 * to_render_data_textured (modeler/mesh_editor.rs:1623-1653) keeps the vertices 1:1 and fan-triangulates the faces, so a slot's vertex
 * indices are the modeler's, but its triangles do not give the polygon edges back.  A b32_topology holds the polygons: poly_start[p] ..
 * poly_start[p + 1] index poly_verts, whose entries index a slot's vertices.  It belongs to no slot (the slot's nv is applied per call) and
 * nothing about the indices is validated: an index >= nv behaves as mesh.vertices.get(..) == None does in each loop.  Creation derives,
 * once, the half-edges (v[k], v[(k + 1) % n]) in loop order (Face::edges, mesh_editor.rs:92-95; also for n = 0, 1, 2) with the id of their
 * normalised edge (min, max), and the fan triangles (v[0], v[k], v[k + 1]) in loop order (Face::triangulate, mesh_editor.rs:99-112; none
 * for n < 3) with their polygon.  A NULL array with np > 0 (poly_verts only when there are indices to read: polygons that are all
 * empty may come with NULL), a poly_start that decreases or poly_start[0] != 0 -> B32_E_ARG.
 *
 * b32_hover_mesh evaluates ALL THREE branches of find_hovered_element for the cursor (mx, my) and reports each as its own loop finds it;
 * the reference's answer is vertex, edge only without a vertex, face only without either (the loops do not read one another, so masking
 * afterwards is the same function).  Positions: place == NULL uses the slot's vertices as they are (the modeler without bones), else the
 * placement is always applied as in b32_pick_meshes; projection is world_to_screen_with_ortho (math.rs:538-575); the framebuffer size is
 * the context's, a band is ignored.  Every expression is a separately rounded f32 operation in the reference's order.
 *   front pass (viewport.rs:2435-2473; not with B32_HOVER_SEE_THROUGH): a polygon with n >= 3 whose first three indices are < nv and
 *       project, with (sx1-sx0)*(sy2-sy0) - (sx2-sx0)*(sy1-sy0) > 0.0 (a NaN area is not front), marks its vertices < nv and all its
 *       normalised edges.
 *   vertices (viewport.rs:2475-2505), in index order: skipped when culling and unmarked; when the mirror is on and not
 *       local_pos[axis] >= -mirror_threshold (state.rs:797-806; a NaN fails); when it does not project;
 *       dist = sqrt((mx-sx)*(mx-sx) + (my-sy)*(my-sy)); candidate when dist < vertex_threshold; kept with a strict `<`.
 *   half-edges (viewport.rs:2507-2542), in loop order: skipped when culling and their normalised edge is unmarked; when an index is >= nv;
 *       unless both local positions pass the mirror test and both ends project; dist = point_to_line_distance (viewport.rs:2604-2622) in
 *       the half-edge's OWN orientation (len_sq < 0.001 -> the distance to the first end; t.clamp(0.0, 1.0) keeps a NaN and -0.0);
 *       candidate when dist < edge_threshold; kept with a strict `<`; reported as the normalised pair.
 *   faces (viewport.rs:2544-2594), polygons in order: a polygon is skipped whole unless EVERY index is < nv and passes the mirror test;
 *       its fan triangles go through the body of b32_pick_meshes' loop (culling = not SEE_THROUGH); closest by a strict `<` (the first of
 *       equal depths; a NaN depth only when it comes first, reported as 0x7FC00000); reported as the POLYGON index.
 * NULL context, camera, slot, topology or params, a slot that does not hold its scene, a zero-size framebuffer, an unknown flag or
 * mirror_axis > 3 -> B32_E_ARG; nv == 0 or np == 0 -> "none" in the branches that have nothing to walk.  Like a pick, the work is enqueued
 * on the context's stream behind the uploads into the slot, touches neither framebuffer nor z-buffer, flushes no clear and settles no
 * frame; the asynchronous form performs no host synchronisation and delivers 32 bytes through the tickets of b32_fb_download_async.
 *
 * b32_box_select is apply_box_selection for one rectangle.  B32_BOX_VERTICES (viewport.rs:1708-1726): bit i is set iff vertex i projects
 * and sx >= x0 && sx <= x1 && sy >= y0 && sy <= y1 (inclusive; any NaN gives false; no culling, no mirror).  B32_BOX_POLYGONS
 * (viewport.rs:1743-1766; needs a topology): the centre fold(Vec3::ZERO, acc + p) * (1.0 / count as f32) over the polygon's vertices with
 * index < nv, in order (a polygon with none is skipped), projected and tested the same way.  The result is {uint32 n_elements; uint32
 * n_selected; 8 bytes of padding}, then ceil(n_elements / 32) words, bit i of word i / 32: the reference pushes in ascending index
 * order, so the bitmap is the selection ("add to selection" stays with the caller).  The blocking form copies the words into `words`
 * (nullable); the asynchronous form delivers 16 + 4 * ceil(n_elements / 32) bytes by ticket.  mode > 1, B32_BOX_POLYGONS without a
 * topology, and what b32_hover_mesh rejects -> B32_E_ARG. */
typedef struct b32_topology b32_topology;
int  b32_topology_create(b32_ctx* ctx, const uint32_t* poly_start /* np + 1, non-decreasing, [0] == 0 */, uint32_t np,
                         const uint32_t* poly_verts /* poly_start[np] indices into a slot's vertices; may be NULL when that is 0 */, b32_topology** out);
void b32_topology_destroy(b32_ctx* ctx, b32_topology* topology);
typedef struct B32HoverParams {
    float mx, my;                             /* cursor, framebuffer coordinates */
    float vertex_threshold, edge_threshold;   /* the reference's constants: 6.0, 4.0 (viewport.rs:2428-2429) */
    uint32_t flags;                           /* B32_HOVER_SEE_THROUGH: xray_mode || double_sided */
    uint32_t mirror_axis;                     /* 0 off, 1 X, 2 Y, 3 Z (MirrorSettings, modeler/state.rs:777-806) */
    float mirror_threshold; uint32_t _pad;
} B32HoverParams;                             /* 32 bytes */
typedef struct B32HoverResult {
    uint32_t vertex; float vertex_dist;       /* none: 0xFFFFFFFF, 0 */
    uint32_t edge_v0, edge_v1; float edge_dist;   /* normalised (min, max) of the winning half-edge; none: both 0xFFFFFFFF, 0 */
    uint32_t face; float face_depth;          /* POLYGON index; none: 0xFFFFFFFF, 0; a NaN depth is reported as 0x7FC00000 */
    uint32_t _pad;
} B32HoverResult;                             /* 32 bytes */
#define B32_HOVER_SEE_THROUGH 1u
int b32_hover_mesh(b32_ctx* ctx, const B32Camera* camera, const struct B32Ortho* ortho /* nullable */, b32_scene* slot, b32_topology* topology,
                   const B32Placement* place /* nullable */, const B32HoverParams* params, B32HoverResult* out);
int b32_hover_mesh_async(b32_ctx* ctx, const B32Camera* camera, const struct B32Ortho* ortho /* nullable */, b32_scene* slot, b32_topology* topology,
                         const B32Placement* place /* nullable */, const B32HoverParams* params, void* out /* 32 bytes */, uint64_t* ticket);
typedef struct B32BoxParams { float x0, y0, x1, y1; uint32_t mode; uint32_t _pad[3]; } B32BoxParams;   /* 32 bytes */
#define B32_BOX_VERTICES 0u
#define B32_BOX_POLYGONS 1u
int b32_box_select(b32_ctx* ctx, const B32Camera* camera, const struct B32Ortho* ortho /* nullable */, b32_scene* slot,
                   b32_topology* topology /* nullable for B32_BOX_VERTICES */, const B32Placement* place /* nullable */, const B32BoxParams* params,
                   uint32_t* words /* ceil(n_elements / 32), nullable */, uint32_t* n_selected);
int b32_box_select_async(b32_ctx* ctx, const B32Camera* camera, const struct B32Ortho* ortho /* nullable */, b32_scene* slot,
                         b32_topology* topology /* nullable for B32_BOX_VERTICES */, const B32Placement* place /* nullable */,
                         const B32BoxParams* params, void* out /* 16 + 4 * ceil(n_elements / 32) bytes */, uint64_t* ticket);

/* ---- room hover and box selection: which sector vertex, edge or face of the CURRENT ROOM lies under the cursor ---------------------------
 * The world editor's find_hovered_elements (editor/viewport_3d.rs:7028-7336: the three sector loops and the priority rule; its object
 * loop is b32_pick_meshes) and find_selections_in_rect (:7512-7594) walk the sector grid itself, not a render mesh: per face four heights
 * on a lattice of sector_size units (SECTOR_SIZE = 1024.0), which the editor changes while it drags.  A b32_room holds the grid and one
 * B32SectorFace per face in the reference's one loop order (iter_sectors, world/geometry.rs:2828-2835: gx outer, gz inner; inside a
 * sector floor, ceiling, the north, east, south and west walls by i, then the nwse and the nesw walls by i), which all four walks share.
 * kind: 0 Floor, 1 Ceiling, 2 WallNorth, 3 WallEast, 4 WallSouth, 5 WallWest, 6 WallNwSe, 7 WallNeSw; index: the i of SectorFace::Wall*(i),
 * 0 for floor and ceiling (carried, not read).  The device derives the corners, each a separately rounded f32 operation:
 *   bx = position[0] + (float)gx * S, bz = position[2] + (float)gz * S, corner k = (bx or bx + S, position[1] + heights[k], bz or bz + S)
 * with the (x, z) selectors (0 = base, 1 = base + S) of viewport_3d.rs:6603-6657, :7099-7170 and :7183-7279, which agree:
 *   Floor / Ceiling (0,0) (1,0) (1,1) (0,1)     North (0,0) (1,0) (1,0) (0,0)     East (1,0) (1,1) (1,1) (1,0)     South (1,1) (0,1) (0,1) (1,1)
 *   West (0,1) (0,0) (0,0) (0,1)                NwSe  (0,0) (1,1) (1,1) (0,0)     NeSw (1,0) (0,1) (0,1) (1,0)
 * b32_room_create copies n records (n == 0 is legal, faces may then be NULL); kind > 7 -> B32_E_ARG, n > 2^24 -> B32_E_UNSUPPORTED (ordinals
 * are 4 * record + k); numbers are not validated.  b32_room_update is a height drag: records [first, first + count) are replaced and,
 * when grid is not NULL, the grid too; the data is copied before return and ordered on the context's stream like a slot upload, so a
 * hover enqueued behind it sees it.  first + count > n or a kind > 7 -> B32_E_ARG (nothing is changed).  b32_room_destroy waits for the
 * stream.
 *
 * b32_room_hover evaluates ALL THREE loops for the cursor and reports each raw.  Projection is world_to_screen_with_depth
 * (math.rs:621-652), perspective only; the framebuffer size is the context's, a band is ignored.  A record's four corners are projected
 * once and feed all three branches (the reference projects the same corner with the same function in each loop).
 *   vertices, ordinal 4 * rec + k: the corner projects; dist = sqrt((mx-sx)*(mx-sx) + (my-sy)*(my-sy)); candidate when
 *       dist < vertex_threshold; its depth is the corner's camera depth.
 *   edges (k, (k + 1) % 4), ordinal 4 * rec + k: both ends project; dist = point_to_segment_distance (math.rs:655-683; len_sq < 1e-6 -> the
 *       distance to the first end; t.clamp(0.0, 1.0) keeps a NaN) in the edge's own orientation; candidate when dist < edge_threshold;
 *       depth = interpolate_edge_depth (viewport_3d.rs:7411-7431: len_sq < 0.0001 -> (d0 + d1) * 0.5, else d0 + t * (d1 - d0)).
 *   faces, ordinal rec: check_quad_hit_with_depth (:7436-7481): all four corners project; triangle (0,1,2), and only when it misses
 *       (0,2,3); point_in_triangle_2d and interpolate_depth_in_triangle as in b32_pick_meshes, no culling.
 * In every loop a candidate is kept when there is none yet or its depth is strictly smaller: the SMALLEST DEPTH wins, not the smallest
 * distance; ties go to the first in loop order, with its own bits; a NaN depth sticks when it comes first and is ignored after a number;
 * it is reported as 0x7FC00000.  "None": indices 0xFFFFFFFF, floats 0.
 * b32_room_hover_winner is the reference's answer (:7283-7336), a pure host function: 0 vertex, 1 edge, 2 face, -1 nothing.  The
 * candidates (depth, type) are sorted by depth, tolerance = closest * 0.01, the lowest type among those with |d - closest| < tolerance
 * wins, else the closest one's type (a tolerance <= 0 -- a closest depth <= 0 -- selects nobody, so the closest wins).  With a NaN among
 * the depths the reference's result depends on its standard library's sort; here the sort is a stable insertion sort in which a NaN
 * compares equal to everything (partial_cmp(..).unwrap_or(Equal)), so a NaN stays where it was pushed relative to its neighbours.
 * Like a pick, the work is enqueued on the context's stream behind the room's uploads, touches neither framebuffer nor z-buffer, flushes
 * no clear and settles no frame; the asynchronous form performs no host synchronisation and delivers 48 bytes through the tickets of
 * b32_fb_download_async.  NULL context, camera, room, params or out, a zero-size framebuffer -> B32_E_ARG.
 *
 * b32_room_box_select is find_selections_in_rect for the rectangle (x0, y0, x1, y1).  Element i is record i for i < n, then point i - n of
 * points_xyz (the room's object positions, :7584-7591; nullable with n_points == 0).  A record's centre (face_center_in_rect /
 * wall_center_in_rect, :7597-7655): avg = (((h0 + h1) + h2) + h3) / 4.0; floor and ceiling (bx + S / 2.0, position[1] + avg, bz + S / 2.0);
 * walls ((x0 + x1) / 2.0, position[1] + avg, (z0 + z1) / 2.0) with that function's own (x0, z0, x1, z1) per direction.  The centre is
 * projected by world_to_screen (math.rs:503-534) and selected when sx >= x0 && sx <= x1 && sy >= y0 && sy <= y1 (inclusive; any NaN is
 * false).  The result has b32_box_select's layout: {uint32 n_elements; uint32 n_selected; 8 bytes of padding}, then ceil(n_elements / 32)
 * words.  n + n_points >= 2^32 -> B32_E_UNSUPPORTED. */
typedef struct b32_room b32_room;
typedef struct B32SectorFace {
    uint16_t gx, gz;                          /* the sector on the room's grid */
    uint8_t  kind;                            /* 0 Floor, 1 Ceiling, 2 WallNorth, 3 WallEast, 4 WallSouth, 5 WallWest, 6 WallNwSe, 7 WallNeSw */
    uint8_t  index;                           /* the i of SectorFace::Wall*(i); 0 for floor and ceiling */
    uint16_t _pad;
    float    heights[4];
} B32SectorFace;                              /* 24 bytes */
typedef struct B32RoomGrid { float position[3]; float sector_size; } B32RoomGrid;   /* Room::position; SECTOR_SIZE = 1024.0 */
#define B32_SECTOR_SIZE 1024.0f
#define B32_ROOM_MAX_FACES (1u << 24)
typedef struct B32RoomHoverParams { float mx, my, vertex_threshold, edge_threshold; } B32RoomHoverParams;   /* the reference's: 6.0, 4.0 */
typedef struct B32RoomHover {
    uint32_t vertex_rec, vertex_corner; float vertex_dist, vertex_depth;
    uint32_t edge_rec,   edge_idx;      float edge_dist,   edge_depth;
    uint32_t face_rec;                  float face_depth;
    uint32_t _pad[2];
} B32RoomHover;                               /* 48 bytes; none: indices 0xFFFFFFFF, floats 0 */
int  b32_room_create(b32_ctx* ctx, const B32RoomGrid* grid, const B32SectorFace* faces, uint32_t n, b32_room** out);
int  b32_room_update(b32_ctx* ctx, b32_room* room, const B32RoomGrid* grid /* nullable */, uint32_t first, uint32_t count, const B32SectorFace* faces);
void b32_room_destroy(b32_ctx* ctx, b32_room* room);
int  b32_room_hover(b32_ctx* ctx, const B32Camera* camera, b32_room* room, const B32RoomHoverParams* params, B32RoomHover* out);
int  b32_room_hover_async(b32_ctx* ctx, const B32Camera* camera, b32_room* room, const B32RoomHoverParams* params, void* out /* 48 bytes */,
                          uint64_t* ticket);
int  b32_room_hover_winner(const B32RoomHover* hover);
int  b32_room_box_select(b32_ctx* ctx, const B32Camera* camera, b32_room* room, float x0, float y0, float x1, float y1,
                         const float* points_xyz /* 3 * n_points, nullable */, uint32_t n_points,
                         uint32_t* words /* ceil((n + n_points) / 32), nullable */, uint32_t* n_selected);
int  b32_room_box_select_async(b32_ctx* ctx, const B32Camera* camera, b32_room* room, float x0, float y0, float x1, float y1,
                               const float* points_xyz /* 3 * n_points, nullable */, uint32_t n_points,
                               void* out /* 16 + 4 * ceil((n + n_points) / 32) bytes */, uint64_t* ticket);

/* ---- a room's render mesh, built on the device from its resident sector table ------------------------------------------------------------
 * render_scene calls Room::to_render_data_with_textures (world/geometry.rs:2839-3352) for every room on every frame; a host of this
 * library keeps the result in a scene slot and has to re-run it, upload 36 bytes per vertex and wait whenever the editor drags a height.
 * The room's heights are resident already (b32_room_update), so the mesh is made where they are: b32_room_build_mesh writes the
 * vertices and faces of that function into a slot's own geometry with one launch on the context's stream.
 *
 * One B32FaceMaterial per B32SectorFace, in the same order, holds everything add_horizontal_face_to_render_data, add_wall_to_render_data
 * and add_diagonal_wall_to_render_data read besides the grid and the heights; the host resolves the Options as the reference's getters
 * do (geometry.rs:1193-1210):
 *   texture_id, tex_width       resolve_texture(&face.texture).unwrap_or((0, 64)); uv_scale = 32.0 / (tex_width as f32), a width of 0 gives inf
 *   texture_id_2, tex_width_2   floor and ceiling only: the same of get_texture_2()
 *   uv, B32_MAT_HAS_UV          face.uv; without the flag the world-aligned defaults from (gx, gz) and uv_scale
 *   uv_2, B32_MAT_HAS_UV_2      get_uv_2(), that is uv_2.or(uv): the flag is set when EITHER is Some; without it triangle 2 has triangle 1's
 *                               UVs when the widths are equal, else the defaults at its own scale
 *   colors, colors_2            r, g, b, blend per corner; colors_2 is get_colors_2() (floor and ceiling only)
 *   heights_2, B32_MAT_HAS_HEIGHTS_2   triangle 2's heights; without the flag the record's own (the hover never reads them)
 *   normal_mode 0 Front 1 Both 2 Back; split_direction 0 NwSe 1 NeSw; uv_projection 0 Default 1 Projected (walls); blend_mode; black_transparent
 * Where a record's output lies depends on (kind, normal_mode) alone: a floor or ceiling emits 6 vertices and 2 faces per rendered side
 * (triangle 1 front, triangle 1 back, triangle 2 front, triangle 2 back), a wall 4 vertices and 2 faces per side (front, then back); Both
 * renders two sides.  The room keeps kinds and modes on the host with the prefix sums of those counts and uploads the sums in stream order
 * whenever b32_room_update or b32_room_update_materials changes a kind or a mode; b32_room_mesh_counts is a pure host function.
 * A face's indices are absolute (vertices.len() in the reference), editor_alpha is 255.  The arithmetic is the reference's, each
 * operation rounded separately (csrc/b32_room_mesh_body.h), with one exception: a float of a vertex that is a NaN is written as
 * 0x7FC00000 -- the sign of a generated NaN is the machine's, not the reference's.
 *
 * b32_room_set_materials copies the whole table (n records); b32_room_update_materials a range, with b32_room_update's contract: the data
 * is copied before return and ordered on the context's stream; first + count > n or normal_mode > 2, split_direction > 1,
 * uv_projection > 1, blend_mode > 5 in any record -> B32_E_ARG, nothing changed (also for a range before any table was set).
 * b32_room_build_mesh(ctx, room, slot): the slot (NULL: the context's resident scene) must hold an uploaded scene -- its textures stay, its
 * geometry, of which it may have had none (an upload with nv == nf == 0 is legal), is replaced, a rig is dropped (b32_scene_pose then
 * returns B32_E_ARG), merged runs that hold the slot are rebuilt.  A pending frame that may still be redrawn is settled first.  No host
 * synchronisation unless the slot's buffers have to grow.  Works for RGB555 and 8-bit-colour slots.  No materials set, no scene in the
 * slot -> B32_E_ARG.  b32_scene_read_faces is b32_scene_read_vertices for the faces (blocking; for tests). */
typedef struct B32FaceMaterial {
    uint32_t texture_id, tex_width;
    uint32_t texture_id_2, tex_width_2;
    float    uv[4][2];
    float    uv_2[4][2];
    uint8_t  colors[4][4];                    /* r, g, b, blend */
    uint8_t  colors_2[4][4];
    float    heights_2[4];
    uint8_t  normal_mode, split_direction, uv_projection, blend_mode, black_transparent, flags;
    uint8_t  _pad[2];
} B32FaceMaterial;                            /* 136 bytes */
#if defined(__cplusplus)
static_assert(sizeof(B32FaceMaterial) == 136, "B32FaceMaterial layout");
#else
_Static_assert(sizeof(B32FaceMaterial) == 136, "B32FaceMaterial layout");
#endif
#define B32_MAT_HAS_UV 1u
#define B32_MAT_HAS_UV_2 2u
#define B32_MAT_HAS_HEIGHTS_2 4u
#define B32_NORMAL_FRONT 0u
#define B32_NORMAL_BOTH 1u
#define B32_NORMAL_BACK 2u
#define B32_SPLIT_NWSE 0u
#define B32_SPLIT_NESW 1u
#define B32_UV_DEFAULT 0u
#define B32_UV_PROJECTED 1u
int  b32_room_set_materials(b32_ctx* ctx, b32_room* room, const B32FaceMaterial* materials /* n records */);
int  b32_room_update_materials(b32_ctx* ctx, b32_room* room, uint32_t first, uint32_t count, const B32FaceMaterial* materials);
int  b32_room_mesh_counts(const b32_room* room, uint32_t* n_vertices, uint32_t* n_faces);
int  b32_room_build_mesh(b32_ctx* ctx, b32_room* room, b32_scene* slot /* NULL: the context's resident scene */);
int  b32_scene_read_faces(b32_ctx* ctx, b32_scene* slot /* NULL: ditto */, uint32_t first, uint32_t count, B32Face* out);  /* blocking */

/* ---- the 8-bit-colour path: render_mesh (render.rs:1971-2264) + rasterize_triangle (render.rs:1202-1433) ----
 * What every caller of the reference runs when settings.use_rgb555 is false (scene.rs:163-169).  Same pipeline and settings
 * as render_mesh_15 except: Texture texels are Color values with a per-texel blend mode, no fog, no opaque/transparent
 * partition (one depth sort of all surfaces in painter's mode), every passing fragment writes depth in z-buffer mode. */
int b32_render_mesh(b32_ctx* ctx,
                    const B32Vertex* vertices, uint32_t nv,
                    const B32Face* faces, uint32_t nf,
                    const B32Texture* textures, uint32_t nt,
                    const B32Camera* camera, const B32Settings* settings,
                    B32Timings* out /* nullable */);
int b32_scene_upload_rgba(b32_ctx* ctx,
                          const B32Vertex* vertices, uint32_t nv,
                          const B32Face* faces, uint32_t nf,
                          const B32Texture* textures, uint32_t nt);
/* Draws the scene uploaded by b32_scene_upload_rgba; finish with b32_frame_finish like the _15 form. */
int b32_render_scene(b32_ctx* ctx, const B32Camera* camera, const B32Settings* settings, B32Timings* out /* nullable */);
int b32_render_scene_async(b32_ctx* ctx, const B32Camera* camera, const B32Settings* settings);

/* ---- the steps around the mesh draw that the reference runs on the same framebuffer ----------
 * so that a whole frame can stay device resident.  The procedural inputs that use sin/cos/powf (Skybox::generate_mesh,
 * world/geometry.rs:529; star directions and twinkle, render.rs:166-196) are computed by the caller, like the camera basis. */
typedef struct B32SkyVertex { float pos[3]; uint8_t r, g, b, blend; } B32SkyVertex;       /* SkyboxVertex{pos, color} */
/* Framebuffer::clear_gradient, render.rs:58-77 (top at y = 0, bottom at y = height-1; also resets the z-buffer) */
int b32_fb_clear_gradient(b32_ctx* ctx, uint8_t top_r, uint8_t top_g, uint8_t top_b, uint8_t top_blend,
                          uint8_t bottom_r, uint8_t bottom_g, uint8_t bottom_b, uint8_t bottom_blend);
/* Framebuffer::clear_transparent, render.rs:47-56 */
int b32_fb_clear_transparent(b32_ctx* ctx);
/* Step 1 of Framebuffer::render_skybox, render.rs:81-134: project (math.rs:117-136), cull and fill the vertex-coloured sphere with
 * rasterize_skybox_triangle (render.rs:251-298).  `faces` = 3 vertex indices per face, drawn in order. */
int b32_render_skybox_mesh(b32_ctx* ctx, const B32SkyVertex* vertices, uint32_t nv, const uint32_t* faces, uint32_t nf,
                           const B32Camera* camera);
/* draw_star_diamond, render.rs:199-240, for n stars in order: centre (cx, cy) = (screen.x as i32, screen.y as i32), colour rgb[3*i..]. */
int b32_draw_star_diamonds(b32_ctx* ctx, const int32_t* cx, const int32_t* cy, const uint8_t* rgb, uint32_t n, float size);

/* A resident sky: the mesh of Skybox::generate_mesh (world/geometry.rs:529-720) kept on the device and drawn per frame from the camera
 * alone.  The reference computes every position as camera_pos + x * radius (sphere :555-559, mountains :686-710) with x * radius
 * independent of the camera, and colours that depend on `time` only inside cloud layers: the host keeps the libm part (sin, cos, acos,
 * powf), the device adds the camera.  A b32_sky belongs to the context it was created on: with another context -> B32_E_ARG. */
typedef struct b32_sky b32_sky;
/* offsets[i].pos = the three products the reference ADDS to camera_pos (world/geometry.rs:555-559, :686-710): x * radius, y * radius,
 * z * radius -- generate_mesh((0, 0, 0), time) gives them, but for the sign of a zero (0.0 + -0.0 = +0.0), which no projected coordinate
 * can see: camera_pos + -0.0 and camera_pos + +0.0 are the same f32 unless camera_pos is -0.0, and then the position is -0.0 or +0.0
 * and position - camera_pos is +0.0 either way (tests/test_resident_sky.py walks every combination).  Colours as in B32SkyVertex.  faces: 3 indices per face, drawn in order.  An index >= nv -> B32_E_INDEX and nothing is created (*out
 * is written on success only).  nv == 0 or nf == 0: a sky that draws nothing.  The arrays are reusable when the call returns. */
int  b32_sky_create(b32_ctx* ctx, const B32SkyVertex* offsets, uint32_t nv, const uint32_t* faces, uint32_t nf, b32_sky** out);
void b32_sky_destroy(b32_ctx* ctx, b32_sky* sky);                           /* NULL: no-op; waits for the context's stream */
/* vertices [first, first + count) replaced (offset and colour; a scrolling cloud layer of world/geometry.rs:600-660 changes the colours
 * of its rows), ordered on the context's stream: a render enqueued before the call sees the old ones, one enqueued after it the new
 * ones.  `verts` reusable when the call returns.  No host synchronisation.  first + count > nv, or count != 0 with verts == NULL ->
 * B32_E_ARG and nothing changes; count == 0: no-op. */
int  b32_sky_update(b32_ctx* ctx, b32_sky* sky, uint32_t first, uint32_t count, const B32SkyVertex* verts);
/* Step 1 of Framebuffer::render_skybox (render.rs:81-139) for generate_mesh(camera.position, ..): per vertex pos = camera.position +
 * offset, then render.rs:99-103 on pos - camera.position (two roundings: not the offset), then the fill of b32_render_skybox_mesh.
 * Only rows of the band are written, the z-buffer is untouched.  Enqueued on the context's stream behind everything enqueued before (a
 * deferred b32_fb_clear is flushed first); never waits, allocates or copies. */
int  b32_render_sky(b32_ctx* ctx, b32_sky* sky, const B32Camera* camera);
/* stage tap: the projected (x, y) per vertex for a w x h framebuffer (1 .. 16384 each), a NaN pair (0x7FC00000) behind the camera
 * (render.rs:99-103); blocking; needs no framebuffer */
int  b32_sky_project_batch(b32_ctx* ctx, b32_sky* sky, const B32Camera* camera, uint32_t w, uint32_t h, float* xy /* 2 * nv */);
/* The Framebuffer's line family (render.rs:684-872), drawn after the meshes by every caller (the player's cylinder, the editor's
 * outlines and gizmos, the modeler's edge overlay).  Lines never write the z-buffer; they read it (f32::MAX everywhere while it is not
 * valid, as in painter's mode).  Colour = Color{r, g, b, blend} (blend: BlendMode, B32_BLEND_ERASE -> alpha byte 0 in set_pixel,
 * types.rs:829-832); the *_ALPHA kinds blend rgb with `alpha` through set_pixel_alpha (render.rs:646-667) and ignore `blend`. */
typedef struct B32Line {
    int32_t x0, y0, x1, y1;
    float   z0, z1;             /* ignored by the 2-D kinds */
    uint8_t r, g, b, blend;
    uint8_t kind;               /* B32_LINE_* */
    uint8_t alpha;              /* the *_ALPHA kinds */
    uint8_t _pad[2];
} B32Line;                      /* 32 bytes */
#define B32_LINE_2D          0u /* draw_line            render.rs:715-755 (draw_line_blended, Opaque -> set_pixel)  */
#define B32_LINE_2D_ALPHA    1u /* draw_line_alpha      render.rs:684-711 (set_pixel_alpha)                          */
#define B32_LINE_3D          2u /* draw_line_3d         render.rs:757-817, z <  zbuffer                               */
#define B32_LINE_3D_OVERLAY  3u /* draw_line_3d_overlay render.rs:764-766, z <= zbuffer                               */
#define B32_LINE_3D_ALPHA    4u /* draw_line_3d_alpha   render.rs:822-872, z * 0.995 both ends, <=, set_pixel_alpha    */
/* Draws lines[0..n) as the reference methods called one after another in array order on the current framebuffer: every pixel and
 * byte equal, only rows of the band written.  Asynchronous: enqueued on the context's stream behind everything enqueued before (a
 * deferred b32_fb_clear is flushed first) and ahead of everything after it; `lines` may be reused as soon as the call returns (the
 * batch is copied).  The whole batch is checked first and nothing is drawn if a line is rejected: an unknown kind -> B32_E_ARG; an
 * extent |x1-x0| or |y1-y0| >= 2^30 (2*err overflows i32 in the reference) -> B32_E_UNSUPPORTED.  n == 0: no-op. */
int b32_draw_lines(b32_ctx* ctx, const B32Line* lines, uint32_t n);
/* The rest of the Framebuffer's drawing methods (render.rs:631-971), in one ordered batch with the line family: circles, thick lines,
 * rectangles and the PS1-blended line.  Colour = Color{r, g, b, blend} as in B32Line.  Single pixels need no kind of their own:
 * set_pixel is a 1x1 B32_PRIM_FILLED_RECT, set_pixel_alpha a one-point B32_LINE_2D_ALPHA (x0 == x1, y0 == y1), set_pixel_blended a
 * one-point B32_PRIM_LINE_BLENDED. */
typedef struct B32Prim {
    int32_t x0, y0, x1, y1;     /* lines, thick line, rects: end points / corners; circles: (x0, y0) = centre */
    float   z0, z1;             /* the 3-D line kinds only */
    int32_t size;               /* circles: radius; thick line: thickness; ignored by the other kinds */
    uint8_t r, g, b, blend;     /* Color{r, g, b, blend}, as in B32Line */
    uint8_t kind;               /* B32_PRIM_* */
    uint8_t alpha;              /* the *_ALPHA kinds */
    uint8_t mode;               /* B32_PRIM_LINE_BLENDED: the BlendMode argument of draw_line_blended */
    uint8_t _pad[5];
} B32Prim;                      /* 40 bytes */
/* kinds 0..4 mean exactly what B32_LINE_2D .. B32_LINE_3D_ALPHA mean */
#define B32_PRIM_LINE_BLENDED  5u /* draw_line_blended  render.rs:720-755 (mode Opaque -> set_pixel, else set_pixel_blended :313-334, which ignores
                                   * the colour's own blend and gives Color::TRANSPARENT for Erase) */
#define B32_PRIM_CIRCLE        6u /* draw_circle        render.rs:631-642 (set_pixel where dx*dx + dy*dy <= r*r; radius < 0: nothing)   */
#define B32_PRIM_CIRCLE_ALPHA  7u /* draw_circle_alpha  render.rs:670-681 (the same pixels, set_pixel_alpha)                          */
#define B32_PRIM_THICK_LINE    8u /* draw_thick_line    render.rs:875-938 (thickness <= 1: draw_line; else the f32 quad, set_pixel)   */
#define B32_PRIM_RECT          9u /* draw_rect          render.rs:941-951 (four draw_line edges of the normalised corners)          */
#define B32_PRIM_FILLED_RECT  10u /* draw_filled_rect   render.rs:954-971 (normalised, clamped, set_pixel: opaque)                  */
/* Draws prims[0..n) as the reference methods called one after another in array order, with b32_draw_lines's contract: every pixel and
 * byte equal, only rows of the band written, the z-buffer read (f32::MAX while it is not valid) and never written, enqueued on the
 * context's stream with no host synchronisation (a deferred clear is flushed first), `prims` reusable as soon as the call returns.
 * The whole batch is checked first and nothing is drawn if a primitive is rejected: an unknown kind, or B32_PRIM_LINE_BLENDED with
 * mode > B32_BLEND_ERASE -> B32_E_ARG; for kinds 0..5, B32_PRIM_THICK_LINE and B32_PRIM_RECT an extent |x1-x0| or |y1-y0| >= 2^30
 * -> B32_E_UNSUPPORTED; for circles |radius| > 32767 or |x0|, |y0| >= 2^30 (r*r, dx*dx + dy*dy or cy +- r overflow i32 in the
 * reference) -> B32_E_UNSUPPORTED.  B32_PRIM_FILLED_RECT takes any i32.  n == 0: no-op. */
int b32_draw_prims(b32_ctx* ctx, const B32Prim* prims, uint32_t n);

/* Stars through the ordered tile pass.  The star's direction, its visibility test and the twinkle stay with the caller: the reference's
 * LCG draws the phase only for a visible star (render.rs:184-191), so star i's direction depends on how many earlier stars the camera
 * sees.  A star is what draw_star_diamond is called with: */
typedef struct B32Star { int32_t cx, cy; uint8_t r, g, b, _pad; } B32Star;   /* 12 bytes: (screen.x as i32, screen.y as i32), the twinkled colour */
/* draw_star_diamond (render.rs:206-237) for stars[0..n) in order: 1, 5 or 9 set_pixel_safe calls per star with s = size.max(1.0) as i32
 * (NaN -> 1, the cast saturates) -- the centre, the four points at distance 1 when s >= 2 (colour channels (c as f32 * 0.7) as u8), the
 * four at distance 2 when s >= 3 ((c as f32 * 0.4) as u8); cx + dx wraps.  Each call becomes a 1x1 B32_PRIM_FILLED_RECT record ON THE
 * DEVICE (draw_filled_rect clamps to an empty range for anything outside, render.rs:954-971), and the records go through the ordered
 * tile pass with b32_draw_prims's contract: every pixel and byte equal, only rows of the band written, the z-buffer read (f32::MAX
 * while it is not valid) and never written, enqueued on the context's stream with no host synchronisation (a deferred clear is flushed
 * first), `stars` reusable as soon as the call returns.  n > (2^31 - 1) / 9 -> B32_E_UNSUPPORTED.  n == 0: no-op. */
int b32_draw_stars(b32_ctx* ctx, const B32Star* stars, uint32_t n, float size);
/* host only: *records = n * (1, 5 or 9) */
int b32_star_record_count(uint32_t n, float size, uint64_t* records);
/* stage tap: the records of b32_draw_stars, star i's at [i * per, (i + 1) * per) in the order centre, (-1,0), (+1,0), (0,-1), (0,+1),
 * (-2,0), (+2,0), (0,-2), (0,+2); blocking; needs no framebuffer.  More than `cap` records -> B32_E_ARG. */
int b32_star_records_batch(b32_ctx* ctx, const B32Star* stars, uint32_t n, float size, B32Prim* out, uint32_t cap, uint32_t* n_records);

/* World-space overlays (rasterizer/draw.rs:12-135, math.rs:503-652).  Every caller of the drawing methods above starts from world positions:
 * it projects both ends with one of the world_to_screen functions, casts with `as i32` and calls fb.draw_*.  An item is one such call:
 * it is projected ON THE DEVICE into the B32Prim of its kind, in array order, and the records go through the ordered tile pass of
 * b32_draw_prims without visiting the host.  The arithmetic is the reference's, operation for operation (f32, no contraction,
 * Vec3::dot = (x*ox + y*oy) + z*oz, Rust's saturating `as i32`).
 *   line kinds (0..5, B32_PRIM_THICK_LINE), no flag: each end through world_to_screen_with_ortho (2-D kinds 0, 1, 5, 8; math.rs:538-575)
 *     or world_to_screen_with_ortho_depth (3-D kinds 2, 3, 4; :580-617, z = camera z); nothing is drawn if either end is None.
 *   line kinds with B32_WORLD_CLIP_NEAR: draw_3d_line_clipped's near-plane clip first (draw.rs:19-42), then world_to_screen (:503-534) or
 *     world_to_screen_with_depth (:621-652); `ortho` is ignored, as the reference's clipped callers ignore it.  A clipped end can come
 *     out at camera z <= 0.1 after rounding, and then the segment is not drawn -- as in the reference.
 *   B32_PRIM_CIRCLE, B32_PRIM_CIRCLE_ALPHA: p0 through world_to_screen_with_ortho, radius `size`.
 * ortho == NULL: the perspective branch (camera z <= 0.1 is None); else the orthographic one, which never answers None.
 * One departure from the reference's bits, visible through the stage tap: a NaN depth (z0 / z1 of the 3-D kinds) is stored as the one
 * quiet NaN 0x7FC00000.  NaN payloads are specified neither by Rust nor by IEEE 754, and every NaN fails every depth test alike. */
typedef struct B32WorldItem {
    float   p0[3], p1[3];       /* world positions; the circle kinds use p0 only */
    int32_t size;               /* circles: radius; B32_PRIM_THICK_LINE: thickness */
    uint8_t r, g, b, blend;     /* Color{r, g, b, blend}, as in B32Prim */
    uint8_t kind;               /* what is drawn with the projected ends: B32_PRIM_* 0..8 (no rectangles) */
    uint8_t alpha, mode;        /* as in B32Prim */
    uint8_t flags;              /* B32_WORLD_CLIP_NEAR */
    uint8_t _pad[4];
} B32WorldItem;                 /* 40 bytes */
#define B32_WORLD_CLIP_NEAR 1u
typedef struct B32Ortho { float zoom, center_x, center_y; } B32Ortho;     /* OrthoProjection, types.rs:1432-1438 */
/* Draws items[0..n) as the reference's calls one after another in array order, with b32_draw_prims's contract: enqueued on the
 * context's stream behind everything enqueued before and ahead of everything after, a deferred clear flushed first, only rows of the
 * band written, the z-buffer read and never written, `items` reusable as soon as the call returns, n == 0 a no-op, no host
 * synchronisation.  An item that draws nothing becomes a record that draws nothing in its place (a circle of radius -1).
 * The whole batch is checked first: kind > B32_PRIM_THICK_LINE, an unknown flag, the clip flag on a circle, B32_PRIM_LINE_BLENDED with
 * mode > B32_BLEND_ERASE -> B32_E_ARG; a circle with |radius| > 32767 -> B32_E_UNSUPPORTED.  What else b32_draw_prims refuses (an extent
 * or a circle centre >= 2^30) is only known after projection: such a record is turned into a no-op on the device and counted as
 * `rejected`. */
int b32_draw_world(b32_ctx* ctx, const B32Camera* camera, const B32Ortho* ortho /* nullable */, const B32WorldItem* items, uint32_t n);
/* draw_floor_grid (draw.rs:81-135): b32_floor_grid_items drawn with b32_draw_world. */
int b32_draw_floor_grid(b32_ctx* ctx, const B32Camera* camera, float y, float spacing, float extent,
                        const uint8_t grid_rgbb[4], const uint8_t x_axis_rgbb[4], const uint8_t z_axis_rgbb[4]);
/* The segments of draw_floor_grid in the reference's call order, as B32_PRIM_LINE_2D items with B32_WORLD_CLIP_NEAR (host only, no
 * context): the two while loops with their f32 accumulation (x += spacing, .min(extent)); a line with |z| < 0.001 takes z_axis_rgbb, one
 * with |x| < 0.001 x_axis_rgbb (Color as r, g, b, blend).  *n = the number of segments; at most `cap` are written (out may be NULL).
 * The reference does not terminate for spacing <= 0, a non-finite argument or a spacing so small that x + spacing == x: B32_E_ARG.
 * More than 2^20 segments: B32_E_UNSUPPORTED. */
int b32_floor_grid_items(float y, float spacing, float extent, const uint8_t grid_rgbb[4], const uint8_t x_axis_rgbb[4],
                         const uint8_t z_axis_rgbb[4], B32WorldItem* out, uint32_t cap, uint32_t* n);
/* Stage tap: the records b32_draw_world would hand to the tile pass for a width x height framebuffer, copied back (synchronous). */
int b32_world_project_batch(b32_ctx* ctx, const B32Camera* camera, const B32Ortho* ortho /* nullable */, const B32WorldItem* items,
                            uint32_t n, uint32_t width, uint32_t height, B32Prim* out);
/* Items projected by this context so far (b32_draw_world, b32_draw_floor_grid and the stage tap): drawn, dropped (the reference itself
 * draws nothing: behind the camera, None) and rejected (see b32_draw_world).  Synchronises the stream. */
int b32_world_counts(b32_ctx* ctx, uint64_t* drawn, uint64_t* dropped, uint64_t* rejected);
/* The world editor's overlay helpers (editor/viewport_3d.rs:5687-6357).  The editor's viewport does not draw its overlay through
 * rasterizer/draw.rs but through a private family of helpers; three of them draw pixels nothing above can reproduce:
 *   draw_3d_line (:5687-5695 -> draw_3d_line_impl(use_depth = false), :5783-5882) clips the projected f32 segment to the framebuffer with
 *     a 16-round Cohen-Sutherland loop (clip_line_to_rect, :5886-5955) BEFORE the `as i32` casts, so a line that crosses the frame edge
 *     starts its Bresenham error term at the clipped end -- other pixels than draw_3d_line_clipped + fb.draw_line (B32_WORLD_CLIP_NEAR);
 *   draw_3d_thick_line_depth (:5709-5781) draws `thickness` parallel draw_line_3d_overlay lines whose integer offsets come from f32
 *     arithmetic on the cast end points;
 *   draw_filled_triangle_3d (:6295-6357), the body of draw_filled_octahedron (:6223-6292): a scan-line fill with no depth test that writes
 *     [r, g, b, 255] whatever the colour's blend.  The modeler's twin (modeler/viewport.rs:4663-4722) was read against it line by line: the
 *     two fill bodies are the same text (only comments differ), so B32_GIZMO_TRIANGLE and B32_GIZMO_TRIANGLE_VIEW differ in the projection
 *     alone (`cam.z < 0.1` and math.rs project against `cam_z <= 0.1` / the ortho branch of world_to_screen_with_ortho_depth).
 * An item is one such call.  It is projected ON THE DEVICE, in array order, into records of the ordered tile pass of b32_draw_prims; the
 * arithmetic is the reference's, operation for operation, as in b32_draw_world (NaN depths are stored as 0x7FC00000 there too):
 *   B32_GIZMO_LINE: the near-plane clip (:5794-5816, draw.rs:19-42 verbatim), world_to_screen on both ends, then
 *     clip_line_to_rect(x0f, y0f, x1f, y1f, 0.0, 0.0, w as f32, h as f32) literally (outcodes with `<` / `>=`, the first end preferred,
 *     BOTTOM, TOP, RIGHT, LEFT, ymax - 1.0 / xmax - 1.0, at most 16 rounds then None, a NaN coordinate has outcode 0), `as i32`, and one
 *     B32_LINE_2D record (the loop at :5861-5880 is draw_line's; set_pixel honours `blend`).
 *   B32_GIZMO_LINE_DEPTH: the record b32_draw_world makes for B32_LINE_3D_OVERLAY with B32_WORLD_CLIP_NEAR.
 *   B32_GIZMO_THICK_LINE_DEPTH: size <= 1 is B32_GIZMO_LINE_DEPTH; else :5750-5780 -- `size` B32_LINE_3D_OVERLAY records
 *     (x0 + ox, y0 + oy, depth0, x1 + ox, y1 + oy, depth1), i = 0 .. size - 1 in that order; len < 0.001: nothing.
 *   B32_GIZMO_POINT: world_to_screen, `as i32`, one B32_PRIM_CIRCLE record of radius `size`.
 *   B32_GIZMO_TRIANGLE / _VIEW: three projections (any None: nothing), then one record of a library-internal kind (11: the third point's
 *     x and y travel as the bit patterns of z0 and z1; visible through the stage tap only -- b32_draw_prims and b32_draw_world keep
 *     answering B32_E_ARG for kind 11).  Pixels per :6302-6356: a STABLE sort of the three points by y, y2 == y0 nothing, rows
 *     y0.max(0) ..= y2.min(h - 1), second_half = y > y1 || y1 == y0, a row whose segment height is 0.0 skipped, columns
 *     (ax as i32).max(0) ..= (bx as i32).min(w - 1) after the swap, [r, g, b, 255], no depth test, no z write. */
typedef struct B32GizmoItem {
    float   p0[3], p1[3], p2[3];    /* world positions; lines use p0, p1; the point uses p0; triangles all three */
    int32_t size;                   /* THICK_LINE_DEPTH: thickness; POINT: radius; ignored otherwise */
    uint8_t r, g, b, blend;         /* Color{r, g, b, blend} */
    uint8_t kind;                   /* B32_GIZMO_* */
    uint8_t _pad[3];                /* must be 0 */
} B32GizmoItem;                     /* 48 bytes */
#define B32_GIZMO_LINE              0u  /* draw_3d_line             viewport_3d.rs:5687-5695, 5783-5882 (use_depth = false) */
#define B32_GIZMO_LINE_DEPTH        1u  /* draw_3d_line_depth       :5698-5706 (use_depth = true)                           */
#define B32_GIZMO_THICK_LINE_DEPTH  2u  /* draw_3d_thick_line_depth :5709-5781                                              */
#define B32_GIZMO_POINT             3u  /* draw_3d_point            :5958-5976                                              */
#define B32_GIZMO_TRIANGLE          4u  /* project_vertex :6239-6245 three times (cam.z < 0.1 -> None; math.rs project :117-136;
                                           `as i32`), then draw_filled_triangle_3d :6295-6357                                */
#define B32_GIZMO_TRIANGLE_VIEW     5u  /* the modeler's: project_vertex modeler/viewport.rs:4592-4607
                                           (world_to_screen_with_ortho_depth, takes `ortho`), then its fill :4663-4722        */
#define B32_GIZMO_MAX_THICKNESS    16   /* the reference only ever passes 3 */
/* Draws items[0..n) as the reference's calls one after another in array order, with b32_draw_world's contract: every pixel and byte
 * equal, enqueued on the context's stream with no host synchronisation, a deferred clear flushed first, only rows of the band written,
 * the z-buffer read (f32::MAX while it is not valid) and never written, `items` reusable on return, n == 0 a no-op.  `ortho` is read
 * by B32_GIZMO_TRIANGLE_VIEW only.
 * The whole batch is checked before anything is enqueued: an unknown kind, non-zero padding or B32_GIZMO_THICK_LINE_DEPTH with
 * size > B32_GIZMO_MAX_THICKNESS -> B32_E_ARG; a point with |size| > 32767 -> B32_E_UNSUPPORTED.  What the reference's i32 arithmetic
 * cannot carry is known only after projection; the item's record(s) become no-ops on the device and the item is counted `rejected`:
 * a line extent |x1-x0| or |y1-y0| >= 2^30; for kinds 2, 4 and 5 any cast coordinate of magnitude >= 2^30 (x0 + ox, y2 - y0, x2 - x0
 * overflow); a point whose centre reaches 2^30 (b32_draw_prims's circle rule).  An item for which the reference draws nothing -- both
 * ends behind the near plane, a None projection, a segment Cohen-Sutherland rejects or fails to converge on, len < 0.001, y2 == y0 -- is
 * counted `dropped`; every other item `drawn`. */
int b32_draw_gizmos(b32_ctx* ctx, const B32Camera* camera, const B32Ortho* ortho /* nullable; read by kind 5 only */,
                    const B32GizmoItem* items, uint32_t n);
/* Stage tap: the records b32_draw_gizmos would hand to the tile pass for a width x height framebuffer, in item order (one per item,
 * `size` for a thick line of thickness > 1; an item that draws nothing: a circle of radius -1), copied back (synchronous).
 * *n_records = how many there are; more than `cap`: B32_E_ARG and nothing is written. */
int b32_gizmo_project_batch(b32_ctx* ctx, const B32Camera* camera, const B32Ortho* ortho /* nullable */, const B32GizmoItem* items,
                            uint32_t n, uint32_t width, uint32_t height, B32Prim* out, uint32_t cap, uint32_t* n_records);
/* Gizmo items projected by this context so far (b32_draw_gizmos and the stage tap): drawn, dropped, rejected.  Synchronises the stream. */
int b32_gizmo_counts(b32_ctx* ctx, uint64_t* drawn, uint64_t* dropped, uint64_t* rejected);
/* The editor's draw_filled_octahedron (viewport_3d.rs:6223-6292) as 20 items in call order (host only, no context): the six corners
 * as f32 centre +- size (:6231-6236), the eight faces of :6257-6266 as B32_GIZMO_TRIANGLE, then the twelve edges of :6280-6291 as
 * B32_GIZMO_LINE in the edge colour (c as u16 * 3 / 4) as u8 (:6275-6279; RasterColor::new: blend Opaque).  The modeler's octahedron
 * (modeler/viewport.rs:4575-4660) is the same faces as B32_GIZMO_TRIANGLE_VIEW followed by its edges as B32_LINE_3D items of
 * b32_draw_world. */
int b32_octahedron_items(const float center[3], float size, const uint8_t rgbb[4], B32GizmoItem out[20]);
/* The modeler's selection overlays (modeler/viewport.rs:1782-2247), drawn from a slot's RESIDENT vertices: draw_selected_object_brackets
 * (:1782-1884), draw_mesh_selection_overlays (:1890-2105) and draw_box_selection_preview (:2108-2247) all start from the selected
 * object's posed positions, which after b32_scene_pose exist in the slot only.  One call makes, on the device, the B32Prim records of the
 * sections asked for -- in the bit order below, which is the reference's call order -- and hands them to the ordered tile pass of
 * b32_draw_prims without visiting the host.  Positions are the slot's as they are (posed or not); there is no placement.  The arithmetic
 * is the reference's, operation for operation (f32, no contraction, saturating `as i32`, a wrapping `as i32 + 1`); all colours are
 * RasterColor::new (blend Opaque):
 *   BRACKETS  min / max over all nv positions (f32::min / max: a NaN never wins), -= 4.0 / += 4.0, bracket_len = the smallest extent * 0.25,
 *             the 8 corners x 3 directions of :1842-1863 as 24 B32_LINE_3D records (0, 200, 230); nv == 0: nothing.
 *   EDGES     every half-edge of the topology in loop order (duplicates included) whose indices are < nv and whose ends project:
 *             B32_LINE_3D_ALPHA (80, 80, 80) alpha 191.
 *   DOTS      every vertex that projects: B32_PRIM_CIRCLE_ALPHA radius 3 (40, 40, 50) alpha 140.
 *   HOVER     (255, 200, 150): the vertex a circle of radius 5; the edge three B32_LINE_2D (as cast, + 1 on both x, + 1 on both y); the
 *             face the outline over its projected vertices when there are >= 3, plus [0] -> [2] when there are >= 4.
 *   SELECTED  (100, 180, 255): vertices a circle of radius 4 each; edges (pairs as given) the line, its + 1 x twin and a circle of radius
 *             3 at each end; polygons the outline with + 1 x twins and a circle of radius 4 at the projected centre -- the sum over the
 *             vertices with index < nv times 1.0 / n, n the number that PROJECTED (:2088); fewer than 3 projected: nothing.
 *   PREVIEW   (255, 220, 100), inclusive tests against (x0, y0)-(x1, y1) (a NaN fails): mode 0 a circle of radius 6 per vertex inside; mode 1
 *             the first half-edge of every normalised edge in loop order whose midpoint is inside, as the line and its + 1 x twin in that
 *             half-edge's orientation; mode 2 per polygon whose centre (sum over indices < nv times 1.0 / their count) projects inside and
 *             that has >= 3 projected vertices: the outline, then a circle of radius 4 at the centre.
 * The reference draws gizmos and the skeleton between the overlays and the preview, and the preview takes the camera and ortho of its own
 * viewport: a caller makes two calls.  wireframe_overlay on: leave out EDGES and DOTS (:1923).  An index out of range is never an error: it
 * behaves as get_pos(..) == None / mesh.faces.get(..) == None.
 * How many records there are, and where each lies, depends on the topology, nv, this struct and the selected list alone -- never on the
 * camera (b32_mesh_overlay_record_count); a call the reference does not make leaves a record that draws nothing (a circle of radius
 * -1).  A record whose extent or circle centre reaches 2^30 becomes such a no-op too, as in b32_draw_world; a NaN depth is stored as
 * 0x7FC00000. */
typedef struct B32MeshOverlay {
    uint32_t sections;                       /* B32_OVERLAY_* bits */
    uint32_t hover_vertex;                   /* 0xFFFFFFFF: none */
    uint32_t hover_edge_v0, hover_edge_v1;   /* both 0xFFFFFFFF: none */
    uint32_t hover_face;                     /* POLYGON index, 0xFFFFFFFF: none -- i.e. a masked B32HoverResult */
    uint32_t select_kind;                    /* 0 none, 1 vertices, 2 edges (pairs), 3 polygons */
    uint32_t n_selected;
    uint32_t preview_mode;                   /* 0 vertex, 1 edge, 2 face (SelectMode) */
    float    x0, y0, x1, y1;                 /* preview rectangle, framebuffer coordinates */
} B32MeshOverlay;                            /* 48 bytes */
#define B32_OVERLAY_BRACKETS 1u   /* draw_selected_object_brackets */
#define B32_OVERLAY_EDGES    2u   /* :1923-1935 */
#define B32_OVERLAY_DOTS     4u   /* :1937-1954 */
#define B32_OVERLAY_HOVER    8u   /* :1960-2020 */
#define B32_OVERLAY_SELECTED 16u  /* :2025-2104 */
#define B32_OVERLAY_PREVIEW  32u  /* draw_box_selection_preview */
/* Draws the sections with b32_draw_world's contract: enqueued on the context's stream with no host synchronisation, a deferred clear
 * flushed first, only rows of the band written, the z-buffer read (f32::MAX while it is not valid) and never written, `overlay` and
 * `selected` (n_selected indices, 2 * n_selected for pairs; copied) reusable on return.  `topology` may be NULL when no section reads
 * polygons (BRACKETS, DOTS, the hovered vertex / edge, selected vertices / edges, PREVIEW mode 0).
 * NULL context, camera, slot or overlay, an unknown section bit, select_kind > 3, preview_mode > 2, a section that walks polygons (EDGES, a
 * hovered face, selected polygons, PREVIEW modes 1 and 2) without a topology, n_selected > 0 with selected == NULL, a zero-size framebuffer,
 * a slot that does not hold its scene -> B32_E_ARG.  More than 2^31 - 1 records -> B32_E_UNSUPPORTED, before anything is enqueued. */
int b32_draw_mesh_overlay(b32_ctx* ctx, const B32Camera* camera, const B32Ortho* ortho /* nullable */, b32_scene* slot,
                          b32_topology* topology /* nullable, see above */, const B32MeshOverlay* overlay, const uint32_t* selected);
/* Stage tap: the records b32_draw_mesh_overlay would hand to the tile pass for a width x height framebuffer, copied back (synchronous).
 * *n_records = how many there are; more than `cap`: B32_E_ARG and nothing is written. */
int b32_mesh_overlay_project_batch(b32_ctx* ctx, const B32Camera* camera, const B32Ortho* ortho /* nullable */, b32_scene* slot,
                                   b32_topology* topology, const B32MeshOverlay* overlay, const uint32_t* selected, uint32_t width,
                                   uint32_t height, B32Prim* out, uint32_t cap, uint32_t* n_records);
/* How many records the call makes for a slot of nv vertices (host only): 24 (nv > 0) + nh + nv + hover (1, 3, n + (n >= 4)) + selected
 * (n_selected, 4 * n_selected, the sum of 2 * n + 1 over the listed polygons that exist) + preview (nv, 2 * distinct edges, nh + np), each
 * for the sections that are on.  The argument rules of b32_draw_mesh_overlay. */
int b32_mesh_overlay_record_count(const b32_topology* topology /* nullable */, uint32_t nv, const B32MeshOverlay* overlay,
                                  const uint32_t* selected, uint32_t* n);
/* The world editor's room overlays (editor/viewport_3d.rs:4273-4658, :4862-5362), drawn from a room's RESIDENT sector table: draw_viewport_3d
 * draws them out of hovered_vertex / hovered_edge / hovered_face, state.selection, state.multi_selection and the box-select preview, from
 * the sector heights, which after b32_room_update exist in the room only.  One call makes, on the device, the B32Prim records of the
 * sections asked for -- in the bit order below, which is the reference's call order -- and hands them to the ordered tile pass of
 * b32_draw_prims without visiting the host.  Only B32_LINE_2D, B32_PRIM_CIRCLE and B32_PRIM_THICK_LINE records are made.  The arithmetic is
 * the reference's, operation for operation (f32, no contraction, saturating `as i32`); all colours are RasterColor::new (blend Opaque);
 * projection is world_to_screen (math.rs:503-534), perspective only; draw_3d_line is B32_GIZMO_LINE.  Corners are the room hover's
 * (bx or bx + S, position[1] + heights[k], bz or bz + S) with the selectors listed there.
 *   VERTICES  (:4273-4316) the loop is over collect_room_vertices order (:6599-6661), i.e. ascending key 4 * rec + corner, and draws only
 *             vertices that are selected or hovered: n_vertices + 1 records.  A selected vertex is a circle (100, 255, 100) of radius 5 when
 *             its key is primary_vertex, else 4.  The hovered vertex, drawn only when the hover's winner is the vertex, is a circle
 *             (255, 200, 150) of radius 4 at its rank among the keys (coincident corners of neighbouring sectors project to one pixel: the
 *             later circle wins); when it is also selected its record draws nothing.  Without a hovered vertex the last record is the no-op.
 *   EDGES     (:4318-4402) one B32_PRIM_THICK_LINE per (rec, edge_idx) pair, thickness 3, (100, 255, 100), between corners edge_idx and
 *             (edge_idx + 1) % 4 of `heights`; either end None: nothing.
 *   HOVER     1 + 6 records.  Winner edge: the thick line of :4404-4478 in (255, 200, 100).  Winner face, and face_rec outside
 *             [skip_first, skip_first + skip_count): the draw_3d_line calls of :4493-4654 in (150, 200, 255) -- floor and ceiling six, in
 *             the order of :4513-4532, triangle 1 from `heights`, triangle 2 from get_heights_2(), split_direction from the room's material
 *             table (no table set: the record's own heights and B32_SPLIT_NWSE, the reference's defaults); a wall five.
 *   SELECTED  draw_selection (:4862-5247) in (255, 200, 80): the listed faces first, six slots each, the same lines as the hover (a wall's
 *             sixth slot draws nothing); then the listed edges, one draw_3d_line each (:5174-5236).  Selection::Sector (:5050-5173) is OUT
 *             OF SCOPE: it draws from a sector's floor and ceiling records at once and comes from the 2-D grid view; a host expresses it
 *             as B32_GIZMO_LINE items of b32_draw_gizmos.
 *   PREVIEW   (:5249-5362) in (100, 220, 255).  rect = min / max of (x0, x1) and (y0, y1) (f32::min / max); when neither extent is > 3.0
 *             the section has NO records.  Element i < n is record i, selected exactly as b32_room_box_select selects it, four slots: the
 *             outline 0-1, 1-2, 2-3, 3-0 from `heights` only, no diagonal.  The preview's own (x0, z0, x1, z1) of WallSouth and WallWest
 *             (:5307, :5309) is the reverse of every other site: corner k stands where corner k ^ 1 stands elsewhere and keeps heights[k], so
 *             a sloped south or west wall previews differently from how it is selected.  Element n + j is point j of points_xyz, three
 *             slots: the 64.0-unit crosses of :5341-5352, p - Vec3(size, 0, 0) to p + Vec3(size, 0, 0) etc. component by component.
 * Where a record lies depends on n, this struct and the lists alone -- never on the camera or the heights
 * (b32_room_overlay_record_count): a call the reference does not make leaves a record that draws nothing (a circle of radius -1); so does
 * a record whose extent or circle centre reaches 2^30, as in b32_draw_gizmos.  A rec >= n in a list or in `hover` behaves as
 * get_sector(..) == None.  Every circle, thick line and draw_3d_line the reference calls is added to b32_gizmo_counts' totals: drawn,
 * dropped (a None projection, a line clipped away) or rejected (2^30).
 * hover_source 1 reads the 48 bytes of the room's last b32_room_hover[_async] ON THE DEVICE, where a copy enqueued behind that call left
 * them: the host need not wait for the ticket; the winner rule (b32_room_hover_winner) runs on the device.  With hover_source 0 the
 * member `hover` is used, raw, all three loops. */
typedef struct B32RoomOverlay {
    uint32_t sections;                       /* B32_ROOM_OVERLAY_* bits, in the reference's call order */
    uint32_t hover_source;                   /* 0: the member `hover`; 1: the room's last b32_room_hover[_async], read on the device */
    B32RoomHover hover;                      /* raw, all three loops; the library applies the winner rule (:7283-7336) */
    uint32_t primary_vertex;                 /* key 4 * rec + corner of Selection::Vertex in state.selection, 0xFFFFFFFF none */
    uint32_t skip_first, skip_count;         /* the records state.selection.includes_face() covers (editor/state.rs:349-363) */
    uint32_t n_vertices, n_edges, n_faces, n_points;
    float    x0, y0, x1, y1;                 /* selection_rect_start / _end as stored */
} B32RoomOverlay;                            /* 100 bytes */
#define B32_ROOM_OVERLAY_VERTICES 1u  /* :4273-4316 */
#define B32_ROOM_OVERLAY_EDGES    2u  /* :4318-4402 selected edges, thick */
#define B32_ROOM_OVERLAY_HOVER    4u  /* :4404-4658 hovered edge (thick), hovered face */
#define B32_ROOM_OVERLAY_SELECTED 8u  /* :4862-5247 draw_selection: SectorFace and Edge */
#define B32_ROOM_OVERLAY_PREVIEW 16u  /* :5249-5362 box-select preview, the selection made on the device */
/* Draws the sections with b32_draw_mesh_overlay's contract: enqueued on the context's stream with no host synchronisation, a deferred
 * clear flushed first, only rows of the band written, the z-buffer never written, the struct and all four arrays copied before return:
 * sel_vertices n_vertices keys, strictly ascending; sel_edges n_edges pairs (rec, edge_idx); sel_faces n_faces recs; points_xyz
 * 3 * n_points floats, the room's object positions.
 * NULL context, camera, room or overlay, an unknown section bit, hover_source > 1, hover_source 1 before any hover of that room, an
 * edge_idx > 3 (in sel_edges, or in `hover` with hover_source 0), keys that are not strictly ascending, a count > 0 with a NULL list, a
 * zero-size framebuffer -> B32_E_ARG.  More than 2^31 - 1 records -> B32_E_UNSUPPORTED.  Nothing is enqueued on error. */
int b32_draw_room_overlay(b32_ctx* ctx, const B32Camera* camera, b32_room* room, const B32RoomOverlay* overlay, const uint32_t* sel_vertices,
                          const uint32_t* sel_edges, const uint32_t* sel_faces, const float* points_xyz);
/* Stage tap: the records b32_draw_room_overlay would hand to the tile pass for a width x height framebuffer, copied back (synchronous).
 * *n_records = how many there are; more than `cap`: B32_E_ARG and nothing is written. */
int b32_room_overlay_project_batch(b32_ctx* ctx, const B32Camera* camera, b32_room* room, const B32RoomOverlay* overlay,
                                   const uint32_t* sel_vertices, const uint32_t* sel_edges, const uint32_t* sel_faces, const float* points_xyz,
                                   uint32_t width, uint32_t height, B32Prim* out, uint32_t cap, uint32_t* n_records);
/* How many records the call makes (host only): (n_vertices + 1) + n_edges + 7 + (6 * n_faces + n_edges) + (4 * n + 3 * n_points when the
 * rectangle passes the gate), each for the sections that are on.  The rules of b32_draw_room_overlay for the struct and these two lists. */
int b32_room_overlay_record_count(const b32_room* room, const B32RoomOverlay* overlay, const uint32_t* sel_edges, const uint32_t* sel_faces,
                                  uint32_t* n);
/* The world editor's object overlays, drawn from RESIDENT asset parts: draw_asset_wireframe (editor/viewport_3d.rs:255-291; the placement
 * preview :4833-4845 and the drag preview :4847-4860) and asset.bounds() (asset/asset.rs:288-312) followed by draw_rotated_bounding_box
 * (viewport_3d.rs:7658-7697; the yellow box of a selected mesh object :4255-4268, the box of a CollisionShapeDef::FromMesh object
 * :4231-4237, and with a given min / max Collision::Box :4215-4224).  An asset is a run of parts in the call's part table, each a slot that
 * HOLDS the part's mesh and, for a wireframe, the b32_topology of its polygons; an item is one reference call.  One call makes, on the
 * device, the B32Prim records of all items in array order and hands them to the ordered tile pass of b32_draw_prims without visiting the
 * host.  Only B32_LINE_2D records are made.  Every expression is a separately rounded f32 operation in the reference's order.
 *   WIRE      owns the sum of nh over its VISIBLE parts, in part order then loop order: the topology's half-edges (v[i], v[(i + 1) % n]),
 *             which are the pairs of :271-273 for n = 0, 1, 2 as well.  Both ends are placed as
 *                 ((x * cos_f - z * sin_f) + wx, y + wy, (x * sin_f + z * cos_f) + wz)                       (:276-285)
 *             and the record is what b32_draw_world makes for a B32_LINE_2D item with B32_WORLD_CLIP_NEAR and alpha 255
 *             (draw_3d_line_clipped, draw.rs:12-67).  The positions are the slot's BODY vertices as they are (posed or patched); bone
 *             octahedra behind the body are neither drawn nor reduced.  A hidden part (B32_OBJECT_PART_HIDDEN: !part.visible) has no records.
 *             DEPARTURE: an index >= nv panics in the reference (verts[indices[i]]); here the record draws nothing and counts as dropped.
 *   BOX_MESH  owns 12 records.  min / max are the fold of asset.rs:291-304 over ALL the item's parts, hidden ones included: minima start at
 *             f32::MAX and maxima at f32::MIN (not at infinities: a mesh of +inf vertices has min f32::MAX), f32::min / f32::max ignore a
 *             NaN (only-NaN vertices give the box f32::MAX .. f32::MIN, which is drawn).  has_verts is false when every part is empty: then
 *             the 12 records draw nothing and one call counts as dropped.  The eight corners in the order of :7669-7678, placed by
 *             :7681-7685, the twelve edges in the order of :7688-7692, each what b32_draw_gizmos makes for a B32_GIZMO_LINE item
 *             (draw_3d_line: near clip, world_to_screen, clip_line_to_rect, cast).  The fold is cached per slot (b32_scene_bounds) and
 *             reduced again on the device only after the slot's vertices changed.
 *             DEPARTURE: Rust leaves the sign of min(-0.0, +0.0) to the operand order; here both zeros are one key and come back as +0.0.
 *             No record can tell (tests/test_object_overlay.py).
 *   BOX       the same 12 records from box_min / box_max as given (min > max is drawn as given); its part range is not read.
 * Where a record lies depends on the topologies' half-edge counts and the item kinds alone, never on the camera
 * (b32_object_overlay_record_count): a call the reference does not make leaves a record that draws nothing (a circle of radius -1); so does
 * a record whose extent reaches 2^30, as in b32_draw_world and b32_draw_gizmos.  Every draw_3d_line_clipped and draw_3d_line the reference
 * calls is added to b32_gizmo_counts' totals: drawn, dropped (a None projection, a line clipped away) or rejected (2^30). */
typedef struct B32ObjectPart {
    b32_scene* slot;                         /* holds the part's mesh (MeshPart::mesh) */
    b32_topology* topology;                  /* its polygons; nullable when the part is hidden or only boxes use it */
    uint32_t flags;                          /* B32_OBJECT_PART_* */
    uint32_t _pad;                           /* must be 0 */
} B32ObjectPart;                             /* 24 bytes */
#define B32_OBJECT_PART_HIDDEN 1u            /* !part.visible: no wireframe (:266); asset.bounds() still reads it (asset.rs:295) */
typedef struct B32ObjectItem {
    B32Placement place;                      /* ALWAYS applied, as in b32_pick_meshes: draw_asset_wireframe has no has_transform shortcut */
    uint32_t first_part, n_parts;            /* the asset's parts in the call's part table */
    float box_min[3], box_max[3];            /* B32_OBJECT_BOX only */
    uint8_t r, g, b, blend;                  /* RasterColor */
    uint8_t kind;                            /* B32_OBJECT_* */
    uint8_t _pad[3];                         /* must be 0 */
} B32ObjectItem;                             /* 60 bytes */
#define B32_OBJECT_WIRE      0u  /* draw_asset_wireframe, viewport_3d.rs:255-291 */
#define B32_OBJECT_BOX_MESH  1u  /* asset.bounds() (asset.rs:288-312) -> draw_rotated_bounding_box (:7658-7697) */
#define B32_OBJECT_BOX       2u  /* draw_rotated_bounding_box with the given min / max (Collision::Box, :4215-4224) */
/* Draws the items with b32_draw_world's contract: enqueued on the context's stream with no host synchronisation, a deferred clear flushed
 * first, only rows of the band written, the z-buffer never written, both arrays reusable on return; n_items == 0 is a no-op.
 * NULL context or camera, a NULL array with a non-zero count, a part range outside the table, a NULL slot or one that does not hold its
 * scene, a visible part of a WIRE item without a topology, an unknown kind or flag, non-zero padding, a zero-size framebuffer ->
 * B32_E_ARG.  More than 2^31 - 1 records -> B32_E_UNSUPPORTED.  Nothing is enqueued on error. */
int b32_draw_object_overlays(b32_ctx* ctx, const B32Camera* camera, const B32ObjectPart* parts, uint32_t n_parts, const B32ObjectItem* items,
                             uint32_t n_items);
/* Stage tap: the records b32_draw_object_overlays would hand to the tile pass for a width x height framebuffer, copied back (synchronous).
 * *n_records = how many there are; more than `cap`: B32_E_ARG and nothing is written. */
int b32_object_overlay_project_batch(b32_ctx* ctx, const B32Camera* camera, const B32ObjectPart* parts, uint32_t n_parts,
                                     const B32ObjectItem* items, uint32_t n_items, uint32_t width, uint32_t height, B32Prim* out, uint32_t cap,
                                     uint32_t* n_records);
/* How many records the call makes (host only): per WIRE item the sum of nh over its visible parts, per box 12.  The argument rules of
 * b32_draw_object_overlays. */
int b32_object_overlay_record_count(const B32ObjectPart* parts, uint32_t n_parts, const B32ObjectItem* items, uint32_t n_items, uint64_t* n);
/* asset.bounds() of ONE slot (NULL: the context's resident scene): the cached reduction BOX_MESH reads, for hosts that keep no copy of the
 * vertices (the modeler's draw_collision_wireframe, modeler/viewport.rs:4215 and :4333-4349; camera framing).  min / max as above (a zero
 * comes back as +0.0), *has_verts = the body has vertices; without vertices min is f32::MAX and max f32::MIN.  The reduction runs on the
 * device, once per change of the slot's vertices (b32_route_count 20 counts the launches); the call touches neither framebuffer nor
 * z-buffer, flushes no clear and settles no frame.  The asynchronous form performs no host synchronisation and delivers 32 bytes -- min[3],
 * max[3], uint32 has_verts, 4 bytes of padding -- through the tickets of b32_fb_download_async.  NULL context or result pointers, a slot
 * that does not hold its scene -> B32_E_ARG. */
int b32_scene_bounds(b32_ctx* ctx, b32_scene* slot, float mn[3], float mx[3], uint32_t* has_verts);
int b32_scene_bounds_async(b32_ctx* ctx, b32_scene* slot, void* out /* 32 bytes */, uint64_t* ticket);
/* The presenter's upscale (game/renderer.rs:179-214: Texture2D::from_rgba8 + FilterMode::Nearest + dest_size): destination pixel
 * (x, y) shows source texel floor((x + 0.5) * w / dst_w), floor((y + 0.5) * h / dst_h).  Writes dst_w*dst_h RGBA8 to host memory. */
int b32_present_nearest(b32_ctx* ctx, uint32_t dst_w, uint32_t dst_h, uint8_t* rgba_out);

/* ---- stage taps (parity tests only; not on the frame path) ---------------- */
/* fixed::project_fixed (fixed.rs:424-441) + float depth (render.rs:2331-2345) for n positions. */
int b32_project_fixed_batch(b32_ctx* ctx, const float* pos_xyz, uint32_t n,
                            const B32Camera* camera, uint32_t width, uint32_t height,
                            int32_t* sx, int32_t* sy, float* z);
/* Draw order of the last frame: face index of every surviving surface, in the order drawn
 * (opaque sorted, then transparent sorted; render.rs:2518-2569). `cap` entries max; returns count via n. */
int b32_last_draw_order(b32_ctx* ctx, uint32_t* face_idx, uint32_t cap, uint32_t* n);
/* What the last frame shaded with, before the fill quantises it: for every surviving surface, in ascending face index,
 * face_idx[i] = its face, shades[9 * i ..] = the nine floats the setup kernel stored for it (render.rs:1466-1483: the flat shade three
 * times, or the Gouraud shades of v1, v2, v3 in the surface's own vertex order, r g b each), colors[3 * i ..] = its three vertex colours
 * after fog (render.rs:2419-2442), r | g << 8 | b << 16, as the shade record holds them.  *n = how many surfaces there are, *n_shaded =
 * how many have shades: *n on a lit frame, 0 when shading is None (the colours are valid either way).  At most `cap` surfaces are
 * written; face_idx, shades and colors may each be NULL.  Copies what the frame's own kernels wrote and launches nothing.  For a finished
 * frame of ONE mesh that is still the context's resident scene (drop-in, resident, placed or posed): B32_E_ARG while a frame is
 * pending, after a merged batch, with a band set, or when the buffers do not belong to that mesh. */
int b32_last_surface_shading(b32_ctx* ctx, uint32_t* face_idx, float* shades, uint32_t* colors, uint32_t cap, uint32_t* n,
                             uint32_t* n_shaded);
/* IEEE-754 f32 self-test of the device arithmetic the pipeline relies on (no FMA contraction,
 * correctly rounded / and sqrt, denormals kept): evaluates op(a[i], b[i], c[i]) on the GPU.
 * op: 0 a*b+c (two roundings), 1 a/b, 2 sqrt(a), 3 (a+b)/c, 4 acos(a) as the lighting code computes it (render.rs:1049),
 * 5 / 6 the bits of `a as i32` / `a as u32` with Rust's semantics (NaN -> 0, saturating; fixed.rs:126, render.rs:1455-1458, 1618),
 * 7 Fixed32::mul_fixed (fixed.rs:161-165) on the operands' bit patterns,
 * 8 the wireframe tile kernel's three-instruction depth parameter against k / N (render.rs:784): a[i] = N, out[i] = how many
 *   k in [0, N] give different bits (the kernel uses it for N < 16384; the test runs every such N and expects zeros). */
int b32_selftest_f32(b32_ctx* ctx, int op, const float* a, const float* b, const float* c,
                     float* out, uint32_t n);

/* The numeric literals of the reference AS THE DEVICE CODE HOLDS THEM (a kernel writes them out): `count` named constants
 * (names[i] = the key in tests/golden/ref_constants.json, which tests/golden/pin_constants.py derives from the reference text;
 * bits[i] = the f32 bit pattern when is_f32[i], else the integer), the UNR_TABLE the projection kernel indexes (fixed.rs:20-31,
 * 257 bytes) and PS1_DITHER_MATRIX as dither_offset() returns it, index (y & 3) * 4 + (x & 3) (render.rs:1150-1155).
 * Any of the output pointers may be NULL; at most `cap` constants are written. */
int b32_device_constants(b32_ctx* ctx, const char** names, uint32_t* bits, uint8_t* is_f32, uint32_t cap, uint32_t* count,
                         uint8_t* unr_table257, int32_t* dither16);

/* Per-kernel device time of the last finished frame (HIP events on the ctx stream), for bench.py.
 * names[i] points at static strings; returns the number of entries written (<= cap).  While profiling is on (b32_set_profiling >= 1) the
 * projection kernel of the last b32_draw_world is timed too and reported as a further entry "world_project" (the call waits for it), and so
 * are the two kernels of the last b32_pick_meshes[_async], as "pick", and the kernels of the last b32_hover_mesh[_async], as "hover";
 * b32_set_profiling(ctx, 0) ends that. */
int b32_last_kernel_times(b32_ctx* ctx, const char** names, float* ms, uint32_t cap);
/* HIP-event instrumentation of the frames enqueued from now on: 0 = none (default for the async path),
 * 1 = events around the coverage kernel (the dominant one), 2 = events around every phase
 * (setup, sort, bin, cover, shade). Averages over the frames between two
 * b32_frame_finish calls (last 64 at most) are returned by b32_last_kernel_times / B32Timings. */
int b32_set_profiling(b32_ctx* ctx, int level);
/* Instrument only every `every`-th frame (default 1: each one).  An event pair around a kernel costs the stream a few microseconds
 * per frame (the kernels of consecutive frames no longer run back to back); bench.py samples every 8th frame of its timed region. */
int b32_set_profiling_stride(b32_ctx* ctx, uint32_t every);
/* Shader clock the fused fill kernel of the last finished frame really ran at (no reference counterpart; instrumentation): workgroup 0
 * reads the shader-cycle counter and the 100 MHz wall clock when it starts and when it runs out of tiles.  *ghz = 0 when that frame had
 * no such kernel; *fill_ms (nullable) = the wall-clock span the cycles were counted over.  bench.py prices VALU issue with it. */
int b32_last_shader_clock(const b32_ctx* ctx, float* ghz, float* fill_ms);
/* Test tap (no reference counterpart): *host_bound = the faces of the resident scene that their own blend mode / editor alpha or their
 * texture's blend mode can put in the transparent pass (render.rs:2403-2415), counted on the host at upload -- what decides whether a
 * frame of a moderate mesh can ever need a redraw; *device_last = the surfaces the setup kernel of the last finished frame really
 * classified as transparent.  device_last <= host_bound must hold for every frame. */
int b32_transparent_counts(const b32_ctx* ctx, uint32_t* host_bound, uint32_t* device_last);
/* Test tap (no reference counterpart): fault injection for the failure paths that cannot be provoked from outside.  what = 1: the NEXT
 * frame that hands its setup kernel over by the flag / join kernel pair loses its flag (it publishes another epoch) and its join waits 2 ms
 * instead of 2 s -- the "setup kernel never arrived" path: the fill draws nothing but the folded clear, b32_frame_finish returns
 * B32_E_HIP, the frames after it are drawn normally.  what = 2: the NEXT fused fill kernel does not publish that it has started, and the gate
 * of the pipelined frame behind it -- which orders its setup kernel after the frame set's last reader by that word -- waits 2 ms instead of
 * 2 s, gives up, goes on and raises the same error: reported once by b32_frame_finish, frames right.  Other bits: B32_E_ARG. */
int b32_debug_inject(b32_ctx* ctx, uint32_t what);
/* Two frames in flight (no reference counterpart; see B32_ROUTE_PIPELINE): when a frame is enqueued while an earlier one is still
 * pending, its setup kernel runs on a second, low-priority stream of the context beside the earlier frame's fill kernel, on a second
 * set of per-face buffers.  permille > 0 holds that setup kernel back so that it runs beside the fill's thinning second half rather than
 * beside its busy start (started together the two kernels only slow each other down), measured on the fill's tile cursor:
 *   1001 .. 2000: until (permille - 1000) / 1000 of the tiles BEHIND the workgroups' first round have been handed out (1150 was the default
 *                 through round 5);
 *   1 .. 1000   : until the last tile has been handed out and (permille - 1) / 1000 of the workgroups have found the queue empty;
 *   0 (default) : no hold on the cursor.  Since round 6 the setup kernel waits anyway -- for the ORDER of the frame sets -- until the fill in
 *                 front of it has started (Events::fill_started, k_gate), which keeps it off that fill's first microseconds; a hold on top
 *                 of that only costs (C3 0.1007-0.1012 against 0.1024-0.1053 ms per frame with 1150, C5 0.1645-0.1653 against 0.1663-0.1670).
 * Results are identical either way.  permille > 2000: B32_E_ARG. */
int b32_set_pipeline_gate(b32_ctx* ctx, uint32_t permille);
/* How far ahead of its fill a pipelined setup kernel runs (no reference counterpart; render.rs:2364-2547 is one sequential call):
 *   sets = 2: k_setup(i + 1) beside the fill of frame i -- the fill of frame i + 1 starts behind a cross-stream event that is
 *             signalled only about when the fill before it ends (10-20 us per frame with little on the GPU);
 *   sets = 3: k_setup(i + 2) beside the fill of frame i, on a third set of per-face buffers: the setup kernel a fill waits for ended
 *             a whole fill earlier and fills run back to back on the main stream.  Measured on C3 (round 4): the hole closes, but the two
 *             kernels then share every CU all the time and the frame is bound by their summed VALU work: 0.127 against 0.122 ms.
 *   sets = 0 (the library's choice, the default): two sets; three while the context draws a NARROW band (b32_set_band: at most a sixth of the
 *             frame's rows -- one rank of a frame sharded over six or more GPUs): that rank still transforms the whole mesh, its frame is
 *             bound by the setup kernel, and with three sets the setup kernels run back to back (240 rows of the 1 M-triangle frame: 0.040 ->
 *             0.034-0.035 ms per frame).  b32_set_band switches when the band crosses that width (everything in flight ends first).
 * Settles a pending frame first.  Results are identical either way.  Other values: B32_E_ARG. */
int b32_set_pipeline_depth(b32_ctx* ctx, uint32_t sets);
/* B32Timings.fragments (the reference's pixel-store count, render.rs:1671-1702) is instrumentation, not an output of
 * render_mesh_15.  on = 0 (default): not counted (B32Timings.fragments = 0 unless the textures force exact coverage); the fill
 * may then resolve opaque visibility without fetching the texel of every overdrawn fragment and without a global depth
 * sort (identical framebuffer, see b32_fill.hip).  on = 1: every fragment is evaluated and counted exactly (painter's mode). */
int b32_set_fragment_counting(b32_ctx* ctx, int on);

/* ---- multi-GPU: the exchange step of a band-sharded frame (BASELINE config C4) ------------------------------------------------------
 * No reference counterpart: the reference draws on one CPU thread; its presenter reads `fb.pixels` of ONE process
 * (game/renderer.rs:179-214), so with the frame sharded by rows (b32_set_band, one rank per GPU) every band must end up in the ROOT
 * rank's framebuffer.  Two transports:
 *
 * (1) Shared framebuffer.  The root exports its library-owned framebuffer; a band rank binds it AS ITS OWN framebuffer -- the fill
 *     kernel of a band rank only writes the rows of its band, so they land directly in the root's HBM (over xGMI between two GPUs):
 *     no copy, no gather launch.  What remains is ordering, carried by one epoch word per rank behind the pixels of the same allocation:
 *
 *         root, once:      b32_fb_new(root, w, h);  b32_band_export(root, &share);           -> hand `share` (96 bytes) to every rank
 *         rank r, once:    b32_band_import(ctx, &share, r)      (another process)   or   b32_band_attach(ctx, root, r)   (same process)
 *                          b32_set_band(ctx, y0_r, y1_r);       b32_scene_upload...(ctx, ...)
 *         rank r, frame n: [b32_band_acquire(ctx, n - 1, us)]   b32_fb_clear(ctx, ...); b32_render_scene_15_async(ctx, ...);
 *                          b32_band_publish(ctx, n)
 *         root,  frame n:  b32_set_band(root, y0_0, y1_0) once; b32_fb_clear; b32_render_scene_15_async(root, ...);
 *                          b32_band_wait(root, r, n, us) for every r;   ... present / b32_fb_download ...;   [b32_band_release(root, n)]
 *
 *     Everything is enqueued on the contexts' streams; no call blocks the host.  publish(n) takes effect behind every kernel the rank
 *     enqueued before it; wait(r, n) holds the ROOT's stream until rank r has published a frame number >= n (wrap-safe compare) or
 *     timeout_us has passed -- a timeout is counted in b32_band_status AND makes the waiting context's next b32_frame_finish return
 *     B32_E_BAND_TIMEOUT, never silent.  release / acquire are the same in the other
 *     direction (the root has consumed frame n: a rank may overwrite its rows); a host that presents every frame before the ranks
 *     start the next one (e.g. behind its own barrier) does not need them.  Frame numbers start at 1 (the words start at 0).
 *     b32_frame_finish on a band rank still reports that rank's errors and counters; triangles_drawn is the whole mesh's on every rank.
 *     A band rank must not call b32_fb_clear* / sky / present functions outside its band: those honour b32_set_band like the draw.
 *
 * (2) RCCL.  b32_gather_bands_rccl: every rank draws into its OWN framebuffer and the rows travel by ncclSend / ncclRecv (grouped, on the
 *     context's stream) to `root`.  `nccl_comm` is the caller's ncclComm_t; librccl.so is loaded on first use (B32_E_UNSUPPORTED when
 *     it is not there).  y0 / y1: the band of every rank, the same arrays on every rank.
 *
 * Status: transport (1) is exercised by real processes sharing ONE GPU (tests: test_band_ranks_share_one_gpu[*-ipc]) and by the C++
 * harness inside one process; peer mappings between two GPUs and transport (2) are compiled and argument-checked but have not run. */
typedef struct B32BandShare {
    unsigned char mem[64];      /* HIP IPC handle of the root's framebuffer allocation (the epoch words sit in its tail) */
    uint32_t width, height;     /* the root's framebuffer */
    uint32_t device;            /* the root's HIP device ordinal (informational) */
    uint32_t reserved;
    uint64_t sync_offset;       /* byte offset of the epoch words inside the allocation */
    uint64_t reserved2;
} B32BandShare;
int b32_band_export(b32_ctx* root, B32BandShare* out);                        /* root; its framebuffer must be library-owned (b32_fb_new / _resize) */
int b32_band_import(b32_ctx* ctx, const B32BandShare* share, uint32_t rank);  /* band rank 1..63 in ANOTHER process: map + bind the root's framebuffer */
int b32_band_attach(b32_ctx* ctx, b32_ctx* root, uint32_t rank);              /* the same inside one process (one process driving several contexts / GPUs) */
int b32_band_close(b32_ctx* ctx);                                             /* unmap / unbind (also done by b32_destroy) */
int b32_band_publish(b32_ctx* ctx, uint32_t frame_no);                        /* band rank: "my rows of frame_no are complete", in stream order */
int b32_band_wait(b32_ctx* root, uint32_t rank, uint32_t frame_no, uint32_t timeout_us);   /* root: hold the stream until rank published >= frame_no */
int b32_band_release(b32_ctx* root, uint32_t frame_no);                       /* root: "frame_no has been consumed", in stream order */
/* root: b32_band_wait for every rank 1 .. nranks-1 and (release_after != 0) b32_band_release(frame_no) behind them, as ONE launch */
int b32_band_wait_all(b32_ctx* root, uint32_t nranks, uint32_t frame_no, uint32_t timeout_us, int release_after);
int b32_band_acquire(b32_ctx* ctx, uint32_t frame_no, uint32_t timeout_us);   /* band rank: hold the stream until the root released >= frame_no */
/* Host-side view of the epoch words (a blocking 4-KB copy): epochs[64] (nullable) = last published frame per rank, *root_epoch
 * (nullable) = last released frame, *timeouts (nullable) = waits that gave up since the export. */
int b32_band_status(b32_ctx* ctx, uint32_t* epochs, uint32_t* root_epoch, uint32_t* timeouts);
int b32_gather_bands_rccl(b32_ctx* ctx, void* nccl_comm, int rank, int nranks, int root, const uint32_t* y0, const uint32_t* y1);
/* The communicator for transport (2) made with the very librccl the library loaded (a host that links RCCL itself may pass its own
 * ncclComm_t instead): b32_rccl_unique_id = ncclGetUniqueId on ONE rank (128 bytes, handed to the others by whatever channel the host
 * has), b32_rccl_comm_create = ncclCommInitRank on the context's device (collective: every rank calls it), _destroy = ncclCommDestroy.
 * B32_E_UNSUPPORTED when librccl.so cannot be loaded; B32_E_HIP + b32_last_hip_error = the ncclResult_t otherwise. */
int b32_rccl_unique_id(unsigned char* id128);
int b32_rccl_comm_create(b32_ctx* ctx, const unsigned char* id128, int rank, int nranks, void** nccl_comm);
int b32_rccl_comm_destroy(void* nccl_comm);
/* Test tap (no reference counterpart): b32_gather_bands_rccl in which the root additionally sends its OWN band to itself and receives it
 * at row self_dst_y0 of the same framebuffer (the rows must not overlap the band).  With a 1-rank communicator this executes the whole
 * RCCL leg -- library load, the resolved entry points, the byte datatype, stream order behind the frame's kernels -- on a single GPU. */
int b32_gather_bands_rccl_loopback(b32_ctx* ctx, void* nccl_comm, int rank, int nranks, int root, const uint32_t* y0, const uint32_t* y1,
                                   uint32_t self_dst_y0);

#ifdef __cplusplus
}
#endif
#endif /* B32RASTER_H */
