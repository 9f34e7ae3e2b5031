// rasterizer.hpp — C++ host-side mirror of the reference rasterizer interface, header-only over the C ABI.
//
// The reference is compiled (Rust) code and no Rust toolchain exists in this image, so the host side above
// include/b32raster.h is written in C++ with the reference's names, argument meaning and error behaviour:
//
//   reference (src/rasterizer/...)                         here
//   Framebuffer::{new, resize, clear}  render.rs:18-45     b32::Framebuffer::{Framebuffer, resize, clear}
//   fb.pixels / fb.width / fb.height   render.rs:10-15     fb.pixels() (downloads RGBA8) / fb.width / fb.height
//   render_mesh_15(fb, vertices, faces, textures, camera,  b32::render_mesh_15(fb, vertices, faces, textures, camera,
//                  settings, fog) -> RasterTimings                            settings, fog) -> RasterTimings
//                                      render.rs:2302-2310
//   panics (index OOB render.rs:2375, NaN key :2531)       b32::Error{code}
//
// The Rust shim a maintainer would add to the reference is shown in INTEGRATION.md; it binds the same C symbols.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "b32raster.h"

namespace b32 {

struct Error : std::runtime_error {
    int code;
    explicit Error(int c, const char* where) : std::runtime_error(std::string(where) + ": " + b32_strerror(c)), code(c) {}
};
inline void check(int rc, const char* where) { if (rc != B32_OK) throw Error(rc, where); }

// math.rs:9-13 / :90-94
struct Vec3 { float x = 0, y = 0, z = 0; };
struct Vec2 { float x = 0, y = 0; };

// types.rs:1380-1388, :1289-1294
enum class BlendMode : uint8_t { Opaque, Average, Add, Subtract, AddQuarter, Erase };
enum class ShadingMode : uint8_t { None, Flat, Gouraud };

// types.rs:721-726
struct Color {
    uint8_t r = 0, g = 0, b = 0; BlendMode blend = BlendMode::Opaque;
    static Color neutral() { return { 128, 128, 128, BlendMode::Opaque }; }       // Color::NEUTRAL types.rs:768
};

// types.rs:947-959
struct Vertex { Vec3 pos; Vec2 uv; Vec3 normal; Color color = Color::neutral(); };

// types.rs:984-1002 (+ constructors :1012-1036)
struct Face {
    size_t v0 = 0, v1 = 0, v2 = 0;
    std::optional<size_t> texture_id;
    bool black_transparent = true;
    BlendMode blend_mode = BlendMode::Opaque;
    uint8_t editor_alpha = 255;
    static Face with_texture(size_t a, size_t b, size_t c, size_t tex) { Face f; f.v0 = a; f.v1 = b; f.v2 = c; f.texture_id = tex; return f; }
};

// types.rs:532-539
struct Texture15 { size_t width = 0, height = 0; std::vector<uint16_t> pixels; BlendMode blend_mode = BlendMode::Opaque; };

// types.rs:1166-1176 — the 8-bit-colour path's texture: Color texels carry their own blend mode (Erase = transparent texel)
struct Texture { size_t width = 0, height = 0; std::vector<Color> pixels; BlendMode blend_mode = BlendMode::Opaque; };

// camera.rs:9-18 (basis vectors are inputs of the path)
struct Camera { Vec3 position; Vec3 basis_x{ 1, 0, 0 }, basis_y{ 0, 1, 0 }, basis_z{ 0, 0, 1 }; };

// types.rs:1297-1314
struct Light {
    uint32_t type = B32_LIGHT_DIRECTIONAL; Vec3 position, direction; float radius = 0, angle = 0;
    Color color{ 255, 255, 255, BlendMode::Opaque }; float intensity = 1.0f; bool enabled = true;
    // types.rs:1355-1369 (the direction is normalized at construction, math.rs:39-49)
    static Light spot(Vec3 position, Vec3 direction, float angle, float radius, float intensity) {
        Light l; l.type = B32_LIGHT_SPOT; l.position = position; l.angle = angle; l.radius = radius; l.intensity = intensity;
        const float len = std::sqrt(direction.x * direction.x + direction.y * direction.y + direction.z * direction.z);
        l.direction = len == 0.0f ? Vec3{ 0, 0, 0 } : Vec3{ direction.x / len, direction.y / len, direction.z / len };
        return l;
    }
};

// types.rs:1392-1428, defaults :1475-1495, game() :1455-1460
struct RasterSettings {
    bool affine_textures = true, use_zbuffer = true;
    ShadingMode shading = ShadingMode::Gouraud;
    bool backface_cull = true, backface_wireframe = true;
    std::vector<Light> lights;        // reference default: one directional (-1,-1,-1).normalize() * 0.7 — supplied by the caller
    float ambient = 0.3f;
    bool dithering = true, wireframe_overlay = false;
    std::optional<Vec3> ortho_projection;   // (zoom, center_x, center_y)
    bool use_rgb555 = true, use_fixed_point = true, xray_mode = false;
    static RasterSettings game() { RasterSettings s; s.backface_wireframe = false; return s; }
};

// types.rs:1499-1514
struct RasterTimings { float transform_ms = 0, fog_ms = 0, cull_ms = 0, sort_ms = 0, draw_ms = 0, wireframe_ms = 0; uint32_t triangles_drawn = 0; uint64_t fragments = 0; };

using Fog = std::optional<std::tuple<float, float, float, Color>>;   // render.rs:2309

// render.rs:10-45 — the pixels live in HBM; `pixels()` is the download the presenter performs (game/renderer.rs:179)
class Framebuffer {
public:
    size_t width = 0, height = 0;
    Framebuffer(size_t w, size_t h, int device = 0) {                       // Framebuffer::new, render.rs:18-25
        check(b32_create(device, &ctx_), "b32_create");
        check(b32_fb_new(ctx_, (uint32_t)w, (uint32_t)h), "Framebuffer::new"); width = w; height = h;
    }
    ~Framebuffer() { b32_destroy(ctx_); }
    Framebuffer(const Framebuffer&) = delete;
    Framebuffer& operator=(const Framebuffer&) = delete;
    void resize(size_t w, size_t h) { check(b32_fb_resize(ctx_, (uint32_t)w, (uint32_t)h), "Framebuffer::resize"); width = w; height = h; }
    void clear(Color c) { check(b32_fb_clear(ctx_, c.r, c.g, c.b, (uint8_t)c.blend), "Framebuffer::clear"); }
    std::vector<uint8_t> pixels() const { std::vector<uint8_t> p(width * height * 4); check(b32_fb_download(ctx_, p.data()), "fb.pixels"); return p; }
    void set_pixels(const std::vector<uint8_t>& p) { if (p.size() != width * height * 4) throw Error(B32_E_ARG, "set_pixels"); check(b32_fb_upload(ctx_, p.data()), "fb.pixels="); }
    // the line family, render.rs:684-872 (enqueued, no host synchronisation; several lines at once: draw_lines, in array order)
    void draw_line(int32_t x0, int32_t y0, int32_t x1, int32_t y1, Color c) { draw_one(B32_LINE_2D, x0, y0, 0.0f, x1, y1, 0.0f, c, 255); }
    void draw_line_alpha(int32_t x0, int32_t y0, int32_t x1, int32_t y1, Color c, uint8_t alpha) { draw_one(B32_LINE_2D_ALPHA, x0, y0, 0.0f, x1, y1, 0.0f, c, alpha); }
    void draw_line_3d(int32_t x0, int32_t y0, float z0, int32_t x1, int32_t y1, float z1, Color c) { draw_one(B32_LINE_3D, x0, y0, z0, x1, y1, z1, c, 255); }
    void draw_line_3d_overlay(int32_t x0, int32_t y0, float z0, int32_t x1, int32_t y1, float z1, Color c) { draw_one(B32_LINE_3D_OVERLAY, x0, y0, z0, x1, y1, z1, c, 255); }
    void draw_line_3d_alpha(int32_t x0, int32_t y0, float z0, int32_t x1, int32_t y1, float z1, Color c, uint8_t alpha) { draw_one(B32_LINE_3D_ALPHA, x0, y0, z0, x1, y1, z1, c, alpha); }
    void draw_lines(const std::vector<B32Line>& lines) { check(b32_draw_lines(ctx_, lines.data(), (uint32_t)lines.size()), "draw_lines"); }
    // the other drawing methods, render.rs:631-971 (enqueued; several at once, mixed with lines: draw_prims / PrimBatch, in array order)
    void draw_line_blended(int32_t x0, int32_t y0, int32_t x1, int32_t y1, Color c, BlendMode mode) { draw_prim(prim(B32_PRIM_LINE_BLENDED, x0, y0, x1, y1, c, 0, 255, mode)); }
    void draw_circle(int32_t cx, int32_t cy, int32_t radius, Color c) { draw_prim(prim(B32_PRIM_CIRCLE, cx, cy, 0, 0, c, radius)); }
    void draw_circle_alpha(int32_t cx, int32_t cy, int32_t radius, Color c, uint8_t alpha) { draw_prim(prim(B32_PRIM_CIRCLE_ALPHA, cx, cy, 0, 0, c, radius, alpha)); }
    void draw_thick_line(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t thickness, Color c) { draw_prim(prim(B32_PRIM_THICK_LINE, x0, y0, x1, y1, c, thickness)); }
    void draw_rect(int32_t x0, int32_t y0, int32_t x1, int32_t y1, Color c) { draw_prim(prim(B32_PRIM_RECT, x0, y0, x1, y1, c)); }
    void draw_filled_rect(int32_t x0, int32_t y0, int32_t x1, int32_t y1, Color c) { draw_prim(prim(B32_PRIM_FILLED_RECT, x0, y0, x1, y1, c)); }
    void draw_prims(const std::vector<B32Prim>& prims) { check(b32_draw_prims(ctx_, prims.data(), (uint32_t)prims.size()), "draw_prims"); }
    // draw_star_diamond, render.rs:206-237, for every star in order (enqueued: the records are made on the device and go through the pass)
    void draw_stars(const std::vector<B32Star>& stars, float size) { check(b32_draw_stars(ctx_, stars.data(), (uint32_t)stars.size(), size), "draw_stars"); }
    // one B32Prim record (kinds B32_LINE_* / B32_PRIM_*; z0 / z1 only for the 3-D line kinds)
    static B32Prim prim(uint8_t kind, int32_t x0, int32_t y0, int32_t x1, int32_t y1, Color c, int32_t size = 0, uint8_t alpha = 255,
                        BlendMode mode = BlendMode::Opaque, float z0 = 0.0f, float z1 = 0.0f) {
        return B32Prim{ x0, y0, x1, y1, z0, z1, size, c.r, c.g, c.b, (uint8_t)c.blend, kind, alpha, (uint8_t)mode, { 0, 0, 0, 0, 0 } };
    }
    // world-space overlays, rasterizer/draw.rs:12-135 and math.rs:503-652: projected on the device (enqueued; several at once: draw_world /
    // WorldBatch, in array order).  ortho: OrthoProjection as (zoom, center_x, center_y).
    void draw_world(const std::vector<B32WorldItem>& items, const Camera& cam, const std::optional<Vec3>& ortho = std::nullopt) {
        const B32Camera c = camera_of(cam);
        const B32Ortho o = ortho ? B32Ortho{ ortho->x, ortho->y, ortho->z } : B32Ortho{ 0, 0, 0 };
        check(b32_draw_world(ctx_, &c, ortho ? &o : nullptr, items.data(), (uint32_t)items.size()), "draw_world");
    }
    void draw_3d_line_clipped(const Camera& cam, Vec3 p0, Vec3 p1, Color c) { draw_world({ world_item(B32_LINE_2D, p0, p1, c, 0, 255, BlendMode::Opaque, B32_WORLD_CLIP_NEAR) }, cam); }
    void draw_floor_grid(const Camera& cam, float y, float spacing, float extent, Color grid, Color x_axis, Color z_axis) {
        const B32Camera c = camera_of(cam);
        const uint8_t g[4] = { grid.r, grid.g, grid.b, (uint8_t)grid.blend }, xa[4] = { x_axis.r, x_axis.g, x_axis.b, (uint8_t)x_axis.blend },
                      za[4] = { z_axis.r, z_axis.g, z_axis.b, (uint8_t)z_axis.blend };
        check(b32_draw_floor_grid(ctx_, &c, y, spacing, extent, g, xa, za), "draw_floor_grid");
    }
    struct WorldCounts { uint64_t drawn = 0, dropped = 0, rejected = 0; };
    WorldCounts world_counts() const { WorldCounts w; check(b32_world_counts(ctx_, &w.drawn, &w.dropped, &w.rejected), "world_counts"); return w; }
    // one B32WorldItem (kinds B32_LINE_* / B32_PRIM_* 0..8; the circle kinds use p0 only)
    static B32WorldItem world_item(uint8_t kind, Vec3 p0, Vec3 p1, Color c, int32_t size = 0, uint8_t alpha = 255, BlendMode mode = BlendMode::Opaque,
                                   uint8_t flags = 0) {
        return B32WorldItem{ { p0.x, p0.y, p0.z }, { p1.x, p1.y, p1.z }, size, c.r, c.g, c.b, (uint8_t)c.blend, kind, alpha, (uint8_t)mode, flags, { 0, 0, 0, 0 } };
    }
    // the world editor's overlay helpers, editor/viewport_3d.rs:5687-6357: projected on the device (enqueued; several at once: draw_gizmos /
    // GizmoBatch, in array order).  ortho is read by B32_GIZMO_TRIANGLE_VIEW only.
    void draw_gizmos(const std::vector<B32GizmoItem>& items, const Camera& cam, const std::optional<Vec3>& ortho = std::nullopt) {
        const B32Camera c = camera_of(cam);
        const B32Ortho o = ortho ? B32Ortho{ ortho->x, ortho->y, ortho->z } : B32Ortho{ 0, 0, 0 };
        check(b32_draw_gizmos(ctx_, &c, ortho ? &o : nullptr, items.data(), (uint32_t)items.size()), "draw_gizmos");
    }
    WorldCounts gizmo_counts() const { WorldCounts w; check(b32_gizmo_counts(ctx_, &w.drawn, &w.dropped, &w.rejected), "gizmo_counts"); return w; }
    // one B32GizmoItem (kinds B32_GIZMO_*)
    static B32GizmoItem gizmo_item(uint8_t kind, Vec3 p0, Vec3 p1, Vec3 p2, Color c, int32_t size = 0) {
        return B32GizmoItem{ { p0.x, p0.y, p0.z }, { p1.x, p1.y, p1.z }, { p2.x, p2.y, p2.z }, size, c.r, c.g, c.b, (uint8_t)c.blend, kind, { 0, 0, 0 } };
    }
    b32_ctx* ctx() const { return ctx_; }
private:
    static B32Camera camera_of(const Camera& c) {
        return { { c.position.x, c.position.y, c.position.z }, { c.basis_x.x, c.basis_x.y, c.basis_x.z }, { c.basis_y.x, c.basis_y.y, c.basis_y.z },
                 { c.basis_z.x, c.basis_z.y, c.basis_z.z } };
    }
    void draw_prim(const B32Prim& p) { check(b32_draw_prims(ctx_, &p, 1), "draw_prims"); }
    void draw_one(uint8_t kind, int32_t x0, int32_t y0, float z0, int32_t x1, int32_t y1, float z1, Color c, uint8_t alpha) {
        const B32Line l = { x0, y0, x1, y1, z0, z1, c.r, c.g, c.b, (uint8_t)c.blend, kind, alpha, { 0, 0 } };
        check(b32_draw_lines(ctx_, &l, 1), "draw_line");
    }
    b32_ctx* ctx_ = nullptr;
};

// Framebuffer's drawing methods recorded in call order; flush() draws them with ONE b32_draw_prims call (a dot per vertex costs one launch
// per frame, not one per circle).  set_pixel / set_pixel_alpha / set_pixel_blended: a 1x1 FILLED_RECT, a one-point LINE_2D_ALPHA, a
// one-point LINE_BLENDED.
class PrimBatch {
public:
    explicit PrimBatch(Framebuffer& fb) : fb_(fb) {}
    void draw_line(int32_t x0, int32_t y0, int32_t x1, int32_t y1, Color c) { add(B32_LINE_2D, x0, y0, x1, y1, c); }
    void draw_line_alpha(int32_t x0, int32_t y0, int32_t x1, int32_t y1, Color c, uint8_t alpha) { add(B32_LINE_2D_ALPHA, x0, y0, x1, y1, c, 0, alpha); }
    void draw_line_3d(int32_t x0, int32_t y0, float z0, int32_t x1, int32_t y1, float z1, Color c) { add(B32_LINE_3D, x0, y0, x1, y1, c, 0, 255, BlendMode::Opaque, z0, z1); }
    void draw_line_3d_overlay(int32_t x0, int32_t y0, float z0, int32_t x1, int32_t y1, float z1, Color c) { add(B32_LINE_3D_OVERLAY, x0, y0, x1, y1, c, 0, 255, BlendMode::Opaque, z0, z1); }
    void draw_line_3d_alpha(int32_t x0, int32_t y0, float z0, int32_t x1, int32_t y1, float z1, Color c, uint8_t alpha) { add(B32_LINE_3D_ALPHA, x0, y0, x1, y1, c, 0, alpha, BlendMode::Opaque, z0, z1); }
    void draw_line_blended(int32_t x0, int32_t y0, int32_t x1, int32_t y1, Color c, BlendMode mode) { add(B32_PRIM_LINE_BLENDED, x0, y0, x1, y1, c, 0, 255, mode); }
    void draw_circle(int32_t cx, int32_t cy, int32_t radius, Color c) { add(B32_PRIM_CIRCLE, cx, cy, 0, 0, c, radius); }
    void draw_circle_alpha(int32_t cx, int32_t cy, int32_t radius, Color c, uint8_t alpha) { add(B32_PRIM_CIRCLE_ALPHA, cx, cy, 0, 0, c, radius, alpha); }
    void draw_thick_line(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t thickness, Color c) { add(B32_PRIM_THICK_LINE, x0, y0, x1, y1, c, thickness); }
    void draw_rect(int32_t x0, int32_t y0, int32_t x1, int32_t y1, Color c) { add(B32_PRIM_RECT, x0, y0, x1, y1, c); }
    void draw_filled_rect(int32_t x0, int32_t y0, int32_t x1, int32_t y1, Color c) { add(B32_PRIM_FILLED_RECT, x0, y0, x1, y1, c); }
    void set_pixel(int32_t x, int32_t y, Color c) { add(B32_PRIM_FILLED_RECT, x, y, x, y, c); }
    void set_pixel_alpha(int32_t x, int32_t y, Color c, uint8_t alpha) { add(B32_LINE_2D_ALPHA, x, y, x, y, c, 0, alpha); }
    void set_pixel_blended(int32_t x, int32_t y, Color c, BlendMode mode) { add(B32_PRIM_LINE_BLENDED, x, y, x, y, c, 0, 255, mode); }
    size_t size() const { return recs_.size(); }
    void flush() { fb_.draw_prims(recs_); recs_.clear(); }
private:
    template <typename... A>
    void add(uint8_t kind, A... args) { recs_.push_back(Framebuffer::prim(kind, args...)); }
    Framebuffer& fb_;
    std::vector<B32Prim> recs_;
};

// World-space overlay calls recorded in call order; flush(camera, ortho) projects and draws them with ONE b32_draw_world call.
class WorldBatch {
public:
    explicit WorldBatch(Framebuffer& fb) : fb_(fb) {}
    void line_clipped(Vec3 p0, Vec3 p1, Color c) { add(B32_LINE_2D, p0, p1, c, 0, 255, BlendMode::Opaque, B32_WORLD_CLIP_NEAR); }       // draw_3d_line_clipped
    void line_clipped_3d(Vec3 p0, Vec3 p1, Color c) { add(B32_LINE_3D, p0, p1, c, 0, 255, BlendMode::Opaque, B32_WORLD_CLIP_NEAR); }    // editor/viewport_3d.rs:5783-5840
    void line(Vec3 p0, Vec3 p1, Color c) { add(B32_LINE_2D, p0, p1, c); }
    void line_alpha(Vec3 p0, Vec3 p1, Color c, uint8_t alpha) { add(B32_LINE_2D_ALPHA, p0, p1, c, 0, alpha); }
    void line_3d(Vec3 p0, Vec3 p1, Color c) { add(B32_LINE_3D, p0, p1, c); }
    void line_3d_overlay(Vec3 p0, Vec3 p1, Color c) { add(B32_LINE_3D_OVERLAY, p0, p1, c); }
    void line_3d_alpha(Vec3 p0, Vec3 p1, Color c, uint8_t alpha) { add(B32_LINE_3D_ALPHA, p0, p1, c, 0, alpha); }
    void line_blended(Vec3 p0, Vec3 p1, Color c, BlendMode mode) { add(B32_PRIM_LINE_BLENDED, p0, p1, c, 0, 255, mode); }
    void thick_line(Vec3 p0, Vec3 p1, int32_t thickness, Color c) { add(B32_PRIM_THICK_LINE, p0, p1, c, thickness); }
    void circle(Vec3 p, int32_t radius, Color c) { add(B32_PRIM_CIRCLE, p, Vec3{ 0, 0, 0 }, c, radius); }
    void circle_alpha(Vec3 p, int32_t radius, Color c, uint8_t alpha) { add(B32_PRIM_CIRCLE_ALPHA, p, Vec3{ 0, 0, 0 }, c, radius, alpha); }
    size_t size() const { return items_.size(); }
    void flush(const Camera& cam, const std::optional<Vec3>& ortho = std::nullopt) { fb_.draw_world(items_, cam, ortho); items_.clear(); }
private:
    template <typename... A>
    void add(uint8_t kind, A... args) { items_.push_back(Framebuffer::world_item(kind, args...)); }
    Framebuffer& fb_;
    std::vector<B32WorldItem> items_;
};

// The editor's overlay helpers recorded in call order; flush(camera, ortho) projects and draws them with ONE b32_draw_gizmos call.
class GizmoBatch {
public:
    explicit GizmoBatch(Framebuffer& fb) : fb_(fb) {}
    void line(Vec3 p0, Vec3 p1, Color c) { add(B32_GIZMO_LINE, p0, p1, Vec3{ 0, 0, 0 }, c); }                                        // draw_3d_line
    void line_depth(Vec3 p0, Vec3 p1, Color c) { add(B32_GIZMO_LINE_DEPTH, p0, p1, Vec3{ 0, 0, 0 }, c); }                            // draw_3d_line_depth
    void thick_line_depth(Vec3 p0, Vec3 p1, Color c, int32_t thickness) { add(B32_GIZMO_THICK_LINE_DEPTH, p0, p1, Vec3{ 0, 0, 0 }, c, thickness); }
    void point(Vec3 p, int32_t radius, Color c) { add(B32_GIZMO_POINT, p, Vec3{ 0, 0, 0 }, Vec3{ 0, 0, 0 }, c, radius); }           // draw_3d_point
    void triangle(Vec3 p0, Vec3 p1, Vec3 p2, Color c) { add(B32_GIZMO_TRIANGLE, p0, p1, p2, c); }                                    // the editor's project_vertex + fill
    void triangle_view(Vec3 p0, Vec3 p1, Vec3 p2, Color c) { add(B32_GIZMO_TRIANGLE_VIEW, p0, p1, p2, c); }                          // the modeler's
    void octahedron(Vec3 center, float size, Color c) {                                                                              // draw_filled_octahedron
        const float ctr[3] = { center.x, center.y, center.z };
        const uint8_t rgbb[4] = { c.r, c.g, c.b, (uint8_t)c.blend };
        B32GizmoItem out[20];
        check(b32_octahedron_items(ctr, size, rgbb, out), "octahedron_items");
        items_.insert(items_.end(), out, out + 20);
    }
    size_t size() const { return items_.size(); }
    const std::vector<B32GizmoItem>& items() const { return items_; }
    void flush(const Camera& cam, const std::optional<Vec3>& ortho = std::nullopt) { fb_.draw_gizmos(items_, cam, ortho); items_.clear(); }
private:
    template <typename... A>
    void add(uint8_t kind, A... args) { items_.push_back(Framebuffer::gizmo_item(kind, args...)); }
    Framebuffer& fb_;
    std::vector<B32GizmoItem> items_;
};
inline void draw_gizmos(Framebuffer& fb, const std::vector<B32GizmoItem>& items, const Camera& cam, const std::optional<Vec3>& ortho = std::nullopt) {
    fb.draw_gizmos(items, cam, ortho);
}

namespace detail {
inline B32Vertex pack(const Vertex& v) {
    return { { v.pos.x, v.pos.y, v.pos.z }, { v.uv.x, v.uv.y }, { v.normal.x, v.normal.y, v.normal.z }, v.color.r, v.color.g, v.color.b, (uint8_t)v.color.blend };
}
inline B32Face pack(const Face& f) {
    // usize indices beyond u32 can never be valid vertex indices: map them to an out-of-range value (=> B32_E_INDEX)
    auto ix = [](size_t i) { return i > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)i; };
    const uint32_t tex = f.texture_id ? (*f.texture_id >= 0xFFFFFFFFull ? 0xFFFFFFFEu : (uint32_t)*f.texture_id) : B32_NO_TEXTURE;
    return { { ix(f.v0), ix(f.v1), ix(f.v2) }, tex, (uint8_t)f.black_transparent, (uint8_t)f.blend_mode, f.editor_alpha, 0 };
}
// Camera (camera.rs:9-18) -> B32Camera: position and the three basis vectors (rotation_x / rotation_y only feed Camera::update_basis)
inline B32Camera pack(const Camera& c) {
    return { { c.position.x, c.position.y, c.position.z }, { c.basis_x.x, c.basis_x.y, c.basis_x.z },
             { c.basis_y.x, c.basis_y.y, c.basis_y.z }, { c.basis_z.x, c.basis_z.y, c.basis_z.z } };
}
// Light (types.rs:1297-1314): LightType::Directional{direction} / Point{position, radius} / Spot{position, direction, angle, radius}
// flattened; the fields a kind does not have stay zero
inline B32Light pack(const Light& x) {
    return { x.type, { x.position.x, x.position.y, x.position.z }, { x.direction.x, x.direction.y, x.direction.z }, x.radius, x.angle,
             x.intensity, x.color.r, x.color.g, x.color.b, (uint8_t)x.enabled };
}
// RasterSettings (types.rs:1392-1428) -> B32Settings; `lights` must outlive the call (the struct points into it).
// ShadingMode None / Flat / Gouraud = 0 / 1 / 2 (types.rs:1289-1293); Option<OrthoProjection> -> has_ortho + three floats (types.rs:1432-1438);
// low_resolution and stretch_to_fill are presentation-only and not part of the C struct.
inline B32Settings pack(const RasterSettings& settings, const std::vector<B32Light>& lights) {
    B32Settings s{};
    s.affine_textures = settings.affine_textures; s.use_zbuffer = settings.use_zbuffer; s.shading = (uint8_t)settings.shading;
    s.backface_cull = settings.backface_cull; s.backface_wireframe = settings.backface_wireframe; s.dithering = settings.dithering;
    s.wireframe_overlay = settings.wireframe_overlay; s.use_rgb555 = settings.use_rgb555; s.use_fixed_point = settings.use_fixed_point;
    s.xray_mode = settings.xray_mode; s.has_ortho = settings.ortho_projection.has_value(); s.ambient = settings.ambient;
    if (settings.ortho_projection) { s.ortho_zoom = settings.ortho_projection->x; s.ortho_center_x = settings.ortho_projection->y; s.ortho_center_y = settings.ortho_projection->z; }
    s.n_lights = (uint32_t)lights.size(); s.lights = lights.empty() ? nullptr : lights.data();
    return s;
}
inline std::vector<B32Light> pack(const std::vector<Light>& lights) {
    std::vector<B32Light> l; l.reserve(lights.size());
    for (const auto& x : lights) l.push_back(pack(x));
    return l;
}
// fog: Option<(f32, f32, f32, Color)> (render.rs:2309) -> nullable B32Fog*
inline bool pack(const Fog& fog, B32Fog& out) {
    if (!fog) return false;
    const auto& [st, fo, cu, col] = *fog;
    out = { st, fo, cu, col.r, col.g, col.b, (uint8_t)col.blend };
    return true;
}
}  // namespace detail

// render.rs:2302-2310
inline RasterTimings render_mesh_15(Framebuffer& fb, const std::vector<Vertex>& vertices, const std::vector<Face>& faces,
                                    const std::vector<Texture15>& textures, const Camera& camera, const RasterSettings& settings,
                                    const Fog& fog = std::nullopt) {
    std::vector<B32Vertex> v; v.reserve(vertices.size());
    for (const auto& x : vertices) v.push_back(detail::pack(x));
    std::vector<B32Face> f; f.reserve(faces.size());
    for (const auto& x : faces) f.push_back(detail::pack(x));
    std::vector<B32Texture15> t; t.reserve(textures.size());
    for (const auto& x : textures)
        t.push_back({ (uint32_t)x.width, (uint32_t)x.height, (uint32_t)x.blend_mode, 0, x.pixels.size() >= x.width * x.height ? x.pixels.data() : nullptr });
    const std::vector<B32Light> l = detail::pack(settings.lights);
    const B32Camera c = detail::pack(camera);
    const B32Settings s = detail::pack(settings, l);
    B32Fog fg{};
    const B32Fog* fgp = detail::pack(fog, fg) ? &fg : nullptr;
    B32Timings tm{};
    check(b32_render_mesh_15(fb.ctx(), v.data(), (uint32_t)v.size(), f.data(), (uint32_t)f.size(), t.data(), (uint32_t)t.size(), &c, &s, fgp, &tm),
          "render_mesh_15");
    return { tm.transform_ms, tm.fog_ms, tm.cull_ms, tm.sort_ms, tm.draw_ms, tm.wireframe_ms, tm.triangles_drawn, tm.fragments };
}

// render.rs:1971-1978 — the path taken when settings.use_rgb555 is false (scene.rs:163-169); no fog parameter
inline RasterTimings render_mesh(Framebuffer& fb, const std::vector<Vertex>& vertices, const std::vector<Face>& faces,
                                 const std::vector<Texture>& textures, const Camera& camera, const RasterSettings& settings) {
    std::vector<B32Vertex> v; v.reserve(vertices.size());
    for (const auto& x : vertices) v.push_back(detail::pack(x));
    std::vector<B32Face> f; f.reserve(faces.size());
    for (const auto& x : faces) f.push_back(detail::pack(x));
    static_assert(sizeof(Color) == 4, "Color packs as r,g,b,blend bytes");
    std::vector<B32Texture> t; t.reserve(textures.size());
    for (const auto& x : textures)
        t.push_back({ (uint32_t)x.width, (uint32_t)x.height, (uint32_t)x.blend_mode, 0,
                      x.pixels.size() >= x.width * x.height && !x.pixels.empty() ? reinterpret_cast<const uint8_t*>(x.pixels.data()) : nullptr });
    const std::vector<B32Light> l = detail::pack(settings.lights);
    const B32Camera c = detail::pack(camera);
    const B32Settings s = detail::pack(settings, l);
    B32Timings tm{};
    check(b32_render_mesh(fb.ctx(), v.data(), (uint32_t)v.size(), f.data(), (uint32_t)f.size(), t.data(), (uint32_t)t.size(), &c, &s, &tm), "render_mesh");
    return { tm.transform_ms, tm.fog_ms, tm.cull_ms, tm.sort_ms, tm.draw_ms, tm.wireframe_ms, tm.triangles_drawn, tm.fragments };
}

// A mesh kept resident in HBM: uploaded once into a scene slot of the framebuffer's context, drawn many times.
class ResidentMesh {
public:
    ResidentMesh(Framebuffer& fb, const std::vector<Vertex>& vertices, const std::vector<Face>& faces, const std::vector<Texture15>& textures) : ctx_(fb.ctx()) {
        std::vector<B32Vertex> v; v.reserve(vertices.size());
        for (const auto& x : vertices) v.push_back(detail::pack(x));
        std::vector<B32Face> f; f.reserve(faces.size());
        for (const auto& x : faces) f.push_back(detail::pack(x));
        std::vector<B32Texture15> t; t.reserve(textures.size());
        for (const auto& x : textures)
            t.push_back({ (uint32_t)x.width, (uint32_t)x.height, (uint32_t)x.blend_mode, 0, x.pixels.size() >= x.width * x.height ? x.pixels.data() : nullptr });
        // The context keeps whatever scene it holds: its scene moves into the fresh slot, the mesh is uploaded into the (now empty)
        // context, and a second exchange leaves the mesh in the slot and the context's own scene where it was -- also when the upload
        // throws (render_scene-style calls and ResidentMesh can then share one Framebuffer).
        check(b32_scene_create(ctx_, &slot_), "scene_create");
        check(b32_scene_swap(ctx_, slot_), "scene_swap");            // context's scene -> slot, context empty
        const int rc = b32_scene_upload(ctx_, v.data(), (uint32_t)v.size(), f.data(), (uint32_t)f.size(), t.data(), (uint32_t)t.size());
        const int rc2 = b32_scene_swap(ctx_, slot_);                 // mesh -> slot, context's scene back
        if (rc2) {
            // the exchange back failed (a deferred error of an earlier frame surfaced in it): the slot still holds the CONTEXT's own scene
            // and must not be destroyed with it -- one more attempt (the deferred error has been consumed), then leave the slot alive
            // (leaked rather than the caller's scene freed) and report
            const int rc3 = b32_scene_swap(ctx_, slot_);
            if (rc3 == B32_OK) { b32_scene_destroy(ctx_, slot_); slot_ = nullptr; }
            else slot_ = nullptr;
            check(rc2, "scene_swap");
        }
        if (rc) { b32_scene_destroy(ctx_, slot_); slot_ = nullptr; check(rc, "scene_upload"); }
    }
    ~ResidentMesh() { if (slot_) b32_scene_destroy(ctx_, slot_); }
    ResidentMesh(const ResidentMesh&) = delete;
    ResidentMesh& operator=(const ResidentMesh&) = delete;
    b32_scene* slot() const { return slot_; }
    // Bones (b32_scene_set_rig / b32_scene_pose): the vertices as they are now become the rest pose, bone_of_vertex has one resolved bone
    // index per vertex (B32_BONE_NONE: none); pose() enqueues one pass from the rest pose with this bone table (empty: the rest vertices
    // come back); read_vertices() is the blocking read-back of what the slot holds now.  Defined below, behind Bone.
    void set_rig(const std::vector<uint16_t>& bone_of_vertex) { check(b32_scene_set_rig(ctx_, slot_, bone_of_vertex.data()), "scene_set_rig"); }
    inline void pose(const std::vector<struct Bone>& bones);
    // The bone octahedra (b32_scene_build_skeleton): one kernel replaces the mesh's tail with 6 vertices and 8 faces per drawn bone
    // (skeleton_to_triangles), the creation preview last; an empty skeleton without a preview removes it.  The tail is drawn with the
    // mesh and never hovered, selected, picked, skinned or overlaid.  Defined below, behind SkelBone.
    inline void build_skeleton(const std::vector<struct SkelBone>& bones, const B32SkeletonStyle& style);
    // Mirror editing (b32_scene_build_mirror): one kernel replaces THIS mesh's geometry with the mesh the modeler assembles from `src`'s
    // body while MirrorSettings is enabled -- the range's twins behind its vertices, each of its faces followed by its twin.  This mesh's
    // textures stay, its rig and tail go (build_skeleton afterwards); src is read only and stays what pose, patch, hover and the overlays
    // address.  Defined below, behind Mirror.
    inline void build_mirror(const ResidentMesh& src, const struct Mirror& mirror);
    std::vector<B32Vertex> read_vertices(uint32_t first, uint32_t count) const {
        std::vector<B32Vertex> out(count);
        check(b32_scene_read_vertices(ctx_, slot_, first, count, out.data()), "scene_read_vertices");
        return out;
    }
    std::vector<B32Face> read_faces(uint32_t first, uint32_t count) const {
        std::vector<B32Face> out(count);
        check(b32_scene_read_faces(ctx_, slot_, first, count, out.data()), "scene_read_faces");
        return out;
    }
    // Asset::bounds of the body's vertices as they are on the device now (b32_scene_bounds, blocking): the cached reduction the object
    // overlays' B32_OBJECT_BOX_MESH reads, reduced again only after the vertices changed.  false: no vertices (min f32::MAX, max f32::MIN).
    bool bounds(Vec3& min, Vec3& max) const {
        float mn[3], mx[3]; uint32_t has_verts = 0;
        check(b32_scene_bounds(ctx_, slot_, mn, mx, &has_verts), "scene_bounds");
        min = { mn[0], mn[1], mn[2] }; max = { mx[0], mx[1], mx[2] };
        return has_verts != 0;
    }
    // In-place edits (b32_scene_patch_*): the mesh stays resident, with its rig, pose and tail, and only the edited elements travel.
    // Records carry strictly ascending indices below the body's count; on a rigged mesh vertex records are in rest space.  A rectangle's
    // rows are `stride` elements apart in the caller's array.  Nothing blocks, except that the first face patch after an upload fetches
    // the faces once.  read_texels() is the blocking read-back of one texture's expanded texels (width * height of them).
    void patch_vertices(const std::vector<B32VertexPatch>& recs) { check(b32_scene_patch_vertices(ctx_, slot_, recs.data(), (uint32_t)recs.size()), "scene_patch_vertices"); }
    void patch_faces(const std::vector<B32FacePatch>& recs) { check(b32_scene_patch_faces(ctx_, slot_, recs.data(), (uint32_t)recs.size()), "scene_patch_faces"); }
    void patch_texels(uint32_t tex, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const uint16_t* texels, uint32_t stride) {
        check(b32_scene_patch_texels(ctx_, slot_, tex, x, y, w, h, texels, stride), "scene_patch_texels");
    }
    void patch_indexed(uint32_t tex, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const uint8_t* indices, uint32_t stride, const std::vector<uint16_t>& clut) {
        check(b32_scene_patch_indexed(ctx_, slot_, tex, x, y, w, h, indices, stride, clut.data(), (uint32_t)clut.size()), "scene_patch_indexed");
    }
    std::vector<uint16_t> read_texels(uint32_t tex, uint32_t width, uint32_t height) const {
        std::vector<uint16_t> out((size_t)width * height);
        check(b32_scene_read_texels(ctx_, slot_, tex, out.data()), "scene_read_texels");
        return out;
    }
private:
    b32_ctx* ctx_ = nullptr;
    b32_scene* slot_ = nullptr;
};

// One frame of scene::render_scene (scene.rs:158-261): one camera, base settings and light list; per mesh the room's ambient and fog and
// the part's backface culling.  The meshes are drawn as merged runs where their draws commute (b32_frame_begin / _add_scene / _end).
// Placement: facing and world offset of one placed object (render_asset_parts, scene.rs:112-159).  from_facing takes cos / sin on the host
// and decides has_transform as scene.rs:125 does; without a transform the reference draws the local vertices as they are, so the draw gets
// no placement at all.  A mesh may appear in a frame any number of times, each time with its own placement.
struct Placement {
    float cos_f = 1.0f, sin_f = 0.0f; Vec3 world_pos; bool has_transform = true;
    static Placement from_facing(float facing, Vec3 world_pos) {
        Placement p;
        p.cos_f = std::cos(facing); p.sin_f = std::sin(facing); p.world_pos = world_pos;
        p.has_transform = std::fabs(facing) > 0.0001f || std::fabs(world_pos.x) > 0.0001f || std::fabs(world_pos.y) > 0.0001f || std::fabs(world_pos.z) > 0.0001f;
        return p;
    }
};
// the host restatement of the same arithmetic (scene.rs:140-156): separately rounded f32 operations in the reference's order
// (compile with -ffp-contract=off where the compiler would fuse)
inline Vertex place_vertex(const Vertex& v, const Placement& p) {
    if (!p.has_transform) return v;
    Vertex o = v;
    const float rx = v.pos.x * p.cos_f - v.pos.z * p.sin_f, rz = v.pos.x * p.sin_f + v.pos.z * p.cos_f;
    o.pos = { rx + p.world_pos.x, v.pos.y + p.world_pos.y, rz + p.world_pos.z };
    o.normal = { v.normal.x * p.cos_f - v.normal.z * p.sin_f, v.normal.y, v.normal.x * p.sin_f + v.normal.z * p.cos_f };
    return o;
}
// Bone: get_bone_world_transform(i) (modeler/state.rs:2585-2614) as the device takes it.  from_euler takes to_radians as x * (PI / 180),
// cos / sin on the host, and decides `rotate` as rotate_by_euler's early return does (state.rs:31: both |rot.x| and |rot.z| < 0.001 degrees
// hand the vector back as it is).
struct Bone {
    Vec3 pos; float cos_x = 1.0f, sin_x = 0.0f, cos_z = 1.0f, sin_z = 0.0f; bool rotate = false;
    static Bone from_euler(Vec3 pos, Vec3 rot_deg) {
        Bone b; b.pos = pos;
        if (std::fabs(rot_deg.x) < 0.001f && std::fabs(rot_deg.z) < 0.001f) return b;
        const float k = 3.14159265358979323846f / 180.0f;
        const float ax = rot_deg.x * k, az = rot_deg.z * k;
        b.cos_x = std::cos(ax); b.sin_x = std::sin(ax); b.cos_z = std::cos(az); b.sin_z = std::sin(az); b.rotate = true;
        return b;
    }
    B32Bone pack() const { return B32Bone{ { pos.x, pos.y, pos.z }, cos_x, sin_x, cos_z, sin_z, rotate ? 1u : 0u }; }
};
// the host restatement of b32_scene_pose for one vertex (rotate_by_euler(v.pos, bone_rot) + bone_pos, the normal rotated alike):
// separately rounded f32 operations in the reference's order (compile with -ffp-contract=off where the compiler would fuse).
// bone == nullptr: bone_transforms.get(idx) == None.
inline B32Vertex pose_vertex(const B32Vertex& v, const B32Bone* bone) {
    if (!bone) return v;
    B32Vertex o = v;
    if (!bone->rotate) { for (int k = 0; k < 3; ++k) o.pos[k] = v.pos[k] + bone->pos[k]; return o; }
    const auto turn = [&](const float* a, float* out) {
        const float y1 = a[1] * bone->cos_x + a[2] * bone->sin_x, z1 = (-a[1]) * bone->sin_x + a[2] * bone->cos_x;
        const float x2 = a[0] * bone->cos_z + y1 * bone->sin_z, y2 = (-a[0]) * bone->sin_z + y1 * bone->cos_z;
        out[0] = x2; out[1] = y2; out[2] = z1;
    };
    float r[3];
    turn(v.pos, r);
    for (int k = 0; k < 3; ++k) o.pos[k] = r[k] + bone->pos[k];
    turn(v.normal, o.normal);
    return o;
}
inline std::vector<B32Vertex> pose_vertices(const std::vector<B32Vertex>& vertices, const std::vector<uint16_t>& bone_of_vertex, const std::vector<Bone>& bones) {
    std::vector<B32Bone> tab; tab.reserve(bones.size());
    for (const auto& b : bones) tab.push_back(b.pack());
    std::vector<B32Vertex> out; out.reserve(vertices.size());
    for (size_t i = 0; i < vertices.size(); ++i) {
        const size_t b = i < bone_of_vertex.size() ? bone_of_vertex[i] : (size_t)B32_BONE_NONE;
        out.push_back(pose_vertex(vertices[i], b < tab.size() ? &tab[b] : nullptr));
    }
    return out;
}
// the host restatement of the in-place edits on the arrays a host keeps: what a patched mesh must be indistinguishable from once these
// arrays are uploaded afresh.  (On a rigged mesh the vertex records patch the REST vertices, which pose_vertices then poses.)
inline void patch_vertices(std::vector<B32Vertex>& vertices, const std::vector<B32VertexPatch>& recs) { for (const auto& r : recs) vertices.at(r.index) = r.v; }
inline void patch_faces(std::vector<B32Face>& faces, const std::vector<B32FacePatch>& recs) { for (const auto& r : recs) faces.at(r.index) = r.f; }
inline void patch_texels(std::vector<uint16_t>& texels, uint32_t tex_width, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const uint16_t* src, uint32_t stride) {
    for (uint32_t row = 0; row < h; ++row)
        for (uint32_t col = 0; col < w; ++col) texels.at((size_t)(y + row) * tex_width + x + col) = src[(size_t)row * stride + col];
}
// Clut::lookup (types.rs:390-397): an index at or past the palette is 0x0000
inline void patch_indexed(std::vector<uint16_t>& texels, uint32_t tex_width, uint32_t x, uint32_t y, uint32_t w, uint32_t h, const uint8_t* indices, uint32_t stride,
                          const std::vector<uint16_t>& clut) {
    for (uint32_t row = 0; row < h; ++row)
        for (uint32_t col = 0; col < w; ++col) {
            const size_t k = indices[(size_t)row * stride + col];
            texels.at((size_t)(y + row) * tex_width + x + col) = k < clut.size() ? clut[k] : (uint16_t)0;
        }
}
inline void ResidentMesh::pose(const std::vector<Bone>& bones) {
    std::vector<B32Bone> tab; tab.reserve(bones.size());
    for (const auto& b : bones) tab.push_back(b.pack());
    check(b32_scene_pose(ctx_, slot_, tab.data(), (uint32_t)tab.size()), "scene_pose");
}
// SkelBone: what the skeleton's drawing reads per bone (modeler/skeleton.rs:412-477, state.rs:2629-2638): the position of
// get_bone_world_transform(i), cos / sin of the WORLD rotation's .x / .z (always read: get_bone_tip_position has no early return), length,
// width = display_width() (state.rs:369-375) and the parent (B32_BONE_NONE: a root).
struct SkelBone {
    Vec3 pos; float cos_x = 1.0f, sin_x = 0.0f, cos_z = 1.0f, sin_z = 0.0f, length = 20.0f, width = 40.0f; uint32_t parent = B32_BONE_NONE;
    static float display_width(float length, float width) {
        if (width > 0.0f) return width;
        const float w = length * 0.15f;
        return w < 20.0f ? 20.0f : (w > 200.0f ? 200.0f : w);
    }
    static SkelBone from_rig(Vec3 pos, Vec3 rot_deg, float length, float width, uint32_t parent = B32_BONE_NONE) {
        SkelBone b; b.pos = pos; b.length = length; b.width = display_width(length, width); b.parent = parent;
        const float k = 3.14159265358979323846f / 180.0f;
        const float ax = rot_deg.x * k, az = rot_deg.z * k;
        b.cos_x = std::cos(ax); b.sin_x = std::sin(ax); b.cos_z = std::cos(az); b.sin_z = std::sin(az);
        return b;
    }
    B32SkelBone pack() const { return B32SkelBone{ { pos.x, pos.y, pos.z }, cos_x, sin_x, cos_z, sin_z, length, width, parent }; }
};
inline std::vector<B32SkelBone> pack_skeleton(const std::vector<SkelBone>& bones) {
    std::vector<B32SkelBone> tab; tab.reserve(bones.size());
    for (const auto& b : bones) tab.push_back(b.pack());
    return tab;
}
// B32SkeletonStyle with nothing selected or hovered: skeleton_to_triangles at this alpha
inline B32SkeletonStyle skeleton_style(uint8_t editor_alpha = 255, uint32_t mode = 0) {
    B32SkeletonStyle s{}; s.selected_bone = s.hovered_bone = s.hovered_tip = -1; s.mode = mode; s.editor_alpha = editor_alpha;
    return s;
}
inline void ResidentMesh::build_skeleton(const std::vector<SkelBone>& bones, const B32SkeletonStyle& style) {
    const std::vector<B32SkelBone> tab = pack_skeleton(bones);
    check(b32_scene_build_skeleton(ctx_, slot_, tab.data(), (uint32_t)tab.size(), &style), "scene_build_skeleton");
}
// MirrorSettings (modeler/state.rs:777-850) with the selected object's vertex and face ranges inside the source's body
struct Mirror {
    uint32_t axis = 1;                          // 1 X, 2 Y, 3 Z
    uint32_t v_first = 0, v_count = 0, f_first = 0, f_count = 0;
    float dim = B32_MIRROR_DIM;                 // viewport.rs:1273
    B32Mirror pack() const { B32Mirror m{}; m.axis = axis; m.dim = dim; m.v_first = v_first; m.v_count = v_count; m.f_first = f_first; m.f_count = f_count; return m; }
};
inline void ResidentMesh::build_mirror(const ResidentMesh& src, const Mirror& mirror) {
    const B32Mirror m = mirror.pack();
    check(b32_scene_build_mirror(ctx_, src.slot_, slot_, &m), "scene_build_mirror");
}
// the built mesh's (vertices, faces) for a body of nv vertices and nf faces
inline std::pair<uint32_t, uint32_t> mirror_counts(uint32_t nv, uint32_t nf, const Mirror& mirror) {
    const B32Mirror m = mirror.pack();
    uint32_t v = 0, f = 0;
    check(b32_mirror_counts(nv, nf, &m, &v, &f), "mirror_counts");
    return { v, f };
}
// draw_skeleton's hierarchy lines followed by draw_bone_dots' circles (skeleton.rs:70-79, :110-143) as world items, for draw_world
inline std::vector<B32WorldItem> skeleton_items(const std::vector<SkelBone>& bones, const B32SkeletonStyle& style) {
    const std::vector<B32SkelBone> tab = pack_skeleton(bones);
    uint32_t n = 0;
    check(b32_skeleton_items(tab.data(), (uint32_t)tab.size(), &style, nullptr, 0, &n), "skeleton_items");
    std::vector<B32WorldItem> out(n);
    check(b32_skeleton_items(tab.data(), (uint32_t)tab.size(), &style, out.data(), n, &n), "skeleton_items");
    return out;
}
struct MeshParams { float ambient; bool backface_cull, backface_wireframe; Fog fog; std::optional<Placement> placement = std::nullopt; };

// Picking: which placed resident mesh, and which of its triangles, lies under the cursor -- check_mesh_hit (editor/viewport_3d.rs:7700-7756)
// for every (mesh, placement) of the object loop (:7344-7377) and the face branch of the modeler's find_hovered_element
// (modeler/viewport.rs:2544-2594), on the device (b32_pick_meshes).  The placement is ALWAYS applied here (has_transform is not consulted:
// check_mesh_hit has no such shortcut).  ortho: OrthoProjection as (zoom, center_x, center_y).
struct PickItem { const ResidentMesh* mesh; Placement placement; };
struct PickResult { int32_t best = -1; std::vector<B32PickHit> hits; };          // best: index into the items, -1 when nothing is hit
namespace detail {
struct PickCall {                                                              // the packed arguments of one pick
    B32Camera cam; B32Ortho ortho; bool has_ortho; std::vector<b32_scene*> slots; std::vector<B32Placement> places;
    PickCall(const std::vector<PickItem>& items, const Camera& camera, const std::optional<Vec3>& o) : cam(pack(camera)), has_ortho((bool)o) {
        ortho = o ? B32Ortho{ o->x, o->y, o->z } : B32Ortho{ 0, 0, 0 };
        for (const auto& it : items) {
            slots.push_back(it.mesh ? it.mesh->slot() : nullptr);
            places.push_back({ it.placement.cos_f, it.placement.sin_f, { it.placement.world_pos.x, it.placement.world_pos.y, it.placement.world_pos.z } });
        }
    }
};
}  // namespace detail
inline PickResult pick_meshes(Framebuffer& fb, const std::vector<PickItem>& items, const Camera& camera, float mx, float my,
                              const std::optional<Vec3>& ortho = std::nullopt, bool cull_backfaces = false) {
    const detail::PickCall c(items, camera, ortho);
    PickResult r; r.hits.resize(items.size());
    check(b32_pick_meshes(fb.ctx(), &c.cam, c.has_ortho ? &c.ortho : nullptr, mx, my, cull_backfaces ? B32_PICK_CULL_BACKFACES : 0u, c.slots.data(),
                          c.places.data(), (uint32_t)items.size(), r.hits.data(), &r.best), "pick_meshes");
    return r;
}
// The asynchronous form: `out` (16 + 16 * items.size() bytes, preferably from b32_host_alloc) holds {int32 best; uint32 n; 8 bytes}, then the
// hits, once the returned ticket is done (b32_ticket_poll / _wait); no host synchronisation.
inline uint64_t pick_meshes_async(Framebuffer& fb, const std::vector<PickItem>& items, const Camera& camera, float mx, float my, void* out,
                                  const std::optional<Vec3>& ortho = std::nullopt, bool cull_backfaces = false) {
    const detail::PickCall c(items, camera, ortho);
    uint64_t ticket = 0;
    check(b32_pick_meshes_async(fb.ctx(), &c.cam, c.has_ortho ? &c.ortho : nullptr, mx, my, cull_backfaces ? B32_PICK_CULL_BACKFACES : 0u, c.slots.data(),
                                c.places.data(), (uint32_t)items.size(), out, &ticket), "pick_meshes_async");
    return ticket;
}
inline PickResult pick_result(const void* out) {                                // what pick_meshes_async delivered, once its ticket is done
    const unsigned char* p = static_cast<const unsigned char*>(out);
    PickResult r; uint32_t n = 0;
    std::memcpy(&r.best, p, 4); std::memcpy(&n, p + 4, 4);
    r.hits.resize(n);
    if (n) std::memcpy(r.hits.data(), p + 16, (size_t)n * sizeof(B32PickHit));
    return r;
}
// The host restatement of one item (what a host without the library walks per mouse move): separately rounded f32 operations in the
// reference's order (compile with -ffp-contract=off where the compiler would fuse).  A NaN depth is reported as the quiet NaN 0x7FC00000.
inline B32PickHit pick_mesh(const std::vector<Vertex>& vertices, const std::vector<Face>& faces, const Placement& p, const Camera& cam, size_t w, size_t h,
                            float mx, float my, const std::optional<Vec3>& ortho = std::nullopt, bool cull_backfaces = false) {
    struct Screen { bool some; float x, y, d; };
    const auto dot = [](Vec3 a, Vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; };   // Vec3::dot, math.rs:23-25
    std::vector<Screen> sv; sv.reserve(vertices.size());
    for (const auto& v : vertices) {                                            // viewport_3d.rs:7714-7728
        const float rx = v.pos.x * p.cos_f - v.pos.z * p.sin_f, rz = v.pos.x * p.sin_f + v.pos.z * p.cos_f;
        const Vec3 rel{ rx + p.world_pos.x - cam.position.x, v.pos.y + p.world_pos.y - cam.position.y, rz + p.world_pos.z - cam.position.z };
        const float cx = dot(rel, cam.basis_x), cy = dot(rel, cam.basis_y), cz = dot(rel, cam.basis_z);
        Screen s{ true, 0, 0, cz };
        if (ortho) {                                                            // math.rs:595-599
            s.x = (cx - ortho->y) * ortho->x + ((float)w / 2.0f);
            s.y = -(cy - ortho->z) * ortho->x + ((float)h / 2.0f);
        } else if (cz <= 0.1f) {                                                // math.rs:634
            s.some = false;
        } else {
            const float vs = ((float)(w < h ? w : h) / 2.0f) * 0.75f, denom = cz + 5.0f;
            s.x = (cx * 4.0f / denom) * vs + ((float)w / 2.0f);
            s.y = (cy * 4.0f / denom) * vs + ((float)h / 2.0f);
        }
        sv.push_back(s);
    }
    bool any = false; uint32_t tri = 0; float closest = 0.0f;
    for (size_t t = 0; t < faces.size(); ++t) {
        const Face& f = faces[t];
        if (f.v0 >= sv.size() || f.v1 >= sv.size() || f.v2 >= sv.size()) continue;
        const Screen &a = sv[f.v0], &b = sv[f.v1], &c = sv[f.v2];
        if (!a.some || !b.some || !c.some) continue;
        const float area = (b.x - a.x) * (c.y - a.y) - (c.x - a.x) * (b.y - a.y);
        if (cull_backfaces && area <= 0.0f) continue;                           // modeler/viewport.rs:2571-2574
        const auto sign = [&](const Screen& u, const Screen& v) { return (mx - v.x) * (u.y - v.y) - (u.x - v.x) * (my - v.y); };
        const float d1 = sign(a, b), d2 = sign(b, c), d3 = sign(c, a);          // point_in_triangle_2d, math.rs:687-706
        if (((d1 < 0.0f) || (d2 < 0.0f) || (d3 < 0.0f)) && ((d1 > 0.0f) || (d2 > 0.0f) || (d3 > 0.0f))) continue;
        float depth;                                                            // interpolate_depth_in_triangle, viewport_3d.rs:7485-7508
        if (std::fabs(area) < 0.0001f) depth = ((a.d + b.d) + c.d) / 3.0f;
        else {
            const float w0 = ((b.x - mx) * (c.y - my) - (c.x - mx) * (b.y - my)) / area;
            const float w1 = ((c.x - mx) * (a.y - my) - (a.x - mx) * (c.y - my)) / area;
            const float w2 = (1.0f - w0) - w1;
            depth = (w0 * a.d + w1 * b.d) + w2 * c.d;
        }
        if (!any || depth < closest) { any = true; closest = depth; tri = (uint32_t)t; }
    }
    if (!any) return B32PickHit{ 0u, 0xFFFFFFFFu, 0.0f, 0u };
    if (closest != closest) { const uint32_t q = 0x7FC00000u; std::memcpy(&closest, &q, 4); }
    return B32PickHit{ 1u, tri, closest, 0u };
}
// the loop over the items, viewport_3d.rs:7370
inline int32_t pick_best(const std::vector<B32PickHit>& hits) {
    int32_t best = -1;
    for (size_t i = 0; i < hits.size(); ++i) if (hits[i].hit && (best < 0 || hits[i].depth < hits[(size_t)best].depth)) best = (int32_t)i;
    return best;
}
// Hover and box selection: the modeler's find_hovered_element (modeler/viewport.rs:2379-2601) and apply_box_selection
// (modeler/viewport.rs:1624-1779) for ONE resident mesh, on the device (b32_hover_mesh, b32_box_select).  A Topology holds the modeler's
// polygons over the mesh's vertices (to_render_data_textured keeps the vertices 1:1, mesh_editor.rs:1623-1653).  Without a placement the
// vertices are used as they are; a placement is always applied.  ortho: OrthoProjection as (zoom, center_x, center_y).
class Topology {
public:
    Topology(Framebuffer& fb, const std::vector<uint32_t>& poly_start, const std::vector<uint32_t>& poly_verts) : ctx_(fb.ctx()), np_(poly_start.empty() ? 0 : (uint32_t)poly_start.size() - 1) {
        if (np_ && poly_start.back() != poly_verts.size()) throw Error(B32_E_ARG, "Topology: poly_start must end at poly_verts.size()");
        check(b32_topology_create(ctx_, poly_start.data(), np_, poly_verts.data(), &t_), "topology_create");
    }
    // the trivial topology of a triangle list: poly_start = 0, 3, 6, ...
    static Topology triangles(Framebuffer& fb, const std::vector<Face>& faces) {
        std::vector<uint32_t> start(faces.size() + 1), verts; verts.reserve(faces.size() * 3);
        for (size_t i = 0; i <= faces.size(); ++i) start[i] = (uint32_t)(3 * i);
        for (const auto& f : faces) { verts.push_back((uint32_t)f.v0); verts.push_back((uint32_t)f.v1); verts.push_back((uint32_t)f.v2); }
        return Topology(fb, start, verts);
    }
    ~Topology() { if (t_) b32_topology_destroy(ctx_, t_); }
    Topology(Topology&& o) noexcept : ctx_(o.ctx_), t_(o.t_), np_(o.np_) { o.t_ = nullptr; }
    Topology(const Topology&) = delete;
    Topology& operator=(const Topology&) = delete;
    b32_topology* handle() const { return t_; }
    uint32_t polygons() const { return np_; }
private:
    b32_ctx* ctx_ = nullptr; b32_topology* t_ = nullptr; uint32_t np_ = 0;
};
inline B32HoverParams hover_params(float mx, float my, bool see_through = false, uint32_t mirror_axis = 0, float mirror_threshold = 1.0f) {
    return B32HoverParams{ mx, my, 6.0f, 4.0f, see_through ? B32_HOVER_SEE_THROUGH : 0u, mirror_axis, mirror_threshold, 0u };   // viewport.rs:2428-2429
}
namespace detail {
struct MeshCall {                                                              // the packed arguments of one hover / box selection
    B32Camera cam; B32Ortho ortho; bool has_ortho; B32Placement place; bool placed;
    MeshCall(const Camera& camera, const std::optional<Vec3>& o, const std::optional<Placement>& p) : cam(pack(camera)), has_ortho((bool)o), placed((bool)p) {
        ortho = o ? B32Ortho{ o->x, o->y, o->z } : B32Ortho{ 0, 0, 0 };
        place = p ? B32Placement{ p->cos_f, p->sin_f, { p->world_pos.x, p->world_pos.y, p->world_pos.z } } : B32Placement{ 1.0f, 0.0f, { 0, 0, 0 } };
    }
};
}  // namespace detail
inline B32HoverResult hover_mesh(Framebuffer& fb, const ResidentMesh& mesh, const Topology& top, const Camera& camera, const B32HoverParams& params,
                                 const std::optional<Vec3>& ortho = std::nullopt, const std::optional<Placement>& placement = std::nullopt) {
    const detail::MeshCall c(camera, ortho, placement);
    B32HoverResult r{};
    check(b32_hover_mesh(fb.ctx(), &c.cam, c.has_ortho ? &c.ortho : nullptr, mesh.slot(), top.handle(), c.placed ? &c.place : nullptr, &params, &r), "hover_mesh");
    return r;
}
// The asynchronous form: `out` (32 bytes, preferably from b32_host_alloc) holds a B32HoverResult once the returned ticket is done.
inline uint64_t hover_mesh_async(Framebuffer& fb, const ResidentMesh& mesh, const Topology& top, const Camera& camera, const B32HoverParams& params, void* out,
                                 const std::optional<Vec3>& ortho = std::nullopt, const std::optional<Placement>& placement = std::nullopt) {
    const detail::MeshCall c(camera, ortho, placement);
    uint64_t ticket = 0;
    check(b32_hover_mesh_async(fb.ctx(), &c.cam, c.has_ortho ? &c.ortho : nullptr, mesh.slot(), top.handle(), c.placed ? &c.place : nullptr, &params, out, &ticket),
          "hover_mesh_async");
    return ticket;
}
// find_hovered_element's return tuple (viewport.rs:2596-2600): the vertex; the edge only without a vertex; the face only without either
struct HoveredElement { std::optional<uint32_t> vertex; std::optional<std::pair<uint32_t, uint32_t>> edge; std::optional<uint32_t> face; };
inline HoveredElement hovered_element(const B32HoverResult& r) {
    HoveredElement e;
    if (r.vertex != 0xFFFFFFFFu) e.vertex = r.vertex;
    else if (r.edge_v0 != 0xFFFFFFFFu) e.edge = std::make_pair(r.edge_v0, r.edge_v1);
    else if (r.face != 0xFFFFFFFFu) e.face = r.face;
    return e;
}
struct BoxSelection { uint32_t n_selected = 0; std::vector<uint32_t> words; bool test(size_t i) const { return (words[i >> 5] >> (i & 31)) & 1u; } };
// mode B32_BOX_VERTICES: n_elements = the mesh's vertex count, top may be NULL; B32_BOX_POLYGONS: n_elements = top->polygons()
inline BoxSelection box_select(Framebuffer& fb, const ResidentMesh& mesh, const Topology* top, const Camera& camera, float x0, float y0, float x1, float y1,
                               uint32_t mode, size_t n_elements, const std::optional<Vec3>& ortho = std::nullopt,
                               const std::optional<Placement>& placement = std::nullopt) {
    const detail::MeshCall c(camera, ortho, placement);
    const B32BoxParams prm{ x0, y0, x1, y1, mode, { 0, 0, 0 } };
    BoxSelection r; r.words.assign((n_elements + 31) / 32, 0u);
    check(b32_box_select(fb.ctx(), &c.cam, c.has_ortho ? &c.ortho : nullptr, mesh.slot(), top ? top->handle() : nullptr, c.placed ? &c.place : nullptr, &prm,
                         r.words.data(), &r.n_selected), "box_select");
    return r;
}
// The modeler's selection overlays (modeler/viewport.rs:1782-2247: draw_selected_object_brackets, draw_mesh_selection_overlays,
// draw_box_selection_preview) made into records on the device from the mesh's resident vertices, posed or not, and drawn in the reference's
// order (b32_draw_mesh_overlay): enqueued, nothing read back.  The hovered element is a masked hover result (hovered_element), the
// selection one of the three lists, the preview its SelectMode and rectangle; the preview of an orthographic viewport is a second call
// with that viewport's camera and ortho.
struct MeshOverlay {
    uint32_t sections = 0;                                                     // B32_OVERLAY_* bits
    HoveredElement hover;
    uint32_t select_kind = 0;                                                  // 0 none, 1 vertices, 2 edges, 3 polygons
    std::vector<uint32_t> selected;                                            // indices; edges: (v0, v1) pairs one after another
    uint32_t preview_mode = 0; float x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    B32MeshOverlay pack() const {
        B32MeshOverlay o{};
        o.sections = sections;
        o.hover_vertex = hover.vertex.value_or(0xFFFFFFFFu);
        o.hover_edge_v0 = hover.edge ? hover.edge->first : 0xFFFFFFFFu; o.hover_edge_v1 = hover.edge ? hover.edge->second : 0xFFFFFFFFu;
        o.hover_face = hover.face.value_or(0xFFFFFFFFu);
        o.select_kind = select_kind; o.n_selected = (uint32_t)(select_kind == 2u ? selected.size() / 2 : selected.size());
        o.preview_mode = preview_mode; o.x0 = x0; o.y0 = y0; o.x1 = x1; o.y1 = y1;
        return o;
    }
};
inline void draw_mesh_overlay(Framebuffer& fb, const ResidentMesh& mesh, const Topology* top, const MeshOverlay& overlay, const Camera& camera,
                              const std::optional<Vec3>& ortho = std::nullopt) {
    const detail::MeshCall c(camera, ortho, std::nullopt);
    const B32MeshOverlay o = overlay.pack();
    check(b32_draw_mesh_overlay(fb.ctx(), &c.cam, c.has_ortho ? &c.ortho : nullptr, mesh.slot(), top ? top->handle() : nullptr, &o,
                                overlay.selected.empty() ? nullptr : overlay.selected.data()), "draw_mesh_overlay");
}
// Room hover and box selection: the world editor's find_hovered_elements (editor/viewport_3d.rs:7028-7336, the three sector loops and the
// priority rule) and find_selections_in_rect (:7512-7594) for the current room, on the device (b32_room_hover, b32_room_box_select).  A Room
// holds the grid and one B32SectorFace per sector face in iter_sectors order (world/geometry.rs:2828-2835: gx outer, gz inner; floor,
// ceiling, north, east, south, west walls by i, then nwse, then nesw); update() is a height drag.
// The room's render mesh (Room::to_render_data_with_textures, world/geometry.rs:2839-3352) is made on the device from the same records and
// one FaceMaterial per record (set_materials / update_materials): build_mesh() writes it into a resident mesh's slot, whose textures stay
// -- one launch, no upload, no host synchronisation.
using FaceMaterial = B32FaceMaterial;
// the reference's defaults: texture (0, 64) on both triangles, Color::NEUTRAL corners, Front, NwSe, Default, Opaque, black_transparent
inline FaceMaterial face_material() {
    FaceMaterial m{};
    m.tex_width = m.tex_width_2 = 64;
    for (int k = 0; k < 4; ++k) for (int c = 0; c < 3; ++c) m.colors[k][c] = m.colors_2[k][c] = 128;
    m.black_transparent = 1;
    return m;
}
// (n_vertices, n_faces) of the mesh of these records: where a record's output lies depends on (kind, normal_mode) alone
inline void room_mesh_counts(const std::vector<B32SectorFace>& faces, const std::vector<FaceMaterial>& materials, uint32_t& n_vertices, uint32_t& n_faces) {
    n_vertices = 0; n_faces = 0;
    for (size_t i = 0; i < faces.size() && i < materials.size(); ++i) {
        const uint32_t sides = materials[i].normal_mode == B32_NORMAL_BOTH ? 2u : 1u;
        n_vertices += (faces[i].kind < 2 ? 6u : 4u) * sides; n_faces += 2u * sides;
    }
}
class Room {
public:
    Room(Framebuffer& fb, const std::vector<B32SectorFace>& faces, const B32RoomGrid& grid = B32RoomGrid{ { 0.0f, 0.0f, 0.0f }, B32_SECTOR_SIZE })
        : ctx_(fb.ctx()), n_((uint32_t)faces.size()) {
        check(b32_room_create(ctx_, &grid, faces.data(), n_, &r_), "room_create");
    }
    ~Room() { if (r_) b32_room_destroy(ctx_, r_); }
    Room(Room&& o) noexcept : ctx_(o.ctx_), r_(o.r_), n_(o.n_) { o.r_ = nullptr; }
    Room(const Room&) = delete;
    Room& operator=(const Room&) = delete;
    // records [first, first + faces.size()) and, when given, the grid
    void update(uint32_t first, const std::vector<B32SectorFace>& faces, const B32RoomGrid* grid = nullptr) {
        check(b32_room_update(ctx_, r_, grid, first, (uint32_t)faces.size(), faces.data()), "room_update");
    }
    // one material per record; a range of them (ordered on the stream like update())
    void set_materials(const std::vector<FaceMaterial>& materials) {
        if (materials.size() != n_) throw std::invalid_argument("Room::set_materials: one material per face");
        check(b32_room_set_materials(ctx_, r_, materials.data()), "room_set_materials");
    }
    void update_materials(uint32_t first, uint32_t count, const FaceMaterial* materials) {
        check(b32_room_update_materials(ctx_, r_, first, count, materials), "room_update_materials");
    }
    void mesh_counts(uint32_t& n_vertices, uint32_t& n_faces) const { check(b32_room_mesh_counts(r_, &n_vertices, &n_faces), "room_mesh_counts"); }
    // the render mesh into `slot` (nullptr: the context's resident scene), which must hold an uploaded scene
    void build_mesh(b32_scene* slot = nullptr) { check(b32_room_build_mesh(ctx_, r_, slot), "room_build_mesh"); }
    b32_room* handle() const { return r_; }
    uint32_t faces() const { return n_; }
private:
    b32_ctx* ctx_ = nullptr; b32_room* r_ = nullptr; uint32_t n_ = 0;
};
inline B32RoomHoverParams room_hover_params(float mx, float my) { return B32RoomHoverParams{ mx, my, 6.0f, 4.0f }; }   // viewport_3d.rs:7038-7039
// all three loops, raw; room_hover_winner is the reference's answer
inline B32RoomHover room_hover(Framebuffer& fb, const Room& room, const Camera& camera, const B32RoomHoverParams& params) {
    const B32Camera cam = detail::pack(camera);
    B32RoomHover r{};
    check(b32_room_hover(fb.ctx(), &cam, room.handle(), &params, &r), "room_hover");
    return r;
}
// The asynchronous form: `out` (48 bytes, preferably from b32_host_alloc) holds a B32RoomHover once the returned ticket is done.
inline uint64_t room_hover_async(Framebuffer& fb, const Room& room, const Camera& camera, const B32RoomHoverParams& params, void* out) {
    const B32Camera cam = detail::pack(camera);
    uint64_t ticket = 0;
    check(b32_room_hover_async(fb.ctx(), &cam, room.handle(), &params, out, &ticket), "room_hover_async");
    return ticket;
}
// viewport_3d.rs:7283-7336: 0 vertex, 1 edge, 2 face, -1 nothing (closest by depth; within 1 % of the closest depth vertex > edge > face)
inline int room_hover_winner(const B32RoomHover& r) { return b32_room_hover_winner(&r); }
// element i is record i, then point i - room.faces() of `points` (the room's object positions)
inline BoxSelection room_box_select(Framebuffer& fb, const Room& room, const Camera& camera, float x0, float y0, float x1, float y1,
                                    const std::vector<Vec3>& points = {}) {
    const B32Camera cam = detail::pack(camera);
    std::vector<float> xyz; xyz.reserve(points.size() * 3);
    for (const auto& p : points) { xyz.push_back(p.x); xyz.push_back(p.y); xyz.push_back(p.z); }
    BoxSelection r; r.words.assign(((size_t)room.faces() + points.size() + 31) / 32, 0u);
    check(b32_room_box_select(fb.ctx(), &cam, room.handle(), x0, y0, x1, y1, xyz.data(), (uint32_t)points.size(), r.words.data(), &r.n_selected),
          "room_box_select");
    return r;
}
// The world editor's room overlays (editor/viewport_3d.rs:4273-4658, :4862-5362: the selected / hovered vertices, the selected edges, the
// hovered edge and face, draw_selection's SectorFace and Edge arms, the box-select preview) made into records on the device from the
// room's resident records and drawn in the reference's order (b32_draw_room_overlay): enqueued, nothing read back.  hover_source 1 reads
// the room's last room_hover[_async] where it lies on the device -- no ticket to wait for.  Selection::Sector is a host's own
// B32_GIZMO_LINE items (draw_gizmos).
struct RoomOverlay {
    uint32_t sections = 0;                                                     // B32_ROOM_OVERLAY_* bits
    uint32_t hover_source = 0;                                                 // 0: `hover`; 1: the room's last hover, on the device
    B32RoomHover hover{ 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0xFFFFFFFFu, 0, { 0, 0 } };   // raw, all three loops
    uint32_t primary_vertex = 0xFFFFFFFFu;                                     // key 4 * rec + corner
    uint32_t skip_first = 0, skip_count = 0;                                   // the records state.selection.includes_face() covers
    std::vector<uint32_t> vertices;                                            // keys, strictly ascending
    std::vector<uint32_t> edges;                                               // (rec, edge_idx) pairs one after another
    std::vector<uint32_t> faces;                                               // recs
    std::vector<Vec3> points;                                                  // the room's object positions
    float x0 = 0, y0 = 0, x1 = 0, y1 = 0;                                      // selection_rect_start / _end as stored
    B32RoomOverlay pack() const {
        B32RoomOverlay o{};
        o.sections = sections; o.hover_source = hover_source; o.hover = hover; o.primary_vertex = primary_vertex;
        o.skip_first = skip_first; o.skip_count = skip_count;
        o.n_vertices = (uint32_t)vertices.size(); o.n_edges = (uint32_t)(edges.size() / 2); o.n_faces = (uint32_t)faces.size(); o.n_points = (uint32_t)points.size();
        o.x0 = x0; o.y0 = y0; o.x1 = x1; o.y1 = y1;
        return o;
    }
};
inline void draw_room_overlay(Framebuffer& fb, const Room& room, const RoomOverlay& overlay, const Camera& camera) {
    const B32Camera cam = detail::pack(camera);
    const B32RoomOverlay o = overlay.pack();
    std::vector<float> xyz; xyz.reserve(overlay.points.size() * 3);
    for (const auto& p : overlay.points) { xyz.push_back(p.x); xyz.push_back(p.y); xyz.push_back(p.z); }
    check(b32_draw_room_overlay(fb.ctx(), &cam, room.handle(), &o, overlay.vertices.empty() ? nullptr : overlay.vertices.data(),
                                overlay.edges.empty() ? nullptr : overlay.edges.data(), overlay.faces.empty() ? nullptr : overlay.faces.data(),
                                xyz.empty() ? nullptr : xyz.data()), "draw_room_overlay");
}
// The world editor's object overlays (draw_asset_wireframe, editor/viewport_3d.rs:255-291; asset.bounds() -> draw_rotated_bounding_box,
// asset/asset.rs:288-312 and viewport_3d.rs:7658-7697) made into records on the device from resident asset parts and drawn in array order
// (b32_draw_object_overlays): enqueued, nothing read back, no per-frame walk of half-edges or vertices on the host.  An asset is a run of
// parts in `parts`; an item is one reference call and always applies its placement.
struct ObjectPart {
    const ResidentMesh* mesh = nullptr;                                        // holds the part's mesh
    const Topology* topology = nullptr;                                        // its polygons; may stay null when hidden or only boxes read it
    bool visible = true;                                                       // part.visible
    B32ObjectPart pack() const {
        return B32ObjectPart{ mesh ? mesh->slot() : nullptr, topology ? topology->handle() : nullptr, visible ? 0u : B32_OBJECT_PART_HIDDEN, 0u };
    }
};
struct ObjectItem {
    uint8_t kind = B32_OBJECT_WIRE;                                            // B32_OBJECT_*
    Placement place;                                                           // has_transform is not consulted (viewport_3d.rs:276-285 has no shortcut)
    uint32_t first_part = 0, n_parts = 0;
    Vec3 box_min, box_max;                                                     // B32_OBJECT_BOX
    Color color{ 255, 200, 50 };
    B32ObjectItem pack() const {
        B32ObjectItem o{};
        o.place = B32Placement{ place.cos_f, place.sin_f, { place.world_pos.x, place.world_pos.y, place.world_pos.z } };
        o.first_part = first_part; o.n_parts = n_parts;
        o.box_min[0] = box_min.x; o.box_min[1] = box_min.y; o.box_min[2] = box_min.z;
        o.box_max[0] = box_max.x; o.box_max[1] = box_max.y; o.box_max[2] = box_max.z;
        o.r = color.r; o.g = color.g; o.b = color.b; o.blend = (uint8_t)color.blend; o.kind = kind;
        return o;
    }
};
inline void draw_object_overlays(Framebuffer& fb, const std::vector<ObjectPart>& parts, const std::vector<ObjectItem>& items, const Camera& camera) {
    const B32Camera cam = detail::pack(camera);
    std::vector<B32ObjectPart> p; p.reserve(parts.size());
    for (const auto& x : parts) p.push_back(x.pack());
    std::vector<B32ObjectItem> it; it.reserve(items.size());
    for (const auto& x : items) it.push_back(x.pack());
    check(b32_draw_object_overlays(fb.ctx(), &cam, p.empty() ? nullptr : p.data(), (uint32_t)p.size(), it.empty() ? nullptr : it.data(), (uint32_t)it.size()),
          "draw_object_overlays");
}
// The host restatements (what a host without the library walks per mouse move): separately rounded f32 operations in the reference's order
// (compile with -ffp-contract=off where the compiler would fuse).
namespace detail {
struct HoverScreen { bool some; float x, y, d; };
inline Vec3 hover_world(const Vec3& v, const std::optional<Placement>& p) {
    if (!p) return v;
    const float rx = v.x * p->cos_f - v.z * p->sin_f, rz = v.x * p->sin_f + v.z * p->cos_f;
    return { rx + p->world_pos.x, v.y + p->world_pos.y, rz + p->world_pos.z };
}
inline HoverScreen hover_project(const Vec3& world, const Camera& cam, size_t w, size_t h, const std::optional<Vec3>& ortho) {   // math.rs:538-575
    const auto dot = [](Vec3 a, Vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; };
    const Vec3 rel{ world.x - cam.position.x, world.y - cam.position.y, world.z - cam.position.z };
    const float cx = dot(rel, cam.basis_x), cy = dot(rel, cam.basis_y), cz = dot(rel, cam.basis_z);
    HoverScreen s{ true, 0, 0, cz };
    if (ortho) { s.x = (cx - ortho->y) * ortho->x + ((float)w / 2.0f); s.y = -(cy - ortho->z) * ortho->x + ((float)h / 2.0f); }
    else if (cz <= 0.1f) s.some = false;
    else {
        const float vs = ((float)(w < h ? w : h) / 2.0f) * 0.75f, denom = cz + 5.0f;
        s.x = (cx * 4.0f / denom) * vs + ((float)w / 2.0f); s.y = (cy * 4.0f / denom) * vs + ((float)h / 2.0f);
    }
    return s;
}
inline float hover_dist(float px, float py, float x, float y) { const float dx = px - x, dy = py - y; return std::sqrt(dx * dx + dy * dy); }
inline float point_to_line_distance(float px, float py, float x0, float y0, float x1, float y1) {   // viewport.rs:2604-2622
    const float dx = x1 - x0, dy = y1 - y0, len_sq = dx * dx + dy * dy;
    if (len_sq < 0.001f) return hover_dist(px, py, x0, y0);
    float t = ((px - x0) * dx + (py - y0) * dy) / len_sq;
    if (t < 0.0f) t = 0.0f;
    if (t > 1.0f) t = 1.0f;
    return hover_dist(px, py, x0 + t * dx, y0 + t * dy);
}
}  // namespace detail
inline B32HoverResult hover_mesh(const std::vector<Vertex>& vertices, const std::vector<uint32_t>& poly_start, const std::vector<uint32_t>& poly_verts,
                                 const std::optional<Placement>& placement, const Camera& cam, size_t w, size_t h, const B32HoverParams& prm,
                                 const std::optional<Vec3>& ortho = std::nullopt) {
    const size_t nv = vertices.size(), np = poly_start.empty() ? 0 : poly_start.size() - 1;
    const bool cull = !(prm.flags & B32_HOVER_SEE_THROUGH);
    std::vector<detail::HoverScreen> sv; sv.reserve(nv);
    for (const auto& v : vertices) sv.push_back(detail::hover_project(detail::hover_world(v.pos, placement), cam, w, h, ortho));
    const auto editable = [&](size_t i) {                                        // state.rs:797-806
        const Vec3& p = vertices[i].pos;
        return prm.mirror_axis == 0 || (prm.mirror_axis == 1 ? p.x : prm.mirror_axis == 2 ? p.y : p.z) >= -prm.mirror_threshold;
    };
    const auto norm = [](uint32_t a, uint32_t b) { return ((uint64_t)(a < b ? a : b) << 32) | (a < b ? b : a); };
    std::vector<bool> vfront(nv, false); std::vector<uint64_t> efront;
    if (cull) {                                                                 // viewport.rs:2435-2473
        for (size_t p = 0; p < np; ++p) {
            const uint32_t s = poly_start[p], n = poly_start[p + 1] - s;
            if (n < 3) continue;
            const uint32_t i0 = poly_verts[s], i1 = poly_verts[s + 1], i2 = poly_verts[s + 2];
            if (i0 >= nv || i1 >= nv || i2 >= nv || !sv[i0].some || !sv[i1].some || !sv[i2].some) continue;
            const float area = (sv[i1].x - sv[i0].x) * (sv[i2].y - sv[i0].y) - (sv[i2].x - sv[i0].x) * (sv[i1].y - sv[i0].y);
            if (!(area > 0.0f)) continue;
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t a = poly_verts[s + k], b = poly_verts[s + (k + 1) % n];
                if (a < nv) vfront[a] = true;
                efront.push_back(norm(a, b));
            }
        }
        std::sort(efront.begin(), efront.end());
    }
    B32HoverResult r{ 0xFFFFFFFFu, 0.0f, 0xFFFFFFFFu, 0xFFFFFFFFu, 0.0f, 0xFFFFFFFFu, 0.0f, 0u };
    for (size_t i = 0; i < nv; ++i) {                                           // viewport.rs:2475-2505
        if ((cull && !vfront[i]) || !editable(i) || !sv[i].some) continue;
        const float dist = detail::hover_dist(prm.mx, prm.my, sv[i].x, sv[i].y);
        if (dist < prm.vertex_threshold && (r.vertex == 0xFFFFFFFFu || dist < r.vertex_dist)) { r.vertex = (uint32_t)i; r.vertex_dist = dist; }
    }
    for (size_t p = 0; p < np; ++p) {                                           // viewport.rs:2507-2542
        const uint32_t s = poly_start[p], n = poly_start[p + 1] - s;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t a = poly_verts[s + k], b = poly_verts[s + (k + 1) % n];
            if (cull && !std::binary_search(efront.begin(), efront.end(), norm(a, b))) continue;
            if (a >= nv || b >= nv || !editable(a) || !editable(b) || !sv[a].some || !sv[b].some) continue;
            const float dist = detail::point_to_line_distance(prm.mx, prm.my, sv[a].x, sv[a].y, sv[b].x, sv[b].y);
            if (dist < prm.edge_threshold && (r.edge_v0 == 0xFFFFFFFFu || dist < r.edge_dist)) { r.edge_v0 = a < b ? a : b; r.edge_v1 = a < b ? b : a; r.edge_dist = dist; }
        }
    }
    bool any = false; float closest = 0.0f;
    for (size_t p = 0; p < np; ++p) {                                           // viewport.rs:2544-2594
        const uint32_t s = poly_start[p], n = poly_start[p + 1] - s;
        bool ok = true;
        for (uint32_t k = 0; k < n && ok; ++k) ok = poly_verts[s + k] < nv && editable(poly_verts[s + k]);
        if (!ok) continue;
        for (uint32_t k = 1; k + 1 < n; ++k) {
            const detail::HoverScreen &a = sv[poly_verts[s]], &b = sv[poly_verts[s + k]], &c = sv[poly_verts[s + k + 1]];
            if (!a.some || !b.some || !c.some) continue;
            const float mx = prm.mx, my = prm.my;
            const float area = (b.x - a.x) * (c.y - a.y) - (c.x - a.x) * (b.y - a.y);
            if (cull && area <= 0.0f) continue;
            const auto sign = [&](const detail::HoverScreen& u, const detail::HoverScreen& v) { return (mx - v.x) * (u.y - v.y) - (u.x - v.x) * (my - v.y); };
            const float d1 = sign(a, b), d2 = sign(b, c), d3 = sign(c, a);
            if (((d1 < 0.0f) || (d2 < 0.0f) || (d3 < 0.0f)) && ((d1 > 0.0f) || (d2 > 0.0f) || (d3 > 0.0f))) continue;
            float depth;
            if (std::fabs(area) < 0.0001f) depth = ((a.d + b.d) + c.d) / 3.0f;
            else {
                const float w0 = ((b.x - mx) * (c.y - my) - (c.x - mx) * (b.y - my)) / area;
                const float w1 = ((c.x - mx) * (a.y - my) - (a.x - mx) * (c.y - my)) / area;
                const float w2 = (1.0f - w0) - w1;
                depth = (w0 * a.d + w1 * b.d) + w2 * c.d;
            }
            if (!any || depth < closest) { any = true; closest = depth; r.face = (uint32_t)p; }
        }
    }
    if (any) { if (closest != closest) { const uint32_t q = 0x7FC00000u; std::memcpy(&closest, &q, 4); } r.face_depth = closest; }
    return r;
}
inline BoxSelection box_select(const std::vector<Vertex>& vertices, const std::vector<uint32_t>& poly_start, const std::vector<uint32_t>& poly_verts,
                               const std::optional<Placement>& placement, const Camera& cam, size_t w, size_t h, float x0, float y0, float x1, float y1,
                               uint32_t mode, const std::optional<Vec3>& ortho = std::nullopt) {
    const size_t nv = vertices.size(), np = poly_start.empty() ? 0 : poly_start.size() - 1, n = mode == B32_BOX_POLYGONS ? np : nv;
    BoxSelection r; r.words.assign((n + 31) / 32, 0u);
    for (size_t i = 0; i < n; ++i) {
        Vec3 world;
        if (mode == B32_BOX_POLYGONS) {                                         // viewport.rs:1743-1766
            Vec3 acc{ 0, 0, 0 }; size_t cnt = 0;
            for (uint32_t j = poly_start[i]; j < poly_start[i + 1]; ++j) if (poly_verts[j] < nv) {
                const Vec3 p = detail::hover_world(vertices[poly_verts[j]].pos, placement);
                acc = { acc.x + p.x, acc.y + p.y, acc.z + p.z }; ++cnt;
            }
            if (!cnt) continue;
            const float inv = 1.0f / (float)cnt;
            world = { acc.x * inv, acc.y * inv, acc.z * inv };
        } else world = detail::hover_world(vertices[i].pos, placement);          // viewport.rs:1708-1726
        const detail::HoverScreen s = detail::hover_project(world, cam, w, h, ortho);
        if (s.some && s.x >= x0 && s.x <= x1 && s.y >= y0 && s.y <= y1) { r.words[i >> 5] |= 1u << (i & 31); ++r.n_selected; }
    }
    return r;
}
namespace detail {
inline bool pack(const std::optional<Placement>& p, B32Placement& out) {
    if (!p || !p->has_transform) return false;
    out = { p->cos_f, p->sin_f, { p->world_pos.x, p->world_pos.y, p->world_pos.z } };
    return true;
}
}  // namespace detail
// One resident mesh on its own, placed (b32_render_scene_15_placed_async): enqueued only; errors and counters by b32_frame_finish.
inline void render_placed_async(Framebuffer& fb, const ResidentMesh& mesh, const Camera& camera, const RasterSettings& settings, const Fog& fog,
                                const std::optional<Placement>& placement) {
    const std::vector<B32Light> l = detail::pack(settings.lights);
    const B32Camera c = detail::pack(camera);
    const B32Settings s = detail::pack(settings, l);
    B32Fog f{}; const bool has_fog = detail::pack(fog, f);
    B32Placement pl{}; const bool placed = detail::pack(placement, pl);
    check(b32_scene_swap(fb.ctx(), mesh.slot()), "scene_swap");
    const int rc = b32_render_scene_15_placed_async(fb.ctx(), &c, &s, has_fog ? &f : nullptr, placed ? &pl : nullptr);
    check(b32_scene_swap(fb.ctx(), mesh.slot()), "scene_swap");
    check(rc, "render_scene_15_placed_async");
}
inline RasterTimings render_frame(Framebuffer& fb, const std::vector<std::pair<const ResidentMesh*, MeshParams>>& meshes, const Camera& camera,
                                  const RasterSettings& base) {
    const std::vector<B32Light> l = detail::pack(base.lights);
    const B32Camera c = detail::pack(camera);
    const B32Settings s = detail::pack(base, l);
    check(b32_frame_begin(fb.ctx(), &c, &s), "frame_begin");
    for (const auto& m : meshes) {
        B32MeshParams p{};
        p.ambient = m.second.ambient; p.backface_cull = m.second.backface_cull; p.backface_wireframe = m.second.backface_wireframe;
        p.has_fog = detail::pack(m.second.fog, p.fog) ? 1 : 0;
        B32Placement pl{};
        check(b32_frame_add_scene_placed(fb.ctx(), m.first->slot(), &p, detail::pack(m.second.placement, pl) ? &pl : nullptr), "frame_add_scene_placed");
    }
    check(b32_frame_end(fb.ctx()), "frame_end");
    B32Timings tm{};
    check(b32_frame_finish(fb.ctx(), &tm), "frame_finish");
    return { tm.transform_ms, tm.fog_ms, tm.cull_ms, tm.sort_ms, tm.draw_ms, tm.wireframe_ms, tm.triangles_drawn, tm.fragments };
}

// The console's loop as the reference runs it -- every frame drawn (scene::render_scene, scene.rs:158-261) AND handed to the presenter from host
// memory (game/renderer.rs:179-214) -- without a host round trip per frame: submit() enqueues Framebuffer::clear, the sky (`sky`), the frame's draws
// (b32_frame_submit: the mesh table in one call) and the copy of the finished frame into page-locked memory (b32_fb_download_async), and
// returns a ticket; wait(ticket) blocks until THAT frame's pixels are in the returned buffer.  Two buffers alternate, so the presenter reads
// frame i while frame i + 1 is drawn: keep at most two tickets outstanding.  A frame may carry one pick (submit's `pick`): it is enqueued
// behind the frame's draws, delivered into page-locked memory of its own and waited for one frame behind like the pixels (wait_pick); and,
// beside it, one hover of one of its meshes (submit's `hover`, wait_hover).
// A resident sky (b32_sky): Skybox::generate_mesh((0, 0, 0), time) once -- its positions are the offsets the reference adds to the camera
// position (world/geometry.rs:555-559, :686-710) -- then render() per frame from the camera alone (render.rs:81-139), and update() for the
// rows of a scrolling cloud layer.  Nothing here waits for the device but the constructor and the destructor.
class Sky {
public:
    Sky(Framebuffer& fb, const std::vector<B32SkyVertex>& offsets, const std::vector<uint32_t>& faces /* 3 per face */)
        : ctx_(fb.ctx()), nv_((uint32_t)offsets.size()) {
        check(b32_sky_create(ctx_, offsets.data(), nv_, faces.data(), (uint32_t)(faces.size() / 3), &s_), "sky_create");
    }
    ~Sky() { if (s_) b32_sky_destroy(ctx_, s_); }
    Sky(Sky&& o) noexcept : ctx_(o.ctx_), s_(o.s_), nv_(o.nv_) { o.s_ = nullptr; }
    Sky(const Sky&) = delete;
    Sky& operator=(const Sky&) = delete;
    void update(uint32_t first, const std::vector<B32SkyVertex>& verts) { check(b32_sky_update(ctx_, s_, first, (uint32_t)verts.size(), verts.data()), "sky_update"); }
    void render(Framebuffer& fb, const Camera& camera) const { const B32Camera c = detail::pack(camera); check(b32_render_sky(fb.ctx(), s_, &c), "render_sky"); }
    // stage tap (blocking): x, y per vertex for a w x h framebuffer, a NaN pair behind the camera
    std::vector<float> project(const Camera& camera, uint32_t w, uint32_t h) const {
        const B32Camera c = detail::pack(camera);
        std::vector<float> xy((size_t)nv_ * 2);
        check(b32_sky_project_batch(ctx_, s_, &c, w, h, xy.data()), "sky_project_batch");
        return xy;
    }
    b32_sky* handle() const { return s_; }
    uint32_t vertices() const { return nv_; }
private:
    b32_ctx* ctx_ = nullptr; b32_sky* s_ = nullptr; uint32_t nv_ = 0;
};
// What FrameLoop::submit draws between the clear and the meshes (game/renderer.rs:88-96): the sky, then the stars of `size`.
struct FrameSky { const Sky* sky = nullptr; std::vector<B32Star> stars; float size = 3.0f; };
struct FrameHover { const ResidentMesh* mesh; const Topology* topology; B32HoverParams params; std::optional<Vec3> ortho = std::nullopt; std::optional<Placement> placement = std::nullopt; };
struct FramePick { std::vector<PickItem> items; float mx = 0, my = 0; std::optional<Vec3> ortho = std::nullopt; bool cull_backfaces = false; };
class FrameLoop {
public:
    explicit FrameLoop(Framebuffer& fb) : fb_(fb) {
        for (auto& b : buf_) { b = static_cast<uint8_t*>(b32_host_alloc(fb.width * fb.height * 4)); if (!b) throw Error(B32_E_HIP, "b32_host_alloc"); }
        hover_buf_ = static_cast<B32HoverResult*>(b32_host_alloc(2 * sizeof(B32HoverResult))); if (!hover_buf_) throw Error(B32_E_HIP, "b32_host_alloc");
    }
    ~FrameLoop() { b32_synchronize(fb_.ctx()); for (auto b : buf_) b32_host_free(b); for (auto b : pick_buf_) b32_host_free(b); b32_host_free(hover_buf_); }
    FrameLoop(const FrameLoop&) = delete;
    FrameLoop& operator=(const FrameLoop&) = delete;
    uint64_t submit(Color clear, const std::vector<std::pair<const ResidentMesh*, MeshParams>>& meshes, const Camera& camera, const RasterSettings& base,
                    const FramePick* pick = nullptr, const FrameHover* hover = nullptr, const FrameSky* sky = nullptr) {
        const std::vector<B32Light> l = detail::pack(base.lights);
        const B32Camera c = detail::pack(camera);
        const B32Settings s = detail::pack(base, l);
        std::vector<b32_scene*> slots; std::vector<B32MeshParams> params; std::vector<B32Placement> places; std::vector<uint8_t> has_place;
        for (const auto& m : meshes) {
            B32MeshParams p{};
            p.ambient = m.second.ambient; p.backface_cull = m.second.backface_cull; p.backface_wireframe = m.second.backface_wireframe;
            p.has_fog = detail::pack(m.second.fog, p.fog) ? 1 : 0;
            slots.push_back(m.first->slot()); params.push_back(p);
            B32Placement pl{};
            has_place.push_back(detail::pack(m.second.placement, pl) ? 1 : 0); places.push_back(pl);
        }
        fb_.clear(clear);
        if (sky) {                                                  // behind the clear, in front of the meshes
            if (sky->sky) sky->sky->render(fb_, camera);
            fb_.draw_stars(sky->stars, sky->size);
        }
        check(b32_frame_submit_placed(fb_.ctx(), &c, &s, slots.data(), params.data(), places.data(), has_place.data(), (uint32_t)slots.size()), "frame_submit_placed");
        const size_t k = n_++ & 1;
        pick_ticket_[k] = 0;
        if (pick) {
            const size_t need = 16 + 16 * pick->items.size();
            if (need > pick_cap_[k]) {                              // (its previous pick was waited for, or is by now: two frames back)
                if (pick_buf_[k]) { check(b32_synchronize(fb_.ctx()), "synchronize"); b32_host_free(pick_buf_[k]); }
                pick_buf_[k] = b32_host_alloc(need + 1024); pick_cap_[k] = pick_buf_[k] ? need + 1024 : 0;
                if (!pick_buf_[k]) throw Error(B32_E_HIP, "b32_host_alloc");
            }
            pick_ticket_[k] = pick_meshes_async(fb_, pick->items, camera, pick->mx, pick->my, pick_buf_[k], pick->ortho, pick->cull_backfaces);
        }
        hover_ticket_[k] = 0;
        if (hover) hover_ticket_[k] = hover_mesh_async(fb_, *hover->mesh, *hover->topology, camera, hover->params, hover_buf_ + k, hover->ortho, hover->placement);
        check(b32_fb_download_async(fb_.ctx(), buf_[k], &ticket_[k]), "fb_download_async");
        return ticket_[k];
    }
    // the hover that travelled with the frame of `ticket` (submit's `hover`), once it has landed
    B32HoverResult wait_hover(uint64_t ticket) {
        for (size_t k = 0; k < 2; ++k) if (ticket_[k] == ticket && hover_ticket_[k]) {
            check(b32_ticket_wait(fb_.ctx(), hover_ticket_[k]), "ticket_wait");
            return hover_buf_[k];
        }
        throw Error(B32_E_ARG, "FrameLoop::wait_hover: no hover travelled with this ticket, or its buffer has been reused");
    }
    // the pick that travelled with the frame of `ticket` (submit's `pick`), once it has landed
    PickResult wait_pick(uint64_t ticket) {
        for (size_t k = 0; k < 2; ++k) if (ticket_[k] == ticket && pick_ticket_[k]) {
            check(b32_ticket_wait(fb_.ctx(), pick_ticket_[k]), "ticket_wait");
            return pick_result(pick_buf_[k]);
        }
        throw Error(B32_E_ARG, "FrameLoop::wait_pick: no pick travelled with this ticket, or its buffer has been reused");
    }
    // the frame of `ticket`, once it has landed (valid until the submit after next)
    const uint8_t* wait(uint64_t ticket) {
        check(b32_ticket_wait(fb_.ctx(), ticket), "ticket_wait");
        for (size_t k = 0; k < 2; ++k) if (ticket_[k] == ticket) return buf_[k];
        throw Error(B32_E_ARG, "FrameLoop::wait: the ticket's buffer has been reused");
    }
    // errors of the frames enqueued so far (b32_frame_finish), like any asynchronous frame
    void finish() { B32Timings tm{}; check(b32_frame_finish(fb_.ctx(), &tm), "frame_finish"); }
private:
    Framebuffer& fb_;
    uint8_t* buf_[2] = { nullptr, nullptr };
    uint64_t ticket_[2] = { 0, 0 };
    void* pick_buf_[2] = { nullptr, nullptr }; size_t pick_cap_[2] = { 0, 0 }; uint64_t pick_ticket_[2] = { 0, 0 };
    B32HoverResult* hover_buf_ = nullptr; uint64_t hover_ticket_[2] = { 0, 0 };
    size_t n_ = 0;
};

// Names used by BASELINE.json's north_star; the reference's real entry point is render_mesh_15 (SURVEY headline fact 3).
inline RasterTimings draw_mesh(Framebuffer& fb, const std::vector<Vertex>& v, const std::vector<Face>& f, const std::vector<Texture15>& t,
                               const Camera& c, const RasterSettings& s, const Fog& fog = std::nullopt) { return render_mesh_15(fb, v, f, t, c, s, fog); }

}  // namespace b32
