// b32_sky_resident.hip -- the first thing the game tab's frame draws (game/renderer.rs:88-96), from inputs that stay on the device:
// the skybox of a resident sky (b32_render_sky) and the star sprites as records of the ordered tile pass (b32_draw_stars).
//
// Reference: Skybox::generate_mesh (world/geometry.rs:529-720) computes every position as camera_pos + x * radius with x * radius
// independent of the camera; Framebuffer::render_skybox (render.rs:81-139) then projects pos - camera.position.  (c + o) - c rounds twice
// and is NOT o: for a camera far from the origin most vertices move, and faces change pixels.  draw_star_diamond (render.rs:206-237) is
// 1, 5 or 9 set_pixel_safe calls, each exactly a 1x1 draw_filled_rect (render.rs:954-971 clamps to an empty range outside).
//
// GPU form: k_sky_place_project is k_sky_project with the placement in front, one lane per vertex, into the sky's own projected table;
// k_sky_fill (b32_sky.hip) reads it unchanged.  k_star_records writes one record per (star, pixel) lane at i * per + k, so the array
// order is the reference's call order; the records stay on the device for the pass of b32_prims.hip.
#include "b32_device.h"
#include "b32_sky_body.h"
#include "b32_prim_record.h"

namespace b32 {

__global__ void k_sky_place_project(const B32SkyVertex* __restrict__ off, uint32_t nv, B32Camera cam, uint32_t width, uint32_t height, float2* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    // camera_pos.x + x * radius (world/geometry.rs:555-559, :686-710), then vertex.pos - camera.position (render.rs:97): two roundings
    const float px = cam.position[0] + off[i].pos[0], py = cam.position[1] + off[i].pos[1], pz = cam.position[2] + off[i].pos[2];
    sky_screen_point(px - cam.position[0], py - cam.position[1], pz - cam.position[2], cam, width, height, &out[i]);
}
void launch_sky_place_project(hipStream_t s, const B32SkyVertex* offsets, uint32_t nv, const B32Camera& cam, uint32_t width, uint32_t height, float2* proj) {
    if (!nv) return;
    hipLaunchKernelGGL(k_sky_place_project, dim3((nv + 255) / 256), dim3(256), 0, s, offsets, nv, cam, width, height, proj);
}

// ---------------------------------------------------------------- star records
struct StarBatch { B32Star s[STAR_SMALL]; };
static_assert(sizeof(B32Star) == 12 && sizeof(StarBatch) == 768 && sizeof(StarArgs) + sizeof(StarBatch) <= 2048, "B32Star layout / kernel argument size");

// lane t: pixel k = t % per of star i = t / per (a.n * a.per <= 2^31 - 1: STAR_MAX)
__global__ __launch_bounds__(256) void k_star_records(StarArgs a, StarBatch few) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n * a.per) return;
    const uint32_t i = t / a.per, k = t - i * a.per;
    const B32Star st = a.stars ? a.stars[i] : few.s[i];
    // k: centre | (-1,0) (+1,0) (0,-1) (0,+1) | (-2,0) (+2,0) (0,-2) (0,+2)   (render.rs:212-236)
    const uint32_t j = (k - 1u) & 3u;
    const int32_t d = k == 0u ? 0 : (k < 5u ? 1 : 2), sd = (j & 1u) ? d : -d;
    // `cx - 1`, `cx + 2` ... on i32: a release build wraps (INT_MAX + 2 is negative -> set_pixel_safe rejects it)
    const int32_t x = (int32_t)((uint32_t)st.cx + (uint32_t)(j < 2u ? sd : 0)), y = (int32_t)((uint32_t)st.cy + (uint32_t)(j < 2u ? 0 : sd));
    const float scale = k < 5u ? 0.7f : 0.4f;
    PrimColor c{ st.r, st.g, st.b };
    if (k) { c.r = (uint8_t)f2u8_sat((float)st.r * scale); c.g = (uint8_t)f2u8_sat((float)st.g * scale); c.b = (uint8_t)f2u8_sat((float)st.b * scale); }
    a.out[t] = prim_line(B32_PRIM_FILLED_RECT, x, y, x, y, 0.0f, 0.0f, c, 255u);      // set_pixel_safe(x, y, c)
}
void launch_star_records(hipStream_t s, const StarArgs& a, const B32Star* small) {
    if (!a.n) return;
    StarBatch few{};
    if (small) for (uint32_t i = 0; i < a.n && i < STAR_SMALL; ++i) few.s[i] = small[i];
    hipLaunchKernelGGL(k_star_records, dim3((a.n * a.per + 255u) / 256u), dim3(256), 0, s, a, few);
}

}  // namespace b32
