"""Times b32_draw_lines in the two situations the line pass is for, and checks each result against the sequential CPU result once.

  1. The console frame of tools/console_frame.py (12 resident meshes, 320x240, z-buffer, Gouraud + lights, fog) delivered by ticket
     (b32_frame_submit + b32_fb_download_async, the presenter one frame behind), with and without the player's wireframe cylinder
     (draw_wireframe_cylinder, game/renderer.rs:984-1050: 30 draw_line_3d segments for 12 segments) between the submit and the download.
     Runs of both variants are interleaved; the medians per delivered frame are compared.
  2. 100 000 random draw_line_3d_alpha lines (alpha 191, the modeler's edge overlay; lengths up to 48 px) over a 2560x1920 z-buffer C3
     frame, tile route on and off: wall time per batch, host copy into the pinned ring and the upload included.

Usage: python tools/lines_time.py [out.json]   (prints one JSON object; writes it to out.json when given)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np

import bonnie32_amd as b32
from bonnie32_amd import abi, build as B, rasterizer as R, scenegen
from test_lines import cylinder_lines, np_lines, random_lines


def console_meshes():
    """the scene of tools/console_frame.py"""
    rng = np.random.default_rng(2024)
    meshes = [scenegen.make_scene("C1", n_tris=int(rng.integers(300, 3000)), seed=1000 + i, variant=("blend" if i % 4 == 3 else "gouraud"),
                                  bbox_px=float(rng.choice([150.0, 400.0, 900.0]))) for i in range(12)]
    st = b32.RasterSettings.game()
    st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.point((0.0, -100.0, 1500.0), 3000.0, 1.2)]
    fog = (1500.0, 3000.0, 5800.0, b32.Color(40, 50, 70))
    return meshes, st, fog


def console_case(reps=9, frames=200):
    meshes, st, fog = console_meshes()
    W, H = meshes[0].width, meshes[0].height
    clear = b32.Color(10, 10, 30)
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in meshes]
    table = ctx.make_frame_table(meshes[0].camera, st, slots, fogs=[fog] * len(slots))
    cam = meshes[0].camera
    center = np.asarray(cam.position) + 1500.0 * np.asarray(cam.basis_z)
    cyl = cylinder_lines(cam, W, H, center, 200.0, 700.0)
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]

    def run(n, with_lines):
        tickets = []
        t0 = time.perf_counter()
        for i in range(n):
            fb.clear(clear)
            ctx.frame_submit(table)
            if with_lines:
                fb.draw_lines(cyl)
            tickets.append(ctx.download_async(bufs[i & 1][1]))
            if i:
                ctx.ticket_wait(tickets[i - 1])
        ctx.ticket_wait(tickets[-1])
        return (time.perf_counter() - t0) / n * 1e3

    run(20, False); run(20, True)
    base, lines = [], []
    for _ in range(reps):
        base.append(run(frames, False)); lines.append(run(frames, True))
    # the delivered frame with the cylinder against the frame without it (pixels and depths read back) + the sequential line result
    run(2, False); ctx.finish()
    px0, z0 = fb.pixels, fb.zbuffer
    run(2, True); ctx.finish()
    want = px0.copy(); np_lines(want, z0, W, H, cyl)
    ok = bool(np.array_equal(bufs[1][0], want))
    for _, p in bufs:
        ctx.host_free(p)
    ctx.close()
    mb, ml = statistics.median(base), statistics.median(lines)
    return {"frame_ms_without": round(mb, 4), "frame_ms_with_cylinder": round(ml, 4), "cylinder_added_us": round((ml - mb) * 1e3, 1),
            "runs_ms_without": [round(x, 4) for x in base], "runs_ms_with": [round(x, 4) for x in lines],
            "segments": int(len(cyl)), "frames_per_run": frames, "delivered_frame_exact": ok}


def alpha_case(n=100_000, reps=20):
    sc = scenegen.make_scene("C3")
    sc.settings.use_zbuffer = True
    W, H = sc.width, sc.height
    rng = np.random.default_rng(7)
    L = random_lines(rng, n, W, H, max_len=48, kinds=(abi.LINE_3D_ALPHA,), zrange=(0.0, 6000.0))
    L["alpha"] = 191
    out = {}
    for name, routes in (("tile_route", 0), ("scan_only", R.Context.ROUTE_LINE_TILES)):
        ctx = R.Context(0)
        ctx.set_routes(routes)
        fb = R.Framebuffer(W, H, ctx)
        fb.clear(sc.clear_color)
        R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
        px0, z0 = fb.pixels, fb.zbuffer
        fb.draw_lines(L)
        want = px0.copy(); np_lines(want, z0, W, H, L)
        ok = bool(np.array_equal(fb.pixels, want))
        for _ in range(3):
            fb.draw_lines(L)
        ctx.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fb.draw_lines(L)
            ctx.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        k = min(reps, 5)
        t0 = time.perf_counter()
        for _ in range(k):
            fb.draw_lines(L)
        ctx.synchronize()
        out[name] = {"batch_ms_median": round(statistics.median(ts), 4), "batch_ms_min": round(min(ts), 4),
                     "back_to_back_ms": round((time.perf_counter() - t0) / k * 1e3, 4), "exact": ok}
        ctx.close()
    out["lines"] = n
    return out


def main():
    res = {"tool": "lines_time", "digest": B.csrc_digest(), "console": console_case(), "alpha_100k_2560x1920": alpha_case()}
    s = json.dumps(res, indent=1)
    print(s)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(s + "\n")


if __name__ == "__main__":
    main()
