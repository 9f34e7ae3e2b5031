"""Times b32_draw_prims in the two situations the primitive pass is for, and checks each result against the sequential CPU result once.

  1. The modeler's overlay (tests/test_prims.py::modeler_overlay: every edge as draw_line_3d_alpha 191, a draw_circle_alpha r=3 alpha 140
     dot per vertex, a hover circle, thick selection edges) over a mesh of a few thousand vertices at 640x480, z-buffer, delivered by
     ticket (b32_frame_submit + b32_fb_download_async, the presenter one frame behind).  Three variants, runs interleaved, medians per
     delivered frame: no overlay, the overlay as ONE b32_draw_prims batch, the overlay issued one call per method (one record per call).
  2. 100 000 draw_circle_alpha (r=3, alpha 140) and 100 000 mixed primitives (every kind, tests/test_prims.py::random_prims) over a
     2560x1920 z-buffer C3 frame, tile route on and off: wall time per batch, host copy into the pinned ring and the upload included.

Usage: python tools/prims_time.py [out.json]   (prints one JSON object; writes it to out.json when given)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import bonnie32_amd as b32
from bonnie32_amd import abi, build as B, rasterizer as R, scenegen
from tests.test_prims import modeler_overlay, np_prims, random_prims


def modeler_case(reps=7, frames=100, per_call_frames=4):
    sc = scenegen.make_scene("C1", n_tris=1500, seed=77, variant="gouraud", width=640, height=480, bbox_px=48.0)
    W, H = sc.width, sc.height
    st = b32.RasterSettings.game()
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()]
    table = ctx.make_frame_table(sc.camera, st, slots)
    P = modeler_overlay(sc, W, H)
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    clear = b32.Color(10, 10, 30)

    def run(n, how):
        tickets = []
        t0 = time.perf_counter()
        for i in range(n):
            fb.clear(clear)
            ctx.frame_submit(table)
            if how == "batch":
                fb.draw_prims(P)
            elif how == "per_call":
                for k in range(len(P)):
                    fb.draw_prims(P[k:k + 1])
            tickets.append(ctx.download_async(bufs[i & 1][1]))
            if i:
                ctx.ticket_wait(tickets[i - 1])
        ctx.ticket_wait(tickets[-1])
        return (time.perf_counter() - t0) / n * 1e3

    run(10, "none"); run(10, "batch"); run(1, "per_call")
    res = {"none": [], "batch": [], "per_call": []}
    for _ in range(reps):
        res["none"].append(run(frames, "none")); res["batch"].append(run(frames, "batch")); res["per_call"].append(run(per_call_frames, "per_call"))
    run(2, "none"); ctx.finish()
    px0, z0 = fb.pixels, fb.zbuffer
    want = px0.copy(); np_prims(want, z0, W, H, P)
    run(2, "batch"); ctx.finish()
    ok_batch = bool(np.array_equal(bufs[1][0], want))
    run(2, "per_call"); ctx.finish()
    ok_per_call = bool(np.array_equal(bufs[1][0], want))
    for _, p in bufs:
        ctx.host_free(p)
    for s in slots:
        s.close()
    ctx.close()
    med = {k: statistics.median(v) for k, v in res.items()}
    return {"width": W, "height": H, "vertices": int(len(sc.vertices)), "prims": int(len(P)),
            "dots": int((P["kind"] == abi.PRIM_CIRCLE_ALPHA).sum()), "edges": int((P["kind"] == abi.LINE_3D_ALPHA).sum()),
            "frame_ms_without": round(med["none"], 4), "frame_ms_batch": round(med["batch"], 4), "frame_ms_per_call": round(med["per_call"], 4),
            "batch_added_us": round((med["batch"] - med["none"]) * 1e3, 1), "per_call_added_us": round((med["per_call"] - med["none"]) * 1e3, 1),
            "runs_ms": {k: [round(x, 4) for x in v] for k, v in res.items()}, "frames_per_run": frames, "per_call_frames_per_run": per_call_frames,
            "delivered_frame_exact": ok_batch and ok_per_call}


def big_case(n=100_000, reps=15):
    sc = scenegen.make_scene("C3")
    sc.settings.use_zbuffer = True
    W, H = sc.width, sc.height
    rng = np.random.default_rng(7)
    dots = random_prims(rng, n, W, H, kinds=(abi.PRIM_CIRCLE_ALPHA,))
    dots["size"] = 3; dots["alpha"] = 140
    mixed = random_prims(rng, n, W, H, max_len=48, max_r=10, zrange=(0.0, 6000.0))
    out = {}
    ctxs = {name: R.Context(0) for name in ("tile_route", "scan_only")}
    ctxs["scan_only"].set_routes(R.Context.ROUTE_PRIM_TILES)
    fbs = {}
    for name, ctx in ctxs.items():
        fb = fbs[name] = R.Framebuffer(W, H, ctx)
        fb.clear(sc.clear_color)
        R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    px0, z0 = fbs["tile_route"].pixels, fbs["tile_route"].zbuffer
    for case, P in (("circle_alpha_r3", dots), ("mixed", mixed)):
        want = px0.copy(); np_prims(want, z0, W, H, P)
        rows = {}
        for name, ctx in ctxs.items():
            fb = fbs[name]
            fb.upload(px0)
            fb.draw_prims(P)
            rows[name] = {"exact": bool(np.array_equal(fb.pixels, want)), "ts": []}
            for _ in range(3):
                fb.draw_prims(P)
            ctx.synchronize()
        for _ in range(reps):                                     # the two routes interleaved
            for name, ctx in ctxs.items():
                t0 = time.perf_counter()
                fbs[name].draw_prims(P)
                ctx.synchronize()
                rows[name]["ts"].append((time.perf_counter() - t0) * 1e3)
        out[case] = {name: {"batch_ms_median": round(statistics.median(r["ts"]), 4), "batch_ms_min": round(min(r["ts"]), 4), "exact": r["exact"]}
                     for name, r in rows.items()}
    for ctx in ctxs.values():
        ctx.close()
    out["prims"] = n
    return out


def main():
    res = {"tool": "prims_time", "digest": B.csrc_digest(), "modeler_640x480": modeler_case(), "prims_100k_2560x1920": big_case()}
    s = json.dumps(res, indent=1)
    print(s)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(s + "\n")


if __name__ == "__main__":
    main()
