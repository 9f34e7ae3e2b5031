"""Times b32_draw_world against the only way of drawing world-space items without it, and checks each result once.

  100 000 draw_line_3d_alpha items (alpha 191, the modeler's edge overlay) in world space over a 2560x1920 z-buffer C3 frame:
    device   b32_draw_world: the items are copied into the pinned ring, projected by k_world_project and drawn from the device record buffer;
    host     the projection restated on the host in numpy (tests/test_world.py::np_world), then b32_draw_prims of its records.
  Wall time per batch with a host synchronisation, host work included on both sides, interleaved; and the device time of k_world_project
  alone (HIP events around the launch, b32_last_kernel_times "world_project").

Usage: python tools/world_time.py [out.json]   (prints one JSON object; writes it to out.json when given)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

from bonnie32_amd import abi, build as B, rasterizer as R, scenegen
from tests.test_prims import np_prims
from tests.test_world import np_world, random_items


def main(n=100_000, reps=15):
    sc = scenegen.make_scene("C3")
    sc.settings.use_zbuffer = True
    W, H = sc.width, sc.height
    rng = np.random.default_rng(7)
    I = random_items(rng, n, sc.camera, kinds=(abi.LINE_3D_ALPHA,), spread=(4000.0, 3000.0), depth=(-600.0, 6000.0), seg=150.0, clip_p=0.0)
    I["alpha"] = 191
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    fb.clear(sc.clear_color)
    R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    px0, z0 = fb.pixels, fb.zbuffer
    recs, counts = np_world(I, sc.camera, None, W, H)
    want = px0.copy(); np_prims(want, z0, W, H, recs)
    c0 = fb.world_counts()
    fb.draw_world(I, sc.camera)
    ok_dev = bool(np.array_equal(fb.pixels, want)) and tuple(a - b for a, b in zip(fb.world_counts(), c0)) == counts
    fb.upload(px0)
    fb.draw_prims(recs)
    ok_host = bool(np.array_equal(fb.pixels, want))

    def device():
        fb.draw_world(I, sc.camera)
        ctx.synchronize()

    def host():
        fb.draw_prims(np_world(I, sc.camera, None, W, H)[0])
        ctx.synchronize()

    for f in (device, host, device, host):
        f()
    td, th = [], []
    for _ in range(reps):
        for f, ts in ((device, td), (host, th)):
            t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
    ctx.set_profiling(1)
    kern = []
    for _ in range(reps):
        device()
        kern.append(ctx.last_kernel_times()["world_project"] * 1e3)
    ctx.set_profiling(0)
    ctx.close()
    res = {"tool": "world_time", "digest": B.csrc_digest(), "items": n, "kind": "LINE_3D_ALPHA", "size": [W, H], "drawn_dropped_rejected": list(counts),
           "b32_draw_world_ms": {"median": round(statistics.median(td), 4), "min": round(min(td), 4), "exact": ok_dev},
           "np_world_then_b32_draw_prims_ms": {"median": round(statistics.median(th), 4), "min": round(min(th), 4), "exact": ok_host},
           "k_world_project_us": {"median": round(statistics.median(kern), 2), "min": round(min(kern), 2), "max": round(max(kern), 2)}}
    s = json.dumps(res, indent=1)
    print(s)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(s + "\n")


if __name__ == "__main__":
    main()
