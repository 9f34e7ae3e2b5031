"""What a height drag costs when the room's render mesh is made on the device (b32_room_update + b32_room_build_mesh) and when the host
makes it (room_mesh in numpy + b32_scene_upload), host time included on both sides, every configuration checked against the mirror
(rasterizer.room_mesh) before it is timed:
  (a) the delivered frame of the Cathedral room (1029 records, its golden scene's camera, settings, fog and textures at 640x480) with a
      9-record drag every frame, every frame delivered by ticket and waited one frame behind.
  (b) the same two paths for a synthetic room of 256 x 256 sectors (a floor and a ceiling each: 131072 records).
  (c) b32_room_build_mesh alone for both rooms: calls enqueued back to back and drained once, per call (launch overhead included; the
      slot's capacity is settled, so no call synchronises).
  (d) the unchanged 12-room delivered frame of tools/placed_frame.py, which runs none of the new code: this library and (--parent-lib
      PATH) the parent commit's, alternately, each repetition a process of its own; whether this build's runs fall inside the parent's
      own range, and by how much if they do not.
usage: python tools/room_mesh_time.py [--parent-lib PATH] [--out profiles/room_mesh_time.json] [--reps 3] [--alternations 3]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.placed_frame import alternate, spread
from tools.room_hover_time import big_room

ROOMS = os.path.join(ROOT, "tests", "golden", "rooms")
SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "real", "cathedral-room0-game-640.b32scene")


def same(a, b):
    return a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def cathedral():
    import bonnie32_amd as b32
    from bonnie32_amd import scenefile
    z = np.load(os.path.join(ROOMS, "cathedral-room0.npz"))
    mats = np.load(os.path.join(ROOMS, "cathedral-room0.materials.npz"))["materials"]
    sc = scenefile.read_scene(SCENE)
    return z["faces"].astype(b32.abi.SECTOR_FACE_DTYPE), mats, z["grid"], sc.textures, sc.camera, sc.settings, sc.fog, sc.clear_color, sc.width, sc.height


def synthetic():
    import bonnie32_amd as b32
    faces, grid, cam, W, H = big_room()
    mats = b32.rtypes.make_face_materials(len(faces))
    y, x = np.mgrid[0:64, 0:64]
    tex = [b32.Texture15(64, 64, ((((x // 8 + y // 8) % 2) * 0x2D6B + 0x1084) & 0x7FFF).astype(np.uint16).reshape(-1), b32.abi.OPAQUE)]
    return faces, mats, grid, tex, cam, b32.RasterSettings.game(), None, b32.Color(20, 22, 28), W, H


def drag_frames(name, room_data, reps, n_frames):
    import bonnie32_amd as b32
    from bonnie32_amd import rasterizer as R
    faces, mats, grid, tex, cam, st, fog, clear, W, H = room_data
    faces = faces.copy()
    n = len(faces)
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    tickets = [0, 0]

    def dragged(i):
        first = (i * 131) % (n - 9)
        d = faces[first:first + 9]
        d["heights"] += np.float32(8.0 if (i // 64) % 2 == 0 else -8.0)
        return first, d

    def deliver(i):
        tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
        if i > 0:
            ctx.ticket_wait(tickets[(i - 1) & 1])

    # ---- the device path: the slot keeps its textures, the room its records
    slot = R.ResidentScene(fb, b32.make_vertices(0), b32.make_faces(0), tex).detach()
    room = R.Room(ctx, faces, grid)
    room.set_materials(mats)

    def device_frame(i):
        first, d = dragged(i)
        room.update(first, d)
        room.build_mesh(slot)
        fb.clear(clear); slot.render_async(cam, st, fog) if i == 0 else slot.render_async()
        deliver(i)

    # ---- the host path: the producer in numpy, then b32_scene_upload of 36 B per vertex (and its synchronisation)
    def host_frame(i, drag=True):
        if drag:
            dragged(i)
        v, f = R.room_mesh(faces, mats, grid)
        rs = R.ResidentScene(fb, v, f, tex)
        fb.clear(clear); rs.render_async(cam, st, fog)
        deliver(i)

    def drain(i):
        ctx.ticket_wait(tickets[i & 1]); ctx.finish()

    ok = True
    for i in range(4):                                      # the two paths draw the same bytes from the same records
        device_frame(i); drain(i)
        dev = bufs[i & 1][0].copy()
        wv, wf = R.room_mesh(faces, mats, grid)
        ok &= same(slot.read_vertices(), wv) and same(slot.read_faces(), wf)
        host_frame(i, drag=False); drain(i)
        ok &= bool(np.array_equal(dev, bufs[i & 1][0]))
    ms = {"device": [], "host": []}
    host_frames = max(8, n_frames // 20) if n > 20000 else n_frames
    for _ in range(reps):
        for how, frame, frames in (("device", device_frame, n_frames), ("host", host_frame, host_frames)):
            t0 = time.perf_counter()
            for i in range(frames):
                frame(i)
            drain(frames - 1)
            ms[how].append((time.perf_counter() - t0) / frames * 1e3)
            room.update(0, faces)
    # ---- the build alone, back to back
    build = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            room.build_mesh(slot)
        ctx.synchronize()
        build.append((time.perf_counter() - t0) / 200 * 1e3)
    nv, nf = room.mesh_counts()
    for _, p in bufs:
        ctx.host_free(p)
    room.close(); slot.close(); ctx.close()
    d, h = spread(ms["device"]), spread(ms["host"])
    return {"room": "%s, %d records -> %d vertices, %d faces, %dx%d; a 9-record drag every frame, every frame delivered to page-locked host memory "
                    "and waited one frame behind; ms per frame, host time included" % (name, n, nv, nf, W, H),
            "paths_equal_mirror_and_each_other": bool(ok),
            "b32_room_update_build_mesh_draw": d, "numpy_room_mesh_scene_upload_draw": h, "host_over_device": round(h["median_ms"] / d["median_ms"], 2),
            "b32_room_build_mesh_back_to_back_ms_per_call": spread(build)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--parent-lib")
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--out", default=os.path.join("profiles", "room_mesh_time.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bonnie32_amd import abi

    def run(mode, lib=None):                                # a fresh process of tools/placed_frame.py per repetition
        cmd = [sys.executable, os.path.join(ROOT, "tools", "placed_frame.py"), "--child", mode, "--reps", str(a.reps)] + (["--lib", lib] if lib else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode:
            raise RuntimeError(f"{mode}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    out = {"tool": "tools/room_mesh_time.py", "digest": abi.check_build_digest(),
           "a_cathedral": drag_frames("Cathedral room 0", cathedral(), a.reps, a.frames),
           "b_256x256_sectors": drag_frames("synthetic 256 x 256 sectors", synthetic(), a.reps, a.frames)}
    c = alternate(a, run, "rooms")
    if "parent" in c:
        lo, hi = c["parent_spread_ms"]
        c["this_outside_parent_range_by_ms"] = [round(max(lo - x, x - hi, 0.0), 4) for x in c["this"]["run_medians_ms"]]
    out["d_rooms_only_unchanged_frame"] = c
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
