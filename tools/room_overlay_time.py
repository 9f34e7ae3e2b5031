"""What the world editor's room overlays cost when the records are made on the device from the resident room (b32_draw_room_overlay) and when
the host makes them (wait for the hover ticket, a blocking b32_room_box_select, rasterizer.room_overlay_records in numpy, b32_draw_prims),
host time included on both sides, every configuration checked against the mirror before it is timed:
  (a) the delivered drag frame of the Cathedral room (1029 records, its golden scene at 640x480): update -> build_mesh -> draw -> hover ->
      overlay -> download every frame, waited one frame behind; 40 selected faces, 30 vertices, 12 edges, a rubber band over half the frame.
  (b) the Ctrl-A overlay alone (every face selected, all sections), a synchronisation per overlay: the Cathedral, and the synthetic room of
      256 x 256 sectors (131072 records: its PREVIEW section alone is 524288 slots, most of them no-ops).
  (c) the unchanged 12-room delivered frame of tools/placed_frame.py, which runs none of the new code: this library and (--parent-lib PATH)
      the parent commit's, alternately, each repetition a process of its own with three 2000-frame windows.
usage: python tools/room_overlay_time.py [--parent-lib PATH] [--out profiles/room_overlay_time.json] [--reps 3] [--alternations 3]"""
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
from tools.room_mesh_time import cathedral, synthetic


def overlay_for(n, cam, w, h, ctrl_a):
    from bonnie32_amd import abi, rasterizer as R
    faces = np.arange(n, dtype=np.uint32) if ctrl_a else np.arange(0, n, max(1, n // 40), dtype=np.uint32)[:40]
    keys = np.arange(0, 4 * n, max(1, 4 * n // 30), dtype=np.uint32)[:30]
    erec = np.arange(3, n, max(1, n // 12), dtype=np.uint32)[:12]
    pos, bz = np.array(cam.position, np.float32), np.array(cam.basis_z, np.float32)
    return R.RoomOverlay(abi.ROOM_OVERLAY_ALL, primary_vertex=int(keys[1]), rect=(w * 0.5, h + 10.0, -10.0, -10.0), vertices=keys,
                         edges=np.stack([erec, erec % 4], axis=1), faces=faces, points=np.stack([pos + bz * np.float32(1500.0), pos + bz * np.float32(2500.0)]))


def with_hover(ov, hover, source):
    from bonnie32_amd import rasterizer as R
    return R.RoomOverlay(ov.sections, hover=hover, hover_source=source, primary_vertex=ov.primary_vertex, skip=ov.skip, rect=ov.rect, vertices=ov.vertices,
                         edges=ov.edges, faces=ov.faces, points=ov.points)


def drag_frames(room_data, reps, n_frames):
    import bonnie32_amd as b32
    from bonnie32_amd import abi, rasterizer as R
    faces, mats, grid, tex, cam, st, fog, clear, W, H = room_data
    faces = faces.copy()
    n = len(faces)
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    hbufs = [ctx.host_alloc(64) for _ in range(2)]
    tickets = [0, 0]
    slot = R.ResidentScene(fb, b32.make_vertices(0), b32.make_faces(0), tex).detach()
    room = R.Room(ctx, faces, grid)
    room.set_materials(mats)
    ov = overlay_for(n, cam, W, H, False)
    resident = with_hover(ov, None, abi.ROOM_OVERLAY_HOVER_RESIDENT)
    lay = R.room_overlay_layout(n, ov)

    def dragged(i):
        first = (i * 131) % (n - 9)
        d = faces[first:first + 9]
        d["heights"] += np.float32(8.0 if (i // 64) % 2 == 0 else -8.0)
        return first, d

    def mouse(i):
        return (W * (0.2 + 0.6 * ((i * 37) % 100) / 100.0), H * (0.3 + 0.5 * ((i * 53) % 100) / 100.0))

    def head(i):
        first, d = dragged(i)
        room.update(first, d)
        room.build_mesh(slot)
        fb.clear(clear); slot.render_async(cam, st, fog) if i == 0 else slot.render_async()

    def deliver(i):
        tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
        if i > 0:
            ctx.ticket_wait(tickets[(i - 1) & 1])

    def device_frame(i):
        head(i)
        ctx.room_hover_async(room, cam, mouse(i), out=hbufs[i & 1])
        fb.draw_room_overlay(room, resident, cam)
        deliver(i)

    def host_frame(i):
        head(i)
        hover = ctx.room_hover(room, cam, mouse(i))                              # (blocking: the ticket is waited for)
        ctx.room_box_select(room, cam, lay["rect"], ov.points)                   # (blocking: the preview's selection)
        fb.draw_prims(R.room_overlay_records(faces, grid, with_hover(ov, hover, 0), cam, W, H, mats))
        deliver(i)

    def drain(i):
        ctx.ticket_wait(tickets[i & 1]); ctx.finish()

    ok = True
    for i in range(3):                                      # the two paths deliver the same bytes
        snapshot = faces.copy()
        device_frame(i); drain(i)
        dev = bufs[i & 1][0].copy()
        hover = hbufs[i & 1][0][:48].view(abi.ROOM_HOVER_DTYPE)[0].copy()
        tap = fb.room_overlay_project_batch(room, with_hover(ov, hover, 0), cam)
        ok &= tap.tobytes() == R.room_overlay_records(faces, grid, with_hover(ov, hover, 0), cam, W, H, mats).tobytes()
        faces[:] = snapshot; room.update(0, faces)
        host_frame(i); drain(i)
        ok &= bool(np.array_equal(dev, bufs[i & 1][0]))
    ms = {"device": [], "host": []}
    for _ in range(reps):
        for how, frame, frames in (("device", device_frame, n_frames), ("host", host_frame, max(20, n_frames // 10))):
            t0 = time.perf_counter()
            for i in range(frames):
                frame(i)
            drain(frames - 1)
            ms[how].append((time.perf_counter() - t0) / frames * 1e3)
    for _, p in bufs + hbufs:
        ctx.host_free(p)
    room.close(); slot.close(); ctx.close()
    d, h = spread(ms["device"]), spread(ms["host"])
    return {"frame": "Cathedral room 0, %d records, %dx%d; a 9-record drag, a hover and the overlays (%d records) every frame, every frame delivered to "
                     "page-locked host memory and waited one frame behind; ms per frame, host time included" % (n, W, H, lay["total"]),
            "paths_equal_mirror_and_each_other": bool(ok), "hover_source_1_draw_room_overlay": d,
            "ticket_wait_box_select_numpy_mirror_draw_prims": h, "host_over_device": round(h["median_ms"] / d["median_ms"], 2)}


def ctrl_a(name, room_data, reps, with_mats=True):
    import bonnie32_amd as b32
    from bonnie32_amd import abi, rasterizer as R
    faces, mats, grid, tex, cam, st, fog, clear, W, H = room_data
    n = len(faces)
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    room = R.Room(ctx, faces, grid)
    if with_mats:
        room.set_materials(mats)
    m = mats if with_mats else None
    ov = overlay_for(n, cam, W, H, True)
    hover = ctx.room_hover(room, cam, (W * 0.5, H * 0.6))
    ov = with_hover(ov, hover, 0)
    lay = R.room_overlay_layout(n, ov)
    want = R.room_overlay_records(faces, grid, ov, cam, W, H, m)
    ok = fb.room_overlay_project_batch(room, ov, cam).tobytes() == want.tobytes()
    fb.clear(clear); fb.draw_room_overlay(room, ov, cam); a = fb.pixels
    fb.clear(clear); fb.draw_prims(want); ok &= bool(np.array_equal(a, fb.pixels))
    drawing = int((~((want["kind"] == abi.PRIM_CIRCLE) & (want["size"] < 0))).sum())

    def device():
        fb.draw_room_overlay(room, ov, cam)
        ctx.synchronize()

    def host():
        ctx.room_box_select(room, cam, lay["rect"], ov.points)
        fb.draw_prims(R.room_overlay_records(faces, grid, ov, cam, W, H, m))
        ctx.synchronize()

    def preview_only():
        fb.draw_room_overlay(room, R.RoomOverlay(abi.ROOM_OVERLAY_PREVIEW, rect=ov.rect), cam)
        ctx.synchronize()

    out = {"room": "%s, %d records, %dx%d: every face selected, all sections: %d records of which %d draw (PREVIEW: %d slots); a synchronisation per "
                   "overlay; ms per overlay, host time included" % (name, n, W, H, lay["total"], drawing, lay["total"] - lay["preview"]),
           "equal_mirror_and_draw_prims": bool(ok)}
    big = n > 20000
    for key, fn, k in (("b32_draw_room_overlay", device, 5 if big else 30), ("numpy_mirror_draw_prims", host, 2 if big else 10),
                       ("preview_section_alone", preview_only, 5 if big else 30)):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            ts.append((time.perf_counter() - t0) / k * 1e3)
        out[key] = spread(ts)
    out["host_over_device"] = round(out["numpy_mirror_draw_prims"]["median_ms"] / out["b32_draw_room_overlay"]["median_ms"], 2)
    room.close(); ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--parent-lib")
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--out", default=os.path.join("profiles", "room_overlay_time.json"))
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
    out = {"tool": "tools/room_overlay_time.py", "digest": abi.check_build_digest(),
           "a_cathedral_drag_frame": drag_frames(cathedral(), a.reps, a.frames),
           "b_ctrl_a_cathedral": ctrl_a("Cathedral room 0", cathedral(), a.reps),
           "b_ctrl_a_256x256_sectors": ctrl_a("synthetic 256 x 256 sectors", synthetic(), a.reps, with_mats=False)}
    c = alternate(a, run, "rooms")
    if "parent" in c:
        lo, hi = c["parent_spread_ms"]
        c["this_outside_parent_range_by_ms"] = [round(max(lo - x, x - hi, 0.0), 4) for x in c["this"]["run_medians_ms"]]
    out["c_rooms_only_unchanged_frame"] = c
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
