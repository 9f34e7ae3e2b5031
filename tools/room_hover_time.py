"""What the world editor's room hover and rubber band cost (b32_room_hover[_async], b32_room_box_select), host time included on both sides,
every configuration checked against the host mirror (rasterizer.RoomMirror) before it is timed:
  (a) the delivered placed console frame of tools/placed_frame.py (12 resident rooms + 24 placed instances of 3 resident parts at 320x240,
      every instance moving every frame, every frame delivered by ticket) with and without ONE asynchronous hover of the Cathedral room
      (1029 records) per frame, its ticket waited one frame behind like the download's; windows of 1000 frames alternate (without, with,
      without, ...) in one process, medians of three.
  (b) one blocking hover and one box selection of the Cathedral room, and of a synthetic room of 256 x 256 sectors (a floor and a ceiling
      each: 131072 records), against RoomMirror in numpy (per call: the corners derived and projected on the host too, as
      find_hovered_elements does per call).
  (c) the unchanged 12-room delivered frame of tools/placed_frame.py, which runs none of the room kernels: this library and
      (--parent-lib PATH) the parent commit's, alternately, each repetition a process of its own; whether this build's runs fall inside the
      parent's own range, and by how much if they do not.
usage: python tools/room_hover_time.py [--parent-lib PATH] [--out profiles/room_hover_time.json] [--reps 3] [--alternations 3]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.placed_frame import alternate, placements, scene, spread

ROOMS = os.path.join(ROOT, "tests", "golden", "rooms")
FIELDS = ("vertex_rec", "vertex_corner", "vertex_dist", "vertex_depth", "edge_rec", "edge_idx", "edge_dist", "edge_depth", "face_rec", "face_depth")


def same(got, want):
    """Two abi.ROOM_HOVER_DTYPE records: indices and float bits, NaN equal to NaN."""
    for k in FIELDS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.tobytes() != b.tobytes() and not (a.dtype.kind == "f" and np.isnan(a) and np.isnan(b)):
            return False
    return True


def cathedral():
    import bonnie32_amd as b32
    z = np.load(os.path.join(ROOMS, "cathedral-room0.npz"))
    cam = b32.Camera(*(tuple(float(v) for v in row) for row in z["camera"]))
    return z["faces"], z["grid"], cam, int(z["size"][0]), int(z["size"][1])


def big_room(side=256):
    """side x side sectors, a floor and a ceiling each, gently sloped; the camera stands in the middle and looks along +z, a little down."""
    import bonnie32_amd as b32
    gx, gz = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    f = b32.rtypes.make_sector_faces(2 * side * side)
    f["gx"] = np.repeat(gx.reshape(-1), 2); f["gz"] = np.repeat(gz.reshape(-1), 2)
    f["kind"] = np.tile([0, 1], side * side)
    slope = ((np.repeat(gx.reshape(-1), 2) + np.repeat(gz.reshape(-1), 2)) % 5).astype(np.float32) * 64.0
    f["heights"] = np.where(f["kind"][:, None] == 0, slope[:, None], 3072.0 + slope[:, None])
    grid = np.zeros(1, b32.abi.ROOM_GRID_DTYPE); grid["sector_size"] = b32.abi.SECTOR_SIZE
    s, c = np.float32(np.sin(0.2)), np.float32(np.cos(0.2))
    cam = b32.Camera((side * 512.0, 900.0, side * 512.0), (1.0, 0.0, 0.0), (0.0, float(c), float(s)), (0.0, float(-s), float(c)))
    return f, grid, cam, 640, 480


def cursors_of(mirror, w, h, n=12):
    on = np.nonzero((mirror.some & (mirror.sx >= 8) & (mirror.sx < w - 8) & (mirror.sy >= 8) & (mirror.sy < h - 8)).reshape(-1))[0]
    pick = on[(np.arange(n) * 997) % len(on)]
    return [(float(mirror.sx.reshape(-1)[i]) + 1.5, float(mirror.sy.reshape(-1)[i]) - 1.0) for i in pick]


def console(reps, n_frames=1000):
    from bonnie32_amd import rasterizer as R
    rooms, parts, st, fog, clear = scene()
    W, H = rooms[0].width, rooms[0].height
    cam = rooms[0].camera
    faces, grid, rcam, _, _ = cathedral()
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    room_slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in rooms]
    part_slots = [R.ResidentScene(fb, p.vertices, p.faces, p.textures).detach() for p in parts]
    table = ctx.make_frame_table(cam, st, room_slots + part_slots * 8, fogs=[fog] * 36, placements=[None] * 36)
    room = R.Room(ctx, faces, grid)
    mirror = R.RoomMirror(faces, grid, rcam, W, H)
    aims = cursors_of(mirror, W, H, 16) + [((i + 0.5) * W / 12.0, (j + 0.5) * H / 9.0) for j in range(9) for i in range(12)]
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    hbufs = [ctx.host_alloc(48) for _ in range(2)]
    tickets, htickets, hresults = [0, 0], [0, 0], [None, None]

    def cursor(i):
        return aims[(37 * i) % len(aims)]

    def frame(i, hover):
        pls = placements(i)
        ctx.set_table_placements(table, [None] * 12 + [pls[k] for k in range(8) for _ in range(3)])
        fb.clear(clear); ctx.frame_submit(table)
        if hover:
            htickets[i & 1], hresults[i & 1] = ctx.room_hover_async(room, rcam, cursor(i), out=hbufs[i & 1])
        tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
        if i > 0:
            ctx.ticket_wait(tickets[(i - 1) & 1])
            if hover and htickets[(i - 1) & 1]:
                ctx.ticket_wait(htickets[(i - 1) & 1])

    def drain(i):
        ctx.ticket_wait(tickets[i & 1])
        if htickets[i & 1]:
            ctx.ticket_wait(htickets[i & 1])
        ctx.finish()

    ok, hit_frames, n_checked = True, 0, 48
    for i in range(n_checked):
        frame(i, True); drain(i)
        with_hover = bufs[i & 1][0].copy()
        got = hresults[i & 1].record
        ok &= same(got, mirror.hover(*cursor(i)))
        hit_frames += any(int(got[k]) != 0xFFFFFFFF for k in ("vertex_rec", "edge_rec", "face_rec"))
        htickets[0] = htickets[1] = 0
        frame(i, False); drain(i)
        ok &= bool(np.array_equal(with_hover, bufs[i & 1][0]))
    ms = {False: [], True: []}
    for _ in range(reps):                                   # alternately in one process: without, with, without, with, ...
        for hover in (False, True):
            htickets[0] = htickets[1] = 0
            t0 = time.perf_counter()
            for i in range(n_frames):
                frame(i, hover)
            drain(n_frames - 1)
            ms[hover].append((time.perf_counter() - t0) / n_frames * 1e3)
    for _, p in bufs + hbufs:
        ctx.host_free(p)
    room.close()
    ctx.close()
    a, b = spread(ms[False]), spread(ms[True])
    return {"frame": "320x240, 12 resident rooms + 24 placed instances of 3 resident parts, every instance moving every frame, every frame delivered to "
                     "page-locked host memory; one asynchronous hover of the Cathedral room (%d records) per frame, its ticket waited one frame "
                     "behind; ms per frame, host time included; windows of %d frames, alternately" % (len(faces), n_frames),
            "hovers_equal_mirror_and_frames_unchanged": ok, "checked_frames": n_checked, "checked_frames_with_a_hit": hit_frames,
            "without_hover": a, "with_one_async_room_hover_per_frame": b, "added_us_per_frame": round((b["median_ms"] - a["median_ms"]) * 1e3, 2)}


def one_room(name, faces, grid, cam, W, H, reps, n_host=3):
    from bonnie32_amd import rasterizer as R
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    room = R.Room(ctx, faces, grid)
    mirror = R.RoomMirror(faces, grid, cam, W, H)
    curs = cursors_of(mirror, W, H)
    rect = (W * 0.25, H * 0.25, W * 0.75, H * 0.75)
    ok, n_hit = True, 0
    for c in curs:
        want = mirror.hover(*c)
        ok &= same(ctx.room_hover(room, cam, c), want)
        n_hit += int(want["vertex_rec"]) != 0xFFFFFFFF
    want_w, want_n = mirror.box_select(rect)
    words, cnt = ctx.room_box_select(room, cam, rect)
    box_ok = bool(cnt == want_n and np.array_equal(words, want_w))
    dev, host, bdev, bhost = [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        for c in curs:
            ctx.room_hover(room, cam, c)
        dev.append((time.perf_counter() - t0) / len(curs) * 1e3)
        t0 = time.perf_counter()
        for c in curs[:n_host]:
            R.room_hover(faces, grid, cam, W, H, *c)
        host.append((time.perf_counter() - t0) / n_host * 1e3)
        t0 = time.perf_counter()
        for _ in range(len(curs)):
            ctx.room_box_select(room, cam, rect)
        bdev.append((time.perf_counter() - t0) / len(curs) * 1e3)
        t0 = time.perf_counter()
        for _ in range(n_host):
            R.room_box_select(faces, grid, cam, W, H, rect)
        bhost.append((time.perf_counter() - t0) / n_host * 1e3)
    room.close(); ctx.close()
    del fb
    d, h, bd, bh = spread(dev), spread(host), spread(bdev), spread(bhost)
    return {"room": "%s, %d records, %dx%d; one blocking call per cursor / rectangle; ms per call, host time included" % (name, len(faces), W, H),
            "hovers_equal_mirror": ok, "cursors_with_a_vertex": n_hit, "box_equals_mirror": box_ok, "box_selected": int(cnt),
            "b32_room_hover": d, "host_room_hover_numpy": h, "hover_host_over_device": round(h["median_ms"] / d["median_ms"], 1),
            "b32_room_box_select": bd, "host_room_box_select_numpy": bh, "box_host_over_device": round(bh["median_ms"] / bd["median_ms"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join("profiles", "room_hover_time.json"))
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
    out = {"tool": "tools/room_hover_time.py", "digest": abi.check_build_digest(), "a_placed_console_frame": console(a.reps),
           "b_cathedral": one_room("Cathedral room 0", *cathedral(), a.reps), "b_256x256_sectors": one_room("synthetic 256 x 256 sectors", *big_room(), a.reps)}
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
