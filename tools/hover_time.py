"""What hovering costs (b32_hover_mesh[_async]), on one build, host time included on both sides, every configuration checked against the
host mirror (rasterizer.HoverMirror) before it is timed:
  (a) the delivered placed console frame of tools/placed_frame.py (12 resident rooms + 24 placed instances of 3 resident parts at 320x240, every
      instance moving every frame, every frame delivered by ticket) with and without ONE asynchronous hover of the first placed part per
      frame, the cursor a little beside one of that part's projected vertices, its ticket waited one frame behind like the download's; windows alternate (without, with, without, ...) in one process, medians
      of three.  The comparison is against the run without hovers; nothing else is a baseline.
  (b) one blocking hover of obj-warrior (its fan pairs merged into quads) and of the C2 mesh (100 000 triangles, the trivial topology) against
      HoverMirror on the host (per call: vertex projection and front pass included on the host side, as find_hovered_element does them per
      call), and the kernels' device time from b32_last_kernel_times ("hover").
usage: python tools/hover_time.py [--out profiles/hover_time.json] [--reps 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tools.placed_frame import placements, scene, spread

REAL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "scenes", "real")


def same(got, want):
    """Two abi.HOVER_RESULT_DTYPE records: indices, distance and depth bits, NaN equal to NaN."""
    for k in ("vertex", "edge_v0", "edge_v1", "face"):
        if int(got[k]) != int(want[k]):
            return False
    for k in ("vertex_dist", "edge_dist", "face_depth"):
        a, b = np.float32(got[k]), np.float32(want[k])
        if a.tobytes() != b.tobytes() and not (np.isnan(a) and np.isnan(b)):
            return False
    return True


def merge_quads(faces):
    """Each consecutive fan pair (a, b, c), (a, c, d) of a triangle list becomes the quad (a, b, c, d)."""
    fv = [tuple(int(i) for i in f) for f in faces["v"]]
    out, i = [], 0
    while i < len(fv):
        if i + 1 < len(fv) and fv[i][0] == fv[i + 1][0] and fv[i][2] == fv[i + 1][1]:
            out.append([fv[i][0], fv[i][1], fv[i][2], fv[i + 1][2]]); i += 2
        else:
            out.append(list(fv[i])); i += 1
    return out


def console(reps, n_frames=1000):
    from bonnie32_amd import rasterizer as R
    rooms, parts, st, fog, clear = scene()
    W, H = rooms[0].width, rooms[0].height
    cam = rooms[0].camera
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    room_slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in rooms]
    part_slots = [R.ResidentScene(fb, p.vertices, p.faces, p.textures).detach() for p in parts]
    table = ctx.make_frame_table(cam, st, room_slots + part_slots * 8, fogs=[fog] * 36, placements=[None] * 36)
    top = R.Topology.from_polygons(merge_quads(parts[0].faces))
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    hbufs = [ctx.host_alloc(32) for _ in range(2)]
    tickets, htickets, hresults = [0, 0], [0, 0], [None, None]

    offs = [(0.0, 0.0), (2.5, -1.25), (-5.0, 3.0), (4.5, 4.5), (0.0, 6.0), (-3.0, -3.5), (9.0, 0.0), (1.0, 0.0)]

    def aim(i):
        """A little beside the projected position of a vertex of the hovered part under its placement of frame i (worked out before the
        timing starts, so that no window pays for it)."""
        m = R.HoverMirror(parts[0].vertices, top, placements(i)[0], cam, W, H)
        ok = np.nonzero(m.some & (m.sx >= 0) & (m.sx < W) & (m.sy >= 0) & (m.sy < H))[0]
        if not len(ok):
            return (W * 0.5, H * 0.5)
        j = ok[(7 * i) % len(ok)]
        return (float(m.sx[j]) + offs[i % 8][0], float(m.sy[j]) + offs[i % 8][1])
    cursors = [aim(i) for i in range(n_frames)]

    def cursor(i):
        return cursors[i]

    def frame(i, hover):
        pls = placements(i)
        per = [pls[k] for k in range(8) for _ in range(3)]
        ctx.set_table_placements(table, [None] * 12 + per)
        fb.clear(clear); ctx.frame_submit(table)
        if hover:
            htickets[i & 1], hresults[i & 1] = ctx.hover_mesh_async(part_slots[0], top, cam, cursor(i), placement=pls[0], see_through=bool(i & 1), out=hbufs[i & 1])
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

    # the hovers against the mirror, and the frames with hovers against the frames without
    ok, hit_frames, n_checked = True, 0, 48
    for i in range(n_checked):
        frame(i, True); drain(i)
        with_hover = bufs[i & 1][0].copy()
        want = R.HoverMirror(parts[0].vertices, top, placements(i)[0], cam, W, H).hover(*cursor(i), see_through=bool(i & 1))
        got = hresults[i & 1].record
        ok &= same(got, want)
        hit_frames += any(int(got[k]) != 0xFFFFFFFF for k in ("vertex", "edge_v0", "face"))
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
    top.close()
    ctx.close()
    a, b = spread(ms[False]), spread(ms[True])
    return {"frame": "320x240, 12 resident rooms + 24 placed instances of 3 resident parts, every instance moving every frame, every frame delivered to "
                     "page-locked host memory; one asynchronous hover of the first placed part (%d vertices, %d polygons) per frame, its ticket "
                     "waited one frame behind; ms per frame, host time included; windows of %d frames, alternately" % (len(parts[0].vertices), top.np, n_frames),
            "hovers_equal_mirror_and_frames_unchanged": ok, "checked_frames": n_checked, "checked_frames_with_a_hit": hit_frames,
            "without_hover": a, "with_one_async_hover_per_frame": b, "added_us_per_frame": round((b["median_ms"] - a["median_ms"]) * 1e3, 2)}


def one_mesh(name, sc, polygons, reps, n_host=3):
    from bonnie32_amd import rasterizer as R
    W, H = sc.width, sc.height
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    top = R.Topology.triangles(sc.faces) if polygons is None else R.Topology.from_polygons(polygons)
    mirror = R.HoverMirror(sc.vertices, top, None, sc.camera, W, H)
    ok_v = np.nonzero(mirror.some)[0]
    curs = [(float(mirror.sx[i]) + 1.5, float(mirror.sy[i]) - 1.0) for i in ok_v[(np.arange(12) * 997) % len(ok_v)]]
    ok, n_hit = True, 0
    for k, c in enumerate(curs):
        got = ctx.hover_mesh(rs, top, sc.camera, c, see_through=bool(k & 1))
        want = mirror.hover(*c, see_through=bool(k & 1))
        ok &= same(got, want)
        n_hit += int(want["vertex"]) != 0xFFFFFFFF
    dev, host, kern = [], [], []
    ctx.set_profiling(1)
    for _ in range(reps):
        t0 = time.perf_counter()
        for c in curs:
            ctx.hover_mesh(rs, top, sc.camera, c)
        dev.append((time.perf_counter() - t0) / len(curs) * 1e3)
        kern.append(dict(ctx.last_kernel_times()).get("hover"))
        t0 = time.perf_counter()
        for c in curs[:n_host]:
            R.hover_mesh(sc.vertices, top, None, sc.camera, W, H, *c)
        host.append((time.perf_counter() - t0) / n_host * 1e3)
    ctx.set_profiling(0)
    rs.close(); top.close(); ctx.close()
    d, h = spread(dev), spread(host)
    return {"mesh": "%s, %d vertices, %d polygons, %d half-edges, %dx%d, one blocking hover per cursor (culling); ms per hover, host time included"
                    % (name, len(sc.vertices), top.np, len(top.poly_verts), W, H),
            "hovers_equal_mirror": ok, "cursors_with_a_vertex": n_hit, "b32_hover_mesh": d, "host_hover_mesh_numpy": h,
            "host_over_device": round(h["median_ms"] / d["median_ms"], 1),
            "hover_kernels_ms": [None if k is None else round(float(k), 4) for k in kern]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "hover_time.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bonnie32_amd import abi, scenefile, scenegen
    warrior = scenefile.read_scene(os.path.join(REAL, "obj-warrior.b32scene"))
    out = {"tool": "tools/hover_time.py", "digest": abi.check_build_digest(), "a_placed_console_frame": console(a.reps),
           "b_obj_warrior": one_mesh("obj-warrior", warrior, merge_quads(warrior.faces), a.reps),
           "b_c2_mesh": one_mesh("C2", scenegen.make_scene("C2"), None, a.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
