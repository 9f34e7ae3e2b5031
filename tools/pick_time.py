"""What picking costs (b32_pick_meshes[_async]), on one build, host time included on both sides, every configuration checked against the host
mirror (b32.pick_mesh / rasterizer.PickMirror) before it is timed:
  (a) the delivered placed console frame of tools/placed_frame.py (12 resident rooms + 24 placed instances of 3 resident parts at 320x240, every
      instance moving every frame, every frame delivered by ticket) with and without ONE asynchronous pick of all 36 items per frame, its
      ticket waited one frame behind like the download's; windows alternate (without, with, without, ...) in one process, medians of three.
      The comparison is against the run without picks; nothing else is a baseline.
  (b) one blocking pick of the 1 M-triangle C3 mesh at 2560x1920 against b32.pick_mesh on the host (vertex projection included on the host side,
      as check_mesh_hit does it per call), and the two kernels' device time from b32_last_kernel_times ("pick").
usage: python tools/pick_time.py [--out profiles/pick_time.json] [--reps 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tools.placed_frame import placements, scene, spread

IDENT = (1.0, 0.0, (0.0, 0.0, 0.0))


def same(hit, want):
    """abi.PICK_HIT_DTYPE record against the mirror's (hit, tri, depth): depth bit for bit, NaN equal to NaN."""
    d, w = np.float32(hit["depth"]), np.float32(want[2])
    return bool(hit["hit"]) == bool(want[0]) and int(hit["tri"]) == int(want[1]) and (d.tobytes() == w.tobytes() or (np.isnan(d) and np.isnan(w)))


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
    meshes = rooms + parts * 8
    ptable = ctx.make_pick_table([(s, IDENT) for s in room_slots + part_slots * 8])
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    pbufs = [ctx.host_alloc(16 + 16 * 36) for _ in range(2)]
    tickets, ptickets, presults = [0, 0], [0, 0], [None, None]

    def cursor(i):
        return (W * (0.5 + 0.45 * np.sin(0.11 * i)), H * (0.5 + 0.4 * np.cos(0.07 * i)))

    def frame(i, pick):
        pls = placements(i)
        per = [pls[k] for k in range(8) for _ in range(3)]
        ctx.set_table_placements(table, [None] * 12 + per)
        fb.clear(clear); ctx.frame_submit(table)
        if pick:
            ctx.set_pick_placements(ptable, [IDENT] * 12 + per)
            ptickets[i & 1], presults[i & 1] = ctx.pick_meshes_async(ptable, cam, cursor(i), out=pbufs[i & 1])
        tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
        if i > 0:
            ctx.ticket_wait(tickets[(i - 1) & 1])
            if pick and ptickets[(i - 1) & 1]:
                ctx.ticket_wait(ptickets[(i - 1) & 1])

    def drain(i):
        ctx.ticket_wait(tickets[i & 1])
        if ptickets[i & 1]:
            ctx.ticket_wait(ptickets[i & 1])
        ctx.finish()

    # the picks against the mirror, and the frames with picks against the frames without
    ok, hit_frames = True, 0
    for i in range(24):
        frame(i, True); drain(i)
        with_pick = bufs[i & 1][0].copy()
        pls = placements(i)
        per = [IDENT] * 12 + [pls[k] for k in range(8) for _ in range(3)]
        want = [R.PickMirror(m.vertices, m.faces, pl, cam, W, H).pick(*cursor(i)) for m, pl in zip(meshes, per)]
        res = presults[i & 1]
        hits = res.hits
        ok &= all(same(h, w) for h, w in zip(hits, want)) and res.best == R.pick_best(hits)
        hit_frames += res.best >= 0
        ptickets[0] = ptickets[1] = 0
        frame(i, False); drain(i)
        ok &= bool(np.array_equal(with_pick, bufs[i & 1][0]))
    ms = {False: [], True: []}
    for _ in range(reps):                                   # alternately in one process: without, with, without, with, ...
        for pick in (False, True):
            ptickets[0] = ptickets[1] = 0
            t0 = time.perf_counter()
            for i in range(n_frames):
                frame(i, pick)
            drain(n_frames - 1)
            ms[pick].append((time.perf_counter() - t0) / n_frames * 1e3)
    for _, p in bufs + pbufs:
        ctx.host_free(p)
    ctx.close()
    a, b = spread(ms[False]), spread(ms[True])
    return {"frame": "320x240, 12 resident rooms + 24 placed instances of 3 resident parts (%d triangles), every instance moving every frame, every frame "
                     "delivered to page-locked host memory; one asynchronous pick of all 36 items per frame, its ticket waited one frame behind; ms per "
                     "frame, host time included; windows of %d frames, alternately" % (sum(len(m.faces) for m in meshes), n_frames),
            "picks_equal_mirror_and_frames_unchanged": ok, "checked_frames_with_a_hit": hit_frames,
            "without_pick": a, "with_one_async_pick_per_frame": b, "added_us_per_frame": round((b["median_ms"] - a["median_ms"]) * 1e3, 2)}


def big(reps):
    import bonnie32_amd as b32
    from bonnie32_amd import rasterizer as R, scenegen
    sc = scenegen.make_scene("C3")
    W, H = sc.width, sc.height
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    table = ctx.make_pick_table([(rs, IDENT)])
    rng = np.random.default_rng(7)
    curs = [(rng.random() * W, rng.random() * H) for _ in range(12)]
    mirror = R.PickMirror(sc.vertices, sc.faces, IDENT, sc.camera, W, H)
    ok, n_hit = True, 0
    for c in curs:
        best, hits = ctx.pick_meshes(table, sc.camera, c)
        want = mirror.pick(*c)
        ok &= same(hits[0], want) and best == (0 if want[0] else -1)
        n_hit += bool(want[0])
    dev, host, kern = [], [], []
    ctx.set_profiling(1)
    for _ in range(reps):
        t0 = time.perf_counter()
        for c in curs:
            ctx.pick_meshes(table, sc.camera, c)
        dev.append((time.perf_counter() - t0) / len(curs) * 1e3)
        kern.append(dict(ctx.last_kernel_times()).get("pick"))
        t0 = time.perf_counter()
        for c in curs[:3]:
            b32.pick_mesh(sc.vertices, sc.faces, IDENT, sc.camera, W, H, *c)
        host.append((time.perf_counter() - t0) / 3 * 1e3)
    ctx.set_profiling(0)
    rs.close(); ctx.close()
    d, h = spread(dev), spread(host)
    return {"mesh": "C3, %d triangles, %dx%d, one item, one blocking pick per cursor; ms per pick, host time included" % (len(sc.faces), W, H),
            "picks_equal_mirror": ok, "cursors_with_a_hit": n_hit, "b32_pick_meshes": d, "host_pick_mesh_numpy": h,
            "host_over_device": round(h["median_ms"] / d["median_ms"], 1),
            "pick_and_resolve_kernels_ms": [None if k is None else round(float(k), 4) for k in kern]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "pick_time.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bonnie32_amd import abi
    out = {"tool": "tools/pick_time.py", "digest": abi.check_build_digest(), "a_placed_console_frame": console(a.reps), "b_c3_mesh": big(a.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
