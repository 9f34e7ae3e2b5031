"""What the world editor's object overlays cost when the records are made on the device from resident asset parts (b32_draw_object_overlays)
and when the host makes them (the ends placed in numpy, B32WorldItems through b32_draw_world, the bounds reduced in numpy, twelve
B32_GIZMO_LINE items through b32_draw_gizmos), host time included on both sides, every configuration checked against the mirror before it
is timed; medians of three windows:
  (a) the editor's drag frame: the delivered 12-room placed console frame of tools/placed_frame.py (12 resident rooms + 24 placed
      instances) plus the drag preview of obj-warrior (OBJECT_WIRE over its merged-quad topology) and one OBJECT_BOX_MESH, another
      placement every frame, waited one frame behind.
  (b) the C2 mesh (300 000 vertices) with the trivial topology of its triangles (300 000 half-edges) as ONE wire item, a synchronisation
      per overlay.
  (c) k_scene_bounds on the 300 000 vertices through b32_scene_bounds: the first call after a one-vertex patch (which clears the cache)
      against the patch and a synchronisation alone, and the second call of the same frame (cache hit: no reduction).
  (d) the unchanged 12-room delivered frame, which runs none of the new code: this library and (--parent-lib PATH) the parent commit's,
      alternately, each repetition a process of its own with three 2000-frame windows.
usage: python tools/object_overlay_time.py [--parent-lib PATH] [--out profiles/object_overlay_time.json] [--reps 3] [--alternations 3]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from tools.hover_time import merge_quads
from tools.placed_frame import alternate, placements, scene, spread

REAL = os.path.join(ROOT, "tests", "golden", "scenes", "real")
f32 = np.float32


def host_items(pos, top, place, color):
    """What a host without the call builds per frame: (the wire's B32WorldItems, the box's twelve B32GizmoItems)."""
    from bonnie32_amd import abi
    from bonnie32_amd.mirrors import overlays as R
    from bonnie32_amd.records import _placement_triple
    c, s, wp = _placement_triple(place)
    P = R._object_place(pos, c, s, wp)
    wire = np.zeros(len(top.poly_verts), abi.WORLD_ITEM_DTYPE)
    wire["p0"], wire["p1"] = P[top.he_v0], P[top.he_v1]
    wire["r"], wire["g"], wire["b"], wire["blend"] = color.r, color.g, color.b, color.blend
    wire["kind"], wire["alpha"], wire["flags"] = abi.LINE_2D, 255, abi.WORLD_CLIP_NEAR
    mn, mx, _ = R.mesh_bounds([pos])
    corners = R._object_place(np.where(R._OBJECT_BOX_CORNERS, mx, mn).astype(f32), c, s, wp)
    box = np.zeros(12, abi.GIZMO_ITEM_DTYPE)
    box["p0"] = corners[[e[0] for e in R._OBJECT_BOX_EDGES]]; box["p1"] = corners[[e[1] for e in R._OBJECT_BOX_EDGES]]
    box["r"], box["g"], box["b"], box["kind"] = 255, 200, 50, abi.GIZMO_LINE
    return wire, box


def drag_frames(warrior, reps, n_frames):
    import bonnie32_amd as b32
    from bonnie32_amd import abi, rasterizer as R
    rooms, parts, st, fog, clear = scene()
    W, H, cam = rooms[0].width, rooms[0].height, rooms[0].camera
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    room_slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in rooms]
    part_slots = [R.ResidentScene(fb, p.vertices, p.faces, p.textures).detach() for p in parts]
    table = ctx.make_frame_table(cam, st, room_slots + part_slots * 8, fogs=[fog] * 36, placements=[None] * 36)
    pos = np.ascontiguousarray(warrior.vertices["pos"], f32)
    pos = ((pos - pos.mean(axis=0, dtype=np.float64).astype(f32)) * f32(60.0 / np.abs(pos).max())).astype(f32)     # an asset's local space, as placed_frame's parts
    wv = warrior.vertices.copy(); wv["pos"] = pos
    top = R.Topology.from_polygons(merge_quads(warrior.faces))
    slot = R.ResidentScene(fb, wv, warrior.faces, warrior.textures).detach()
    dev_parts = [R.ObjectPart(slot, top, True, pos)]
    cyan, yellow = b32.Color(100, 200, 255), b32.Color(255, 200, 50)
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    tickets = [0, 0]

    def place(i):
        a = f32(0.03 * i)
        return (float(np.cos(a)), float(np.sin(a)), (-20.0 + 0.3 * (i % 120), -10.0, 230.0 + 0.2 * (i % 90)))

    def head(i):
        pls = placements(i)
        ctx.set_table_placements(table, [None] * 12 + [pls[k] for k in range(8) for _ in range(3)])
        fb.clear(clear); ctx.frame_submit(table)

    def deliver(i):
        tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
        if i > 0:
            ctx.ticket_wait(tickets[(i - 1) & 1])

    def items_of(i):
        return [R.ObjectItem(abi.OBJECT_WIRE, place(i), 0, 1, cyan), R.ObjectItem(abi.OBJECT_BOX_MESH, place(i), 0, 1, yellow)]

    def device_frame(i):
        head(i)
        fb.draw_object_overlays(dev_parts, items_of(i), cam)
        deliver(i)

    def host_frame(i):
        head(i)
        wire, box = host_items(pos, top, place(i), cyan)
        fb.draw_world(wire, cam); fb.draw_gizmos(box, cam)
        deliver(i)

    def drain(i):
        ctx.ticket_wait(tickets[i & 1]); ctx.finish()

    ok, drawing = True, 0
    for i in (0, 7, 33):                                    # the two paths deliver the same bytes, and the tap is the mirror's
        device_frame(i); drain(i)
        dev = bufs[i & 1][0].copy()
        tap = fb.object_overlay_project_batch(dev_parts, items_of(i), cam)
        ok &= tap.tobytes() == R.object_overlay_records(dev_parts, items_of(i), cam, W, H).tobytes()
        drawing = int((tap["kind"] != abi.PRIM_CIRCLE).sum())
        host_frame(i); drain(i)
        ok &= bool(np.array_equal(dev, bufs[i & 1][0]))
    ms = {"device": [], "host": []}
    for _ in range(reps):
        for how, frame, frames in (("device", device_frame, n_frames), ("host", host_frame, max(50, n_frames // 4))):
            t0 = time.perf_counter()
            for i in range(frames):
                frame(i)
            drain(frames - 1)
            ms[how].append((time.perf_counter() - t0) / frames * 1e3)
    n_records = len(top.poly_verts) + 12
    reductions = ctx.route_counts()["bounds_reductions"]    # (one: the slot's vertices never change)
    for _, p in bufs:
        ctx.host_free(p)
    ctx.close()
    d, h = spread(ms["device"]), spread(ms["host"])
    return {"frame": "%dx%d, 12 resident rooms + 24 placed instances + the drag preview of obj-warrior (%d half-edges) and its mesh box: %d records, %d of them "
                     "drawing in the last checked frame; another placement every frame, every frame delivered to page-locked host memory and waited one frame "
                     "behind; ms per frame, host time included" % (W, H, len(top.poly_verts), n_records, drawing),
            "paths_equal_mirror_and_each_other": bool(ok), "b32_draw_object_overlays": d, "numpy_place_draw_world_numpy_bounds_draw_gizmos": h,
            "host_over_device": round(h["median_ms"] / d["median_ms"], 2), "bounds_reductions_launched": reductions}


def c2_wire(c2, reps):
    import bonnie32_amd as b32
    from bonnie32_amd import abi, rasterizer as R
    W, H, cam = c2.width, c2.height, c2.camera
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    pos = np.ascontiguousarray(c2.vertices["pos"], f32)
    top = R.Topology.triangles(c2.faces)
    slot = R.ResidentScene(fb, c2.vertices, c2.faces, c2.textures).detach()
    parts = [R.ObjectPart(slot, top, True, pos)]
    place = (float(np.cos(f32(0.2))), float(np.sin(f32(0.2))), (0.0, 0.0, 0.0))
    green = b32.Color(100, 255, 100)
    items = [R.ObjectItem(abi.OBJECT_WIRE, place, 0, 1, green)]
    want = R.object_overlay_records(parts, items, cam, W, H)
    ok = fb.object_overlay_project_batch(parts, items, cam).tobytes() == want.tobytes()
    fb.clear(b32.Color(0, 0, 0)); fb.draw_object_overlays(parts, items, cam); a = fb.pixels
    wire, _ = host_items(pos, top, place, green)
    fb.clear(b32.Color(0, 0, 0)); fb.draw_world(wire, cam); ok &= bool(np.array_equal(a, fb.pixels))

    def device():
        fb.draw_object_overlays(parts, items, cam)
        ctx.synchronize()

    def host():
        w_, _ = host_items(pos, top, place, green)
        fb.draw_world(w_, cam)
        ctx.synchronize()

    out = {"mesh": "C2, %d vertices, %d half-edges as one wire item at %dx%d: %d records of which %d draw; a synchronisation per overlay; ms per overlay, host time included"
                   % (len(pos), len(top.poly_verts), W, H, len(want), int((want["kind"] != abi.PRIM_CIRCLE).sum())), "equal_mirror_and_draw_world": bool(ok)}
    for key, fn, k in (("b32_draw_object_overlays", device, 20), ("numpy_place_draw_world", host, 3)):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            ts.append((time.perf_counter() - t0) / k * 1e3)
        out[key] = spread(ts)
    out["host_over_device"] = round(out["numpy_place_draw_world"]["median_ms"] / out["b32_draw_object_overlays"]["median_ms"], 2)

    # (c) the bounds of the same 300 000 vertices
    mn, mx, _ = R.mesh_bounds([pos])
    gmn, gmx, has = slot.bounds()
    bounds_ok = gmn.tobytes() == mn.tobytes() and gmx.tobytes() == mx.tobytes() and has
    one = c2.vertices[:1].copy()

    def stale():
        slot.patch_vertices([0], one)                       # the same record again: the vertices "moved", the answer stays
        slot.bounds()

    def patch_only():
        slot.patch_vertices([0], one)
        ctx.synchronize()

    def cached():
        slot.bounds()

    r0 = ctx.route_counts()["bounds_reductions"]
    b = {"equal_mesh_bounds": bool(bounds_ok)}
    for key, fn, k in (("patch_one_vertex_then_b32_scene_bounds", stale, 50), ("patch_one_vertex_then_synchronize", patch_only, 50), ("b32_scene_bounds_cache_hit", cached, 50)):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            ts.append((time.perf_counter() - t0) / k * 1e3)
        b[key] = spread(ts)
    b["reductions_launched"] = ctx.route_counts()["bounds_reductions"] - r0
    b["expected_reductions"] = (reps * 50 + 1) + 1           # every stale() call, and the first cached() behind the last patch_only()
    b["numpy_mesh_bounds_ms"] = spread([_timed(lambda: R.mesh_bounds([pos])) for _ in range(reps)])
    ctx.close()
    return out, b


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--parent-lib")
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--out", default=os.path.join("profiles", "object_overlay_time.json"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bonnie32_amd import abi, scenefile, scenegen

    def run(mode, lib=None):                                # a fresh process of tools/placed_frame.py per repetition
        cmd = [sys.executable, os.path.join(ROOT, "tools", "placed_frame.py"), "--child", mode, "--reps", str(a.reps)] + (["--lib", lib] if lib else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode:
            raise RuntimeError(f"{mode}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    warrior = scenefile.read_scene(os.path.join(REAL, "obj-warrior.b32scene"))
    out = {"tool": "tools/object_overlay_time.py", "digest": abi.check_build_digest(), "a_editor_drag_frame": drag_frames(warrior, a.reps, a.frames)}
    print("(a) done", file=sys.stderr, flush=True)
    out["b_c2_wire"], out["c_scene_bounds_300000_vertices"] = c2_wire(scenegen.make_scene("C2"), a.reps)
    print("(b), (c) done", file=sys.stderr, flush=True)
    c = alternate(a, run, "rooms")
    if "parent" in c:
        lo, hi = c["parent_spread_ms"]
        c["this_outside_parent_range_by_ms"] = [round(x - hi if x > hi else (x - lo if x < lo else 0.0), 4) for x in c["this"]["run_medians_ms"]]
    out["d_rooms_only_unchanged_frame"] = c
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
