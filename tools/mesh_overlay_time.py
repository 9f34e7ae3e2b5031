"""What the modeler's selection overlays cost when they are made on the device from the slot's resident vertices (b32_draw_mesh_overlay),
host time included on both sides, every configuration checked against the host mirror (rasterizer.mesh_overlay_records) before it is timed:
  (a) a delivered modeler frame of the rigged obj-warrior -- clear, b32_scene_pose with another bone table every frame, the mesh, ALL overlay
      sections (brackets, edges, dots, hovered face, selected polygons, face preview), b32_fb_download_async, the presenter one frame behind --
        b32_draw_mesh_overlay                                                  against
        b32_scene_read_vertices + mesh_overlay_records (numpy) + b32_draw_prims   (the host path, on this same build: the mirror already
                                                                                   projects, so its records go to b32_draw_prims directly)
      medians of three windows.
  (b) the same for the C2 mesh (100 000 triangles, 300 000 vertices, the trivial topology of its triangles).
  (c) the unchanged 12-room delivered frame of tools/placed_frame.py, which runs none of the new code: this library and (--parent-lib PATH)
      the parent commit's, alternately, each repetition a process of its own; this build's median must lie inside the parent's own range or
      above its slowest run by no more than the parent's own spread.
usage: python tools/mesh_overlay_time.py [--parent-lib PATH] [--out profiles/mesh_overlay_time.json] [--reps 3] [--alternations 3]"""
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
from tools.placed_frame import alternate, spread
from tools.pose_time import bones

REAL = os.path.join(ROOT, "tests", "golden", "scenes", "real")


def modeler(name, sc, polys, scale, reps, n_dev, n_host):
    import bonnie32_amd as b32
    from bonnie32_amd import abi, rasterizer as R
    from bonnie32_amd.mirrors.screen import _project_f32
    W, H = sc.width, sc.height
    bo = (np.arange(len(sc.vertices)) // 3 % 7).astype(np.uint16)              # 5, 6: past the table
    tables = [bones(i, scale) for i in range(max(n_dev, n_host, 4))]
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    rs.set_rig(bo)
    top = R.Topology.from_polygons(polys) if polys is not None else R.Topology.triangles(sc.faces)
    with np.errstate(all="ignore"):
        sx, _, _, some = _project_f32(sc.vertices["pos"][:, 0], sc.vertices["pos"][:, 1], sc.vertices["pos"][:, 2], sc.camera, W, H, None)
    rect = (0.0, 0.0, float(np.median(sx[some])), float(H))
    quad = next((i for i in range(top.np) if top.count[i] == 4), 0)
    ov = R.MeshOverlay(abi.OVERLAY_ALL, hover_face=quad, select_kind=abi.SELECT_POLYGONS, preview_mode=abi.PREVIEW_FACE, rect=rect)
    sel = np.arange(0, top.np, 2, dtype=np.uint32)
    n_records = R.mesh_overlay_record_count(top, len(sc.vertices), ov, sel)
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    tickets = [0, 0]

    def frame(i, device):
        fb.clear(sc.clear_color)
        rs.pose(tables[i % len(tables)])
        rs.render_async(sc.camera, sc.settings) if i == 0 else rs.render_async()
        if device:
            fb.draw_mesh_overlay(rs, top, ov, sc.camera, None, sel)
        else:
            fb.draw_prims(R.mesh_overlay_records(rs.read_vertices(), top, ov, sel, sc.camera, W, H))
        tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
        if i > 0:
            ctx.ticket_wait(tickets[(i - 1) & 1])

    def drain(i):
        ctx.ticket_wait(tickets[i & 1]); ctx.finish()

    ok, moved = True, False
    frames = []
    for i in range(3):                                      # the two paths deliver the same frame, and the pose moves it
        frame(i, True); drain(i); dev = bufs[i & 1][0].copy()
        frame(i, False); drain(i)
        ok &= bool(np.array_equal(dev, bufs[i & 1][0]))
        frames.append(dev)
    moved = not np.array_equal(frames[0], frames[1])
    tap = fb.mesh_overlay_project_batch(rs, top, ov, sc.camera, None, sel)
    want = R.mesh_overlay_records(rs.read_vertices(), top, ov, sel, sc.camera, W, H)
    ok &= tap.tobytes() == want.tobytes()
    drawn = int((~((want["kind"] == abi.PRIM_CIRCLE) & (want["size"] == -1))).sum())
    ms = {True: [], False: []}
    for _ in range(reps):                                   # alternately in one process: host, device, host, device, ...
        for device, n in ((False, n_host), (True, n_dev)):
            frame(0, device); drain(0)
            t0 = time.perf_counter()
            for i in range(n):
                frame(i, device)
            drain(n - 1)
            ms[device].append((time.perf_counter() - t0) / n * 1e3)
    for _, p in bufs:
        ctx.host_free(p)
    top.close(); rs.close(); ctx.close()
    d, h = spread(ms[True]), spread(ms[False])
    return {"frame": "%s, %dx%d, %d vertices, %d polygons; another bone table every frame; all overlay sections: %d records of which %d draw; every "
                     "frame delivered to page-locked host memory; ms per frame, host time included; windows of %d (device) / %d (host) frames, alternately"
                     % (name, W, H, len(sc.vertices), top.np, n_records, drawn, n_dev, n_host),
            "device_equals_host_path_and_tap_equals_mirror": ok, "pose_moves_the_frame": bool(moved),
            "b32_draw_mesh_overlay": d, "read_vertices_mirror_draw_prims": h, "host_over_device": round(h["median_ms"] / d["median_ms"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join("profiles", "mesh_overlay_time.json"))
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
    c2 = scenegen.make_scene("C2")
    out = {"tool": "tools/mesh_overlay_time.py", "digest": abi.check_build_digest(),
           "a_obj_warrior": modeler("obj-warrior", warrior, merge_quads(warrior.faces), 1000.0, a.reps, 300, 20),
           "b_c2": modeler("C2", c2, None, 3000.0, a.reps, 30, 2)}
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
