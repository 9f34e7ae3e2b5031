"""What posing on the device costs and what it leaves alone, host time included on every side, every configuration checked against the CPU
oracle (or the host mirror) before it is timed:
  (a) a modeler-like frame: a rigged mesh drawn and delivered every frame (b32_fb_download_async + tickets, the presenter one frame behind),
      the bone table changing every frame --
        b32_scene_pose + draw                                      against
        pose_vertices on the host + b32_scene_upload + draw        (what a caller had to do before; on this same build)
      medians of three windows, for obj-warrior and for the C2 mesh (100 000 triangles).  The bone tables are worked out before the timing
      starts: both sides need the same ones.
  (b) the unchanged delivered console frame (tools/placed_frame.py's 12 rooms, no bones anywhere): this build and (--parent-lib PATH) the
      parent commit's library, alternately, each repetition a process of its own.
  (c) one blocking hover of obj-warrior WITHOUT a rig (the only existing kernel this feature touched), the two libraries the same way.
usage: python tools/pose_time.py [--parent-lib PATH] [--out profiles/pose_time.json] [--reps 3] [--alternations 3]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tools.hover_time import merge_quads, same
from tools.placed_frame import load, spread

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden", "scenes", "real")


def bones(t, scale):
    """Five bones at time t for a mesh of extent `scale`: three that rotate, two that take rotate_by_euler's early return."""
    from bonnie32_amd import rasterizer as R
    s = scale
    return R.pack_bones([R.Bone.from_euler((0.06 * s * np.sin(0.07 * t), 0.03 * s, -0.04 * s * np.cos(0.04 * t)), (6.0 + 20.0 * np.sin(0.05 * t), 0.0, -5.0 + 15.0 * np.cos(0.03 * t))),
                         R.Bone.from_euler((0.2 * s * np.sin(0.02 * t), -0.05 * s, 0.02 * s), (0.0004, 30.0, 0.0)),
                         R.Bone.from_euler((0.0, 0.0, 0.0), (-4.0 - 10.0 * np.sin(0.04 * t), 0.0, 3.0)),
                         R.Bone.from_euler((-0.1 * s, 0.02 * s * np.cos(0.06 * t), 0.05 * s), (12.0 * np.sin(0.09 * t), 0.0, 9.0)),
                         R.Bone.from_euler((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))])


def modeler(name, sc, scale, reps, n_pose, n_upload):
    import bonnie32_amd as b32
    from bonnie32_amd import rasterizer as R
    from oracle import oracle as O
    W, H = sc.width, sc.height
    bo = (np.arange(len(sc.vertices)) // 3 % 7).astype(np.uint16)              # 5, 6: past the table
    tables = [bones(i, scale) for i in range(max(n_pose, n_upload))]
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    rs.set_rig(bo)
    faces = np.ascontiguousarray(sc.faces, b32.abi.FACE_DTYPE)
    tex, _keep = b32.rtypes.pack_textures(sc.textures)
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    tickets = [0, 0]

    def deliver(i):
        tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
        if i > 0:
            ctx.ticket_wait(tickets[(i - 1) & 1])

    def drain(i):
        ctx.ticket_wait(tickets[i & 1]); ctx.finish()

    def posed_frame(i):
        rs.pose(tables[i])
        fb.clear(sc.clear_color)
        rs.render_async(sc.camera, sc.settings) if i == 0 else rs.render_async()
        deliver(i)

    def uploaded_frame(i):
        v = R.pose_vertices(sc.vertices, bo, tables[i])
        rc = ctx.lib.b32_scene_upload(ctx.h, v.ctypes.data, len(v), faces.ctypes.data, len(faces), C.cast(tex, C.c_void_p), len(sc.textures))
        assert rc == 0
        fb.clear(sc.clear_color)
        rs.render_async(sc.camera, sc.settings) if i == 0 else rs.render_async()
        deliver(i)

    def oracle_frame(i):
        ofb = O.Framebuffer(W, H); ofb.clear(sc.clear_color)
        assert O.render_mesh_15(ofb, R.pose_vertices(sc.vertices, bo, tables[i]), sc.faces, sc.textures, sc.camera, sc.settings)[0] == 0
        return ofb.pixels

    def checked(frame):
        ok = True
        for i in range(8):
            frame(i)
            if i in (1, 7):
                ctx.ticket_wait(tickets[(i - 1) & 1]); ok &= bool(np.array_equal(bufs[(i - 1) & 1][0], oracle_frame(i - 1)))
        drain(7)
        return ok

    def windows(frame, n):
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for i in range(n):
                frame(i)
            drain(n - 1)
            out.append((time.perf_counter() - t0) / n * 1e3)
        return out

    ok_pose = checked(posed_frame)
    ms_pose = windows(posed_frame, n_pose)
    ok_up = checked(uploaded_frame)                                              # (the upload dropped the rig: this side runs last)
    ms_up = windows(uploaded_frame, n_upload)
    for _, p in bufs:
        ctx.host_free(p)
    ctx.close()
    a, b = spread(ms_pose), spread(ms_up)
    return {"mesh": "%s, %d vertices, %d triangles, %dx%d, 5 bones, another table every frame, every frame delivered to page-locked host memory; "
                    "ms per frame, host time included; windows of %d (pose) / %d (host pose + upload) frames" % (name, len(sc.vertices), len(sc.faces), W, H, n_pose, n_upload),
            "frames_equal_oracle": bool(ok_pose and ok_up), "b32_scene_pose_and_draw": a, "host_pose_vertices_upload_and_draw": b,
            "upload_over_pose": round(b["median_ms"] / a["median_ms"], 2)}


def child_hover(lib_path, reps, n=2000):
    digest = load(lib_path)
    from bonnie32_amd import rasterizer as R, scenefile
    sc = scenefile.read_scene(os.path.join(REAL, "obj-warrior.b32scene"))
    W, H = sc.width, sc.height
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    top = R.Topology.from_polygons(merge_quads(sc.faces))
    mirror = R.HoverMirror(sc.vertices, top, None, sc.camera, W, H)
    ok_v = np.nonzero(mirror.some)[0]
    curs = [(float(mirror.sx[i]) + 1.5, float(mirror.sy[i]) - 1.0) for i in ok_v[(np.arange(12) * 19) % len(ok_v)]]
    ok = all(same(ctx.hover_mesh(rs, top, sc.camera, c, see_through=bool(k & 1), mirror_axis=k % 4), mirror.hover(*c, see_through=bool(k & 1), mirror_axis=k % 4))
             for k, c in enumerate(curs))
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for i in range(n):
            ctx.hover_mesh(rs, top, sc.camera, curs[i % 12], mirror_axis=1)
        ms.append((time.perf_counter() - t0) / n * 1e3)
    rs.close(); top.close(); ctx.close()
    print("RESULT " + json.dumps({"mode": "hover", "digest": digest, "exact": bool(ok), "ms": ms}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child"); ap.add_argument("--lib"); ap.add_argument("--parent-lib"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join("profiles", "pose_time.json"))
    a = ap.parse_args()
    if a.child == "hover":
        return child_hover(a.lib, a.reps)
    if a.child == "modeler":
        import __graft_entry__ as g
        g.build()
        from bonnie32_amd import scenefile, scenegen
        res = {"obj_warrior": modeler("obj-warrior", scenefile.read_scene(os.path.join(REAL, "obj-warrior.b32scene")), 1000.0, a.reps, a.frames, a.frames),
               "c2_mesh": modeler("C2", scenegen.make_scene("C2"), 3000.0, a.reps, a.frames, max(a.frames // 10, 8))}
        print("RESULT " + json.dumps(res))
        return

    def run(script, mode, lib=None):
        cmd = [sys.executable, script, "--child", mode, "--reps", str(a.reps)] + (["--lib", lib] if lib else [])
        if mode == "modeler":
            cmd += ["--frames", str(a.frames)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode:
            raise RuntimeError(f"{mode}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])

    def alternate(script, mode):
        runs = {"this": [], "parent": []}
        for _ in range(a.alternations):                       # alternately: parent, this, parent, this, ... each a fresh process
            if a.parent_lib:
                runs["parent"].append(run(script, mode, os.path.abspath(a.parent_lib)))
            runs["this"].append(run(script, mode))
        c = {}
        for who, rs in runs.items():
            if rs:
                c[who] = {"digest": rs[0]["digest"], "exact": all(r["exact"] for r in rs),
                          "run_medians_ms": [round(sorted(r["ms"])[len(r["ms"]) // 2], 5) for r in rs], "all_windows": spread([x for r in rs for x in r["ms"]])}
        if "parent" in c:
            lo, hi = min(c["parent"]["run_medians_ms"]), max(c["parent"]["run_medians_ms"])
            c["parent_range_ms"] = [lo, hi]
            c["this_within_parent_range"] = all(lo <= x <= hi for x in c["this"]["run_medians_ms"])
            c["this_median_minus_parent_median_us"] = round((sorted(c["this"]["run_medians_ms"])[len(runs["this"]) // 2] - sorted(c["parent"]["run_medians_ms"])[len(runs["parent"]) // 2]) * 1e3, 2)
            c["parent_own_spread_us"] = round((hi - lo) * 1e3, 2)
        return c

    me = os.path.abspath(__file__)
    out = {"tool": "tools/pose_time.py", "a_modeler_frame": run(me, "modeler")}
    out["b_console_frame_12_rooms_no_bones"] = dict(alternate(os.path.join(ROOT, "tools", "placed_frame.py"), "rooms"),
                                                    frame="tools/placed_frame.py (c): 320x240, 12 resident rooms, b32_frame_submit, every frame delivered; windows of 2000 frames")
    out["c_blocking_hover_obj_warrior_no_rig"] = dict(alternate(me, "hover"), what="one b32_hover_mesh (mirror axis X, culling) per call, 640x480; ms per hover, host time included; windows of 2000 hovers")
    out["digest"] = out["b_console_frame_12_rooms_no_bones"]["this"]["digest"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
