"""What building the bone octahedra on the device costs and what it leaves alone, host time included on every side, every configuration
checked against the CPU oracle on (posed body + mirror tail) as ONE mesh before it is timed:
  (a) the modeler's frame with bones shown: a rigged mesh drawn and delivered every frame (b32_fb_download_async + tickets, the presenter
      one frame behind), the bone table changing every frame --
        b32_scene_pose + b32_scene_build_skeleton + draw                                      against
        pose_vertices + skeleton_mesh on the host + b32_scene_upload of the combined mesh + draw   (what a caller had to do before; this build)
      medians of the windows, for obj-warrior at 640x480 with 20 bones and for the C2 mesh (300 000 vertices) with 64 bones.  The tables
      are worked out before the timing starts: both sides need the same ones.  The host side's skeleton_mesh is the numpy mirror, a scalar
      loop; its share is timed alone and reported beside the frame, so that a reader can take it out.
  (b) the unchanged delivered console frame (tools/placed_frame.py's 12 rooms, no bones anywhere): this build and (--parent-lib PATH) the
      parent commit's library, alternately, each repetition a process of its own.
  (c) one blocking hover of obj-warrior without a tail (tools/pose_time.py's): a path whose host-side counts this feature touches, the two
      libraries the same way.
Acceptance of (b) and (c): this build's run medians lie inside the parent's own run-to-run range.
usage: python tools/skeleton_time.py [--parent-lib PATH] [--out profiles/skeleton_time.json] [--reps 3] [--alternations 3] [--frames 1000]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tools.placed_frame import spread
from tools.pose_time import bones as pose_bones, child_hover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden", "scenes", "real")


def skeleton(t, scale, n):
    """n bones at time t for a mesh of extent `scale`: a root and chains of four, every rotation moving; every eighth width is 0
    (display_width resolves it)."""
    from bonnie32_amd import rasterizer as R
    s = scale
    out = []
    for k in range(n):
        pos = (0.3 * s * np.sin(0.9 * k) + 0.02 * s * np.sin(0.05 * t + k), 0.35 * s * np.cos(0.7 * k) + 0.01 * s * np.cos(0.03 * t), 0.25 * s * np.sin(0.4 * k + 1.0))
        rot = (40.0 * np.sin(0.04 * t + 0.5 * k), 0.0, 170.0 * np.cos(0.03 * t + 0.3 * k))
        out.append(R.SkelBone.from_rig(pos, rot, (0.08 + 0.01 * (k % 5)) * s, 0.0 if k % 8 == 0 else 0.012 * s, None if k % 4 == 0 else k - 1))
    return R.pack_skel_bones(out)


def modeler(name, sc, scale, n_bones, reps, n_device, n_host):
    import bonnie32_amd as b32
    from bonnie32_amd import rasterizer as R
    from oracle import oracle as O
    W, H = sc.width, sc.height
    nv = len(sc.vertices)
    bo = (np.arange(nv) // 3 % 7).astype(np.uint16)                             # 5, 6: past the pose table
    n_tab = max(n_device, n_host, 8)
    tables = [pose_bones(i, scale) for i in range(n_tab)]
    skels = [skeleton(i, scale, n_bones) for i in range(n_tab)]
    style = R.SkeletonStyle(selected_bone=1, hovered_bone=2, editor_alpha=180)  # the selected bone opaque-ish, the others dimmed to 30
    st = style.pack()
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    rs.set_rig(bo)
    rs.build_skeleton(skels[0], style)                                          # (the slot's buffers grow here, before any window)
    faces = np.ascontiguousarray(sc.faces, b32.abi.FACE_DTYPE)
    tex, _keep = b32.rtypes.pack_textures(sc.textures)
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    tickets = [0, 0]
    lib, h = ctx.lib, ctx.h

    def deliver(i):
        tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
        if i > 0:
            ctx.ticket_wait(tickets[(i - 1) & 1])

    def drain(i):
        ctx.ticket_wait(tickets[i & 1]); ctx.finish()

    def device_frame(i):
        rs.pose(tables[i])
        assert lib.b32_scene_build_skeleton(h, None, skels[i].ctypes.data, len(skels[i]), st.ctypes.data) == 0
        fb.clear(sc.clear_color)
        rs.render_async(sc.camera, sc.settings) if i == 0 else rs.render_async()
        deliver(i)

    def combined(i):
        body = R.pose_vertices(sc.vertices, bo, tables[i])
        tv, tf = R.skeleton_mesh(skels[i], style, nv)
        return np.concatenate([body, tv]), np.concatenate([faces, tf])

    def host_frame(i):
        v, f = combined(i)
        assert lib.b32_scene_upload(h, v.ctypes.data, len(v), f.ctypes.data, len(f), C.cast(tex, C.c_void_p), len(sc.textures)) == 0
        fb.clear(sc.clear_color)
        rs.render_async(sc.camera, sc.settings) if i == 0 else rs.render_async()
        deliver(i)

    def oracle_frame(i):
        v, f = combined(i)
        ofb = O.Framebuffer(W, H); ofb.clear(sc.clear_color)
        assert O.render_mesh_15(ofb, v, f, sc.textures, sc.camera, sc.settings)[0] == 0
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

    ok_dev = checked(device_frame)
    tail = R.skeleton_mesh(skels[7], style, nv)
    ms_dev = windows(device_frame, n_device)
    ok_host = checked(host_frame)                                               # (the upload dropped rig and tail: this side runs last)
    ms_host = windows(host_frame, n_host)
    t0 = time.perf_counter()
    for i in range(min(n_host, 8)):
        R.skeleton_mesh(skels[i], style, nv)
    mirror_ms = (time.perf_counter() - t0) / min(n_host, 8) * 1e3
    for _, p in bufs:
        ctx.host_free(p)
    ctx.close()
    a, b = spread(ms_dev), spread(ms_host)
    return {"mesh": "%s, %d vertices, %d triangles, %dx%d, %d bones shown (%d octahedra drawn, %d tail faces), 5 pose bones, another table every frame, every frame "
                    "delivered to page-locked host memory; ms per frame, host time included; windows of %d (device) / %d (host) frames"
                    % (name, nv, len(sc.faces), W, H, n_bones, len(tail[1]) // 8, len(tail[1]), n_device, n_host),
            "combined_upload_bytes_per_frame": int((nv + len(tail[0])) * 36 + (len(faces) + len(tail[1])) * 20),
            "frames_equal_oracle": bool(ok_dev and ok_host), "pose_build_skeleton_and_draw": a, "host_pose_skeleton_mesh_upload_and_draw": b,
            "of_which_numpy_skeleton_mesh_alone_ms": round(mirror_ms, 4), "host_over_device": round(b["median_ms"] / a["median_ms"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child"); ap.add_argument("--lib"); ap.add_argument("--parent-lib"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join("profiles", "skeleton_time.json"))
    a = ap.parse_args()
    if a.child == "hover":
        return child_hover(a.lib, a.reps)
    if a.child == "modeler":
        import __graft_entry__ as g
        g.build()
        from bonnie32_amd import scenefile, scenegen
        warrior = scenefile.read_scene(os.path.join(REAL, "obj-warrior.b32scene"))
        warrior.width, warrior.height = 640, 480
        c2 = scenegen.make_scene("C2")
        res = {"obj_warrior_20_bones": modeler("obj-warrior", warrior, 1000.0, 20, a.reps, a.frames, max(a.frames // 5, 8)),
               "c2_mesh_64_bones": modeler("C2", c2, 3000.0, 64, a.reps, a.frames, max(a.frames // 50, 8))}
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
    out = {"tool": "tools/skeleton_time.py", "a_modeler_frame_with_bones": run(me, "modeler")}
    out["b_console_frame_12_rooms_no_bones"] = dict(alternate(os.path.join(ROOT, "tools", "placed_frame.py"), "rooms"),
                                                    frame="tools/placed_frame.py (c): 320x240, 12 resident rooms, b32_frame_submit, every frame delivered; windows of 2000 frames")
    out["c_blocking_hover_obj_warrior_no_tail"] = dict(alternate(me, "hover"), what="one b32_hover_mesh (mirror axis X, culling) per call, 640x480; ms per hover, host time included; windows of 2000 hovers")
    out["digest"] = out["b_console_frame_12_rooms_no_bones"]["this"]["digest"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
