"""What building the mirrored half on the device costs and what it leaves alone, host time included on every side, every configuration
checked against the CPU oracle on the mirror-built arrays before it is timed:
  (a) the modeler's frame with mirror editing on: a rigged mesh drawn and delivered every frame (b32_fb_download_async + tickets, the
      presenter one frame behind), another bone table every frame --
        b32_scene_pose(src) + b32_scene_build_mirror(src, dst) + draw dst                     against
        pose_vertices + mirror_mesh on the host + b32_scene_upload of the doubled mesh + b32_scene_set_rig + draw   (what a caller had
        to do before; this build)
      medians of the windows, for obj-warrior at 640x480 and for the C2 mesh (300 000 vertices, 320x240), the whole mesh mirrored.  The
      host side's mirror_mesh is the numpy mirror; its share is timed alone and reported beside the frame.
  (b) the unchanged delivered console frame (tools/placed_frame.py's 12 rooms, none of the new code): this build and (--parent-lib PATH)
      the parent commit's library, alternately, each repetition a process of its own.
Acceptance of (b): this build's run medians lie inside the parent's own run-to-run range; one outside is reported with its distance.
usage: python tools/mirror_time.py [--parent-lib PATH] [--out profiles/mirror_time.json] [--reps 3] [--alternations 3] [--frames 1000]"""
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
from tools.pose_time import bones as pose_bones

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden", "scenes", "real")


def modeler(name, sc, scale, reps, n_device, n_host):
    import bonnie32_amd as b32
    from bonnie32_amd import mirror_edit as ME, rasterizer as R
    from oracle import oracle as O
    W, H = sc.width, sc.height
    nv, nf = len(sc.vertices), len(sc.faces)
    bo = (np.arange(nv) // 3 % 7).astype(np.uint16)                             # 5, 6: past the pose table
    n_tab = max(n_device, n_host, 8)
    tables = [pose_bones(i, scale) for i in range(n_tab)]
    mirror = ME.Mirror(b32.abi.MIRROR_X, 0, nv, 0, nf)
    m = mirror.pack()
    rest = R.rest_stream(sc.vertices)
    faces = np.ascontiguousarray(sc.faces, b32.abi.FACE_DTYPE)
    tex, _keep = b32.rtypes.pack_textures(sc.textures)
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    src = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    src.set_rig(bo)
    dst = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)              # the context's scene: what the frame draws
    ME.build_mirror(dst, src, mirror)                                           # (dst's buffers grow and src's faces reach the host here, before any window)
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
        src.pose(tables[i])
        assert lib.b32_scene_build_mirror(h, src._slot, None, m.ctypes.data) == 0
        fb.clear(sc.clear_color)
        dst.render_async(sc.camera, sc.settings) if i == 0 else dst.render_async()
        deliver(i)

    def built(i):
        return ME.mirror_mesh(R.pose_vertices(sc.vertices, bo, tables[i]), faces, mirror, rest, bo, tables[i])

    bo2 = np.concatenate([bo, bo])

    def host_frame(i):
        v, f = built(i)
        assert lib.b32_scene_upload(h, v.ctypes.data, len(v), f.ctypes.data, len(f), C.cast(tex, C.c_void_p), len(sc.textures)) == 0
        assert lib.b32_scene_set_rig(h, None, bo2.ctypes.data) == 0            # (the upload dropped the rig the hover's mirror test reads)
        fb.clear(sc.clear_color)
        dst.render_async(sc.camera, sc.settings) if i == 0 else dst.render_async()
        deliver(i)

    def oracle_frame(i):
        v, f = built(i)
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
    ms_dev = windows(device_frame, n_device)
    ok_host = checked(host_frame)                                               # (uploads into dst: this side runs last)
    ms_host = windows(host_frame, n_host)
    posed = R.pose_vertices(sc.vertices, bo, tables[0])
    t0 = time.perf_counter()
    for i in range(min(n_host, 8)):
        ME.mirror_mesh(posed, faces, mirror, rest, bo, tables[i])
    mirror_ms = (time.perf_counter() - t0) / min(n_host, 8) * 1e3
    for _, p in bufs:
        ctx.host_free(p)
    src.close()
    ctx.close()
    a, b = spread(ms_dev), spread(ms_host)
    return {"mesh": "%s, %d vertices, %d triangles, %dx%d, the whole mesh mirrored about X (%d vertices and %d faces drawn), 5 pose bones, another table every "
                    "frame, every frame delivered to page-locked host memory; ms per frame, host time included; windows of %d (device) / %d (host) frames"
                    % (name, nv, nf, W, H, 2 * nv, 2 * nf, n_device, n_host),
            "doubled_upload_bytes_per_frame": int(2 * nv * 36 + 2 * nf * 20),
            "frames_equal_oracle": bool(ok_dev and ok_host), "pose_build_mirror_and_draw": a, "host_pose_mirror_mesh_upload_set_rig_and_draw": b,
            "of_which_numpy_mirror_mesh_alone_ms": round(mirror_ms, 4), "host_over_device": round(b["median_ms"] / a["median_ms"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child"); ap.add_argument("--lib"); ap.add_argument("--parent-lib"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join("profiles", "mirror_time.json"))
    a = ap.parse_args()
    if a.child == "modeler":
        import __graft_entry__ as g
        g.build()
        from bonnie32_amd import scenefile, scenegen
        warrior = scenefile.read_scene(os.path.join(REAL, "obj-warrior.b32scene"))
        warrior.width, warrior.height = 640, 480
        c2 = scenegen.make_scene("C2")
        res = {"obj_warrior": modeler("obj-warrior", warrior, 1000.0, a.reps, a.frames, max(a.frames // 5, 8)),
               "c2_mesh": modeler("C2", c2, 3000.0, a.reps, max(a.frames // 2, 8), max(a.frames // 50, 8))}
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
            c["this_outside_parent_range_by_us"] = [round((x - hi if x > hi else x - lo) * 1e3, 2) for x in c["this"]["run_medians_ms"] if not lo <= x <= hi]
            c["this_median_minus_parent_median_us"] = round((sorted(c["this"]["run_medians_ms"])[len(runs["this"]) // 2] - sorted(c["parent"]["run_medians_ms"])[len(runs["parent"]) // 2]) * 1e3, 2)
            c["parent_own_spread_us"] = round((hi - lo) * 1e3, 2)
        return c

    me = os.path.abspath(__file__)
    out = {"tool": "tools/mirror_time.py", "a_modeler_frame_with_mirror_editing": run(me, "modeler")}
    out["b_console_frame_12_rooms_none_of_the_new_code"] = dict(alternate(os.path.join(ROOT, "tools", "placed_frame.py"), "rooms"),
                                                                frame="tools/placed_frame.py (c): 320x240, 12 resident rooms, b32_frame_submit, every frame delivered; windows of 2000 frames")
    out["digest"] = out["b_console_frame_12_rooms_none_of_the_new_code"]["this"]["digest"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
