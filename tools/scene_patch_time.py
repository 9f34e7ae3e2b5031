"""What editing a resident scene in place costs against uploading it again, host time included on both sides, every configuration checked
against the CPU oracle on the host-patched arrays before it is timed.  Every frame is delivered (b32_fb_download_async + tickets, the
presenter one frame behind); medians of the windows.
  (a) drag frame, obj-warrior: the rigged obj-warrior at 640x480, 16 vertices edited per frame --
        b32_scene_patch_vertices + draw                              against
        b32_scene_upload + b32_scene_set_rig + b32_scene_pose + draw   (what a caller had to do before; this build)
  (b) drag frame, C2: the same for the C2 mesh (300 000 vertices) with 1 000 vertices per frame.
  (c) paint stroke: an 8x8 b32_scene_patch_indexed per frame into a 256x256 atlas, against b32_scene_upload_indexed per frame.
  (d) opacity drag: every face of obj-warrior patched per frame (b32_scene_patch_faces), against b32_scene_upload per frame.
  (e) the unchanged delivered console frame (tools/placed_frame.py's 12 rooms, which runs none of the new code): this build and
      (--parent-lib PATH) the parent commit's library, alternately, each repetition a process of its own.  The yardstick is the parent's
      own run-to-run range.
usage: python tools/scene_patch_time.py [--parent-lib PATH] [--out profiles/scene_patch_time.json] [--reps 3] [--alternations 3] [--frames 1000]"""
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
TAB = 8         # edits are worked out for this many frames before the timing starts and repeat from there: both sides need the same ones


class Bench:
    """One context, one resident scene, frames delivered by ticket."""

    def __init__(self, sc, reps):
        from bonnie32_amd import rasterizer as R
        self.sc, self.reps = sc, reps
        self.ctx = R.Context(0)
        self.fb = R.Framebuffer(sc.width, sc.height, self.ctx)
        self.bufs = [self.ctx.host_alloc(sc.width * sc.height * 4) for _ in range(2)]
        self.tickets = [0, 0]
        self.rs = None

    def draw_and_deliver(self, i):
        self.fb.clear(self.sc.clear_color)
        self.rs.render_async(self.sc.camera, self.sc.settings, getattr(self.sc, "fog", None)) if i == 0 else self.rs.render_async()
        self.tickets[i & 1] = self.ctx.download_async(self.bufs[i & 1][1])
        if i > 0:
            self.ctx.ticket_wait(self.tickets[(i - 1) & 1])

    def drain(self, i):
        self.ctx.ticket_wait(self.tickets[i & 1]); self.ctx.finish()

    def checked(self, frame, oracle_pixels):
        ok = True
        for i in range(TAB):
            frame(i)
            self.draw_and_deliver(i)
            if i in (1, TAB - 1):
                self.ctx.ticket_wait(self.tickets[(i - 1) & 1])
                ok &= bool(np.array_equal(self.bufs[(i - 1) & 1][0], oracle_pixels(i - 1).reshape(-1).view(np.uint8)))
        self.drain(TAB - 1)
        return ok

    def windows(self, frame, n):
        out = []
        for _ in range(self.reps):
            t0 = time.perf_counter()
            for i in range(n):
                frame(i % TAB)
                self.draw_and_deliver(i)
            self.drain(n - 1)
            out.append((time.perf_counter() - t0) / n * 1e3)
        return out

    def close(self):
        for _, p in self.bufs:
            self.ctx.host_free(p)
        self.ctx.close()


def oracle_15(sc, v, f, textures):
    from oracle import oracle as O
    ofb = O.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    assert O.render_mesh_15(ofb, v, f, textures, sc.camera, sc.settings, getattr(sc, "fog", None))[0] == 0
    return ofb.pixels


def drag(name, sc, scale, n_edit, reps, n_patch, n_upload):
    import bonnie32_amd as b32
    from bonnie32_amd import rasterizer as R
    nv = len(sc.vertices)
    bo = (np.arange(nv) // 3 % 7).astype(np.uint16)                             # 5, 6: past the pose table
    table = pose_bones(3, scale)
    idx = np.unique(np.linspace(0, nv - 1, n_edit).astype(np.uint32))
    rng = np.random.default_rng(1)
    recs = []
    for i in range(TAB):
        r = np.zeros(len(idx), b32.abi.VERTEX_PATCH_DTYPE)
        r["index"] = idx; r["v"] = sc.vertices[idx]
        r["v"]["pos"] += (rng.standard_normal((len(idx), 3)) * 0.01 * scale).astype(np.float32)
        recs.append(r)
    rests = [R.patch_vertices(sc.vertices, idx, r["v"]) for r in recs]           # (absolute positions: frame i does not depend on frame i - 1)
    faces = np.ascontiguousarray(sc.faces, b32.abi.FACE_DTYPE)
    tex, _keep = b32.rtypes.pack_textures(sc.textures)
    B = Bench(sc, reps)
    lib, h = B.ctx.lib, B.ctx.h
    B.rs = R.ResidentScene(B.fb, sc.vertices, sc.faces, sc.textures)
    B.rs.set_rig(bo); B.rs.pose(table)

    def patch_frame(i):
        assert lib.b32_scene_patch_vertices(h, None, recs[i].ctypes.data, len(idx)) == 0

    def upload_frame(i):
        v = rests[i]
        assert lib.b32_scene_upload(h, v.ctypes.data, nv, faces.ctypes.data, len(faces), C.cast(tex, C.c_void_p), len(sc.textures)) == 0
        assert lib.b32_scene_set_rig(h, None, bo.ctypes.data) == 0 and lib.b32_scene_pose(h, None, table.ctypes.data, len(table)) == 0

    want = lambda i: oracle_15(sc, R.pose_vertices(rests[i], bo, table), sc.faces, sc.textures)
    ok = B.checked(patch_frame, want)
    a = spread(B.windows(patch_frame, n_patch))
    ok &= B.checked(upload_frame, want)
    b = spread(B.windows(upload_frame, n_upload))
    B.close()
    return {"mesh": "%s, %d vertices, %d triangles, %dx%d, rigged and posed, %d vertices edited per frame, every frame delivered to page-locked host memory; "
                    "ms per frame, host time included; windows of %d (patch) / %d (upload) frames" % (name, nv, len(faces), sc.width, sc.height, len(idx), n_patch, n_upload),
            "patch_bytes_per_frame": int(len(idx) * 40), "upload_bytes_per_frame": int(nv * 36 + len(faces) * 20 + nv * 2),
            "frames_equal_oracle": bool(ok), "patch_vertices_and_draw": a, "upload_set_rig_pose_and_draw": b, "upload_over_patch": round(b["median_ms"] / a["median_ms"], 2)}


def paint(reps, n_patch, n_upload):
    import bonnie32_amd as b32
    from bonnie32_amd import rasterizer as R, scenegen
    sc = scenegen.make_scene("C3", n_tris=20000, width=320, height=240, seed=24242)
    at = sc.indexed_textures[0]
    assert (at.width, at.height) == (256, 256) and len(sc.indexed_textures) == 1
    rng = np.random.default_rng(2)
    blocks = [rng.integers(0, at.clut.size, (8, 8)).astype(np.uint8) for _ in range(TAB)]
    spots = [(17 + 29 * i, 40 + 23 * i) for i in range(TAB)]
    atlases, cur = [], at.indices.reshape(256, 256).copy()
    texels = R.clut_lookup(at.clut, cur)
    for i in range(TAB):                                                        # (after one round every block is in place and the atlas repeats)
        texels, cur = R.patch_indexed(texels, cur, spots[i][0], spots[i][1], blocks[i], at.clut)
        atlases.append(cur.copy())
    final = atlases[-1]
    B = Bench(sc, reps)
    lib, h = B.ctx.lib, B.ctx.h
    B.rs = R.ResidentScene(B.fb, sc.vertices, sc.faces, indexed_textures=[at])
    v = np.ascontiguousarray(sc.vertices, b32.abi.VERTEX_DTYPE); f = np.ascontiguousarray(sc.faces, b32.abi.FACE_DTYPE)
    clut = np.ascontiguousarray(at.clut, np.uint16)
    before = B.ctx.route_counts()["lds_atlas"]

    def patch_frame(i):
        assert lib.b32_scene_patch_indexed(h, None, 0, spots[i][0], spots[i][1], 8, 8, blocks[i].ctypes.data, 8, clut.ctypes.data, len(clut)) == 0

    def upload_frame(i, table=atlases):
        t = b32.IndexedTexture(256, 256, table[i], at.clut, at.blend_mode)
        arr, _keep = b32.rtypes.pack_indexed_textures([t])
        assert lib.b32_scene_upload_indexed(h, v.ctypes.data, len(v), f.ctypes.data, len(f), C.cast(arr, C.c_void_p), 1) == 0

    want = lambda i: oracle_15(sc, sc.vertices, sc.faces, [b32.Texture15(256, 256, R.clut_lookup(at.clut, atlases[i]), at.blend_mode)])
    ok = B.checked(patch_frame, want)
    a = spread(B.windows(patch_frame, n_patch))
    lds = B.ctx.route_counts()["lds_atlas"] - before
    ok &= B.checked(upload_frame, want)
    b = spread(B.windows(lambda i: upload_frame(i, [final] * TAB), n_upload))
    B.close()
    return {"mesh": "C3, %d triangles, 320x240, one 256x256 8-bit index atlas kept for the LDS route, an 8x8 rectangle of indices edited per frame, every frame delivered; "
                    "ms per frame, host time included; windows of %d (patch) / %d (upload) frames" % (len(f), n_patch, n_upload),
            "patch_bytes_per_frame": 512 + 64, "upload_bytes_per_frame": int(256 * 256 + 512 + len(v) * 36 + len(f) * 20), "patched_frames_on_the_lds_route": int(lds),
            "frames_equal_oracle": bool(ok), "patch_indexed_and_draw": a, "upload_indexed_and_draw": b, "upload_over_patch": round(b["median_ms"] / a["median_ms"], 2)}


def opacity(sc, reps, n_patch, n_upload):
    import bonnie32_amd as b32
    from bonnie32_amd import rasterizer as R
    nf = len(sc.faces)
    recs, faces = [], []
    for i in range(TAB):
        r = np.zeros(nf, b32.abi.FACE_PATCH_DTYPE)
        r["index"] = np.arange(nf); r["f"] = sc.faces
        r["f"]["editor_alpha"] = 250 - 25 * i
        recs.append(r); faces.append(np.ascontiguousarray(r["f"]))
    v = np.ascontiguousarray(sc.vertices, b32.abi.VERTEX_DTYPE)
    tex, _keep = b32.rtypes.pack_textures(sc.textures)
    B = Bench(sc, reps)
    lib, h = B.ctx.lib, B.ctx.h
    B.rs = R.ResidentScene(B.fb, sc.vertices, sc.faces, sc.textures)

    def patch_frame(i):
        assert lib.b32_scene_patch_faces(h, None, recs[i].ctypes.data, nf) == 0

    def upload_frame(i):
        assert lib.b32_scene_upload(h, v.ctypes.data, len(v), faces[i].ctypes.data, nf, C.cast(tex, C.c_void_p), len(sc.textures)) == 0

    want = lambda i: oracle_15(sc, sc.vertices, faces[i], sc.textures)
    ok = B.checked(patch_frame, want)
    a = spread(B.windows(patch_frame, n_patch))
    ok &= B.checked(upload_frame, want)
    b = spread(B.windows(upload_frame, n_upload))
    B.close()
    return {"mesh": "obj-warrior, %d vertices, %d triangles, %dx%d, editor_alpha of every face edited per frame (every face in the transparent pass), every frame delivered; "
                    "ms per frame, host time included; windows of %d frames" % (len(v), nf, sc.width, sc.height, n_patch),
            "patch_bytes_per_frame": int(nf * 24), "upload_bytes_per_frame": int(len(v) * 36 + nf * 20),
            "frames_equal_oracle": bool(ok), "patch_faces_and_draw": a, "upload_and_draw": b, "upload_over_patch": round(b["median_ms"] / a["median_ms"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child"); ap.add_argument("--lib"); ap.add_argument("--parent-lib"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join("profiles", "scene_patch_time.json"))
    a = ap.parse_args()
    if a.child == "edits":
        import __graft_entry__ as g
        g.build()
        from bonnie32_amd import scenefile, scenegen
        warrior = scenefile.read_scene(os.path.join(REAL, "obj-warrior.b32scene"))
        warrior.width, warrior.height = 640, 480
        c2 = scenegen.make_scene("C2")
        n = a.frames
        res = {"a_drag_frame_obj_warrior_16_vertices": drag("obj-warrior", warrior, 1000.0, 16, a.reps, n, n),
               "b_drag_frame_c2_1000_vertices": drag("C2", c2, 3000.0, 1000, a.reps, n, max(n // 20, 8)),
               "c_paint_stroke_8x8_of_256x256": paint(a.reps, n, max(n // 4, 8)),
               "d_opacity_drag_obj_warrior_all_faces": opacity(warrior, a.reps, n, n)}
        print("RESULT " + json.dumps(res))
        return

    def run(script, mode, lib=None):
        cmd = [sys.executable, script, "--child", mode, "--reps", str(a.reps)] + (["--lib", lib] if lib else [])
        if mode == "edits":
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
    out = {"tool": "tools/scene_patch_time.py"}
    out.update(run(me, "edits"))
    out["e_console_frame_12_rooms_unchanged"] = dict(alternate(os.path.join(ROOT, "tools", "placed_frame.py"), "rooms"),
                                                     frame="tools/placed_frame.py (c): 320x240, 12 resident rooms, b32_frame_submit, every frame delivered; windows of 2000 frames")
    out["digest"] = out["e_console_frame_12_rooms_unchanged"]["this"]["digest"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
