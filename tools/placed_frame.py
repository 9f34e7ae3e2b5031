"""A console frame with placed objects (render_scene, scene.rs:180-261): 12 resident rooms plus 24 placed instances of 3 resident asset parts
(8 objects x 3 parts, one placement per object), 320x240, game() + lights + fog, EVERY instance moving EVERY frame, every frame delivered to
page-locked host memory (b32_fb_download_async + tickets, the presenter one frame behind).  Three forms, each checked against the CPU oracle on
host-placed vertices before it is timed, host time included on every side:
  (a) b32_frame_submit_placed: the parts uploaded once, the placements rewritten in the frame table every frame;
  (b) what the library could do before placements existed: place_vertices on the host and a b32_scene_upload into one slot per instance per
      frame, then b32_frame_submit -- on this same build;
  (c) the 12 rooms alone, no placement anywhere: this build and (--parent-lib PATH) the parent commit's library, alternately, each repetition a
      process of its own.  The placement is compiled out of the kernels this frame uses, so the two must lie within each other's spread.
usage: python tools/placed_frame.py [--parent-lib PATH] [--out profiles/placed_frame.json] [--reps 3] [--alternations 3]
Writes the JSON with the build digest; prints a one-line summary.
--host-ab (with --parent-lib): only the host-bound comparison of two builds -- (c), and (d) the same 12 rooms drawn through their scene slots,
one b32_scene_swap pair and one b32_render_scene_15_async per room -- for a change that touches host code alone."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def load(lib_path):
    """The package over the given library (None: the tree's own, digest checked).  A parent library lacks the placed entries: only the symbols
    it exports are bound."""
    from bonnie32_amd import abi
    if lib_path:
        probe = C.CDLL(lib_path)
        abi.SYMBOLS = [s for s in abi.SYMBOLS if hasattr(probe, s[0])]
        os.environ["B32_LIB"] = lib_path
        lib = abi.load_library()
        return (lib.b32_build_digest() or b"").decode()
    import __graft_entry__ as g
    g.build()
    return abi.check_build_digest()


def scene():
    import bonnie32_amd as b32
    from bonnie32_amd import scenegen
    rng = np.random.default_rng(2024)
    rooms = [scenegen.make_scene("C1", n_tris=int(rng.integers(300, 3000)), seed=1000 + i, variant=("blend" if i % 4 == 3 else "gouraud"),
                                 bbox_px=float(rng.choice([150.0, 400.0, 900.0]))) for i in range(12)]
    parts = [scenegen.make_scene("C1", n_tris=n, seed=1100 + i, variant="gouraud", bbox_px=120.0) for i, n in enumerate((400, 150, 60))]
    for p in parts:                       # an asset's local space: around the origin, a few dozen units across (placed in front of the rooms)
        p.vertices["pos"] -= p.vertices["pos"].mean(axis=0, dtype=np.float64).astype(np.float32)
        p.vertices["pos"] *= np.float32(0.012)
    st = b32.RasterSettings.game()
    st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.point((0.0, -100.0, 1500.0), 3000.0, 1.2)]
    fog = (1500.0, 3000.0, 5800.0, b32.Color(40, 50, 70))
    return rooms, parts, st, fog, b32.Color(10, 10, 30)


def placements(t, n_objects=8):
    import bonnie32_amd as b32
    return [b32.Placement(facing=0.4 * k + 0.05 * t, world_pos=(-105.0 + 30.0 * k + 6.0 * np.sin(0.1 * t + k), -40.0 + 30.0 * (k % 3) + 5.0 * np.cos(0.07 * t),
                                                                 220.0 + 25.0 * (k % 4) + 6.0 * np.sin(0.05 * t + 2 * k))) for k in range(n_objects)]


def windows(frame, n_frames, reps, drain):
    """ms per frame of `reps` windows of n_frames each (host clock around work that ends in a wait for the last frame's pixels)."""
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for i in range(n_frames):
            frame(i)
        drain(n_frames - 1)
        out.append((time.perf_counter() - t0) / n_frames * 1e3)
    return out


def spread(v):
    v = sorted(v)
    return {"min_ms": round(v[0], 4), "median_ms": round(v[len(v) // 2], 4), "max_ms": round(v[-1], 4), "windows": [round(x, 4) for x in v]}


def child(mode, lib_path, reps):
    digest = load(lib_path)
    import bonnie32_amd as b32
    from bonnie32_amd import rasterizer as R
    from oracle import oracle as O
    rooms, parts, st, fog, clear = scene()
    W, H = rooms[0].width, rooms[0].height
    cam = rooms[0].camera
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    room_slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in rooms]
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    tickets = [0, 0]

    def oracle_frame(t, with_objects):
        ofb = O.Framebuffer(W, H); ofb.clear(clear)
        for sc in rooms:
            assert O.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, st, fog)[0] == 0
        if with_objects:
            for pl in placements(t):
                for p in parts:
                    assert O.render_mesh_15(ofb, pl.apply(p.vertices), p.faces, p.textures, cam, st, fog)[0] == 0
        return ofb.pixels

    def deliver(i):
        tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
        if i > 0:
            ctx.ticket_wait(tickets[(i - 1) & 1])

    def drain(i):
        ctx.ticket_wait(tickets[i & 1]); ctx.finish()

    res = {"mode": mode, "digest": digest}
    if mode == "rooms":                                   # (c)
        table = ctx.make_frame_table(cam, st, room_slots, fogs=[fog] * 12)

        def frame(i):
            fb.clear(clear); ctx.frame_submit(table); deliver(i)
        for i in range(50): frame(i)
        drain(49)
        res["exact"] = bool(np.array_equal(bufs[49 & 1][0], oracle_frame(0, False)))
        res["ms"] = windows(frame, 2000, reps, drain)
    elif mode == "slots":                                 # (d)
        def frame(i):
            fb.clear(clear)
            for rs in room_slots:
                rs.render_async(cam, st, fog) if i == 0 else rs.render_async()
            deliver(i)
        for i in range(50): frame(i)
        drain(49)
        res["exact"] = bool(np.array_equal(bufs[49 & 1][0], oracle_frame(0, False)))
        res["ms"] = windows(lambda i: frame(i + 1), 2000, reps, drain)
    elif mode == "placed":                                # (a)
        part_slots = [R.ResidentScene(fb, p.vertices, p.faces, p.textures).detach() for p in parts]
        table = ctx.make_frame_table(cam, st, room_slots + part_slots * 8, fogs=[fog] * 36, placements=[None] * 36)

        def frame(i):
            pls = placements(i)
            ctx.set_table_placements(table, [None] * 12 + [pls[k] for k in range(8) for _ in range(3)])
            fb.clear(clear); ctx.frame_submit(table); deliver(i)
        ok = True
        for i in range(40):
            frame(i)
            if i in (1, 17, 39):
                ctx.ticket_wait(tickets[(i - 1) & 1]); ok &= bool(np.array_equal(bufs[(i - 1) & 1][0], oracle_frame(i - 1, True)))
        drain(39)
        built = ctx.batch_counts()["merged_built"]
        res["exact"] = ok
        res["ms"] = windows(frame, 1000, reps, drain)
        res["merged_built_constant"] = ctx.batch_counts()["merged_built"] == built
        res["merged_draws_per_frame"] = ctx.batch_counts()["merged_draws"] / ctx.batch_counts()["frames"]
    else:                                                 # (b) "uploaded"
        inst = [R.ResidentScene(fb, p.vertices, p.faces, p.textures).detach() for _ in range(8) for p in parts]
        table = ctx.make_frame_table(cam, st, room_slots + inst, fogs=[fog] * 36)
        packed = [(np.ascontiguousarray(p.faces, b32.abi.FACE_DTYPE), b32.rtypes.pack_textures(p.textures)) for p in parts]

        def frame(i):
            pls = placements(i)
            for k in range(8):
                for j, p in enumerate(parts):
                    v = pls[k].apply(p.vertices)
                    rs = inst[3 * k + j]; f, (tex, _keep) = packed[j]
                    rs._swap()
                    rc = ctx.lib.b32_scene_upload(ctx.h, v.ctypes.data, len(v), f.ctypes.data, len(f), C.cast(tex, C.c_void_p), len(p.textures))
                    rs._swap()
                    assert rc == 0
            fb.clear(clear); ctx.frame_submit(table); deliver(i)
        ok = True
        for i in range(12):
            frame(i)
            if i in (1, 11):
                ctx.ticket_wait(tickets[(i - 1) & 1]); ok &= bool(np.array_equal(bufs[(i - 1) & 1][0], oracle_frame(i - 1, True)))
        drain(11)
        res["exact"] = ok
        res["ms"] = windows(frame, 150, reps, drain)
    for _, p in bufs:
        ctx.host_free(p)
    ctx.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child"); ap.add_argument("--lib"); ap.add_argument("--parent-lib"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--host-ab", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "placed_frame.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.lib, a.reps)

    def run(mode, lib=None):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(a.reps)] + (["--lib", lib] if lib else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode:
            raise RuntimeError(f"{mode}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    out = {"tool": "tools/placed_frame.py", "frame": "320x240, 12 resident rooms + 24 placed instances of 3 resident parts, every instance moving every frame, "
           "every frame delivered to page-locked host memory; ms per frame, host time included; windows of 2000 / 1000 / 150 frames"}
    if a.host_ab:
        return host_ab(a, run, out)
    placed, uploaded = run("placed"), run("uploaded")
    out["digest"] = placed["digest"]
    out["a_frame_submit_placed"] = dict(spread(placed["ms"]), exact=placed["exact"], merged_built_constant=placed["merged_built_constant"],
                                        merged_draws_per_frame=placed["merged_draws_per_frame"])
    out["b_host_place_and_upload_per_instance"] = dict(spread(uploaded["ms"]), exact=uploaded["exact"])
    out["b_over_a"] = round(out["b_host_place_and_upload_per_instance"]["median_ms"] / out["a_frame_submit_placed"]["median_ms"], 2)
    out["c_rooms_only_no_placement"] = alternate(a, run, "rooms")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


def alternate(a, run, mode):
    runs = {"this": [], "parent": []}
    for _ in range(a.alternations):                       # alternately: parent, this, parent, this, ...
        if a.parent_lib:
            runs["parent"].append(run(mode, os.path.abspath(a.parent_lib)))
        runs["this"].append(run(mode))
    c = {}
    for who, rs in runs.items():
        if rs:
            per_run = [sorted(r["ms"])[len(r["ms"]) // 2] for r in rs]
            c[who] = {"digest": rs[0]["digest"], "exact": all(r["exact"] for r in rs), "run_medians_ms": [round(x, 4) for x in per_run],
                      "all_windows": spread([x for r in rs for x in r["ms"]])}
    if "parent" in c:
        lo, hi = min(c["parent"]["run_medians_ms"]), max(c["parent"]["run_medians_ms"])
        c["parent_spread_ms"] = [lo, hi]
        c["this_within_parent_spread"] = all(lo <= x <= hi for x in c["this"]["run_medians_ms"])
        mid = sorted(c["this"]["all_windows"]["windows"])[len(c["this"]["all_windows"]["windows"]) // 2]
        c["this_median_of_windows_ms"] = mid
        c["this_median_at_most_parent_spread_above_parent_range"] = bool(mid <= hi + (hi - lo))
    return c


def host_ab(a, run, out):
    out["frame"] = "320x240, 12 resident rooms, every frame delivered to page-locked host memory; ms per frame, host time included; windows of 2000 frames"
    out["command"] = "python tools/placed_frame.py --host-ab --parent-lib <the parent commit's libb32raster.so> --out " + a.out
    out["c_frame_submit"] = alternate(a, run, "rooms")
    out["d_scene_slots_one_swap_pair_per_room"] = alternate(a, run, "slots")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
