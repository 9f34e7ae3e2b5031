"""What the sky costs in front of the delivered console frame, and that the frame without a sky costs what it did.
  (a) tools/placed_frame.py's 12 rooms (320x240, game() + lights + fog, every frame delivered to page-locked host memory by ticket, the
      presenter one frame behind) with a sky in front: the reference-sized sphere (49 x 33 vertices plus 3 x 20 mountain peaks of 4
      vertices) and 80 / 2000 stars of size 3.  Three forms, alternating windows in ONE process, host time included on every side, each
      checked against the CPU oracle before it is timed:
        per_call   b32_render_skybox_mesh (the placed vertices uploaded every frame) + b32_draw_star_diamonds
        resident   b32_render_sky (from the camera alone) + b32_draw_stars
        resident_update   the same with a b32_sky_update of every vertex every frame (a cloud layer that covers the whole sky)
  (b) the unchanged delivered console frame (placed_frame.py's "rooms": no sky, none of the new code): this build and (--parent-lib PATH)
      the parent commit's library, alternately, each repetition a process of its own.
Acceptance of (b): this build's run medians lie inside the parent's own run-to-run range; one outside is reported with its distance.
usage: python tools/sky_time.py [--parent-lib PATH] [--out profiles/sky_time.json] [--reps 5] [--alternations 3] [--frames 400]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np

import placed_frame as PF


def sky_mesh(h_segments=48, v_segments=32, radius=10000.0, ranges=3, peaks=20, seed=5):
    """A sky of the reference's size around the origin (its positions are the offsets): sphere rows of h_segments + 1 vertices with the faces
    [i0, i2, i1], [i1, i2, i3], then per mountain peak four vertices (peak, left base, right base, centre base) and two faces.  The colours
    are test data: the reference samples its gradients there with libm."""
    from bonnie32_amd import abi
    rng = np.random.default_rng(seed)
    pos, faces = [], []
    for v in range(v_segments + 1):
        phi = np.pi * v / v_segments
        for h in range(h_segments + 1):
            th = 2 * np.pi * h / h_segments
            pos.append((np.sin(phi) * np.cos(th) * radius, np.cos(phi) * radius, np.sin(phi) * np.sin(th) * radius))
    rw = h_segments + 1
    for v in range(v_segments):
        for h in range(h_segments):
            i0, i1, i2, i3 = v * rw + h, v * rw + h + 1, (v + 1) * rw + h, (v + 1) * rw + h + 1
            faces += [[i0, i2, i1], [i1, i2, i3]]
    for r in range(ranges):
        mr = radius * (0.99 - 0.01 * r)
        base_phi = np.pi / 2
        for p in range(peaks):
            th = 2 * np.pi * (p + 0.3 * r) / peaks
            half = np.pi / peaks * 1.3
            peak_phi = base_phi - (0.05 + 0.1 * rng.random())
            k = len(pos)
            for ph, t in ((peak_phi, th), (base_phi, th - half), (base_phi, th + half), (base_phi, th)):
                pos.append((np.sin(ph) * np.cos(t) * mr, np.cos(ph) * mr, np.sin(ph) * np.sin(t) * mr))
            faces += [[k, k + 3, k + 1], [k, k + 2, k + 3]]
    verts = np.zeros(len(pos), abi.SKY_VERTEX_DTYPE)
    verts["pos"] = np.array(pos, np.float32)
    col = rng.integers(0, 256, (len(verts), 3), dtype=np.uint8)
    verts["r"], verts["g"], verts["b"] = col[:, 0], col[:, 1], col[:, 2]
    return verts, np.array(faces, np.uint32)


def child(lib_path, reps, n_frames):
    digest = PF.load(lib_path)
    from bonnie32_amd import rasterizer as R, sky
    from bonnie32_amd.records import pack_stars
    from oracle import oracle as O
    rooms, _parts, st, fog, clear = PF.scene()
    W, H = rooms[0].width, rooms[0].height
    cam = rooms[0].camera
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in rooms]
    table = ctx.make_frame_table(cam, st, slots, fogs=[fog] * len(slots))
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    tickets = [0, 0]
    offsets, faces = sky_mesh()
    placed = sky.sky_place(offsets, cam.position)
    other = offsets.copy()
    other["r"], other["g"], other["b"] = offsets["g"], offsets["b"], offsets["r"]
    resident = sky.ResidentSky(ctx, offsets, faces)
    rng = np.random.default_rng(31)
    res = {"digest": digest, "sky_vertices": len(offsets), "sky_faces": len(faces), "frames_per_window": n_frames, "stars": {}}

    def deliver(i):
        tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
        if i > 0:
            ctx.ticket_wait(tickets[(i - 1) & 1])

    def drain(i):
        ctx.ticket_wait(tickets[i & 1]); ctx.finish()

    for n_stars in (80, 2000):
        cx, cy, rgb = rng.integers(-3, W + 3, n_stars).astype(np.int32), rng.integers(-3, H + 3, n_stars).astype(np.int32), rng.integers(0, 256, (n_stars, 3)).astype(np.uint8)
        stars = pack_stars(cx, cy, rgb)

        def oracle_frame(verts):
            o = O.Framebuffer(W, H); o.clear(clear)
            assert o.render_skybox_mesh(sky.sky_place(verts, cam.position), faces, cam) == 0
            o.draw_star_diamonds(cx, cy, rgb, 3.0)
            for sc in rooms:
                assert O.render_mesh_15(o, sc.vertices, sc.faces, sc.textures, cam, st, fog)[0] == 0
            return o.pixels

        def per_call(i):
            fb.clear(clear); fb.render_skybox_mesh(placed, faces, cam); fb.draw_star_diamonds(cx, cy, rgb, 3.0)
            ctx.frame_submit(table); deliver(i)

        def res_frame(i):
            fb.clear(clear); resident.render(fb, cam); sky.draw_stars(fb, stars, 3.0)
            ctx.frame_submit(table); deliver(i)

        def res_update(i):
            fb.clear(clear); resident.update(0, other if i & 1 else offsets); resident.render(fb, cam); sky.draw_stars(fb, stars, 3.0)
            ctx.frame_submit(table); deliver(i)

        forms = {"per_call": per_call, "resident": res_frame, "resident_update": res_update}
        want = {0: oracle_frame(offsets), 1: oracle_frame(other)}
        exact = {}
        for name, frame in forms.items():
            resident.update(0, offsets)
            for i in range(20): frame(i)
            drain(19)
            exact[name] = bool(np.array_equal(bufs[19 & 1][0], want[1 if name == "resident_update" else 0]))
        ms = {name: [] for name in forms}
        for _ in range(reps):                               # alternating windows
            for name, frame in forms.items():
                t0 = time.perf_counter()
                for i in range(n_frames): frame(i)
                drain(n_frames - 1)
                ms[name].append((time.perf_counter() - t0) / n_frames * 1e3)
        resident.update(0, offsets)
        res["stars"][str(n_stars)] = {"exact": exact, "ms": ms}
    ctx.synchronize()
    resident.destroy()
    for _, p in bufs:
        ctx.host_free(p)
    ctx.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true"); ap.add_argument("--lib"); ap.add_argument("--parent-lib"); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--alternations", type=int, default=3); ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--out", default=os.path.join("profiles", "sky_time.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.lib, a.reps, a.frames)

    def run(cmd):
        r = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=900)
        if r.returncode:
            raise RuntimeError(f"{cmd}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    out = {"tool": "tools/sky_time.py", "command": "python tools/sky_time.py --parent-lib <the parent commit's libb32raster.so>",
           "frame": "320x240, 12 resident rooms delivered to page-locked host memory by ticket; ms per frame, host time included"}
    s = run([os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--frames", str(a.frames)])
    out["digest"] = s["digest"]
    sky_out = {"sky_vertices": s["sky_vertices"], "sky_faces": s["sky_faces"], "frames_per_window": s["frames_per_window"], "windows": "alternating, one process"}
    for n_stars, r in s["stars"].items():
        forms = {name: dict(PF.spread(v), exact=r["exact"][name]) for name, v in r["ms"].items()}
        forms["per_call_over_resident"] = round(forms["per_call"]["median_ms"] / forms["resident"]["median_ms"], 3)
        forms["per_call_over_resident_update"] = round(forms["per_call"]["median_ms"] / forms["resident_update"]["median_ms"], 3)
        forms["resident_is_faster"] = bool(forms["resident"]["median_ms"] < forms["per_call"]["median_ms"])
        sky_out[f"{n_stars}_stars"] = forms
    out["a_console_frame_with_a_sky"] = sky_out
    pf = os.path.join(HERE, "placed_frame.py")
    runs = {"this": [], "parent": []}
    for _ in range(a.alternations):                         # alternately: parent, this, parent, this, ...
        if a.parent_lib:
            runs["parent"].append(run([pf, "--child", "rooms", "--reps", "3", "--lib", os.path.abspath(a.parent_lib)]))
        runs["this"].append(run([pf, "--child", "rooms", "--reps", "3"]))
    c = {"frame": "placed_frame.py's rooms: no sky, none of the new code; windows of 2000 frames, every run a process of its own"}
    for who, rs in runs.items():
        if rs:
            c[who] = {"digest": rs[0]["digest"], "exact": all(r["exact"] for r in rs),
                      "run_medians_ms": [round(sorted(r["ms"])[len(r["ms"]) // 2], 5) for r in rs], "all_windows": PF.spread([x for r in rs for x in r["ms"]])}
    if "parent" in c:
        lo, hi = min(c["parent"]["run_medians_ms"]), max(c["parent"]["run_medians_ms"])
        c["parent_range_ms"] = [lo, hi]
        c["this_within_parent_range"] = all(lo <= x <= hi for x in c["this"]["run_medians_ms"])
        c["this_outside_parent_range_by_us"] = [round((x - hi if x > hi else x - lo) * 1e3, 2) for x in c["this"]["run_medians_ms"] if not lo <= x <= hi]
        c["this_median_minus_parent_median_us"] = round((sorted(c["this"]["run_medians_ms"])[len(runs["this"]) // 2] - sorted(c["parent"]["run_medians_ms"])[len(runs["parent"]) // 2]) * 1e3, 2)
        c["parent_own_spread_us"] = round((hi - lo) * 1e3, 2)
    out["b_unchanged_console_frame"] = c
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
