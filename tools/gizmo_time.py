"""Times b32_draw_gizmos in an editor-like overlay, and shows that the console frame it does not touch is unchanged.  Every configuration is
checked against tests/test_gizmos.py's ref_gizmos before it is timed.

  1. Editor-like overlay: 2 000 draw_3d_line items, 36 thick lines (thickness 3) and 4 filled octahedra at 640x480 over the golden room
     drawn in z-buffer mode.  (a) one b32_draw_gizmos call; (b) the helpers restated on the host, vectorised in numpy (np_gizmos below),
     followed by b32_draw_prims of the line records and, for every run of triangles, a host round trip of the frame (download, fill,
     upload).  Wall time per overlay, host time included on both sides, a synchronisation per overlay.
  2. The delivered console frame with the player's cylinder (tools/lines_time.py's console case, profiles/lines_time.json), which runs
     none of the new kernels: the parent commit's library (--parent-lib) and this one alternately, a fresh process per window, three
     windows each.  Accepted when this build's median lies within the parent's own window-to-window range.

Usage: python tools/gizmo_time.py [out.json] [--parent-lib libb32raster_parent.so]"""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import numpy as np

NEW_SYMBOLS = ("b32_draw_gizmos", "b32_gizmo_project_batch", "b32_gizmo_counts", "b32_octahedron_items")
f32 = np.float32


def _vdot(r, b):
    return (r[:, 0] * b[0] + r[:, 1] * b[1]) + r[:, 2] * b[2]


def _i32(v):
    x = np.asarray(v, f32).astype(np.float64)
    return np.trunc(np.clip(np.where(np.isnan(x), 0.0, x), -2147483648.0, 2147483647.0)).astype(np.int64)


def np_gizmos(items, camera, w, h):
    """ref_gizmos vectorised over the batch for the kinds of the overlay (LINE, THICK_LINE_DEPTH, TRIANGLE): the records, in order."""
    from bonnie32_amd import abi
    from tests.test_world import _cam_f32, noop_records, QNAN
    I = np.ascontiguousarray(items, abi.GIZMO_ITEM_DTYPE).reshape(-1)
    n = len(I)
    kind, size = I["kind"].astype(np.int64), I["size"].astype(np.int64)
    assert np.isin(kind, (abi.GIZMO_LINE, abi.GIZMO_THICK_LINE_DEPTH, abi.GIZMO_TRIANGLE)).all()
    pos, bx, by, bz = (np.array(v, f32) for v in _cam_f32(camera))
    NEAR = f32(0.1)
    vs = (f32(min(w, h)) / f32(2.0)) * f32(0.75)
    hw, hh = f32(w) / f32(2.0), f32(h) / f32(2.0)
    with np.errstate(all="ignore"):
        def project(P):
            rel = P - pos
            cx, cy, cz = _vdot(rel, bx), _vdot(rel, by), _vdot(rel, bz)
            denom = cz + f32(5.0)
            return (cx * f32(4.0) / denom) * vs + hw, (cy * f32(4.0) / denom) * vs + hh, cz

        P0, P1 = I["p0"].astype(f32), I["p1"].astype(f32)
        z0, z1 = _vdot(P0 - pos, bz), _vdot(P1 - pos, bz)
        b0, b1 = z0 <= NEAR, z1 <= NEAR
        t = (NEAR - z0) / (z1 - z0)
        Q = P0 + (P1 - P0) * t[:, None]
        C0 = np.where((b0 & ~b1)[:, None], Q, P0); C1 = np.where((~b0 & b1)[:, None], Q, P1)
        x0, y0, d0 = project(C0); x1, y1, d1 = project(C1)
        line_ok = ~(b0 & b1) & ~(d0 <= NEAR) & ~(d1 <= NEAR)
        # clip_line_to_rect on every segment at once: 16 rounds, lanes that have returned keep their state
        cx0, cy0, cx1, cy1 = x0.copy(), y0.copy(), x1.copy(), y1.copy()
        xmax, ymax, one, zero = f32(w), f32(h), f32(1.0), f32(0.0)

        def outcode(x, y):
            return np.where(x < zero, 1, np.where(x >= xmax, 2, 0)) | np.where(y < zero, 8, np.where(y >= ymax, 4, 0))

        c0, c1 = outcode(cx0, cy0), outcode(cx1, cy1)
        live = np.ones(n, bool); accept = np.zeros(n, bool)
        for _ in range(16):
            acc = live & ((c0 | c1) == 0); rej = live & ((c0 & c1) != 0)
            accept |= acc; live &= ~(acc | rej)
            if not live.any():
                break
            co = np.where(c0 != 0, c0, c1)
            bot, top, right = (co & 4) != 0, (co & 8) != 0, (co & 2) != 0
            dx, dy = cx1 - cx0, cy1 - cy0
            xh = np.where(bot, cx0 + dx * (ymax - one - cy0) / dy, cx0 + dx * (zero - cy0) / dy)
            yv = np.where(right, cy0 + dy * (xmax - one - cx0) / dx, cy0 + dy * (zero - cx0) / dx)
            horiz = bot | top
            nx = np.where(horiz, xh, np.where(right, xmax - one, zero)).astype(f32)
            ny = np.where(horiz, np.where(bot, ymax - one, zero), yv).astype(f32)
            first = live & (co == c0); second = live & ~(co == c0)
            cx0 = np.where(first, nx, cx0); cy0 = np.where(first, ny, cy0); cx1 = np.where(second, nx, cx1); cy1 = np.where(second, ny, cy1)
            c0 = np.where(first, outcode(cx0, cy0), c0); c1 = np.where(second, outcode(cx1, cy1), c1)
        accept |= live & ((c0 | c1) == 0) & False                    # (after 16 rounds: None)
        # the editor's project_vertex for the triangles
        tri = []
        tri_ok = np.ones(n, bool)
        for f in ("p0", "p1", "p2"):
            rel = I[f].astype(f32) - pos
            cx, cy, cz = _vdot(rel, bx), _vdot(rel, by), _vdot(rel, bz)
            denom = cz + f32(5.0)
            flat = np.abs(denom) < f32(0.001)
            sx = np.where(flat, hw, (cx * f32(4.0)) / denom * vs + hw); sy = np.where(flat, hh, (cy * f32(4.0)) / denom * vs + hh)
            tri_ok &= ~(cz < NEAR)
            tri.append((_i32(sx), _i32(sy)))
        # the thick lines' offsets
        ix0, iy0, ix1, iy1 = _i32(x0), _i32(y0), _i32(x1), _i32(y1)
        ddx, ddy = (ix1 - ix0).astype(f32), (iy1 - iy0).astype(f32)
        length = np.sqrt(ddx * ddx + ddy * ddy)
        half = size.astype(f32) * f32(0.5)
        px, py = -ddy / length * half, ddx / length * half
    LIM = 1 << 30
    thick = (kind == abi.GIZMO_THICK_LINE_DEPTH) & (size > 1)
    count = np.where(thick, size, 1)
    first_rec = np.concatenate([[0], np.cumsum(count)])
    out = noop_records(int(first_rec[-1]))
    zi = {f: out[f].view(np.int32) for f in ("z0", "z1")}

    def put(sel, at, fields):
        for f, v in fields.items():
            out[f][at] = v[sel] if isinstance(v, np.ndarray) else v
        for f in ("r", "g", "b", "blend"):
            out[f][at] = I[f][sel]
        out["size"][at] = 0

    k0 = (kind == abi.GIZMO_LINE) & line_ok & accept
    a = {"x0": _i32(cx0), "y0": _i32(cy0), "x1": _i32(cx1), "y1": _i32(cy1)}
    k0 &= (np.abs(a["x1"] - a["x0"]) < LIM) & (np.abs(a["y1"] - a["y0"]) < LIM)
    put(k0, first_rec[:-1][k0], dict(a, kind=abi.LINE_2D))
    ext_ok = (np.abs(ix1 - ix0) < LIM) & (np.abs(iy1 - iy0) < LIM)
    dz0, dz1 = np.where(np.isnan(d0), QNAN, d0), np.where(np.isnan(d1), QNAN, d1)
    k1 = (kind == abi.GIZMO_THICK_LINE_DEPTH) & ~thick & line_ok & ext_ok
    put(k1, first_rec[:-1][k1], {"x0": ix0, "y0": iy0, "x1": ix1, "y1": iy1, "z0": dz0, "z1": dz1, "kind": abi.LINE_3D_OVERLAY})
    small = (np.abs(ix0) < LIM) & (np.abs(iy0) < LIM) & (np.abs(ix1) < LIM) & (np.abs(iy1) < LIM)
    k2 = thick & line_ok & ext_ok & small & ~(length < f32(0.001))
    with np.errstate(all="ignore"):
        for i in range(int(size[k2].max()) if k2.any() else 0):
            sel = k2 & (size > i)
            offset = f32(i) - half + f32(0.5)
            ox, oy = _i32(px * offset / half), _i32(py * offset / half)
            put(sel, first_rec[:-1][sel] + i, {"x0": ix0 + ox, "y0": iy0 + oy, "x1": ix1 + ox, "y1": iy1 + oy, "z0": dz0, "z1": dz1, "kind": abi.LINE_3D_OVERLAY})
    k4 = (kind == abi.GIZMO_TRIANGLE) & tri_ok
    for x, y in tri:
        k4 &= (np.abs(x) < LIM) & (np.abs(y) < LIM)
    k4 &= ~((tri[0][1] == tri[1][1]) & (tri[1][1] == tri[2][1]))
    at = first_rec[:-1][k4]
    put(k4, at, {"x0": tri[0][0], "y0": tri[0][1], "x1": tri[1][0], "y1": tri[1][1], "kind": abi.PRIM_TRIANGLE_INTERNAL})
    zi["z0"][at] = tri[2][0][k4]; zi["z1"][at] = tri[2][1][k4]
    return out


def overlay_items(camera, zmax):
    from bonnie32_amd import abi, rasterizer as R
    import bonnie32_amd as b32
    from tests.test_gizmos import cam_point, random_gizmos
    rng = np.random.default_rng(9100)
    kw = dict(spread=(zmax * 0.6, zmax * 0.45), depth=(-0.1 * zmax, 1.2 * zmax), seg=zmax * 0.05, hostile=False)
    lines = random_gizmos(rng, 2000, camera, kinds=(abi.GIZMO_LINE,), **kw)
    thick = random_gizmos(rng, 36, camera, kinds=(abi.GIZMO_THICK_LINE_DEPTH,), **kw)
    thick["size"] = 3
    octa = [R.octahedron_items(cam_point(camera, x * zmax, y * zmax, 0.25 * zmax), 0.04 * zmax, b32.Color(255, 200, 50)) for x, y in ((-0.12, -0.05), (0.1, 0.04), (0.0, -0.08), (0.05, 0.09))]
    return np.concatenate([lines, thick] + octa)


def editor_case(reps=20):
    import bonnie32_amd as b32
    from bonnie32_amd import abi, rasterizer as R
    from tests.test_gizmos import TRI, cpu_records, np_tri, ref_gizmos, tri_points
    from tests.test_world import _game_scene
    W, H = 640, 480
    sc = _game_scene()
    sc.settings.use_zbuffer = True
    ctx = R.Context(0)
    fb = R.Framebuffer(W, H, ctx)
    fb.clear(sc.clear_color)
    R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    px0, z0 = fb.pixels, fb.zbuffer
    zmax = float(z0[z0 < 1e30].max())
    items = overlay_items(sc.camera, zmax)
    want_recs, counts = ref_gizmos(items, sc.camera, None, W, H)
    host_recs = np_gizmos(items, sc.camera, W, H)
    assert host_recs.tobytes() == want_recs.tobytes(), "the vectorised restatement differs from ref_gizmos"
    want = px0.copy(); cpu_records(want, z0, W, H, want_recs)

    def device():
        fb.draw_gizmos(items, sc.camera)
        ctx.synchronize()

    def host():
        recs = np_gizmos(items, sc.camera, W, H)
        tri = recs["kind"] == TRI
        i = 0
        while i < len(recs):
            j = i
            while j < len(recs) and tri[j] == tri[i]:
                j += 1
            if tri[i]:                                                     # a host round trip of the frame for a run of triangles
                px = fb.pixels
                for r in recs[i:j]:
                    np_tri(px.reshape(-1, 4), W, H, *tri_points(r), (int(r["r"]), int(r["g"]), int(r["b"])))
                fb.upload(px)
            else:
                fb.draw_prims(recs[i:j])
            i = j
        ctx.synchronize()

    out = {"items": int(len(items)), "records": int(len(want_recs)), "counts": list(counts)}
    for name, fn in (("draw_gizmos", device), ("host_restatement", host)):
        fb.upload(px0)
        fn()
        out[name + "_exact"] = bool(np.array_equal(fb.pixels, want))
        ts = []
        for _ in range(reps):
            fb.upload(px0)
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name + "_ms_median"] = round(statistics.median(ts), 4); out[name + "_ms_min"] = round(min(ts), 4)
    out["speedup"] = round(out["host_restatement_ms_median"] / out["draw_gizmos_ms_median"], 2)
    ctx.close()
    return out


def console_window():
    """One window of the console frame with the cylinder (a fresh process; --lib PATH: that library, without the new symbols)."""
    from bonnie32_amd import abi
    if "--lib" in sys.argv:
        abi.SYMBOLS = [s for s in abi.SYMBOLS if s[0] not in NEW_SYMBOLS]
        os.environ["B32_LIB"] = sys.argv[sys.argv.index("--lib") + 1]
    sys.path.insert(0, HERE)
    import lines_time
    r = lines_time.console_case(reps=3, frames=400)
    print(json.dumps({"frame_ms_with_cylinder": r["frame_ms_with_cylinder"], "frame_ms_without": r["frame_ms_without"], "exact": r["delivered_frame_exact"]}))


def console_case(parent_lib):
    rows = {"parent": [], "this": []}
    for _ in range(3):
        for name in ("parent", "this"):
            cmd = [sys.executable, os.path.abspath(__file__), "--console-window"] + (["--lib", parent_lib] if name == "parent" else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"{name} window failed: {r.stderr[-2000:]}")
            rows[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {}
    for name, ws in rows.items():
        v = [w["frame_ms_with_cylinder"] for w in ws]
        out[name] = {"windows_ms": v, "median_ms": round(statistics.median(v), 4), "exact": all(w["exact"] for w in ws)}
    lo, hi = min(out["parent"]["windows_ms"]), max(out["parent"]["windows_ms"])
    m = out["this"]["median_ms"]
    out["within_parent_range"] = bool(lo <= m <= hi) or bool(m < lo)
    out["above_parent_max_us"] = round(max(0.0, m - hi) * 1e3, 2)
    return out


def main():
    if "--console-window" in sys.argv:
        return console_window()
    from bonnie32_amd import build as B
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    if parent in args:
        args.remove(parent)
    res = {"tool": "gizmo_time", "digest": B.csrc_digest(), "editor_overlay_640x480": editor_case()}
    if parent:
        res["console_frame_with_cylinder"] = console_case(os.path.abspath(parent))
    s = json.dumps(res, indent=1)
    print(s)
    if args:
        open(args[0], "w").write(s + "\n")


if __name__ == "__main__":
    main()
