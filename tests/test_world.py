"""World-space overlay items through b32_draw_world / b32_draw_floor_grid (rasterizer/draw.rs:12-135, math.rs:503-652).

The oracle has no entry for these functions, so the expectation is built here:
  `ref_world`  a literal scalar restatement of draw_3d_line_clipped and the four world_to_screen functions, every operand an np.float32,
               returning the abi.PRIM_DTYPE records the reference's fb.draw_* calls would be made with (a record that draws nothing --
               a circle of radius -1 -- where the reference makes no call) and the counts (drawn, dropped, rejected);
  `np_world`   the same vectorised over the batch, pinned to ref_world on CPU.
ref_world itself is pinned by hand-computed cases and, for the near-plane clip (whose outcome hangs on the last bit of
p0 + (p1 - p0) * t), by the same expressions evaluated in exact rational arithmetic with an explicit round-to-nearest-even.
Every GPU frame is compared byte for byte with a frame composed on the CPU in the same order: the oracle renders the meshes,
tests.test_prims.np_prims draws np_world's records wherever the GPU side calls a world entry."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi
from tests.test_lines import ROOT, _upload_zbuffer
from tests.test_prims import _as_i32, np_prims

f32 = np.float32
NEAR = f32(0.1)                                                # NEAR_PLANE, math.rs:155
LINE_KINDS = (0, 1, 2, 3, 4, abi.PRIM_LINE_BLENDED, abi.PRIM_THICK_LINE)
DEPTH_KINDS = (abi.LINE_3D, abi.LINE_3D_OVERLAY, abi.LINE_3D_ALPHA)
CIRCLE_KINDS = (abi.PRIM_CIRCLE, abi.PRIM_CIRCLE_ALPHA)
LIM = 1 << 30
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]   # a NaN depth is stored as this one: NaN payloads are specified neither by Rust nor by
                                                               # IEEE 754 (x86 and the GPU make different ones), and every NaN fails every depth test alike
SIZES = ((320, 240), (2560, 1920))
ORTHO = (0.05, 120.0, -40.0)                                   # OrthoProjection { zoom, center_x, center_y }


# ---------------------------------------------------------------- cameras
def look_at(position, target):
    """The issue's camera: in float64 basis_z = the normalised direction, basis_x = normalize(cross((0, 1, 0), basis_z)),
    basis_y = -cross(basis_z, basis_x); all four vectors cast to f32."""
    p = np.asarray(position, np.float64); t = np.asarray(target, np.float64)
    bz = (t - p) / np.linalg.norm(t - p)
    bx = np.cross((0.0, 1.0, 0.0), bz); bx /= np.linalg.norm(bx)
    by = -np.cross(bz, bx)
    return b32.Camera(*(tuple(float(x) for x in v.astype(f32)) for v in (p, bx, by, bz)))


CENSUS_CAM = look_at((300, 1500, -700), (0, 0, 2000))
GRID_CAMS = (CENSUS_CAM, look_at((37.5, 40, 12.25), (5000, 0, 3000)), look_at((100, 600, 100), (400, 0, 300)))
IDENTITY_CAM = b32.Camera()


def _cam_f32(cam):
    return tuple(tuple(f32(x) for x in getattr(cam, n)) for n in ("position", "basis_x", "basis_y", "basis_z"))


# ---------------------------------------------------------------- literal restatement (math.rs:503-652, draw.rs:12-67)
def _sub(a, b):                                                # Vec3 - Vec3
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):                                                # Vec3::dot, math.rs:23-25
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _perspective(cam_x, cam_y, cam_z, w, h):                   # math.rs:524-531 (and :564-571, :606-613, :642-649)
    scale = f32(0.75)
    vs = (f32(min(w, h)) / f32(2.0)) * scale
    ud = f32(5.0)
    us = ud - f32(1.0)
    denom = cam_z + ud
    sx = (cam_x * us / denom) * vs + (f32(w) / f32(2.0))
    sy = (cam_y * us / denom) * vs + (f32(h) / f32(2.0))
    return sx, sy


def ref_world_to_screen(p, cam, w, h):
    """world_to_screen (math.rs:503-534) and world_to_screen_with_depth (:621-652: the same expressions, cam_z returned too)."""
    pos, bx, by, bz = cam
    rel = _sub(p, pos)
    cam_z = _dot(rel, bz)
    if cam_z <= f32(0.1):
        return None
    cam_x = _dot(rel, bx)
    cam_y = _dot(rel, by)
    sx, sy = _perspective(cam_x, cam_y, cam_z, w, h)
    return sx, sy, cam_z


def ref_world_to_screen_with_ortho(p, cam, w, h, ortho):
    """world_to_screen_with_ortho (math.rs:538-575) and world_to_screen_with_ortho_depth (:580-617: cam_z returned too)."""
    pos, bx, by, bz = cam
    rel = _sub(p, pos)
    cam_x = _dot(rel, bx)
    cam_y = _dot(rel, by)
    cam_z = _dot(rel, bz)
    if ortho is not None:
        zoom, cx, cy = (f32(v) for v in ortho)
        sx = (cam_x - cx) * zoom + (f32(w) / f32(2.0))
        sy = -(cam_y - cy) * zoom + (f32(h) / f32(2.0))
        return sx, sy, cam_z
    if cam_z <= f32(0.1):
        return None
    sx, sy = _perspective(cam_x, cam_y, cam_z, w, h)
    return sx, sy, cam_z


def ref_clip(p0, p1, cam):
    """draw_3d_line_clipped's clip, draw.rs:19-42: None (both behind) or the two ends to project."""
    pos, _, _, bz = cam
    z0 = _dot(_sub(p0, pos), bz)
    z1 = _dot(_sub(p1, pos), bz)
    if z0 <= NEAR and z1 <= NEAR:
        return None
    if z0 <= NEAR:
        t = (NEAR - z0) / (z1 - z0)
        d = _sub(p1, p0)
        return (p0[0] + d[0] * t, p0[1] + d[1] * t, p0[2] + d[2] * t), p1
    if z1 <= NEAR:
        t = (NEAR - z0) / (z1 - z0)
        d = _sub(p1, p0)
        return p0, (p0[0] + d[0] * t, p0[1] + d[1] * t, p0[2] + d[2] * t)
    return p0, p1


def _same(a, b):
    return a.tobytes() == b.tobytes()


def noop_records(n):
    """Records that draw nothing: a circle of radius -1 (PrimPass::bounds), everything else zero."""
    P = np.zeros(n, abi.PRIM_DTYPE)
    P["kind"] = abi.PRIM_CIRCLE; P["size"] = -1
    return P


def ref_world(items, camera, ortho, w, h):
    """(records, (drawn, dropped, rejected)) of `items` (abi.WORLD_ITEM_DTYPE), one reference call after another."""
    cam = _cam_f32(camera)
    out = noop_records(len(items))
    counts = [0, 0, 0]
    with np.errstate(all="ignore"):
        for i, it in enumerate(items):
            kind = int(it["kind"])
            p0 = tuple(f32(v) for v in it["p0"]); p1 = tuple(f32(v) for v in it["p1"])
            circle = kind in CIRCLE_KINDS
            if circle:
                ends = (ref_world_to_screen_with_ortho(p0, cam, w, h, ortho),)
            elif int(it["flags"]) & abi.WORLD_CLIP_NEAR:
                cl = ref_clip(p0, p1, cam)
                ends = (None,) if cl is None else tuple(ref_world_to_screen(p, cam, w, h) for p in cl)
            else:
                ends = tuple(ref_world_to_screen_with_ortho(p, cam, w, h, ortho) for p in (p0, p1))
            if any(e is None for e in ends):
                counts[1] += 1
                continue
            xy = [(_as_i32(e[0]), _as_i32(e[1])) for e in ends]
            if circle:
                bad = abs(xy[0][0]) >= LIM or abs(xy[0][1]) >= LIM
            else:
                bad = abs(xy[1][0] - xy[0][0]) >= LIM or abs(xy[1][1] - xy[0][1]) >= LIM
            if bad:                                            # b32_draw_prims's B32_E_UNSUPPORTED rules: a no-op, counted
                counts[2] += 1
                continue
            counts[0] += 1
            r = out[i]
            r["x0"], r["y0"] = xy[0]
            if not circle:
                r["x1"], r["y1"] = xy[1]
                if kind in DEPTH_KINDS:
                    r["z0"], r["z1"] = (QNAN if np.isnan(e[2]) else e[2] for e in ends)
            for f in ("size", "r", "g", "b", "blend", "kind", "alpha", "mode"):
                r[f] = it[f]
    return out, tuple(counts)


# ---------------------------------------------------------------- vectorised model
def _as_i32_vec(v):
    x = np.asarray(v, f32).astype(np.float64)
    x = np.where(np.isnan(x), 0.0, x)
    return np.trunc(np.clip(x, -2147483648.0, 2147483647.0)).astype(np.int64)


def _vdot(r, b):
    return (r[:, 0] * b[0] + r[:, 1] * b[1]) + r[:, 2] * b[2]


def np_world(items, camera, ortho, w, h):
    """ref_world, vectorised over the batch."""
    I = np.ascontiguousarray(items, abi.WORLD_ITEM_DTYPE).reshape(-1)
    n = len(I)
    pos, bx, by, bz = (np.array(v, f32) for v in _cam_f32(camera))
    kind = I["kind"]
    circle = np.isin(kind, CIRCLE_KINDS)
    depth = np.isin(kind, DEPTH_KINDS)
    clip = ((I["flags"] & abi.WORLD_CLIP_NEAR) != 0) & ~circle
    P0 = I["p0"].astype(f32).copy(); P1 = I["p1"].astype(f32).copy()
    with np.errstate(all="ignore"):
        z0 = _vdot(P0 - pos, bz); z1 = _vdot(P1 - pos, bz)
        b0 = z0 <= NEAR; b1 = z1 <= NEAR
        t = (NEAR - z0) / (z1 - z0)
        Q = P0 + (P1 - P0) * t[:, None]
        some = ~(clip & b0 & b1)
        r0 = clip & b0 & ~b1; r1 = clip & ~b0 & b1
        P0 = np.where(r0[:, None], Q, P0); P1 = np.where(r1[:, None], Q, P1)
        use_ortho = np.full(n, ortho is not None) & ~clip
        zoom, ocx, ocy = (f32(v) for v in (ortho if ortho is not None else (0, 0, 0)))
        vs = (f32(min(w, h)) / f32(2.0)) * f32(0.75)
        hw, hh = f32(w) / f32(2.0), f32(h) / f32(2.0)
        scr = []
        for P in (P0, P1):
            rel = P - pos
            cx, cy, cz = _vdot(rel, bx), _vdot(rel, by), _vdot(rel, bz)
            denom = cz + f32(5.0)
            sx = np.where(use_ortho, (cx - ocx) * zoom + hw, (cx * f32(4.0) / denom) * vs + hw)
            sy = np.where(use_ortho, -(cy - ocy) * zoom + hh, (cy * f32(4.0) / denom) * vs + hh)
            scr.append((_as_i32_vec(sx), _as_i32_vec(sy), cz, use_ortho | ~(cz <= f32(0.1))))
    some &= scr[0][3] & (circle | scr[1][3])
    x0, y0, x1, y1 = scr[0][0], scr[0][1], np.where(circle, 0, scr[1][0]), np.where(circle, 0, scr[1][1])
    bad = np.where(circle, (np.abs(x0) >= LIM) | (np.abs(y0) >= LIM), (np.abs(x1 - x0) >= LIM) | (np.abs(y1 - y0) >= LIM))
    draw = some & ~bad
    out = noop_records(n)
    for f, v in (("x0", x0), ("y0", y0), ("x1", x1), ("y1", y1)):
        out[f] = np.where(draw, v, 0)
    for f, z in (("z0", scr[0][2]), ("z1", scr[1][2])):
        out[f] = np.where(draw & depth, np.where(np.isnan(z), QNAN, z), f32(0.0))
    for f in ("size", "r", "g", "b", "blend", "kind", "alpha", "mode"):
        out[f] = np.where(draw, I[f], out[f])
    return out, (int(draw.sum()), int((~some).sum()), int((some & bad).sum()))


# ---------------------------------------------------------------- batches
def random_items(rng, n, camera, kinds=LINE_KINDS + CIRCLE_KINDS, spread=(1500.0, 1000.0), depth=(-400.0, 3000.0), seg=120.0, clip_p=0.5):
    """Items around the camera's view: one end `depth` along basis_z (some behind), the other within `seg` of it (so segments cross the
    near plane now and then)."""
    pos, bx, by, bz = (np.array(v, np.float64) for v in (camera.position, camera.basis_x, camera.basis_y, camera.basis_z))
    I = np.zeros(n, abi.WORLD_ITEM_DTYPE)
    a = pos + rng.uniform(*depth, (n, 1)) * bz + rng.uniform(-spread[0], spread[0], (n, 1)) * bx + rng.uniform(-spread[1], spread[1], (n, 1)) * by
    I["p0"] = a.astype(f32); I["p1"] = (a + rng.uniform(-seg, seg, (n, 3))).astype(f32)
    I["kind"] = rng.choice(np.array(kinds, np.uint8), n)
    circle = np.isin(I["kind"], CIRCLE_KINDS)
    I["size"] = np.where(circle, rng.integers(-1, 9, n), rng.choice(np.array([-2, 0, 1, 2, 3, 5], np.int32), n))
    I["r"], I["g"], I["b"] = (rng.integers(0, 256, n) for _ in range(3))
    I["blend"] = np.where(rng.random(n) < 0.15, abi.ERASE, abi.OPAQUE)
    I["alpha"] = rng.choice(np.array([0, 1, 128, 140, 191, 255], np.uint8), n)
    I["mode"] = rng.integers(0, 6, n)
    I["flags"] = np.where(~circle & (rng.random(n) < clip_p), abi.WORLD_CLIP_NEAR, 0)
    return I


def hostile_items(rng, n, camera):
    """random_items with NaN, +-inf and 1e30 coordinates, ends exactly on cam_z == 0.1 (for the identity camera at the origin: z = 0.1f),
    around it by one ulp, and z0 == z1."""
    I = random_items(rng, n, camera)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, 1e-40, 0.0, -0.0], f32)
    for end in ("p0", "p1"):
        m = rng.random((n, 3)) < 0.04
        I[end] = np.where(m, rng.choice(bad, (n, 3)), I[end])
    pz = np.array(camera.position, f32)[2]
    edge = np.array([NEAR, np.nextafter(NEAR, f32(1)), np.nextafter(NEAR, f32(-1))], f32) + pz
    for end in ("p0", "p1"):
        m = rng.random(n) < 0.08
        I[end][:, 2] = np.where(m, rng.choice(edge, n), I[end][:, 2])
    m = rng.random(n) < 0.05                                      # z0 == z1 (t = x / 0)
    I["p1"][:, 2] = np.where(m, I["p0"][:, 2], I["p1"][:, 2])
    m = rng.random(n) < 0.03                                      # both ends the same point
    I["p1"] = np.where(m[:, None], I["p0"], I["p1"])
    return I


def the_20000(rng_seed=2024):
    """The 20 000 items of the CPU comparison and the GPU stage tap: (camera, items) pairs -- every kind, flag, plain and hostile."""
    rng = np.random.default_rng(rng_seed)
    return [(IDENTITY_CAM, hostile_items(rng, 6000, IDENTITY_CAM)), (CENSUS_CAM, hostile_items(rng, 4000, CENSUS_CAM)),
            (IDENTITY_CAM, random_items(rng, 4000, IDENTITY_CAM)), (GRID_CAMS[1], random_items(rng, 3000, GRID_CAMS[1], seg=2000.0)),
            (GRID_CAMS[2], random_items(rng, 3000, GRID_CAMS[2], depth=(-50.0, 200.0), seg=300.0))]


GRID_COLORS = (b32.Color(60, 60, 70), b32.Color(200, 40, 40), b32.Color(40, 40, 200))


def grid_items(y=0.0, spacing=1024.0, extent=10240.0):
    from bonnie32_amd import rasterizer as R
    return R.floor_grid_items(y, spacing, extent, *GRID_COLORS)


def census(items, camera, w, h):
    """(behind, unclipped, clipped and drawn, clipped and vanished) of clipped line items, by the literal model."""
    cam = _cam_f32(camera)
    c = [0, 0, 0, 0]
    with np.errstate(all="ignore"):
        for it in items:
            p0 = tuple(f32(v) for v in it["p0"]); p1 = tuple(f32(v) for v in it["p1"])
            cl = ref_clip(p0, p1, cam)
            if cl is None:
                c[0] += 1
            elif cl == (p0, p1):
                c[1] += 1
            elif all(ref_world_to_screen(p, cam, w, h) is not None for p in cl):
                c[2] += 1
            else:
                c[3] += 1
    return tuple(c)


# ---------------------------------------------------------------- exact arithmetic (the hand computation of the clip)
def _rn(x):
    """A rational rounded to the nearest f32 (ties to even), as a Fraction; normal range only."""
    x = Fraction(x)
    if x == 0:
        return x
    s = -1 if x < 0 else 1
    x = abs(x)
    e = 0
    while x >= 2:
        x /= 2; e += 1
    while x < 1:
        x *= 2; e -= 1
    assert -126 <= e <= 127
    m = x * (1 << 23)
    q, r = divmod(m.numerator, m.denominator)
    if 2 * r > m.denominator or (2 * r == m.denominator and q & 1):
        q += 1
    return s * Fraction(q, 1 << 23) * Fraction(2) ** e


def exact_clipped(p0, p1, cam, w, h):
    """draw_3d_line_clipped with every operation an exact rational operation followed by _rn: None / 'vanished' / (x0, y0, x1, y1)."""
    F = lambda v: Fraction(float(v))
    pos, bx, by, bz = ([F(x) for x in v] for v in cam)
    p0 = [F(v) for v in p0]; p1 = [F(v) for v in p1]
    near = F(f32(0.1))
    sub = lambda a, b: [_rn(a[k] - b[k]) for k in range(3)]
    dot = lambda a, b: _rn(_rn(_rn(a[0] * b[0]) + _rn(a[1] * b[1])) + _rn(a[2] * b[2]))
    z0, z1 = dot(sub(p0, pos), bz), dot(sub(p1, pos), bz)
    if z0 <= near and z1 <= near:
        return None
    if z0 <= near or z1 <= near:
        t = _rn(_rn(near - z0) / _rn(z1 - z0))
        d = sub(p1, p0)
        q = [_rn(p0[k] + _rn(d[k] * t)) for k in range(3)]
        p0, p1 = (q, p1) if z0 <= near else (p0, q)
    out = []
    for p in (p0, p1):
        rel = sub(p, pos)
        cz = dot(rel, bz)
        if cz <= near:
            return "vanished"
        cx, cy = dot(rel, bx), dot(rel, by)
        vs = _rn(_rn(Fraction(min(w, h)) / 2) * Fraction(3, 4))
        denom = _rn(cz + 5)
        for c, half in ((cx, Fraction(w) / 2), (cy, Fraction(h) / 2)):
            s = _rn(_rn(_rn(_rn(c * 4) / denom) * vs) + half)
            out.append(int(s))                                  # toward zero, like `as i32` (in range here)
    return tuple(out)


# ---------------------------------------------------------------- CPU
def test_world_item_layout_matches_c():
    """B32WorldItem / B32Ortho compiled with gcc against the public header have the layout of abi.WORLD_ITEM_DTYPE / abi.B32Ortho."""
    import ctypes as C
    fields = ("p0", "p1", "size", "r", "g", "b", "blend", "kind", "alpha", "mode", "flags", "_pad")
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void){ printf("%zu %zu", sizeof(B32WorldItem), sizeof(B32Ortho));'
            + "".join(f' printf(" %zu", offsetof(B32WorldItem, {f}));' for f in fields) + ' printf(" %u\\n", B32_WORLD_CLIP_NEAR); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == abi.WORLD_ITEM_DTYPE.itemsize == 40 and out[1] == C.sizeof(abi.B32Ortho) == 12
    assert out[2:2 + len(fields)] == [abi.WORLD_ITEM_DTYPE.fields[f][1] for f in fields]
    assert out[-1] == abi.WORLD_CLIP_NEAR == 1
    from bonnie32_amd import rasterizer as R
    assert R.Context.WORLD_ROUTES == ("world_tiles", "world_scan") and len(R.Context.ROUTES) == 18      # b32_route_count 18, 19


def test_ref_world_hand_cases():
    """Identity basis, camera at the origin, 320x240: vs = 90; (10, 20, 95) lands at (10*4/100*90 + 160, 20*4/100*90 + 120) = (196, 192).
    Ortho (zoom 2, centre (1, -3)): sx = (10 - 1) * 2 + 160 = 178, sy = -(20 + 3) * 2 + 120 = 74.  cam_z == 0.1 is None, the next f32 is not."""
    from bonnie32_amd import rasterizer as R
    c = b32.Color(9, 8, 7, abi.ERASE)
    W, H = 320, 240
    b = R.WorldBatch(None)
    b.circle((10, 20, 95), 3, c)
    b.line_3d((10, 20, 95), (-10, -20, 45), c)                 # (-10*4/50*90 + 160, -20*4/50*90 + 120) = (88, -24), z = 45
    b.line((10, 20, 95), (0, 0, 0.1), c)                       # second end: cam_z <= 0.1 -> None
    b.line((10, 20, 95), (0, 0, float(np.nextafter(NEAR, f32(1)))), c)   # just in front: (160, 120)
    b.line_clipped((0, 0, -3), (0, 0, -1), c)                  # both behind
    b.circle_alpha((0, 0, -50), 2, c, 140)                     # behind: None
    b.thick_line((10, 20, 95), (-10, -20, 45), 3, c)
    I = b.items()
    P, counts = ref_world(I, IDENTITY_CAM, None, W, H)
    assert counts == (4, 3, 0)
    assert (P[0]["x0"], P[0]["y0"], P[0]["x1"], P[0]["y1"], P[0]["size"], P[0]["kind"]) == (196, 192, 0, 0, 3, abi.PRIM_CIRCLE)
    assert (P[1]["x0"], P[1]["y0"], P[1]["z0"], P[1]["x1"], P[1]["y1"], P[1]["z1"], P[1]["kind"]) == (196, 192, 95.0, 88, -24, 45.0, abi.LINE_3D)
    assert (P[3]["x0"], P[3]["y0"], P[3]["x1"], P[3]["y1"], P[3]["z0"], P[3]["z1"]) == (196, 192, 160, 120, 0.0, 0.0)       # 2-D kinds carry no depth
    assert (P[6]["x1"], P[6]["y1"], P[6]["size"], P[6]["kind"]) == (88, -24, 3, abi.PRIM_THICK_LINE)
    noop = noop_records(1)[0]
    assert all(_same(P[i], noop) for i in (2, 4, 5))
    assert (P[[0, 1, 3, 6]]["blend"] == abi.ERASE).all() and (P[[0, 1, 3, 6]]["r"] == 9).all() and P[0]["alpha"] == 255
    Po, co = ref_world(I, IDENTITY_CAM, (2.0, 1.0, -3.0), W, H)
    assert co == (6, 1, 0)                                      # ortho never answers None; the clipped line ignores it and stays behind
    assert (Po[0]["x0"], Po[0]["y0"]) == (178, 74) and (Po[5]["x0"], Po[5]["y0"]) == (158, 114) and Po[1]["z1"] == 45.0
    assert _same(Po[4], noop)
    far = R.world_item(abi.LINE_2D, (10, 20, 95), (3e9, 0, 0.2), c)           # sx ~ 2e11 -> i32::MAX: the extent rule
    farc = R.world_item(abi.PRIM_CIRCLE, (-3e9, 0, 0.2), (0, 0, 0), c, size=2)  # centre at i32::MIN
    Pf, cf = ref_world(np.concatenate([far, farc, I[:1]]), IDENTITY_CAM, None, W, H)
    assert cf == (1, 0, 2) and _same(Pf[0], noop) and _same(Pf[1], noop) and _same(Pf[2], P[0])


def _clipped_ints(p0, p1, cam, w, h):
    cl = ref_clip(p0, p1, cam)
    ends = [ref_world_to_screen(p, cam, w, h) for p in cl]
    return "vanished" if any(e is None for e in ends) else tuple(v for e in ends for v in (_as_i32(e[0]), _as_i32(e[1])))


def test_ref_world_clip_hand_cases():
    """Two clipped segments worked by hand, camera at the origin with the identity basis, 320x240 (vs = 90).  The clipped end lies ON the
    near plane by construction, so its second projection always hangs on a few ulps of z against 0.1f; the operands here are chosen so
    that every rounding can be followed in integers.  u = 2^-27; 0.1f = 13421773 u (N).

    Drawn: (0, 0, -0.5) -> (6, 3, 1).  NEAR - z0 = 80530637 u -> 80530640 u (ulp 8 u); z1 - z0 = 1.5; t = 53687093.3 u -> 53687092 u (ulp 4 u:
    exactly 0.4f).  d * t: 1.5 t = 80530638 u -> 80530640 u, so new z = -0.5 + 0.6000000238 = 13421776 u: 3 ulps IN FRONT of 0.1f -- drawn.
    new x = 6 t -> 2.4000000954, new y = 3 t -> 1.2000000477; denom = 5.1f; sx = 9.6000004 / 5.1 * 90 + 160 = 329.41, sy = 4.8000002 / 5.1
    * 90 + 120 = 204.70; the far end: (6 * 4 / 6 * 90 + 160, 3 * 4 / 6 * 90 + 120) = (520, 300).

    Vanished: (0, 0, -N) -> (8, 4, f32(0.3)).  f32(0.3) = 40265320 u (3 N = 40265319 u is a tie in its binade, to even); NEAR - z0 = 2 N exactly;
    z1 - z0 = 53687093 u -> 53687092 u = 4 N (ulp 4 u); t = 2 N / 4 N = 0.5 exactly; new z = -N + 4 N * 0.5 = N exactly: cam_z <= 0.1 -> None."""
    W, H = 320, 240
    cam = _cam_f32(IDENTITY_CAM)
    u = 2.0 ** -27
    assert float(NEAR) == 13421773 * u and float(f32(0.3)) == 40265320 * u and float(f32(0.4)) == 53687092 * u
    p0 = tuple(f32(v) for v in (0, 0, -0.5)); p1 = tuple(f32(v) for v in (6, 3, 1))
    cl = ref_clip(p0, p1, cam)
    assert cl[1] == p1 and float(cl[0][2]) == 13421776 * u and float(cl[0][0]) == 322122560 * u and float(cl[0][1]) == 161061280 * u
    assert _clipped_ints(p0, p1, cam, W, H) == (329, 204, 520, 300) == exact_clipped(p0, p1, cam, W, H)
    assert _clipped_ints(p1, p0, cam, W, H)[:2] == (520, 300)           # the other branch (z1 <= NEAR): the same t, the second end replaced
    q0 = (f32(0), f32(0), -NEAR); q1 = (f32(8), f32(4), f32(0.3))
    cl = ref_clip(q0, q1, cam)
    assert cl[1] == q1 and cl[0] == (f32(4), f32(2), NEAR)
    assert _clipped_ints(q0, q1, cam, W, H) == "vanished" == exact_clipped(q0, q1, cam, W, H)
    from bonnie32_amd import rasterizer as R
    c = b32.Color(1, 2, 3)
    I = np.concatenate([R.world_item(abi.LINE_2D, p0, p1, c, flags=1), R.world_item(abi.LINE_3D, q0, q1, c, flags=1), R.world_item(abi.LINE_3D, p0, p1, c, flags=1)])
    P, counts = ref_world(I, IDENTITY_CAM, (2.0, 1.0, -3.0), W, H)         # (the ortho is ignored by clipped items)
    assert counts == (2, 1, 0) and _same(P[1], noop_records(1)[0])
    assert (P[0]["x0"], P[0]["y0"], P[0]["x1"], P[0]["y1"], P[0]["z0"]) == (329, 204, 520, 300, 0.0)
    assert (P[2]["x0"], P[2]["y0"], P[2]["x1"], P[2]["y1"], float(P[2]["z0"]), P[2]["z1"]) == (329, 204, 520, 300, 13421776 * u, 1.0)


def test_ref_world_clip_exact_arithmetic():
    """The literal model's clip against the same expressions in exact rational arithmetic with an explicit round-to-nearest-even: one
    segment on the knife's edge ((0, 0, -0.9) -> (8, 4, 3.1): t ~ 1 / 4, the new end ~ (2, 1, 0.1)), then every clipped segment of the floor
    grid under the census camera -- the two agree on drawn / vanished and on the integers."""
    W, H = 320, 240
    cam = _cam_f32(IDENTITY_CAM)
    p0 = tuple(f32(v) for v in (0, 0, -0.9)); p1 = tuple(f32(v) for v in (8, 4, 3.1))
    assert _clipped_ints(p0, p1, cam, W, H) == exact_clipped(p0, p1, cam, W, H)
    G = grid_items()
    gcam = _cam_f32(CENSUS_CAM)
    seen = {"vanished": 0, "drawn": 0}
    for it in G:
        q0 = tuple(f32(v) for v in it["p0"]); q1 = tuple(f32(v) for v in it["p1"])
        cl = ref_clip(q0, q1, gcam)
        if cl is None or cl == (q0, q1):
            continue
        want = exact_clipped(q0, q1, gcam, W, H)
        P, _ = ref_world(np.atleast_1d(it), CENSUS_CAM, None, W, H)
        if want == "vanished":
            assert _same(P[0], noop_records(1)[0])
        else:
            assert (P[0]["x0"], P[0]["y0"], P[0]["x1"], P[0]["y1"]) == want
        seen["vanished" if want == "vanished" else "drawn"] += 1
    assert seen == {"vanished": 11, "drawn": 12}


def test_floor_grid_generator_and_census():
    """draw_floor_grid(0, 1024, 10240): 840 segments, 20 of each axis colour, in the reference's order; under the census camera 347 lie
    behind, 470 are not clipped, 12 are clipped and drawn and 11 are clipped and VANISH (the clipped end projects to None), at 320x240 and
    at 2560x1920 alike; the other two grid cameras reach both clipped branches too."""
    G = grid_items()
    assert len(G) == 840 and (G["kind"] == abi.LINE_2D).all() and (G["flags"] == abi.WORLD_CLIP_NEAR).all()
    rgb = np.stack([G["r"], G["g"], G["b"]], 1)
    assert int((rgb == [40, 40, 200]).all(1).sum()) == 20 and int((rgb == [200, 40, 40]).all(1).sum()) == 20
    assert (G[:420]["p0"][:, 2] == G[:420]["p1"][:, 2]).all() and (G[420:]["p0"][:, 0] == G[420:]["p1"][:, 0]).all()     # X-parallel first
    zax = (rgb[:420] == [40, 40, 200]).all(1)
    assert (G[:420]["p0"][zax][:, 2] == 0).all() and (G[420:]["p0"][(rgb[420:] == [200, 40, 40]).all(1)][:, 0] == 0).all()   # z ~ 0: z_axis_color
    assert tuple(G[0]["p0"]) == (-10240.0, 0.0, -10240.0) and tuple(G[0]["p1"]) == (-9216.0, 0.0, -10240.0) and tuple(G[-1]["p1"]) == (10240.0, 0.0, 10240.0)
    for w, h in SIZES:
        assert census(G, CENSUS_CAM, w, h) == (347, 470, 12, 11)
        assert census(G, GRID_CAMS[1], w, h)[2:] == (11, 22)
        assert census(G, GRID_CAMS[2], w, h)[2:] == (18, 16)
        P, counts = np_world(G, CENSUS_CAM, None, w, h)
        assert counts == (482, 358, 0)
    # an extent that is no multiple of the spacing: the last segment is cut by .min(extent); f32 accumulation
    G2 = grid_items(3.5, 0.3, 1.0)
    row = G2[:int(np.nonzero(G2["p0"][1:, 0] == f32(-1.0))[0][0]) + 1]      # the first X-parallel line
    assert 7 <= len(row) <= 8 and (row["p0"][:, 2] == f32(-1.0)).all() and (row["p1"][:, 0] <= f32(1.0)).all() and row["p1"][-1, 0] == f32(1.0) and (row["p0"][:, 1] == f32(3.5)).all()
    x = f32(-1.0)
    for r in row:
        assert r["p0"][0] == x
        x = f32(x + f32(0.3))
    from bonnie32_amd import rasterizer as R
    for bad in ((0, 0.0, 10), (0, -1.0, 10), (float("nan"), 1, 10), (0, float("inf"), 10), (0, 1, float("inf")), (0, 1e-3, 1e6), (0, 1.0, 1e30)):
        with pytest.raises(ValueError):
            R.floor_grid_items(*bad, *GRID_COLORS)
    with pytest.raises(OverflowError):
        R.floor_grid_items(0, 1.0, 1000.0, *GRID_COLORS)           # 2001 * 2000 * 2 segments
    assert len(R.floor_grid_items(0, 1.0, -5.0, *GRID_COLORS)) == 0


def test_floor_grid_generator_equals_library():
    """b32_floor_grid_items (host code of the library, no device needed) builds the same items byte for byte, and refuses what the Python
    generator refuses."""
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    lib = abi.load_library()
    from bonnie32_amd import rasterizer as R
    cols = [(C.c_uint8 * 4)(c.r, c.g, c.b, c.blend) for c in GRID_COLORS]

    def lib_items(y, spacing, extent):
        n = C.c_uint32()
        rc = lib.b32_floor_grid_items(y, spacing, extent, *cols, None, 0, C.byref(n))
        if rc:
            return rc
        out = np.zeros(n.value, abi.WORLD_ITEM_DTYPE)
        assert lib.b32_floor_grid_items(y, spacing, extent, *cols, out.ctypes.data if n.value else None, n.value, C.byref(n)) == 0 and n.value == len(out)
        return out

    for args in ((0.0, 1024.0, 10240.0), (3.5, 0.3, 1.0), (-7.25, 100.0, 1234.5), (0.0, 0.1, 3.0), (1.0, 5.0, 0.0), (0.0, 1.0, -5.0), (0.0, 7.0, 3.0)):
        got = lib_items(*args)
        want = R.floor_grid_items(*args, *GRID_COLORS)
        assert not isinstance(got, int) and got.tobytes() == want.tobytes(), args
    for bad in ((0, 0.0, 10), (0, -1.0, 10), (float("nan"), 1, 10), (0, float("inf"), 10), (0, 1, float("inf")), (0, 1e-3, 1e6), (0, 1.0, 1e30)):
        assert lib_items(*bad) == abi.B32_E_ARG, bad
    assert lib_items(0, 1.0, 1000.0) == abi.B32_E_UNSUPPORTED


def test_vectorised_world_model_equals_literal_model():
    """np_world == ref_world record for record on 20 000 random items of every kind, flag and both projections, hostile inputs included
    (NaN, +-inf, 1e30, ends exactly on cam_z == 0.1, z0 == z1); every branch is reached."""
    total = 0
    reached = np.zeros(3, np.int64)
    for k, (cam, I) in enumerate(the_20000()):
        total += len(I)
        for ortho in (None, ORTHO):
            for w, h in SIZES:
                got, gc = np_world(I, cam, ortho, w, h)
                want, wc = ref_world(I, cam, ortho, w, h)
                assert gc == wc and sum(gc) == len(I)
                assert got.tobytes() == want.tobytes(), f"batch {k} {w}x{h}: records {np.nonzero(got != want)[0][:8]} differ"
                reached += gc
    assert total == 20000 and (reached > 50).all()
    I = np.concatenate([I for _, I in the_20000()])
    assert set(np.unique(I["kind"])) == set(range(9)) and set(np.unique(I["flags"])) == {0, 1}
    assert np.isnan(I["p0"]).any() and np.isinf(I["p1"]).any() and (I["p0"][:, 2] == NEAR).any()


@functools.lru_cache(maxsize=None)
def _world_host_exe():
    d = tempfile.mkdtemp(prefix="b32_world_host_")
    atexit.register(shutil.rmtree, d, True)
    exe = os.path.join(d, "world_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bonnie-32_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "world_host.cpp"), "-o", exe], check=True)
    return exe


def host_world(items, camera, ortho, w, h):
    """(records, counts, which) from b32_world_body.h compiled for the host."""
    items = np.ascontiguousarray(items, abi.WORLD_ITEM_DTYPE).reshape(-1)
    exe = _world_host_exe()
    fin, fout = exe + ".in", exe + ".out"
    with open(fin, "wb") as fh:
        fh.write(np.array([w, h, int(ortho is not None), len(items)], np.uint32).tobytes())
        fh.write(np.array([v for g in _cam_f32(camera) for v in g], f32).tobytes())
        fh.write(np.array(ortho if ortho is not None else (0, 0, 0), f32).tobytes())
        fh.write(items.tobytes())
    subprocess.run([exe, fin, fout], check=True)
    blob = open(fout, "rb").read()
    assert len(blob) == 24 + 44 * len(items)
    counts = tuple(int(v) for v in np.frombuffer(blob, np.uint64, 3))
    which = np.frombuffer(blob, np.uint32, len(items), 24)
    return np.frombuffer(blob, abi.PRIM_DTYPE, len(items), 24 + 4 * len(items)), counts, which


def test_world_body_on_the_host_equals_the_models():
    """csrc/b32_world_body.h built for the host (g++ -O1 -ffp-contract=off -Wall -Werror): the records, the per-item outcomes and the
    counts equal np_world bit for bit on the 20 000 items (both sizes, perspective and ortho), and ref_world item by item on 400 hostile
    items of every kind, with and without the clip flag."""
    noop = noop_records(1).tobytes()
    for k, (cam, I) in enumerate(the_20000()):
        for ortho in (None, ORTHO):
            for w, h in SIZES:
                want, wc = np_world(I, cam, ortho, w, h)
                got, gc, which = host_world(I, cam, ortho, w, h)
                assert got.tobytes() == want.tobytes(), f"batch {k} {w}x{h} ortho={ortho}: records {np.nonzero(got != want)[0][:8]} differ"
                assert gc == wc and tuple(np.bincount(which, minlength=3)) == wc
                assert all(got[i].tobytes() == noop for i in np.nonzero(which != 0)[0])
    I = hostile_items(np.random.default_rng(77), 400, IDENTITY_CAM)
    lines = ~np.isin(I["kind"], CIRCLE_KINDS)
    assert set(np.unique(I["kind"])) == set(range(9))
    assert all({0, 1} == set(I["flags"][I["kind"] == kd]) for kd in LINE_KINDS) and (I["flags"][~lines] == 0).all()
    for ortho in (None, ORTHO):
        want, wc = ref_world(I, IDENTITY_CAM, ortho, 320, 240)
        got, gc, which = host_world(I, IDENTITY_CAM, ortho, 320, 240)
        assert got.tobytes() == want.tobytes() and gc == wc and min(wc) > 0
        each = [ref_world(I[i:i + 1], IDENTITY_CAM, ortho, 320, 240)[1].index(1) for i in range(len(I))]
        assert list(which) == each


def test_cpp_mirror_world_compiles():
    """host/rasterizer.hpp: the world-space methods and the WorldBatch builder compile (header-only over the C ABI)."""
    hpp_dir = os.path.join(ROOT, "bonnie-32_amd", "host")
    src = ('#include "rasterizer.hpp"\nvoid f(b32::Framebuffer& fb, const b32::Camera& cam) { b32::Color c{ 1, 2, 3, b32::BlendMode::Erase };\n'
           ' fb.draw_3d_line_clipped(cam, b32::Vec3{ 0, 0, -1 }, b32::Vec3{ 1, 2, 3 }, c); fb.draw_floor_grid(cam, 0.0f, 1024.0f, 10240.0f, c, c, c);\n'
           ' fb.draw_world(std::vector<B32WorldItem>{ b32::Framebuffer::world_item(B32_PRIM_CIRCLE, b32::Vec3{ 1, 1, 9 }, b32::Vec3{}, c, 3) }, cam, b32::Vec3{ 2, 0, 0 });\n'
           ' b32::WorldBatch b(fb); b.line_clipped({ 0, 0, 0 }, { 1, 1, 1 }, c); b.line_clipped_3d({ 0, 0, 0 }, { 1, 1, 1 }, c); b.line({ 0, 0, 0 }, { 1, 1, 1 }, c);\n'
           ' b.line_alpha({ 0, 0, 0 }, { 1, 1, 1 }, c, 9); b.line_3d({ 0, 0, 0 }, { 1, 1, 1 }, c); b.line_3d_overlay({ 0, 0, 0 }, { 1, 1, 1 }, c);\n'
           ' b.line_3d_alpha({ 0, 0, 0 }, { 1, 1, 1 }, c, 191); b.line_blended({ 0, 0, 0 }, { 1, 1, 1 }, c, b32::BlendMode::Add); b.thick_line({ 0, 0, 0 }, { 1, 1, 1 }, 3, c);\n'
           ' b.circle({ 0, 0, 9 }, 5, c); b.circle_alpha({ 0, 0, 9 }, 3, c, 140); if (b.size() == 11) b.flush(cam);\n'
           ' const auto n = fb.world_counts(); (void)(n.drawn + n.dropped + n.rejected); }\nint main() { (void)&f; return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", hpp_dir, "-I", os.path.join(ROOT, "include"),
                        os.path.join(d, "t.cpp")], check=True)


def test_python_world_batch_records():
    """WorldBatch records the world-space calls in call order."""
    from bonnie32_amd import rasterizer as R
    b = R.WorldBatch(None)
    c = b32.Color(1, 2, 3, abi.ERASE)
    b.line_clipped((1, 2, 3), (4, 5, 6), c); b.line_3d_alpha((0, 0, 1), (0, 0, 2), c, 191); b.circle_alpha((7, 8, 9), 3, c, 140)
    b.thick_line((0, 0, 0), (1, 1, 1), 4, c); b.line_blended((0, 0, 0), (1, 1, 1), c, abi.ADD); b.line_clipped_3d((0, 0, 0), (1, 1, 1), c)
    I = b.items()
    assert len(b) == 6 and I.dtype == abi.WORLD_ITEM_DTYPE
    assert list(I["kind"]) == [abi.LINE_2D, abi.LINE_3D_ALPHA, abi.PRIM_CIRCLE_ALPHA, abi.PRIM_THICK_LINE, abi.PRIM_LINE_BLENDED, abi.LINE_3D]
    assert list(I["flags"]) == [1, 0, 0, 0, 0, 1] and tuple(I[0]["p1"]) == (4.0, 5.0, 6.0) and tuple(I[2]["p0"]) == (7.0, 8.0, 9.0)
    assert (I[1]["alpha"], I[2]["size"], I[2]["alpha"], I[3]["size"], I[4]["mode"]) == (191, 3, 140, 4, abi.ADD)
    assert (I["blend"] == abi.ERASE).all() and (I["b"] == 3).all()


# ---------------------------------------------------------------- GPU
def _frame_items(rng, n, camera, **kw):
    """Items for drawn frames: plain ones (a NaN end projects to 0 and a thick line from there to the screen would cover it all)."""
    return random_items(rng, n, camera, **kw)


def cpu_world(px, zb, w, h, items, camera, ortho=None):
    """What a world entry does to the frame on the CPU: np_world's records through np_prims.  Returns the counts."""
    recs, counts = np_world(items, camera, ortho, w, h)
    np_prims(px, zb, w, h, recs)
    return counts


def _counts_delta(fb, before):
    return tuple(a - b for a, b in zip(fb.world_counts(), before))


def _same_z(fb, zb):
    assert np.array_equal(fb.zbuffer.view(np.uint32), np.asarray(zb, f32).view(np.uint32)), "the z-buffer changed"


def _game_scene(name="dungeon-room0-game.b32scene"):
    from bonnie32_amd import scenefile
    return scenefile.read_scene(os.path.join(ROOT, "tests", "golden", "scenes", "real", name))


@pytest.mark.gpu
def test_gpu_world_stage_tap(gpu_ctx):
    """b32_world_project_batch == ref_world / np_world byte for byte on the 20 000 items at 320x240 and 2560x1920, perspective and ortho;
    the counts move by the model's counts."""
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(64, 64, gpu_ctx)
    for k, (cam, I) in enumerate(the_20000()):
        for w, h in SIZES:
            for ortho in (None, ORTHO):
                want, wc = np_world(I, cam, ortho, w, h)
                lit, lc = ref_world(I, cam, ortho, w, h)
                c0 = fb.world_counts()
                got = fb.world_project_batch(I, cam, ortho, w, h)
                assert got.tobytes() == want.tobytes(), f"batch {k} {w}x{h} ortho={ortho}: records {np.nonzero(got != want)[0][:8]} differ"
                assert got.tobytes() == lit.tobytes() and lc == wc
                assert _counts_delta(fb, c0) == wc
    G = grid_items()
    for cam in GRID_CAMS:
        for w, h in SIZES:
            want, wc = ref_world(G, cam, None, w, h)
            c0 = fb.world_counts()
            assert fb.world_project_batch(G, cam, None, w, h).tobytes() == want.tobytes()
            assert _counts_delta(fb, c0) == wc and wc[2] == 0
    assert len(fb.world_project_batch(G[:0], CENSUS_CAM)) == 0


def modeler_world_overlay(sc):
    """The modeler's frame over the mesh from the scene's own vertices, as one world batch: clipped hierarchy lines (vertex to vertex
    across the mesh, as bone lines run), LINE_3D box brackets around the bounds, LINE_3D_ALPHA 191 edges, a CIRCLE_ALPHA r=3 alpha 140 dot
    per vertex."""
    from bonnie32_amd import rasterizer as R
    pos = sc.vertices["pos"].astype(f32)
    b = R.WorldBatch(None)
    bone_c, box_c, edge_c, dot_c = b32.Color(255, 255, 255), b32.Color(255, 160, 0), b32.Color(255, 200, 60), b32.Color(80, 220, 255)
    step = max(1, len(pos) // 40)
    chain = pos[::step]
    for a_, b_ in zip(chain[:-1], chain[1:]):
        b.line_clipped(a_, b_, bone_c)
    lo, hi = pos.min(0), pos.max(0)
    corners = [np.array([x, y, z], f32) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]
    for i in range(8):
        for ax in range(3):
            j = i ^ (4 >> ax)
            if j > i:
                b.line_3d(corners[i], corners[j], box_c)
    edges = set()
    for f in sc.faces["v"]:
        for a_, b_ in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            edges.add((int(min(a_, b_)), int(max(a_, b_))))
    for a_, b_ in sorted(edges):
        b.line_3d_alpha(pos[a_], pos[b_], edge_c, 191)
    for p in pos:
        b.circle_alpha(p, 3, dot_c, 140)
    return b.items()


@pytest.mark.gpu
def test_gpu_world_modeler_frame(gpu_ctx, oracle):
    """clear, draw_floor_grid, a real golden scene with a valid z-buffer, one world batch of overlays -- against the same frame composed
    on the CPU.  The grid and the overlay each change pixels; no world call changes the z-buffer; nothing is rejected."""
    from bonnie32_amd import rasterizer as R
    sc = _game_scene()
    W, H = sc.width, sc.height
    assert sc.settings.use_zbuffer
    ofb = oracle.Framebuffer(W, H)
    ofb.clear(sc.clear_color)
    cleared = ofb.pixels.copy()
    gc = cpu_world(ofb.pixels, None, W, H, grid_items(), sc.camera)
    assert gc[0] > 0 and gc[2] == 0 and not np.array_equal(ofb.pixels, cleared)
    assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)[0] == 0
    meshes = ofb.pixels.copy()
    I = modeler_world_overlay(sc)
    assert (I["kind"] == abi.LINE_3D_ALPHA).sum() > 500 and (I["kind"] == abi.PRIM_CIRCLE_ALPHA).sum() > 500 and (I["flags"] == 1).sum() >= 30
    want = meshes.copy()
    oc = cpu_world(want, ofb.zbuffer, W, H, I, sc.camera)
    assert not np.array_equal(want, meshes) and oc[0] > 500

    fb = R.Framebuffer(W, H, gpu_ctx)
    c0 = fb.world_counts()
    r0 = gpu_ctx.route_counts()
    fb.clear(sc.clear_color)
    fb.draw_floor_grid(sc.camera, 0.0, 1024.0, 10240.0, *GRID_COLORS)
    R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
    assert np.array_equal(fb.pixels, meshes)
    fb.draw_world(I, sc.camera)
    got = fb.pixels
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    _same_z(fb, ofb.zbuffer)
    assert _counts_delta(fb, c0) == tuple(a + b_ for a, b_ in zip(gc, oc))
    r1 = gpu_ctx.route_counts()
    assert r1["world_tiles"] == r0["world_tiles"] + 2 and r1["prim_tiles"] == r0["prim_tiles"] + 2
    # the same overlay one call per method through the Python mirror's single-item entry
    fb.upload(meshes)
    for it in I[:: max(1, len(I) // 60)]:
        fb.draw_world(np.atleast_1d(it), sc.camera)
    sub = meshes.copy()
    cpu_world(sub, ofb.zbuffer, W, H, I[:: max(1, len(I) // 60)], sc.camera)
    assert np.array_equal(fb.pixels, sub)
    fb.upload(meshes)
    fb.draw_3d_line_clipped(sc.camera, I[0]["p0"], I[0]["p1"], b32.Color(255, 255, 255))
    one = meshes.copy(); cpu_world(one, ofb.zbuffer, W, H, I[:1], sc.camera)
    assert np.array_equal(fb.pixels, one)


@pytest.mark.gpu
def test_gpu_world_floor_grid_three_cameras(gpu_ctx):
    """The floor grid alone from three cameras at both sizes: lines whose ends lie millions of pixels off screen, all inside the 2^30
    rule (rejected == 0); every camera reaches the clipped-and-drawn and the clipped-and-vanished branch."""
    from bonnie32_amd import rasterizer as R
    G = grid_items()
    for w, h in SIZES:
        fb = R.Framebuffer(w, h, gpu_ctx)
        for cam in GRID_CAMS:
            fb.clear(b32.Color(5, 10, 20))
            base = fb.pixels
            want = base.copy()
            wc = cpu_world(want, None, w, h, G, cam)
            c0 = fb.world_counts()
            fb.draw_floor_grid(cam, 0.0, 1024.0, 10240.0, *GRID_COLORS)
            got = fb.pixels
            assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
            assert not np.array_equal(got, base)
            assert _counts_delta(fb, c0) == wc and wc[2] == 0
            cen = census(G, cam, w, h)
            assert cen[2] > 0 and cen[3] > 0 and wc == (cen[1] + cen[2], cen[0] + cen[3], 0)
    recs, _ = np_world(G, CENSUS_CAM, None, 2560, 1920)
    assert max(np.abs(recs[f].astype(np.int64)).max() for f in ("x0", "y0", "x1", "y1")) > 1_000_000       # far off screen


@pytest.mark.gpu
def test_gpu_world_ortho_view(gpu_ctx):
    """An orthographic view with dots and depth lines over an uploaded z-buffer; the clipped lines in the batch ignore the ortho."""
    from bonnie32_amd import rasterizer as R
    W, H = 640, 480
    rng = np.random.default_rng(61)
    fb = R.Framebuffer(W, H, gpu_ctx)
    cam = look_at((0, 300, -2000), (0, 0, 0))
    ortho = (0.2, 50.0, -30.0)
    I = _frame_items(rng, 1500, cam, kinds=DEPTH_KINDS + CIRCLE_KINDS + (abi.LINE_2D,), depth=(-200.0, 4000.0), seg=400.0, clip_p=0.2)
    zb = rng.uniform(0.0, 4000.0, W * H).astype(f32)
    for items in (I, I[:40]):
        fb.clear(b32.Color(30, 30, 30))
        _upload_zbuffer(fb, zb)
        base = fb.pixels
        want = base.copy()
        wc = cpu_world(want, zb, W, H, items, cam, ortho)
        c0 = fb.world_counts()
        fb.draw_world(items, cam, ortho)
        got = fb.pixels
        assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
        assert not np.array_equal(got, base) and _counts_delta(fb, c0) == wc
        _same_z(fb, zb)
        persp = base.copy(); cpu_world(persp, zb, W, H, items, cam, None)
        assert not np.array_equal(persp, want)                     # (the ortho matters)


@pytest.mark.gpu
def test_gpu_world_order(gpu_ctx):
    """Overlapping opaque and alpha items whose result depends on the array order, a dropped item between them: both orders, small and
    copied batches."""
    from bonnie32_amd import rasterizer as R
    W, H = 320, 240
    fb = R.Framebuffer(W, H, gpu_ctx)
    rng = np.random.default_rng(62)
    for n in (40, 600):
        I = _frame_items(rng, n, IDENTITY_CAM, kinds=(abi.LINE_2D, abi.LINE_2D_ALPHA, abi.PRIM_CIRCLE, abi.PRIM_CIRCLE_ALPHA, abi.PRIM_LINE_BLENDED,
                                                      abi.PRIM_THICK_LINE), spread=(12.0, 9.0), depth=(40.0, 60.0), seg=8.0)
        I["mode"] = rng.integers(1, 5, n)
        I[1::7]["p0"][:, 2] = -50.0; I[1::7]["p1"][:, 2] = -80.0          # behind the camera: dropped, in place
        results = []
        for items in (I, I[::-1].copy()):
            fb.clear(b32.Color(12, 200, 90))
            base = fb.pixels
            want = base.copy()
            wc = cpu_world(want, None, W, H, items, IDENTITY_CAM)
            assert wc[1] >= n // 7 and wc[0] > n // 2
            c0 = fb.world_counts()
            fb.draw_world(items, IDENTITY_CAM)
            got = fb.pixels
            assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
            assert _counts_delta(fb, c0) == wc
            results.append(got)
        assert not np.array_equal(results[0], results[1])


@pytest.mark.gpu
def test_gpu_world_sizes_and_routes(oracle):
    """n = 1, 48, 49 and 100 000 over a rendered z-buffer frame at 2560x1920: the scan form up to 48, the tile route from 49, and the scan
    again with the route switched off -- each asserts the counters it moved (world batches count as primitive batches too)."""
    from bonnie32_amd import rasterizer as R, scenegen
    sc = scenegen.make_scene("C3", n_tris=100_000)
    sc.settings.use_zbuffer = True
    W, H = sc.width, sc.height
    ofb = oracle.Framebuffer(W, H)
    ofb.clear(sc.clear_color)
    assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)[0] == 0
    rng = np.random.default_rng(63)
    zs = ofb.zbuffer[ofb.zbuffer < 1e30]
    zmax = float(zs.max()) if len(zs) else 3000.0
    big = _frame_items(rng, 100_000, sc.camera, spread=(zmax, zmax * 0.75), depth=(-0.2 * zmax, 1.5 * zmax), seg=zmax * 0.03)
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        fb.clear(sc.clear_color)
        R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
        assert np.array_equal(fb.pixels, ofb.pixels)
        first_drawn = big[np.nonzero(np_world(big, sc.camera, None, W, H)[0]["size"] != -1)[0][:1]]
        expect = {}
        for n in (1, 48, 49, 100_000):
            items = big[:n] if n > 1 else first_drawn
            want = ofb.pixels.copy()
            expect[n] = (items, want, cpu_world(want, ofb.zbuffer, W, H, items, sc.camera))
        for routes in (0, R.Context.ROUTE_PRIM_TILES):
            ctx.set_routes(routes)
            for n in (1, 48, 49, 100_000):
                items, want, wc = expect[n]
                fb.upload(ofb.pixels)
                r0, c0 = ctx.route_counts(), fb.world_counts()
                fb.draw_world(items, sc.camera)
                got = fb.pixels
                assert np.array_equal(got, want), f"n={n} routes={routes}: {int((got != want).sum())} bytes differ"
                assert n < 48 or not np.array_equal(got, ofb.pixels), n
                _same_z(fb, ofb.zbuffer)
                assert _counts_delta(fb, c0) == wc
                r1 = ctx.route_counts()
                tiles = n > 48 and routes == 0
                moved = {k: r1[k] - r0[k] for k in ("world_tiles", "world_scan", "prim_tiles", "prim_scan", "line_tiles", "line_scan")}
                assert moved == {"world_tiles": int(tiles), "world_scan": int(not tiles), "prim_tiles": int(tiles), "prim_scan": int(not tiles),
                                 "line_tiles": 0, "line_scan": 0}, (n, routes, moved)
        ctx.set_routes(0)
        fb.draw_world(big[:0], sc.camera)                                 # n == 0: a no-op
        assert ctx.route_counts() == r1
        # b32_draw_prims behind a world batch reuses the device record buffer the world batch wrote: still exact
        recs = np_world(big[:5000], sc.camera, None, W, H)[0]
        fb.upload(ofb.pixels)
        fb.draw_world(big[5000:9000], sc.camera); fb.draw_prims(recs); fb.draw_world(big[9000:9040], sc.camera)
        want = ofb.pixels.copy()
        cpu_world(want, ofb.zbuffer, W, H, big[5000:9000], sc.camera); np_prims(want, ofb.zbuffer, W, H, recs)
        cpu_world(want, ofb.zbuffer, W, H, big[9000:9040], sc.camera)
        assert np.array_equal(fb.pixels, want)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_world_band(gpu_ctx):
    """With a band set only its rows change; the bands of a frame add up to the frame."""
    from bonnie32_amd import rasterizer as R
    W, H = 640, 480
    fb = R.Framebuffer(W, H, gpu_ctx)
    rng = np.random.default_rng(64)
    zb = rng.uniform(0.0, 3000.0, W * H).astype(f32)
    cam = GRID_CAMS[2]
    try:
        for n in (40, 3000):
            I = _frame_items(rng, n, cam, seg=300.0)
            fb.set_band(0, H)
            fb.clear(b32.Color(9, 9, 9))
            _upload_zbuffer(fb, zb)
            base = fb.pixels
            want = base.copy(); cpu_world(want, zb, W, H, I, cam)
            assert not np.array_equal(want, base)
            for band in ((0, 100), (100, 333), (333, 334), (334, H)):
                fb.set_band(*band)
                fb.draw_world(I, cam)
            fb.set_band(0, H)
            assert np.array_equal(fb.pixels, want)
            fb.upload(base)
            fb.set_band(100, 333)
            fb.draw_world(I, cam)
            fb.draw_floor_grid(cam, 0.0, 1024.0, 10240.0, *GRID_COLORS)
            fb.set_band(0, H)
            full = want.copy(); cpu_world(full, zb, W, H, grid_items(), cam)
            part = base.reshape(H, -1).copy(); part[100:333] = full.reshape(H, -1)[100:333]
            assert np.array_equal(fb.pixels, part.reshape(-1))
            fb.set_band(200, 200)                                         # an empty band: nothing
            fb.draw_world(I, cam)
            fb.set_band(0, H)
            assert np.array_equal(fb.pixels, part.reshape(-1))
    finally:
        fb.set_band(0, H)


@pytest.mark.gpu
def test_gpu_world_pipeline(oracle):
    """Two frames in flight: grid, b32_frame_submit, world batches (small and copied, the caller's array overwritten at once),
    b32_fb_download_async -- every delivered frame equals the synchronous composition."""
    from bonnie32_amd import rasterizer as R, scenegen
    rng = np.random.default_rng(65)
    ctx = R.Context(0)
    try:
        st = b32.RasterSettings.game()
        meshes = [scenegen.make_scene("C1", n_tris=800, seed=300 + i, variant="gouraud") for i in range(3)]
        W, H = meshes[0].width, meshes[0].height
        cam = meshes[0].camera
        fb = R.Framebuffer(W, H, ctx)
        slots = [R.ResidentScene(fb, m.vertices, m.faces, m.textures).detach() for m in meshes]
        table = ctx.make_frame_table(cam, st, slots)
        bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
        frames = [(_frame_items(rng, 36, cam), _frame_items(rng, 700, cam)) for _ in range(4)]
        want = []
        for small, large in frames:
            o = oracle.Framebuffer(W, H); o.clear(b32.Color(10, 10, 30))
            cpu_world(o.pixels, None, W, H, grid_items(-3.0, 4.0, 40.0), cam)
            for m in meshes:
                assert oracle.render_mesh_15(o, m.vertices, m.faces, m.textures, cam, st)[0] == 0
            px = o.pixels.copy()
            cpu_world(px, o.zbuffer, W, H, small, cam); cpu_world(px, o.zbuffer, W, H, large, cam)
            assert not np.array_equal(px, o.pixels)
            want.append(px)
        assert not np.array_equal(want[0], want[1])
        tickets = []
        for i, (small, large) in enumerate(frames):
            fb.clear(b32.Color(10, 10, 30))
            fb.draw_floor_grid(cam, -3.0, 4.0, 40.0, *GRID_COLORS)
            ctx.frame_submit(table)
            for items in (small, large):
                arr = items.copy()
                fb.draw_world(arr, cam)
                arr[:] = _frame_items(rng, len(arr), cam)                 # the caller reuses its array at once
            tickets.append(ctx.download_async(bufs[i & 1][1]))
            if i >= 1:
                ctx.ticket_wait(tickets[i - 1])
                assert np.array_equal(bufs[(i - 1) & 1][0], want[i - 1]), f"frame {i - 1}"
        ctx.ticket_wait(tickets[-1])
        assert np.array_equal(bufs[(len(frames) - 1) & 1][0], want[-1])
        ctx.finish()
        for _, p in bufs:
            ctx.host_free(p)
        for s in slots:
            s.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_world_rejection(gpu_ctx):
    """An item built to project beyond 2^30 draws nothing and is counted as rejected; its neighbours are drawn (small and copied)."""
    from bonnie32_amd import rasterizer as R
    W, H = 320, 240
    fb = R.Framebuffer(W, H, gpu_ctx)
    rng = np.random.default_rng(66)
    c = b32.Color(250, 250, 0)
    far_line = R.world_item(abi.LINE_2D, (0, 0, 50), (3e9, 0, 0.2), c)            # x1 saturates at i32::MAX: extent >= 2^30
    far_dot = R.world_item(abi.PRIM_CIRCLE, (-3e9, 0, 0.2), (0, 0, 0), c, size=4)
    for n in (20, 400):
        I = _frame_items(rng, n, IDENTITY_CAM, spread=(12.0, 9.0), depth=(40.0, 60.0), seg=8.0, clip_p=0.0)
        for bad in (far_line, far_dot):
            items = np.concatenate([I[:n // 2], bad, I[n // 2:]])
            fb.clear(b32.Color(1, 2, 3))
            base = fb.pixels
            want = base.copy()
            wc = cpu_world(want, None, W, H, items, IDENTITY_CAM)
            assert wc == (n, 0, 1)
            plain = base.copy(); cpu_world(plain, None, W, H, I, IDENTITY_CAM)
            assert np.array_equal(plain, want)                        # the model: exactly the neighbours
            c0 = fb.world_counts()
            fb.draw_world(items, IDENTITY_CAM)
            assert np.array_equal(fb.pixels, want)
            assert _counts_delta(fb, c0) == (n, 0, 1)


@pytest.mark.gpu
def test_gpu_world_argument_errors(gpu_ctx):
    """Kinds 9 / 10 / unknown, an unknown flag, the clip flag on a circle, a bad mode: B32_E_ARG; a circle radius beyond 32767:
    B32_E_UNSUPPORTED; floor grids the reference would never finish: B32_E_ARG -- and the frame and the counts untouched."""
    from bonnie32_amd import rasterizer as R
    W, H = 200, 150
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(b32.Color(1, 2, 3))
    rng = np.random.default_rng(67)
    base = fb.pixels
    good = _frame_items(rng, 30, IDENTITY_CAM, spread=(12.0, 9.0), depth=(40.0, 60.0), seg=8.0)
    good["kind"][15] = abi.LINE_2D
    c0 = fb.world_counts()
    cases = [({"kind": abi.PRIM_RECT}, abi.B32_E_ARG), ({"kind": abi.PRIM_FILLED_RECT}, abi.B32_E_ARG), ({"kind": 11}, abi.B32_E_ARG),
             ({"kind": 255}, abi.B32_E_ARG), ({"flags": 2}, abi.B32_E_ARG), ({"flags": 3}, abi.B32_E_ARG), ({"flags": 128}, abi.B32_E_ARG),
             ({"kind": abi.PRIM_CIRCLE, "flags": 1}, abi.B32_E_ARG), ({"kind": abi.PRIM_CIRCLE_ALPHA, "flags": 1}, abi.B32_E_ARG),
             ({"kind": abi.PRIM_LINE_BLENDED, "mode": 6}, abi.B32_E_ARG),
             ({"kind": abi.PRIM_CIRCLE, "flags": 0, "size": 32768}, abi.B32_E_UNSUPPORTED), ({"kind": abi.PRIM_CIRCLE_ALPHA, "flags": 0, "size": -32768}, abi.B32_E_UNSUPPORTED)]
    for n in (30, 300):
        batch = np.concatenate([good] * (n // 30))
        for fields, code in cases:
            bad = batch.copy()
            for f, v in fields.items():
                bad[f][n // 2] = v
            for call in (lambda: fb.draw_world(bad, IDENTITY_CAM), lambda: fb.world_project_batch(bad, IDENTITY_CAM)):
                with pytest.raises(R.B32Error) as e:
                    call()
                assert e.value.code == code, fields
    for bad in ((0, 0.0, 10), (0, -1.0, 10), (float("nan"), 1, 10), (0, float("inf"), 10), (0, 1, float("inf")), (0, 1e-3, 1e6)):
        with pytest.raises(R.B32Error) as e:
            fb.draw_floor_grid(IDENTITY_CAM, *bad, *GRID_COLORS)
        assert e.value.code == abi.B32_E_ARG, bad
    with pytest.raises(R.B32Error) as e:
        fb.draw_floor_grid(IDENTITY_CAM, 0, 1.0, 1000.0, *GRID_COLORS)
    assert e.value.code == abi.B32_E_UNSUPPORTED
    lib = gpu_ctx.lib
    cam = IDENTITY_CAM.pack()
    import ctypes as C
    assert lib.b32_draw_world(gpu_ctx.h, None, None, good.ctypes.data, len(good)) == abi.B32_E_ARG
    assert lib.b32_draw_world(gpu_ctx.h, C.byref(cam), None, None, 5) == abi.B32_E_ARG
    assert lib.b32_draw_world(None, C.byref(cam), None, good.ctypes.data, len(good)) == abi.B32_E_ARG
    assert lib.b32_world_counts(gpu_ctx.h, None, None, None) == abi.B32_E_ARG
    ok = good.copy()                                                  # accepted: radius +-32767 (off screen), mode 5, every kind 0..8
    ok["kind"][:9] = np.arange(9); ok["flags"][:9] = 0; ok["mode"][:9] = 5
    ok["size"][6] = 32767; ok["size"][7] = -32767; ok["p0"][6] = (1e6, 1e6, 50)
    fb.world_project_batch(ok, IDENTITY_CAM)
    fb.draw_world(good[:0], IDENTITY_CAM)
    assert np.array_equal(fb.pixels, base)
    assert fb.world_counts()[0] - c0[0] <= len(ok) and sum(_counts_delta(fb, c0)) == len(ok)      # only the accepted tap batch was projected
