"""The world editor's overlay helpers through b32_draw_gizmos (editor/viewport_3d.rs:5687-6357, modeler/viewport.rs:4575-4722).

Neither the oracle nor anything else in the repository draws these, so the expectation is built here:
  `ref_gizmos`  a literal scalar restatement of draw_3d_line / draw_3d_line_depth / draw_3d_thick_line_depth / draw_3d_point,
                clip_line_to_rect, both project_vertex forms and the triangle's sort, every operand an np.float32, returning the
                abi.PRIM_DTYPE records the device hands to the tile pass (a circle of radius -1 where the reference draws nothing) and
                the counts (drawn, dropped, rejected);
  `ref_tri_spans` / `np_tri`  draw_filled_triangle_3d's rows, literally and vectorised over the rows.
ref_gizmos is pinned by hand-computed cases; csrc/b32_gizmo_body.h -- the device code -- is compiled for the host and compared with it
bit for bit, with and without FMA contraction.  Every GPU frame is compared byte for byte with a frame composed on the CPU in the same
order: tests.test_prims.np_prims draws the line and circle records, np_tri the triangles."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi
from tests.test_lines import ROOT, _upload_zbuffer
from tests.test_prims import _as_i32, np_prims
from tests.test_world import (CENSUS_CAM, IDENTITY_CAM, QNAN, _cam_f32, _dot, _game_scene, _same_z, _sub, look_at, noop_records, ref_clip,
                              ref_world, ref_world_to_screen, ref_world_to_screen_with_ortho)

f32 = np.float32
LIM = 1 << 30
SIZES = ((320, 240), (203, 117))
ORTHO = (0.05, 120.0, -40.0)
TRI = abi.PRIM_TRIANGLE_INTERNAL
K_LINE, K_LINE_DEPTH, K_THICK, K_POINT, K_TRI, K_TRI_VIEW = range(6)
LINE_KINDS = (K_LINE, K_LINE_DEPTH, K_THICK)


# ---------------------------------------------------------------- literal restatement
def ref_clip_line_to_rect(x0, y0, x1, y1, xmin, ymin, xmax, ymax):
    """clip_line_to_rect, viewport_3d.rs:5886-5955: None, or (x0, y0, x1, y1, rounds taken)."""
    INSIDE, LEFT, RIGHT, BOTTOM, TOP = 0, 1, 2, 4, 8
    one = f32(1.0)

    def outcode(x, y):
        code = INSIDE
        if x < xmin:
            code |= LEFT
        elif x >= xmax:
            code |= RIGHT
        if y < ymin:
            code |= TOP
        elif y >= ymax:
            code |= BOTTOM
        return code

    code0 = outcode(x0, y0)
    code1 = outcode(x1, y1)
    for rounds in range(16):
        if (code0 | code1) == 0:
            return x0, y0, x1, y1, rounds
        if (code0 & code1) != 0:
            return None
        code_out = code0 if code0 != 0 else code1
        if code_out & BOTTOM:
            x = x0 + (x1 - x0) * (ymax - one - y0) / (y1 - y0)
            y = ymax - one
        elif code_out & TOP:
            x = x0 + (x1 - x0) * (ymin - y0) / (y1 - y0)
            y = ymin
        elif code_out & RIGHT:
            y = y0 + (y1 - y0) * (xmax - one - x0) / (x1 - x0)
            x = xmax - one
        else:
            y = y0 + (y1 - y0) * (xmin - x0) / (x1 - x0)
            x = xmin
        if code_out == code0:
            x0, y0 = x, y
            code0 = outcode(x0, y0)
        else:
            x1, y1 = x, y
            code1 = outcode(x1, y1)
    return None


def ref_thick_offsets(x0, y0, x1, y1, thickness):
    """draw_3d_thick_line_depth's offsets, viewport_3d.rs:5763-5778: None (len < 0.001) or [(ox, oy)] for i in 0..thickness."""
    dx = f32(x1 - x0)
    dy = f32(y1 - y0)
    length = np.sqrt(dx * dx + dy * dy)
    if length < f32(0.001):
        return None
    half = f32(thickness) * f32(0.5)
    px = -dy / length * half
    py = dx / length * half
    out = []
    for i in range(thickness):
        offset = f32(i) - half + f32(0.5)
        out.append((_as_i32(px * offset / half), _as_i32(py * offset / half)))
    return out


def ref_project_vertex(p, cam, w, h):
    """The editor's project_vertex, viewport_3d.rs:6239-6245: perspective_transform (math.rs:103-109), cam.z < 0.1 -> None, project
    (math.rs:117-136), `as i32`."""
    pos, bx, by, bz = cam
    rel = _sub(p, pos)
    cx, cy, cz = _dot(rel, bx), _dot(rel, by), _dot(rel, bz)
    if cz < f32(0.1):
        return None
    ud = f32(5.0)
    us = ud - f32(1.0)
    vs = (f32(min(w, h)) / f32(2.0)) * f32(0.75)
    denom = cz + ud
    if abs(denom) < f32(0.001):
        return _as_i32(f32(w) / f32(2.0)), _as_i32(f32(h) / f32(2.0))
    return _as_i32((cx * us) / denom * vs + (f32(w) / f32(2.0))), _as_i32((cy * us) / denom * vs + (f32(h) / f32(2.0)))


def ref_project_vertex_view(p, cam, w, h, ortho):
    """The modeler's project_vertex, modeler/viewport.rs:4592-4607."""
    s = ref_world_to_screen_with_ortho(p, cam, w, h, ortho)
    return None if s is None else (_as_i32(s[0]), _as_i32(s[1]))


def ref_tri_sorted(p0, p1, p2):
    """pts.sort_by(|a, b| a.1.cmp(&b.1)): stable, as Python's sort."""
    return sorted([p0, p1, p2], key=lambda p: p[1])


def ref_tri_spans(p0, p1, p2, w, h):
    """draw_filled_triangle_3d, viewport_3d.rs:6302-6345: [(y, x_start, x_end)] of the rows that are not skipped."""
    (x0, y0), (x1, y1), (x2, y2) = ref_tri_sorted(p0, p1, p2)
    if y2 == y0:
        return []
    total_height = f32(y2 - y0)
    out = []
    for y in range(max(y0, 0), min(y2, h - 1) + 1):
        second_half = y > y1 or y1 == y0
        segment_height = f32(y2 - y1) if second_half else f32(y1 - y0)
        if segment_height == f32(0.0):
            continue
        alpha = f32(y - y0) / total_height
        beta = f32(y - y1) / segment_height if second_half else f32(y - y0) / segment_height
        ax = f32(x0) + f32(x2 - x0) * alpha
        bx = f32(x1) + f32(x2 - x1) * beta if second_half else f32(x0) + f32(x1 - x0) * beta
        if ax > bx:
            ax, bx = bx, ax
        out.append((y, max(_as_i32(ax), 0), min(_as_i32(bx), w - 1)))
    return out


def _i32v(v):
    x = np.asarray(v, f32).astype(np.float64)
    return np.trunc(np.clip(np.where(np.isnan(x), 0.0, x), -2147483648.0, 2147483647.0)).astype(np.int64)


def np_tri_spans(p0, p1, p2, w, h):
    """ref_tri_spans vectorised over the rows: arrays (y, x_start, x_end)."""
    (x0, y0), (x1, y1), (x2, y2) = ref_tri_sorted(p0, p1, p2)
    e = np.zeros(0, np.int64)
    if y2 == y0:
        return e, e, e
    y = np.arange(max(y0, 0), min(y2, h - 1) + 1, dtype=np.int64)
    second = (y > y1) | (y1 == y0)
    seg = np.where(second, f32(y2 - y1), f32(y1 - y0)).astype(f32)
    with np.errstate(all="ignore"):
        alpha = (y - y0).astype(f32) / f32(y2 - y0)
        beta = np.where(second, (y - y1).astype(f32) / seg, (y - y0).astype(f32) / seg).astype(f32)
        ax = f32(x0) + f32(x2 - x0) * alpha
        bx = np.where(second, f32(x1) + f32(x2 - x1) * beta, f32(x0) + f32(x1 - x0) * beta).astype(f32)
    lo, hi = np.where(ax > bx, bx, ax), np.where(ax > bx, ax, bx)
    keep = seg != f32(0.0)
    return y[keep], np.maximum(_i32v(lo), 0)[keep], np.minimum(_i32v(hi), w - 1)[keep]


def np_tri(img, w, h, p0, p1, p2, rgb):
    """draw_filled_triangle_3d on img (the frame as [w * h, 4] bytes, modified): [r, g, b, 255] on every span, no depth test."""
    im = img.reshape(h, w, 4)
    for y, xs, xe in zip(*np_tri_spans(p0, p1, p2, w, h)):
        if xs <= xe:
            im[y, xs:xe + 1] = (rgb[0], rgb[1], rgb[2], 255)


def tri_points(rec):
    """The three points of a triangle record, in argument order (the third travels as the bit patterns of z0 and z1)."""
    r = np.atleast_1d(rec)
    x2, y2 = int(r["z0"].view(np.int32)[0]), int(r["z1"].view(np.int32)[0])
    return (int(r["x0"][0]), int(r["y0"][0])), (int(r["x1"][0]), int(r["y1"][0])), (x2, y2)


def ref_gizmos(items, camera, ortho, w, h):
    """(records, (drawn, dropped, rejected)) of `items` (abi.GIZMO_ITEM_DTYPE), one reference call after another."""
    from bonnie32_amd.rasterizer import gizmo_record_count
    cam = _cam_f32(camera)
    items = np.ascontiguousarray(items, abi.GIZMO_ITEM_DTYPE).reshape(-1)
    firsts = np.concatenate([[0], np.cumsum([gizmo_record_count(int(k), int(s)) for k, s in zip(items["kind"], items["size"])])]).astype(np.int64)
    out = noop_records(int(firsts[-1]))
    zi = {f: out[f].view(np.int32) for f in ("z0", "z1")}
    counts = [0, 0, 0]
    big = lambda v: abs(v) >= LIM

    def colour(r, it, kind):
        for f in ("r", "g", "b", "blend"):
            r[f] = it[f]
        r["kind"] = kind; r["size"] = 0

    def one(i, it):
        kind, size, at = int(it["kind"]), int(it["size"]), int(firsts[i])
        p = [tuple(f32(v) for v in it[n]) for n in ("p0", "p1", "p2")]
        if kind in LINE_KINDS:
            cl = ref_clip(p[0], p[1], cam)                      # viewport_3d.rs:5794-5816 == draw.rs:19-42
            if cl is None:
                return 1
            ends = [ref_world_to_screen(q, cam, w, h) for q in cl]
            if any(e is None for e in ends):
                return 1
            (sx0, sy0, d0), (sx1, sy1, d1) = ends
            if kind == K_LINE:
                c = ref_clip_line_to_rect(sx0, sy0, sx1, sy1, f32(0.0), f32(0.0), f32(w), f32(h))
                if c is None:
                    return 1
                x0, y0, x1, y1 = (_as_i32(v) for v in c[:4])
                if big(x1 - x0) or big(y1 - y0):
                    return 2
                r = out[at]
                colour(r, it, abi.LINE_2D)
                r["x0"], r["y0"], r["x1"], r["y1"] = x0, y0, x1, y1
                return 0
            x0, y0, x1, y1 = _as_i32(sx0), _as_i32(sy0), _as_i32(sx1), _as_i32(sy1)
            if big(x1 - x0) or big(y1 - y0):
                return 2
            z0, z1 = (QNAN if np.isnan(d) else d for d in (d0, d1))
            if kind == K_LINE_DEPTH or size <= 1:
                offs = [(0, 0)]
            else:
                if any(big(v) for v in (x0, y0, x1, y1)):
                    return 2
                offs = ref_thick_offsets(x0, y0, x1, y1, size)
                if offs is None:
                    return 1
            for k, (ox, oy) in enumerate(offs):
                r = out[at + k]
                colour(r, it, abi.LINE_3D_OVERLAY)
                r["x0"], r["y0"], r["x1"], r["y1"], r["z0"], r["z1"] = x0 + ox, y0 + oy, x1 + ox, y1 + oy, z0, z1
            return 0
        if kind == K_POINT:
            s = ref_world_to_screen(p[0], cam, w, h)
            if s is None:
                return 1
            x, y = _as_i32(s[0]), _as_i32(s[1])
            if big(x) or big(y):
                return 2
            r = out[at]
            colour(r, it, abi.PRIM_CIRCLE)
            r["x0"], r["y0"], r["size"] = x, y, size
            return 0
        pts = [ref_project_vertex(q, cam, w, h) if kind == K_TRI else ref_project_vertex_view(q, cam, w, h, ortho) for q in p]
        if any(q is None for q in pts):
            return 1
        if any(big(v) for q in pts for v in q):
            return 2
        if pts[0][1] == pts[1][1] == pts[2][1]:                # y2 == y0
            return 1
        r = out[at]
        colour(r, it, TRI)
        r["x0"], r["y0"], r["x1"], r["y1"] = pts[0][0], pts[0][1], pts[1][0], pts[1][1]
        zi["z0"][at], zi["z1"][at] = pts[2]
        return 0

    with np.errstate(all="ignore"):
        for i, it in enumerate(items):
            counts[one(i, it)] += 1
    return out, tuple(counts)


def cpu_records(px, zb, w, h, recs):
    """The records of a gizmo batch on the frame px (flat RGBA, modified), in order: np_prims for the runs of lines and circles, np_tri
    for the triangles."""
    recs = np.ascontiguousarray(recs, abi.PRIM_DTYPE).reshape(-1)
    tri = recs["kind"] == TRI
    i = 0
    while i < len(recs):
        j = i
        while j < len(recs) and tri[j] == tri[i]:
            j += 1
        if tri[i]:
            for r in recs[i:j]:
                np_tri(px.reshape(-1, 4), w, h, *tri_points(r), (int(r["r"]), int(r["g"]), int(r["b"])))
        else:
            np_prims(px, zb, w, h, recs[i:j])
        i = j


def cpu_gizmos(px, zb, w, h, items, camera, ortho=None):
    recs, counts = ref_gizmos(items, camera, ortho, w, h)
    cpu_records(px, zb, w, h, recs)
    return counts


# ---------------------------------------------------------------- batches
def cam_point(camera, cx, cy, cz):
    """The world position with these camera-space coordinates (f64, cast by the caller)."""
    pos, bx, by, bz = (np.array(v, np.float64) for v in (camera.position, camera.basis_x, camera.basis_y, camera.basis_z))
    return pos + cx * bx + cy * by + cz * bz


def G(kind, p0, p1=(0, 0, 0), p2=(0, 0, 0), rgb=(200, 60, 30), blend=abi.OPAQUE, size=0):
    from bonnie32_amd import rasterizer as R
    return R.gizmo_item(kind, p0, p1, p2, b32.Color(*rgb, blend), size)


def random_gizmos(rng, n, camera, kinds=range(6), spread=(1500.0, 1000.0), depth=(-400.0, 3000.0), seg=120.0, long_p=0.4, near_p=0.15, hostile=True):
    """Items around the camera's view, in the style of test_world.random_items: one end `depth` along basis_z (some behind), the others
    within `seg` of it -- or, for a share `long_p`, within 12 x seg, so that segments leave the frame --; a share `near_p` starts within
    seg / 2 of the camera's plane, so that segments cross the near plane; ties in y for some triangles
    (points displaced along basis_x only); with `hostile`, NaN / inf / huge coordinates, ends on the near plane and items whose
    projection passes 2^30."""
    pos, bx, by, bz = (np.array(v, np.float64) for v in (camera.position, camera.basis_x, camera.basis_y, camera.basis_z))
    I = np.zeros(n, abi.GIZMO_ITEM_DTYPE)
    d = np.where(rng.random((n, 1)) < near_p, rng.uniform(-0.5 * seg, 0.5 * seg, (n, 1)), rng.uniform(*depth, (n, 1)))
    a = pos + d * bz + rng.uniform(-spread[0], spread[0], (n, 1)) * bx + rng.uniform(-spread[1], spread[1], (n, 1)) * by
    reach = np.where(rng.random((n, 1)) < long_p, 12.0 * seg, seg)
    I["p0"] = a.astype(f32)
    I["p1"] = (a + rng.uniform(-1.0, 1.0, (n, 3)) * reach).astype(f32)
    I["p2"] = (a + rng.uniform(-1.0, 1.0, (n, 3)) * reach).astype(f32)
    I["kind"] = rng.choice(np.array(list(kinds), np.uint8), n)
    tri = I["kind"] >= K_TRI
    tie = rng.random(n)
    along = rng.uniform(-1.0, 1.0, (n, 1)) * reach * bx
    I["p1"] = np.where((tri & (tie < 0.12))[:, None], (a + along).astype(f32), I["p1"])                 # p0, p1 on one row
    I["p2"] = np.where((tri & (tie >= 0.08) & (tie < 0.2))[:, None], (I["p1"].astype(np.float64) - 0.7 * along).astype(f32), I["p2"])   # p1, p2 (0.08-0.12: all three)
    I["p2"] = np.where((tri & (tie >= 0.2) & (tie < 0.24))[:, None], I["p0"], I["p2"])                  # two points equal
    I["size"] = np.where(I["kind"] == K_POINT, rng.integers(-1, 9, n), rng.choice(np.array([-2, 0, 1, 2, 3, 3, 3, 5, 16], np.int32), n))
    I["r"], I["g"], I["b"] = (rng.integers(0, 256, n) for _ in range(3))
    I["blend"] = np.where(rng.random(n) < 0.15, abi.ERASE, abi.OPAQUE)
    if hostile:
        bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, 1e-40, 0.0, -0.0], f32)
        for end in ("p0", "p1", "p2"):
            m = rng.random((n, 3)) < 0.01
            I[end] = np.where(m, rng.choice(bad, (n, 3)), I[end])
        m = rng.random(n) < 0.03                                      # both ends the same point
        I["p1"] = np.where(m[:, None], I["p0"], I["p1"])
        near = cam_point(camera, 3e9, 0.0, 0.2).astype(f32)           # projects beyond i32: x saturates
        for k, i in enumerate(rng.choice(n, 12, replace=False)):
            I["kind"][i] = (K_LINE_DEPTH, K_THICK, K_TRI, K_TRI_VIEW, K_POINT, K_LINE)[k % 6]
            I["size"][i] = 3
            I["p0"][i] = cam_point(camera, 0.0, 0.0, 50.0).astype(f32); I["p1"][i] = near; I["p2"][i] = cam_point(camera, 5.0, 9.0, 60.0).astype(f32)
            if I["kind"][i] == K_POINT:
                I["p0"][i] = near
        half = cam_point(camera, 7e8, 0.0, 0.2).astype(f32), cam_point(camera, -7e8, 0.0, 0.2).astype(f32)      # |x| < 2^30 each, the extent beyond
        for i in rng.choice(n, 4, replace=False):
            I["kind"][i] = K_LINE_DEPTH; I["p0"][i], I["p1"][i] = half
    return I


@functools.lru_cache(maxsize=None)
def the_random_set():
    return random_gizmos(np.random.default_rng(7001), 4000, CENSUS_CAM)


def frame_gizmos(rng, n, camera, zmax, **kw):
    """Items for drawn frames over a scene whose depths reach zmax."""
    return random_gizmos(rng, n, camera, spread=(zmax * 0.6, zmax * 0.45), depth=(-0.1 * zmax, 1.2 * zmax), seg=zmax * 0.05, hostile=False, **kw)


# ---------------------------------------------------------------- the host build of the device header
# (g++ forms fused multiply-adds from -O2 on, and only where the target has them)
HOST_FLAGS = {"off": ["-O1", "-ffp-contract=off"], "fused": ["-O2", "-ffp-contract=fast", "-mfma"]}


@functools.lru_cache(maxsize=None)
def _host_dir():
    d = tempfile.mkdtemp(prefix="b32_gizmo_host_")
    atexit.register(shutil.rmtree, d, True)
    return d


@functools.lru_cache(maxsize=None)
def host_exe(mode):
    exe = os.path.join(_host_dir(), "gizmo_host_" + mode)
    subprocess.run(["g++", "-std=c++17"] + HOST_FLAGS[mode] + ["-I", os.path.join(ROOT, "bonnie-32_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "gizmo_host.cpp"),
                    "-o", exe], check=True)
    return exe


def host_gizmos(items, camera, ortho, w, h, mode="off"):
    """(records, counts, which, spans [n, 4]) from b32_gizmo_body.h compiled for the host."""
    items = np.ascontiguousarray(items, abi.GIZMO_ITEM_DTYPE).reshape(-1)
    d = _host_dir()
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.array([w, h, int(ortho is not None), len(items)], np.uint32).tobytes())
        fh.write(np.array([v for g in _cam_f32(camera) for v in g], f32).tobytes())
        fh.write(np.array(ortho if ortho is not None else (0, 0, 0), f32).tobytes())
        fh.write(items.tobytes())
    subprocess.run([host_exe(mode), fin, fout], check=True)
    blob = open(fout, "rb").read()
    n_rec, n_span = np.frombuffer(blob, np.uint32, 2)
    counts = tuple(int(v) for v in np.frombuffer(blob, np.uint64, 3, 8))
    o = 32
    which = np.frombuffer(blob, np.uint32, len(items), o); o += 4 * len(items)
    recs = np.frombuffer(blob, abi.PRIM_DTYPE, int(n_rec), o); o += 40 * int(n_rec)
    spans = np.frombuffer(blob, np.int32, 4 * int(n_span), o).reshape(-1, 4)
    return recs, counts, which, spans


def ref_spans_table(recs, w, h):
    """What gizmo_host prints behind the records: (record index, y, x_start, x_end) of every triangle record."""
    rows = []
    for i in np.nonzero(recs["kind"] == TRI)[0]:
        y, xs, xe = np_tri_spans(*tri_points(recs[i]), w, h)
        rows.append(np.stack([np.full(len(y), i), y, xs, xe], axis=1))
    return np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 4), np.int32)


# ================================================================== CPU
def test_gizmo_item_layout_matches_c():
    """B32GizmoItem compiled with gcc against the public header has the layout of abi.GIZMO_ITEM_DTYPE, and the kinds match."""
    fields = ("p0", "p1", "p2", "size", "r", "g", "b", "blend", "kind", "_pad")
    kinds = ("B32_GIZMO_LINE", "B32_GIZMO_LINE_DEPTH", "B32_GIZMO_THICK_LINE_DEPTH", "B32_GIZMO_POINT", "B32_GIZMO_TRIANGLE", "B32_GIZMO_TRIANGLE_VIEW",
             "B32_GIZMO_MAX_THICKNESS")
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void){ printf("%zu", sizeof(B32GizmoItem));'
            + "".join(f' printf(" %zu", offsetof(B32GizmoItem, {f}));' for f in fields)
            + "".join(f' printf(" %u", (unsigned){k});' for k in kinds) + ' printf("\\n"); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    dt = abi.GIZMO_ITEM_DTYPE
    assert got == [dt.itemsize] + [dt.fields[f][1] for f in fields] + [0, 1, 2, 3, 4, 5, abi.GIZMO_MAX_THICKNESS]
    assert (abi.GIZMO_LINE, abi.GIZMO_LINE_DEPTH, abi.GIZMO_THICK_LINE_DEPTH, abi.GIZMO_POINT, abi.GIZMO_TRIANGLE, abi.GIZMO_TRIANGLE_VIEW) == tuple(range(6))


def _screen(x, y, z=95.0, w=320, h=240):
    """For the identity camera at the origin: a world point that world_to_screen puts at (x, y) of a w x h frame exactly when the numbers
    are small integers: cam_x = (x - w/2) * (z + 5) / (4 * vs) with z + 5 = 100 and vs = 90 -> cam_x = (x - w/2) / 3.6 -- not exact in
    general, so the hand cases below use multiples of 9 pixels off the centre: cam_x = 2.5 per 9 pixels."""
    assert (w, h) == (320, 240) and z == 95.0 and (x - 160) % 9 == 0 and (y - 120) % 9 == 0
    return ((x - 160) // 9 * 2.5, (y - 120) // 9 * 2.5, z)


def _one(item, w=320, h=240, ortho=None, cam=IDENTITY_CAM):
    recs, counts = ref_gizmos(item, cam, ortho, w, h)
    return recs, counts


def test_ref_gizmos_line_hand_cases():
    """draw_3d_line by hand, identity camera, 320x240 (vs = 90, a point at z = 95 lands on 160 + 3.6 x, 120 + 3.6 y)."""
    F = f32
    # the projection helper itself: (2.5, -5, 95) -> (169, 102)
    assert ref_world_to_screen(tuple(F(v) for v in _screen(169, 102)), _cam_f32(IDENTITY_CAM), 320, 240)[:2] == (F(169.0), F(102.0))
    # wholly inside: the record of B32_LINE_2D + B32_WORLD_CLIP_NEAR
    from bonnie32_amd import rasterizer as R
    it = G(K_LINE, _screen(16, 30), _screen(304, 210), rgb=(1, 2, 3), blend=abi.ERASE)
    recs, counts = _one(it)
    wi = R.world_item(abi.LINE_2D, _screen(16, 30), _screen(304, 210), b32.Color(1, 2, 3, abi.ERASE), alpha=0, flags=abi.WORLD_CLIP_NEAR)
    assert recs.tobytes() == ref_world(wi, IDENTITY_CAM, None, 320, 240)[0].tobytes() and counts == (1, 0, 0)
    assert tuple(int(recs[0][f]) for f in ("x0", "y0", "x1", "y1", "kind")) == (16, 30, 304, 210, abi.LINE_2D)
    # leaving through the bottom-right corner region: (160, 120) -> (520, 300): slope 1/2.  Round 1 (BOTTOM first): y = 239,
    # x = 160 + 360 * 119 / 180 = 398; still RIGHT.  Round 2: x = 319, y = 120 + 119 * 159 / 238 = 199.5 -> the record ends at (319, 199).
    c = ref_clip_line_to_rect(F(160), F(120), F(520), F(300), F(0), F(0), F(320), F(240))
    assert c == (F(160), F(120), F(319), F(199.5), 2)
    recs, counts = _one(G(K_LINE, _screen(160, 120), _screen(520, 300)))
    assert tuple(int(recs[0][f]) for f in ("x0", "y0", "x1", "y1")) == (160, 120, 319, 199) and counts == (1, 0, 0)
    #   draw_3d_line_clipped + draw_line would walk from (160, 120) to (520, 300) instead: other pixels (the reason for this entry)
    wrec = ref_world(R.world_item(abi.LINE_2D, _screen(160, 120), _screen(520, 300), b32.Color(1, 2, 3), flags=abi.WORLD_CLIP_NEAR), IDENTITY_CAM, None, 320, 240)[0]
    a = np.zeros(320 * 240 * 4, np.uint8); b = a.copy()
    np_prims(a, None, 320, 240, recs); np_prims(b, None, 320, 240, wrec)
    assert not np.array_equal(a, b)
    # both ends outside, crossing the frame: (-20, 120) -> (340, 120), horizontal.  The first end is LEFT: y = 120 + 0 * ... = 120, x = 0;
    # then the second is RIGHT: x = 319.
    assert ref_clip_line_to_rect(F(-20), F(120), F(340), F(120), F(0), F(0), F(320), F(240)) == (F(0), F(120), F(319), F(120), 2)
    recs, counts = _one(G(K_LINE, _screen(-20, 120), _screen(340, 120)))
    assert tuple(int(recs[0][f]) for f in ("x0", "y0", "x1", "y1")) == (0, 120, 319, 120) and counts == (1, 0, 0)
    # both ends outside and rejected: both above the frame (TOP & TOP), and a diagonal that passes the corner outside --
    # (-20, 30) -> (70, -60): round 1 clips the first end (LEFT) to (0, 10); round 2 the second (TOP) to x = 0 + 70 * (0 - 10) / -70 = 10, y = 0:
    # that one is INSIDE, so it is drawn from (0, 10) to (10, 0); the rejected diagonal is (-20, 12) -> (16, -24): LEFT -> (0, -8): TOP & TOP.
    assert ref_clip_line_to_rect(F(16), F(-60), F(304), F(-6), F(0), F(0), F(320), F(240)) is None
    assert ref_clip_line_to_rect(F(-20), F(30), F(70), F(-60), F(0), F(0), F(320), F(240)) == (F(0), F(10), F(10), F(0), 2)
    assert ref_clip_line_to_rect(F(-20), F(12), F(16), F(-24), F(0), F(0), F(320), F(240)) is None
    recs, counts = _one(G(K_LINE, _screen(-20, 12), _screen(16, -24)))
    assert recs.tobytes() == noop_records(1).tobytes() and counts == (0, 1, 0)
    # x == 320.0 and y == 240.0 are outside (`>=`), 319.99 is inside and casts to 319
    assert ref_clip_line_to_rect(F(160), F(120), F(320), F(120), F(0), F(0), F(320), F(240)) == (F(160), F(120), F(319), F(120), 1)
    # a NaN end has outcode 0: the segment is "inside" at once and the NaN casts to 0 (a NaN x makes every camera coordinate of that end
    # NaN -- NaN * 0.0 is NaN --, so both its screen coordinates are)
    nan = F(np.nan)
    c = ref_clip_line_to_rect(nan, F(50), F(100), F(60), F(0), F(0), F(320), F(240))
    assert c[4] == 0 and np.isnan(c[0])
    recs, counts = _one(G(K_LINE, (np.nan, 0.0, 95.0), _screen(250, 129)))
    assert tuple(int(recs[0][f]) for f in ("x0", "y0", "x1", "y1")) == (0, 0, 250, 129) and counts == (1, 0, 0)
    # ... and a NaN that appears while clipping (inf - inf) ends the loop the same way
    with np.errstate(all="ignore"):
        c = ref_clip_line_to_rect(F(np.inf), F(50), F(100), F(60), F(0), F(0), F(320), F(240))
    assert c is not None and c[4] == 1 and c[0] == F(319) and np.isnan(c[1])
    # both behind the near plane; one end clipped by it first (whether the clipped end survives hangs on the last bit of
    # p0 + (p1 - p0) * t, tests/test_world.py: here the outcome is draw_3d_line_clipped's, and so is the record while it stays inside)
    assert _one(G(K_LINE, (0, 0, -5), (3, 3, 0.1)))[1] == (0, 1, 0)
    for p1 in ((0, 0, -5), (0.25, -0.5, -3), (0.125, 0.0, -40)):
        recs, counts = _one(G(K_LINE, _screen(169, 102), p1))
        wrec, wc = ref_world(R.world_item(abi.LINE_2D, _screen(169, 102), p1, b32.Color(200, 60, 30), alpha=0, flags=abi.WORLD_CLIP_NEAR), IDENTITY_CAM, None, 320, 240)
        assert recs.tobytes() == wrec.tobytes() and counts == wc


def test_clip_rounds_never_run_out_on_a_frame():
    """A segment that exhausts the 16 rounds could not be constructed for a frame rectangle (xmin = ymin = 0): every round moves the
    chosen end ONTO an edge line, which clears that end's bit for that edge for good (x = xmax - 1.0 and y = ymax - 1.0 are inside, x = 0.0
    and y = 0.0 are inside), and the other coordinate's bits can only be set once more per edge -- a finite end needs at most two rounds, a
    non-finite one turns into NaN (outcode 0).  So at most four rounds are ever taken; asserted over the random set and a sweep of
    adversarial ends (huge, tiny, denormal slopes), and the loop's exit is covered by a rectangle that is NOT a frame: xmax - 1.0 < xmin."""
    F = f32
    worst = 0
    rng = np.random.default_rng(5)
    vals = np.array([-3e38, -1e30, -1e9, -1e-40, -0.0, 0.0, 1e-40, 0.5, 239.0, 239.99998, 240.0, 319.0, 319.99997, 320.0, 1e9, 1e30, 3e38, np.inf, -np.inf, np.nan], f32)
    with np.errstate(all="ignore"):
        for _ in range(4000):
            x0, y0, x1, y1 = (F(v) for v in rng.choice(vals, 4))
            if rng.random() < 0.5:
                x0, y1 = F(rng.uniform(-1000, 1000)), F(rng.uniform(-1000, 1000))
            c = ref_clip_line_to_rect(x0, y0, x1, y1, F(0), F(0), F(320), F(240))
            if c is not None:
                worst = max(worst, c[4])
        assert worst <= 4, worst
        # not a frame: xmin = 10, xmax = 10.5 -> the RIGHT clip puts x at 9.5, which is LEFT; the LEFT clip puts it at 10.0 ... wait, 10.0 is
        # inside [10, 10.5): the rectangle that never converges needs xmax - 1.0 < xmin AND xmin >= xmax for the clipped value, i.e. an empty
        # one: xmin = 10, xmax = 10 -> every x is LEFT or RIGHT and each round swaps them
        assert ref_clip_line_to_rect(F(0), F(5), F(20), F(5), F(10), F(0), F(10), F(240)) is None


def test_ref_gizmos_thick_line_hand_cases():
    """Thickness 3: half = 1.5, offsets -1, 0, 1 -> ox = (px * offset / 1.5) as i32 with (px, py) = (-dy, dx) / len * 1.5."""
    assert ref_thick_offsets(10, 50, 110, 50, 3) == [(0, -1), (0, 0), (0, 1)]              # horizontal: px = -0.0, py = 1.5
    assert ref_thick_offsets(10, 50, 10, 150, 3) == [(1, 0), (0, 0), (-1, 0)]              # vertical: px = -1.5, py = 0
    # 45 degrees: |px| = |py| = 1.5 / sqrt(2) = 1.06; * (-1) / 1.5 = -+0.707 -> truncates to 0: three coincident lines
    assert ref_thick_offsets(10, 10, 110, 110, 3) == [(0, 0), (0, 0), (0, 0)]
    assert ref_thick_offsets(7, 7, 7, 7, 3) is None                                        # len < 0.001
    # thickness 16 on a horizontal: offsets -7.5 .. 7.5 -> oy = offset as i32 (toward zero: two zeros)
    assert [o[1] for o in ref_thick_offsets(0, 0, 50, 0, 16)] == [-7, -6, -5, -4, -3, -2, -1, 0, 0, 1, 2, 3, 4, 5, 6, 7]
    recs, counts = _one(G(K_THICK, _screen(16, 30), _screen(304, 30), size=3))
    assert counts == (1, 0, 0) and len(recs) == 3
    assert [tuple(int(r[f]) for f in ("x0", "y0", "x1", "y1", "kind")) for r in recs] == [(16, 29, 304, 29, 3), (16, 30, 304, 30, 3), (16, 31, 304, 31, 3)]
    assert all(r["z0"] == f32(95.0) and r["z1"] == f32(95.0) for r in recs)
    recs, counts = _one(G(K_THICK, _screen(16, 30), _screen(16, 30), size=3))              # len < 0.001: three no-ops, dropped
    assert recs.tobytes() == noop_records(3).tobytes() and counts == (0, 1, 0)
    for size in (1, 0, -4):                                                                # thickness <= 1: draw_3d_line_depth
        a, ca = _one(G(K_THICK, _screen(16, 30), _screen(304, 210), size=size)); b, cb = _one(G(K_LINE_DEPTH, _screen(16, 30), _screen(304, 210)))
        assert a.tobytes() == b.tobytes() and ca == cb == (1, 0, 0)
    # draw_3d_line_depth does NOT clip to the frame; its record is b32_draw_world's for B32_LINE_3D_OVERLAY + B32_WORLD_CLIP_NEAR
    from bonnie32_amd import rasterizer as R
    it = G(K_LINE_DEPTH, _screen(160, 120), _screen(520, 300), rgb=(9, 8, 7))
    wi = R.world_item(abi.LINE_3D_OVERLAY, _screen(160, 120), _screen(520, 300), b32.Color(9, 8, 7), alpha=0, flags=abi.WORLD_CLIP_NEAR)
    assert _one(it)[0].tobytes() == ref_world(wi, IDENTITY_CAM, None, 320, 240)[0].tobytes()
    # a point: world_to_screen, `as i32`, the radius
    recs, counts = _one(G(K_POINT, _screen(169, 102), size=4, blend=abi.ERASE))
    assert tuple(int(recs[0][f]) for f in ("x0", "y0", "size", "kind", "blend")) == (169, 102, 4, abi.PRIM_CIRCLE, abi.ERASE) and counts == (1, 0, 0)


def _rows(p0, p1, p2, w=40, h=30):
    return {y: (xs, xe) for y, xs, xe in ref_tri_spans(p0, p1, p2, w, h)}


def test_triangle_hand_cases():
    """draw_filled_triangle_3d by hand."""
    # flat top (y0 == y1): second_half on every row; the long edge runs (2, 3) -> (6, 11), the short one (12, 3) -> (6, 11)
    r = _rows((2, 3), (12, 3), (6, 11))
    assert r[3] == (2, 12) and r[7] == (4, 9) and r[11] == (6, 6) and sorted(r) == list(range(3, 12))
    # flat bottom (y1 == y2): the first half up to y1; the row y == y1 is not second_half (y > y1 is false) and uses the upper edge's end
    r = _rows((6, 3), (2, 11), (12, 11))
    assert r[3] == (6, 6) and r[7] == (4, 9) and r[11] == (2, 12)
    # two points equal: (5, 5), (5, 5), (9, 13) -> y1 == y0: the second half everywhere, both edges the same line
    r = _rows((5, 5), (5, 5), (9, 13))
    assert all(xs == xe for xs, xe in r.values()) and r[5] == (5, 5) and r[13] == (9, 9) and r[9] == (7, 7)
    # ... and (5, 5), (9, 13), (9, 13): the row y1 == y2 == 13 has segment_height (first half: y1 - y0 = 8) -> drawn from the upper edges
    assert _rows((5, 5), (9, 13), (9, 13))[13] == (9, 9)
    # the stable sort: with y1 == y2 the point that came first in the arguments is (x1, y1), the other one ends the long edge
    assert ref_tri_sorted((0, 0), (5, 4), (9, 4)) == [(0, 0), (5, 4), (9, 4)] and ref_tri_sorted((0, 0), (9, 4), (5, 4)) == [(0, 0), (9, 4), (5, 4)]
    assert ref_tri_sorted((4, 7), (1, 7), (0, 0)) == [(0, 0), (4, 7), (1, 7)]        # (an unstable sort may swap the two)
    # A triangle whose tie changes the SPAN could not be constructed, and there is none: with y0 == y1 every row is second_half and
    # segment_height == total_height, with y1 == y2 no row is and segment_height == total_height again -- so alpha and beta are the same
    # f32 in every row, and swapping the tied points only swaps the expressions of ax and bx, which the fill then orders.  The order
    # shows in the record (argument order kept) and in nothing else; checked here on every pair of tied triangles of a small lattice.
    rng = np.random.default_rng(4)
    for _ in range(400):
        (xa, xb, xc), (ya, yc) = (int(v) for v in rng.integers(-20, 60, 3)), (int(v) for v in rng.integers(-10, 40, 2))
        assert ref_tri_spans((xa, ya), (xb, ya), (xc, yc), 40, 30) == ref_tri_spans((xb, ya), (xa, ya), (xc, yc), 40, 30)
    #   rounding in the spans themselves: (0, 0), (7, 3), (100, 3), row 1: alpha = beta = 1/3 -> 0.33333334; 100 * alpha = 33.333336 -> 33, 7 * alpha -> 2
    assert _rows((0, 0), (7, 3), (100, 3), w=200)[1] == (2, 33) and _rows((0, 0), (100, 3), (7, 3), w=200)[1] == (2, 33)
    #   (0, 5), (10, 5), (3, 8), row 6: ax = 0 + 3 * 0.33333334 = 1.0000001 -> 1, bx = 10 + -7 * 0.33333334 = 7.666667 -> 7
    assert _rows((0, 5), (10, 5), (3, 8))[6] == (1, 7) == _rows((10, 5), (0, 5), (3, 8))[6]
    #   the third point ABOVE a tie: (4, 7), (1, 7), (0, 0) sorts to (0, 0), (4, 7), (1, 7): row 7 is first-half (y == y1), spans x1 .. x2
    r = _rows((4, 7), (1, 7), (0, 0))
    assert r[7] == (1, 4) and r[0] == (0, 0)
    # negative ax: `as i32` truncates toward zero, then .max(0).  (-3, 0), (1, 0), (-3, 8): second half everywhere, ax = -3 always,
    # bx = 1 + -4 * (y / 8): row 1: 0.5 -> 0: the pixel (0, 1) is drawn; row 3: -0.5 -> 0 (toward zero, not -1): drawn too; row 5: -1.5 -> -1: empty
    r = _rows((-3, 0), (1, 0), (-3, 8))
    assert r[1] == (0, 0) and r[2] == (0, 0) and r[3] == (0, 0) and r[4] == (0, -1) and r[5] == (0, -1) and r[6] == (0, -2)
    # a triangle left of the frame: every row empty
    assert all(xs > xe for xs, xe in _rows((-9, 0), (-1, 0), (-9, 8)).values())
    # wholly above / below the frame, and the frame's last row
    assert _rows((0, -9), (5, -2), (9, -1)) == {} and _rows((0, 30), (5, 35), (9, 31)) == {}
    assert sorted(_rows((0, 25), (5, 35), (9, 31))) == [25, 26, 27, 28, 29]
    # y2 == y0: nothing, although the three x differ
    assert _rows((0, 4), (5, 4), (9, 4)) == {}
    # x_end beyond the frame is clamped to w - 1
    assert _rows((30, 0), (60, 0), (30, 4), w=40)[0] == (30, 39)
    # the vectorised rows equal the literal ones
    rng = np.random.default_rng(3)
    for _ in range(300):
        p = [(int(rng.integers(-30, 90)), int(rng.integers(-20, 60))) for _ in range(3)]
        if rng.random() < 0.3:
            p[1] = (p[1][0], p[0][1])
        if rng.random() < 0.2:
            p[2] = (p[2][0], p[1][1])
        y, xs, xe = np_tri_spans(*p, 64, 40)
        assert list(zip(y.tolist(), xs.tolist(), xe.tolist())) == ref_tri_spans(*p, 64, 40), p
    # np_tri: bytes [r, g, b, 255] whatever the blend
    img = np.zeros((30 * 40, 4), np.uint8)
    np_tri(img, 40, 30, (2, 3), (12, 3), (6, 11), (9, 8, 7))
    im = img.reshape(30, 40, 4)
    assert im[3, 2:13].tolist() == [[9, 8, 7, 255]] * 11 and not im[3, 13].any() and not im[2].any() and im[11, 6].tolist() == [9, 8, 7, 255]
    assert int((im[..., 3] == 255).sum()) == sum(xe - xs + 1 for xs, xe in _rows((2, 3), (12, 3), (6, 11)).values())


def test_ref_gizmos_triangle_records():
    """Both project_vertex forms: cam.z < 0.1 against cam_z <= 0.1, the ortho branch for kind 5 only, argument order kept."""
    p = [_screen(169, 102), _screen(16, 30), _screen(304, 210)]
    for kind in (K_TRI, K_TRI_VIEW):
        recs, counts = _one(G(kind, *p, rgb=(5, 6, 7), blend=abi.ERASE))
        assert counts == (1, 0, 0) and int(recs[0]["kind"]) == TRI and tri_points(recs[0]) == ((169, 102), (16, 30), (304, 210))
        assert (int(recs[0]["r"]), int(recs[0]["blend"]), int(recs[0]["size"])) == (5, abi.ERASE, 0)
    edge = (0.0, 0.0, float(f32(0.1)))                                # cam_z == 0.1f exactly
    assert _one(G(K_TRI, edge, p[1], p[2]))[1] == (1, 0, 0) and _one(G(K_TRI_VIEW, edge, p[1], p[2]))[1] == (0, 1, 0)
    below = (0.0, 0.0, float(np.nextafter(f32(0.1), f32(0))))
    assert _one(G(K_TRI, below, p[1], p[2]))[1] == (0, 1, 0)
    # kind 5 takes the ortho (which never answers None), kind 4 and the lines ignore it
    behind = (40.0, 10.0, -50.0)
    recs, counts = _one(G(K_TRI_VIEW, behind, p[1], p[2]), ortho=(2.0, 0.0, 0.0))
    assert counts == (1, 0, 0) and tri_points(recs[0])[0] == (160 + 80, 120 - 20)
    assert _one(G(K_TRI, behind, p[1], p[2]), ortho=(2.0, 0.0, 0.0))[1] == (0, 1, 0)
    a = _one(G(K_LINE, p[1], p[2]), ortho=(2.0, 0.0, 0.0))[0]; b = _one(G(K_LINE, p[1], p[2]))[0]
    assert a.tobytes() == b.tobytes()
    # y2 == y0 after projection: dropped; beyond 2^30: rejected
    assert _one(G(K_TRI, _screen(16, 30), _screen(160, 30), _screen(304, 30)))[1] == (0, 1, 0)
    assert _one(G(K_TRI, (3e9, 0.0, 0.2), p[1], p[2]))[1] == (0, 0, 1)
    assert _one(G(K_THICK, (3e9, 0.0, 0.2), p[1], size=3))[1] == (0, 0, 1) and _one(G(K_LINE_DEPTH, (7e8, 0.0, 0.2), (-7e8, 0.0, 0.2)))[1] == (0, 0, 1)
    assert _one(G(K_LINE, (3e9, 0.0, 0.2), p[1]))[1] == (1, 0, 0)      # the screen clip brings it back to the frame


def _py_octahedron(center, size, rgbb):
    """draw_filled_octahedron, viewport_3d.rs:6231-6291, as items."""
    cx, cy, cz = (f32(v) for v in center)
    s = f32(size)
    top, bottom, front, back, left, right = (cx, cy + s, cz), (cx, cy - s, cz), (cx, cy, cz + s), (cx, cy, cz - s), (cx - s, cy, cz), (cx + s, cy, cz)
    faces = [(top, front, right), (top, right, back), (top, back, left), (top, left, front),
             (bottom, right, front), (bottom, back, right), (bottom, left, back), (bottom, front, left)]
    edges = [(top, front), (top, back), (top, left), (top, right), (bottom, front), (bottom, back), (bottom, left), (bottom, right),
             (front, right), (right, back), (back, left), (left, front)]
    edge = tuple((c * 3 // 4) & 255 for c in rgbb[:3])
    return np.concatenate([G(K_TRI, *f, rgb=rgbb[:3], blend=rgbb[3]) for f in faces] + [G(K_LINE, *e, rgb=edge, blend=abi.OPAQUE) for e in edges])


def test_octahedron_items_equal_the_restatement():
    """b32_octahedron_items (no context) against draw_filled_octahedron restated: corners as f32 centre +- size, faces, edge colour, edges."""
    from bonnie32_amd import rasterizer as R
    for center, size, rgbb in (((10.5, -3.25, 700.0), 24.0, (255, 200, 50, abi.OPAQUE)), ((1e7, 0.1, -0.3), 0.7, (1, 2, 3, abi.ERASE)),
                               ((0.0, 0.0, 0.0), 1e-3, (0, 255, 127, abi.ADD))):
        got = R.octahedron_items(center, size, b32.Color(*rgbb))
        assert got.tobytes() == _py_octahedron(center, size, rgbb).tobytes()
    b = R.GizmoBatch(None)
    b.line((0, 0, 1), (1, 1, 2), b32.Color(1, 2, 3)); b.octahedron((10.5, -3.25, 700.0), 24.0, b32.Color(255, 200, 50))
    b.thick_line_depth((0, 0, 1), (1, 1, 2), b32.Color(1, 2, 3), 3); b.point((1, 2, 3), 4, b32.Color(9, 9, 9, abi.ERASE))
    b.line_depth((0, 0, 1), (1, 1, 2), b32.Color(1, 2, 3)); b.triangle_view((0, 0, 1), (1, 1, 2), (2, 2, 2), b32.Color(1, 2, 3))
    b.triangle((0, 0, 1), (1, 1, 2), (2, 2, 2), b32.Color(1, 2, 3))
    I = b.items()
    assert I["kind"].tolist() == [0] + [4] * 8 + [0] * 12 + [2, 3, 1, 5, 4] and I[1:21].tobytes() == _py_octahedron((10.5, -3.25, 700.0), 24.0, (255, 200, 50, 0)).tobytes()
    assert (int(I["size"][21]), int(I["size"][22]), int(I["blend"][22]), I["p2"][24].tolist()) == (3, 4, abi.ERASE, [2.0, 2.0, 2.0])
    assert not I["_pad"].any()


def gizmo_census(items, camera, w, h):
    """What the random set exercises, by the literal model."""
    cam = _cam_f32(camera)
    c = dict(kind0=0, kind0_drawn=0, kind0_shortened=0, kind0_screen_rejected=0, lines=0, lines_near_clipped=0, ties_top=0, ties_bottom=0, ties_all=0,
             rej_extent=0, rej_coord=0, kinds=set())
    counts = ref_gizmos(items, camera, None, w, h)[1]
    with np.errstate(all="ignore"):
        for i, it in enumerate(items):
            kind = int(it["kind"])
            c["kinds"].add(kind)
            p = [tuple(f32(v) for v in it[n]) for n in ("p0", "p1", "p2")]
            if kind in LINE_KINDS:
                c["lines"] += 1
                cl = ref_clip(p[0], p[1], cam)
                if cl is not None and cl != (p[0], p[1]):
                    c["lines_near_clipped"] += 1
                ends = None if cl is None else [ref_world_to_screen(q, cam, w, h) for q in cl]
                if ends is None or any(e is None for e in ends):
                    continue
                if kind == K_LINE:
                    sc = ref_clip_line_to_rect(ends[0][0], ends[0][1], ends[1][0], ends[1][1], f32(0), f32(0), f32(w), f32(h))
                    if sc is None:
                        c["kind0_screen_rejected"] += 1
                    else:
                        c["kind0_drawn"] += 1
                        c["kind0_shortened"] += sc[4] > 0
                else:
                    xy = [_as_i32(v) for e in ends for v in e[:2]]
                    if abs(xy[2] - xy[0]) >= LIM or abs(xy[3] - xy[1]) >= LIM:
                        c["rej_extent"] += 1
                    elif kind == K_THICK and int(it["size"]) > 1 and any(abs(v) >= LIM for v in xy):
                        c["rej_coord"] += 1
            elif kind >= K_TRI:
                pts = [ref_project_vertex(q, cam, w, h) if kind == K_TRI else ref_project_vertex_view(q, cam, w, h, None) for q in p]
                if any(q is None for q in pts):
                    continue
                if any(abs(v) >= LIM for q in pts for v in q):
                    c["rej_coord"] += 1
                    continue
                (_, y0), (_, y1), (_, y2) = ref_tri_sorted(*pts)
                c["ties_all"] += y0 == y2
                c["ties_top"] += y0 == y1 != y2
                c["ties_bottom"] += y0 != y1 == y2
    c["kind0"] = int((items["kind"] == K_LINE).sum())
    c["counts"] = counts
    return c


def test_random_set_census():
    """The floors of the issue on the inputs (not on the code): the random set is not trivial."""
    I = the_random_set()
    for w, h in SIZES:
        c = gizmo_census(I, CENSUS_CAM, w, h)
        n = len(I)
        assert c["kinds"] == set(range(6))
        assert c["kind0_shortened"] * 4 >= c["kind0_drawn"] > 100, c
        assert c["kind0_screen_rejected"] * 50 >= c["kind0"], c
        assert c["lines_near_clipped"] * 10 >= c["lines"], c
        assert c["counts"][1] * 20 >= n and sum(c["counts"]) == n, c
        assert min(c["ties_top"], c["ties_bottom"], c["ties_all"]) >= 5, c
        assert c["rej_extent"] >= 1 and c["rej_coord"] >= 1 and c["counts"][2] >= c["rej_extent"] + c["rej_coord"], c
        assert c["counts"][0] * 3 >= n, c


def hand_items():
    """The hand cases above as one batch for the identity camera at 320x240."""
    p = [_screen(169, 102), _screen(16, 30), _screen(304, 210)]
    return np.concatenate([
        G(K_LINE, _screen(16, 30), _screen(304, 210), blend=abi.ERASE), G(K_LINE, _screen(160, 120), _screen(520, 300)), G(K_LINE, _screen(-20, 120), _screen(340, 120)),
        G(K_LINE, _screen(-20, 12), _screen(16, -24)), G(K_LINE, _screen(-20, 30), _screen(70, -60)), G(K_LINE, (np.nan, 0.0, 95.0), _screen(250, 129)),
        G(K_LINE, (np.inf, 0.0, 95.0), _screen(250, 129)), G(K_LINE, (0, 0, -5), (3, 3, 0.1)), G(K_LINE, (0, 0, 95), (0, 0, -5)), G(K_LINE, (3e9, 0.0, 0.2), p[1]),
        G(K_THICK, _screen(16, 30), _screen(304, 30), size=3), G(K_THICK, _screen(16, 30), _screen(16, 210), size=3), G(K_THICK, _screen(16, 30), _screen(196, 210), size=3),
        G(K_THICK, _screen(16, 30), _screen(16, 30), size=3), G(K_THICK, _screen(16, 30), _screen(304, 210), size=16), G(K_THICK, _screen(16, 30), _screen(304, 210), size=1),
        G(K_THICK, _screen(16, 30), _screen(304, 210), size=-4), G(K_THICK, (3e9, 0.0, 0.2), p[1], size=3), G(K_LINE_DEPTH, _screen(160, 120), _screen(520, 300)),
        G(K_LINE_DEPTH, (7e8, 0.0, 0.2), (-7e8, 0.0, 0.2)), G(K_LINE_DEPTH, (np.nan, 0.0, 95.0), (1.0, np.nan, 95.0)), G(K_POINT, _screen(169, 102), size=4, blend=abi.ERASE),
        G(K_POINT, (0, 0, 0.05), size=4), G(K_POINT, (-3e9, 0, 0.2), size=4), G(K_TRI, *p), G(K_TRI_VIEW, *p), G(K_TRI, (0.0, 0.0, float(f32(0.1))), p[1], p[2]),
        G(K_TRI_VIEW, (0.0, 0.0, float(f32(0.1))), p[1], p[2]), G(K_TRI, _screen(16, 30), _screen(160, 30), _screen(304, 30)), G(K_TRI, _screen(16, 30), _screen(160, 30), _screen(97, 210)),
        G(K_TRI, _screen(97, 30), _screen(16, 210), _screen(304, 210)), G(K_TRI, _screen(16, 30), _screen(16, 30), _screen(97, 210)), G(K_TRI, _screen(160, 30), _screen(16, 30), _screen(97, -60)),
        G(K_TRI, _screen(-200, 30), _screen(16, 30), _screen(-200, 210)), G(K_TRI, _screen(16, -600), _screen(160, -330), _screen(97, -60)),
        G(K_TRI, _screen(16, 300), _screen(160, 3000), _screen(97, 597)), G(K_TRI, (3e9, 0.0, 0.2), p[1], p[2]), G(K_TRI_VIEW, (40.0, 10.0, -50.0), p[1], p[2]),
        G(K_TRI, (np.nan, 0.0, 95.0), p[1], p[2])])


def _check_host(items, cam, ortho, w, h):
    want, wc = ref_gizmos(items, cam, ortho, w, h)
    got, gc, which, spans = host_gizmos(items, cam, ortho, w, h)
    assert got.tobytes() == want.tobytes(), np.nonzero(got != want)[0][:8]
    assert gc == wc and tuple(int((which == k).sum()) for k in range(3)) == wc
    assert np.array_equal(spans, ref_spans_table(want, w, h))
    return want, spans


def test_host_compile_of_the_device_header_equals_ref_gizmos():
    """csrc/b32_gizmo_body.h built for the host (g++ -O1 -ffp-contract=off): records, counts and triangle spans equal ref_gizmos bit for
    bit on the hand cases (perspective and ortho) and on the random set, at 320x240 and 203x117."""
    H = hand_items()
    recs, spans = _check_host(H, IDENTITY_CAM, None, 320, 240)
    assert (recs["kind"] == TRI).sum() >= 8 and len(spans) > 500
    _check_host(H, IDENTITY_CAM, (2.0, 0.0, 0.0), 320, 240)
    for w, h in SIZES:
        for ortho in (None, ORTHO):
            _check_host(the_random_set(), CENSUS_CAM, ortho, w, h)


def lattice_triangles(rng, n, w, h):
    """Triangles with integer screen points as B32_GIZMO_TRIANGLE_VIEW items for the identity camera and OrthoProjection { zoom 1,
    centre (0, 0) }: sx = cam_x + w / 2, sy = -cam_y + h / 2, all exact -- so only the fill's arithmetic is exercised."""
    P = np.stack([rng.integers(-40, w + 40, (n, 3)), rng.integers(-30, h + 30, (n, 3))], axis=2)
    I = np.zeros(n, abi.GIZMO_ITEM_DTYPE)
    I["kind"] = K_TRI_VIEW
    for k, f in enumerate(("p0", "p1", "p2")):
        I[f][:, 0] = P[:, k, 0] - w // 2; I[f][:, 1] = -(P[:, k, 1] - h // 2); I[f][:, 2] = 10.0
    return I, P


def _rows_differ(a, b):
    return int((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1).sum())


def test_random_set_tells_a_fused_evaluation_apart():
    """The same program built with FMA contraction (g++ -O2 -ffp-contract=fast -mfma) gives other records on the random set, and other
    spans on 3 000 lattice triangles (whose points are exact either way: x0 as f32 + (x2 - x0) as f32 * alpha fused keeps the bits
    below alpha's rounding, and `as i32` lands on the other side of an integer): nothing contracted can pass the comparisons of this file."""
    I = the_random_set()
    n_rec = 0
    for w, h in SIZES:
        a = host_gizmos(I, CENSUS_CAM, None, w, h, "off"); b = host_gizmos(I, CENSUS_CAM, None, w, h, "fused")
        assert len(a[0]) == len(b[0])
        n_rec += _rows_differ(a[0], b[0])
    L, P = lattice_triangles(np.random.default_rng(7002), 3000, 320, 240)
    a = host_gizmos(L, IDENTITY_CAM, (1.0, 0.0, 0.0), 320, 240, "off"); b = host_gizmos(L, IDENTITY_CAM, (1.0, 0.0, 0.0), 320, 240, "fused")
    want = ref_gizmos(L, IDENTITY_CAM, (1.0, 0.0, 0.0), 320, 240)[0]
    assert a[0].tobytes() == b[0].tobytes() == want.tobytes() and [tri_points(r) for r in want[:50] if r["kind"] == TRI] == \
        [tuple(map(tuple, p.tolist())) for p, r in zip(P[:50], want[:50]) if r["kind"] == TRI]
    assert np.array_equal(a[3], ref_spans_table(want, 320, 240)) and a[3].shape == b[3].shape
    n_span = _rows_differ(a[3], b[3])
    assert n_rec >= 10 and n_span >= 10, (n_rec, n_span)


def test_cpp_mirror_gizmos_compile():
    """host/rasterizer.hpp: draw_gizmos, gizmo_counts and the GizmoBatch builder compile (header-only over the C ABI)."""
    hpp_dir = os.path.join(ROOT, "bonnie-32_amd", "host")
    src = ('#include "rasterizer.hpp"\nvoid f(b32::Framebuffer& fb, const b32::Camera& cam) { b32::Color c{ 1, 2, 3, b32::BlendMode::Erase };\n'
           ' b32::GizmoBatch g(fb); g.line({ 0, 0, 1 }, { 1, 1, 2 }, c); g.line_depth({ 0, 0, 1 }, { 1, 1, 2 }, c); g.thick_line_depth({ 0, 0, 1 }, { 1, 1, 2 }, c, 3);\n'
           ' g.point({ 1, 2, 3 }, 4, c); g.triangle({ 0, 0, 1 }, { 1, 1, 2 }, { 2, 2, 2 }, c); g.triangle_view({ 0, 0, 1 }, { 1, 1, 2 }, { 2, 2, 2 }, c);\n'
           ' g.octahedron({ 1, 2, 3 }, 24.0f, c); (void)g.size(); g.flush(cam, b32::Vec3{ 1.0f, 0.0f, 0.0f });\n'
           ' b32::draw_gizmos(fb, { b32::Framebuffer::gizmo_item(B32_GIZMO_POINT, { 1, 2, 3 }, { 0, 0, 0 }, { 0, 0, 0 }, c, 4) }, cam);\n'
           ' fb.draw_gizmos(g.items(), cam); (void)fb.gizmo_counts().rejected; }\nint main() { (void)&f; return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", hpp_dir, "-I", os.path.join(ROOT, "include"),
                        os.path.join(d, "t.cpp")], check=True)


# ================================================================== GPU
def _counts_delta(fb, before):
    return tuple(a - b for a, b in zip(fb.gizmo_counts(), before))


@pytest.mark.gpu
def test_gpu_gizmo_stage_tap(gpu_ctx):
    """b32_gizmo_project_batch == ref_gizmos byte for byte (NaN depths as 0x7FC00000) on the random set and the hand cases, at 320x240
    and 203x117, with and without an ortho; the counts move by the model's counts."""
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(64, 64, gpu_ctx)
    for cam, I in ((CENSUS_CAM, the_random_set()), (IDENTITY_CAM, hand_items())):
        for w, h in SIZES if cam is CENSUS_CAM else ((320, 240),):
            for ortho in (None, ORTHO):
                want, wc = ref_gizmos(I, cam, ortho, w, h)
                c0 = fb.gizmo_counts()
                got = gpu_ctx.gizmo_project_batch(I, cam, ortho, w, h)
                assert len(got) == len(want) and got.tobytes() == want.tobytes(), f"{w}x{h} ortho={ortho}: records {np.nonzero(got != want)[0][:8]} differ"
                assert _counts_delta(fb, c0) == wc
    assert len(gpu_ctx.gizmo_project_batch(the_random_set()[:0], CENSUS_CAM, None, 320, 240)) == 0


@functools.lru_cache(maxsize=None)
def _room(w, h):
    """The golden room drawn in z-buffer mode by the oracle at w x h: (scene, pixels, z-buffer, zmax)."""
    from oracle import oracle as O
    sc = _game_scene()
    sc.settings.use_zbuffer = True
    ofb = O.Framebuffer(w, h)
    ofb.clear(sc.clear_color)
    assert O.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)[0] == 0
    zs = ofb.zbuffer[ofb.zbuffer < 1e30]
    return sc, ofb.pixels.copy(), ofb.zbuffer.copy(), float(zs.max())


def _load(fb, px, zb):
    fb.upload(px)
    _upload_zbuffer(fb, zb)


def _frame_batches():
    """(name, w, h, items) of the frames test: 1, 48 (the last small batch), 49 (the first staged), about 3 000 (the tile route over
    several workgroups), and at 640x480 three triangles that cover the whole frame with small items before, between and after."""
    sc, _, _, zmax = _room(320, 240)
    rng = np.random.default_rng(7100)
    big = frame_gizmos(rng, 3000, sc.camera, zmax)
    _, px, zb, _ = _room(320, 240)

    def visible(it):
        want = px.copy()
        cpu_gizmos(want, zb, 320, 240, it, sc.camera)
        return not np.array_equal(want, px)

    one = next(big[i:i + 1] for i in range(200) if big["kind"][i] == K_LINE and visible(big[i:i + 1]))      # (a clipped line that shows)
    out = [("one", 320, 240, one), ("48", 320, 240, big[:48]), ("49", 320, 240, big[100:149]), ("3000", 320, 240, big)]
    cam = sc.camera
    far = [cam_point(cam, sx * 3.0 * zmax, sy * 3.0 * zmax, 0.5 * zmax) for sx, sy in ((-1, -1), (1, -1), (-1, 1), (1, 1))]
    cover = [G(K_TRI, far[0], far[1], far[2], rgb=(200, 10, 10)), G(K_TRI_VIEW, far[1], far[3], far[2], rgb=(10, 200, 10)), G(K_TRI, far[0], far[3], far[2], rgb=(10, 10, 200), blend=abi.ERASE)]
    small = frame_gizmos(rng, 200, sc.camera, zmax)
    out.append(("cover", 640, 480, np.concatenate([small[:50], cover[0], small[50:100], cover[1], small[100:150], cover[2], small[150:]])))
    return out


@pytest.mark.gpu
def test_gpu_gizmo_frames_and_routes(gpu_ctx):
    """Batches of 1, 48, 49, about 3 000 items and the screen-covering triangles over the golden room in z-buffer mode: pixels equal the
    CPU composition, the z-buffer is unchanged, the counts move by the model's; then the same frames with B32_ROUTE_PRIM_TILES off."""
    from bonnie32_amd import rasterizer as R
    expect = []
    for name, w, h, items in _frame_batches():
        sc, px, zb, _ = _room(w, h)
        want = px.copy()
        wc = cpu_gizmos(want, zb, w, h, items, sc.camera)
        assert not np.array_equal(want, px), name
        expect.append((name, w, h, items, want, wc))
    assert expect[-1][5][0] >= 100 and expect[3][5][0] > 1000 and expect[3][5][1] > 100      # (the batches are not trivial)
    try:
        for routes in (0, R.Context.ROUTE_PRIM_TILES):
            gpu_ctx.set_routes(routes)
            for name, w, h, items, want, wc in expect:
                sc, px, zb, _ = _room(w, h)
                fb = R.Framebuffer(w, h, gpu_ctx)
                _load(fb, px, zb)
                r0, c0 = gpu_ctx.route_counts(), fb.gizmo_counts()
                fb.draw_gizmos(items, sc.camera)
                got = fb.pixels
                assert np.array_equal(got, want), f"{name} routes={routes}: {int((got != want).sum())} bytes differ"
                _same_z(fb, zb)
                assert _counts_delta(fb, c0) == wc
                r1 = gpu_ctx.route_counts()
                n_rec = len(ref_gizmos(items, sc.camera, None, w, h)[0])
                tiles = n_rec > 48 and routes == 0
                assert (r1["prim_tiles"] - r0["prim_tiles"], r1["prim_scan"] - r0["prim_scan"]) == (int(tiles), int(not tiles)), (name, routes)
    finally:
        gpu_ctx.set_routes(0)


@pytest.mark.gpu
def test_gpu_gizmo_order(gpu_ctx):
    """An octahedron's fill followed by its edges and the same items reversed; a triangle over and under a LINE_DEPTH item; an Erase
    kind-0 line (alpha byte 0) crossed by a triangle (alpha byte 255) in both orders: each order gives its own reference image."""
    from bonnie32_amd import rasterizer as R
    W, H = 320, 240
    sc, px, zb, zmax = _room(W, H)
    cam = sc.camera
    fb = R.Framebuffer(W, H, gpu_ctx)
    octa = R.octahedron_items(cam_point(cam, 0.02 * zmax, 0.01 * zmax, 0.25 * zmax), 0.06 * zmax, b32.Color(255, 200, 50))
    a, b, c = (cam_point(cam, x * zmax, y * zmax, 0.3 * zmax) for x, y in ((-0.1, -0.08), (0.12, -0.02), (0.0, 0.1)))
    tri = G(K_TRI, a, b, c, rgb=(40, 90, 220))
    depth_line = G(K_LINE_DEPTH, cam_point(cam, -0.15 * zmax, 0.0, 0.02 * zmax), cam_point(cam, 0.15 * zmax, 0.02 * zmax, 0.04 * zmax), rgb=(250, 250, 0))
    erase_line = G(K_LINE, cam_point(cam, -0.15 * zmax, -0.05 * zmax, 0.3 * zmax), cam_point(cam, 0.4 * zmax, 0.09 * zmax, 0.3 * zmax), rgb=(7, 7, 7), blend=abi.ERASE)
    for name, items in (("octahedron", octa), ("depth line", np.concatenate([tri, depth_line])), ("erase line", np.concatenate([erase_line, tri]))):
        results = []
        for order in (items, items[::-1].copy()):
            want = px.copy()
            wc = cpu_gizmos(want, zb, W, H, order, cam)
            assert wc == (len(items), 0, 0), (name, wc)
            _load(fb, px, zb)
            fb.draw_gizmos(order, cam)
            got = fb.pixels
            assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} bytes differ"
            _same_z(fb, zb)
            results.append(got)
        assert not np.array_equal(results[0], results[1]), name
        if name == "erase line":
            al = [r.reshape(-1, 4)[:, 3] for r in results]
            assert (al[1] == 0).sum() > (al[0] == 0).sum() > 0                       # the line last: its alpha-0 pixels cross the triangle


@pytest.mark.gpu
def test_gpu_gizmo_band(gpu_ctx):
    """320x240 with the band at rows 37..151: rows outside are untouched, rows inside equal the full frame's; an empty band draws nothing."""
    from bonnie32_amd import rasterizer as R
    W, H = 320, 240
    sc, px, zb, zmax = _room(W, H)
    fb = R.Framebuffer(W, H, gpu_ctx)
    rng = np.random.default_rng(7200)
    try:
        for n in (40, 700):
            I = frame_gizmos(rng, n, sc.camera, zmax)
            full = px.copy()
            wc = cpu_gizmos(full, zb, W, H, I, sc.camera)
            part = px.reshape(H, -1).copy(); part[37:151] = full.reshape(H, -1)[37:151]
            assert not np.array_equal(part[37:151], px.reshape(H, -1)[37:151]) and not np.array_equal(full.reshape(H, -1)[:37], px.reshape(H, -1)[:37])
            fb.set_band(0, H)
            _load(fb, px, zb)
            fb.set_band(37, 151)
            c0 = fb.gizmo_counts()
            fb.draw_gizmos(I, sc.camera)
            assert _counts_delta(fb, c0) == wc
            fb.set_band(90, 90)
            fb.draw_gizmos(I, sc.camera)                                      # an empty band: nothing, not even counted
            assert _counts_delta(fb, c0) == wc
            fb.set_band(0, H)
            assert np.array_equal(fb.pixels, part.reshape(-1))
            _same_z(fb, zb)
    finally:
        fb.set_band(0, H)


@pytest.mark.gpu
def test_gpu_gizmo_pipeline(oracle):
    """Two frames in flight through b32_frame_submit + b32_draw_gizmos + b32_fb_download_async, the caller's item array overwritten right
    after each call: every delivered frame is exact (the console's settings: the depth kinds test against the frame's own z-buffer)."""
    from bonnie32_amd import rasterizer as R, scenegen
    rng = np.random.default_rng(7300)
    ctx = R.Context(0)
    try:
        st = b32.RasterSettings.game()
        meshes = [scenegen.make_scene("C1", n_tris=800, seed=300 + i, variant="gouraud") for i in range(2)]
        W, H = meshes[0].width, meshes[0].height
        cam = meshes[0].camera
        fb = R.Framebuffer(W, H, ctx)
        slots = [R.ResidentScene(fb, m.vertices, m.faces, m.textures).detach() for m in meshes]
        table = ctx.make_frame_table(cam, st, slots)
        bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
        frames = [(random_gizmos(rng, 36, cam, spread=(12.0, 9.0), depth=(-5.0, 60.0), seg=8.0, hostile=False),
                   random_gizmos(rng, 500, cam, spread=(12.0, 9.0), depth=(-5.0, 60.0), seg=8.0, hostile=False)) for _ in range(3)]
        want = []
        for small, large in frames:
            o = oracle.Framebuffer(W, H); o.clear(b32.Color(10, 10, 30))
            for m in meshes:
                assert oracle.render_mesh_15(o, m.vertices, m.faces, m.textures, cam, st)[0] == 0
            px = o.pixels.copy()
            zb = o.zbuffer if st.use_zbuffer else None
            cpu_gizmos(px, zb, W, H, small, cam); cpu_gizmos(px, zb, W, H, large, cam)
            assert not np.array_equal(px, o.pixels)
            want.append(px)
        assert not np.array_equal(want[0], want[1])
        tickets = []
        for i, (small, large) in enumerate(frames):
            fb.clear(b32.Color(10, 10, 30))
            ctx.frame_submit(table)
            for items in (small, large):
                arr = items.copy()
                fb.draw_gizmos(arr, cam)
                arr[:] = random_gizmos(rng, len(arr), cam, hostile=False)     # the caller reuses its array at once
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
def test_gpu_gizmo_invalid_zbuffer():
    """A fresh framebuffer's z-buffer is not valid: LINE_DEPTH and THICK_LINE_DEPTH items draw as against f32::MAX (every finite depth
    passes, a NaN depth does not), and b32_zbuffer_download still answers f32::MAX everywhere."""
    from bonnie32_amd import rasterizer as R
    W, H = 203, 117
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        fb.clear(b32.Color(3, 4, 5))
        base = fb.pixels
        rng = np.random.default_rng(7400)
        I = random_gizmos(rng, 300, IDENTITY_CAM, kinds=(K_LINE_DEPTH, K_THICK, K_TRI), spread=(12.0, 9.0), depth=(-5.0, 60.0), seg=8.0, hostile=False)
        I = np.concatenate([I, G(K_LINE_DEPTH, (np.nan, 0.0, 30.0), (2.0, np.nan, 30.0), rgb=(255, 0, 255))])
        want = base.copy()
        wc = cpu_gizmos(want, None, W, H, I, IDENTITY_CAM)
        assert wc[0] > 150 and not np.array_equal(want, base)
        fb.draw_gizmos(I, IDENTITY_CAM)
        assert np.array_equal(fb.pixels, want)
        assert fb.gizmo_counts() == wc
        assert (fb.zbuffer == np.finfo(f32).max).all()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_gizmo_argument_errors(gpu_ctx):
    """An unknown kind, non-zero padding, a thickness beyond 16: B32_E_ARG; a point radius beyond 32767: B32_E_UNSUPPORTED -- small and
    staged batches, draw and tap, the frame and the counts untouched; NULL arguments; n == 0; b32_draw_prims with kind 11 and
    b32_draw_world with flag 2 still answer B32_E_ARG."""
    from bonnie32_amd import rasterizer as R
    W, H = 200, 150
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(b32.Color(1, 2, 3))
    base = fb.pixels
    rng = np.random.default_rng(7500)
    good = random_gizmos(rng, 30, IDENTITY_CAM, spread=(12.0, 9.0), depth=(40.0, 60.0), seg=8.0, hostile=False)
    c0 = fb.gizmo_counts()
    cases = [({"kind": 6}, abi.B32_E_ARG), ({"kind": 11}, abi.B32_E_ARG), ({"kind": 255}, abi.B32_E_ARG),
             ({"_pad": (1, 0, 0)}, abi.B32_E_ARG), ({"_pad": (0, 1, 0)}, abi.B32_E_ARG), ({"_pad": (0, 0, 128)}, abi.B32_E_ARG),
             ({"kind": K_THICK, "size": 17}, abi.B32_E_ARG), ({"kind": K_THICK, "size": 1 << 30}, abi.B32_E_ARG),
             ({"kind": K_POINT, "size": 32768}, abi.B32_E_UNSUPPORTED), ({"kind": K_POINT, "size": -32768}, abi.B32_E_UNSUPPORTED)]
    for n in (30, 300):
        batch = np.concatenate([good] * (n // 30))
        for fields, code in cases:
            bad = batch.copy()
            for f, v in fields.items():
                bad[f][n // 2] = v
            for call in (lambda: fb.draw_gizmos(bad, IDENTITY_CAM), lambda: gpu_ctx.gizmo_project_batch(bad, IDENTITY_CAM, None, W, H)):
                with pytest.raises(R.B32Error) as e:
                    call()
                assert e.value.code == code, fields
    assert np.array_equal(fb.pixels, base) and fb.gizmo_counts() == c0
    lib, cam = gpu_ctx.lib, IDENTITY_CAM.pack()
    out = np.zeros(64, abi.PRIM_DTYPE); nrec = C.c_uint32(77)
    assert lib.b32_draw_gizmos(gpu_ctx.h, None, None, good.ctypes.data, len(good)) == abi.B32_E_ARG
    assert lib.b32_draw_gizmos(gpu_ctx.h, C.byref(cam), None, None, 5) == abi.B32_E_ARG
    assert lib.b32_draw_gizmos(None, C.byref(cam), None, good.ctypes.data, len(good)) == abi.B32_E_ARG
    assert lib.b32_gizmo_counts(gpu_ctx.h, None, None, None) == abi.B32_E_ARG
    assert lib.b32_gizmo_project_batch(gpu_ctx.h, C.byref(cam), None, good.ctypes.data, len(good), W, H, out.ctypes.data, 64, None) == abi.B32_E_ARG
    assert lib.b32_gizmo_project_batch(gpu_ctx.h, C.byref(cam), None, good.ctypes.data, len(good), W, H, None, 64, C.byref(nrec)) == abi.B32_E_ARG
    assert lib.b32_gizmo_project_batch(gpu_ctx.h, C.byref(cam), None, good.ctypes.data, len(good), W, H, out.ctypes.data, 29, C.byref(nrec)) == abi.B32_E_ARG
    assert lib.b32_gizmo_project_batch(gpu_ctx.h, C.byref(cam), None, good.ctypes.data, len(good), 0, H, out.ctypes.data, 64, C.byref(nrec)) == abi.B32_E_ARG
    assert lib.b32_octahedron_items(None, C.c_float(1.0), None, None) == abi.B32_E_ARG
    assert lib.b32_draw_gizmos(gpu_ctx.h, C.byref(cam), None, None, 0) == abi.B32_OK          # n == 0: a no-op
    fb.draw_gizmos(good[:0], IDENTITY_CAM)
    assert np.array_equal(fb.pixels, base) and fb.gizmo_counts() == c0
    ok = good.copy()                                                   # accepted: thickness 16 and below 1, radius +-32767 (off screen)
    ok["kind"][:4] = (K_THICK, K_THICK, K_POINT, K_POINT); ok["size"][:4] = (16, -5, 32767, -32767); ok["p0"][2] = (1e6, 1e6, 50)
    recs = gpu_ctx.gizmo_project_batch(ok, IDENTITY_CAM, None, W, H)
    assert recs.tobytes() == ref_gizmos(ok, IDENTITY_CAM, None, W, H)[0].tobytes() and sum(_counts_delta(fb, c0)) == len(ok)
    # still rejected by the older entries
    p = np.zeros(3, abi.PRIM_DTYPE); p["kind"][1] = TRI
    with pytest.raises(R.B32Error) as e:
        fb.draw_prims(p)
    assert e.value.code == abi.B32_E_ARG
    wi = R.world_item(abi.LINE_2D, (0, 0, 50), (1, 1, 50), b32.Color(1, 2, 3), flags=2)
    with pytest.raises(R.B32Error) as e:
        fb.draw_world(wi, IDENTITY_CAM)
    assert e.value.code == abi.B32_E_ARG
    assert np.array_equal(fb.pixels, base)
