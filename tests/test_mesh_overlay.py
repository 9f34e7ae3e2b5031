"""The modeler's selection overlays from resident vertices (b32_draw_mesh_overlay): draw_selected_object_brackets,
draw_mesh_selection_overlays and draw_box_selection_preview (modeler/viewport.rs:1782-2247).

Without a GPU: ref_mesh_overlay restates the three Rust functions loop for loop (Python lists, a real set for drawn_edges, np.float32
scalars).  Hand cases with the expected records written out; the numpy mirror (rasterizer.mesh_overlay_records) and the device header
compiled for the host (tests/cpp/overlay_host.cpp over csrc/b32_overlay_body.h) equal the restatement -- the sequence of records that draw,
per section -- on obj-warrior (unposed and posed), asset3-part0-game, the order mesh and random meshes; a build with FMA contraction does
not; a census keeps the comparisons from passing on nothing.  On the GPU: the stage tap equals the mirror record for record, frames equal
the CPU composition byte for byte, and the overlay of a posed slot equals the host path with no read-back."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile
import atexit

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi
from bonnie32_amd import rasterizer as RM
from bonnie32_amd.mirrors.screen import _project_f32
from tests.test_lines import ROOT, _upload_zbuffer
from tests.test_prims import _as_i32, np_prims
from tests.test_gizmos import cpu_records
from tests.test_world import IDENTITY_CAM, QNAN, _cam_f32, look_at, noop_records, ref_world_to_screen_with_ortho
from tests.test_pick import UNIT_ORTHO
from tests.test_hover import hover_scene, order_mesh

f32 = np.float32
NONE = 0xFFFFFFFF
LIM = 1 << 30
SECTIONS = ("brackets", "edges", "dots", "hover", "selected", "preview")
BITS = dict(brackets=abi.OVERLAY_BRACKETS, edges=abi.OVERLAY_EDGES, dots=abi.OVERLAY_DOTS, hover=abi.OVERLAY_HOVER, selected=abi.OVERLAY_SELECTED,
            preview=abi.OVERLAY_PREVIEW)
MO = RM.MeshOverlay


# ================================================================== the literal restatement
def _inc(v):                                                   # `as i32 + 1` in a release build: wraps
    return ((int(v) + 1 + (1 << 31)) % (1 << 32)) - (1 << 31)


def _rmin(a, b):                                               # f32::min: a NaN is ignored
    return b if a != a else (a if b != b else (b if b < a else a))


def _rmax(a, b):
    return b if a != a else (a if b != b else (b if b > a else a))


class Recorder:
    """The Framebuffer calls of one section, as the records that draw: a call whose extent or centre reaches 2^30 is left out (the rule of
    b32_draw_prims that k_world_project applies on the device), a NaN depth is stored as 0x7FC00000."""

    def __init__(self):
        self.recs = []

    def _put(self, kind, x0, y0, x1, y1, z0, z1, size, color, alpha):
        r = np.zeros(1, abi.PRIM_DTYPE)
        r["x0"], r["y0"], r["x1"], r["y1"], r["size"] = x0, y0, x1, y1, size
        r["z0"], r["z1"] = (QNAN if z0 != z0 else z0), (QNAN if z1 != z1 else z1)
        r["r"], r["g"], r["b"], r["blend"], r["kind"], r["alpha"] = color[0], color[1], color[2], abi.OPAQUE, kind, alpha
        self.recs.append(r)

    def _line(self, kind, x0, y0, x1, y1, z0, z1, color, alpha=255):
        if abs(x1 - x0) >= LIM or abs(y1 - y0) >= LIM:
            return
        self._put(kind, x0, y0, x1, y1, z0, z1, 0, color, alpha)

    def draw_line(self, x0, y0, x1, y1, color):
        self._line(abi.LINE_2D, x0, y0, x1, y1, f32(0.0), f32(0.0), color)

    def draw_line_3d(self, x0, y0, z0, x1, y1, z1, color):
        self._line(abi.LINE_3D, x0, y0, x1, y1, z0, z1, color)

    def draw_line_3d_alpha(self, x0, y0, z0, x1, y1, z1, color, alpha):
        self._line(abi.LINE_3D_ALPHA, x0, y0, x1, y1, z0, z1, color, alpha)

    def _circle(self, kind, cx, cy, radius, color, alpha=255):
        if abs(cx) >= LIM or abs(cy) >= LIM:
            return
        self._put(kind, cx, cy, 0, 0, f32(0.0), f32(0.0), radius, color, alpha)

    def draw_circle(self, cx, cy, radius, color):
        self._circle(abi.PRIM_CIRCLE, cx, cy, radius, color)

    def draw_circle_alpha(self, cx, cy, radius, color, alpha):
        self._circle(abi.PRIM_CIRCLE_ALPHA, cx, cy, radius, color, alpha)


def ref_mesh_overlay(positions, polygons, o, selected, camera, w, h, ortho=None):
    """draw_selected_object_brackets, draw_mesh_selection_overlays and draw_box_selection_preview for the sections of `o` (a MeshOverlay):
    {section: the records that draw, in call order}.  positions: the posed positions (world_vertices)."""
    with np.errstate(all="ignore"):
        return _ref_mesh_overlay(positions, polygons, o, selected, camera, w, h, ortho)


def _ref_mesh_overlay(positions, polygons, o, selected, camera, w, h, ortho):
    cam = _cam_f32(camera)
    verts = [tuple(f32(c) for c in p) for p in np.asarray(positions, f32).reshape(-1, 3)]
    faces = [list(p) for p in polygons]
    fbs = {s: Recorder() for s in SECTIONS}

    def get_pos(idx):
        return verts[idx] if idx < len(verts) else None

    def w2s(p):                                                # world_to_screen_with_ortho[_depth]: (sx, sy, z) or None
        return ref_world_to_screen_with_ortho(p, cam, w, h, ortho)

    def edges_of(face):                                        # Face::edges, mesh_editor.rs:92-95
        n = len(face)
        return [(face[i], face[(i + 1) % n]) for i in range(n)]

    def add(a, b):
        return (a[0] + b[0], a[1] + b[1], a[2] + b[2])

    def scale(a, s):
        return (a[0] * s, a[1] * s, a[2] * s)

    ZERO = (f32(0.0), f32(0.0), f32(0.0))

    # ---- draw_selected_object_brackets, :1782-1884
    if o.sections & abi.OVERLAY_BRACKETS and len(verts):
        fb = fbs["brackets"]
        mn = [np.finfo(f32).max] * 3
        mx = [np.finfo(f32).min] * 3
        for pos in verts:
            for c in range(3):
                mn[c] = _rmin(mn[c], pos[c])
                mx[c] = _rmax(mx[c], pos[c])
        margin = f32(4.0)
        for c in range(3):
            mn[c] = mn[c] - margin
            mx[c] = mx[c] + margin
        size = (mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2])
        bracket_len = _rmin(_rmin(size[0], size[1]), size[2]) * f32(0.25)
        color = (0, 200, 230)
        corners = [(mn[0], mn[1], mn[2]), (mx[0], mn[1], mn[2]), (mx[0], mn[1], mx[2]), (mn[0], mn[1], mx[2]),
                   (mn[0], mx[1], mn[2]), (mx[0], mx[1], mn[2]), (mx[0], mx[1], mx[2]), (mn[0], mx[1], mx[2])]
        dirs = [(0, [(1, 0, 0), (0, 1, 0), (0, 0, 1)]), (1, [(-1, 0, 0), (0, 1, 0), (0, 0, 1)]), (2, [(-1, 0, 0), (0, 1, 0), (0, 0, -1)]),
                (3, [(1, 0, 0), (0, 1, 0), (0, 0, -1)]), (4, [(1, 0, 0), (0, -1, 0), (0, 0, 1)]), (5, [(-1, 0, 0), (0, -1, 0), (0, 0, 1)]),
                (6, [(-1, 0, 0), (0, -1, 0), (0, 0, -1)]), (7, [(1, 0, 0), (0, -1, 0), (0, 0, -1)])]
        for corner_idx, edge_dirs in dirs:
            corner = corners[corner_idx]
            for d in edge_dirs:
                d = tuple(f32(float(x)) for x in d)            # (Vec3::new(0.0, ..): positive zeros)
                end = (corner[0] + d[0] * bracket_len, corner[1] + d[1] * bracket_len, corner[2] + d[2] * bracket_len)
                a, b = w2s(corner), w2s(end)
                if a is not None and b is not None:
                    fb.draw_line_3d(_as_i32(a[0]), _as_i32(a[1]), a[2], _as_i32(b[0]), _as_i32(b[1]), b[2], color)

    # ---- draw_mesh_selection_overlays, :1890-2105
    hover_color, select_color, edge_overlay_color = (255, 200, 150), (100, 180, 255), (80, 80, 80)
    if o.sections & abi.OVERLAY_EDGES:                         # (with DOTS: `!wireframe_overlay`, :1923)
        fb = fbs["edges"]
        for face in faces:
            for v0_idx, v1_idx in edges_of(face):
                p0, p1 = get_pos(v0_idx), get_pos(v1_idx)
                if p0 is not None and p1 is not None:
                    a, b = w2s(p0), w2s(p1)
                    if a is not None and b is not None:
                        fb.draw_line_3d_alpha(_as_i32(a[0]), _as_i32(a[1]), a[2], _as_i32(b[0]), _as_i32(b[1]), b[2], edge_overlay_color, 191)
    if o.sections & abi.OVERLAY_DOTS:
        fb = fbs["dots"]
        vertex_overlay_color = (40, 40, 50)
        for idx in range(len(verts)):
            pos = get_pos(idx)
            if pos is not None:
                s = w2s(pos)
                if s is not None:
                    fb.draw_circle_alpha(_as_i32(s[0]), _as_i32(s[1]), 3, vertex_overlay_color, 140)
    if o.sections & abi.OVERLAY_HOVER:
        fb = fbs["hover"]
        if o.hover_vertex != NONE:
            pos = get_pos(o.hover_vertex)
            if pos is not None:
                s = w2s(pos)
                if s is not None:
                    fb.draw_circle(_as_i32(s[0]), _as_i32(s[1]), 5, hover_color)
        if o.hover_edge != (NONE, NONE):
            p0, p1 = get_pos(o.hover_edge[0]), get_pos(o.hover_edge[1])
            if p0 is not None and p1 is not None:
                a, b = w2s(p0), w2s(p1)
                if a is not None and b is not None:
                    fb.draw_line(_as_i32(a[0]), _as_i32(a[1]), _as_i32(b[0]), _as_i32(b[1]), hover_color)
                    fb.draw_line(_inc(_as_i32(a[0])), _as_i32(a[1]), _inc(_as_i32(b[0])), _as_i32(b[1]), hover_color)
                    fb.draw_line(_as_i32(a[0]), _inc(_as_i32(a[1])), _as_i32(b[0]), _inc(_as_i32(b[1])), hover_color)
        if o.hover_face != NONE and o.hover_face < len(faces):
            face = faces[o.hover_face]
            screen_positions = [s for s in (w2s(p) for p in (get_pos(vi) for vi in face) if p is not None) if s is not None]
            n = len(screen_positions)
            if n >= 3:
                for i in range(n):
                    a, b = screen_positions[i], screen_positions[(i + 1) % n]
                    fb.draw_line(_as_i32(a[0]), _as_i32(a[1]), _as_i32(b[0]), _as_i32(b[1]), hover_color)
                if n >= 4:
                    a, b = screen_positions[0], screen_positions[2]
                    fb.draw_line(_as_i32(a[0]), _as_i32(a[1]), _as_i32(b[0]), _as_i32(b[1]), hover_color)
    if o.sections & abi.OVERLAY_SELECTED:
        fb = fbs["selected"]
        sel = [int(x) for x in (selected if selected is not None else [])]
        if o.select_kind == abi.SELECT_VERTICES:
            for idx in sel:
                pos = get_pos(idx)
                if pos is not None:
                    s = w2s(pos)
                    if s is not None:
                        fb.draw_circle(_as_i32(s[0]), _as_i32(s[1]), 4, select_color)
        if o.select_kind == abi.SELECT_EDGES:
            for v0_idx, v1_idx in zip(sel[0::2], sel[1::2]):
                p0, p1 = get_pos(v0_idx), get_pos(v1_idx)
                if p0 is not None and p1 is not None:
                    a, b = w2s(p0), w2s(p1)
                    if a is not None and b is not None:
                        fb.draw_line(_as_i32(a[0]), _as_i32(a[1]), _as_i32(b[0]), _as_i32(b[1]), select_color)
                        fb.draw_line(_inc(_as_i32(a[0])), _as_i32(a[1]), _inc(_as_i32(b[0])), _as_i32(b[1]), select_color)
                        fb.draw_circle(_as_i32(a[0]), _as_i32(a[1]), 3, select_color)
                        fb.draw_circle(_as_i32(b[0]), _as_i32(b[1]), 3, select_color)
        if o.select_kind == abi.SELECT_POLYGONS:
            for face_idx in sel:
                if face_idx < len(faces):
                    face = faces[face_idx]
                    world_positions = [p for p in (get_pos(vi) for vi in face) if p is not None]
                    screen_positions = [s for s in (w2s(p) for p in world_positions) if s is not None]
                    n = len(screen_positions)
                    if n >= 3:
                        for i in range(n):
                            a, b = screen_positions[i], screen_positions[(i + 1) % n]
                            fb.draw_line(_as_i32(a[0]), _as_i32(a[1]), _as_i32(b[0]), _as_i32(b[1]), select_color)
                            fb.draw_line(_inc(_as_i32(a[0])), _as_i32(a[1]), _inc(_as_i32(b[0])), _as_i32(b[1]), select_color)
                        acc = ZERO
                        for p in world_positions:
                            acc = add(acc, p)
                        center = scale(acc, f32(1.0) / f32(n))
                        c = w2s(center)
                        if c is not None:
                            fb.draw_circle(_as_i32(c[0]), _as_i32(c[1]), 4, select_color)

    # ---- draw_box_selection_preview, :2108-2247
    if o.sections & abi.OVERLAY_PREVIEW:
        fb = fbs["preview"]
        fb_x0, fb_y0, fb_x1, fb_y1 = (f32(v) for v in o.rect)
        preview_color = (255, 220, 100)
        if o.preview_mode == abi.PREVIEW_VERTEX:
            for idx in range(len(verts)):
                pos = get_pos(idx)
                if pos is not None:
                    s = w2s(pos)
                    if s is not None:
                        sx, sy = s[0], s[1]
                        if sx >= fb_x0 and sx <= fb_x1 and sy >= fb_y0 and sy <= fb_y1:
                            fb.draw_circle(_as_i32(sx), _as_i32(sy), 6, preview_color)
        elif o.preview_mode == abi.PREVIEW_EDGE:
            drawn_edges = set()
            for face in faces:
                for v0_idx, v1_idx in edges_of(face):
                    edge = (min(v0_idx, v1_idx), max(v0_idx, v1_idx))
                    if edge in drawn_edges:
                        continue
                    p0, p1 = get_pos(v0_idx), get_pos(v1_idx)
                    if p0 is not None and p1 is not None:
                        a, b = w2s(p0), w2s(p1)
                        if a is not None and b is not None:
                            mid_x = (a[0] + b[0]) / f32(2.0)
                            mid_y = (a[1] + b[1]) / f32(2.0)
                            if mid_x >= fb_x0 and mid_x <= fb_x1 and mid_y >= fb_y0 and mid_y <= fb_y1:
                                fb.draw_line(_as_i32(a[0]), _as_i32(a[1]), _as_i32(b[0]), _as_i32(b[1]), preview_color)
                                fb.draw_line(_inc(_as_i32(a[0])), _as_i32(a[1]), _inc(_as_i32(b[0])), _as_i32(b[1]), preview_color)
                                drawn_edges.add(edge)
        else:
            for face in faces:
                world_positions = [p for p in (get_pos(vi) for vi in face) if p is not None]
                if world_positions:
                    acc = ZERO
                    for p in world_positions:
                        acc = add(acc, p)
                    center = scale(acc, f32(1.0) / f32(len(world_positions)))
                    c = w2s(center)
                    if c is not None:
                        cx, cy = c[0], c[1]
                        if cx >= fb_x0 and cx <= fb_x1 and cy >= fb_y0 and cy <= fb_y1:
                            screen_positions = [s for s in (w2s(p) for p in world_positions) if s is not None]
                            n = len(screen_positions)
                            if n >= 3:
                                for i in range(n):
                                    a, b = screen_positions[i], screen_positions[(i + 1) % n]
                                    fb.draw_line(_as_i32(a[0]), _as_i32(a[1]), _as_i32(b[0]), _as_i32(b[1]), preview_color)
                                fb.draw_circle(_as_i32(cx), _as_i32(cy), 4, preview_color)
    return {s: (np.concatenate(fbs[s].recs) if fbs[s].recs else np.zeros(0, abi.PRIM_DTYPE)) for s in SECTIONS}


# ================================================================== comparing
def drawing(recs):
    """The records that draw: everything but the no-op (a circle of radius -1)."""
    return recs[~((recs["kind"] == abi.PRIM_CIRCLE) & (recs["size"] == -1))]


def by_section(recs, lay):
    """A device-layout record array cut into the six sections (lay: mesh_overlay_layout), each as its records that draw."""
    cuts = [lay["brackets"], lay["edges"], lay["dots"], lay["hover_vertex"], lay["selected"], lay["preview"], lay["total"]]
    return {s: drawing(recs[cuts[i]:cuts[i + 1]]) for i, s in enumerate(SECTIONS)}


def slots_of(lay):
    cuts = [lay["brackets"], lay["edges"], lay["dots"], lay["hover_vertex"], lay["selected"], lay["preview"], lay["total"]]
    return {s: cuts[i + 1] - cuts[i] for i, s in enumerate(SECTIONS)}


def assert_equals_ref(recs, lay, want, what=""):
    got = by_section(recs, lay)
    for s in SECTIONS:
        assert len(got[s]) == len(want[s]) and got[s].tobytes() == want[s].tobytes(), \
            f"{what} section {s}: {len(got[s])} records against {len(want[s])}; first difference at {_first_diff(got[s], want[s])}"


def _first_diff(a, b):
    for i in range(min(len(a), len(b))):
        if a[i].tobytes() != b[i].tobytes():
            return i, a[i], b[i]
    return min(len(a), len(b))


def P(kind, x0, y0, x1=0, y1=0, rgb=(0, 0, 0), size=0, alpha=255, z0=0.0, z1=0.0):
    r = np.zeros(1, abi.PRIM_DTYPE)
    r["x0"], r["y0"], r["x1"], r["y1"], r["size"], r["z0"], r["z1"] = x0, y0, x1, y1, size, z0, z1
    r["r"], r["g"], r["b"], r["kind"], r["alpha"] = rgb[0], rgb[1], rgb[2], kind, alpha
    return r


def cat(recs):
    return np.concatenate(recs) if len(recs) else np.zeros(0, abi.PRIM_DTYPE)


HOVER_C, SELECT_C, PREVIEW_C, EDGE_C, DOT_C, BRACKET_C = (255, 200, 150), (100, 180, 255), (255, 220, 100), (80, 80, 80), (40, 40, 50), (0, 200, 230)


def both(positions, polygons, o, selected, camera, w, h, ortho=None):
    """(restatement, mirror cut into sections) -- the mirror must equal the restatement, then either serves as `the answer`."""
    top = RM.Topology.from_polygons(polygons)
    want = ref_mesh_overlay(positions, polygons, o, selected, camera, w, h, ortho)
    recs = RM.mesh_overlay_records(np.asarray(positions, f32).reshape(-1, 3), top, o, selected, camera, w, h, ortho)
    lay = RM.mesh_overlay_layout(top, len(np.asarray(positions, f32).reshape(-1, 3)), o, selected)
    assert len(recs) == lay["total"] == RM.mesh_overlay_record_count(top, len(np.asarray(positions).reshape(-1, 3)), o, selected)
    assert_equals_ref(recs, lay, want)
    return want


# ================================================================== hand cases: one mesh of 16 vertices at 64x48
HW, HH = 64, 48
# screen positions under the identity camera and UNIT_ORTHO (a vertex (x, y, z) lands at (x + 32, 24 - y), depth z)
HAND_SCREEN = {0: (10, 10), 1: (20, 8), 2: (26, 16), 3: (18, 24), 4: (8, 20),           # a pentagon
               5: (30, 10), 6: (40, 10), 7: (40, 20), 8: (30, 20),                      # a quad
               9: (45, 30), 10: (55, 30), 11: (50, 40),                                 # a triangle
               12: (5, 40), 13: (15, 40), 15: (60, 5)}                                  # 14: a NaN position
HAND_POLYS = [[0, 1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11], [12, 13], [12], [], [9, 10, 16],
              [6, 5, 15],                                      # shares the edge (5, 6) with the quad, the other way round
              [5, 6, 14]]                                      # shares it the same way round; 14 is the NaN vertex


def hand_mesh():
    pos = np.zeros((16, 3), f32)
    for i, (sx, sy) in HAND_SCREEN.items():
        pos[i] = (sx - 32.0, 24.0 - sy, 5.0)
    pos[14] = (np.nan, 1.0, 5.0)
    return pos


def S(i):                                                      # where vertex i lands, as cast (a NaN x makes every camera coordinate NaN: 0)
    return (0, 0) if i == 14 else HAND_SCREEN[i]


def Z(i):                                                      # its depth (a NaN is stored as 0x7FC00000)
    return QNAN if i == 14 else 5.0


def test_hand_edges_dots_and_brackets():
    pos = hand_mesh()
    o = MO(abi.OVERLAY_EDGES | abi.OVERLAY_DOTS | abi.OVERLAY_BRACKETS)
    got = both(pos, HAND_POLYS, o, None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    # every half-edge in loop order, duplicates included; n = 2 gives both directions, n = 1 a point, an index >= nv nothing
    half = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (5, 6), (6, 7), (7, 8), (8, 5), (9, 10), (10, 11), (11, 9), (12, 13), (13, 12), (12, 12),
            (9, 10), (6, 5), (5, 15), (15, 6), (5, 6), (6, 14), (14, 5)]
    want = cat([P(abi.LINE_3D_ALPHA, *S(a), *S(b), rgb=EDGE_C, alpha=191, z0=Z(a), z1=Z(b)) for a, b in half])
    assert got["edges"].tobytes() == want.tobytes()
    # the orthographic projection never answers None: the NaN vertex is a dot at (0, 0)
    want = cat([P(abi.PRIM_CIRCLE_ALPHA, *S(i), rgb=DOT_C, size=3, alpha=140) for i in range(16)])
    assert got["dots"].tobytes() == want.tobytes()
    # the bounds ignore the NaN: x -27 .. 28, y -16 .. 19, z 5 .. 5; margin 4; bracket_len = min(63, 43, 8) * 0.25 = 2
    mn, mx = (-31.0, -20.0, 1.0), (32.0, 23.0, 9.0)
    corners = [(mn[0], mn[1], mn[2]), (mx[0], mn[1], mn[2]), (mx[0], mn[1], mx[2]), (mn[0], mn[1], mx[2]),
               (mn[0], mx[1], mn[2]), (mx[0], mx[1], mn[2]), (mx[0], mx[1], mx[2]), (mn[0], mx[1], mx[2])]
    recs = []
    for ci, c in enumerate(corners):
        sign = (1 if c[0] == mn[0] else -1, 1 if c[1] == mn[1] else -1, 1 if c[2] == mn[2] else -1)
        for d in range(3):
            e = list(c); e[d] += 2.0 * sign[d]
            recs.append(P(abi.LINE_3D, int(c[0] + 32), int(24 - c[1]), int(e[0] + 32), int(24 - e[1]), rgb=BRACKET_C, z0=c[2], z1=e[2]))
    assert got["brackets"].tobytes() == cat(recs).tobytes() and len(recs) == 24


def test_hand_hover():
    pos = hand_mesh()
    line = lambda a, b, dx=0, dy=0: P(abi.LINE_2D, S(a)[0] + dx, S(a)[1] + dy, S(b)[0] + dx, S(b)[1] + dy, rgb=HOVER_C)
    # a hovered quad gets its diagonal [0] -> [2], a hovered triangle does not; a pentagon gets [0] -> [2] too
    for face, want in ((1, [line(5, 6), line(6, 7), line(7, 8), line(8, 5), line(5, 7)]), (2, [line(9, 10), line(10, 11), line(11, 9)]),
                       (0, [line(0, 1), line(1, 2), line(2, 3), line(3, 4), line(4, 0), line(0, 2)]),
                       (3, []), (4, []), (5, []), (6, []),     # 2-gon, 1-gon, empty, two vertices left of (9, 10, 16)
                       (9, []), (NONE - 1, [])):               # mesh.faces.get(..) == None
        got = both(pos, HAND_POLYS, MO(abi.OVERLAY_HOVER, hover_face=face), None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
        assert got["hover"].tobytes() == cat(want).tobytes(), face
    # vertex, edge and face together, in that order; the edge as three lines: as cast, + 1 on both x, + 1 on both y
    got = both(pos, HAND_POLYS, MO(abi.OVERLAY_HOVER, hover_vertex=3, hover_edge=(6, 5), hover_face=2), None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    want = [P(abi.PRIM_CIRCLE, 18, 24, rgb=HOVER_C, size=5), line(6, 5), line(6, 5, dx=1), line(6, 5, dy=1), line(9, 10), line(10, 11), line(11, 9)]
    assert got["hover"].tobytes() == cat(want).tobytes()
    # indices out of range: get_pos(..) == None
    got = both(pos, HAND_POLYS, MO(abi.OVERLAY_HOVER, hover_vertex=16, hover_edge=(5, 16)), None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    assert len(got["hover"]) == 0
    got = both(pos, HAND_POLYS, MO(abi.OVERLAY_HOVER, hover_edge=(NONE, 5)), None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    assert len(got["hover"]) == 0


def test_hand_selected():
    pos = hand_mesh()
    line = lambda a, b, dx=0: P(abi.LINE_2D, S(a)[0] + dx, S(a)[1], S(b)[0] + dx, S(b)[1], rgb=SELECT_C)
    dot = lambda i, r: P(abi.PRIM_CIRCLE, *S(i), rgb=SELECT_C, size=r)
    got = both(pos, HAND_POLYS, MO(abi.OVERLAY_SELECTED, select_kind=abi.SELECT_VERTICES), [0, 16, 14, 0, NONE], IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    assert got["selected"].tobytes() == cat([dot(0, 4), dot(14, 4), dot(0, 4)]).tobytes()
    # pairs as given, not normalised: (6, 5) runs from 6 to 5
    got = both(pos, HAND_POLYS, MO(abi.OVERLAY_SELECTED, select_kind=abi.SELECT_EDGES), [6, 5, 5, 16, 12, 12], IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    want = [line(6, 5), line(6, 5, 1), dot(6, 3), dot(5, 3), line(12, 12), line(12, 12, 1), dot(12, 3), dot(12, 3)]
    assert got["selected"].tobytes() == cat(want).tobytes()
    # polygons: every outline edge followed by its + 1 x twin, then the centre; the quad's centre (35, 15), the triangle's (50, 33.33)
    got = both(pos, HAND_POLYS, MO(abi.OVERLAY_SELECTED, select_kind=abi.SELECT_POLYGONS), [1, 3, 9, 2, 4, 5, 6], IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    want = []
    for a, b in ((5, 6), (6, 7), (7, 8), (8, 5)):
        want += [line(a, b), line(a, b, 1)]
    want.append(P(abi.PRIM_CIRCLE, 35, 15, rgb=SELECT_C, size=4))
    for a, b in ((9, 10), (10, 11), (11, 9)):
        want += [line(a, b), line(a, b, 1)]
    want.append(P(abi.PRIM_CIRCLE, 50, 33, rgb=SELECT_C, size=4))
    assert got["selected"].tobytes() == cat(want).tobytes()


def _near_quad():
    """A quad in front of the identity camera (perspective, 64x48: sx = x * 4 / (z + 5) * 18 + 32): three vertices at z = 5 and vertex 3
    behind the near plane."""
    return np.array([(-2.0, -1.0, 5.0), (2.0, -1.0, 5.0), (2.0, 2.0, 5.0), (-8.0, 2.0, 0.05)], f32)


def test_hand_vertex_behind_the_near_plane():
    """The selected quad's outline closes over the 3 vertices that project and its centre is the sum of FOUR positions times 1 / 3
    (:2088 divides by screen_positions.len()); the preview divides by 4."""
    pos, polys = _near_quad(), [[0, 1, 2, 3]]
    cam = _cam_f32(IDENTITY_CAM)
    s = [ref_world_to_screen_with_ortho(tuple(p), cam, HW, HH, None) for p in pos]
    assert s[3] is None and all(x is not None for x in s[:3])
    I = [(_as_i32(x[0]), _as_i32(x[1])) for x in s[:3]]
    assert I == [(17, 16), (46, 16), (46, 38)]                                          # 32 -+ 0.8 * 18, 24 - 0.4 * 18, 24 + 0.8 * 18
    acc = (f32(0.0), f32(0.0), f32(0.0))
    for p in pos:
        acc = (acc[0] + p[0], acc[1] + p[1], acc[2] + p[2])
    third, quarter = f32(1.0) / f32(3.0), f32(1.0) / f32(4.0)
    c3 = ref_world_to_screen_with_ortho((acc[0] * third, acc[1] * third, acc[2] * third), cam, HW, HH, None)
    c4 = ref_world_to_screen_with_ortho((acc[0] * quarter, acc[1] * quarter, acc[2] * quarter), cam, HW, HH, None)
    C3, C4 = (_as_i32(c3[0]), _as_i32(c3[1])), (_as_i32(c4[0]), _as_i32(c4[1]))
    assert C3 == (17, 28) and C4 == (19, 28)                                            # x: -2 * 4 / 10.0167 * 18 + 32 = 17.6 against -1.5 * 4 / 8.7625 * 18 + 32 = 19.7
    got = both(pos, polys, MO(abi.OVERLAY_SELECTED | abi.OVERLAY_PREVIEW, select_kind=abi.SELECT_POLYGONS, preview_mode=abi.PREVIEW_FACE, rect=(0, 0, 64, 48)),
               [0], IDENTITY_CAM, HW, HH)
    want = []
    for a, b in ((0, 1), (1, 2), (2, 0)):
        want += [P(abi.LINE_2D, *I[a], *I[b], rgb=SELECT_C), P(abi.LINE_2D, I[a][0] + 1, I[a][1], I[b][0] + 1, I[b][1], rgb=SELECT_C)]
    want.append(P(abi.PRIM_CIRCLE, *C3, rgb=SELECT_C, size=4))
    assert got["selected"].tobytes() == cat(want).tobytes()
    want = [P(abi.LINE_2D, *I[a], *I[b], rgb=PREVIEW_C) for a, b in ((0, 1), (1, 2), (2, 0))] + [P(abi.PRIM_CIRCLE, *C4, rgb=PREVIEW_C, size=4)]
    assert got["preview"].tobytes() == cat(want).tobytes()
    # two projected vertices left: nothing, the centre included -- selected, hovered and previewed
    pos2 = pos.copy(); pos2[2, 2] = 0.0
    got = both(pos2, polys, MO(abi.OVERLAY_ALL & ~abi.OVERLAY_EDGES & ~abi.OVERLAY_DOTS & ~abi.OVERLAY_BRACKETS, hover_face=0, select_kind=abi.SELECT_POLYGONS,
                               preview_mode=abi.PREVIEW_FACE, rect=(0, 0, 64, 48)), [0], IDENTITY_CAM, HW, HH)
    assert len(got["selected"]) == 0 and len(got["hover"]) == 0 and len(got["preview"]) == 0


def test_hand_preview():
    pos = hand_mesh()
    rect = (25.0, 5.0, 45.0, 20.0)                             # inclusive: the quad's corners (30, 10) .. (40, 20) and (26, 16)
    dot = lambda x, y, r: P(abi.PRIM_CIRCLE, x, y, rgb=PREVIEW_C, size=r)
    got = both(pos, HAND_POLYS, MO(abi.OVERLAY_PREVIEW, preview_mode=abi.PREVIEW_VERTEX, rect=rect), None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    assert got["preview"].tobytes() == cat([dot(*S(i), 6) for i in (2, 5, 6, 7, 8)]).tobytes()     # (the NaN vertex fails every test)
    # edges: the first half-edge of every edge whose midpoint is inside, in ITS orientation: (5, 6) from the quad -- not (6, 5) from
    # polygon 7 nor the second (5, 6) of polygon 8; (8, 5) has its midpoint (30, 15) inside; (1, 2) at (23, 12) is outside, (2, 3) too
    line = lambda a, b, dx=0: P(abi.LINE_2D, S(a)[0] + dx, S(a)[1], S(b)[0] + dx, S(b)[1], rgb=PREVIEW_C)
    got = both(pos, HAND_POLYS, MO(abi.OVERLAY_PREVIEW, preview_mode=abi.PREVIEW_EDGE, rect=rect), None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    want = []
    for a, b in ((5, 6), (6, 7), (7, 8), (8, 5), (5, 15)):    # ((5, 15) of polygon 7: its midpoint (45, 7.5) lies on the border)
        want += [line(a, b), line(a, b, 1)]
    assert got["preview"].tobytes() == cat(want).tobytes()
    # the other orientation first: polygon 7 moved in front of the quad draws (6, 5)
    polys = [HAND_POLYS[7]] + HAND_POLYS[:7] + HAND_POLYS[8:]
    got = both(pos, polys, MO(abi.OVERLAY_PREVIEW, preview_mode=abi.PREVIEW_EDGE, rect=(25.0, 5.0, 45.0, 12.0)), None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    assert got["preview"].tobytes() == cat([line(6, 5), line(6, 5, 1), line(5, 15), line(5, 15, 1)]).tobytes()
    # faces: the quad's centre (35, 15) is inside; polygon 7's centre (43.33, 8.33) too; polygon 8 has a NaN centre; the pentagon's is outside
    got = both(pos, HAND_POLYS, MO(abi.OVERLAY_PREVIEW, preview_mode=abi.PREVIEW_FACE, rect=rect), None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    one = lambda a, b: P(abi.LINE_2D, *S(a), *S(b), rgb=PREVIEW_C)
    want = [one(5, 6), one(6, 7), one(7, 8), one(8, 5), dot(35, 15, 4), one(6, 5), one(5, 15), one(15, 6), dot(43, 8, 4)]
    assert got["preview"].tobytes() == cat(want).tobytes()
    # polygon 6 = (9, 10, 16): count = 2 vertices exist, the centre (50, 30) is inside this rectangle, but only 2 project: nothing
    got = both(pos, HAND_POLYS[6:7], MO(abi.OVERLAY_PREVIEW, preview_mode=abi.PREVIEW_FACE, rect=(0, 0, 64, 48)), None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    assert len(got["preview"]) == 0


def test_hand_nan_mesh_and_saturating_casts():
    # an all-NaN mesh: min stays f32::MAX and max f32::MIN, the corners cast to +-2^31 and the extent rule leaves nothing
    pos = np.full((5, 3), np.nan, f32)
    for ortho in (UNIT_ORTHO, None):
        got = both(pos, [[0, 1, 2]], MO(abi.OVERLAY_BRACKETS), None, IDENTITY_CAM, HW, HH, ortho)
        assert len(got["brackets"]) == 0
    # a cast that saturates: sx = 3e9 + 32 -> i32::MAX, and `+ 1` wraps to i32::MIN
    pos = np.array([(3e9, 4.0, 5.0), (3e9, -6.0, 5.0), (0.0, 0.0, 5.0)], f32)
    got = both(pos, [[0, 1, 2]], MO(abi.OVERLAY_HOVER, hover_edge=(0, 1)), None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    IMAX, IMIN = 2147483647, -2147483648
    want = [P(abi.LINE_2D, IMAX, 20, IMAX, 30, rgb=HOVER_C), P(abi.LINE_2D, IMIN, 20, IMIN, 30, rgb=HOVER_C), P(abi.LINE_2D, IMAX, 21, IMAX, 31, rgb=HOVER_C)]
    assert got["hover"].tobytes() == cat(want).tobytes()
    # ... and where only one end saturates the extent reaches 2^30: the line is left out, its twin wraps and is left out too; a circle there as well
    got = both(pos, [[0, 1, 2]], MO(abi.OVERLAY_HOVER | abi.OVERLAY_DOTS, hover_edge=(0, 2)), None, IDENTITY_CAM, HW, HH, UNIT_ORTHO)
    assert len(got["hover"]) == 0 and got["dots"].tobytes() == P(abi.PRIM_CIRCLE_ALPHA, 32, 24, rgb=DOT_C, size=3, alpha=140).tobytes()


def test_layout_and_pod_layout_match_c():
    """B32MeshOverlay is 48 bytes with the fields where the C header puts them (compiled with g++), and the record count is the length of
    the mirror's output for every combination of the hand mesh."""
    src = ('#include <cstdio>\n#include <cstddef>\n#include "b32raster.h"\nint main() { std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u\\n", sizeof(B32MeshOverlay),'
           ' offsetof(B32MeshOverlay, sections), offsetof(B32MeshOverlay, hover_vertex), offsetof(B32MeshOverlay, hover_edge_v1), offsetof(B32MeshOverlay, hover_face),'
           ' offsetof(B32MeshOverlay, select_kind), offsetof(B32MeshOverlay, n_selected), offsetof(B32MeshOverlay, preview_mode), offsetof(B32MeshOverlay, y1),'
           ' B32_OVERLAY_BRACKETS | B32_OVERLAY_EDGES | B32_OVERLAY_DOTS | B32_OVERLAY_HOVER | B32_OVERLAY_SELECTED, B32_OVERLAY_PREVIEW); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.cpp"), "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    F = abi.B32MeshOverlay
    assert [int(x) for x in out] == [C.sizeof(F), F.sections.offset, F.hover_vertex.offset, F.hover_edge_v1.offset, F.hover_face.offset, F.select_kind.offset,
                                     F.n_selected.offset, F.preview_mode.offset, F.y1.offset, 31, abi.OVERLAY_PREVIEW]
    assert C.sizeof(F) == 48
    o, sel = MO(63, hover_vertex=3, hover_edge=(1, 2), hover_face=4, select_kind=2, preview_mode=1, rect=(1, 2, 3, 4)).pack([7, 8, 9, 10])
    assert (o.sections, o.hover_vertex, o.hover_edge_v0, o.hover_edge_v1, o.hover_face, o.select_kind, o.n_selected, o.preview_mode, o.x0, o.y1) == \
        (63, 3, 1, 2, 4, 2, 2, 1, 1.0, 4.0) and sel.dtype == np.uint32 and len(sel) == 4
    pos, top = hand_mesh(), RM.Topology.from_polygons(HAND_POLYS)
    nh, npoly, ne = 24, 9, len({(min(a, b), max(a, b)) for p in HAND_POLYS for a, b in zip(p, p[1:] + p[:1])})
    assert RM.mesh_overlay_record_count(top, 16, MO(abi.OVERLAY_ALL, hover_vertex=1, hover_edge=(NONE, 3), hover_face=0, select_kind=3, preview_mode=2), [1, 77, 2, 5]) == \
        24 + nh + 16 + (1 + 3 + 6) + (9 + 7 + 1) + (nh + npoly)
    assert RM.mesh_overlay_record_count(top, 16, MO(abi.OVERLAY_PREVIEW, preview_mode=1)) == 2 * ne
    assert RM.mesh_overlay_record_count(top, 0, MO(abi.OVERLAY_BRACKETS | abi.OVERLAY_DOTS)) == 0
    assert RM.mesh_overlay_record_count(None, 16, MO(abi.OVERLAY_BRACKETS | abi.OVERLAY_DOTS | abi.OVERLAY_SELECTED, select_kind=2), [1, 2]) == 24 + 16 + 4
    for bad in (MO(64), MO(1, select_kind=4), MO(1, preview_mode=3)):
        with pytest.raises(ValueError):
            RM.mesh_overlay_record_count(top, 16, bad)
    with pytest.raises(ValueError):
        RM.mesh_overlay_record_count(None, 16, MO(abi.OVERLAY_EDGES))
    # the camera never moves a record: the same places under another camera
    for o_ in (MO(abi.OVERLAY_ALL, hover_face=1, select_kind=3, preview_mode=1, rect=(0, 0, 30, 30)),):
        a = RM.mesh_overlay_records(pos, top, o_, [0, 1], IDENTITY_CAM, HW, HH, UNIT_ORTHO)
        b = RM.mesh_overlay_records(pos, top, o_, [0, 1], look_at((3, 4, -50), (0, 0, 5)), HW, HH)
        assert len(a) == len(b) and not np.array_equal(a, b)


# ================================================================== the scenes
def _warrior_bones(t=3.0, s=1000.0):
    """A non-trivial bone table (tests/test_pose.py's frame t)."""
    return RM.pack_bones([RM.Bone.from_euler((0.06 * s * np.sin(0.7 * t), 0.03 * s, -0.04 * s * np.cos(0.4 * t)), (6.0 + 3.0 * t, 0.0, -5.0 + 2.0 * t)),
                          RM.Bone.from_euler((0.35 * s - 0.02 * s * t, -0.05 * s, 0.02 * s * t), (0.0004, 30.0, 0.0)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (-4.0 - 1.5 * t, 0.0, 3.0 + t)),
                          RM.Bone.from_euler((-0.3 * s + 0.01 * s * t, 0.02 * s * t, 0.05 * s), (2.0 * t, 0.0, 9.0)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))])


def _warrior_bone_of(n, seed=5):
    rng = np.random.default_rng(seed)
    bo = np.repeat(rng.integers(0, 8, (n + 7) // 8 + 1).astype(np.uint16), 8)[:n].copy()
    bo[bo == 7] = abi.BONE_NONE
    return bo


def _screen(pos, cam, w, h, ortho):
    with np.errstate(all="ignore"):
        sx, sy, _, some = _project_f32(pos[:, 0], pos[:, 1], pos[:, 2], cam, w, h, ortho)
    return sx, sy, some


def fit_ortho(pos, cam, w, h):
    """An orthographic view of `cam` that holds the whole mesh in 80 % of a w x h frame: (zoom, center_x, center_y)."""
    sx, sy, _ = _screen(pos, cam, w, h, (1.0, 0.0, 0.0))
    zoom = 0.8 * min(w / float(sx.max() - sx.min()), h / float(sy.max() - sy.min()))
    return (zoom, float((sx.max() + sx.min()) / 2 - w / 2), float(-((sy.max() + sy.min()) / 2 - h / 2)))


@functools.lru_cache(maxsize=None)
def overlay_case(name, posed=False, ortho=False):
    """(positions, polygons, topology, camera, w, h, ortho, rect): a golden scene with its merged-quad topology; the rectangle is the left
    part of the frame up to the median of the projected vertices, so that about half of the elements lie inside."""
    if name == "order":
        v, polys = order_mesh("nan_last")
        pos, cam, w, h, o = v["pos"].copy(), IDENTITY_CAM, 320, 240, UNIT_ORTHO
        top = RM.Topology.from_polygons(polys)
    else:
        sc, v, polys, top, _ = hover_scene(name)
        pos, cam, w, h = np.ascontiguousarray(v["pos"], f32), sc.camera, sc.width, sc.height
        if posed:
            pos = np.ascontiguousarray(RM.pose_vertices(v, _warrior_bone_of(len(v)), _warrior_bones())["pos"], f32)
        o = None
        if ortho:
            o = fit_ortho(pos, cam, w, h)
    sx, sy, some = _screen(pos, cam, w, h, o)
    rect = (-1e6, -1e6, float(np.median(sx[some])), 1e6)
    return pos, polys, top, cam, w, h, o, rect


def case_overlays(polys, nv, rect):
    """Every section bit alone, all together, the three select kinds and the three preview modes: (MeshOverlay, selected)."""
    quad = next(i for i, p in enumerate(polys) if len(p) == 4)
    he = [(a, b) for p in polys[:40] for a, b in zip(p, p[1:] + p[:1])]
    sel = {abi.SELECT_VERTICES: list(range(0, nv, 3)) + [nv, NONE], abi.SELECT_EDGES: [i for e in he for i in e] + [0, nv],
           abi.SELECT_POLYGONS: list(range(0, len(polys), 2)) + [len(polys), NONE]}
    hov = dict(hover_vertex=10 % nv, hover_edge=(polys[quad][1], polys[quad][0]), hover_face=quad)
    out = [(MO(bit, select_kind=abi.SELECT_POLYGONS, preview_mode=abi.PREVIEW_VERTEX, rect=rect, **hov), sel[abi.SELECT_POLYGONS]) for bit in (1, 2, 4, 8, 16, 32)]
    for kind in (abi.SELECT_VERTICES, abi.SELECT_EDGES, abi.SELECT_POLYGONS):
        out.append((MO(abi.OVERLAY_ALL, select_kind=kind, preview_mode=kind - 1, rect=rect, **hov), sel[kind]))
    return out


SCENE_CASES = [("obj-warrior", False, False), ("obj-warrior", False, True), ("obj-warrior", True, False), ("obj-warrior", True, True),
               ("asset3-part0-game", False, False), ("order", False, False)]


@pytest.mark.parametrize("name,posed,ortho", SCENE_CASES)
def test_mirror_equals_the_restatement(name, posed, ortho):
    """rasterizer.mesh_overlay_records == ref_mesh_overlay, the records that draw per section, and the census: on obj-warrior at least
    half of each section's places draw and the rectangle holds between a quarter and three quarters of the elements."""
    pos, polys, top, cam, w, h, o, rect = overlay_case(name, posed, ortho)
    nv = len(pos)
    ne = top.ne
    for ov, sel in case_overlays(polys, nv, rect):
        want = ref_mesh_overlay(pos, polys, ov, sel, cam, w, h, o)
        recs = RM.mesh_overlay_records(pos, top, ov, sel, cam, w, h, o)
        lay = RM.mesh_overlay_layout(top, nv, ov, sel)
        assert len(recs) == RM.mesh_overlay_record_count(top, nv, ov, sel) == lay["total"]
        assert_equals_ref(recs, lay, want, f"{name} sections={ov.sections} kind={ov.select_kind} mode={ov.preview_mode}")
        if name == "obj-warrior":
            slots = slots_of(lay)
            for s in SECTIONS[:5]:
                if ov.sections & BITS[s]:
                    assert slots[s] > 0 and 2 * len(want[s]) >= slots[s], (s, len(want[s]), slots[s])
            if ov.sections & abi.OVERLAY_PREVIEW:
                n_el, per = {0: (nv, 1), 1: (ne, 2), 2: (len(polys), None)}[ov.preview_mode]
                n_in = len(want["preview"]) // per if per else int((want["preview"]["kind"] == abi.PRIM_CIRCLE).sum())
                assert n_el / 4 <= n_in <= 3 * n_el / 4, (ov.preview_mode, n_in, n_el)
    if posed:                                                  # the pose moved the records
        ov, sel = case_overlays(polys, nv, rect)[-1]
        rest = overlay_case(name, False, ortho)[0]
        assert RM.mesh_overlay_records(rest, top, ov, sel, cam, w, h, o).tobytes() != RM.mesh_overlay_records(pos, top, ov, sel, cam, w, h, o).tobytes()


# ================================================================== the device header compiled for the host
HOST_FLAGS = {"off": ["-O1", "-ffp-contract=off"], "fused": ["-O2", "-ffp-contract=fast", "-mfma"],
              "sanitized": ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@functools.lru_cache(maxsize=None)
def _host_dir():
    d = tempfile.mkdtemp(prefix="b32_overlay_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def host_exe(mode):
    exe = os.path.join(_host_dir(), "overlay_host_" + mode)
    subprocess.run(["g++", "-std=c++17"] + HOST_FLAGS[mode] + ["-I", os.path.join(ROOT, "bonnie-32_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "overlay_host.cpp"),
                    "-o", exe], check=True)
    return exe


_host_calls = [0]


def host_overlay(pos, top, ov, sel, cam, w, h, ortho, mode="off"):
    """tests/cpp/overlay_host.cpp on one case: (records in the device's layout, the layout's nine numbers)."""
    _host_calls[0] += 1
    base = os.path.join(_host_dir(), f"case{_host_calls[0]}")
    o, s = ov.pack(sel)
    pos = np.ascontiguousarray(pos, f32).reshape(-1, 3)
    with open(base + ".in", "wb") as fh:
        fh.write(np.array([w, h, int(ortho is not None), len(pos), top.np, len(top.poly_verts), len(s)], np.uint32).tobytes())
        fh.write(bytes(o))
        c = cam.pack()
        fh.write(np.array(list(c.position) + list(c.basis_x) + list(c.basis_y) + list(c.basis_z), f32).tobytes())
        fh.write(np.array(ortho if ortho is not None else (0, 0, 0), f32).tobytes())
        fh.write(pos.tobytes()); fh.write(top.poly_start.tobytes()); fh.write(top.poly_verts.tobytes()); fh.write(s.tobytes())
    r = subprocess.run([host_exe(mode), base + ".in", base + ".out"], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    blob = open(base + ".out", "rb").read()
    lay = np.frombuffer(blob[:36], np.uint32)
    recs = np.frombuffer(blob[36:], abi.PRIM_DTYPE)
    assert len(recs) == lay[8]
    os.remove(base + ".in"); os.remove(base + ".out")
    return recs, lay


@functools.lru_cache(maxsize=None)
def random_mesh(seed, nv=1500, npoly=700):
    """Positions around the view of a look_at camera (a few behind it, a NaN, an infinity), polygons of 0 .. 8 positions with a few indices
    out of range."""
    rng = np.random.default_rng(seed)
    cam = look_at((30.0, 60.0, -250.0), (0.0, 10.0, 40.0))
    pos = (rng.normal(size=(nv, 3)) * (90.0, 70.0, 110.0) + (3.0, 11.0, 37.0)).astype(f32)
    pos[rng.integers(0, nv, 25)] += (0.0, 0.0, -400.0)         # behind the camera
    pos[7, 0] = np.nan; pos[11, 2] = np.inf
    polys = []
    for _ in range(npoly):
        n = int(rng.choice([0, 1, 2, 3, 3, 4, 4, 4, 5, 6, 7, 8]))
        base = int(rng.integers(0, nv))
        p = [int((base + k) % nv) if rng.random() < 0.6 else int(rng.integers(0, nv)) for k in rng.permutation(n)]
        if n and rng.random() < 0.03:
            p[int(rng.integers(0, n))] = nv + int(rng.integers(0, 3))
        polys.append(p)
    return pos, polys, RM.Topology.from_polygons(polys), cam


def host_cases():
    """(name, positions, polygons, topology, camera, w, h, ortho, MeshOverlay, selected)"""
    out = []
    for name, posed, ortho in SCENE_CASES:
        pos, polys, top, cam, w, h, o, rect = overlay_case(name, posed, ortho)
        for ov, sel in case_overlays(polys, len(pos), rect)[6:]:
            out.append((f"{name} posed={posed} ortho={ortho}", pos, polys, top, cam, w, h, o, ov, sel))
    for seed in (1, 2):
        pos, polys, top, cam = random_mesh(seed)
        for o in (None, (0.9, 3.0, -2.0)):
            sx, _, some = _screen(pos, cam, 320, 240, o)
            rect = (-1e6, -1e6, float(np.nanmedian(sx[some])), 1e6)
            for ov, sel in case_overlays(polys, len(pos), rect)[6:]:
                out.append((f"random {seed} ortho={o}", pos, polys, top, cam, 320, 240, o, ov, sel))
    pos, top = hand_mesh(), RM.Topology.from_polygons(HAND_POLYS)
    for ov, sel in case_overlays(HAND_POLYS, 16, (25.0, 5.0, 45.0, 20.0)):
        out.append(("hand", pos, HAND_POLYS, top, IDENTITY_CAM, HW, HH, UNIT_ORTHO, ov, sel))
    return out


def test_host_compile_of_the_device_header_equals_the_restatement():
    """csrc/b32_overlay_body.h built for the host (g++ -O1 -ffp-contract=off): the records that draw equal ref_mesh_overlay bit for bit per
    section, and the whole array -- places included -- equals the mirror's, on the scenes, the hand mesh and random meshes with polygons
    of up to 8 positions."""
    n_drawn = 0
    for name, pos, polys, top, cam, w, h, o, ov, sel in host_cases():
        recs, lay9 = host_overlay(pos, top, ov, sel, cam, w, h, o)
        lay = RM.mesh_overlay_layout(top, len(pos), ov, sel)
        assert [int(x) for x in lay9] == [lay[k] for k in ("brackets", "edges", "dots", "hover_vertex", "hover_edge", "hover_face", "selected", "preview", "total")], name
        assert_equals_ref(recs, lay, ref_mesh_overlay(pos, polys, ov, sel, cam, w, h, o), name)
        mirror = RM.mesh_overlay_records(pos, top, ov, sel, cam, w, h, o)
        assert recs.tobytes() == mirror.tobytes(), f"{name}: records {np.nonzero(recs != mirror)[0][:8]} differ from the mirror"
        n_drawn += len(drawing(recs))
    assert n_drawn > 20000


def test_a_fused_evaluation_differs():
    """The same program built with FMA contraction (g++ -O2 -ffp-contract=fast -mfma) gives other records on the random meshes: nothing
    contracted can pass the comparisons of this file."""
    n = 0
    for name, pos, polys, top, cam, w, h, o, ov, sel in host_cases():
        if not name.startswith("random"):
            continue
        a, _ = host_overlay(pos, top, ov, sel, cam, w, h, o, "off")
        b, _ = host_overlay(pos, top, ov, sel, cam, w, h, o, "fused")
        assert len(a) == len(b)
        n += int((a != b).sum())
    assert n >= 10, n


def test_host_program_under_the_sanitizers():
    """The stand-alone program once more with -fsanitize=address,undefined, run directly on the hand mesh, a scene and a random mesh:
    it ends clean and gives the same records."""
    cases = host_cases()
    picks = [c for c in cases if c[0] == "hand"][-3:] + [c for c in cases if c[0].startswith("random 1")][:3] + [c for c in cases if c[0].startswith("order")][-1:]
    for name, pos, polys, top, cam, w, h, o, ov, sel in picks:
        a, _ = host_overlay(pos, top, ov, sel, cam, w, h, o, "off")
        b, _ = host_overlay(pos, top, ov, sel, cam, w, h, o, "sanitized")
        assert a.tobytes() == b.tobytes(), name


def test_cpp_mirror_mesh_overlay_compiles():
    """host/rasterizer.hpp: b32::MeshOverlay and b32::draw_mesh_overlay compile (header-only over the C ABI)."""
    hpp_dir = os.path.join(ROOT, "bonnie-32_amd", "host")
    src = ('#include "rasterizer.hpp"\nvoid f(b32::Framebuffer& fb, b32::ResidentMesh& a, const b32::Camera& cam, const std::vector<b32::Face>& fc) {\n'
           ' b32::Topology top = b32::Topology::triangles(fb, fc);\n'
           ' b32::MeshOverlay o; o.sections = B32_OVERLAY_BRACKETS | B32_OVERLAY_EDGES | B32_OVERLAY_DOTS | B32_OVERLAY_HOVER | B32_OVERLAY_SELECTED;\n'
           ' o.hover = b32::hovered_element(b32::hover_mesh(fb, a, top, cam, b32::hover_params(1.0f, 2.0f)));\n'
           ' o.select_kind = 2; o.selected = { 0, 1, 1, 2 }; b32::draw_mesh_overlay(fb, a, &top, o, cam);\n'
           ' b32::MeshOverlay p; p.sections = B32_OVERLAY_PREVIEW; p.preview_mode = 0; p.x0 = 1; p.y0 = 2; p.x1 = 30; p.y1 = 40;\n'
           ' b32::draw_mesh_overlay(fb, a, nullptr, p, cam, b32::Vec3{ 1.0f, 0.0f, 0.0f }); (void)sizeof(B32MeshOverlay); (void)p.pack().n_selected; }\n'
           'int main() { (void)&f; return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", hpp_dir, "-I", os.path.join(ROOT, "include"),
                        os.path.join(d, "t.cpp")], check=True)


# ================================================================== GPU
def _slot(R, fb, vertices):
    """A detached resident scene with these vertices (one degenerate face: the overlay reads vertices only)."""
    return R.ResidentScene(fb, vertices, b32.make_faces(1), []).detach()


def _mesh_vertices(pos):
    v = b32.make_vertices(len(pos))
    v["pos"] = pos
    return v


@pytest.mark.gpu
def test_gpu_overlay_stage_tap(gpu_ctx):
    """b32_mesh_overlay_project_batch == the mirror, record for record with the no-ops in their places, on the hand mesh and obj-warrior
    (perspective and ortho) for every section alone and together; the C record count agrees."""
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(64, 48, gpu_ctx)
    cases = [("hand", hand_mesh(), HAND_POLYS, RM.Topology.from_polygons(HAND_POLYS), IDENTITY_CAM, HW, HH, UNIT_ORTHO, (25.0, 5.0, 45.0, 20.0)),
             ("near", _near_quad(), [[0, 1, 2, 3]], RM.Topology.from_polygons([[0, 1, 2, 3]]), IDENTITY_CAM, HW, HH, None, (0.0, 0.0, 64.0, 48.0))]
    for ortho in (False, True):
        pos, polys, top, cam, w, h, o, rect = overlay_case("obj-warrior", False, ortho)
        cases.append(("warrior", pos, polys, top, cam, w, h, o, rect))
    pos, polys, top, cam, w, h, o, rect = overlay_case("order")
    cases.append(("order", pos, polys, top, cam, w, h, o, rect))
    n = 0
    for name, pos, polys, top, cam, w, h, o, rect in cases:
        rs = _slot(R, fb, _mesh_vertices(pos))
        try:
            for ov, sel in case_overlays(polys, len(pos), rect):
                want = RM.mesh_overlay_records(pos, top, ov, sel, cam, w, h, o)
                got = fb.mesh_overlay_project_batch(rs, top, ov, cam, o, sel, w, h)
                assert len(got) == len(want) == gpu_ctx.mesh_overlay_record_count(top, len(pos), ov, sel)
                assert got.tobytes() == want.tobytes(), f"{name} sections={ov.sections}: records {np.nonzero(got != want)[0][:8]} differ"
                n += len(drawing(got))
        finally:
            rs.close()
    assert n > 5000
    for _, _, _, top, *_ in cases:
        top.close()


@functools.lru_cache(maxsize=None)
def _warrior_frame(w, h):
    """obj-warrior drawn in z-buffer mode by the oracle at w x h: (scene, pixels, z-buffer)."""
    from oracle import oracle as O
    import copy
    sc = hover_scene("obj-warrior")[0]
    st = copy.copy(sc.settings)
    st.use_zbuffer = True
    ofb = O.Framebuffer(w, h)
    ofb.clear(sc.clear_color)
    assert O.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, st)[0] == 0
    assert (ofb.zbuffer < 1e30).sum() > w * h // 50
    return sc, ofb.pixels.copy(), ofb.zbuffer.copy()


def _load(fb, px, zb):
    fb.upload(px)
    _upload_zbuffer(fb, zb)


def _frame_overlays(w, h):
    """The warrior's overlays for a w x h frame: (positions, topology, camera, the first call's MeshOverlay + list, the preview's)."""
    sc, v, polys, top, _ = hover_scene("obj-warrior")
    pos = np.ascontiguousarray(v["pos"], f32)
    sx, sy, some = _screen(pos, sc.camera, w, h, None)
    rect = (0.0, 0.0, float(np.median(sx[some])), float(h))
    ovs = case_overlays(polys, len(pos), rect)
    return pos, polys, top, sc.camera, ovs


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(64, 48), (320, 240)])
def test_gpu_overlay_frames_and_routes(gpu_ctx, w, h):
    """All sections in one call over the warrior's own z-buffer frame (the depth-tested edges and brackets are partly hidden), each of the
    three selections / preview modes; the two-call form with an orthographic camera for the preview; both choices of
    B32_ROUTE_PRIM_TILES: pixels equal cpu_records of the mirror's records byte for byte and the z-buffer is unchanged."""
    from bonnie32_amd import rasterizer as R
    sc, px, zb = _warrior_frame(w, h)
    pos, polys, top, cam, ovs = _frame_overlays(w, h)
    ortho_cam = IDENTITY_CAM                                   # (a Front viewport: its own camera, its own ortho)
    ortho = fit_ortho(pos, ortho_cam, w, h)
    fb = R.Framebuffer(w, h, gpu_ctx)
    rs = _slot(R, fb, sc.vertices)
    try:
        for routes in (0, R.Context.ROUTE_PRIM_TILES):
            gpu_ctx.set_routes(routes)
            for ov, sel in ovs[6:] + [(MO(abi.OVERLAY_BRACKETS | abi.OVERLAY_EDGES), None)]:
                recs = RM.mesh_overlay_records(pos, top, ov, sel, cam, w, h)
                want = px.copy()
                cpu_records(want, zb, w, h, recs)
                assert not np.array_equal(want, px)
                if w == 320 and ov.sections == abi.OVERLAY_BRACKETS | abi.OVERLAY_EDGES:
                    nodepth = px.copy()                                                 # the z-buffer hides part of the edges (at 64x48 the mesh
                    cpu_records(nodepth, None, w, h, recs)                              # covers 135 pixels and hides none)
                    assert int((nodepth != want).sum()) >= 100
                _load(fb, px, zb)
                fb.draw_mesh_overlay(rs, top, ov, cam, None, sel)
                got = fb.pixels
                assert np.array_equal(got, want), f"routes={routes} kind={ov.select_kind}: {int((got != want).sum())} bytes differ"
                assert np.array_equal(fb.zbuffer.view(np.uint32), zb.view(np.uint32))
            # two calls: the overlays with the frame's camera, the preview with an orthographic viewport's own camera and ortho
            ov, sel = ovs[-1]
            first = MO(ov.sections & ~abi.OVERLAY_PREVIEW, ov.hover_vertex, ov.hover_edge, ov.hover_face, ov.select_kind)
            for mode in range(3):
                osx, _, _ = _screen(pos, ortho_cam, w, h, ortho)
                second = MO(abi.OVERLAY_PREVIEW, preview_mode=mode, rect=(0.0, 0.0, float(np.median(osx)), float(h)))
                want = px.copy()
                cpu_records(want, zb, w, h, RM.mesh_overlay_records(pos, top, first, sel, cam, w, h))
                mid = want.copy()
                cpu_records(want, zb, w, h, RM.mesh_overlay_records(pos, top, second, None, ortho_cam, w, h, ortho))
                assert not np.array_equal(mid, want)
                _load(fb, px, zb)
                fb.draw_mesh_overlay(rs, top, first, cam, None, sel)
                fb.draw_mesh_overlay(rs, top if mode else None, second, ortho_cam, ortho)
                assert np.array_equal(fb.pixels, want), f"two calls, routes={routes} mode={mode}"
    finally:
        gpu_ctx.set_routes(0)
        rs.close()


@pytest.mark.gpu
def test_gpu_overlay_band_and_invalid_zbuffer(gpu_ctx):
    """320x240 with the band at rows 37..151: rows outside are untouched, rows inside equal the full frame's, an empty band draws nothing.
    A fresh framebuffer's z-buffer is not valid: the depth-tested records draw as against f32::MAX and the z-buffer stays so."""
    from bonnie32_amd import rasterizer as R
    w, h = 320, 240
    sc, px, zb = _warrior_frame(w, h)
    pos, polys, top, cam, ovs = _frame_overlays(w, h)
    ov, sel = ovs[-1]
    recs = RM.mesh_overlay_records(pos, top, ov, sel, cam, w, h)
    fb = R.Framebuffer(w, h, gpu_ctx)
    rs = _slot(R, fb, sc.vertices)
    try:
        full = px.copy()
        cpu_records(full, zb, w, h, recs)
        part = px.reshape(h, -1).copy(); part[37:151] = full.reshape(h, -1)[37:151]
        assert not np.array_equal(part[37:151], px.reshape(h, -1)[37:151]) and not np.array_equal(full.reshape(h, -1)[151:], px.reshape(h, -1)[151:])
        _load(fb, px, zb)
        fb.set_band(37, 151)
        fb.draw_mesh_overlay(rs, top, ov, cam, None, sel)
        fb.set_band(90, 90)
        fb.draw_mesh_overlay(rs, top, ov, cam, None, sel)
        fb.set_band(0, h)
        assert np.array_equal(fb.pixels, part.reshape(-1))
        assert np.array_equal(fb.zbuffer.view(np.uint32), zb.view(np.uint32))
    finally:
        fb.set_band(0, h)
        rs.close()
    ctx = R.Context(0)
    try:
        fb2 = R.Framebuffer(w, h, ctx)
        fb2.clear(b32.Color(3, 4, 5))                          # (deferred: the overlay flushes it)
        rs2 = _slot(R, fb2, sc.vertices)
        base = np.tile(np.array([3, 4, 5, 255], np.uint8), w * h)
        want = base.copy()
        cpu_records(want, None, w, h, recs)
        fb2.draw_mesh_overlay(rs2, top, ov, cam, None, sel)
        assert np.array_equal(fb2.pixels, want) and not np.array_equal(want, base)
        assert (fb2.zbuffer == np.finfo(f32).max).all()
        rs2.close()
    finally:
        for c, hnd in list(top._handles):
            if c is ctx:
                ctx.lib.b32_topology_destroy(ctx.h, hnd); top._handles.remove((c, hnd))
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(64, 48), (320, 240)])
def test_gpu_overlay_of_a_posed_slot_without_read_back(gpu_ctx, w, h):
    """b32_scene_pose, then the overlay -- nothing read back in between: the frame equals the host path pose_vertices -> mirror ->
    b32_draw_prims, and differs from the rest pose's; a second bone table moves it again; pose([]) brings the rest overlay back."""
    from bonnie32_amd import rasterizer as R
    sc, px, zb = _warrior_frame(w, h)
    pos, polys, top, cam, ovs = _frame_overlays(w, h)
    ov, sel = ovs[-1]
    bo = _warrior_bone_of(len(sc.vertices))
    fb = R.Framebuffer(w, h, gpu_ctx)
    rs = _slot(R, fb, sc.vertices)
    try:
        rs.set_rig(bo)
        frames = []
        for t in (3.0, 5.0, None):
            tab = _warrior_bones(t) if t is not None else []
            posed = RM.pose_vertices(sc.vertices, bo, tab) if t is not None else sc.vertices
            recs = RM.mesh_overlay_records(posed, top, ov, sel, cam, w, h)
            _load(fb, px, zb)
            fb.draw_prims(recs)                                                         # the host path
            want = fb.pixels
            ref = px.copy()
            cpu_records(ref, zb, w, h, recs)
            assert np.array_equal(want, ref)
            _load(fb, px, zb)
            rs.pose(tab)
            fb.draw_mesh_overlay(rs, top, ov, cam, None, sel)                           # (enqueued behind the pose: no synchronisation, no read-back)
            got = fb.pixels
            assert np.array_equal(got, want), f"t={t}: {int((got != want).sum())} bytes differ"
            frames.append(got)
        assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    finally:
        rs.close()


@pytest.mark.gpu
def test_gpu_overlay_order(gpu_ctx):
    """An overlay between two b32_draw_prims batches that overlap it: filled rectangles under it, circles over it -- and the other way
    round gives another image."""
    from bonnie32_amd import rasterizer as R
    w, h = 320, 240
    sc, px, zb = _warrior_frame(w, h)
    pos, polys, top, cam, ovs = _frame_overlays(w, h)
    ov, sel = ovs[-1]
    recs = RM.mesh_overlay_records(pos, top, ov, sel, cam, w, h)
    d = drawing(recs)
    cx, cy = int(np.median(d["x0"])), int(np.median(d["y0"]))
    under = np.concatenate([RM.prim(abi.PRIM_FILLED_RECT, cx - 40, cy - 40, cx + 10, cy + 30, b32.Color(200, 30, 30)) for _ in range(2)])
    over = np.concatenate([RM.prim(abi.PRIM_CIRCLE, cx + 5 * k, cy + 3 * k, 0, 0, b32.Color(30, 200, 30), size=6) for k in range(-3, 4)])
    fb = R.Framebuffer(w, h, gpu_ctx)
    rs = _slot(R, fb, sc.vertices)
    try:
        results = []
        for order in ((under, None, over), (over, None, under), (None, under, over)):
            want = px.copy()
            _load(fb, px, zb)
            for batch in order:
                cpu_records(want, zb, w, h, recs if batch is None else batch)
                if batch is None:
                    fb.draw_mesh_overlay(rs, top, ov, cam, None, sel)
                else:
                    fb.draw_prims(batch)
            got = fb.pixels
            assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
            results.append(got)
        assert not np.array_equal(results[0], results[1]) and not np.array_equal(results[0], results[2])
    finally:
        rs.close()


@pytest.mark.gpu
def test_gpu_overlay_in_the_delivered_frame_loop(oracle):
    """Two frames in flight through b32_frame_submit + one overlay per frame (another bone table each frame, the caller's list overwritten
    right after the call) + b32_fb_download_async: every delivered frame is byte-equal to the loop with the same records drawn through
    b32_draw_prims, and the tickets are the same numbers."""
    from bonnie32_amd import rasterizer as R, scenegen
    ctx = R.Context(0)
    try:
        st = b32.RasterSettings.game()
        meshes = [scenegen.make_scene("C1", n_tris=800, seed=300 + i, variant="gouraud") for i in range(2)]
        W, H = meshes[0].width, meshes[0].height
        cam = meshes[0].camera
        fb = R.Framebuffer(W, H, ctx)
        slots = [R.ResidentScene(fb, m.vertices, m.faces, m.textures).detach() for m in meshes]
        table = ctx.make_frame_table(cam, st, slots)
        # the overlaid mesh: the second console mesh's own vertices with the trivial topology of its triangles
        m = meshes[1]
        top = R.Topology.triangles(m.faces[:300])
        bo = _warrior_bone_of(len(m.vertices), seed=9)
        slots[1].set_rig(bo)
        sx, _, some = _screen(np.ascontiguousarray(m.vertices["pos"], f32), cam, W, H, None)
        rect = (0.0, 0.0, float(np.median(sx[some])), float(H))
        ov = MO(abi.OVERLAY_ALL, hover_vertex=5, hover_edge=(1, 2), hover_face=3, select_kind=abi.SELECT_POLYGONS, preview_mode=abi.PREVIEW_EDGE, rect=rect)
        sel0 = np.arange(0, 300, 3, dtype=np.uint32)
        bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
        span = float(np.ptp(m.vertices["pos"], axis=0).max())

        def run(device):
            out, tickets = [], []
            for i in range(4):
                tab = _warrior_bones(1.0 + i, 0.02 * span)
                fb.clear(b32.Color(10, 10, 30))
                slots[1].pose(tab)
                ctx.frame_submit(table)
                if device:
                    sel = sel0.copy()
                    fb.draw_mesh_overlay(slots[1], top, ov, cam, None, sel)
                    sel[:] = 7                                                          # the caller reuses its list at once
                else:
                    posed = RM.pose_vertices(m.vertices, bo, tab)
                    fb.draw_prims(RM.mesh_overlay_records(posed, top, ov, sel0, cam, W, H))
                tickets.append(ctx.download_async(bufs[i & 1][1]))
                if i >= 1:
                    ctx.ticket_wait(tickets[i - 1])
                    out.append(bufs[(i - 1) & 1][0].copy())
            ctx.ticket_wait(tickets[-1])
            out.append(bufs[3 & 1][0].copy())
            ctx.finish()
            return out, tickets

        host, t_host = run(False)
        dev, t_dev = run(True)
        for i, (a, b) in enumerate(zip(host, dev)):
            assert np.array_equal(a, b), f"frame {i}: {int((a != b).sum())} bytes differ"
        assert not np.array_equal(dev[0], dev[1])
        assert [t - t_host[0] for t in t_host] == [t - t_dev[0] for t in t_dev] == [0, 1, 2, 3]
        for _, p in bufs:
            ctx.host_free(p)
        top.close()
        for s in slots:
            s.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_overlay_argument_errors_and_empty_cases(gpu_ctx):
    """NULL context / camera / slot / struct, an unknown section bit, select_kind > 3, preview_mode > 2, a polygon section without a
    topology, a list that is missing, a slot without a scene: B32_E_ARG with the frame untouched; indices out of range are no error; nv ==
    0, np == 0, n_selected == 0 and sections == 0 draw nothing."""
    from bonnie32_amd import rasterizer as R
    W, H = 200, 150
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(b32.Color(1, 2, 3))
    base = fb.pixels
    pos, top = hand_mesh(), RM.Topology.from_polygons(HAND_POLYS)
    rs = _slot(R, fb, _mesh_vertices(pos))
    lib, cam = gpu_ctx.lib, IDENTITY_CAM.pack()
    sel = np.array([1, 2, 3, 4], np.uint32)
    good, _ = MO(abi.OVERLAY_ALL, select_kind=1).pack(sel)
    th = top.handle(gpu_ctx)
    call = lambda c=gpu_ctx.h, cm=C.byref(cam), s=rs._slot, t=th, o=good, l=sel.ctypes.data: lib.b32_draw_mesh_overlay(c, cm, None, s, t, C.byref(o) if o is not None else None, l)
    try:
        assert call(c=None) == call(cm=None) == call(s=None) == call(o=None) == abi.B32_E_ARG
        assert call(l=None) == abi.B32_E_ARG                                            # n_selected > 0 without a list
        for bad in (MO(64), MO(abi.OVERLAY_ALL | 128), MO(1, select_kind=4), MO(1, preview_mode=3)):
            assert call(o=bad.pack()[0]) == abi.B32_E_ARG
        for need in (MO(abi.OVERLAY_EDGES), MO(abi.OVERLAY_HOVER, hover_face=0), MO(abi.OVERLAY_PREVIEW, preview_mode=1), MO(abi.OVERLAY_PREVIEW, preview_mode=2)):
            assert call(t=None, o=need.pack()[0]) == abi.B32_E_ARG
        o3, s3 = MO(abi.OVERLAY_SELECTED, select_kind=3).pack([0])
        assert call(t=None, o=o3, l=s3.ctypes.data) == abi.B32_E_ARG
        empty = C.c_void_p()
        assert lib.b32_scene_create(gpu_ctx.h, C.byref(empty)) == 0
        assert call(s=empty) == abi.B32_E_ARG                                           # a slot that does not hold its scene
        lib.b32_scene_destroy(gpu_ctx.h, empty)
        out = np.zeros(400, abi.PRIM_DTYPE); n = C.c_uint32(77)
        tap = lambda w=W, h=H, cap=400, o=good, nn=C.byref(n): lib.b32_mesh_overlay_project_batch(gpu_ctx.h, C.byref(cam), None, rs._slot, th, C.byref(o), sel.ctypes.data, w, h,
                                                                                                   out.ctypes.data, cap, nn)
        assert tap(w=0) == tap(h=0) == tap(cap=10) == tap(nn=None) == abi.B32_E_ARG
        assert lib.b32_mesh_overlay_record_count(th, 16, None, None, C.byref(n)) == abi.B32_E_ARG
        assert lib.b32_mesh_overlay_record_count(None, 16, C.byref(MO(abi.OVERLAY_EDGES).pack()[0]), None, C.byref(n)) == abi.B32_E_ARG
        assert np.array_equal(fb.pixels, base)
        # no topology where none is read
        fb.draw_mesh_overlay(rs, None, MO(abi.OVERLAY_BRACKETS | abi.OVERLAY_DOTS | abi.OVERLAY_HOVER | abi.OVERLAY_SELECTED | abi.OVERLAY_PREVIEW, hover_vertex=1,
                                          hover_edge=(5, 6), select_kind=abi.SELECT_EDGES, rect=(0, 0, W, H)), IDENTITY_CAM, UNIT_ORTHO, [5, 6, 99, 1])
        assert not np.array_equal(fb.pixels, base)
        fb.upload(base)
        # the empty cases
        fb.draw_mesh_overlay(rs, top, MO(0, hover_vertex=1, select_kind=1), IDENTITY_CAM, UNIT_ORTHO, [1, 2])
        fb.draw_mesh_overlay(rs, top, MO(abi.OVERLAY_SELECTED, select_kind=abi.SELECT_POLYGONS), IDENTITY_CAM, UNIT_ORTHO, [])
        fb.draw_mesh_overlay(rs, top, MO(abi.OVERLAY_SELECTED | abi.OVERLAY_HOVER, select_kind=abi.SELECT_NONE), IDENTITY_CAM, UNIT_ORTHO, [1])
        none = RM.Topology.from_polygons([])
        fb.draw_mesh_overlay(rs, none, MO(abi.OVERLAY_EDGES | abi.OVERLAY_PREVIEW | abi.OVERLAY_HOVER | abi.OVERLAY_SELECTED, hover_face=0, select_kind=3, preview_mode=2,
                                          rect=(0, 0, W, H)), IDENTITY_CAM, UNIT_ORTHO, [0, 1])
        nov = R.ResidentScene(fb, b32.make_vertices(0), b32.make_faces(0), []).detach()
        fb.draw_mesh_overlay(nov, top, MO(abi.OVERLAY_ALL, hover_vertex=0, hover_edge=(0, 1), hover_face=1, select_kind=3, preview_mode=2, rect=(0, 0, W, H)),
                             IDENTITY_CAM, UNIT_ORTHO, [0, 1])
        assert len(fb.mesh_overlay_project_batch(nov, top, MO(abi.OVERLAY_ALL, select_kind=1), IDENTITY_CAM, UNIT_ORTHO, [0, 1])) == \
            RM.mesh_overlay_record_count(top, 0, MO(abi.OVERLAY_ALL, select_kind=1), [0, 1])
        nov.close(); none.close()
        assert np.array_equal(fb.pixels, base)
        # the bounds are armed again after every call: the same brackets twice
        a = fb.mesh_overlay_project_batch(rs, top, MO(abi.OVERLAY_BRACKETS), IDENTITY_CAM, UNIT_ORTHO)
        b = fb.mesh_overlay_project_batch(rs, top, MO(abi.OVERLAY_BRACKETS), IDENTITY_CAM, UNIT_ORTHO)
        assert a.tobytes() == b.tobytes() == RM.mesh_overlay_records(pos, top, MO(abi.OVERLAY_BRACKETS), None, IDENTITY_CAM, W, H, UNIT_ORTHO).tobytes() and len(drawing(a)) == 24
    finally:
        rs.close(); top.close()
