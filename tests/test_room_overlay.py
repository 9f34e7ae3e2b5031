"""The world editor's room overlays through b32_draw_room_overlay (editor/viewport_3d.rs:4273-4658, :4862-5362).

Nothing else in the repository draws these, so the expectation is built here:
  `ref_room_overlay`  a literal scalar restatement of the five sections of draw_viewport_3d over a room's records, every operand an
                      np.float32: it records the calls the reference makes (fb.draw_circle, fb.draw_thick_line, draw_3d_line) per section
                      in call order; draw_3d_line goes through tests.test_gizmos.ref_gizmos, the circles and thick lines through
                      tests.test_room_hover.ref_world_to_screen and a cast.
The mirror (rasterizer.room_overlay_records, vectorised, written from the Rust text) and csrc/b32_room_overlay_body.h -- the device code --
compiled for the host are compared with it: the records that draw equal the restatement's calls per section, in order, and mirror and
header agree byte for byte, places included.  Every GPU frame is compared byte for byte with a frame composed on the CPU:
tests.test_prims.np_prims draws the restatement's records over the oracle's frame."""
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
from bonnie32_amd import rasterizer as RM
from tests.test_prims import _as_i32, np_prims
from tests.test_gizmos import ref_clip_line_to_rect, ref_gizmos
from tests.test_world import noop_records, ref_clip
from tests.test_room_hover import (IDENTITY_CAM, KINDS, RefRoom, _cam_f32, face, faces_of, grid_of, make_camera, random_room, real_room, ref_corners,
                                   ref_winner, ref_world_to_screen, room_cursors, winner_cases)
from tests.test_room_mesh import real_room as real_room_materials, real_scene

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
LIM = 1 << 30
S = abi.SECTOR_SIZE
RO = RM.RoomOverlay
ALL = abi.ROOM_OVERLAY_ALL
SECTIONS = ("vertices", "edges", "hover", "selected", "preview")
REAL_ROOMS = ("cathedral", "cave", "dungeon", "sewers")
SELECTED_VERTEX, HOVER_VERTEX, HOVER_EDGE, HOVER_FACE, SELECT, PREVIEW = (100, 255, 100), (255, 200, 150), (255, 200, 100), (150, 200, 255), (255, 200, 80), (100, 220, 255)


# ================================================================== the literal restatement
def ref_min(a, b):                                               # f32::min: a NaN is ignored
    return b if np.isnan(a) else (a if np.isnan(b) else (b if b < a else a))


def ref_max(a, b):
    return b if np.isnan(a) else (a if np.isnan(b) else (b if b > a else a))


def ref_preview_wall_corners(rec, grid):
    """The preview's own wall corners, viewport_3d.rs:5305-5329: WallSouth and WallWest run the other way round than in ref_corners."""
    px, py, pz = (f32(v) for v in grid["position"])
    SS = f32(grid["sector_size"])
    base_x = px + f32(int(rec["gx"])) * SS
    base_z = pz + f32(int(rec["gz"])) * SS
    h = [f32(v) for v in rec["heights"]]
    x0, z0, x1, z1 = {"North": (base_x, base_z, base_x + SS, base_z), "South": (base_x, base_z + SS, base_x + SS, base_z + SS),
                      "East": (base_x + SS, base_z, base_x + SS, base_z + SS), "West": (base_x, base_z, base_x, base_z + SS),
                      "NwSe": (base_x, base_z, base_x + SS, base_z + SS), "NeSw": (base_x + SS, base_z, base_x, base_z + SS)}[KINDS[int(rec["kind"])]]
    return [(x0, py + h[0], z0), (x1, py + h[1], z1), (x1, py + h[2], z1), (x0, py + h[3], z0)]


class Calls:
    """The reference's calls per section, in call order: ("circle", x, y, radius, rgb) and ("thick", x0, y0, x1, y1, rgb) as fb receives
    them, ("line", p0, p1, rgb, kind of the face) for draw_3d_line; `missed`: calls the reference does not make because a projection is None."""

    def __init__(self):
        self.sec = {s: [] for s in SECTIONS}
        self.missed = 0
        self.cur = None

    def add(self, *call):
        self.sec[self.cur].append(call)


def _ref_calls(faces, mats, grid, ov, camera, w, h):
    F = np.ascontiguousarray(faces, abi.SECTOR_FACE_DTYPE).reshape(-1)
    g = np.ascontiguousarray(grid, abi.ROOM_GRID_DTYPE).reshape(-1)[0]
    cam = _cam_f32(camera)
    n = len(F)
    c = Calls()
    hv = ov.hover
    winner = ref_winner(hv)
    hovered_vertex = (int(hv["vertex_rec"]), int(hv["vertex_corner"])) if winner == 0 else None
    hovered_edge = (int(hv["edge_rec"]), int(hv["edge_idx"])) if winner == 1 else None
    hovered_face = int(hv["face_rec"]) if winner == 2 else None
    screen = lambda p: ref_world_to_screen(p, cam, w, h)
    sector = lambda rec: F[rec] if rec < n else None             # room.get_sector(gx, gz) / sector.floor / walls.get(i)

    def draw_edge_highlight(rec, edge_idx, color):               # :4320-4388
        r = sector(rec)
        if r is None:
            return
        corners = ref_corners(r, g)
        v0, v1 = corners[edge_idx], corners[(edge_idx + 1) % 4]
        s0, s1 = screen(v0), screen(v1)
        if s0 is not None and s1 is not None:
            c.add("thick", _as_i32(s0[0]), _as_i32(s0[1]), _as_i32(s1[0]), _as_i32(s1[1]), color)
        else:
            c.missed += 1

    def face_lines(rec, color):                                  # :4493-4654, :4875-5046
        r = sector(rec)
        if r is None:
            return
        kind = int(r["kind"])
        line = lambda p0, p1: c.add("line", p0, p1, color, kind)
        if kind < 2:
            corners_1 = ref_corners(r, g)
            r2 = r.copy()
            split = abi.SPLIT_NWSE
            if mats is not None:
                m = mats[rec]
                split = int(m["split_direction"])
                if int(m["flags"]) & abi.MAT_HAS_HEIGHTS_2:      # get_heights_2()
                    r2["heights"] = m["heights_2"]
            corners_2 = ref_corners(r2, g)
            if split == abi.SPLIT_NWSE:
                line(corners_1[0], corners_1[1]); line(corners_1[1], corners_1[2])
                line(corners_2[2], corners_2[3]); line(corners_2[3], corners_2[0])
                line(corners_1[0], corners_1[2]); line(corners_2[0], corners_2[2])
            else:
                line(corners_1[0], corners_1[1]); line(corners_1[0], corners_1[3])
                line(corners_2[1], corners_2[2]); line(corners_2[2], corners_2[3])
                line(corners_1[1], corners_1[3]); line(corners_2[1], corners_2[3])
        else:
            p0, p1, p2, p3 = ref_corners(r, g)
            line(p0, p1); line(p1, p2); line(p2, p3); line(p3, p0); line(p0, p2)

    with np.errstate(all="ignore"):
        if ov.sections & abi.ROOM_OVERLAY_VERTICES:              # :4273-4316
            c.cur = "vertices"
            selected = set(int(k) for k in ov.vertices)
            for rec in range(n):                                 # collect_room_vertices order
                for corner_idx, world_pos in enumerate(ref_corners(F[rec], g)):
                    key = 4 * rec + corner_idx
                    is_hovered = hovered_vertex == (rec, corner_idx)
                    is_multi_selected = key in selected
                    is_primary_selected = is_multi_selected and key == ov.primary_vertex
                    if not (is_hovered or is_multi_selected):
                        continue                                 # (the reference projects first and skips then: the same calls)
                    s = screen(world_pos)
                    if s is None:
                        c.missed += 1
                        continue
                    color = SELECTED_VERTEX if (is_primary_selected or is_multi_selected) else HOVER_VERTEX
                    radius = 5 if is_primary_selected else 4
                    c.add("circle", _as_i32(s[0]), _as_i32(s[1]), radius, color)
        if ov.sections & abi.ROOM_OVERLAY_EDGES:                 # :4390-4402
            c.cur = "edges"
            for rec, edge_idx in ov.edges:
                draw_edge_highlight(int(rec), int(edge_idx), SELECTED_VERTEX)
        if ov.sections & abi.ROOM_OVERLAY_HOVER:                 # :4404-4658
            c.cur = "hover"
            if hovered_edge is not None:
                draw_edge_highlight(hovered_edge[0], hovered_edge[1], HOVER_EDGE)
            if hovered_face is not None:
                is_selected = ov.skip[0] <= hovered_face < ov.skip[0] + ov.skip[1]
                if not is_selected:
                    face_lines(hovered_face, HOVER_FACE)
        if ov.sections & abi.ROOM_OVERLAY_SELECTED:              # :4862-5247
            c.cur = "selected"
            for rec in ov.faces:
                face_lines(int(rec), SELECT)
            for rec, edge_idx in ov.edges:
                r = sector(int(rec))
                if r is not None:
                    corners = ref_corners(r, g)
                    c.add("line", corners[int(edge_idx)], corners[(int(edge_idx) + 1) % 4], SELECT, int(r["kind"]))
        if ov.sections & abi.ROOM_OVERLAY_PREVIEW:               # :5249-5362
            c.cur = "preview"
            x0, y0, x1, y1 = (f32(v) for v in ov.rect)
            rect_min_x, rect_max_x, rect_min_y, rect_max_y = ref_min(x0, x1), ref_max(x0, x1), ref_min(y0, y1), ref_max(y0, y1)
            if (rect_max_x - rect_min_x) > f32(3.0) or (rect_max_y - rect_min_y) > f32(3.0):
                items = RefRoom(F, grid, camera, w, h).box((rect_min_x, rect_min_y, rect_max_x, rect_max_y), [tuple(p) for p in ov.points])
                c.preview_items = items
                for i in items:
                    if i < n:
                        r = F[i]
                        kind = int(r["kind"])
                        corners = ref_corners(r, g) if kind < 2 else ref_preview_wall_corners(r, g)
                        for k in range(4):
                            c.add("line", corners[k], corners[(k + 1) % 4], PREVIEW, kind)
                    else:
                        world_pos = tuple(f32(v) for v in ov.points[i - n])
                        size = f32(64.0)
                        zero = f32(0.0)
                        sub = lambda a, b: (a[0] - b[0], a[1] - b[1], a[2] - b[2])
                        add = lambda a, b: (a[0] + b[0], a[1] + b[1], a[2] + b[2])
                        for d in ((size, zero, zero), (zero, size, zero), (zero, zero, size)):
                            c.add("line", sub(world_pos, d), add(world_pos, d), PREVIEW, -1)
    return c


def ref_room_overlay(faces, mats, grid, ov, camera, w, h):
    """({section: the abi.PRIM_DTYPE records of the calls that draw, in call order}, (drawn, dropped, rejected), the calls)."""
    c = _ref_calls(faces, mats, grid, ov, camera, w, h)
    lines = [call for s in SECTIONS for call in c.sec[s] if call[0] == "line"]
    items = np.zeros(len(lines), abi.GIZMO_ITEM_DTYPE)
    for i, (_, p0, p1, rgb, _kind) in enumerate(lines):
        items["p0"][i], items["p1"][i] = p0, p1
        items["r"][i], items["g"][i], items["b"][i] = rgb
    items["blend"], items["kind"] = abi.OPAQUE, abi.GIZMO_LINE
    line_recs, counts = ref_gizmos(items, camera, None, w, h) if len(lines) else (noop_records(0), (0, 0, 0))
    counts = [counts[0], counts[1] + c.missed, counts[2]]
    out, at = {}, 0
    for s in SECTIONS:
        recs = noop_records(len(c.sec[s]))
        for i, call in enumerate(c.sec[s]):
            r = recs[i]
            if call[0] == "line":
                recs[i] = line_recs[at]; at += 1
                continue
            rgb = call[-1]
            if call[0] == "circle":
                _, x, y, radius, _ = call
                if abs(x) >= LIM or abs(y) >= LIM:
                    counts[2] += 1
                    continue
                r["kind"], r["x0"], r["y0"], r["size"] = abi.PRIM_CIRCLE, x, y, radius
            else:
                _, x0, y0, x1, y1, _ = call
                if abs(x1 - x0) >= LIM or abs(y1 - y0) >= LIM:
                    counts[2] += 1
                    continue
                r["kind"], r["x0"], r["y0"], r["x1"], r["y1"], r["size"] = abi.PRIM_THICK_LINE, x0, y0, x1, y1, 3
            r["r"], r["g"], r["b"], r["blend"], r["alpha"] = rgb[0], rgb[1], rgb[2], abi.OPAQUE, 255
            counts[0] += 1
        out[s] = drawing(recs)
    return out, tuple(counts), c


def drawing(recs):
    """The records that draw: everything but the no-op (a circle of radius -1)."""
    return recs[~((recs["kind"] == abi.PRIM_CIRCLE) & (recs["size"] < 0))]


def by_section(recs, lay):
    edge = {"vertices": (lay["vertices"], lay["edges"]), "edges": (lay["edges"], lay["hover"]), "hover": (lay["hover"], lay["sel_faces"]),
            "selected": (lay["sel_faces"], lay["preview"]), "preview": (lay["preview"], lay["total"])}
    return {s: recs[a:b] for s, (a, b) in edge.items()}


def assert_equals_ref(recs, lay, want, what=""):
    got = by_section(recs, lay)
    for s in SECTIONS:
        g = drawing(got[s])
        assert len(g) == len(want[s]), f"{what} {s}: {len(g)} records draw, the reference makes {len(want[s])} calls"
        bad = np.nonzero(g != want[s])[0]
        assert not len(bad), f"{what} {s}: call {bad[0]}: {g[bad[0]]} != {want[s][bad[0]]}"


def ref_all_records(want):
    return np.concatenate([want[s] for s in SECTIONS])


# ================================================================== cases
@functools.lru_cache(maxsize=None)
def room_and_materials(name):
    faces, grid, cam, w, h = real_room(name)
    f2, mats, _ = real_room_materials(name)
    assert np.array_equal(faces, f2)
    return faces, mats, grid, cam, w, h


def hovers_of_each_winner(faces, grid, cam, w, h):
    """{winner: an abi.ROOM_HOVER_DTYPE record} from the mirror's hover at cursors near projected corners and on a lattice (inputs only)."""
    m = RM.RoomMirror(faces, grid, cam, w, h)
    corners, lattice = room_cursors(faces, grid, cam, w, h, 24)
    out = {}
    for mx, my in corners + lattice:
        r = m.hover(mx, my)
        if not any(np.isnan(float(r[k])) for k in ("vertex_depth", "edge_depth", "face_depth")):
            out.setdefault(ref_winner(r), r)
    return out


def half_rect(faces, grid, cam, w, h):
    """selection_rect_start / _end, stored end before start, covering the left half of the frame or so."""
    return (float(w) * 0.55, float(h) + 20.0, -10.0, -20.0)


# a camera inside the Cathedral from which faces of all eight kinds are in the frame (its own camera sees no ceiling), found by a search over
# sector centres with the mirror and kept as data
CATHEDRAL_CAM = b32.Camera(position=(15872.0, 800.0, -5632.0), basis_x=(-0.46672430634498596, -0.0, -0.884402871131897),
                           basis_y=(-0.15543900430202484, -0.9844337701797485, 0.08202953636646271),
                           basis_z=(-0.8706360459327698, 0.17575587332248688, 0.4594591557979584))


def ctrl_a_overlay(name, winner, sections=ALL, size=None, cam=None):
    """Every face selected, every 7th vertex key (one of them primary), every 5th record's edge rec % 4, a hover of the winner type, a
    rectangle over about half the frame, three object positions."""
    faces, mats, grid, own_cam, w, h = room_and_materials(name)
    cam = cam or own_cam
    if size is not None:
        w, h = size
    n = len(faces)
    hov = hovers_of_each_winner(faces, grid, cam, w, h)
    keys = np.arange(0, 4 * n, 7, dtype=np.uint32)
    recs = np.arange(0, n, 5, dtype=np.uint32)
    pos = np.array(cam.position, f32)
    bz = np.array(cam.basis_z, f32)
    bx = np.array(cam.basis_x, f32)
    points = np.stack([pos + bz * f32(2000.0) - bx * f32(600.0), pos + bz * f32(1500.0) + bx * f32(900.0), pos - bz * f32(500.0)]).astype(f32)
    return RO(sections, hover=hov.get(winner), primary_vertex=int(keys[len(keys) // 2]), skip=(0, 0), rect=half_rect(faces, grid, cam, w, h),
              vertices=keys, edges=np.stack([recs, recs % 4], axis=1), faces=np.arange(n, dtype=np.uint32), points=points)


def wild_room(seed):
    """A random room with every kind, several walls per side, then NaN / inf heights, materials with heights_2 and both splits."""
    faces, grid, cam, w, h = random_room(seed, 6, 5)
    faces = faces.copy()
    rng = np.random.default_rng(seed + 100)
    n = len(faces)
    mats = np.zeros(n, abi.FACE_MATERIAL_DTYPE)
    mats["split_direction"] = rng.integers(0, 2, n)
    has2 = rng.random(n) < 0.4
    mats["flags"] = np.where(has2, abi.MAT_HAS_HEIGHTS_2, 0)
    mats["heights_2"] = faces["heights"] + rng.choice(np.array([0.0, 128.0, -256.0], f32), (n, 4))
    bad = rng.choice(n, 6, replace=False)
    faces["heights"][bad[0], 1] = np.nan; faces["heights"][bad[1], 2] = np.inf; faces["heights"][bad[2], 0] = -np.inf
    mats["heights_2"][bad[3], 3] = np.nan; faces["heights"][bad[4], :] = 3e38; faces["heights"][bad[5], 3] = -0.0
    return faces, mats, grid, cam, w, h


def fine_room(seed):
    """A larger random room whose heights, grid origin and camera are off every lattice, at 640 x 480: the products of its projections are
    not exact, so a fused multiply-add rounds some of them differently."""
    faces, grid, cam, _, _ = random_room(seed, 12, 10)
    faces = faces.copy()
    rng = np.random.default_rng(seed + 7)
    faces["heights"] = (faces["heights"] + rng.uniform(-90.0, 90.0, faces["heights"].shape)).astype(f32)
    grid = grid_of((-2011.37, 13.71, -1777.93), 1000.0 / 3.0)
    cam = make_camera((-1200.3 + rng.normal() * 50.0, 777.7, -900.9 + rng.normal() * 50.0), 0.31, 0.83)
    mats = np.zeros(len(faces), abi.FACE_MATERIAL_DTYPE)
    mats["split_direction"] = rng.integers(0, 2, len(faces))
    mats["flags"] = abi.MAT_HAS_HEIGHTS_2
    mats["heights_2"] = (faces["heights"] + rng.uniform(-40.0, 40.0, faces["heights"].shape)).astype(f32)
    return faces, mats, grid, cam, 640, 480


# (position, rot_x, rot_y) inside the fine room: cameras at which a build of the device header with fused multiply-adds makes other records
# than the separately rounded one (a search over random cameras found one at every second; four are kept as data)
FINE_CAMERAS = (((-458.21, 426.78, -1464.17), -0.256, 6.275), ((483.29, 287.61, -295.16), 0.577, 5.637), ((1245.31, 281.85, 1086.34), 0.485, 0.116),
                ((594.72, 471.06, -934.33), 0.277, 0.673))


def wild_overlay(faces, grid, cam, w, h, winner, seed):
    rng = np.random.default_rng(seed)
    n = len(faces)
    hov = hovers_of_each_winner(faces, grid, cam, w, h)
    keys = np.unique(rng.integers(0, 4 * n + 8, n)).astype(np.uint32)
    erec = rng.integers(0, n + 2, n // 2).astype(np.uint32)
    pts = (np.array(cam.position, f32) + rng.normal(size=(9, 3)).astype(f32) * f32(2500.0)).astype(f32)
    return RO(ALL, hover=hov.get(winner), primary_vertex=int(keys[3]), skip=(2, 5), rect=(float(w) * 0.6, -5.0, -5.0, float(h) + 5.0), vertices=keys,
              edges=np.stack([erec, rng.integers(0, 4, len(erec)).astype(np.uint32)], axis=1), faces=rng.permutation(n + 3).astype(np.uint32), points=pts)


# ---- the hand room: sector (0, 0) is x in [-512, 512], z in [2000, 3024] before the identity camera at 320 x 240
HAND_GRID = grid_of((-512.0, -300.0, 2000.0), S)
HW, HH = 320, 240


def hand_room():
    """0 floor (0,0)   1 floor (1,0), its NW / SW corners coincide with 0's NE / SE   2 sloped WallSouth (0,0)   3 sloped WallWest (0,0)
    4 WallNorth (0,0)   5 floor (0,-2): crosses the near plane   6 NeSw diagonal   7 ceiling (0,0) with heights_2 and a NeSw split"""
    rows = [face(0, 0, abi.ROOM_FLOOR, (0.0, 0.0, 0.0, 0.0)), face(1, 0, abi.ROOM_FLOOR, (0.0, 64.0, 64.0, 0.0)),
            face(0, 0, abi.ROOM_WALL_SOUTH, (0.0, 128.0, 700.0, 400.0)), face(0, 0, abi.ROOM_WALL_WEST, (32.0, 96.0, 512.0, 300.0)),
            face(0, 0, abi.ROOM_WALL_NORTH, (0.0, 0.0, 600.0, 600.0)), face(0, -2 & 0xFFFF, abi.ROOM_FLOOR, (0.0, 0.0, 0.0, 0.0)),
            face(0, 0, abi.ROOM_WALL_NESW, (0.0, 10.0, 500.0, 520.0)), face(0, 0, abi.ROOM_CEILING, (600.0, 610.0, 620.0, 630.0))]
    faces = faces_of(rows)
    mats = np.zeros(len(rows), abi.FACE_MATERIAL_DTYPE)
    mats["flags"][7] = abi.MAT_HAS_HEIGHTS_2; mats["heights_2"][7] = (650.0, 640.0, 700.0, 660.0); mats["split_direction"][7] = abi.SPLIT_NESW
    return faces, mats


def hover_record(vertex=None, edge=None, face_=None):
    """(rec, corner, depth) / (rec, idx, depth) / (rec, depth)"""
    r = RO().hover.copy()
    if vertex is not None:
        r["vertex_rec"], r["vertex_corner"], r["vertex_depth"] = vertex; r["vertex_dist"] = 1.0
    if edge is not None:
        r["edge_rec"], r["edge_idx"], r["edge_depth"] = edge; r["edge_dist"] = 1.0
    if face_ is not None:
        r["face_rec"], r["face_depth"] = face_
    return r


def hand_cases():
    """(name, faces, mats or None, grid, camera, w, h, RoomOverlay)"""
    faces, mats = hand_room()
    near_faces = faces.copy()
    grid = HAND_GRID
    # the floor at gz = -2 would need a negative gz; instead a second grid puts sector (0, 0) across the camera plane
    near_grid = grid_of((-512.0, -50.0, -300.0), S)
    out = []
    add = lambda name, ov, f=faces, m=mats, g=grid, cam=IDENTITY_CAM: out.append((name, f, m, g, cam, HW, HH, ov))
    V, E, H_, SEL, P = (abi.ROOM_OVERLAY_VERTICES, abi.ROOM_OVERLAY_EDGES, abi.ROOM_OVERLAY_HOVER, abi.ROOM_OVERLAY_SELECTED, abi.ROOM_OVERLAY_PREVIEW)
    # a hovered vertex coincident with a selected one of the neighbouring sector, in both key orders: record 0's NE (key 1) and record 1's NW (key 4)
    add("hovered before selected", RO(V, hover=hover_record(vertex=(0, 1, 2000.0)), vertices=[4]))
    add("hovered after selected", RO(V, hover=hover_record(vertex=(1, 0, 2000.0)), vertices=[1]))
    add("hovered vertex is selected", RO(V, hover=hover_record(vertex=(1, 0, 2000.0)), vertices=[1, 4, 9]))
    add("primary vertex", RO(V, vertices=[1, 4, 9, 30], primary_vertex=9))
    add("hover loses to the edge", RO(V | H_, hover=hover_record(vertex=(0, 1, 2500.0), edge=(4, 2, 2000.0)), vertices=[4]))
    add("hovered face outside the skip range", RO(H_, hover=hover_record(face_=(7, 2100.0)), skip=(0, 7)))
    add("hovered face inside the skip range", RO(H_, hover=hover_record(face_=(7, 2100.0)), skip=(6, 2)))
    add("hovered wall", RO(H_, hover=hover_record(face_=(6, 2100.0))))
    add("sloped south and west walls, selected and previewed", RO(SEL | P, faces=[2, 3], edges=[(2, 0), (3, 2)], rect=(0.0, 0.0, 320.0, 240.0)))
    add("all sections", RO(ALL, hover=hover_record(face_=(0, 2400.0)), vertices=[0, 5, 6, 28, 31], primary_vertex=5, edges=[(2, 1), (7, 3), (6, 0)],
                           faces=[7, 0, 6, 2], rect=(320.0, 240.0, 0.0, 0.0), points=[(0.0, 0.0, 2500.0)]))
    add("an edge with one end behind the near plane", RO(E | SEL, edges=[(0, 1), (0, 3), (0, 0)], faces=[0]), near_faces, mats, near_grid)
    add("a point with -0.0 coordinates", RO(P, rect=(0.0, 0.0, 320.0, 240.0), points=[(-0.0, -0.0, 900.0), (-0.0, 10.0, -0.0), (0.0, -0.0, 1200.0)]))
    add("a rectangle that fails the gate", RO(ALL, faces=[0], rect=(100.0, 50.0, 103.0, 47.0), points=[(0.0, 0.0, 2500.0)]))
    add("a rectangle that passes by one extent", RO(P, rect=(100.0, 0.0, 103.0, 240.0)))
    add("list indices >= n", RO(ALL, hover=hover_record(face_=(8, 2100.0)), vertices=[3, 32, 33, 4000], edges=[(8, 1), (1, 1), (4000000, 3)], faces=[9, 1, 8],
                                rect=(0.0, 0.0, 320.0, 240.0)))
    add("a hovered edge >= n", RO(ALL, hover=hover_record(edge=(8, 1, 2100.0)), vertices=[3]))
    add("a hovered vertex >= n", RO(ALL, hover=hover_record(vertex=(8, 1, 2100.0)), vertices=[3, 7]))
    add("a room without materials", RO(H_ | SEL, hover=hover_record(face_=(7, 2100.0)), faces=[7, 0]), faces, None)
    add("a NaN rectangle", RO(P, rect=(np.nan, 0.0, 200.0, 240.0)))
    return out


def room_cases():
    """(name, faces, mats or None, grid, camera, w, h, RoomOverlay): the real rooms with every face selected and a hover of each winner, wild
    random rooms, the hand cases."""
    out = []
    for name in REAL_ROOMS:
        faces, mats, grid, cam, w, h = room_and_materials(name)
        for winner in ((0, 1, 2) if name != "cathedral" else (2,)):
            out.append((f"{name} ctrl-a winner {winner}", faces, mats, grid, cam, w, h, ctrl_a_overlay(name, winner)))
    faces, mats, grid, _, w, h = room_and_materials("cathedral")
    out.append(("cathedral census", faces, mats, grid, CATHEDRAL_CAM, w, h, ctrl_a_overlay("cathedral", 2, cam=CATHEDRAL_CAM)))
    faces, mats, grid, _, w, h = fine_room(44)
    for k, (pos, rx, ry) in enumerate(FINE_CAMERAS):
        out.append((f"fine 44 camera {k}", faces, mats, grid, make_camera(pos, rx, ry), w, h,
                    RO(abi.ROOM_OVERLAY_SELECTED | abi.ROOM_OVERLAY_EDGES | abi.ROOM_OVERLAY_VERTICES, faces=np.arange(len(faces)), vertices=np.arange(0, 4 * len(faces), 3),
                       edges=np.stack([np.arange(len(faces)), np.arange(len(faces)) % 4], axis=1))))
    for seed in (41, 42):
        faces, mats, grid, cam, w, h = wild_room(seed)
        for winner in (0, 1, 2):
            out.append((f"wild {seed} winner {winner}", faces, mats, grid, cam, w, h, wild_overlay(faces, grid, cam, w, h, winner, seed)))
    faces, mats, grid, cam, w, h = wild_room(43)
    out.append(("wild 43 sector size 0", faces, mats, grid_of(tuple(grid["position"][0]), 0.0), cam, w, h, wild_overlay(faces, grid, cam, w, h, 2, 43)))
    return out + hand_cases()


@functools.lru_cache(maxsize=None)
def answers():
    """[(case, the restatement's (records per section, counts, calls))]: computed once, shared by the CPU and the GPU tests."""
    return [(c, ref_room_overlay(c[1], c[2], c[3], c[7], c[4], c[5], c[6])) for c in room_cases()]


@functools.lru_cache(maxsize=None)
def cathedral_answer():
    return next((c, a) for c, a in answers() if c[0] == "cathedral census")


# ================================================================== the device header compiled for the host
HOST_FLAGS = {"off": ["-O1", "-ffp-contract=off"], "fused": ["-O2", "-ffp-contract=fast", "-mfma"],
              "sanitized": ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@functools.lru_cache(maxsize=None)
def _host_dir():
    d = tempfile.mkdtemp(prefix="b32_room_overlay_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def host_exe(mode):
    exe = os.path.join(_host_dir(), "room_overlay_host_" + mode)
    subprocess.run(["g++", "-std=c++17"] + HOST_FLAGS[mode] + ["-I", os.path.join(ROOT, "bonnie-32_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "room_overlay_host.cpp"), "-o", exe], check=True)
    return exe


_host_calls = [0]


def host_overlay(faces, mats, grid, ov, cam, w, h, mode="off"):
    """tests/cpp/room_overlay_host.cpp on one case: (records in the device's layout, the layout's eight numbers, counts, winner)."""
    _host_calls[0] += 1
    base = os.path.join(_host_dir(), f"case{_host_calls[0]}")
    o, _ = ov.pack()
    F = np.ascontiguousarray(faces, abi.SECTOR_FACE_DTYPE).reshape(-1)
    with open(base + ".in", "wb") as fh:
        fh.write(np.array([w, h, len(F), int(mats is not None)], np.uint32).tobytes())
        fh.write(bytes(o))
        fh.write(np.ascontiguousarray(grid, abi.ROOM_GRID_DTYPE).reshape(-1)[:1].tobytes())
        c = cam.pack()
        fh.write(np.array(list(c.position) + list(c.basis_x) + list(c.basis_y) + list(c.basis_z), f32).tobytes())
        fh.write(F.tobytes())
        if mats is not None:
            fh.write(np.ascontiguousarray(mats, abi.FACE_MATERIAL_DTYPE).tobytes())
        for a in (ov.vertices, ov.edges, ov.faces, ov.points):
            fh.write(a.tobytes())
    r = subprocess.run([host_exe(mode), base + ".in", base + ".out"], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    blob = open(base + ".out", "rb").read()
    lay = np.frombuffer(blob[:32], np.uint32)
    counts = tuple(int(v) for v in np.frombuffer(blob[32:56], np.uint64))
    winner = int(np.frombuffer(blob[56:60], np.int32)[0])
    recs = np.frombuffer(blob[64:], abi.PRIM_DTYPE)
    assert len(recs) == lay[7]
    os.remove(base + ".in"); os.remove(base + ".out")
    return recs, lay, counts, winner


LAY_KEYS = ("vertices", "edges", "hover", "sel_faces", "sel_edges", "preview", "points", "total")


# ================================================================== CPU
def test_restatement_hand_cases():
    """The restatement pinned by hand: where the identity camera puts the hand room's corners, the order of coincident circles, the
    preview's reversed south and west walls, the sign of a zero in the crosses, the gate."""
    ans = {c[0]: a for c, a in answers()}
    sx = lambda x, z: int(f32(x) * f32(4.0) / (f32(z) + f32(5.0)) * f32(90.0) + f32(160.0))
    sy = lambda y, z: int(f32(y) * f32(4.0) / (f32(z) + f32(5.0)) * f32(90.0) + f32(120.0))
    at = (sx(512.0, 2000.0), sy(-300.0, 2000.0))                 # record 0's NE corner == record 1's NW corner
    v = ans["hovered before selected"][0]["vertices"]
    assert [(int(r["x0"]), int(r["y0"]), int(r["size"]), int(r["g"])) for r in v] == [(*at, 4, 200), (*at, 4, 255)]        # the selected one is drawn last
    v = ans["hovered after selected"][0]["vertices"]
    assert [(int(r["x0"]), int(r["y0"]), int(r["g"])) for r in v] == [(*at, 255), (*at, 200)]                                 # the hovered one is drawn last
    v = ans["hovered vertex is selected"][0]["vertices"]
    assert [int(r["g"]) for r in v] == [255, 255, 255]
    v = ans["primary vertex"][0]["vertices"]
    assert [int(r["size"]) for r in v] == [4, 4, 5, 4]
    a = ans["hover loses to the edge"][0]
    assert len(a["vertices"]) == 1 and len(a["hover"]) == 1 and int(a["hover"][0]["kind"]) == abi.PRIM_THICK_LINE and int(a["hover"][0]["size"]) == 3
    a = ans["sloped south and west walls, selected and previewed"]
    sel = [c for c in a[2].sec["selected"]][:5]
    pre = [c for c in a[2].sec["preview"] if c[4] == abi.ROOM_WALL_SOUTH][:4]
    # the selected south wall starts at (bx + S, h0, bz + S); the previewed one at (bx, h0, bz + S): heights[0] over the other end
    assert tuple(float(v) for v in sel[0][1]) == (512.0, -300.0, 3024.0) and tuple(float(v) for v in pre[0][1]) == (-512.0, -300.0, 3024.0)
    assert a[0]["selected"].tobytes() != a[0]["preview"].tobytes()
    a = ans["a point with -0.0 coordinates"]
    first = [c for c in a[2].sec["preview"] if c[4] == -1][0]
    assert np.signbit(first[1][1]) and not np.signbit(first[2][1])                   # -0.0 - 0.0 == -0.0, -0.0 + 0.0 == +0.0
    assert len([c for c in a[2].sec["preview"] if c[4] == -1]) == 6                  # two of the three points are in front of the camera
    a = ans["a rectangle that fails the gate"]
    assert len(a[2].sec["preview"]) == 0 and len(a[2].sec["selected"]) == 6
    assert "preview_items" not in vars(a[2]) and "preview_items" in vars(ans["a rectangle that passes by one extent"][2])
    a = ans["list indices >= n"]
    assert len(a[2].sec["vertices"]) == 1 and len(a[2].sec["edges"]) == 1 and len(a[2].sec["hover"]) == 0 and len(a[2].sec["selected"]) == 6 + 1
    a = ans["an edge with one end behind the near plane"]
    assert a[2].missed == 3 and a[1] == (3, 9, 0) and len(a[0]["selected"]) == 3 and len(a[0]["edges"]) == 0     # (two clipped at the near plane, one in front)
    a = ans["a room without materials"]
    # triangle 2 from the record's own heights and the NwSe split: slot 2 is corners_2[2] -> corners_2[3], y = -300 + 620 and -300 + 630
    assert len(a[2].sec["hover"]) == 6 and float(a[2].sec["hover"][2][1][1]) == 320.0 and float(a[2].sec["hover"][2][2][1]) == 330.0
    # f32::min / max ignore the NaN: the rectangle is x in [200, 200], y in [0, 240], which passes by its height
    assert "preview_items" in vars(ans["a NaN rectangle"][2])


def test_hover_skip_range_hand_case():
    """The restatement's hovered face: the ceiling with heights_2 and a NeSw split outside the skip range draws its six lines in the order
    of :4523-4532, inside the range nothing; a wall draws five."""
    ans = {c[0]: a for c, a in answers()}
    # record 7 with skip (0, 7): outside -> six lines; with skip (6, 2): inside -> nothing
    assert len(ans["hovered face outside the skip range"][2].sec["hover"]) == 6
    assert len(ans["hovered face inside the skip range"][2].sec["hover"]) == 0
    calls = ans["hovered face outside the skip range"][2].sec["hover"]
    # NeSw with heights_2: slot 2 is corners_2[1] -> corners_2[2], y = -300 + 640 and -300 + 700
    assert float(calls[2][1][1]) == 340.0 and float(calls[2][2][1]) == 400.0 and float(calls[1][2][1]) == 330.0      # slot 1: corners_1[0] -> corners_1[3]
    assert len(ans["hovered wall"][2].sec["hover"]) == 5


def test_mirror_and_host_header_equal_the_restatement():
    """rasterizer.room_overlay_records and csrc/b32_room_overlay_body.h built for the host (g++ -O1 -ffp-contract=off): the records that draw
    equal ref_room_overlay's calls per section, in order; mirror and header agree byte for byte, places included; so do the drawn / dropped
    / rejected counts, the layout and the record count."""
    n_drawn = 0
    for (name, faces, mats, grid, cam, w, h, ov), (want, counts, _) in answers():
        lay = RM.room_overlay_layout(len(faces), ov)
        mirror, mcounts = RM.room_overlay_records(faces, grid, ov, cam, w, h, mats, with_counts=True)
        assert len(mirror) == lay["total"] == RM.room_overlay_record_count(len(faces), ov), name
        assert_equals_ref(mirror, lay, want, name + " (mirror)")
        assert mcounts == counts, (name, mcounts, counts)
        recs, lay8, hcounts, winner = host_overlay(faces, mats, grid, ov, cam, w, h)
        assert [int(x) for x in lay8] == [lay[k] for k in LAY_KEYS], name
        assert winner == ref_winner(ov.hover), name
        assert recs.tobytes() == mirror.tobytes(), f"{name}: records {np.nonzero(recs != mirror)[0][:8]} differ from the mirror"
        assert hcounts == counts, (name, hcounts, counts)
        n_drawn += len(drawing(recs))
    assert n_drawn > 10000


def test_a_fused_evaluation_differs():
    """The same program built with FMA contraction (g++ -O2 -ffp-contract=fast -mfma) differs from the restatement: nothing contracted can
    pass the comparisons of this file.  A contraction moves a cast coordinate or a near-plane decision about once in ten thousand lines,
    so the inputs are the fine room's all-selected cases at FINE_CAMERAS."""
    n = 0
    for (name, faces, mats, grid, cam, w, h, ov), (want, _, _) in answers():
        if not name.startswith("fine"):
            continue
        recs, lay8, _, _ = host_overlay(faces, mats, grid, ov, cam, w, h, "fused")
        got = by_section(recs, RM.room_overlay_layout(len(faces), ov))
        for s in SECTIONS:
            g = drawing(got[s])
            n += 1 if len(g) != len(want[s]) else int((g != want[s]).sum())
    assert n >= 1, n


def test_cathedral_case_exercises_what_the_issue_lists():
    """Counted from the restatement's calls and records, never from the code under test: the Cathedral with every face selected."""
    (name, faces, mats, grid, cam, w, h, ov), (want, counts, calls) = cathedral_answer()
    assert len(faces) == 1029 and int((faces["kind"] >= 6).sum()) == 37
    assert int(((mats["flags"] & abi.MAT_HAS_HEIGHTS_2) != 0).sum()) == 7 and int((mats["split_direction"] == abi.SPLIT_NESW).sum()) == 5
    for s in SECTIONS:
        assert len(want[s]) > 0, s
    camf = _cam_f32(cam)
    sel = [c for c in calls.sec["selected"] if c[0] == "line"]
    drawn_kinds, shortened, behind = set(), 0, 0
    with np.errstate(all="ignore"):
        for _, p0, p1, _rgb, kind in sel:
            p0, p1 = tuple(f32(v) for v in p0), tuple(f32(v) for v in p1)
            cl = ref_clip(p0, p1, camf)
            if cl is None:
                behind += 1
                continue
            ends = [ref_world_to_screen(q, camf, w, h) for q in cl]
            if any(e is None for e in ends):
                continue
            sc = ref_clip_line_to_rect(ends[0][0], ends[0][1], ends[1][0], ends[1][1], f32(0), f32(0), f32(w), f32(h))
            if sc is not None:
                drawn_kinds.add(kind)
                shortened += sc[4] > 0
    n_sel = sum(1 for i in calls.preview_items if i < len(faces))
    census = (sorted(drawn_kinds), shortened, behind, n_sel, len(faces) - n_sel, counts)
    assert drawn_kinds == set(range(8)) and shortened >= 1 and behind >= 1 and 0 < n_sel < len(faces), census
    assert census == CATHEDRAL_CENSUS, census


# (kinds drawn, lines shortened by the screen clip, calls dropped behind the camera, preview records selected, not selected,
#  (drawn, dropped, rejected)) of the Cathedral case, from the restatement
CATHEDRAL_CENSUS = ([0, 1, 2, 3, 4, 5, 6, 7], 242, 56, 305, 724, (5193, 2862, 0))


def test_host_program_under_the_sanitizers():
    """The stand-alone program once more with -fsanitize=address,undefined, run directly: it ends clean and gives the same records."""
    picks = [(c, a) for c, a in answers() if c[0] in ("all sections", "list indices >= n", "cave ctrl-a winner 0", "wild 41 winner 2", "a room without materials")]
    assert len(picks) == 5
    for (name, faces, mats, grid, cam, w, h, ov), _ in picks:
        a = host_overlay(faces, mats, grid, ov, cam, w, h, "off")
        b = host_overlay(faces, mats, grid, ov, cam, w, h, "sanitized")
        assert a[0].tobytes() == b[0].tobytes() and a[2] == b[2], name


def test_layout_and_pod_layout_match_c():
    """B32RoomOverlay is 100 bytes with the fields where the C header puts them (compiled with g++ and gcc), the section bits match, and the
    record count follows the struct and the lists alone."""
    fields = ("sections", "hover_source", "hover", "primary_vertex", "skip_first", "skip_count", "n_vertices", "n_edges", "n_faces", "n_points", "x0", "y1")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void) { printf("%zu", sizeof(B32RoomOverlay));'
           + "".join(f' printf(" %zu", offsetof(B32RoomOverlay, {f}));' for f in fields)
           + ' printf(" %u %u %u %u %u\\n", B32_ROOM_OVERLAY_VERTICES, B32_ROOM_OVERLAY_EDGES, B32_ROOM_OVERLAY_HOVER, B32_ROOM_OVERLAY_SELECTED, B32_ROOM_OVERLAY_PREVIEW); return 0; }\n')
    T_ = abi.B32RoomOverlay
    want = [C.sizeof(T_)] + [getattr(T_, f).offset for f in fields] + [1, 2, 4, 8, 16]
    with tempfile.TemporaryDirectory() as d:
        for cc, ext in (("gcc", "c"), ("g++", "cpp")):
            open(os.path.join(d, "t." + ext), "w").write(src)
            subprocess.run([cc, "-I", os.path.join(ROOT, "include"), os.path.join(d, "t." + ext), "-o", os.path.join(d, "t")], check=True)
            out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
            assert [int(x) for x in out] == want, cc
    assert C.sizeof(T_) == 100
    assert (abi.ROOM_OVERLAY_VERTICES, abi.ROOM_OVERLAY_EDGES, abi.ROOM_OVERLAY_HOVER, abi.ROOM_OVERLAY_SELECTED, abi.ROOM_OVERLAY_PREVIEW) == (1, 2, 4, 8, 16)
    ov = RO(ALL, vertices=[1, 2, 3], edges=[(0, 1), (5, 2)], faces=[4, 5, 6, 7, 900], points=[(0, 0, 0)] * 2, rect=(0, 0, 10, 1))
    o, lists = ov.pack()
    assert (o.n_vertices, o.n_edges, o.n_faces, o.n_points, o.hover.vertex_rec, o.primary_vertex, o.x1) == (3, 2, 5, 2, NONE, NONE, 10.0) and all(lists)
    assert RM.room_overlay_record_count(98, ov) == (3 + 1) + 2 + 7 + (6 * 5 + 2) + (4 * 98 + 3 * 2)
    assert RM.room_overlay_record_count(98, RO(ALL, faces=[1], rect=(0, 0, 3, 3))) == 1 + 0 + 7 + 6
    assert RM.room_overlay_record_count(0, RO(abi.ROOM_OVERLAY_PREVIEW, rect=(0, 0, 9, 9), points=[(1, 2, 3)])) == 3
    assert RM.room_overlay_record_count(98, RO(0, faces=[1], vertices=[2])) == 0
    for bad in (RO(32), RO(1, hover_source=2), RO(2, edges=[(0, 4)]), RO(1, vertices=[3, 3]), RO(1, vertices=[4, 3])):
        with pytest.raises(ValueError):
            RM.room_overlay_record_count(98, bad)
    # the camera and the heights never move a record: the same places under another camera
    faces, mats = hand_room()
    ov = hand_cases()[9][7]
    a = RM.room_overlay_records(faces, HAND_GRID, ov, IDENTITY_CAM, HW, HH, mats)
    lifted = faces.copy(); lifted["heights"] += f32(77.0)
    b = RM.room_overlay_records(lifted, HAND_GRID, ov, make_camera((30.0, 40.0, -50.0), 0.1, 0.2), HW, HH, mats)
    assert len(a) == len(b) and not np.array_equal(a, b)


def test_winner_through_the_shared_header_equals_room_hover_winner():
    """b32_room_winner.h (what the device runs) built for the host answers every existing winner case as room_hover_winner does."""
    faces, mats = hand_room()
    for rec, want in winner_cases():
        ov = RO(abi.ROOM_OVERLAY_HOVER, hover=rec)
        ov.hover["edge_idx"] = min(int(ov.hover["edge_idx"]), 3) if int(ov.hover["edge_rec"]) != NONE else ov.hover["edge_idx"]
        got = host_overlay(faces, mats, HAND_GRID, ov, IDENTITY_CAM, HW, HH)[3]
        assert got == RM.room_hover_winner(rec) == want, (rec, got, want)


def test_cpp_mirror_room_overlay_compiles():
    """host/rasterizer.hpp: b32::RoomOverlay and b32::draw_room_overlay compile (header-only over the C ABI)."""
    hpp_dir = os.path.join(ROOT, "bonnie-32_amd", "host")
    src = ('#include "rasterizer.hpp"\nvoid f(b32::Framebuffer& fb, b32::Room& room, const b32::Camera& cam) {\n'
           ' b32::RoomOverlay o; o.sections = B32_ROOM_OVERLAY_VERTICES | B32_ROOM_OVERLAY_EDGES | B32_ROOM_OVERLAY_HOVER | B32_ROOM_OVERLAY_SELECTED | B32_ROOM_OVERLAY_PREVIEW;\n'
           ' o.hover_source = 1; o.vertices = { 1, 4 }; o.primary_vertex = 4; o.edges = { 0, 1, 3, 2 }; o.faces = { 0, 1, 2 };\n'
           ' o.points = { b32::Vec3{ 1.0f, 2.0f, 3.0f } }; o.x0 = 1; o.y0 = 2; o.x1 = 30; o.y1 = 40; o.skip_first = 1; o.skip_count = 2;\n'
           ' b32::draw_room_overlay(fb, room, o, cam); (void)sizeof(B32RoomOverlay); (void)o.pack().n_faces; }\n'
           'int main() { (void)&f; return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", hpp_dir, "-I", os.path.join(ROOT, "include"),
                        os.path.join(d, "t.cpp")], check=True)


# ================================================================== GPU
CAVE_SCENE = "cave-room0-game"
GPU_SIZES = [(64, 48), (320, 240)]


@functools.lru_cache(maxsize=None)
def cave_frame(w, h):
    """The golden Cave scene drawn by the oracle at w x h: (scene, pixels, z-buffer)."""
    from oracle import oracle as O
    sc = real_scene(CAVE_SCENE)
    ofb = O.Framebuffer(w, h)
    ofb.clear(sc.clear_color)
    assert O.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)[0] == 0
    return sc, ofb.pixels.copy(), ofb.zbuffer.copy()


@functools.lru_cache(maxsize=None)
def cave_case(w, h, winner=2, sections=ALL):
    """(faces, mats, grid, camera, RoomOverlay, the restatement's answer) of the Cave with every face selected at w x h."""
    faces, mats, grid, _, _, _ = room_and_materials("cave")
    cam = real_scene(CAVE_SCENE).camera
    ov = ctrl_a_overlay("cave", winner, sections, (w, h), cam)
    return faces, mats, grid, cam, ov, ref_room_overlay(faces, mats, grid, ov, cam, w, h)


def composed(px, zb, w, h, want):
    """The frame with the restatement's records drawn over it by np_prims, in section order."""
    out = px.copy()
    np_prims(out, zb, w, h, ref_all_records(want))
    return out


def _load(fb, px, zb):
    from tests.test_lines import _upload_zbuffer
    fb.upload(px)
    _upload_zbuffer(fb, zb)


def _room(R, ctx, faces, grid, mats):
    room = R.Room(ctx, faces, grid)
    if mats is not None:
        room.set_materials(mats)
    return room


def _with(ov, **kw):
    """A copy of a RoomOverlay with some members replaced."""
    args = dict(sections=ov.sections, hover=ov.hover, hover_source=ov.hover_source, primary_vertex=ov.primary_vertex, skip=ov.skip, rect=ov.rect,
                vertices=ov.vertices, edges=ov.edges, faces=ov.faces, points=ov.points)
    args.update(kw)
    return RO(**args)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cave-64x48", "cave-320x240", "cathedral-640x480"])
def test_gpu_room_overlay_stage_tap(gpu_ctx, which):
    """b32_room_overlay_project_batch equals the mirror record for record, places included, and the restatement call for call: the Cave at
    both frame sizes with all sections on, the Cathedral with every face selected at 640 x 480."""
    from bonnie32_amd import rasterizer as R
    if which.startswith("cave"):
        w, h = GPU_SIZES[which.endswith("320x240")]
        faces, mats, grid, cam, ov, (want, _, _) = cave_case(w, h)
    else:
        (_, faces, mats, grid, cam, w, h, ov), (want, _, _) = cathedral_answer()
    fb = R.Framebuffer(w, h, gpu_ctx)
    room = _room(R, gpu_ctx, faces, grid, mats)
    try:
        got = fb.room_overlay_project_batch(room, ov, cam, w, h)
        mirror = RM.room_overlay_records(faces, grid, ov, cam, w, h, mats)
        assert len(got) == gpu_ctx.room_overlay_record_count(room, ov) == len(mirror)
        assert got.tobytes() == mirror.tobytes(), f"records {np.nonzero(got != mirror)[0][:8]} differ from the mirror"
        assert_equals_ref(got, RM.room_overlay_layout(len(faces), ov), want, which)
        bare = R.Room(gpu_ctx, faces, grid)                      # no material table: the reference's defaults
        got = fb.room_overlay_project_batch(bare, ov, cam, w, h)
        assert got.tobytes() == RM.room_overlay_records(faces, grid, ov, cam, w, h, None).tobytes()
        bare.close()
    finally:
        room.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GPU_SIZES)
def test_gpu_room_overlay_frames(gpu_ctx, w, h):
    """The golden Cave frame, then b32_draw_room_overlay with all sections and a hover of each winner: the pixels equal the oracle's frame
    with the restatement's records drawn by np_prims, byte for byte, and the z-buffer is byte-equal before and after.  On a band only its
    rows are written, and an empty band draws nothing."""
    from bonnie32_amd import rasterizer as R
    sc, px, zb = cave_frame(w, h)
    fb = R.Framebuffer(w, h, gpu_ctx)
    room = None
    try:
        for winner in (0, 1, 2):
            faces, mats, grid, cam, ov, (want, _, _) = cave_case(w, h, winner)
            room = room or _room(R, gpu_ctx, faces, grid, mats)
            full = composed(px, zb, w, h, want)
            assert not np.array_equal(full, px)
            _load(fb, px, zb)
            fb.draw_room_overlay(room, ov, cam)
            got = fb.pixels
            assert np.array_equal(got, full), f"winner {winner}: {int((got != full).sum())} bytes differ"
            assert np.array_equal(fb.zbuffer.view(np.uint32), zb.view(np.uint32))
        y0, y1 = (h * 3) // 20, (h * 5) // 8
        rows = lambda a: a.reshape(h, -1)
        part = rows(px).copy(); part[y0:y1] = rows(full)[y0:y1]
        assert not np.array_equal(part[y0:y1], rows(px)[y0:y1]) and not np.array_equal(rows(full)[y1:], rows(px)[y1:])
        _load(fb, px, zb)
        fb.set_band(y0, y1)
        fb.draw_room_overlay(room, ov, cam)
        fb.set_band(y0 + 3, y0 + 3)
        fb.draw_room_overlay(room, ov, cam)
        fb.set_band(0, h)
        assert np.array_equal(fb.pixels, part.reshape(-1))
        assert np.array_equal(fb.zbuffer.view(np.uint32), zb.view(np.uint32))
    finally:
        fb.set_band(0, h)
        if room is not None:
            room.close()


@pytest.mark.gpu
def test_gpu_room_overlay_invalid_zbuffer_and_deferred_clear():
    """A fresh framebuffer's z-buffer is not valid and its clear is deferred: the overlay flushes the clear, draws, and the z-buffer stays
    f32::MAX everywhere."""
    from bonnie32_amd import rasterizer as R
    w, h = 320, 240
    faces, mats, grid, cam, ov, (want, _, _) = cave_case(w, h)
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(w, h, ctx)
        fb.clear(b32.Color(3, 4, 5))
        room = _room(R, ctx, faces, grid, mats)
        base = np.tile(np.array([3, 4, 5, 255], np.uint8), w * h)
        full = composed(base, None, w, h, want)
        fb.draw_room_overlay(room, ov, cam)
        assert np.array_equal(fb.pixels, full) and not np.array_equal(full, base)
        assert (fb.zbuffer == np.finfo(f32).max).all()
        room.close()
    finally:
        ctx.close()


def _drag(faces, step):
    """A height drag of seven records (all of them selected, so every section that reads heights moves)."""
    first = 72                                                   # (records 72 .. 78 of the Cave are in its camera's view)
    d = faces[first:first + 7].copy()
    d["heights"] += f32(48.0 + 16.0 * step)
    return first, d


@pytest.mark.gpu
def test_gpu_room_overlay_hover_on_the_device(gpu_ctx):
    """hover_source 1 behind b32_room_hover_async, WITHOUT waiting for the ticket before the draw, gives the frame of hover_source 0 with the
    delivered record; across a b32_room_update in between, the next overlay shows the new heights and the new hover.  Before any hover of
    a room: B32_E_ARG."""
    from bonnie32_amd import rasterizer as R
    w, h = 320, 240
    sc, px, zb = cave_frame(w, h)
    faces, mats, grid, cam, ov, _ = cave_case(w, h)
    faces = faces.copy()
    fb = R.Framebuffer(w, h, gpu_ctx)
    room = _room(R, gpu_ctx, faces, grid, mats)
    resident = _with(ov, hover_source=abi.ROOM_OVERLAY_HOVER_RESIDENT, hover=None)
    try:
        cam_p = cam.pack()
        o, lists = resident.pack()
        assert gpu_ctx.lib.b32_draw_room_overlay(gpu_ctx.h, C.byref(cam_p), room._h, C.byref(o), *lists) == abi.B32_E_ARG
        seen = set()
        for step, winner in enumerate((2, 0, 1, 2)):
            m = RM.RoomMirror(faces, grid, cam, w, h)
            corners, lattice = room_cursors(faces, grid, cam, w, h, 24)
            mouse = next((mx, my) for mx, my in corners + lattice if ref_winner(m.hover(mx, my)) == winner)
            _load(fb, px, zb)
            t, res = gpu_ctx.room_hover_async(room, cam, mouse)
            fb.draw_room_overlay(room, resident, cam)                       # (the ticket is not waited for)
            got = fb.pixels
            gpu_ctx.ticket_wait(t)
            rec = res.record
            res.close()
            assert rec.tobytes() == m.hover(*mouse).tobytes() and ref_winner(rec) == winner
            given = _with(ov, hover=rec)
            want, _, _ = ref_room_overlay(faces, mats, grid, given, cam, w, h)
            plain, _, _ = ref_room_overlay(faces, mats, grid, _with(ov, hover=None), cam, w, h)
            assert ref_all_records(want).tobytes() != ref_all_records(plain).tobytes()      # (the hovered element is among the calls)
            full = composed(px, zb, w, h, want)
            assert np.array_equal(got, full), f"step {step}: {int((got != full).sum())} bytes differ"
            _load(fb, px, zb)
            fb.draw_room_overlay(room, given, cam)
            assert np.array_equal(fb.pixels, full)
            seen.add(got.tobytes())
            first, d = _drag(faces, step)                                    # the drag: the next step sees it
            faces[first:first + 7] = d
            room.update(first, d)
        assert len(seen) == 4
    finally:
        room.close()


@pytest.mark.gpu
def test_gpu_room_overlay_in_the_delivered_drag_loop(oracle):
    """Eight frames of update -> build_mesh -> frame_submit -> hover_async -> overlay (hover_source 1) -> download_async with nothing
    blocking in between and two frames in flight: every delivered frame equals the oracle's frame of that step's mesh with the
    restatement's records drawn over it, and every delivered hover the mirror's."""
    from bonnie32_amd import rasterizer as R
    from tests.test_room_mesh import _empty_scene
    sc = real_scene(CAVE_SCENE)
    W, H, st = sc.width, sc.height, sc.settings
    faces, mats, grid, cam, ov, _ = cave_case(W, H)
    faces = faces.copy()
    resident = _with(ov, hover_source=abi.ROOM_OVERLAY_HOVER_RESIDENT, hover=None)
    ctx = R.Context(0)
    bufs, hbufs = [], []
    try:
        fb = R.Framebuffer(W, H, ctx)
        rs = _empty_scene(R, fb, sc.textures)
        room = _room(R, ctx, faces, grid, mats)
        room.build_mesh(rs)
        fb.clear(sc.clear_color); rs.render_async(cam, st, sc.fog); rs.finish()              # (capacities settled by a warm-up frame)
        table = ctx.make_frame_table(cam, st, [rs], fogs=[sc.fog])
        bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
        hbufs = [ctx.host_alloc(64) for _ in range(2)]
        corners, lattice = room_cursors(faces, grid, cam, W, H, 24)
        steps, tickets, delivered = [], [], []

        def collect(i):
            ctx.ticket_wait(tickets[i][0]); ctx.ticket_wait(tickets[i][1])
            delivered.append((bufs[i & 1][0].copy(), hbufs[i & 1][0][:48].view(abi.ROOM_HOVER_DTYPE)[0].copy()))

        for i in range(8):
            first, d = _drag(faces, i)
            faces[first:first + 7] = d
            mouse = (corners + lattice)[(5 * i) % len(corners + lattice)]
            steps.append((faces.copy(), mouse))
            # ---- everything enqueued without a host synchronisation in between
            room.update(first, d)
            room.build_mesh(rs)
            fb.clear(sc.clear_color)
            ctx.frame_submit(table)
            th, _res = ctx.room_hover_async(room, cam, mouse, out=hbufs[i & 1])
            fb.draw_room_overlay(room, resident, cam)
            tickets.append((ctx.download_async(bufs[i & 1][1]), th))
            if i >= 1:
                collect(i - 1)
        collect(7)
        ctx.finish()
        frames = set()
        for i, ((f_i, mouse), (pixels, hover)) in enumerate(zip(steps, delivered)):
            want_hover = RM.RoomMirror(f_i, grid, cam, W, H).hover(*mouse)
            assert hover.tobytes() == want_hover.tobytes(), f"frame {i}: hover"
            v, f = b32.room_mesh(f_i, mats, grid)
            ofb = oracle.Framebuffer(W, H); ofb.clear(sc.clear_color)
            assert oracle.render_mesh_15(ofb, v, f, sc.textures, cam, st, sc.fog)[0] == 0
            want, _, _ = ref_room_overlay(f_i, mats, grid, _with(ov, hover=want_hover), cam, W, H)
            full = composed(ofb.pixels.copy(), ofb.zbuffer.copy(), W, H, want)
            assert np.array_equal(pixels, full.reshape(-1)), f"frame {i}: {int((pixels != full.reshape(-1)).sum())} bytes differ"
            frames.add(pixels.tobytes())
        assert len(frames) == 8
        room.close(); rs.close()
    finally:
        for _, p in bufs + hbufs:
            ctx.host_free(p)
        ctx.close()


@pytest.mark.gpu
def test_gpu_room_overlay_split_calls_counts_and_empty_cases(gpu_ctx):
    """Two calls with disjoint section bits equal one call with both; b32_gizmo_counts rises by the restatement's drawn / dropped / rejected;
    empty lists and sections == 0 draw nothing."""
    from bonnie32_amd import rasterizer as R
    w, h = 320, 240
    sc, px, zb = cave_frame(w, h)
    faces, mats, grid, cam, ov, (want, counts, _) = cave_case(w, h)
    fb = R.Framebuffer(w, h, gpu_ctx)
    room = _room(R, gpu_ctx, faces, grid, mats)
    try:
        _load(fb, px, zb)
        before = fb.gizmo_counts()
        fb.draw_room_overlay(room, ov, cam)
        after = fb.gizmo_counts()
        one = fb.pixels
        assert tuple(a - b for a, b in zip(after, before)) == counts and counts[0] > 100 and counts[1] > 100
        first = abi.ROOM_OVERLAY_VERTICES | abi.ROOM_OVERLAY_EDGES | abi.ROOM_OVERLAY_HOVER
        _load(fb, px, zb)
        fb.draw_room_overlay(room, _with(ov, sections=first), cam)
        fb.draw_room_overlay(room, _with(ov, sections=ALL & ~first), cam)
        assert np.array_equal(fb.pixels, one)
        assert tuple(a - b for a, b in zip(fb.gizmo_counts(), after)) == counts
        # nothing to draw: the frame and the counts stay
        _load(fb, px, zb)
        fb.draw_room_overlay(room, _with(ov, sections=0), cam)
        fb.draw_room_overlay(room, RO(abi.ROOM_OVERLAY_VERTICES | abi.ROOM_OVERLAY_EDGES | abi.ROOM_OVERLAY_HOVER | abi.ROOM_OVERLAY_SELECTED), cam)
        fb.draw_room_overlay(room, RO(ALL, rect=(5.0, 5.0, 6.0, 7.0)), cam)                     # (the gate fails too)
        none = R.Room(gpu_ctx, b32.rtypes.make_sector_faces(0), grid)
        fb.draw_room_overlay(none, RO(ALL, vertices=[1, 2], edges=[(0, 1)], faces=[0, 5], rect=(0.0, 0.0, float(w), float(h))), cam)
        none.close()
        assert np.array_equal(fb.pixels, px.reshape(-1)) and fb.gizmo_counts()[0] == after[0] + counts[0]
    finally:
        room.close()


@pytest.mark.gpu
def test_gpu_room_overlay_argument_errors(gpu_ctx):
    """Every argument error returns its code and leaves the frame byte-equal: a NULL context, camera, room or overlay; an unknown section
    bit; hover_source > 1; hover_source 1 before any hover; an edge_idx > 3; keys not strictly ascending; a count > 0 with a NULL list; more
    than 2^31 - 1 records (B32_E_UNSUPPORTED); a zero-size framebuffer."""
    from bonnie32_amd import rasterizer as R
    W, H = 200, 150
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(b32.Color(1, 2, 3))
    base = fb.pixels
    faces, mats = hand_room()
    room = _room(R, gpu_ctx, faces, HAND_GRID, mats)
    lib, cam = gpu_ctx.lib, IDENTITY_CAM.pack()
    good = RO(ALL, vertices=[1, 4, 9], edges=[(2, 1), (7, 3)], faces=[0, 7], points=[(0.0, 0.0, 2500.0)], rect=(0.0, 0.0, float(W), float(H)),
              hover=hover_record(edge=(4, 2, 2000.0)))

    def call(ov=good, c=gpu_ctx.h, cm=C.byref(cam), r=None, o="pack", drop=None):
        po, lists = ov.pack()
        lists = [None if k == drop else p for k, p in enumerate(lists)]
        return lib.b32_draw_room_overlay(c, cm, room._h if r is None else r, C.byref(po) if o == "pack" else None, *lists), (po, lists)

    try:
        E = abi.B32_E_ARG
        assert call(c=None)[0] == call(cm=None)[0] == call(o=None)[0] == E
        assert lib.b32_draw_room_overlay(gpu_ctx.h, C.byref(cam), None, C.byref(good.pack()[0]), *good.pack()[1]) == E
        for drop in range(4):
            assert call(drop=drop)[0] == E                                               # a count > 0 with a NULL list
        for bad in (_with(good, sections=32), _with(good, sections=ALL | 64), _with(good, hover_source=2), _with(good, hover_source=1),
                    _with(good, edges=[(2, 4)]), _with(good, vertices=[4, 4]), _with(good, vertices=[4, 9, 1]),
                    _with(good, hover=hover_record(edge=(4, 7, 2000.0)))):
            assert call(bad)[0] == E
        huge, lists = _with(good, sections=abi.ROOM_OVERLAY_SELECTED).pack()
        huge.n_faces = 400_000_000                                                        # 6 slots each: past 2^31 - 1 before a record is read
        n = C.c_uint32(77)
        assert lib.b32_draw_room_overlay(gpu_ctx.h, C.byref(cam), room._h, C.byref(huge), *lists) == abi.B32_E_UNSUPPORTED
        assert lib.b32_room_overlay_record_count(room._h, C.byref(huge), lists[1], lists[2], C.byref(n)) == abi.B32_E_UNSUPPORTED and n.value == 77
        out = np.zeros(200, abi.PRIM_DTYPE)
        po, pl = good.pack()
        tap = lambda w=W, h=H, cap=200, nn=C.byref(n): lib.b32_room_overlay_project_batch(gpu_ctx.h, C.byref(cam), room._h, C.byref(po), *pl, w, h, out.ctypes.data, cap, nn)
        assert tap(w=0) == tap(h=0) == tap(cap=10) == tap(nn=None) == E
        assert lib.b32_room_overlay_record_count(None, C.byref(po), pl[1], pl[2], C.byref(n)) == E
        assert lib.b32_room_overlay_record_count(room._h, C.byref(po), None, pl[2], C.byref(n)) == E
        assert np.array_equal(fb.pixels, base)
        assert call()[0] == abi.B32_OK and not np.array_equal(fb.pixels, base)
        assert gpu_ctx.room_overlay_record_count(room, good) == RM.room_overlay_record_count(len(faces), good)
    finally:
        room.close()
    ctx = R.Context(0)                                                                    # a context without a framebuffer
    try:
        r2 = R.Room(ctx, faces, HAND_GRID)
        po, pl = good.pack()
        assert ctx.lib.b32_draw_room_overlay(ctx.h, C.byref(cam), r2._h, C.byref(po), *pl) == abi.B32_E_ARG
        r2.close()
    finally:
        ctx.close()
