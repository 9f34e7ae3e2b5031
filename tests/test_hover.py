"""Hover and box selection: which vertex, else edge, else face of one resident mesh lies under the cursor (b32_hover_mesh), and which
vertices / polygons fall into a rectangle (b32_box_select).

The reference answers both on the host: find_hovered_element (modeler/viewport.rs:2379-2601) and apply_box_selection
(modeler/viewport.rs:1624-1779), over the modeler's n-gons (Face::edges / Face::triangulate, modeler/mesh_editor.rs:92-112).
  `ref_hover` / `ref_box_select`   literal scalar restatements of those loops, every operand an np.float32, built on tests.test_world's
               restatement of world_to_screen_with_ortho; pinned by hand-computed cases;
  `rasterizer.HoverMirror` / `box_select_mesh`   the library's numpy host mirrors, pinned to the restatements on the CPU;
  the device   compared with the mirrors.
Every comparison is exact: indices, distance and depth bits (any NaN equals any NaN), bitmaps.  All three branches of the hover are
compared raw for every cursor; the reference's tuple is `hovered_element` of them."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi
from tests.test_pick import PLACEMENTS, UNIT_ORTHO, interpolate_depth_in_triangle, point_in_triangle_2d, scene
from tests.test_world import IDENTITY_CAM, ORTHO, _cam_f32, ref_world_to_screen_with_ortho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NONE = 0xFFFFFFFF
# NULL; one turned by -2.9 rad about the origin, which keeps the scenes under their cursors and sends x and z to nearly -x and -z, so that
# the mirror test answers differently for the local and for the placed position; the infinite one
HOVER_PLACEMENTS = (None, PLACEMENTS[2], PLACEMENTS[4])
MIRRORS = [(axis, thr) for axis in (1, 2, 3) for thr in (1.0, 0.0, np.nan)]
MIRROR_GRID = [(0, 1.0)] + MIRRORS                             # off, then every axis with every threshold
OFFS = [(0, 0), (2.5, -1.25), (-5, 3), (4.5, 4.5), (0, 6), (-3, -3.5), (9, 0), (1, 0)]


def _bits(x):
    return int(np.array([x], f32).view(np.uint32)[0])


def _fbits(x):
    return "nan" if np.isnan(x) else _bits(x)


def canon(r):
    """A hover answer (a HOVER_RESULT_DTYPE record or ref_hover's dict) as a comparable tuple: indices, distance / depth bits, any NaN
    equal to any NaN."""
    return (int(r["vertex"]), _fbits(r["vertex_dist"]), int(r["edge_v0"]), int(r["edge_v1"]), _fbits(r["edge_dist"]), int(r["face"]),
            _fbits(r["face_depth"]))


# ---------------------------------------------------------------- literal restatement
def face_edges(vs):                                            # Face::edges, mesh_editor.rs:92-95
    n = len(vs)
    return [(vs[i], vs[(i + 1) % n]) for i in range(n)]


def face_triangulate(vs):                                      # Face::triangulate, mesh_editor.rs:99-112
    n = len(vs)
    if n < 3:
        return []
    if n == 3:
        return [(vs[0], vs[1], vs[2])]
    return [(vs[0], vs[i], vs[i + 1]) for i in range(1, n - 1)]


def point_to_line_distance(px, py, x0, y0, x1, y1):            # viewport.rs:2604-2622
    dx = x1 - x0
    dy = y1 - y0
    len_sq = dx * dx + dy * dy
    if len_sq < f32(0.001):
        return np.sqrt((px - x0) * (px - x0) + (py - y0) * (py - y0))
    t = ((px - x0) * dx + (py - y0) * dy) / len_sq
    if t < f32(0.0):                                           # f32::clamp(0.0, 1.0): a NaN and -0.0 stay
        t = f32(0.0)
    if t > f32(1.0):
        t = f32(1.0)
    proj_x = x0 + t * dx
    proj_y = y0 + t * dy
    return np.sqrt((px - proj_x) * (px - proj_x) + (py - proj_y) * (py - proj_y))


def ref_world_positions(positions, placement):
    """get_world_pos without bones (viewport.rs:2409-2421): the position as it is; with a placement, rotated and translated as
    check_mesh_hit does (viewport_3d.rs:7716-7718)."""
    out = []
    with np.errstate(all="ignore"):
        for p in positions:
            x, y, z = f32(p[0]), f32(p[1]), f32(p[2])
            if placement is None:
                out.append((x, y, z))
                continue
            c, s = f32(placement[0]), f32(placement[1])
            wx, wy, wz = (f32(v) for v in placement[2])
            rx = x * c - z * s
            rz = x * s + z * c
            out.append((rx + wx, y + wy, rz + wz))
    return out


class RefMesh:
    """What the reference has per mesh and frame: the vertices' screen positions (None stays None) and the front pass.  hover() walks the
    three loops as they stand; what an element's own expressions give for a cursor (a vertex's distance, a half-edge's distance, a fan
    triangle's area, hit and depth) depends on nothing else, so it is kept per cursor for the next call with other flags or mirror
    settings: the grid of the tests asks for each cursor forty times."""

    def __init__(self, positions, polygons, placement, camera, w, h, ortho=None):
        cam = _cam_f32(camera)
        self.local = [(f32(p[0]), f32(p[1]), f32(p[2])) for p in positions]
        self.polygons = [[int(i) for i in vs] for vs in polygons]
        with np.errstate(all="ignore"):
            self.sv = [ref_world_to_screen_with_ortho(p, cam, w, h, ortho) for p in ref_world_positions(positions, placement)]
            self._seen = {}
            nv = len(self.sv)
            self.vertex_on_front_face = [False] * nv                                   # viewport.rs:2435-2473
            self.edge_on_front_face = set()
            for vs in self.polygons:
                if len(vs) >= 3 and vs[0] < nv and vs[1] < nv and vs[2] < nv:
                    a, b, c = self.sv[vs[0]], self.sv[vs[1]], self.sv[vs[2]]
                    if a is not None and b is not None and c is not None:
                        signed_area = (b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1])
                        if signed_area > 0.0:
                            for vi in vs:
                                if vi < nv:
                                    self.vertex_on_front_face[vi] = True
                            for v0, v1 in face_edges(vs):
                                self.edge_on_front_face.add((min(v0, v1), max(v0, v1)))

    def editable(self, i, axis, threshold):                                             # state.rs:797-806
        if not axis:
            return True
        return bool(self.local[i][axis - 1] >= -f32(threshold))

    def hover(self, mx, my, see_through=False, mirror_axis=0, mirror_threshold=1.0, vertex_threshold=6.0, edge_threshold=4.0):
        """All three loops of find_hovered_element, each run whatever the others found.  Also reports the candidates of the vertex and of
        the half-edge loop: [(index or ordinal, dist)]."""
        mx, my = f32(mx), f32(my)
        nv = len(self.sv)
        vthr, ethr = f32(vertex_threshold), f32(edge_threshold)
        vdist, edist, tris = self._seen.setdefault((_bits(mx), _bits(my)), ({}, {}, {}))
        hovered_vertex = hovered_edge = hovered_face = None
        vcands, ecands = [], []
        with np.errstate(all="ignore"):
            for idx in range(nv):                                                       # viewport.rs:2475-2505
                if not see_through and not self.vertex_on_front_face[idx]:
                    continue
                if not self.editable(idx, mirror_axis, mirror_threshold):
                    continue
                s = self.sv[idx]
                if s is None:
                    continue
                dist = vdist.get(idx)
                if dist is None:
                    dist = vdist[idx] = np.sqrt((mx - s[0]) * (mx - s[0]) + (my - s[1]) * (my - s[1]))
                if dist < vthr:
                    vcands.append((idx, dist))
                    if hovered_vertex is None or dist < hovered_vertex[1]:
                        hovered_vertex = (idx, dist)
            ordinal = -1
            for vs in self.polygons:                                                    # viewport.rs:2507-2542
                for v0, v1 in face_edges(vs):
                    ordinal += 1
                    edge = (v0, v1) if v0 < v1 else (v1, v0)
                    if not see_through and edge not in self.edge_on_front_face:
                        continue
                    if v0 >= nv or v1 >= nv:
                        continue
                    if not self.editable(v0, mirror_axis, mirror_threshold) or not self.editable(v1, mirror_axis, mirror_threshold):
                        continue
                    a, b = self.sv[v0], self.sv[v1]
                    if a is None or b is None:
                        continue
                    dist = edist.get(ordinal)
                    if dist is None:
                        dist = edist[ordinal] = point_to_line_distance(mx, my, a[0], a[1], b[0], b[1])
                    if dist < ethr:
                        ecands.append((ordinal, dist))
                        if hovered_edge is None or dist < hovered_edge[1]:
                            hovered_edge = (edge, dist)
            for idx, vs in enumerate(self.polygons):                                    # viewport.rs:2544-2594
                if not all(vi < nv and self.editable(vi, mirror_axis, mirror_threshold) for vi in vs):
                    continue
                for k, (i0, i1, i2) in enumerate(face_triangulate(vs)):
                    a, b, c = self.sv[i0], self.sv[i1], self.sv[i2]
                    if a is None or b is None or c is None:
                        continue
                    seen = tris.get((idx, k))
                    if seen is None:
                        signed_area = (b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1])
                        inside = point_in_triangle_2d(mx, my, a[0], a[1], b[0], b[1], c[0], c[1])
                        depth = interpolate_depth_in_triangle(mx, my, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]) if inside else None
                        seen = tris[(idx, k)] = (signed_area, inside, depth)
                    signed_area, inside, depth = seen
                    if not see_through and signed_area <= 0.0:
                        continue
                    if inside:
                        if hovered_face is None or depth < hovered_face[1]:
                            hovered_face = (idx, depth)
        r = dict(vertex=NONE, vertex_dist=f32(0.0), edge_v0=NONE, edge_v1=NONE, edge_dist=f32(0.0), face=NONE, face_depth=f32(0.0))
        if hovered_vertex is not None:
            r["vertex"], r["vertex_dist"] = hovered_vertex
        if hovered_edge is not None:
            (r["edge_v0"], r["edge_v1"]), r["edge_dist"] = hovered_edge
        if hovered_face is not None:
            r["face"], r["face_depth"] = hovered_face
        r["vcands"], r["ecands"] = vcands, ecands
        return r


class WorldSpaceMirrorRefMesh(RefMesh):
    """What the reference does NOT do: the mirror test on the placed position.  The tests count how often its answer differs from
    RefMesh's, to show that their cases tell the two apart."""

    def __init__(self, positions, polygons, placement, camera, w, h, ortho=None):
        super().__init__(positions, polygons, placement, camera, w, h, ortho)
        self.local = ref_world_positions(positions, placement)


def ref_hover(positions, polygons, placement, camera, w, h, mx, my, ortho=None, **params):
    return RefMesh(positions, polygons, placement, camera, w, h, ortho).hover(mx, my, **params)


def ref_hovered_element(r):
    """The reference's return tuple (viewport.rs:2596-2600) given the three loops' answers: `if hovered_vertex.is_none()`,
    `if hovered_vertex.is_none() && hovered_edge.is_none()`."""
    v = None if r["vertex"] == NONE else int(r["vertex"])
    e = None if v is not None or r["edge_v0"] == NONE else (int(r["edge_v0"]), int(r["edge_v1"]))
    fc = None if v is not None or e is not None or r["face"] == NONE else int(r["face"])
    return v, e, fc


def ref_box_select(positions, polygons, placement, camera, w, h, rect, mode, ortho=None):
    """apply_box_selection (viewport.rs:1708-1726 vertices, :1743-1766 faces) for one rectangle: the selected indices, ascending."""
    cam = _cam_f32(camera)
    x0, y0, x1, y1 = (f32(v) for v in rect)
    world = ref_world_positions(positions, placement)
    selected = []
    with np.errstate(all="ignore"):
        if mode == abi.BOX_VERTICES:
            for idx, p in enumerate(world):
                s = ref_world_to_screen_with_ortho(p, cam, w, h, ortho)
                if s is not None and s[0] >= x0 and s[0] <= x1 and s[1] >= y0 and s[1] <= y1:
                    selected.append(idx)
        else:
            for idx, vs in enumerate(polygons):
                ps = [world[vi] for vi in vs if vi < len(world)]
                if ps:
                    acc = (f32(0.0), f32(0.0), f32(0.0))
                    for p in ps:
                        acc = (acc[0] + p[0], acc[1] + p[1], acc[2] + p[2])
                    k = f32(1.0) / f32(len(ps))
                    s = ref_world_to_screen_with_ortho((acc[0] * k, acc[1] * k, acc[2] * k), cam, w, h, ortho)
                    if s is not None and s[0] >= x0 and s[0] <= x1 and s[1] >= y0 and s[1] <= y1:
                        selected.append(idx)
    return selected


def words_of(selected, n):
    w = np.zeros((n + 31) // 32, np.uint32)
    for i in selected:
        w[i >> 5] |= np.uint32(1 << (i & 31))
    return w


# ---------------------------------------------------------------- inputs
def merge_quads(faces):
    """Each consecutive fan pair (a, b, c), (a, c, d) of a triangle list becomes the quad (a, b, c, d)."""
    fv = [tuple(int(i) for i in f) for f in faces["v"]]
    out, i = [], 0
    while i < len(fv):
        if i + 1 < len(fv) and fv[i][0] == fv[i + 1][0] and fv[i][2] == fv[i + 1][1]:
            out.append([fv[i][0], fv[i][1], fv[i][2], fv[i + 1][2]]); i += 2
        else:
            out.append(list(fv[i])); i += 1
    return out


_HOVER_SCENES = {}


def hover_scene(name, whole=False):
    """(scene, vertices, polygons, Topology, the 96 cursors).  The real scenes with their fan pairs merged into quads; C1 with the trivial
    topology of its first 256 faces (all of them with whole=True)."""
    from bonnie32_amd.rasterizer import Topology
    key = (name, whole)
    if key not in _HOVER_SCENES:
        sc = scene(name)[0]
        if name == "C1":
            polys = [[int(i) for i in f] for f in (sc.faces if whole else sc.faces[:256])["v"]]
        else:
            polys = merge_quads(sc.faces)
        top = Topology.from_polygons(polys)
        rm = RefMesh(sc.vertices["pos"], polys, None, sc.camera, sc.width, sc.height)
        ok = [s for s in rm.sv if s is not None]
        curs = []
        for k in range(96):
            o = OFFS[(k // 2) % 8]
            if k % 2 == 0:
                s = ok[(k // 2 * 7) % len(ok)]
                curs.append((float(s[0]) + o[0], float(s[1]) + o[1]))
            else:
                vs = polys[(k // 2 * 5) % len(polys)]
                a, b = rm.sv[vs[0]], rm.sv[vs[1]]
                curs.append(((float(a[0]) + float(b[0])) / 2 + o[1] / 2, (float(a[1]) + float(b[1])) / 2 + o[0] / 3))
        _HOVER_SCENES[key] = (sc, sc.vertices, polys, top, curs)
    return _HOVER_SCENES[key]


NV_ORDER = 2100
A_IDX = (5, 1030, 2050)


def _ngon(cx, cy, r, n):
    """n world positions around the screen point (cx, cy) (identity camera, UNIT_ORTHO, 320x240), ordered so that the polygon is front."""
    return [(cx + r * np.cos(2 * np.pi * k / n) - 160.0, 120.0 - (cy + r * np.sin(2 * np.pi * k / n)), 7.0) for k in range(n)]


def order_mesh(variant="base"):
    """The order cases in one mesh under the identity camera and UNIT_ORTHO (a vertex (x, y, z) lands at (x + 160, 120 - y), depth z):
    2100 vertices, nearly all of them a row far off screen; a few are moved to where the cases need them.
      5, 1030, 2050          coincident at screen (170, 110), on no polygon (three different workgroups of the vertex range)
      20, 21, 22 / 23        the front triangles (20, 21, 22) -- the FIRST polygon -- and (21, 20, 23) -- the LAST one, 400 filler triangles
                             and the other cases between them: the edge (20, 21) is half-edge 0 and, reversed, half-edge 1232
      30, 31, 32             a back-facing triangle
      40 / 41, 42            a polygon of one vertex and one of two; an empty polygon
      50..54 / 60..65        a front pentagon around (200, 180) and a front hexagon around (260, 180), radius 20
      70..72, 73..75, 76..78 (70, 71, 72, nv), (73, 74, 75, 0xFFFFFFFF): first three indices valid and front; (nv, 76, 77, 78): not
    variants: a polygon with a NaN / an infinite vertex first or last, a polygon (i, i, i) last."""
    v = b32.make_vertices(NV_ORDER)
    v["pos"][:, 0] = 500.0 + np.arange(NV_ORDER); v["pos"][:, 1] = -300.0; v["pos"][:, 2] = 10.0
    put = lambda i, sx, sy, z=5.0: v["pos"].__setitem__(i, (sx - 160.0, 120.0 - sy, z))
    for i in A_IDX:
        put(i, 170.0, 110.0)
    put(20, 109.7, 99.3); put(21, 121.9, 92.1); put(22, 115.0, 160.0); put(23, 115.0, 30.0)
    put(30, 40.0, 40.0); put(31, 60.0, 40.0); put(32, 40.0, 60.0)
    put(40, 60.0, 170.0); put(41, 80.0, 170.0); put(42, 100.0, 170.0)
    for k, p in enumerate(_ngon(200.0, 180.0, 20.0, 5)):
        v["pos"][50 + k] = p
    for k, p in enumerate(_ngon(260.0, 180.0, 20.0, 6)):
        v["pos"][60 + k] = p
    put(70, 200.0, 40.0); put(71, 230.0, 40.0); put(72, 200.0, 70.0)
    put(73, 250.0, 40.0); put(74, 280.0, 40.0); put(75, 250.0, 70.0)
    put(76, 200.0, 90.0); put(77, 230.0, 90.0); put(78, 200.0, 110.0)
    filler = [[100 + 3 * k, 101 + 3 * k, 102 + 3 * k] for k in range(400)]
    polys = ([[20, 21, 22]] + filler + [[30, 32, 31], [40], [41, 42], [], [50, 51, 52, 53, 54], [60, 61, 62, 63, 64, 65],
                                        [70, 71, 72, NV_ORDER], [73, 74, 75, NONE], [NV_ORDER, 76, 77, 78], [21, 20, 23]])
    if variant in ("nan_first", "nan_last", "inf_first", "inf_last"):
        v["pos"][90] = (np.nan if variant.startswith("nan") else np.inf, 0.0, 1000.0)
        polys = [[90, 20, 21]] + polys if variant.endswith("first") else polys + [[20, 90, 21]]
    elif variant == "same_thrice_last":
        polys = polys + [[20, 20, 20]]
    else:
        assert variant == "base"
    return v, polys


ORDER_VARIANTS = ("base", "nan_first", "nan_last", "inf_first", "inf_last", "same_thrice_last")
# the cursors the order cases are read at, then a spread over the screen
ORDER_CURSORS = [(171.0, 110.0), (41.0, 41.0), (60.0, 171.0), (90.0, 172.0), (200.0, 180.0), (260.0, 180.0), (201.0, 41.0), (210.0, 50.0),
                 (200.0, 55.0), (251.0, 41.0), (260.0, 50.0), (201.0, 91.0), (115.0, 100.0), (115.0, 90.0), (116.3, 94.1)] + \
                [(12.5 + 37.0 * (k % 8) + 0.25 * k, 9.0 + 29.0 * (k // 8)) for k in range(48)]


def edge_scan_cursors():
    """Cursors beside the edge (20, 21) of order_mesh: its two half-edges (20 -> 21 in the first polygon, 21 -> 20 in the last) see each of
    them in their own orientation."""
    ax, ay, bx, by = 109.7, 99.3, 121.9, 92.1
    rng = np.random.default_rng(3)
    out = []
    for _ in range(160):                                       # the middle of the edge (its neighbours are far), up to 3 beside it
        t = 0.3 + 0.4 * rng.random(); d = 6.0 * (rng.random() - 0.5)
        out.append((ax + t * (bx - ax) + d * 0.508, ay + t * (by - ay) + d * 0.861))
    return out


# ================================================================== without a GPU
def test_hover_pod_layout_matches_c():
    """B32HoverParams, B32HoverResult and B32BoxParams compiled against the public header have the layout of the abi dtypes, and the built
    library exports the entries."""
    import __graft_entry__ as g
    g.build()
    lib = abi.load_library()
    structs = (("B32HoverParams", abi.HOVER_PARAMS_DTYPE), ("B32HoverResult", abi.HOVER_RESULT_DTYPE), ("B32BoxParams", abi.BOX_PARAMS_DTYPE))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void){'
    for name, dt in structs:
        prog += f' printf("%zu", sizeof({name}));' + "".join(f' printf(" %zu", offsetof({name}, {f}));' for f in dt.names) + ' printf("\\n");'
    prog += ' printf("%u %u %u\\n", B32_HOVER_SEE_THROUGH, B32_BOX_VERTICES, B32_BOX_POLYGONS); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        lines = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    for (name, dt), line in zip(structs, lines):
        out = [int(x) for x in line.split()]
        assert out[0] == dt.itemsize == 32, name
        assert out[1:] == [dt.fields[f][1] for f in dt.names], name
    assert [int(x) for x in lines[3].split()] == [abi.HOVER_SEE_THROUGH, abi.BOX_VERTICES, abi.BOX_POLYGONS] == [1, 0, 1]
    names = {n for n, _, _ in abi.SYMBOLS}
    for name in ("b32_topology_create", "b32_topology_destroy", "b32_hover_mesh", "b32_hover_mesh_async", "b32_box_select", "b32_box_select_async"):
        assert name in names and getattr(lib, name).argtypes is not None
    E = abi.B32_E_ARG                                               # NULL context: no device needed
    assert lib.b32_hover_mesh(None, None, None, None, None, None, None, None) == E
    assert lib.b32_hover_mesh_async(None, None, None, None, None, None, None, None, None) == E
    assert lib.b32_box_select(None, None, None, None, None, None, None, None, None) == E
    assert lib.b32_box_select_async(None, None, None, None, None, None, None, None, None) == E
    assert lib.b32_topology_create(None, None, 0, None, None) == E


def _mesh(points, polygons):
    v = b32.make_vertices(len(points))
    v["pos"] = np.array(points, f32)
    return v, [list(p) for p in polygons]


def placed_mirror_mesh():
    """Two vertices joined by a polygon of two, for PLACEMENTS[3] (cos 0, sin -1, no offset: (x, y, z) becomes (z, y, -x)) under the
    identity camera and UNIT_ORTHO:
      Q = (5, 10, -8) is placed at (-8, 10, -5) -> screen (152, 110): x >= -1 holds for the local 5 and fails for the placed -8;
      S = (-5, 0, 8) is placed at (8, 0, 5) -> screen (168, 120): x >= -1 fails for the local -5 and holds for the placed 8."""
    return _mesh([(5, 10, -8), (-5, 0, 8)], [(0, 1)])


def _placed_mirror_checks(answer):
    """The mirror test reads the LOCAL position of a placed vertex; answer(mx, my, **mirror) -> a see-through hover of placed_mirror_mesh()
    under PLACEMENTS[3].  With the mirror on X (threshold 1.0) Q is hovered although it is placed at x = -8, S is not although it is placed
    at x = 8, and their edge goes with S; without the mirror both vertices and the edge are there."""
    none = (NONE, 0, NONE, NONE, 0, NONE, 0)
    assert canon(answer(152.0, 110.0, mirror_axis=1, mirror_threshold=1.0)) == (0, 0, NONE, NONE, 0, NONE, 0)
    assert canon(answer(168.0, 120.0, mirror_axis=1, mirror_threshold=1.0)) == none
    assert canon(answer(152.0, 110.0)) == (0, 0, 0, 1, 0, NONE, 0) and canon(answer(168.0, 120.0)) == (1, 0, 0, 1, 0, NONE, 0)
    # Z: the local z = -8 of Q fails z >= -1 (its placed z = -5 fails too), the local z = 8 of S passes
    assert canon(answer(152.0, 110.0, mirror_axis=3, mirror_threshold=1.0)) == none
    assert canon(answer(168.0, 120.0, mirror_axis=3, mirror_threshold=1.0)) == (1, 0, NONE, NONE, 0, NONE, 0)


def test_ref_hover_hand_cases():
    """Identity camera, 320x240, UNIT_ORTHO: a vertex (x, y, z) lands at (x + 160, 120 - y) with depth z.  The triangle A = (0, 0, 2),
    B = (8, 0, 4), C = (0, -8, 6) is (160, 120), (168, 120), (160, 128), signed area 8 * 8 = 64 > 0: front.
      cursor ON A: vertex 0 at distance 0; the half-edges A->B and C->A (and B->A, A->F of the third polygon) pass through it (distance 0;
        the first, (0, 1), stays), B->C is 8 / sqrt 2 = 5.66 away; the face is hit with depth 2.
      cursor (154, 120): 6.0 from A -- `dist < 6.0` is false: no vertex (B is 14 away), no edge (t clamps to 0: 6.0 >= 4.0), no face.
      cursor (155, 120): vertex 0 at 5.0.
      cursor (164, 116): 4.0 above the middle of AB (t = 0.5, projection (164, 120)): `dist < 4.0` is false, and B->C, C->A are farther: no
        edge; A and B are both sqrt(32) = 5.657 away: two candidates, the first stays.  (164, 117): edge (0, 1) at 3.0.
      a zero-length edge: the polygon (3, 4) of two vertices at the same place (20, 0, 1) -> (180, 120); len_sq = 0 < 0.001, so the distance is
        that to its first end: cursor (180, 123) -> edge (3, 4) at 3.0 (see-through: a polygon of two vertices is never front, so with culling
        there is neither edge nor vertex); cursor (183, 124): 5.0 -- no edge, but vertex 3.
      the reversed duplicate: (0, 1, 2) and (1, 0, 5), F = (4, 40, 3) -> (164, 80), share the edge as 0 -> 1 and 1 -> 0; cursor (164, 117) is
        exactly 3.0 from both: the first stays and the pair is reported normalised, (0, 1); A->F and F->B are 148 / sqrt(1616) = 3.68 away.
      The cursors at exactly 6.0 and 4.0 are read on the mesh without that third polygon (A->F passes within 4.0 of them).
      a placed vertex that passes the mirror test locally and fails it where it is placed, and one the other way round: see
        placed_mirror_mesh and _placed_mirror_checks."""
    W, H = 320, 240
    v, polys = _mesh([(0, 0, 2), (8, 0, 4), (0, -8, 6), (20, 0, 1), (20, 0, 1), (4, 40, 3)], [(0, 1, 2), (3, 4), (1, 0, 5)])
    hov = lambda mx, my, **kw: ref_hover(v["pos"], polys, None, IDENTITY_CAM, W, H, mx, my, UNIT_ORTHO, **kw)
    hov2 = lambda mx, my, **kw: ref_hover(v["pos"], polys[:2], None, IDENTITY_CAM, W, H, mx, my, UNIT_ORTHO, **kw)
    rm = RefMesh(v["pos"], polys, None, IDENTITY_CAM, W, H, UNIT_ORTHO)
    assert rm.sv[:3] == [(160.0, 120.0, 2.0), (168.0, 120.0, 4.0), (160.0, 128.0, 6.0)] and rm.sv[3] == rm.sv[4] == (180.0, 120.0, 1.0)
    assert rm.vertex_on_front_face == [True, True, True, False, False, True]
    assert rm.edge_on_front_face == {(0, 1), (1, 2), (0, 2), (0, 5), (1, 5)}
    r = hov(160.0, 120.0)
    assert canon(r) == (0, 0, 0, 1, 0, 0, _bits(2.0)) and [c[0] for c in r["ecands"]] == [0, 2, 5, 6]
    assert [c[0] for c in hov2(160.0, 120.0)["ecands"]] == [0, 2]
    assert ref_hovered_element(r) == (0, None, None)
    assert canon(hov2(154.0, 120.0)) == (NONE, 0, NONE, NONE, 0, NONE, 0)
    assert canon(hov2(155.0, 120.0))[:2] == (0, _bits(5.0))
    r = hov2(164.0, 116.0)
    assert r["vertex"] == 0 and _bits(r["vertex_dist"]) == _bits(np.sqrt(f32(32.0))) and [c[0] for c in r["vcands"]] == [0, 1]
    assert r["edge_v0"] == NONE and r["edge_dist"] == 0.0
    r = hov(164.0, 117.0)
    assert (r["edge_v0"], r["edge_v1"], _bits(r["edge_dist"])) == (0, 1, _bits(3.0))
    assert [(o, float(d)) for o, d in r["ecands"][:2]] == [(0, 3.0), (5, 3.0)]                 # 0 -> 1, and 1 -> 0 of the third polygon
    assert [o for o, d in r["ecands"][2:]] == [6, 7] and all(3.67 < d < 3.69 for _, d in r["ecands"][2:])
    r2 = hov2(164.0, 117.0)
    assert (r2["edge_v0"], r2["edge_v1"], _bits(r2["edge_dist"])) == (0, 1, _bits(3.0)) and [c[0] for c in r2["ecands"]] == [0]
    assert canon(hov(180.0, 123.0))[:5] == (NONE, 0, NONE, NONE, 0)                              # culling: the 2-gon is never front
    r = hov(180.0, 123.0, see_through=True)
    assert (r["vertex"], r["edge_v0"], r["edge_v1"], _bits(r["edge_dist"])) == (3, 3, 4, _bits(3.0))
    assert [c[0] for c in r["ecands"]] == [3, 4]
    r = hov(183.0, 124.0, see_through=True)
    assert (r["vertex"], _bits(r["vertex_dist"]), r["edge_v0"]) == (3, _bits(5.0), NONE)
    assert ref_hovered_element(hov(164.0, 117.0, vertex_threshold=2.0)) == (None, (0, 1), None)
    assert ref_hovered_element(hov(162.0, 123.0, vertex_threshold=2.0, edge_threshold=1.0)) == (None, None, 0)
    # the mirror test reads the LOCAL position: x >= -threshold; a NaN threshold lets nothing through
    assert hov(160.0, 120.0, mirror_axis=1, mirror_threshold=0.0)["vertex"] == 0
    assert canon(hov2(160.0, 120.0, mirror_axis=2, mirror_threshold=7.5)) == (0, 0, 0, 1, 0, NONE, 0)     # C.y = -8 fails: C->A and the face go
    assert canon(hov(160.0, 120.0, mirror_axis=3, mirror_threshold=np.nan)) == (NONE, 0, NONE, NONE, 0, NONE, 0)
    pv, ppolys = placed_mirror_mesh()
    prm = RefMesh(pv["pos"], ppolys, PLACEMENTS[3], IDENTITY_CAM, W, H, UNIT_ORTHO)
    assert prm.sv == [(152.0, 110.0, -5.0), (168.0, 120.0, 5.0)]
    _placed_mirror_checks(lambda mx, my, **kw: prm.hover(mx, my, see_through=True, **kw))
    wrong = WorldSpaceMirrorRefMesh(pv["pos"], ppolys, PLACEMENTS[3], IDENTITY_CAM, W, H, UNIT_ORTHO)       # the placed position: the other vertex
    assert wrong.hover(152.0, 110.0, see_through=True, mirror_axis=1)["vertex"] == NONE
    assert wrong.hover(168.0, 120.0, see_through=True, mirror_axis=1)["vertex"] == 1
    # point_to_line_distance: the clamp keeps -0.0 and a NaN
    assert _bits(point_to_line_distance(f32(0), f32(5), f32(0), f32(0), f32(10), f32(0))) == _bits(5.0)
    assert np.isnan(point_to_line_distance(f32(0), f32(5), f32(np.nan), f32(0), f32(10), f32(0)))
    # box selection: inclusive bounds, an empty and a NaN rectangle, the polygons' centres
    box = lambda rect, mode: ref_box_select(v["pos"], polys, None, IDENTITY_CAM, W, H, rect, mode, UNIT_ORTHO)
    assert box((160.0, 120.0, 168.0, 120.0), 0) == [0, 1] and box((160.0, 120.0, 167.99, 128.0), 0) == [0, 2]
    assert box((168.0, 0.0, 160.0, 240.0), 0) == [] and box((np.nan, 0.0, 320.0, 240.0), 0) == [] and box((0.0, 0.0, 320.0, 240.0), 0) == [0, 1, 2, 3, 4, 5]
    third = f32(1.0) / f32(3.0)
    cx, cy = (f32(0) + f32(0) + f32(8) + f32(0)) * third + f32(160.0), -((f32(0) + f32(0) + f32(0) + f32(-8)) * third) + f32(120.0)
    assert box((cx, cy, cx, cy), 1) == [0] and box((180.0, 120.0, 180.0, 120.0), 1) == [1]
    assert box((0.0, 0.0, 320.0, 240.0), 1) == [0, 1, 2]


def test_topology_helper():
    """rasterizer.Topology derives half-edges, edge ids and fan triangles in the reference's loop order."""
    from bonnie32_amd.rasterizer import Topology
    polys = [[0, 1, 2, 3], [], [4], [1, 0], [2, 1, 5, 6, 7]]
    t = Topology.from_polygons(polys)
    assert list(zip(t.he_v0, t.he_v1)) == [e for p in polys for e in face_edges(p)]
    assert [tuple(r) for r in t.fan] == [tr for p in polys for tr in face_triangulate(p)]
    assert list(t.fan_poly) == [0, 0, 4, 4, 4]
    norm = [(min(a, b), max(a, b)) for p in polys for a, b in face_edges(p)]
    assert t.ne == len(set(norm)) and all((t.he_edge[i] == t.he_edge[j]) == (norm[i] == norm[j]) for i in range(len(norm)) for j in range(len(norm)))
    tri = Topology.triangles(np.array([[0, 1, 2], [2, 1, 3]], np.uint32))
    assert list(tri.poly_start) == [0, 3, 6] and list(tri.poly_verts) == [0, 1, 2, 2, 1, 3]
    with pytest.raises(ValueError):
        Topology([1, 3], [0, 1, 2])
    with pytest.raises(ValueError):
        Topology([0, 3, 2], [0, 1, 2])


def _mirror_equals_ref(vertices, polys, top, camera, w, h, curs, placements=(None,), orthos=(None,), modes=(False, True), mirrors=((0, 1.0),)):
    """HoverMirror == ref_hover on every branch for every cursor; returns {(placement index, ortho, see_through, mirror): [ref answers]}."""
    from bonnie32_amd.rasterizer import HoverMirror, hovered_element
    out = {}
    for pi, pl in enumerate(placements):
        for ortho in orthos:
            rm = RefMesh(vertices["pos"], polys, pl, camera, w, h, ortho)
            hm = HoverMirror(vertices, top, pl, camera, w, h, ortho)
            for see in modes:
                for axis, thr in mirrors:
                    rows = []
                    for mx, my in curs:
                        want = rm.hover(mx, my, see_through=see, mirror_axis=axis, mirror_threshold=thr)
                        got = hm.hover(mx, my, see_through=see, mirror_axis=axis, mirror_threshold=thr)
                        assert canon(got) == canon(want), (pi, ortho, see, axis, thr, mx, my, got, want)
                        assert hovered_element(got) == ref_hovered_element(want)
                        rows.append(want)
                    out[(pi, ortho, see, (axis, thr))] = rows
    return out


def _floors(rows_cull, rows_see):
    hit = lambda r, k: r[k] != NONE
    multi = sum(len(r["vcands"]) >= 2 for r in rows_cull) if isinstance(rows_cull[0], dict) else None        # (the restatement lists its candidates)
    return dict(vertex_hits=sum(hit(r, "vertex") for r in rows_cull), multi=multi,
                edge_no_vertex=sum(hit(r, "edge_v0") and not hit(r, "vertex") for r in rows_cull), face_hits=sum(hit(r, "face") for r in rows_cull),
                vertex_differs=sum(canon(a)[:2] != canon(b)[:2] for a, b in zip(rows_cull, rows_see)),
                edge_differs=sum(canon(a)[2:5] != canon(b)[2:5] for a, b in zip(rows_cull, rows_see)))


FLOORS = {"obj-warrior": dict(vertex_hits=60, multi=30, edge_no_vertex=10, face_hits=60, vertex_differs=15, edge_differs=20),
          "asset3-part0-game": dict(vertex_hits=15, edge_no_vertex=40, vertex_differs=10)}


# under PLACEMENTS[2], see-through, mirror on X with threshold 0.0, perspective and ORTHO together: the cursors (of 2 * 96) at which the
# mirror test on the placed position would answer differently.  Measured on the restatement: 82, 160 and 38.
LOCAL_NOT_WORLD_FLOORS = {"obj-warrior": 40, "asset3-part0-game": 80, "C1": 15}


def _placed_answers_differ(name, v, polys, sc, curs, rows_by_ortho):
    """How many of ref_hover's answers under PLACEMENTS[2] (rows_by_ortho: {ortho: rows}, mirror X / 0.0, see-through) a mirror test on
    the placed position would change."""
    n = 0
    for ortho, rows in rows_by_ortho.items():
        wrong = WorldSpaceMirrorRefMesh(v["pos"], polys, HOVER_PLACEMENTS[1], sc.camera, sc.width, sc.height, ortho)
        n += sum(canon(wrong.hover(mx, my, see_through=True, mirror_axis=1, mirror_threshold=0.0)) != canon(r) for (mx, my), r in zip(curs, rows))
    return n


@pytest.mark.parametrize("pi", [0, 1, 2])
@pytest.mark.parametrize("name", ["obj-warrior", "asset3-part0-game", "C1"])
def test_host_mirror_equals_ref_hover(name, pi):
    """HoverMirror == ref_hover on the 96 cursors over the whole grid: perspective and ORTHO, culling and see-through, the mirror off and
    all three axes with thresholds 1.0, 0.0 and NaN, for one of NULL placement and two placements (the infinite one included).  The floors
    are asserted on the reference's own answers, so that the comparison cannot pass on "none" == "none": the issue's (perspective, NULL
    placement), and under the finite placement the number of answers that a mirror test on the placed position would change."""
    sc, v, polys, top, curs = hover_scene(name)
    if name == "obj-warrior":
        assert len(polys) == 442 and sum(len(p) == 4 for p in polys) == 8
    if name == "asset3-part0-game":
        assert sum(len(p) == 4 for p in polys) == 10
    res = _mirror_equals_ref(v, polys, top, sc.camera, sc.width, sc.height, curs, (HOVER_PLACEMENTS[pi],), (None, ORTHO), mirrors=MIRROR_GRID)
    nan_rows = [r for key, rows in res.items() if np.isnan(key[3][1]) for r in rows]
    assert len(nan_rows) == 2 * 2 * 3 * 96
    assert all(canon(r) == (NONE, 0, NONE, NONE, 0, NONE, 0) for r in nan_rows)             # a NaN threshold: nothing is editable
    if pi == 0:
        fl = _floors(res[(0, None, False, (0, 1.0))], res[(0, None, True, (0, 1.0))])
        print(name, fl)
        for k, least in FLOORS.get(name, {}).items():
            assert fl[k] >= least, (name, fl)
        base = res[(0, None, True, (0, 1.0))]
        changed = sum(canon(a) != canon(b) for key, rows in res.items() if key[1] is None and key[2] and key[3][0] for a, b in zip(rows, base))
        assert changed >= 24, changed                                                        # (the NaN thresholds alone give that many)
    if pi == 1:
        n = _placed_answers_differ(name, v, polys, sc, curs, {o: res[(0, o, True, (1, 0.0))] for o in (None, ORTHO)})
        print(name, "answers that a mirror test on the placed position would change:", n)
        assert n >= LOCAL_NOT_WORLD_FLOORS[name], (name, n)


def _order_checks(name, answer):
    """What must hold for an order case; answer(mx, my, see_through) -> a comparable record."""
    v, polys = order_mesh(name)
    first = 1 if name.endswith("first") else 0                       # a polygon in front shifts the indices
    P = lambda i: i + first
    if name in ("base", "nan_last", "inf_last", "same_thrice_last"):
        r = answer(171.0, 110.0, True)
        assert (r["vertex"], _bits(r["vertex_dist"])) == (5, _bits(1.0))                     # coincident vertices: the lowest index
        assert answer(171.0, 110.0, False)["vertex"] == NONE                                 # ... on no polygon: only see-through
        assert answer(41.0, 41.0, False)["vertex"] == NONE and answer(41.0, 41.0, False)["edge_v0"] == NONE      # back faces only
        r = answer(41.0, 41.0, True)
        assert r["vertex"] == 30 and (r["edge_v0"], r["edge_v1"]) in ((30, 32), (30, 31))
        r = answer(60.0, 171.0, True)                                                        # the polygon of one vertex: the edge (40, 40)
        assert (r["vertex"], r["edge_v0"], r["edge_v1"], _bits(r["edge_dist"])) == (40, 40, 40, _bits(1.0))
        r = answer(90.0, 172.0, True)                                                        # the polygon of two
        assert (r["vertex"], r["edge_v0"], r["edge_v1"], _bits(r["edge_dist"])) == (NONE, 41, 42, _bits(2.0))
        assert canon(answer(90.0, 172.0, False))[:5] == (NONE, 0, NONE, NONE, 0) and canon(answer(60.0, 171.0, False))[:5] == (NONE, 0, NONE, NONE, 0)
        if name != "same_thrice_last":
            for see in (False, True):
                r = answer(200.0, 180.0, see)                                                # five and six vertices: the POLYGON index
                assert (r["vertex"], r["edge_v0"], r["face"]) == (NONE, NONE, P(405))
                assert answer(260.0, 180.0, see)["face"] == P(406)
                if name == "base":                                                           # an index out of range: skipped whole
                    assert answer(210.0, 50.0, see)["face"] == NONE and answer(260.0, 50.0, see)["face"] == NONE
        assert answer(201.0, 41.0, False)["vertex"] == 70 and answer(251.0, 41.0, False)["vertex"] == 73         # ... but its vertices are front
        assert answer(201.0, 41.0, False)["edge_v0"] == 70 and answer(201.0, 41.0, False)["edge_v1"] == 71
        assert answer(200.0, 55.0, True)["edge_v0"] == NONE                                  # (72, nv) and (nv, 70) are no edges
        assert answer(201.0, 91.0, False)["vertex"] == NONE and answer(201.0, 91.0, True)["vertex"] == 76        # first index out of range: not front
    if name == "nan_first":
        for mx, my in ORDER_CURSORS[::5]:
            for see in (False, True):
                r = answer(mx, my, see)
                assert r["face"] == 0 and np.isnan(r["face_depth"])                          # the sticky NaN, from every cursor
    if name == "inf_first":
        # the vertex (inf, 0, 1000) does not land at (inf, 120): the camera's dot products multiply the inf by the zeros of the other basis
        # vectors, so it projects to (inf, NaN) with a NaN depth.  Every sign of point_in_triangle_2d of polygon 0 is then a NaN, neither
        # negative nor positive: a hit from every cursor, and the NaN area is kept by the face loop (`<= 0.0`) with culling too.  The
        # depth is a NaN, and as the first polygon it stays: what "nan_first" gives.  No vertex or edge comes of it (inf and NaN distances).
        sv = RefMesh(v["pos"], polys, None, IDENTITY_CAM, 320, 240, UNIT_ORTHO).sv[90]
        assert np.isposinf(sv[0]) and np.isnan(sv[1]) and np.isnan(sv[2])
        for mx, my in ORDER_CURSORS[::5] + [(300.0, 10.0), (10.0, 200.0)]:
            for see in (False, True):
                r = answer(mx, my, see)
                assert r["face"] == 0 and np.isnan(r["face_depth"])
        r = answer(300.0, 10.0, True)
        assert (r["vertex"], r["edge_v0"]) == (NONE, NONE)
        r = answer(115.0, 100.0, False)                               # inside (20, 21, 22), now polygon 1: its vertices and edges are front
        assert (r["vertex"], r["edge_v0"], r["edge_v1"]) == (20, 20, 21)
    if name == "nan_last":
        base = RefMesh(order_mesh("base")[0]["pos"], order_mesh("base")[1], None, IDENTITY_CAM, 320, 240, UNIT_ORTHO)
        for mx, my in ORDER_CURSORS[::3]:
            b, r = base.hover(mx, my, see_through=True), answer(mx, my, True)
            if b["face"] != NONE:
                assert (r["face"], _fbits(r["face_depth"])) == (b["face"], _fbits(b["face_depth"]))      # a NaN behind a number is ignored
            else:
                assert r["face"] == len(polys) - 1 and np.isnan(r["face_depth"])             # ... unless it is the only hit
    if name == "same_thrice_last":
        assert all(answer(mx, my, True)["face"] != NONE for mx, my in ORDER_CURSORS[::4])    # (i, i, i) is hit from every cursor
        r = answer(300.0, 10.0, True)
        assert (r["face"], _bits(r["face_depth"])) == (len(polys) - 1, _bits(5.0))
        assert answer(300.0, 10.0, False)["face"] == NONE                                    # area 0 <= 0: culled


def _edge_pair_checks(answer):
    """The edge (20, 21) as half-edge 0 (20 -> 21) and half-edge 1232 (21 -> 20): equal distances keep the first, a strictly smaller later one
    replaces it; the reported distance is the winner's own."""
    v, polys = order_mesh("base")
    rm = RefMesh(v["pos"], polys, None, IDENTITY_CAM, 320, 240, UNIT_ORTHO)
    a, b = rm.sv[20], rm.sv[21]
    n_equal = n_first = n_second = 0
    with np.errstate(all="ignore"):
        for mx, my in edge_scan_cursors():
            mxf, myf = f32(mx), f32(my)
            d_fwd = point_to_line_distance(mxf, myf, a[0], a[1], b[0], b[1])
            d_rev = point_to_line_distance(mxf, myf, b[0], b[1], a[0], a[1])
            if not set(o for o, _ in rm.hover(mx, my)["ecands"]) <= {0, 1232} or not (d_fwd < f32(4.0) or d_rev < f32(4.0)):
                continue                                                                     # (another edge is a candidate too, or none is)
            r = answer(mx, my, False)
            want = d_rev if (d_rev < f32(4.0) and (not d_fwd < f32(4.0) or d_rev < d_fwd)) else d_fwd
            assert (r["edge_v0"], r["edge_v1"], _bits(r["edge_dist"])) == (20, 21, _bits(want)), (mx, my, d_fwd, d_rev, r)
            n_equal += _bits(d_fwd) == _bits(d_rev); n_first += d_fwd < d_rev; n_second += d_rev < d_fwd
    return n_equal, n_first, n_second


def test_order_cases_on_the_host():
    """The order cases in ref_hover terms, and HoverMirror == ref_hover on each of their meshes."""
    from bonnie32_amd.rasterizer import HoverMirror, Topology
    v, polys = placed_mirror_mesh()
    hm = HoverMirror(v, Topology.from_polygons(polys), PLACEMENTS[3], IDENTITY_CAM, 320, 240, UNIT_ORTHO)
    _placed_mirror_checks(lambda mx, my, **kw: hm.hover(mx, my, see_through=True, **kw))
    for name in ORDER_VARIANTS:
        v, polys = order_mesh(name)
        rm = RefMesh(v["pos"], polys, None, IDENTITY_CAM, 320, 240, UNIT_ORTHO)
        _order_checks(name, lambda mx, my, see: rm.hover(mx, my, see_through=see))
        _mirror_equals_ref(v, polys, Topology.from_polygons(polys), IDENTITY_CAM, 320, 240, ORDER_CURSORS, orthos=(UNIT_ORTHO,))
    v, polys = order_mesh("base")
    t = Topology.from_polygons(polys)
    assert (t.he_v0[0], t.he_v1[0]) == (20, 21) and (t.he_v0[1232], t.he_v1[1232]) == (21, 20) and t.he_edge[0] == t.he_edge[1232]
    rm = RefMesh(v["pos"], polys, None, IDENTITY_CAM, 320, 240, UNIT_ORTHO)
    assert rm.vertex_on_front_face[50] and rm.vertex_on_front_face[65] and rm.vertex_on_front_face[20] and not rm.vertex_on_front_face[30]
    counts = _edge_pair_checks(lambda mx, my, see: rm.hover(mx, my, see_through=see))
    print("edge pair: equal, first smaller, second smaller:", counts)
    assert counts[0] >= 1 and counts[1] >= 1 and counts[2] >= 1, counts     # each rule is met: a tie, the first smaller, the later one smaller
    _mirror_equals_ref(v, polys, t, IDENTITY_CAM, 320, 240, edge_scan_cursors(), orthos=(UNIT_ORTHO,), modes=(False,))


def _box_cases(sc, v, polys, placement, ortho, mode):
    """[(rectangle, must select this index or None)] for one scene, placement, projection and mode."""
    cam = _cam_f32(sc.camera)
    world = ref_world_positions(v["pos"], placement)
    with np.errstate(all="ignore"):
        if mode == abi.BOX_VERTICES:
            pts = [ref_world_to_screen_with_ortho(p, cam, sc.width, sc.height, ortho) for p in world]
        else:
            pts = []
            for vs in polys:
                ps = [world[i] for i in vs if i < len(world)]
                acc = (f32(0.0), f32(0.0), f32(0.0))
                for p in ps:
                    acc = (acc[0] + p[0], acc[1] + p[1], acc[2] + p[2])
                k = f32(1.0) / f32(max(len(ps), 1))
                pts.append(ref_world_to_screen_with_ortho((acc[0] * k, acc[1] * k, acc[2] * k), cam, sc.width, sc.height, ortho) if ps else None)
    fin = [(i, p) for i, p in enumerate(pts) if p is not None and np.isfinite(p[0]) and np.isfinite(p[1])]
    W, H = float(sc.width), float(sc.height)
    cases = [((0.0, 0.0, W, H), None), ((W, 0.0, 0.0, H), None), ((0.0, np.nan, W, H), None)]
    if fin:
        i, p = fin[len(fin) // 3]
        cases.append(((p[0], p[1], p[0], p[1]), i))
        xs = sorted(float(q[0]) for _, q in fin); ys = sorted(float(q[1]) for _, q in fin)
        cases.append(((xs[len(xs) // 4], ys[len(ys) // 5], xs[(3 * len(xs)) // 4], ys[(4 * len(ys)) // 5]), None))
    return cases


@pytest.mark.parametrize("name", ["obj-warrior", "asset3-part0-game", "C1"])
def test_host_box_select_equals_ref(name):
    """box_select_mesh == ref_box_select, both modes, the five rectangles, perspective and ORTHO, NULL placement and a placed copy; at
    least one rectangle per scene and mode selects more than none and fewer than all."""
    from bonnie32_amd.rasterizer import box_select_mesh
    sc, v, polys, top, _ = hover_scene(name)
    for mode in (abi.BOX_VERTICES, abi.BOX_POLYGONS):
        n = len(v) if mode == abi.BOX_VERTICES else len(polys)
        partial = 0
        for pl in (None, PLACEMENTS[1]):
            for ortho in (None, ORTHO):
                for rect, must in _box_cases(sc, v, polys, pl, ortho, mode):
                    want = ref_box_select(v["pos"], polys, pl, sc.camera, sc.width, sc.height, rect, mode, ortho)
                    words, cnt = box_select_mesh(v, top, pl, sc.camera, sc.width, sc.height, rect, mode, ortho)
                    assert cnt == len(want) and np.array_equal(words, words_of(want, n)), (name, mode, pl, ortho, rect)
                    assert must is None or must in want
                    partial += pl is None and 0 < len(want) < n
        assert partial >= 1, (name, mode)


def test_cpp_mirror_hover_compiles():
    """host/rasterizer.hpp: Topology, the hover and box-selection wrappers, their host restatements, hovered_element and FrameLoop's hover
    compile (header-only over the C ABI)."""
    hpp_dir = os.path.join(ROOT, "bonnie-32_amd", "host")
    src = ('#include "rasterizer.hpp"\nvoid f(b32::Framebuffer& fb, b32::ResidentMesh& a, const b32::Camera& cam, const std::vector<b32::Vertex>& v, const std::vector<b32::Face>& fc,\n'
           '       const b32::RasterSettings& st) {\n'
           ' b32::Topology top = b32::Topology::triangles(fb, fc); b32::Topology quads(fb, { 0, 4 }, { 0, 1, 2, 3 });\n'
           ' B32HoverResult r = b32::hover_mesh(fb, a, top, cam, b32::hover_params(1.0f, 2.0f));\n'
           ' r = b32::hover_mesh(fb, a, quads, cam, b32::hover_params(1.0f, 2.0f, true, 1, 0.5f), b32::Vec3{ 1, 0, 0 }, b32::Placement{});\n'
           ' const b32::HoveredElement e = b32::hovered_element(r); (void)e.vertex.has_value(); (void)e.edge.has_value(); (void)e.face.has_value();\n'
           ' void* out = b32_host_alloc(32); const uint64_t t = b32::hover_mesh_async(fb, a, top, cam, b32::hover_params(1.0f, 2.0f), out);\n'
           ' b32::check(b32_ticket_wait(fb.ctx(), t), "wait"); b32_host_free(out);\n'
           ' b32::BoxSelection s = b32::box_select(fb, a, &top, cam, 0, 0, 10, 10, B32_BOX_POLYGONS, top.polygons()); (void)s.n_selected;\n'
           ' s = b32::box_select(fb, a, nullptr, cam, 0, 0, 10, 10, B32_BOX_VERTICES, v.size()); (void)s.test(0);\n'
           ' const std::vector<uint32_t> ps{ 0, 3 }, pv{ 0, 1, 2 };\n'
           ' r = b32::hover_mesh(v, ps, pv, std::nullopt, cam, 320, 240, b32::hover_params(1.0f, 2.0f));\n'
           ' s = b32::box_select(v, ps, pv, b32::Placement{}, cam, 320, 240, 0, 0, 10, 10, B32_BOX_VERTICES, b32::Vec3{ 1, 0, 0 });\n'
           ' b32::FrameLoop loop(fb); b32::FrameHover hv{ &a, &top, b32::hover_params(3.0f, 4.0f) };\n'
           ' const uint64_t ft = loop.submit(b32::Color{}, { { &a, b32::MeshParams{ 0.5f, true, false, std::nullopt } } }, cam, st, nullptr, &hv);\n'
           ' (void)loop.wait(ft); (void)loop.wait_hover(ft).vertex; }\n'
           'int main() { (void)&f; return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", hpp_dir, "-I", os.path.join(ROOT, "include"),
                        os.path.join(d, "t.cpp")], check=True)


def test_cpp_host_restatement_equals_ref(tmp_path):
    """tests/cpp/hover_host.cpp: the C++ host restatements (hover_mesh / box_select over vectors, compiled without contraction, no device)
    on the order mesh against ref_hover and ref_box_select."""
    exe = tmp_path / "hover_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "bonnie-32_amd", "host"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "hover_host.cpp"), "-o", str(exe)], check=True)
    v, polys = order_mesh("nan_last")
    mesh = tmp_path / "mesh.txt"
    with open(mesh, "w") as fh:
        fh.write(f"{len(v)} {len(polys)}\n")
        for p in v["pos"]:
            fh.write(" ".join("%08x" % _bits(x) for x in p) + "\n")
        for vs in polys:
            fh.write(" ".join([str(len(vs))] + [str(i) for i in vs]) + "\n")
    curs = ORDER_CURSORS[:24] + edge_scan_cursors()[:16]
    rm = RefMesh(v["pos"], polys, None, IDENTITY_CAM, 320, 240, UNIT_ORTHO)
    for see in (0, 1):
        r = subprocess.run([str(exe), str(mesh), str(see)] + [repr(float(f32(c))) for cur in curs for c in cur], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.strip().splitlines()
        assert len(lines) == len(curs) + 2
        for (mx, my), line in zip(curs, lines):
            t = line.split()
            got = dict(vertex=int(t[0]), vertex_dist=np.array([int(t[1], 16)], np.uint32).view(f32)[0], edge_v0=int(t[2]), edge_v1=int(t[3]),
                       edge_dist=np.array([int(t[4], 16)], np.uint32).view(f32)[0], face=int(t[5]), face_depth=np.array([int(t[6], 16)], np.uint32).view(f32)[0])
            assert canon(got) == canon(rm.hover(mx, my, see_through=bool(see))), (see, mx, my, line)
        for mode, line in zip((0, 1), lines[len(curs):]):
            want = ref_box_select(v["pos"], polys, None, IDENTITY_CAM, 320, 240, (30.0, 30.0, 210.0, 175.0), mode, UNIT_ORTHO)
            assert [int(x) for x in line.split()] == want and len(want) >= 3


# ================================================================== on the GPU
def _device_equals_mirror(ctx, rs, vertices, top, camera, w, h, curs, placements=(None,), orthos=(None,), modes=(False, True), mirrors=((0, 1.0),)):
    """b32_hover_mesh == HoverMirror on every branch for every cursor; returns the mirror's answers like _mirror_equals_ref."""
    from bonnie32_amd.rasterizer import HoverMirror
    out = {}
    for pi, pl in enumerate(placements):
        for ortho in orthos:
            hm = HoverMirror(vertices, top, pl, camera, w, h, ortho)
            for see in modes:
                for axis, thr in mirrors:
                    rows = []
                    for mx, my in curs:
                        want = hm.hover(mx, my, see_through=see, mirror_axis=axis, mirror_threshold=thr)
                        got = ctx.hover_mesh(rs, top, camera, (mx, my), ortho, pl, see_through=see, mirror_axis=axis, mirror_threshold=thr)
                        assert canon(got) == canon(want), (pi, ortho, see, axis, thr, mx, my, got, want)
                        if np.isnan(want["face_depth"]):
                            assert _bits(got["face_depth"]) == 0x7FC00000
                        rows.append(want)
                    out[(pi, ortho, see, (axis, thr))] = rows
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pi", [0, 1, 2])
@pytest.mark.parametrize("name", ["obj-warrior", "asset3-part0-game", "C1"])
def test_gpu_hover_scenes(gpu_ctx, name, pi):
    """b32_hover_mesh == HoverMirror over the whole grid of the host test, one placement per case; C1 whole (6 000 vertices and 6 000
    half-edges: six workgroups per range, the last one partial).  Under the finite placement the mirror's answers with the mirror test on
    are asserted to be answers: enough of them hit, and a mirror test on the placed position would change enough of them."""
    from bonnie32_amd import rasterizer as R
    sc, v, polys, top, curs = hover_scene(name, whole=True)
    if name == "C1":
        assert len(v) == 6000 and len(top.poly_verts) == 6000
        hm0 = R.HoverMirror(v, top, None, sc.camera, sc.width, sc.height)                    # ... and cursors at vertices of all six workgroups
        ok = np.nonzero(hm0.some)[0]
        curs = curs + [(float(hm0.sx[i]) + 1.0, float(hm0.sy[i]) - 0.5) for i in ok[(np.arange(24) * 251) % len(ok)]]
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    try:
        res = _device_equals_mirror(gpu_ctx, rs, v, top, sc.camera, sc.width, sc.height, curs, (HOVER_PLACEMENTS[pi],), (None, ORTHO), mirrors=MIRROR_GRID)
    finally:
        rs.close(); top.close()
    if pi == 0:
        fl = _floors(res[(0, None, False, (0, 1.0))], res[(0, None, True, (0, 1.0))])
        print(name, fl)
        for k, least in FLOORS.get(name, {}).items():
            assert k == "multi" or fl[k] >= least, (name, fl)
        if name == "C1":
            assert fl["vertex_hits"] >= 20 and len({int(r["vertex"]) // 1024 for r in res[(0, None, True, (0, 1.0))] if r["vertex"] != NONE}) >= 3
    if pi == 1:
        if name == "C1":                                                                     # (the floor is that of the first 256 faces)
            sc, v, polys, top, curs = hover_scene(name)
            hms = {o: R.HoverMirror(v, top, HOVER_PLACEMENTS[1], sc.camera, sc.width, sc.height, o) for o in (None, ORTHO)}
            rows = {o: [hm.hover(mx, my, see_through=True, mirror_axis=1, mirror_threshold=0.0) for mx, my in curs] for o, hm in hms.items()}
        else:
            rows = {o: res[(0, o, True, (1, 0.0))] for o in (None, ORTHO)}
        n = _placed_answers_differ(name, v, polys, sc, curs, rows)
        assert n >= LOCAL_NOT_WORLD_FLOORS[name], (name, n)


@pytest.mark.gpu
def test_gpu_hover_order_cases(gpu_ctx):
    """The order cases on the device: the coincident vertices sit in three workgroups of the vertex range, the two half-edges of one edge
    in two of the half-edge range.  First the placed vertex that passes the mirror test locally and fails it where it is placed."""
    from bonnie32_amd import rasterizer as R
    from bonnie32_amd.rasterizer import Topology
    fb = R.Framebuffer(320, 240, gpu_ctx)
    v, polys = placed_mirror_mesh()
    top = Topology.from_polygons(polys)
    rs = R.ResidentScene(fb, v, b32.make_faces(0), []).detach()
    try:
        _placed_mirror_checks(lambda mx, my, **kw: gpu_ctx.hover_mesh(rs, top, IDENTITY_CAM, (mx, my), UNIT_ORTHO, PLACEMENTS[3], see_through=True, **kw))
    finally:
        rs.close(); top.close()
    for name in ORDER_VARIANTS:
        v, polys = order_mesh(name)
        top = Topology.from_polygons(polys)
        rs = R.ResidentScene(fb, v, b32.make_faces(0), []).detach()
        try:
            answer = lambda mx, my, see: gpu_ctx.hover_mesh(rs, top, IDENTITY_CAM, (mx, my), UNIT_ORTHO, None, see_through=see)
            _order_checks(name, answer)
            _device_equals_mirror(gpu_ctx, rs, v, top, IDENTITY_CAM, 320, 240, ORDER_CURSORS, orthos=(UNIT_ORTHO,))
            if name == "base":
                assert len({i // 1024 for i in A_IDX}) == 3 and 1232 // 1024 != 0
                counts = _edge_pair_checks(answer)
                assert counts[0] >= 1 and counts[1] >= 1 and counts[2] >= 1, counts
        finally:
            rs.close(); top.close()


@pytest.mark.gpu
def test_gpu_hover_rearms_between_calls():
    """On one context: culling, see-through, culling with different cursors, then a second, smaller topology (and a smaller mesh): each answer
    is its own mirror's, so the bitmaps and the words are clear between calls."""
    from bonnie32_amd import rasterizer as R
    from bonnie32_amd.rasterizer import HoverMirror, Topology
    sc, v, polys, top, curs = hover_scene("obj-warrior")
    ctx = R.Context(0)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    sv, spolys = _mesh([(0, 0, 2), (8, 0, 4), (0, -8, 6), (30, 30, 3)], [(0, 1, 2)])
    stop = Topology.from_polygons(spolys)
    srs = R.ResidentScene(fb, sv, b32.make_faces(0), []).detach()
    try:
        hm = HoverMirror(v, top, None, sc.camera, sc.width, sc.height)
        small = HoverMirror(sv, stop, None, IDENTITY_CAM, sc.width, sc.height, UNIT_ORTHO)
        hx, hy = sc.width / 2.0, sc.height / 2.0
        n_hits = 0
        for k in range(0, 90, 3):
            for see, cur in ((False, curs[k]), (True, curs[k + 1]), (False, curs[k + 2])):
                want = hm.hover(*cur, see_through=see)
                assert canon(ctx.hover_mesh(rs, top, sc.camera, cur, see_through=see)) == canon(want), (k, see, cur)
                n_hits += want["vertex"] != NONE
            for cur, see in (((hx + 1.0, hy), False), ((hx + 30.0, hy - 29.0), False), ((hx + 30.0, hy - 29.0), True)):
                want = small.hover(*cur, see_through=see)
                assert canon(ctx.hover_mesh(srs, stop, IDENTITY_CAM, cur, UNIT_ORTHO, see_through=see)) == canon(want), (k, cur, see)
        assert n_hits >= 40
        assert small.hover(hx + 1.0, hy)["vertex"] == 0 and small.hover(hx + 30.0, hy - 29.0)["vertex"] == NONE
        assert small.hover(hx + 30.0, hy - 29.0, see_through=True)["vertex"] == 3
    finally:
        rs.close(); srs.close(); top.close(); stop.close(); ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["obj-warrior", "asset3-part0-game", "C1"])
def test_gpu_box_select(gpu_ctx, name):
    """b32_box_select == box_select_mesh, both modes and the five rectangles, blocking and by ticket; element counts that are no multiple
    of 32 and below 32."""
    from bonnie32_amd import rasterizer as R
    from bonnie32_amd.rasterizer import Topology, box_select_mesh
    sc, v, polys, top, _ = hover_scene(name, whole=True)
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    tv, tpolys = _mesh([(0, 0, 2), (8, 0, 4), (0, -8, 6), (30, 30, 3), (-20, 5, 1)] + [(3.0 * k, -2.0 * k, 4.0) for k in range(40)], [(0, 1, 2), (3, 4, 0, 1), (4,), (), (9, 8)])
    ttop = Topology.from_polygons(tpolys)
    trs = R.ResidentScene(fb, tv, b32.make_faces(0), []).detach()
    try:
        n_partial = 0
        for mode in (abi.BOX_VERTICES, abi.BOX_POLYGONS):
            n = len(v) if mode == abi.BOX_VERTICES else len(polys)
            for pl in (None, PLACEMENTS[1]):
                for ortho in (None, ORTHO):
                    for rect, _ in _box_cases(sc, v, polys, pl, ortho, mode):
                        want_w, want_n = box_select_mesh(v, top, pl, sc.camera, sc.width, sc.height, rect, mode, ortho)
                        words, cnt = gpu_ctx.box_select(rs, top, sc.camera, rect, mode, ortho, pl)
                        assert cnt == want_n and np.array_equal(words, want_w), (name, mode, pl, ortho, rect, cnt, want_n)
                        n_partial += 0 < cnt < n
            t, res = gpu_ctx.box_select_async(rs, top, sc.camera, (0.0, 0.0, sc.width * 0.6, sc.height * 0.7), mode)
            gpu_ctx.ticket_wait(t)
            want_w, want_n = box_select_mesh(v, top, None, sc.camera, sc.width, sc.height, (0.0, 0.0, sc.width * 0.6, sc.height * 0.7), mode)
            assert (res.n_elements, res.n_selected) == (n, want_n) and np.array_equal(res.words, want_w)
            res.close()
            # 45 vertices (not a multiple of 32), 5 polygons (fewer than 32)
            for rect in ((0.0, 0.0, 320.0, 240.0), (150.0, 100.0, 200.0, 150.0), (320.0, 0.0, 0.0, 240.0)):
                want_w, want_n = box_select_mesh(tv, ttop, None, IDENTITY_CAM, sc.width, sc.height, rect, mode, UNIT_ORTHO)
                words, cnt = gpu_ctx.box_select(trs, ttop, IDENTITY_CAM, rect, mode, UNIT_ORTHO)
                assert cnt == want_n and np.array_equal(words, want_w) and len(words) == (2 if mode == abi.BOX_VERTICES else 1), (mode, rect)
        assert n_partial >= 2
    finally:
        rs.close(); trs.close(); top.close(); ttop.close()


@pytest.mark.gpu
def test_gpu_hover_errors_and_empty_cases(gpu_ctx):
    """NULL context, camera, slot, topology or params, an empty slot, an unknown flag, mirror_axis > 3, a zero-size framebuffer, NULL
    outputs: B32_E_ARG; b32_topology_create's argument errors; nv == 0 or np == 0: "none" where there is nothing to walk."""
    from bonnie32_amd import rasterizer as R
    from bonnie32_amd.rasterizer import Topology
    fb = R.Framebuffer(320, 240, gpu_ctx)
    v, polys = _mesh([(0, 0, 2), (8, 0, 4), (0, -8, 6)], [(0, 1, 2)])
    top = Topology.from_polygons(polys); empty_top = Topology.from_polygons([])
    rs = R.ResidentScene(fb, v, b32.make_faces(0), []).detach()
    nov = R.ResidentScene(fb, b32.make_vertices(0), b32.make_faces(0), []).detach()
    lib, h = gpu_ctx.lib, gpu_ctx.h
    cam = IDENTITY_CAM.pack()
    orth = abi.B32Ortho(*UNIT_ORTHO)
    E = abi.B32_E_ARG
    prm = np.zeros(1, abi.HOVER_PARAMS_DTYPE); prm["mx"], prm["my"], prm["vertex_threshold"], prm["edge_threshold"] = 161.0, 120.0, 6.0, 4.0
    out = np.zeros(1, abi.HOVER_RESULT_DTYPE); t = C.c_uint64(); cnt = C.c_uint32()
    th = top.handle(gpu_ctx)
    empty = C.c_void_p()
    assert lib.b32_scene_create(h, C.byref(empty)) == 0
    try:
        call = lambda c_, cam_, slot, topo, p, o: lib.b32_hover_mesh(c_, cam_, C.byref(orth), slot, topo, None, p, o)
        P, O = prm.ctypes.data, out.ctypes.data
        assert call(h, C.byref(cam), rs._slot, th, P, O) == abi.B32_OK and out[0]["vertex"] == 0
        assert call(None, C.byref(cam), rs._slot, th, P, O) == E and call(h, None, rs._slot, th, P, O) == E
        assert call(h, C.byref(cam), None, th, P, O) == E and call(h, C.byref(cam), rs._slot, None, P, O) == E
        assert call(h, C.byref(cam), rs._slot, th, None, O) == E and call(h, C.byref(cam), rs._slot, th, P, None) == E
        assert call(h, C.byref(cam), empty, th, P, O) == E                                  # a slot that does not hold its scene
        for field, bad in (("flags", 2), ("flags", 0x80000001), ("mirror_axis", 4)):
            q = prm.copy(); q[field] = bad
            assert call(h, C.byref(cam), rs._slot, th, q.ctypes.data, O) == E, field
        buf, p = gpu_ctx.host_alloc(64)
        try:
            acall = lambda o, tk: lib.b32_hover_mesh_async(h, C.byref(cam), C.byref(orth), rs._slot, th, None, P, o, tk)
            assert acall(None, C.byref(t)) == E and acall(p, None) == E
            assert acall(p, C.byref(t)) == abi.B32_OK
            gpu_ctx.ticket_wait(t.value)
            assert buf[:32].view(abi.HOVER_RESULT_DTYPE)[0]["vertex"] == 0
            bp = np.zeros(1, abi.BOX_PARAMS_DTYPE); bp["x1"], bp["y1"] = 320.0, 240.0
            words = np.zeros(1, np.uint32)
            bcall = lambda slot, topo, q, c_: lib.b32_box_select(h, C.byref(cam), C.byref(orth), slot, topo, None, q, words.ctypes.data, c_)
            assert bcall(rs._slot, None, bp.ctypes.data, C.byref(cnt)) == abi.B32_OK and cnt.value == 3 and words[0] == 7
            assert bcall(None, None, bp.ctypes.data, C.byref(cnt)) == E and bcall(rs._slot, None, None, C.byref(cnt)) == E
            assert bcall(rs._slot, None, bp.ctypes.data, None) == E and bcall(empty, None, bp.ctypes.data, C.byref(cnt)) == E
            q = bp.copy(); q["mode"] = 1
            assert bcall(rs._slot, None, q.ctypes.data, C.byref(cnt)) == E                  # polygons need a topology
            assert bcall(rs._slot, th, q.ctypes.data, C.byref(cnt)) == abi.B32_OK and cnt.value == 1
            q["mode"] = 2
            assert bcall(rs._slot, th, q.ctypes.data, C.byref(cnt)) == E
            assert lib.b32_box_select_async(h, C.byref(cam), None, rs._slot, th, None, bp.ctypes.data, None, C.byref(t)) == E
            assert lib.b32_box_select_async(h, C.byref(cam), None, rs._slot, th, None, bp.ctypes.data, p, None) == E
        finally:
            gpu_ctx.host_free(p)
        # b32_topology_create
        th2 = C.c_void_p()
        ps = np.array([0, 3], np.uint32); pv = np.array([0, 1, 2], np.uint32)
        assert lib.b32_topology_create(h, ps.ctypes.data, 1, pv.ctypes.data, None) == E
        assert lib.b32_topology_create(h, None, 1, pv.ctypes.data, C.byref(th2)) == E and lib.b32_topology_create(h, ps.ctypes.data, 1, None, C.byref(th2)) == E
        for bad in ([1, 3], [0, 3, 2]):
            b = np.array(bad, np.uint32)
            assert lib.b32_topology_create(h, b.ctypes.data, len(bad) - 1, pv.ctypes.data, C.byref(th2)) == E
        assert lib.b32_topology_create(h, None, 0, None, C.byref(th2)) == abi.B32_OK and th2.value
        lib.b32_topology_destroy(h, th2); lib.b32_topology_destroy(h, None)
        zs = np.zeros(3, np.uint32)                                                          # two empty polygons: no index to read, NULL is fine
        assert lib.b32_topology_create(h, zs.ctypes.data, 2, None, C.byref(th2)) == abi.B32_OK and th2.value
        lib.b32_topology_destroy(h, th2)
        hollow = Topology.from_polygons([[], []])
        try:
            r = gpu_ctx.hover_mesh(rs, hollow, IDENTITY_CAM, (161.0, 120.0), UNIT_ORTHO, see_through=True)
            assert canon(r) == (0, _bits(1.0), NONE, NONE, 0, NONE, 0)
            assert canon(gpu_ctx.hover_mesh(rs, hollow, IDENTITY_CAM, (161.0, 120.0), UNIT_ORTHO)) == (NONE, 0, NONE, NONE, 0, NONE, 0)
            wh, ch = gpu_ctx.box_select(rs, hollow, IDENTITY_CAM, (0.0, 0.0, 320.0, 240.0), abi.BOX_POLYGONS, UNIT_ORTHO)
            assert (len(wh), ch) == (1, 0) and wh[0] == 0
        finally:
            hollow.close()
        # nothing to walk
        none = (NONE, 0, NONE, NONE, 0, NONE, 0)
        for see in (False, True):
            assert canon(gpu_ctx.hover_mesh(nov, top, IDENTITY_CAM, (161.0, 120.0), UNIT_ORTHO, see_through=see)) == none
            assert canon(gpu_ctx.hover_mesh(nov, empty_top, IDENTITY_CAM, (161.0, 120.0), UNIT_ORTHO, see_through=see)) == none
        r = gpu_ctx.hover_mesh(rs, empty_top, IDENTITY_CAM, (161.0, 120.0), UNIT_ORTHO, see_through=True)     # np == 0: the vertices remain
        assert canon(r) == (0, _bits(1.0), NONE, NONE, 0, NONE, 0)
        assert canon(gpu_ctx.hover_mesh(rs, empty_top, IDENTITY_CAM, (161.0, 120.0), UNIT_ORTHO)) == none
        w0, c0 = gpu_ctx.box_select(nov, empty_top, IDENTITY_CAM, (0.0, 0.0, 320.0, 240.0), abi.BOX_POLYGONS, UNIT_ORTHO)
        w1, c1 = gpu_ctx.box_select(nov, None, IDENTITY_CAM, (0.0, 0.0, 320.0, 240.0), abi.BOX_VERTICES, UNIT_ORTHO)
        assert (len(w0), c0, len(w1), c1) == (0, 0, 0, 0)
        fresh = R.Context(0)                                                                 # no framebuffer yet: zero-size
        try:
            frs = C.c_void_p()
            assert fresh.lib.b32_scene_create(fresh.h, C.byref(frs)) == 0
            fth = C.c_void_p()
            assert fresh.lib.b32_topology_create(fresh.h, ps.ctypes.data, 1, pv.ctypes.data, C.byref(fth)) == abi.B32_OK
            fbuf, fp = fresh.host_alloc(64)
            bq = bp.copy(); bq["mode"] = 1; out[:] = 0; words[:] = 0
            try:                                                                             # the slot holds a scene: only the size is wrong
                assert fresh.lib.b32_scene_upload(fresh.h, v.ctypes.data, len(v), None, 0, None, 0) == abi.B32_OK
                assert fresh.lib.b32_scene_swap(fresh.h, frs) == abi.B32_OK
                assert fresh.lib.b32_hover_mesh(fresh.h, C.byref(cam), C.byref(orth), frs, fth, None, P, O) == E
                assert fresh.lib.b32_hover_mesh_async(fresh.h, C.byref(cam), C.byref(orth), frs, fth, None, P, fp, C.byref(t)) == E
                for q, topo in ((bp, None), (bq, fth)):
                    assert fresh.lib.b32_box_select(fresh.h, C.byref(cam), C.byref(orth), frs, topo, None, q.ctypes.data, words.ctypes.data, C.byref(cnt)) == E
                    assert fresh.lib.b32_box_select_async(fresh.h, C.byref(cam), C.byref(orth), frs, topo, None, q.ctypes.data, fp, C.byref(t)) == E
                ffb = R.Framebuffer(320, 240, fresh)                                         # ... and with a framebuffer the same calls answer
                assert fresh.lib.b32_hover_mesh(fresh.h, C.byref(cam), C.byref(orth), frs, fth, None, P, O) == abi.B32_OK and out[0]["vertex"] == 0
                assert fresh.lib.b32_box_select(fresh.h, C.byref(cam), C.byref(orth), frs, None, None, bp.ctypes.data, words.ctypes.data, C.byref(cnt)) == abi.B32_OK
                assert cnt.value == 3 and words[0] == 7
                del ffb
            finally:
                fresh.host_free(fp)
                fresh.lib.b32_topology_destroy(fresh.h, fth); fresh.lib.b32_scene_destroy(fresh.h, frs)
        finally:
            fresh.close()
    finally:
        lib.b32_scene_destroy(h, empty)
        rs.close(); nov.close(); top.close(); empty_top.close()


def _delivered_run_with_hover(R, fr, mode, with_hover, top, n_frames=30):
    """tests.test_pick._delivered_run's frame -- clear, b32_frame_submit_placed, b32_fb_download_async per frame, moving placements, tickets
    waited one frame behind -- with one b32_hover_mesh_async of part 0 of object 0 (its moving placement, a moving cursor) per frame."""
    ctx = R.Context(0)
    ctx.set_async_depth(1 if mode == "deep" else 0)
    fb = R.Framebuffer(fr.W, fr.H, ctx)
    slots = fr.upload(R, fb)
    st = fr.settings()
    entries = fr.entries(fr.placements(0.0))
    table = ctx.make_frame_table(fr.cam, st, [slots[i] for i, _, _ in entries], fogs=[p["fog"] for _, p, _ in entries],
                                 ambients=[p["ambient"] for _, p, _ in entries], placements=[pl for _, _, pl in entries],
                                 backface_culls=[p["backface_cull"] for _, p, _ in entries])
    bufs = [ctx.host_alloc(fr.W * fr.H * 4) for _ in range(2)]
    hbufs = [ctx.host_alloc(32) for _ in range(2)]
    tickets, htickets, hresults = [0, 0], [0, 0], [None, None]
    frames, hovers, counts = [], [], []

    def collect(t):
        ctx.ticket_wait(tickets[t & 1])
        frames.append(bufs[t & 1][0].copy())
        if with_hover:
            ctx.ticket_wait(htickets[t & 1])
            hovers.append(hresults[t & 1].record)
    try:
        for t in range(n_frames):
            pls = fr.placements(float(t))
            ctx.set_table_placements(table, [None] + [pls[k] for k in range(fr.n_objects) for _ in range(3)])
            fb.clear(fr.clear)
            if with_hover and mode == "safe_clear_pending":
                htickets[t & 1], hresults[t & 1] = ctx.hover_mesh_async(slots[1], top, fr.cam, hover_cursor(fr, t), placement=pls[0], see_through=bool(t & 1), out=hbufs[t & 1])
            ctx.frame_submit(table)
            if with_hover and mode != "safe_clear_pending":
                htickets[t & 1], hresults[t & 1] = ctx.hover_mesh_async(slots[1], top, fr.cam, hover_cursor(fr, t), placement=pls[0], see_through=bool(t & 1), out=hbufs[t & 1])
            tickets[t & 1] = ctx.download_async(bufs[t & 1][1])
            counts.append(ctx.batch_counts())
            if t > 0:
                collect(t - 1)
        collect(n_frames - 1)
        ctx.finish()
        counts.append(ctx.batch_counts())
    finally:
        for _, p in bufs + hbufs:
            ctx.host_free(p)
        top.close()
        ctx.close()
    return frames, hovers, counts


def hover_cursor(fr, t):
    """The projected position of a vertex of object 0's first part under its placement at time t, a little beside it."""
    from bonnie32_amd.rasterizer import HoverMirror, Topology
    m = fr.mesh(1)
    hm = HoverMirror(m.vertices, Topology.from_polygons([]), fr.placements(float(t))[0], fr.cam, fr.W, fr.H)
    ok = np.nonzero(hm.some)[0]
    i = ok[(7 * t) % len(ok)] if len(ok) else 0
    o = OFFS[t % 8]
    return (float(hm.sx[i]) + o[0], float(hm.sy[i]) + o[1]) if len(ok) else (10.0, 10.0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["deep", "safe_clear_pending"])
def test_gpu_hover_does_not_interfere_with_delivered_frames(mode):
    """30 delivered frames with one asynchronous hover each: the frames are byte-equal to the same run without hovers, every hover equals
    the mirror's, and every b32_batch_count is the same after every frame."""
    from bonnie32_amd import rasterizer as R
    from bonnie32_amd.rasterizer import HoverMirror, Topology
    from tests.test_placement import _Frame
    fr = _Frame()
    polys = merge_quads(fr.mesh(1).faces)
    plain_frames, _, plain_counts = _delivered_run_with_hover(R, fr, mode, False, Topology.from_polygons(polys))
    frames, hovers, counts = _delivered_run_with_hover(R, fr, mode, True, Topology.from_polygons(polys))
    assert len(frames) == len(plain_frames) == 30 and len(hovers) == 30
    for t, (a, b) in enumerate(zip(frames, plain_frames)):
        assert np.array_equal(a, b), f"frame {t}: {int((a != b).sum())} bytes differ"
    assert all(not np.array_equal(frames[t], frames[t + 1]) for t in range(29)) and counts == plain_counts
    top = Topology.from_polygons(polys)
    n_hit = 0
    for t, got in enumerate(hovers):
        hm = HoverMirror(fr.mesh(1).vertices, top, fr.placements(float(t))[0], fr.cam, fr.W, fr.H)
        want = hm.hover(*hover_cursor(fr, t), see_through=bool(t & 1))
        assert canon(got) == canon(want), (t, got, want)
        n_hit += want["vertex"] != NONE or want["edge_v0"] != NONE
    assert n_hit >= 12, n_hit


@pytest.mark.gpu
def test_gpu_nine_outstanding_tickets_with_hovers():
    """Downloads, picks, hovers and box selections share the tickets: nine are issued without a wait in between (the ninth first waits for
    the oldest), then all are waited for; every answer is right."""
    from bonnie32_amd import rasterizer as R
    sc, v, polys, top, curs = hover_scene("obj-warrior")
    ctx = R.Context(0)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings, sc.fog); rs.finish()
    want_px = np.asarray(fb.pixels).reshape(-1)
    table = ctx.make_pick_table([(rs, PLACEMENTS[0])])
    rect = (0.0, 0.0, sc.width * 0.5, sc.height * 0.5)
    want_pick = [ctx.pick_meshes(table, sc.camera, curs[k]) for k in range(9)]
    want_hover = [ctx.hover_mesh(rs, top, sc.camera, curs[k]) for k in range(9)]
    want_box = ctx.box_select(rs, top, sc.camera, rect, abi.BOX_POLYGONS)
    fbufs = [ctx.host_alloc(sc.width * sc.height * 4) for _ in range(2)]
    try:
        issued = []
        for k in range(9):
            kind = ("hover", "frame", "pick", "hover", "box", "frame", "hover", "pick", "hover")[k]
            if kind == "hover":
                issued.append((kind, k) + ctx.hover_mesh_async(rs, top, sc.camera, curs[k]))
            elif kind == "pick":
                issued.append((kind, k) + ctx.pick_meshes_async(table, sc.camera, curs[k]))
            elif kind == "box":
                issued.append((kind, k) + ctx.box_select_async(rs, top, sc.camera, rect, abi.BOX_POLYGONS))
            else:
                issued.append((kind, k, ctx.download_async(fbufs[k // 5][1]), fbufs[k // 5][0]))
        ts = [i[2] for i in issued]
        assert ts == list(range(ts[0], ts[0] + 9))
        assert ctx.ticket_done(ts[0])                                          # the ninth waited for it
        for kind, k, t, res in issued:
            ctx.ticket_wait(t)
            if kind == "hover":
                assert res.record.tobytes() == want_hover[k].tobytes(), k
            elif kind == "pick":
                assert res.best == want_pick[k][0] and res.hits.tobytes() == want_pick[k][1].tobytes(), k
            elif kind == "box":
                assert res.n_selected == want_box[1] and np.array_equal(res.words, want_box[0]) and 0 < want_box[1] < len(polys)
            else:
                assert np.array_equal(res, want_px), k
            if kind != "frame":
                res.close()
        assert sum(w["vertex"] != NONE for w in want_hover) >= 4
    finally:
        for _, p in fbufs:
            ctx.host_free(p)
        rs.close(); top.close(); ctx.close()
