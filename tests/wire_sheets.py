"""Wire sheets: meshes in which every decision of the wireframe phases (render.rs:2574-2635, draw_line_3d render.rs:757-817, draw_line
render.rs:716-750) is a pixel of the frame (tests/test_wire_sheets.py).

Isolated lines come from degenerate faces: (A, B, B) has signed area 0, is a back face, and contributes the edge A-B, the point B-B and
B-A, which is A-B again after direction normalisation; (A, A, A) contributes a point.  Proper back-facing triangles stand where three
distinct edges per list entry are wanted.  "Floors" -- pairs of front-facing triangles with equal vertex depths -- make the depth the
lines are tested against; a sheet with floors is built in two passes: the floors alone are drawn by the oracle, their stored depth bits
are read per pixel, and the lines' depths are chosen against those bits (lines never write depth, floors never depend on lines).

  L  line geometry: every direction vector |dx|, |dy| <= 7 from a cell's centre, as A->B and in a second cell as B->A, the centres on
     the 64-column and 16-row tile boundaries; edges through every side and corner of the frame and wholly outside; float projection
     adds fractional and negative fractional screen coordinates.  (450 cells of 16 x 16 do not fit 256 x 192: the frame is 288 x 526,
     neither a multiple of 64 wide nor of 16 high.)
  O  occurrence: one screen edge carried by two or three back faces with depths on either side of a floor
  Z  depth: edges at the floor's stored bits and one ulp on either side, sloped edges, searched fused / unfused verdicts, the point edge,
     the non-normalised direction; orthographic: negative depths, FLT_MAX, a depth difference that overflows
  T  the tile route's thresholds: box sizes, the union box, list capacity, segment passes, walk selection, refusal, hash chains

Not reachable: 3072 segments in one tile.  A segment is 16 steps of one drawn edge inside the 64 x 16 tile; 3072 of them need 768 edges
of 64 steps each from the 256 faces a list holds, i.e. all three edges of every face x-major across all 64 columns.  Two edges of a
triangle can be (a vertex left of the tile, two right of it); the third then joins two vertices on the same side and has no step inside
wider than the tile's 16 rows: at most 4 + 4 + 1 = 9 segments per face, 2304 per tile.  T-seg-max aims at that and reaches 2288 (two passes).

This module only builds, projects and caches; what the tests compare is always the oracle's frame."""
import functools
from dataclasses import dataclass, field

import numpy as np

from bonnie32_amd.rtypes import Camera, RasterSettings, make_faces, make_vertices
from oracle import np_model as M
from tests.frontend_sheets import CLEAR, ORTHO, bits, down, face_colour, fog, place, project, up

f32 = np.float32
DIST = f32(M.K("mesh.distance"))
FLT_MAX = np.finfo(f32).max
COL_BACK, COL_FRONT = (80, 80, 100), (200, 200, 220)       # render.rs:2600, 2629
O_FOG = "normal"                                            # cull distance 12 (camera depth), no colour change: frontend_sheets.fog


def camz_of(want):
    """the camera depth whose screen depth (camera depth + 5.0) is `want`: exact for `want` in [8, 16)"""
    want = f32(want)
    with np.errstate(all="ignore"):
        c = f32(want - DIST)
        if 8.0 <= want < 16.0:
            assert bits(f32(c + DIST)) == bits(want), want
    return c


@dataclass
class WSheet:
    name: str
    proj: str
    width: int
    height: int
    vertices: np.ndarray
    faces: np.ndarray
    tags: list                      # per face
    cells: list                     # dicts: tag, faces [ids], whatever the family's census reads
    info: dict = field(default_factory=dict)
    fog_name: str = None            # the fog the RGB555 path draws the sheet with
    camera: Camera = field(default_factory=Camera)
    textures: list = field(default_factory=list)
    _oracle: dict = field(default_factory=dict)
    _proj: tuple = None

    @property
    def n(self):
        return len(self.faces)

    def textures8(self):
        return []

    def settings(self, zbuffer=True, fmt8=False, cull=True, xray=False, overlay=False, wire=True):
        st = RasterSettings.benchmark()
        st.dithering = False
        st.backface_cull = cull
        st.backface_wireframe = wire
        st.wireframe_overlay = overlay
        st.use_zbuffer = zbuffer
        st.use_rgb555 = not fmt8
        st.xray_mode = xray
        st.use_fixed_point = self.proj == "fixed"
        st.ortho_projection = ORTHO if self.proj == "ortho" else None
        return st

    def fog(self, mode):
        return fog(self.fog_name) if self.fog_name and not mode.get("fmt8") else None

    def projected(self):
        if self._proj is None:
            self._proj = project(self.vertices["pos"], self.camera, self.proj, self.width, self.height)
        return self._proj

    def edges_i32(self):
        """[nf, 3, 2] the faces' screen points after `as i32` (the projection's, never the intent)"""
        scr, _ = self.projected()
        xy = np.array([[M._as_i32(scr[i][0]), M._as_i32(scr[i][1])] for i in range(len(scr))], np.int64)
        return xy[self.faces["v"].astype(np.int64)]

    def oracle(self, O, **mode):
        """dict(rc, px [H, W, 4], zb bits [H, W], tm) of the reference restatement; computed once per mode, shared and read-only"""
        key = tuple(sorted(mode.items()))
        if key not in self._oracle:
            fb = O.Framebuffer(self.width, self.height)
            fb.clear(CLEAR)
            st = self.settings(**mode)
            with np.errstate(all="ignore"):
                if mode.get("fmt8"):
                    rc, tm = O.render_mesh(fb, self.vertices, self.faces, [], self.camera, st)
                else:
                    rc, tm = O.render_mesh_15(fb, self.vertices, self.faces, [], self.camera, st, self.fog(mode))
            px = fb.image().copy(); px.setflags(write=False)
            zb = fb.zbuffer.view(np.uint32).reshape(self.height, self.width).copy(); zb.setflags(write=False)
            self._oracle[key] = dict(rc=rc, px=px, zb=zb, tm=tm)
        return self._oracle[key]

    def first_difference(self, got, want, what):
        g = np.asarray(got).reshape(self.height, self.width, -1)
        w = np.asarray(want).reshape(self.height, self.width, -1)
        bad = (g != w).any(axis=2)
        if not bad.any():
            return ""
        y, x = [int(v[0]) for v in np.nonzero(bad)]
        near = min(self.cells, key=lambda c: abs(c.get("at", (0, 0))[0] - x) + abs(c.get("at", (0, 0))[1] - y))["tag"] if self.cells else ""
        return f"[{self.name} {what}] {int(bad.sum())} pixels differ, first at ({x}, {y}): got {g[y, x].tolist()}, oracle {w[y, x].tolist()}; nearest cell '{near}'"


class _Mesh:
    """faces by screen targets and depths, three vertices of their own each"""

    def __init__(self, proj, width, height):
        self.proj, self.width, self.height = proj, width, height
        self.pts, self.cz, self.tags, self.world = [], [], [], {}
        self.cells = []

    def face(self, pts, z, tag, camz=False, world=None):
        """pts: three screen targets; z: three screen depths (camz: camera depths as they are; orthographic: the same thing)"""
        z = [f32(t) for t in z]
        if not camz and self.proj != "ortho":
            z = [camz_of(t) for t in z]
        if world is not None:
            self.world[len(self.tags)] = np.asarray(world, np.float32).reshape(3, 3)
        self.pts.append([(float(p[0]), float(p[1])) for p in pts]); self.cz.append(z); self.tags.append(tag)
        return len(self.tags) - 1

    def line(self, a, b, za, zb, tag, rev=False):
        """the degenerate face (A, B, B), or (B, A, A)"""
        return self.face((b, a, a), (zb, za, za), tag) if rev else self.face((a, b, b), (za, zb, zb), tag)

    def floor(self, x0, y0, x1, y1, z, tag="floor"):
        """two front-facing triangles over [x0, x1) x [y0, y1) with equal vertex depths"""
        a = self.face(((x0, y0), (x1, y0), (x0, y1)), (z, z, z), tag)
        self.face(((x1, y0), (x1, y1), (x0, y1)), (z, z, z), tag)
        return [a, a + 1]

    def cell(self, tag, faces, **kw):
        self.cells.append(dict(tag=tag, faces=list(faces), **kw))

    def build(self, name, **kw):
        nf = len(self.tags)
        p = np.asarray(self.pts, np.float64).reshape(-1, 2)
        cz = np.asarray(self.cz, np.float32).reshape(-1)
        with np.errstate(all="ignore"):
            pos = place(self.proj, Camera(), p[:, 0], p[:, 1], cz, self.width, self.height)
        for i, w in self.world.items():
            pos[3 * i:3 * i + 3] = w
        v = make_vertices(3 * nf)
        v["pos"] = pos
        v["normal"] = (0.0, 0.0, -1.0)
        col = np.repeat(np.array([face_colour(i) for i in range(nf)], np.uint8), 3, axis=0)
        v["r"], v["g"], v["b"] = col[:, 0], col[:, 1], col[:, 2]
        f = make_faces(nf)
        f["v"] = np.arange(3 * nf, dtype=np.uint32).reshape(nf, 3)
        v.setflags(write=False); f.setflags(write=False)
        return WSheet(name, self.proj, self.width, self.height, v, f, list(self.tags), self.cells, **kw)


# ------------------------------------------------------------------------------------------------ family L
L_W, L_H, L_ORG, L_PER_ROW = 288, 526, 24, 15
L_VECTORS = [(dx, dy) for dy in range(-7, 8) for dx in range(-7, 8)]
L_BORDER = [("left", (6, 100), (-6, 104)), ("right", (281, 60), (294, 57)), ("top", (100, 5), (103, -6)), ("bottom", (100, 520), (97, 531)),
            ("corner-tl", (3, 3), (-4, -5)), ("corner-tr", (284, 3), (292, -4)), ("corner-bl", (3, 522), (-3, 529)), ("corner-br", (284, 522), (291, 528)),
            ("outside-tl", (-10, -10), (-3, -20)), ("outside-r", (300, 100), (310, 120)), ("outside-t", (100, -7), (120, -3)), ("outside-b", (100, 530), (130, 540)),
            ("outside-across-corner", (-6, 3), (4, -7)), ("through", (-5, 10), (293, 14)), ("through-steep", (2, -9), (9, 535))]
L_FRACTIONS = [("-0.9 -> 0", (-0.9, 300.4), (5.99, 303.7)), ("-1.5 -> -1", (-1.5, 310.2), (4.3, 316.8)), ("10.99 -> 10", (10.99, 320.99), (2.01, 326.5)),
               ("y -0.9 -> 0", (40.3, -0.9), (44.6, 6.99)), ("y -1.5 -> -1", (50.7, -1.5), (47.2, 5.5)), ("-0.5, -0.5 -> 0, 0", (-0.5, -0.5), (7.9, 3.2)),
               ("-6.99 -> -6", (-6.99, 330.5), (6.5, 333.1)), ("-7.01 -> -7", (-7.01, 340.5), (6.5, 343.1))]


def family_l(proj):
    m = _Mesh(proj, L_W, L_H)
    fr = (0.37, 0.61) if proj == "float" else (0.0, 0.0)
    for n, (dx, dy) in enumerate(L_VECTORS):
        for rev in (False, True):
            c = 2 * n + rev
            cx, cy = L_ORG + 16 * (c % L_PER_ROW) + 8, L_ORG + 16 * (c // L_PER_ROW) + 8
            a, b = (cx + fr[0], cy + fr[1]), (cx + dx + fr[0], cy + dy + fr[1])
            fi = m.line(a, b, 9.0, 9.0, f"L {dx},{dy} {'BA' if rev else 'AB'}", rev=rev)
            m.cell(f"L {dx},{dy} {'BA' if rev else 'AB'}", [fi], at=(cx, cy), vec=(dx, dy), rev=rev)
    for tag, a, b in L_BORDER + (L_FRACTIONS if proj == "float" else []):
        for rev in (False, True):
            fi = m.line(a, b, 9.0, 10.0, f"L {tag}", rev=rev)
            m.cell(f"L {tag}", [fi], at=(int(a[0]), int(a[1])), border=tag)
    return m.build("L-" + proj)


# ------------------------------------------------------------------------------------------------ family O
O_W, O_H = 256, 192
O_FLOOR, O_NEAR, O_FAR, O_FRONT = 10.0, 9.0, 11.0, 12.0
# the shapes an occurrence of the edge A-B comes in: vertex order over A, B and a third point C (or C2, so that two triangles of one
# cell share no other edge); the slot j the edge A-B has in it.  A = (2, 3), B = (12, 7); (A, C, B) is a back face, (A, B, C) a front face
O_SHAPES = {"d0": ("ABB", 0), "d1": ("BAA", 0), "d2": ("BBA", 1), "t0": ("BAC", 0), "t1": ("CBA", 1), "t2": ("ACB", 2),
            "u0": ("BAD", 0), "u1": ("DBA", 1), "u2": ("ADB", 2), "front": ("ABC", 0), "front2": ("CAB", 1)}
O_POINTS = {"A": (2, 3), "B": (12, 7), "C": (4, 13), "D": (8, 14)}
O_PAIRS = [("d0", "d0"), ("d0", "d1"), ("d1", "d0"), ("d2", "d0"), ("d0", "d2"), ("t0", "u0"), ("t0", "u1"), ("t0", "u2"), ("t1", "u0"), ("t2", "u0"),
           ("t1", "u2"), ("t2", "u1"), ("t2", "d0"), ("d1", "u1")]


def _o_face(m, x0, y0, shape, z, tag, camz=None):
    pts = [(x0 + O_POINTS[c][0], y0 + O_POINTS[c][1]) for c in O_SHAPES[shape][0]]
    if camz is not None:
        return m.face(pts, camz, tag, camz=True)
    return m.face(pts, (z, z, z), tag)


def family_o(width=O_W, height=O_H, blocks=((0, 0),), floor=O_FLOOR, rotate=0, name="O"):
    """Every cell: a floor at depth 10 and two or three occurrences of the edge A-B, each face at one depth, 9 (visible) or 11 (hidden).
    kinds: 'pair' / 'triple' (both orders of the depths), 'ends' (the occurrences are faces 0, 1 and nf-2, nf-1 of the mesh), 'near' /
    'fog' (the first occurrence sits in a face the near plane rejects / the fog culls: the second one owns the edge), 'overlay' (the edge
    in a back face and in a front face: two lists).
    blocks: origins of the 256 x 192 blocks of 192 cells each (one, in the frame's top left corner, unless the sheet is a large mesh for
    the frames in flight); rotate: where in the list of cell kinds a block starts; floor: the floors' depth."""
    m = _Mesh("fixed", width, height)
    specs = []                                      # (kind, tag, [(shape, depth or camera depths)])
    for a, b in O_PAIRS:
        for first, second in ((O_FAR, O_NEAR), (O_NEAR, O_FAR)):
            specs.append(("pair", f"O {a} then {b}, {'hidden' if first == O_FAR else 'visible'} first", [(a, first), (b, second)]))
    for zs in ((O_FAR, O_NEAR, O_FAR), (O_NEAR, O_FAR, O_NEAR), (O_FAR, O_FAR, O_NEAR)):
        specs.append(("triple", f"O three occurrences {zs}", [("d0", zs[0]), ("t1", zs[1]), ("u2", zs[2])]))
    # the rejected occurrence: a back face (B, A, C) whose vertex C is in front of the near plane / whose vertices are all beyond the fog's distance
    for second in (O_FAR, O_NEAR):
        specs.append(("near", f"O first occurrence near-rejected, owner at {second}", [("t0", "near"), ("u1", second)]))
        specs.append(("fog", f"O first occurrence fog-culled, owner at {second}", [("t0", "fog"), ("d1", second)]))
    for back in ("t2", "d0"):
        specs.append(("overlay", f"O back {back} then front", [(back, O_NEAR), ("front", O_FRONT)]))
        specs.append(("overlay", f"O front then back {back}", [("front2", O_FRONT), (back, O_NEAR)]))
    ends = [("ends", "O faces 0 and nf-2, hidden first", [("d0", O_FAR), ("d1", O_NEAR)]), ("ends", "O faces 1 and nf-1, visible first", [("t0", O_NEAR), ("u2", O_FAR)])]
    per_row = O_W // 16
    cells = []                                      # (kind, tag, occurrences, x0, y0, shift): the repeats of a kind are moved by a pixel
    for bi, (bx, by) in enumerate(blocks):
        own = ends if bi == 0 else []
        block = own + [specs[(i + rotate + 5 * bi) % len(specs)] for i in range(per_row * (O_H // 16) - len(own))]
        cells += [(kind, tag, occ, bx + 16 * (c % per_row), by + 16 * (c // per_row), (c // len(specs)) % 2) for c, (kind, tag, occ) in enumerate(block)]
    first_of_end, last_of_end = [], []
    for c, (kind, tag, occ, x0, y0, _) in enumerate(cells[:len(ends)]):
        first_of_end.append((c, x0, y0, occ[0])); last_of_end.append((c, x0, y0, occ[1]))
        m.cell(tag, [], at=(x0, y0), kind=kind, occ=[], floor=[])
    for c, x0, y0, (shape, z) in first_of_end:                    # faces 0 and 1
        m.cells[c]["occ"].append(_o_face(m, x0, y0, shape, z, m.cells[c]["tag"]))
    for c, (kind, tag, occ, x0, y0, sh) in enumerate(cells):
        if kind == "ends":
            m.cells[c]["floor"] = m.floor(x0, y0, x0 + 16, y0 + 16, floor)
            continue
        ids = []
        for shape, z in occ:
            if z == "near":
                ids.append(_o_face(m, x0 + sh, y0, shape, None, tag, camz=(camz_of(O_NEAR), camz_of(O_NEAR), f32(0.05))))
            elif z == "fog":
                ids.append(_o_face(m, x0 + sh, y0, shape, None, tag, camz=(f32(12.5), f32(13.0), f32(14.0))))
            else:
                ids.append(_o_face(m, x0 + sh, y0, shape, z, tag))
        fl = m.floor(x0, y0, x0 + 16, y0 + 16, floor)
        pt = [m.face(((x0 + 14, y0 + 2 + k),) * 3, (O_NEAR if k % 2 else O_FAR,) * 3, "O point") for k in range(2)]        # (A, A, A): a point
        m.cell(tag, ids + fl + pt, at=(x0, y0), kind=kind, occ=ids, floor=fl, shift=sh)
    for c, x0, y0, (shape, z) in last_of_end:                     # faces nf-2 and nf-1
        m.cells[c]["occ"].append(_o_face(m, x0, y0, shape, z, m.cells[c]["tag"]))
        m.cells[c]["faces"] = m.cells[c]["occ"] + m.cells[c]["floor"]
        m.cells[c]["shift"] = 0
    return m.build(name, fog_name=O_FOG)


# two large meshes for the frames in flight: nine blocks of sheet O's cells on a 1920 x 1440 frame (690 fill tiles, more than two per
# CU, and more than 8192 faces: the direct-binning route, whose next frame may run its setup and its wire binning on the side stream);
# the second one starts elsewhere in the list of kinds and has nearer floors, so alternating frames change depths and verdicts
BIG_W, BIG_H = 1920, 1440
BIG_BLOCKS = tuple((40 + 600 * i, 24 + 460 * j) for j in range(3) for i in range(3))


# ------------------------------------------------------------------------------------------------ family Z
Z_W, Z_H = 256, 192
Z_GEOMS = [((2, 8), (13, 8)), ((3, 3), (13, 13)), ((6, 2), (9, 13)), ((13, 4), (2, 11)), ((8, 13), (8, 2))]        # A, B inside the cell
Z_KINDS = ("at", "below", "above", "cross", "cross-reversed", "fused-a", "fused-b", "point-below", "point-at", "point-above")


def _floors_zb(m):
    """pass one: the stored depth of every pixel after the floors alone, by the oracle"""
    from oracle import oracle as O
    sh = m.build("floors")
    return sh.oracle(O)["zb"].view(np.float32)


def _line_zb(zb, a, b):
    xs, ys, _ = M.line_points(min(a, b)[0], min(a, b)[1], max(a, b)[0], max(a, b)[1])
    return zb[ys, xs]


def _unfused(z0, z1, k, n):
    t = (f32(k) / f32(n))
    return f32(z0 + f32(t * f32(z1 - z0)))


def _search_fused(zline, n, rng):
    """(z0, z1): endpoint depths in [8, 16) of a line of n steps over the stored depths zline[0..n] for which, at some step k, the verdict
    z < zb of z0 + fl(t * dz) (the reference) and of the fused fl(z0 + t * dz) differ; also which of the two draws the pixel (True: the unfused one)"""
    for _ in range(400):
        cnt = 4096
        k = rng.integers(1, n, cnt)
        zbk = zline[k].astype(np.float64)
        z0 = rng.uniform(8.0, 16.0, cnt).astype(np.float32)
        t = (k.astype(np.float32) / f32(n)).astype(np.float32)
        z1 = (z0.astype(np.float64) + (zbk - z0) / t).astype(np.float32)
        z1 = (z1 + rng.integers(-3, 4, cnt).astype(np.float32) * np.spacing(z1)).astype(np.float32)
        dz = (z1 - z0).astype(np.float32)
        prod = t.astype(np.float64) * dz.astype(np.float64)                       # exact
        zu = (z0 + prod.astype(np.float32)).astype(np.float32)
        zf = (z0.astype(np.float64) + prod).astype(np.float32)                    # (the census confirms with exact rationals)
        ok = (z1 >= 8.0) & (z1 < 16.0) & ((zu < zbk) != (zf < zbk))
        hit = np.nonzero(ok)[0]
        if len(hit):
            return f32(z0[hit[0]]), f32(z1[hit[0]]), bool(zu[hit[0]] < zbk[hit[0]])
    raise AssertionError("no fused / unfused pair found; widen the search")


# the inputs _search_fused found (seed 20260), in cell order: bits of z0, bits of z1, does the unfused form draw the deciding pixel; kept
# so that the sheet does not depend on a search at build time (the census confirms every one with exact rationals); a cell beyond the
# table, should the sheet grow, is searched
Z_FUSED = [(0x41086EB7, 0x414D0350, True), (0x410FE4C1, 0x4161ADFC, False), (0x415C3A3B, 0x411DDE87, True), (0x4141BE2C, 0x4155135A, False),
           (0x414F9587, 0x410D822D, True), (0x4115B7B8, 0x413E9B8E, False), (0x410EB033, 0x415E16C9, True), (0x413BDA33, 0x4159AB1E, False),
           (0x413BE6CF, 0x416944D7, True), (0x4102C393, 0x41267F34, False), (0x4142C990, 0x410C790F, True), (0x4179BFBA, 0x41124CFA, False),
           (0x41659B0A, 0x4152B39B, True), (0x417C05E0, 0x41499C85, False), (0x413B5DCA, 0x41003207, True), (0x412092F4, 0x4149F038, False),
           (0x410BC65D, 0x415A9FCE, False), (0x410EB6EF, 0x41557D79, False), (0x41740285, 0x410BEA10, True), (0x41448B7E, 0x410C812B, False),
           (0x415146EE, 0x4138E80B, True), (0x4121C6C9, 0x417E371B, False), (0x416A4333, 0x410D6F34, True), (0x4116BF02, 0x4123F85E, False),
           (0x41225573, 0x4168092F, True), (0x41057C12, 0x416DEADD, False), (0x41488110, 0x41715B96, False), (0x4138762C, 0x41619C04, False),
           (0x41686163, 0x412E1359, True), (0x416ACB89, 0x410A44A4, False), (0x41668725, 0x413B7EFE, False), (0x415AEF85, 0x413C9044, False),
           (0x4150F631, 0x4121997E, True), (0x414C0284, 0x4109A2DD, False), (0x4120A445, 0x414A9021, False), (0x411AF2D4, 0x416421DD, False),
           (0x414E5927, 0x4109DD72, True), (0x4101A73F, 0x41437031, False)]


@functools.lru_cache(maxsize=None)
def family_z():
    """Perspective (fixed point): 16 x 16 cells, each a floor of its own depth and one line chosen against the floor's stored bits."""
    per_row = Z_W // 16
    ncell = per_row * (Z_H // 16)
    floors = _Mesh("fixed", Z_W, Z_H)
    depth = [f32(10.0 + 0.173 * (c % 23)) for c in range(ncell)]
    # (where the two forms differ, the unfused sum is nearly always a tie rounded to even: it can be the smaller of the two neighbours --
    #  and pass where the fused one does not -- only below an ODD stored depth, and the larger one only at an even one)
    for c in range(ncell):
        kind = Z_KINDS[c % len(Z_KINDS)]
        if (kind == "fused-a" and bits(depth[c]) % 2 == 0) or (kind == "fused-b" and bits(depth[c]) % 2 == 1):
            depth[c] = up(depth[c])
    for c in range(ncell):
        x0, y0 = 16 * (c % per_row), 16 * (c // per_row)
        floors.floor(x0, y0, x0 + 16, y0 + 16, depth[c])
    zb = _floors_zb(floors)
    m = _Mesh("fixed", Z_W, Z_H)
    m.pts, m.cz, m.tags = list(floors.pts), list(floors.cz), list(floors.tags)
    rng = np.random.default_rng(20260)
    fused = []
    for c in range(ncell):
        x0, y0 = 16 * (c % per_row), 16 * (c // per_row)
        kind = Z_KINDS[c % len(Z_KINDS)]
        ga, gb = Z_GEOMS[(c // len(Z_KINDS) + c) % len(Z_GEOMS)]
        a, b = (x0 + ga[0], y0 + ga[1]), (x0 + gb[0], y0 + gb[1])
        lo, hi = min(a, b), max(a, b)                               # the normalised direction: the walk starts at lo
        zl = _line_zb(zb, a, b)
        n = max(abs(b[0] - a[0]), abs(b[1] - a[1]))
        F = f32(zl[0])
        rev = (c // 3) % 2 == 1
        if kind in ("at", "below", "above"):
            v = {"at": F, "below": down(F), "above": up(F)}[kind]
            fi = m.line(a, b, v, v, f"Z {kind}", rev=rev)
        elif kind == "cross":
            fi = m.line(lo, hi, F - f32(1.0), F + f32(1.0), "Z cross")
        elif kind == "cross-reversed":                              # given from the larger end: the depths must swap with the endpoints
            fi = m.line(hi, lo, F + f32(1.0), F - f32(1.0), "Z cross-reversed")
        elif kind in ("fused-a", "fused-b"):
            # (which way is possible depends on the parity of the stored bits)
            if len(fused) < len(Z_FUSED):
                b0, b1, unfused = Z_FUSED[len(fused)]
                z0, z1 = np.array([b0, b1], np.uint32).view(np.float32)
            else:
                z0, z1, unfused = _search_fused(zl, n, rng)
            fused.append((bits(z0), bits(z1), unfused))
            kind = "fused-a" if unfused else "fused-b"
            fi = m.line(lo, hi, z0, z1, f"Z {kind}", rev=rev)
        else:
            F = f32(zb[a[1], a[0]])
            v = {"point-at": F, "point-below": down(F), "point-above": up(F)}[kind]
            fi = m.face((a, a, a), (v, v, v), f"Z {kind}")
            lo = hi = a
        m.cell(f"Z {kind}", [fi], at=(x0, y0), kind=kind, lo=lo, hi=hi, floor=[2 * c, 2 * c + 1])
    return m.build("Z")


# (Not reachable: a back edge with an infinite or NaN depth.  The camera transform is dot3(rel, basis) = (x * bx.x + y * bx.y) + z * bx.z
#  for every axis: a non-finite z makes the camera-space x and y NaN (inf * 0), the signed area NaN and `area <= 0` false -- the face is a
#  front face and never enters the back-face list.  What remains of the issue's orthographic cases is below.)
ZO_CASES = [("negative", -3.0, -4.0), ("negative to positive", -30.0, 30.0), ("FLT_MAX", FLT_MAX, FLT_MAX), ("below FLT_MAX", down(FLT_MAX), down(FLT_MAX)),
            ("-FLT_MAX to FLT_MAX", -FLT_MAX, FLT_MAX), ("FLT_MAX to -FLT_MAX", FLT_MAX, -FLT_MAX), ("zero", 0.0, -0.0)]


@functools.lru_cache(maxsize=None)
def family_z_ortho():
    """Orthographic projection has no near reject and takes the camera depth as it is: negative and huge line depths, over
    a floor at depth 10 (even cells) or a negative floor (cells 4k + 1) or the cleared z-buffer (odd cells otherwise)"""
    per_row = Z_W // 16
    m = _Mesh("ortho", Z_W, 64)
    ncell = per_row * 4
    floor_of = {}
    for c in range(ncell):
        x0, y0 = 16 * (c % per_row), 16 * (c // per_row)
        if c % 2 == 0 or c % 4 == 1:
            floor_of[c] = m.floor(x0, y0, x0 + 16, y0 + 16, 10.0 if c % 2 == 0 else -3.5)
    for c in range(ncell):
        x0, y0 = 16 * (c % per_row), 16 * (c // per_row)
        tag, z0, z1 = ZO_CASES[(c // 2 + (c % 2) * 3) % len(ZO_CASES)]
        ga, gb = Z_GEOMS[c % 3]
        a, b = (x0 + ga[0], y0 + ga[1]), (x0 + gb[0], y0 + gb[1])
        fi = m.line(a, b, z0, z1, f"ZO {tag}", rev=c % 3 == 1)
        m.cell(f"ZO {tag}", [fi], at=(x0, y0), case=tag, lo=min(a, b), hi=max(a, b), floor=floor_of.get(c, []))
    return m.build("Z-ortho")


# ------------------------------------------------------------------------------------------------ family T
def family_t_box():
    """320 x 272 = 5 x 17 wire tiles.  Back edges whose clipped box is 4 x 16 = 64 tiles (tile route) and 5 x 13 = 65 tiles (global
    kernels), a front triangle whose hypotenuse has a 65-tile box, small edges of the other kind crossing each big edge, a floor."""
    m = _Mesh("fixed", 320, 272)
    m.floor(96, 96, 224, 208, 10.0)
    big64 = m.line((0, 0), (255, 255), 8.0, 12.0, "T box 64 tiles")
    big65 = m.line((0, 207), (319, 0), 12.0, 8.0, "T box 65 tiles")
    m.cell("T box 64 tiles", [big64], at=(0, 0), box=64); m.cell("T box 65 tiles", [big65], at=(0, 207), box=65)
    front = m.face(((2, 2), (319, 207), (0, 205)), (13.0, 13.0, 13.0), "T front 65 tiles")        # front-facing; its long edge: 5 x 13 tiles
    m.cell("T front 65 tiles", [front], at=(2, 2), box=65)
    small_front, small_back = [], []
    for k in range(12):
        x = 20 + 24 * k
        y = 207 - (207 * x) // 319                                  # on the 65-tile back edge
        small_front.append(m.face(((x - 3, y - 4), (x + 4, y + 3), (x - 4, y + 4)), (13.0, 13.0, 13.0), "T small front across the big back edge"))
        y2 = 2 + (205 * (x - 2)) // 317                             # on the front triangle's long edge
        small_back.append(m.line((x - 4, y2 + 3), (x + 4, y2 - 3), 8.0, 8.5, "T small back across the big front edge", rev=k % 2 == 1))
    m.cell("T small front across the big back edge", small_front, at=(20, 190)); m.cell("T small back across the big front edge", small_back, at=(20, 20))
    return m.build("T-box")


def family_t_union():
    """1024 x 256 = 16 x 16 wire tiles.  Faces with one edge along a tile row, one along a tile column and a big hypotenuse: the union
    of the two small boxes is 16 x 16 = 256 tiles (box by box), 16 x 9 = 144 (box by box), 16 x 8 = 128 (the simple path); both windings
    (a front face enters the overlay's list), a pair sharing its small edges with other depths."""
    m = _Mesh("fixed", 1024, 256)
    m.floor(300, 40, 700, 200, 10.0)
    for tag, a, b, c, tiles in (("256", (1, 8), (1020, 10), (3, 250), 256), ("144", (5, 5), (1021, 7), (8, 140), 144), ("128", (9, 3), (1019, 4), (12, 125), 128),
                                ("256 lower", (2, 245), (1022, 243), (60, 2), 256)):
        back = m.face((a, c, b), (8.0, 12.0, 9.0), f"T union {tag} back")
        m.cell(f"T union {tag} back", [back], at=a, union=tiles, winding="back")
        if tag == "256":
            again = m.face((b, a, c), (12.0, 11.0, 8.0), "T union 256 back again")
            m.cell("T union 256 back again", [again], at=a, union=tiles, winding="back")
    for tag, a, b, c, tiles in (("256", (40, 10), (1000, 12), (43, 250), 256), ("128", (50, 130), (1010, 131), (52, 250), 128)):
        fr = m.face((a, b, c), (13.0, 13.0, 13.0), f"T union {tag} front")
        m.cell(f"T union {tag} front", [fr], at=a, union=tiles, winding="front")
    return m.build("T-union")


def family_t_cap(extra):
    """64 x 16 = one wire tile.  256 proper back faces in 2 x 2 pixel cells of their own: 768 distinct edges, a full list; extra = 1: one
    more face, the list overflows and the frame falls back to the global kernels"""
    m = _Mesh("fixed", 64, 16)
    m.floor(0, 0, 64, 16, 10.0)
    ids = []
    for k in range(256):
        x, y = 2 * (k % 32), 2 * (k // 32)
        z = 9.0 if (k + k // 32) % 2 else 11.0
        ids.append(m.face(((x, y), (x, y + 1), (x + 1, y)), (z, z, z), "T cap"))
    for k in range(extra):
        ids.append(m.face(((1, 1), (1, 2), (2, 1)), (9.0, 9.0, 9.0), "T cap extra"))
    m.cell("T cap", ids, at=(0, 0))
    return m.build(f"T-cap-{256 + extra}")


def family_t_follow():
    """the small different mesh drawn after the overflowing frame on the same context"""
    m = _Mesh("fixed", 64, 16)
    m.floor(0, 0, 32, 16, 10.0)
    ids = [m.line((3 + 5 * k, 2), (6 + 5 * k, 13), 9.0 + (k % 2) * 2, 9.0, "T follow") for k in range(11)]
    m.cell("T follow", ids, at=(0, 0))
    return m.build("T-follow")


def family_t_seg(which):
    """64 x 16 = one wire tile.  Back triangles with one vertex left of the tile and two right of it: two edges of 64 steps inside the
    tile (4 segments of 16 steps each), the third outside.  '1536': 192 of them; '1537': the same and one edge of 4 steps; 'max': 256
    triangles whose third edge runs down the tile (two vertices in its last columns: at most 16 steps, 1 segment): up to 2304 segments, the most 256 faces can have."""
    m = _Mesh("fixed", 64, 16)
    m.floor(0, 0, 64, 16, 10.0)
    ids = []
    for k in range(256 if which == "max" else 192):
        p = (-2 - k, 1 + k % 14)
        if which == "max":
            q, r = (63, (5 * k) % 16), (48 + k % 15, (3 + 7 * (k // 15) + k) % 16)
        else:
            q, r = (66 + k, 14 - k % 13), (68 + k, 1 + k % 13)
        area = (q[0] - p[0]) * (r[1] - p[1]) - (r[0] - p[0]) * (q[1] - p[1])
        assert area != 0, (which, k)
        if area > 0:
            q, r = r, q                                     # (p, q, r) is a back face
        ids.append(m.face((p, q, r), (8.0 + (k % 5) * 0.5, 12.0 - (k % 3) * 0.5, 9.0 + (k % 7) * 0.5), "T seg"))
    if which == "1537":
        ids.append(m.line((60, 5), (70, 5), 9.0, 9.0, "T seg short"))
    m.cell("T seg", ids, at=(0, 0))
    return m.build(f"T-seg-{which}")


T_WALK_W, T_WALK_H = 256, 192
T_WALK = [("extent 16383", (-16283, 40), (100, 90), 8.0, 12.0), ("extent 16384", (-16284, 60), (100, 110), 8.0, 12.0), ("extent 20000", (-19850, 150), (150, 30), 12.0, 8.0),
          ("start beyond -2^20", (-1200000, 20), (200, 170), 8.0, 12.0), ("start beyond -2^20 in y", (30, -1100000), (220, 180), 8.0, 12.0),
          ("end beyond +2^20", (50, 100), (1300000, 9000), 9.0, 14.0)]


@functools.lru_cache(maxsize=None)
def family_t_walk():
    """float projection: edges the tile kernel cannot walk in 32 bits -- extents of 2^14 and more, start coordinates beyond +-2^20 --
    beside their neighbours that it can; and one of extent above 2^24 whose visible pixels all have step numbers above 2^24: its depth
    slopes from 10 to 1e6 over a floor at 999 970, so that the `step` that stops counting at 2^24 (t constant) decides every pixel"""
    m = _Mesh("float", T_WALK_W, T_WALK_H)
    m.floor(40, 20, 200, 170, 10.0)
    for tag, a, b, za, zb_ in T_WALK:
        for rev in (False, True):
            fi = m.line(a, b, za, zb_, f"T walk {tag}", rev=rev)
            m.cell(f"T walk {tag}", [fi], at=(100, 100), case=tag)
    sat_floor = m.floor(0, 176, 256, 192, 999970.0, "floor far")
    fi = m.line((-(2 ** 24 + 1000), 180), (200, 188), 10.0, 1.0e6, "T walk saturated step")
    m.cell("T walk saturated step", [fi], at=(0, 180), case="saturated", floor=sat_floor)
    return m.build("T-walk")


def _solve_x(target, y, width, height):
    """a world position whose float projection has `as i32` x equal to target at about row y (searched over camera depths and the
    neighbouring f32 values of the x coordinate); None if the projection cannot reach it"""
    for z in (3.0, 1.0, 11.0, 2.0, 5.0, 7.0):
        base = place("float", Camera(), np.array([float(target)]), np.array([float(y)]), np.array([z], np.float32), width, height)[0]
        offs = np.arange(-256, 257)
        cand = np.repeat(base[None, :], len(offs), axis=0)
        cand[:, 0] = base[0] + offs.astype(np.float32) * np.spacing(np.abs(base[0]))
        scr, _ = project(cand, Camera(), "float", width, height)
        for i in np.argsort(np.abs(offs), kind="stable"):
            if M._as_i32(scr[i][0]) == target and M._as_i32(scr[i][1]) == y:
                return cand[i]
    return None


# x of the far end, x of the near end, minor extent, refused?  (The float projection ends in `t + W / 2` with t a multiple of 64 out there: a
# tie that rounds to even, so the far end can only be a multiple of 128; the near end, inside the frame, supplies the rest.)  2^30 is the
# rule's limit; 715 827 884 the first extent at which 3 * dmaj - 2 * dmin - r_min reaches 2^31 with one minor step: `2 * err` overflows
# i32 in the reference's loop (2^31 / 3 = 715 827 882.7)
REFUSE_CASES = {"flat-2^30-1": (-((1 << 30) - 128), 127, 0, False), "flat-2^30": (-(1 << 30), 0, 0, True),
                "shallow-715827883": (-715827840, 43, 1, False), "shallow-715827884": (-715827840, 44, 1, True)}
REFUSE_W, REFUSE_H = 128, 16


@functools.lru_cache(maxsize=None)
def family_t_refuse(case):
    """float projection, 128 x 16: one edge from far left of the frame to a pixel inside it (positions solved by search), over a floor"""
    ax, bx, minor, _ = REFUSE_CASES[case]
    m = _Mesh("float", REFUSE_W, REFUSE_H)
    m.floor(0, 0, REFUSE_W, REFUSE_H, 10.0)
    wa = _solve_x(ax, 8, REFUSE_W, REFUSE_H)
    wb = _solve_x(bx, 8 + minor, REFUSE_W, REFUSE_H)
    assert wa is not None and wb is not None, case
    fi = m.face(((0, 0),) * 3, (8.0, 8.0, 8.0), f"T {case}", world=np.stack([wa, wb, wb]))
    m.cell(f"T {case}", [fi], at=(0, 8), case=case)
    return m.build("T-refuse-" + case)


def edge_hash(x0, y0, x1, y1):
    """b32_wire.hip's edge_hash, mirrored in Python integers"""
    M32 = 0xFFFFFFFF
    h = (x0 & M32) * 0x9E3779B1 & M32
    h = ((h ^ (h >> 15)) + (y0 & M32) * 0x85EBCA77) & M32
    h = ((h ^ (h >> 13)) + (x1 & M32) * 0xC2B2AE3D) & M32
    h = ((h ^ (h >> 16)) + (y1 & M32) * 0x27D4EB2F) & M32
    return h ^ (h >> 15)


def hash_chains(x_lo, y_lo, want=3, length=3):
    """`want` chains of `length` distinct direction-normalised edges inside the tile at (x_lo, y_lo) whose hashes are equal modulo
    1024, the smallest table; edges of at most 9 x 6 pixels, no two of one chain sharing both endpoints' pixels"""
    buckets = {}
    for x0 in range(x_lo + 1, x_lo + 54, 3):
        for y0 in range(y_lo + 1, y_lo + 10, 2):
            for dx in range(0, 9, 2):
                for dy in range(-4, 6, 3):
                    x1, y1 = x0 + dx, y0 + dy
                    if not ((x0, y0) < (x1, y1)) or not (y_lo <= y1 < y_lo + 16):
                        continue
                    buckets.setdefault(edge_hash(x0, y0, x1, y1) & 1023, []).append((x0, y0, x1, y1))
    chains = [v[:length] for _, v in sorted(buckets.items()) if len(v) >= length]
    assert len(chains) >= want, (x_lo, y_lo, len(chains))
    return chains[:want]


@functools.lru_cache(maxsize=None)
def family_t_hash():
    """256 x 64, fewer than 171 faces (the global table has 1024 slots, like the tile kernel's): in six tiles three chains each of three
    distinct edges with equal hash modulo 1024; the last edge of every chain comes twice, visible first or hidden first"""
    m = _Mesh("fixed", 256, 64)
    m.floor(0, 0, 256, 64, 10.0)
    n = 0
    for tx, ty in ((0, 0), (1, 1), (2, 2), (3, 3), (3, 0), (0, 3)):
        for chain in hash_chains(64 * tx, 16 * ty):
            first, later = ((9.0, 11.0), (11.0, 9.0))[n % 2]
            ids = [m.line(e[:2], e[2:], 9.0, 9.5, "T hash") for e in chain[:-1]]
            ids.append(m.line(chain[-1][:2], chain[-1][2:], first, first, "T hash last"))
            ids.append(m.line(chain[-1][:2], chain[-1][2:], later, later, "T hash last again", rev=n % 3 == 0))
            m.cell("T hash chain", ids, at=(64 * tx, 16 * ty), chain=chain, visible_first=first < 10.0)
            n += 1
    assert len(m.tags) < 171
    return m.build("T-hash")


# ------------------------------------------------------------------------------------------------ the sheets by name
BUILDERS = {"L-fixed": lambda: family_l("fixed"), "L-float": lambda: family_l("float"), "O": family_o, "Z": family_z, "Z-ortho": family_z_ortho,
            "T-box": family_t_box, "T-union": family_t_union, "T-cap-256": lambda: family_t_cap(0), "T-cap-257": lambda: family_t_cap(1), "T-follow": family_t_follow,
            "T-seg-1536": lambda: family_t_seg("1536"), "T-seg-1537": lambda: family_t_seg("1537"), "T-seg-max": lambda: family_t_seg("max"),
            "T-walk": family_t_walk, "T-hash": family_t_hash}
NAMES = list(BUILDERS)
BANDS = ((0, 21), (21, 22), (22, None))


@functools.lru_cache(maxsize=None)
def sheet(name):
    """the sheet of that name, built once per process"""
    if name.startswith("T-refuse-"):
        return family_t_refuse(name[len("T-refuse-"):])
    if name == "O-on-L":                      # (the cells stay in the top left 256 x 192: the sheet is a member of a batched frame with sheet L)
        return family_o(L_W, L_H, name="O-on-L")
    if name == "O-big-a":
        return family_o(BIG_W, BIG_H, BIG_BLOCKS, name=name)
    if name == "O-big-b":
        return family_o(BIG_W, BIG_H, BIG_BLOCKS, floor=9.75, rotate=11, name=name)
    return BUILDERS[name]()


def modes(sh):
    """the draws a sheet is compared in: [(label, settings keywords)]"""
    out = [("zbuffer", {}), ("painter", {"zbuffer": False})]
    if sh.name == "O":
        out += [("xray", {"xray": True}), ("cull off", {"cull": False}), ("overlay", {"overlay": True}), ("overlay painter", {"overlay": True, "zbuffer": False})]
    if sh.name in ("T-box", "T-union", "T-walk", "L-fixed"):
        out += [("overlay", {"overlay": True})]
    if sh.name.startswith("T-cap") or sh.name.startswith("T-seg") or sh.name.startswith("T-refuse"):
        out = out[:1]
    return out
