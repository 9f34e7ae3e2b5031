"""Coverage sheets: meshes in which every triangle has its own cell of the frame, so that every coverage decision of the fill is visible
in the frame instead of being painted over (tests/test_coverage_sheets.py).

Faces are untextured, opaque and flat-coloured; the colour encodes the triangle's index, so a pixel reports exactly one thing: which
triangle covered it last.  Vertices are placed on EXACT integer screen coordinates through the fixed-point perspective projection
(oracle/np_model.py: project_fixed, inverted by search), all at one camera depth, which is the path the closed-form walk and the span
route of the fill serve.  The families aim triangles at the limits where the fill's coverage routes change hands:

  A  every non-degenerate triangle of a 6 x 6 lattice, both windings (13 536 cells of pitch 11), plus prefixes of it
  B  doubled areas A on both sides of the span route's limit (A <= 8192, extent <= 512): "inside", "outside" and "mixed" sheets
  C  A on both sides of row_trim's regime changes (A about 4900, A = 2^20)
  D  lattice cells hanging over every frame edge
  E  wedges with far vertices: the 16-bit vertex form (|coordinate| <= 32767) and the exactness guards of k_setup (2^24)
  F  quads split along a diagonal: the only overlap, exactly the diagonal's pixels, decided by face order

This module only builds and labels; what the tests compare is always the oracle's frame."""
import itertools
import math
from dataclasses import dataclass, field

import numpy as np

from bonnie32_amd import abi, scenegen
from bonnie32_amd.rtypes import Camera, Color, RasterSettings, make_faces, make_vertices
from oracle import np_model as M

DEPTH = 100.0                       # camera depth of every vertex
CLEAR = Color(20, 22, 28)           # (not an RGB555 colour: no triangle can produce it)
SPAN_MAX_AREA, SPAN_MAX_EXT = 8192, 512
LATTICE, PITCH = 6, 11              # family A: lattice points 0..5 in cells of pitch 11 (coprime to the 64-px tile)
MAX_PIXELS = 1_700_000


# ------------------------------------------------------------------------------------------------ integer geometry
def doubled_area(t):
    (x1, y1), (x2, y2), (x3, y3) = [(int(a), int(b)) for a, b in t]
    return abs((y2 - y3) * (x1 - x3) + (x3 - x2) * (y1 - y3))


def extent(t):
    t = np.asarray(t, np.int64)
    return int(max(np.abs(t - np.roll(t, 1, axis=0)).max(), 0))


def span_eligible(t):
    """what the span route takes: 1 <= A <= 8192 and every edge component at most 512 (b32_cover.h)"""
    return 1 <= doubled_area(t) <= SPAN_MAX_AREA and extent(t) <= SPAN_MAX_EXT


def int_inside(t, x0, y0, x1, y1):
    """The closed integer triangle s*w0 >= 0, s*w1 >= 0, A - s*w0 - s*w1 >= 0 on the window [x0, x1) x [y0, y1)."""
    (xa, ya), (xb, yb), (xc, yc) = [(int(a), int(b)) for a, b in t]
    area = (yb - yc) * (xa - xc) + (xc - xb) * (ya - yc)
    s = -1 if area < 0 else 1
    X, Y = np.meshgrid(np.arange(x0, x1, dtype=np.int64), np.arange(y0, y1, dtype=np.int64))
    e0 = s * ((yb - yc) * (X - xc) + (xc - xb) * (Y - yc))
    e1 = s * ((yc - ya) * (X - xc) + (xa - xc) * (Y - yc))
    return (e0 >= 0) & (e1 >= 0) & (abs(area) - e0 - e1 >= 0)


def setup_quantities(t, width, height):
    """What k_setup's exactness guard looks at (b32_setup.hip, "Closed-form eligibility"), in plain integers: the surface after the
    back-face swap of v2 / v3, its clipped box, the largest coordinate, 2 * amax * dmax, and the largest corner product or sum."""
    (x1, y1), (x2, y2), (x3, y3) = [(int(a), int(b)) for a, b in t]
    if (x2 - x1) * (y3 - y1) - (x3 - x1) * (y2 - y1) <= 0:
        x2, y2, x3, y3 = x3, y3, x2, y2
    min_x, max_x = max(min(x1, x2, x3), 0), min(max(x1, x2, x3) + 1, width)
    min_y, max_y = max(min(y1, y2, y3), 0), min(max(y1, y2, y3) + 1, height)
    a0, b0, a1, b1 = y2 - y3, x3 - x2, y3 - y1, x1 - x3
    dxs, dys = (min_x - x3, max_x - 1 - x3), (min_y - y3, max_y - 1 - y3)
    amax = max(abs(a0), abs(b0), abs(a1), abs(b1))
    dmax = max(abs(v) for v in dxs + dys)
    corner = 0
    for dx in dxs:
        for dy in dys:
            p0, q0, p1, q1 = a0 * dx, b0 * dy, a1 * dx, b1 * dy
            corner = max(corner, abs(p0), abs(q0), abs(p1), abs(q1), abs(p0 + q0), abs(p1 + q1))
    cmax = max(abs(v) for v in (x1, y1, x2, y2, x3, y3))
    quick = 2 * amax * dmax
    slow = cmax > (1 << 22) or (quick >= (1 << 24) and corner >= (1 << 24))
    return {"cmax": cmax, "quick": quick, "corner": corner, "slow": slow, "narrow": not slow and cmax <= 32767,
            "empty": min_x >= max_x or min_y >= max_y}


# ------------------------------------------------------------------------------------------------ exact screen placement
class ScreenMap:
    """World coordinates whose fixed-point projection is a given integer screen coordinate, for one frame size and depth: with the
    default camera a column depends on world x alone and a row on world y alone, so each axis is inverted by a sweep of its own."""

    def __init__(self, width, height, depth=DEPTH):
        self.width, self.height, self.depth = width, height, depth
        vs = (min(width, height) / M.K("project_fixed.viewport_div")) * M.K("project_fixed.viewport_frac")
        self.per_px = (depth + float(M.K("project_fixed.distance"))) / float(M.K("project_fixed.scale")) / float(vs)    # world units per pixel
        self._cache = ({}, {})

    def _solve(self, targets, axis):
        t = np.asarray(targets, np.int64)
        half = (self.width // 2, self.height // 2)[axis]
        est = (t + 0.5 - half) * self.per_px
        # 64 candidates per pixel where the formats allow it (fixed point: 2^-12; f32 spacing far out), 1.5 px to either side
        step = np.maximum(np.maximum(self.per_px / 64.0, 2.0 ** -12), np.spacing(np.abs(est).astype(np.float32)).astype(np.float64))
        n = np.ceil(1.5 * self.per_px / step).astype(np.int64).max()
        j = np.arange(-n, n + 1)
        cand = (est[:, None] + j[None, :] * step[:, None]).astype(np.float32)
        pos = np.zeros((cand.size, 3), np.float32)
        pos[:, axis] = cand.reshape(-1)
        pos[:, 2] = self.depth
        got = M.project_fixed(pos, Camera(), self.width, self.height)[axis].reshape(cand.shape)
        out = np.zeros(len(t), np.float32)
        for i in range(len(t)):
            hit = np.nonzero(got[i] == t[i])[0]
            assert len(hit), f"screen coordinate {t[i]} (axis {axis}) is not reachable at depth {self.depth} on a {self.width} x {self.height} frame"
            out[i] = cand[i, hit[len(hit) // 2]]
        return out

    def world(self, targets, axis):
        cache = self._cache[axis]
        t = np.asarray(targets, np.int64)
        missing = sorted(set(t.tolist()) - set(cache))
        if missing:
            cache.update(zip(missing, self._solve(missing, axis)))
        return np.array([cache[v] for v in t.tolist()], np.float32)


# ------------------------------------------------------------------------------------------------ sheets
@dataclass
class Sheet:
    name: str
    family: str
    width: int
    height: int
    tris: np.ndarray                # [n, 3, 2] target screen coordinates, face order
    cells: np.ndarray               # [m, 4] x0, y0, x1, y1 (half open, clipped to the frame)
    cell_of: np.ndarray             # [n] cell of every triangle
    scene: scenegen.Scene
    overlap: bool = False           # family F: two triangles per cell
    labels: list = field(default_factory=list)
    _owner: np.ndarray = None
    _oracle: dict = field(default_factory=dict)

    @property
    def n(self):
        return len(self.tris)

    def settings(self, zbuffer=False, fmt8=False):
        st = RasterSettings.benchmark()
        st.backface_cull = False
        st.use_zbuffer = zbuffer
        st.use_rgb555 = not fmt8
        return st

    def owner(self):
        """[H, W] cell index of every pixel, -1 between the cells"""
        if self._owner is None:
            own = np.full((self.height, self.width), -1, np.int32)
            for c, (x0, y0, x1, y1) in enumerate(self.cells):
                assert (own[y0:y1, x0:x1] == -1).all(), f"{self.name}: cell {c} overlaps another"
                own[y0:y1, x0:x1] = c
            self._owner = own
        return self._owner

    def oracle(self, O, zbuffer=False, fmt8=False, dump=False):
        """(pixels [H, W, 4], zbuffer bits, timings, stage dump) of the reference restatement; computed once per mode and shared"""
        key = (zbuffer, fmt8)
        if key not in self._oracle:
            sc = self.scene
            fb = O.Framebuffer(self.width, self.height)
            fb.clear(sc.clear_color)
            st = self.settings(zbuffer, fmt8)
            if fmt8:
                rc, tm, d = O.render_mesh(fb, sc.vertices, sc.faces, [], sc.camera, st, dump=True)
            else:
                rc, tm, d = O.render_mesh_15(fb, sc.vertices, sc.faces, [], sc.camera, st, dump=True)
            assert rc == 0
            px = fb.image().copy(); px.setflags(write=False)
            zb = fb.zbuffer.view(np.uint32).copy(); zb.setflags(write=False)
            self._oracle[key] = (px, zb, tm, d)
        return self._oracle[key]

    def decode(self, image):
        """[H, W] triangle index painted at every pixel of an RGB555-path frame, -1 where the clear colour is left"""
        img = image.reshape(self.height, self.width, 4).astype(np.int64)
        code = (img[..., 0] >> 3) | ((img[..., 1] >> 3) << 5) | ((img[..., 2] >> 3) << 10)
        clear = (img[..., 0] == CLEAR.r) & (img[..., 1] == CLEAR.g) & (img[..., 2] == CLEAR.b)
        return np.where(clear, -1, code - 1)

    def covered(self, idx_map, i):
        """pixels of triangle i's cell that carry its colour, and the cell's window"""
        x0, y0, x1, y1 = self.cells[self.cell_of[i]]
        return idx_map[y0:y1, x0:x1] == i, (x0, y0, x1, y1)

    def describe(self, i):
        t = self.tris[i]
        return f"triangle {i} of {self.name}: cell {tuple(int(v) for v in self.cells[self.cell_of[i]])}, vertices {[tuple(int(v) for v in p) for p in t]}, A = {doubled_area(t)}"

    def first_difference(self, got, want, route):
        """'' when the frames are equal, else a message naming the route, the first offending cell, its vertices and its A"""
        g = np.asarray(got).reshape(self.height, self.width, -1)
        w = np.asarray(want).reshape(self.height, self.width, -1)
        bad = (g != w).any(axis=2)
        if not bad.any():
            return ""
        y, x = [int(v[0]) for v in np.nonzero(bad)]
        c = int(self.owner()[y, x])
        who = [i for i in np.nonzero(self.cell_of == c)[0]] if c >= 0 else []
        what = "; ".join(self.describe(i) for i in who[:2]) if who else "outside every cell"
        return (f"[{route}] {int(bad.sum())} pixels differ, first at ({x}, {y}): got {g[y, x].tolist()}, oracle {w[y, x].tolist()}; {what}")


def _vertex_colour(i):
    """r, g, b = 4 q + 2 over the 5-bit digits q of i + 1: every digit lands in the middle of its RGB555 step, so the quantised colour
    is unique per triangle, never black and never the clear colour (asserted on the oracle's frame by check_placement)"""
    code = i + 1
    assert 0 < code < 32768
    return [4 * ((code >> s) & 31) + 2 for s in (0, 5, 10)]


def make_sheet(name, family, width, height, tris, cells, cell_of=None, overlap=False, labels=None):
    tris = np.asarray(tris, np.int64).reshape(-1, 3, 2)
    n = len(tris)
    assert width * height <= MAX_PIXELS, (name, width, height)
    cells = np.asarray(cells, np.int64).reshape(-1, 4).copy()
    cells[:, [0, 2]] = np.clip(cells[:, [0, 2]], 0, width)
    cells[:, [1, 3]] = np.clip(cells[:, [1, 3]], 0, height)
    cell_of = np.arange(n) if cell_of is None else np.asarray(cell_of, np.int64)
    sm = ScreenMap(width, height)
    v = make_vertices(3 * n)
    v["pos"][:, 0] = sm.world(tris[:, :, 0].reshape(-1), 0)
    v["pos"][:, 1] = sm.world(tris[:, :, 1].reshape(-1), 1)
    v["pos"][:, 2] = DEPTH
    v["normal"] = (0.0, 0.0, -1.0)
    col = np.repeat(np.array([_vertex_colour(i) for i in range(n)], np.uint8), 3, axis=0)
    v["r"], v["g"], v["b"] = col[:, 0], col[:, 1], col[:, 2]
    v["blend"] = abi.OPAQUE
    f = make_faces(n)                                      # NO_TEXTURE, OPAQUE, editor_alpha 255
    f["v"] = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    st = RasterSettings.benchmark()
    st.backface_cull = False
    sc = scenegen.Scene(name, width, height, v, f, [], [], Camera(), st, CLEAR)
    return Sheet(name, family, width, height, tris, cells, cell_of, sc, overlap, labels or [])


def check_placement(sheet, O):
    """Every vertex landed on its target (the oracle's stage dump), every pixel of a cell carries the clear colour or the colour of
    (one of) the cell's own triangle(s), and nothing is drawn between the cells.  Returns the index map of the oracle's frame."""
    px, _, tm, d = sheet.oracle(O)
    assert np.array_equal(d["sx"], sheet.tris[:, :, 0].reshape(-1)), f"{sheet.name}: a vertex missed its target column"
    assert np.array_equal(d["sy"], sheet.tris[:, :, 1].reshape(-1)), f"{sheet.name}: a vertex missed its target row"
    idx = sheet.decode(px)
    own = sheet.owner()
    drawn = idx >= 0
    assert not (drawn & (own < 0)).any(), f"{sheet.name}: {int((drawn & (own < 0)).sum())} pixels drawn outside every cell"
    # the colour really is the quantised code (every channel expands a 5-bit value), so decode() loses nothing
    rgb = px[..., :3][drawn].astype(np.int64)
    assert np.array_equal(rgb, ((rgb >> 3) << 3) | (rgb >> 5)), f"{sheet.name}: a pixel is no RGB555 colour"
    assert (idx[drawn] < sheet.n).all()
    assert np.array_equal(sheet.cell_of[idx[drawn]], own[drawn]), f"{sheet.name}: a pixel carries the colour of another cell's triangle"
    return idx


# ------------------------------------------------------------------------------------------------ packing and shapes
def shelf_pack(sizes, width, margin=(3, 2), gap=2):
    """Cells of the given (w, h) in rows, tallest first; returns (x0, y0) per cell in the given order, and the frame height used."""
    order = sorted(range(len(sizes)), key=lambda i: (-sizes[i][1], -sizes[i][0], i))
    pos = [None] * len(sizes)
    x, y, row_h = margin[0], margin[1], 0
    for i in order:
        w, h = sizes[i]
        assert w + margin[0] <= width, (w, width)
        if x + w > width:
            x, y, row_h = margin[0], y + row_h + gap, 0
        pos[i] = (x, y)
        x += w + gap
        row_h = max(row_h, h)
    return pos, y + row_h + 1


def shapes_of_area(A, aspects=(1.0, 0.5, 2.0)):
    """Integer triangles (0, 0), (w, y1), (x2, h) with w h - x2 y1 == A exactly, one per aspect ratio h / w, found by a bounded scan
    (a random search finds too few: 8191 is prime).  Slanted edges are preferred to axis-parallel ones."""
    out = []
    for asp in aspects:
        h0 = max(1, round(math.sqrt(A * asp)))
        found = None
        for dh in range(0, 64):
            for h in ((h0 + dh, h0 - dh) if dh else (h0,)):
                if h < 1 or found:
                    continue
                for y1, x2 in itertools.product(range(1, 10), range(1, 10)):
                    if (A + x2 * y1) % h == 0:
                        w = (A + x2 * y1) // h
                        if x2 <= w and y1 <= h:
                            found = ((0, 0), (w, y1), (x2, h)); break
            if found:
                break
        if found is None:
            found = ((0, 0), (A, 0), (0, 1))
        assert doubled_area(found) == A
        if found not in out:
            out.append(found)
    return out


def _variants(shape, k):
    """both windings of a shape, its vertex order rotated by k (which vertex is v3 decides the edge coefficients)"""
    p = [shape[(j + k) % 3] for j in range(3)]
    return [p, [p[0], p[2], p[1]]]


def _packed_sheet(name, family, width, shapes, pad=1, labels=None):
    """shapes: triangles with their own origin; every one gets a cell of its bounding box plus `pad`, packed into rows"""
    shapes = [np.asarray(s, np.int64) for s in shapes]
    mins = [s.min(axis=0) for s in shapes]
    sizes = [tuple((s.max(axis=0) - m + 1 + 2 * pad).tolist()) for s, m in zip(shapes, mins)]
    pos, height = shelf_pack(sizes, width)
    tris, cells = [], []
    for s, m, (w, h), (x, y) in zip(shapes, mins, sizes, pos):
        tris.append(s - m + (x + pad, y + pad))
        cells.append((x, y, x + w, y + h))
    return make_sheet(name, family, width, height, tris, cells, labels=labels)


# ------------------------------------------------------------------------------------------------ the families
def lattice_triangles():
    """every non-degenerate triangle with vertices in the 6 x 6 lattice, both windings, in a fixed scattered order (so that every prefix
    holds all kinds of shapes)"""
    pts = [(i, j) for j in range(LATTICE) for i in range(LATTICE)]
    base = []
    for a, b, c in itertools.combinations(pts, 3):
        if doubled_area((a, b, c)):
            base += [(a, b, c), (a, c, b)]
    n = len(base)
    assert n == 13536 and math.gcd(7919, n) == 1
    return [base[(i * 7919) % n] for i in range(n)]


def _lattice_sheet(name, family, width, height, shapes, margin):
    cols = (width - margin[0] - LATTICE) // PITCH + 1
    tris, cells = [], []
    for i, s in enumerate(shapes):
        x, y = margin[0] + PITCH * (i % cols), margin[1] + PITCH * (i // cols)
        tris.append(np.asarray(s, np.int64) + (x, y))
        cells.append((x - 2, y - 2, x - 2 + PITCH - 1, y - 2 + PITCH - 1))
    assert max(t[:, 0].max() for t in tris) < width and max(t[:, 1].max() for t in tris) < height
    return make_sheet(name, family, width, height, tris, cells)


def family_a(which):
    lat = lattice_triangles()
    if which == "A":                    # above the 8192 faces from which a resident mesh is drawn from packed streams
        return _lattice_sheet("A", "A", 1283, 1292, lat, (3, 2))
    if which == "A-2048":               # in-kernel list collection
        return _lattice_sheet("A-2048", "A", 1283, 2 + PITCH * 18, lat[:2048], (3, 2))
    if which == "A-55":                 # less than one tile
        return _lattice_sheet("A-55", "A", 55, 55, lat[:25], (2, 2))
    if which == "A-63x65":              # one tile plus a pixel
        return _lattice_sheet("A-63x65", "A", 63, 65, lat[:25], (5, 6))
    raise KeyError(which)


B_AREAS = (1, 2, 8190, 8191, 8192, 8193, 8194, 9999, 10000, 10001, 12000, 20000, 40000)


def family_b_shapes():
    shapes = []
    for k, A in enumerate(B_AREAS):
        for j, s in enumerate(shapes_of_area(A)):
            shapes += _variants(s, k + j)
    # needles: the extent alone decides (A is small); transposed, so that the row steps H as well as the pixel steps G carry it
    for e in (511, 512, 513):
        for s in (((0, 0), (e, 0), (0, 1)), ((0, 0), (e, 3), (2, 1)), ((0, 0), (e, 0), (0, 16)) if e == 512 else None):
            if s is None:
                continue
            for tr in (False, True):
                q = tuple((y, x) for x, y in s) if tr else s
                shapes += _variants(q, e)
    return shapes


def family_b(which):
    shapes = family_b_shapes()
    inside = [s for s in shapes if span_eligible(s)]
    outside = [s for s in shapes if not span_eligible(s)]
    assert inside and outside
    if which == "B-inside":
        return _packed_sheet("B-inside", "B", 1021, inside)
    if which == "B-outside":
        return _packed_sheet("B-outside", "B", 1021, outside)
    if which == "B-mixed":              # alternating in face order; packed by height, so both kinds share tiles
        mixed = [s for pair in itertools.zip_longest(inside, outside) for s in pair if s is not None]
        return _packed_sheet("B-mixed", "B", 1281, mixed)
    raise KeyError(which)


C_SMALL = (4898, 4899, 4900, 4901, 4902, 4903)      # T = 1.02e-4 A reaches half an edge-value unit at A about 4900
C_BIG = {1048575: ((0, 0), (1024, 1), (1, 1024)), 1048576: ((0, 0), (1025, 32), (32, 1024)), 1048577: ((0, 0), (1024, 31), (33, 1025))}
C_SHIFTS = ("centre", "left", "right", "top", "bottom")


def family_c(which):
    if which == "C-small":
        shapes = []
        for k, A in enumerate(C_SMALL):
            for j, s in enumerate(shapes_of_area(A)):
                shapes += _variants(s, k + j)
        return _packed_sheet("C-small", "C", 701, shapes)
    # C-<A>-<shift>: one triangle of about 1024 px per frame; shifted, half of it is off-screen on one side
    _, a, shift = which.split("-")
    A = int(a)
    s = np.asarray(C_BIG[A], np.int64)
    assert doubled_area(s) == A
    W = H = 1101
    off = {"centre": (37, 41), "left": (-512, 41), "right": (W - 512, 41), "top": (37, -512), "bottom": (37, H - 512)}[shift]
    k = C_SHIFTS.index(shift)
    tri = _variants([tuple(p) for p in (s + off).tolist()], k)[k & 1]
    return make_sheet(which, "C", W, H, [tri], [(0, 0, W, H)])


C_NAMES = ["C-small"] + [f"C-{A}-{s}" for A in C_BIG for s in C_SHIFTS]


def family_d():
    """Lattice cells over every frame edge by 1 to 5 px: vertices at negative coordinates and at W, W + 1, H, H + 1 and beyond."""
    W, H = 203, 190
    lat = lattice_triangles()
    tris, cells = [], []
    k = 0
    def put(x, y):
        nonlocal k
        tris.append(np.asarray(lat[(k * 97) % len(lat)], np.int64) + (x, y)); k += 1
        cells.append((x - 2, y - 2, x - 2 + PITCH - 1, y - 2 + PITCH - 1))
    nx, ny = (W - 16) // PITCH, (H - 30) // PITCH
    for i in range(nx):
        put(9 + PITCH * i, -(1 + i % 5))                      # over the top edge by 1..5
        put(9 + PITCH * i, H - LATTICE + 1 + i % 5)           # lattice row 5 at H .. H + 4
    for j in range(ny):
        put(-(1 + j % 5), 15 + PITCH * j)
        put(W - LATTICE + 1 + j % 5, 15 + PITCH * j)
    for x, y in ((-3, -2), (W - 3, -4), (-1, H - 2), (W - 4, H - 3)):      # the corners: over two edges at once
        put(x, y)
    return make_sheet("D", "D", W, H, tris, cells)


def _wedge(left, right, y0, h, apex_left=True):
    """a wedge across the frame in the rows y0 .. y0 + h: one vertex far on one side, two far on the other"""
    if apex_left:
        return [(-left, y0 + h // 2), (right, y0), (right, y0 + h)]
    return [(right, y0 + h // 2), (-left, y0 + h), (-left, y0)]


def family_e(transposed=False):
    """Wedges with far vertices, one strip of rows each (transposed: one strip of columns each, so that y carries the far values)."""
    W = 301
    cases = []      # (left, right, h, apex_left, label, what setup_quantities must say)
    # the 16-bit vertex form: |coordinate| <= 32767
    for left, right in ((32767, 32767), (32766, 32767), (32768, 32767), (32767, 32768), (32769, 32766), (32768, 32768), (32767, 40000), (40000, 32767)):
        cases.append((left, right, 5, left <= right, "cmax16", {"narrow": max(left, right) <= 32767}))
    cases.append((32767, 32767, 4, False, "cmax16", {"narrow": True}))
    cases.append((32768, 32767, 4, False, "cmax16", {"narrow": False}))

    def scan(lo, hi, h, key):
        """the last size n in [lo, hi) whose wedge keeps `key` below 2^24 and the first that does not"""
        prev = None
        for n in range(lo, hi):
            q = setup_quantities(_wedge(n, n, 10, h), W, 4096)
            if q[key] >= (1 << 24):
                assert prev is not None, (key, lo)
                return prev, n
            prev = n
        raise AssertionError((key, lo, hi))

    b, a = scan(1500, 2600, 6, "quick")                     # 2 * amax * dmax on both sides of 2^24 (the corner products stay far below)
    for n, over in ((b - 1, False), (b, False), (a, True), (a + 1, True)):
        cases.append((n, n, 6, True, "quick", {"quick_over": over, "slow": False}))
        cases.append((n, n, 6, False, "quick", {"slow": False}))
    b, a = scan((1 << 18) - 64, (1 << 18) + 64, 32, "corner")   # one corner product (b * dy, 32 rows) on both sides of 2^24: F_SLOW
    for n, over in ((b - 1, False), (b, False), (a, True), (a + 1, True)):
        cases.append((n, n, 32, True, "corner", {"quick_over": True, "slow": over}))
    tris, cells, labels = [], [], []
    y = 3
    for left, right, h, apex_left, label, _ in cases:
        for wind in (0, 1):
            w = _wedge(left, right, y, h, apex_left)
            tris.append(w if wind == 0 else [w[0], w[2], w[1]])
            cells.append((0, y, W, y + h + 1))
            y += h + 3
    H = y + 2
    assert min(W, H) >= 200
    n = 0
    for left, right, h, apex_left, label, want in cases:
        for wind in (0, 1):
            q = setup_quantities(tris[n], W, H)
            assert not q["empty"]
            if "narrow" in want:
                assert q["narrow"] == want["narrow"], (tris[n], q)
            if "quick_over" in want:
                assert (q["quick"] >= (1 << 24)) == want["quick_over"], (tris[n], q)
            if "slow" in want:
                assert q["slow"] == want["slow"], (tris[n], q)
            labels.append((label, q))
            n += 1
    tris = np.asarray(tris, np.int64)
    cells = np.asarray(cells, np.int64)
    if transposed:
        return make_sheet("E-columns", "E", H, W, tris[:, :, ::-1], cells[:, [1, 0, 3, 2]], labels=labels)
    return make_sheet("E-rows", "E", W, H, tris, cells, labels=labels)


F_QUADS = ((8, 8), (12, 8), (13, 7), (5, 30), (30, 30), (70, 70), (1, 1))


def family_f():
    """Quads split along either diagonal, the halves in both face orders and both windings: both closed triangles claim the pixels
    of the diagonal, the order of the faces decides (painter's at equal depth: the later face; z-buffer, strict `<`: the first)."""
    halves, sizes = [], []
    for w, h in F_QUADS:
        a, b, c, d = (0, 0), (w, 0), (w, h), (0, h)
        for diag in (0, 1):
            t1, t2 = ([a, b, c], [a, c, d]) if diag == 0 else ([a, b, d], [b, c, d])
            for order in (0, 1):
                for wind in (0, 1):
                    p, q = (t1, t2) if order == 0 else (t2, t1)
                    if wind:
                        p, q = [p[0], p[2], p[1]], [q[1], q[0], q[2]]
                    halves.append((p, q)); sizes.append((w + 3, h + 3))
    W = 331
    pos, H = shelf_pack(sizes, W)
    tris, cells, cell_of = [], [], []
    for c, ((p, q), (w, h), (x, y)) in enumerate(zip(halves, sizes, pos)):
        for t in (p, q):
            tris.append(np.asarray(t, np.int64) + (x + 1, y + 1)); cell_of.append(c)
        cells.append((x, y, x + w, y + h))
    sh = make_sheet("F", "F", W, H, tris, cells, cell_of=cell_of, overlap=True)
    # the overlap of the two closed triangles of a cell is exactly the lattice points of the shared diagonal
    for c in range(len(cells)):
        x0, y0, x1, y1 = sh.cells[c]
        ta, tb = sh.tris[2 * c], sh.tris[2 * c + 1]
        both = int_inside(ta, x0, y0, x1, y1) & int_inside(tb, x0, y0, x1, y1)
        shared = [tuple(p) for p in ta.tolist() if list(p) in tb.tolist()]
        assert len(shared) == 2
        (xa, ya), (xb, yb) = shared
        g = math.gcd(abs(xb - xa), abs(yb - ya))
        on = np.zeros_like(both)
        for k in range(g + 1):
            on[ya + (yb - ya) // g * k - y0, xa + (xb - xa) // g * k - x0] = True
        assert np.array_equal(both, on), f"F: cell {c} overlaps on more or less than its diagonal"
    return sh


BUILDERS = {"A": lambda: family_a("A"), "A-2048": lambda: family_a("A-2048"), "A-55": lambda: family_a("A-55"), "A-63x65": lambda: family_a("A-63x65"),
            "B-inside": lambda: family_b("B-inside"), "B-outside": lambda: family_b("B-outside"), "B-mixed": lambda: family_b("B-mixed"),
            **{n: (lambda n=n: family_c(n)) for n in C_NAMES},
            "D": family_d, "E-rows": lambda: family_e(False), "E-columns": lambda: family_e(True), "F": family_f}
NAMES = list(BUILDERS)
_sheets = {}


def sheet(name):
    """the sheet of that name, built once per process"""
    if name not in _sheets:
        _sheets[name] = BUILDERS[name]()
    return _sheets[name]


# ------------------------------------------------------------------------------------------------ the device side
def gpu_draw(ctx, sh, resident=False, zbuffer=False, fmt8=False, band=None):
    """One frame of the sheet through the C ABI -> (framebuffer object, timings)."""
    from bonnie32_amd import rasterizer as R
    sc = sh.scene
    st = sh.settings(zbuffer, fmt8)
    fb = R.Framebuffer(sh.width, sh.height, ctx)
    fb.clear(sc.clear_color)
    if band:
        fb.set_band(*band)
    if resident:
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, textures8=[]) if fmt8 else R.ResidentScene(fb, sc.vertices, sc.faces, [])
        tm = rs.render(sc.camera, st)
    elif fmt8:
        tm = R.render_mesh(fb, sc.vertices, sc.faces, [], sc.camera, st)
    else:
        tm = R.render_mesh_15(fb, sc.vertices, sc.faces, [], sc.camera, st)
    return fb, tm
