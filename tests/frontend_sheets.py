"""Front-end sheets: meshes in which every face has a cell of its own (or shares one screen triangle with the few faces it is ordered
against), so that every decision of k_setup's front end -- near reject, area sign, fog cull, painter's key and class, draw order -- and
the per-pixel priority the fill derives from it is a pixel of the frame or an entry of the draw order (tests/test_frontend_sheets.py).

Faces are untextured, unlit, undithered and flat-coloured; the colour encodes the face index.  A sheet is built for ONE projection:
positions are solved from the wanted screen point and camera depth of every vertex (`place`), then projected again with the model's own
arithmetic (`project`: np_model.project_fixed / dot3 and the float and orthographic formulas of np_model.render_mesh_15); the census of
the test module reads the exact bits from that projection, never from the intent.

  N  near reject: camera depth 0.1f, its two neighbours, 0.0, -0.0, -0.1 on every subset of the three vertex slots; identity camera
     and a camera rotated about two axes and translated (positions snapped by a seeded search until dot3 gives the wanted bits)
  A  area sign and empty surfaces: integer collinear / coincident / area +-1 triples, and -- float and orthographic projection -- searched
     near-collinear triples whose f32 signed area is 0 where the exact one is not, or changes its verdict under one fused multiply-add
  F  fog cull: camera depth at cull_distance and its neighbours, for the distances 12, 0 and -1; drawn with six cull distances
  K  order: 2 to 4 faces on one screen triangle, both face orders: keys one ulp apart, equal keys, non-associative sums, /3 against
     * 1/3, the + 5.0 of perspective depth, huge / negative / zero / denormal / infinite orthographic keys, the transparent class
  D  per-pixel depth: 16 x 16 cells, two faces whose vertex depths cross inside the triangle
  V  (no sheet) tiny meshes with one NaN-depth face in every composition of the reference's "NaN key panics" rule

The back-face swap of the attributes shows on a few cells of family A (drawn with culling off, both windings): some whose three vertices
have three different colours, some that carry an 8 x 8 identity-address texture, one corner of it per vertex.

Not reachable: a transparent face whose key 0x80000000 | (0x7FFFFFFF - bits(mean depth)) equals the sentinel 0xFFFFFFFF needs a mean
depth of +0.0.  Fixed-point and float projection add 5.0 to a camera depth above 0.1, so their mean depth is above 5; the orthographic
key is ~zsort_key(z), which is 0xFFFFFFFF only for the bit pattern of a NaN.  The one way in is a NaN mean depth, which k_setup replaces
by +0.0 before packing: a transparent NaN face that is alone in its list (family V, "nan_transparent_alone") is drawn with the patched key.

This module only builds, projects and caches; what the tests compare is always the oracle's frame."""
import functools
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from bonnie32_amd import abi
from bonnie32_amd.rtypes import Camera, Color, RasterSettings, Texture, Texture15, make_faces, make_vertices
from oracle import np_model as M

f32 = np.float32
W, H = 256, 192
CLEAR = Color(20, 22, 28)            # (not an RGB555 colour: no face can produce it)
PROJS = ("fixed", "float", "ortho")
NEAR = f32(M.K("near_plane"))
DIST = float(M.K("mesh.distance"))
ORTHO = (1.0, -200.0, -200.0)        # zoom and centre: camera-space x and y are negative all over the frame, so that x * 0 + y * 0 + z keeps a -0.0
AREA_EPS = f32(M.K("fill.area_eps"))
FOG_COLOR = Color(90, 20, 20)
FOG_DISTANCES = {"normal": 12.0, "zero": 0.0, "negative": -1.0, "+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan")}
SLOTS = ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2))
SHAPES = (((1, 1), (6, 1), (1, 6)), ((6, 6), (1, 6), (6, 1)), ((1, 2), (6, 3), (3, 6)))      # all front-facing on the screen
SHAPE_D = ((1, 1), (14, 1), (1, 14))


def bits(x):
    return int(f32(x).view(np.uint32))


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


def down(x):
    return np.nextafter(f32(x), f32(-np.inf))


def fog(name):
    """(start, falloff, cull_distance, colour): the start is so far out that every fog factor is 0 and the colours stay the faces' own"""
    return (1e30, 1.0, FOG_DISTANCES[name], FOG_COLOR)


def rotated_camera():
    """Rotated about two axes and translated.  The angles are small on purpose: dot3 adds (x * bz.x + y * bz.y) + z * bz.z, and the sum can
    have the bits of 0.1f (an odd multiple of 2^-27) only where both summands are below 0.125, i.e. where the view axis has small x and y
    components; with the angles of a free camera no position at all gives camera depth 0.1f."""
    cy, sy, cx, sx = (f32(t) for t in (np.cos(0.02), np.sin(0.02), np.cos(0.015), np.sin(0.015)))
    return Camera(position=(3.25, -1.5, -2.0), basis_x=(cy, 0.0, -sy), basis_y=(sx * sy, cx, sx * cy), basis_z=(cx * sy, -sx, cx * cy))


# ------------------------------------------------------------------------------------------------ exact f32 arithmetic
def rne32(q):
    """A rational rounded to the nearest f32, ties to even (subnormals and overflow to infinity included)."""
    q = Fraction(q)
    if q == 0:
        return f32(0.0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n, r = divmod(a / quantum, 1)
    n = int(n)
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    v = n * quantum
    if v >= Fraction(2) ** 128:
        return f32(sign * np.inf)
    return f32(sign * float(v))          # (exact: v has at most 24 significant bits)


def area_forms(v1, v2, v3):
    """The cull's signed area (render.rs:2393) of three f32 screen points, restated exactly: the uncontracted f32 chain, the exact rational
    value of the same differences, and the chain with one product fused into the subtraction, in either of the two ways a compiler may
    contract  a * b - c * d:  fma(a, b, -(c * d))  and  fma(-c, d, a * b)."""
    x1, y1, x2, y2, x3, y3 = (Fraction(float(t)) for t in (v1[0], v1[1], v2[0], v2[1], v3[0], v3[1]))
    a, b, c, d = (Fraction(float(rne32(t))) for t in (x2 - x1, y3 - y1, x3 - x1, y2 - y1))
    p, q = Fraction(float(rne32(a * b))), Fraction(float(rne32(c * d)))
    return {"chain": float(rne32(p - q)), "exact": a * b - c * d, "fma_a": float(rne32(a * b - q)), "fma_b": float(rne32(p - c * d))}


def key_of(t):
    """(v1.z + v2.z) + v3.z over 3.0f in f32 (render.rs:2529-2531)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(f32(f32(f32(t[0]) + f32(t[1])) + f32(t[2])) / f32(3.0))


# ------------------------------------------------------------------------------------------------ placement and projection
def camera_space(proj, tx, ty, cz, width=W, height=H):
    """camera-space x, y (float64) whose projection is the screen point (tx, ty) at camera depth cz"""
    tx, ty, cz = (np.asarray(t, np.float64) for t in (tx, ty, cz))
    if proj == "ortho":                                           # x = (cam.x - cx) * zoom + W / 2, y = -(cam.y - cy) * zoom + H / 2
        return (tx - width / 2.0) / ORTHO[0] + ORTHO[1], -(ty - height / 2.0) / ORTHO[0] + ORTHO[2]
    vs = min(width, height) / float(M.K("project.viewport_div")) * float(M.K("project.viewport_frac"))
    us = float(M.K("project.distance")) - float(M.K("project.us_sub"))
    half = 0.5 if proj == "fixed" else 0.0                        # fixed point floors: aim at the pixel's middle
    s = (cz + DIST) / (us * vs)
    return (tx + half - width / 2.0) * s, (ty + half - height / 2.0) * s


def place(proj, camera, tx, ty, cz, width=W, height=H):
    """f32 world positions [n, 3] that land on the screen points (tx, ty) at camera depth cz"""
    cz = np.asarray(cz, np.float32)
    finite = np.where(np.isfinite(cz), cz, 0.0)      # (Fixed32::from_f32 of a NaN is 0: that is where fixed point projects it from)
    cx, cy = camera_space(proj, tx, ty, finite, width, height)
    if camera.basis_z == (0.0, 0.0, 1.0) and camera.position == (0.0, 0.0, 0.0):
        return np.stack([cx.astype(np.float32), cy.astype(np.float32), cz], axis=1)       # (keeps -0.0 and NaN as they are)
    P, bx, by, bz = (np.asarray(np.asarray(t, np.float32), np.float64) for t in (camera.position, camera.basis_x, camera.basis_y, camera.basis_z))
    w = P[None, :] + cx[:, None] * bx[None, :] + cy[:, None] * by[None, :] + finite.astype(np.float64)[:, None] * bz[None, :]
    return w.astype(np.float32)


def project(pos, camera, proj, width=W, height=H):
    """(screen [n, 3] f32, camera depth [n] f32) of world positions, in the arithmetic of np_model.render_mesh_15 (math.rs:103-148,
    fixed.rs:424-441, render.rs:2323-2345)"""
    pos = np.asarray(pos, np.float32)
    cpos = np.asarray(camera.position, np.float32)
    B = [np.asarray(b, np.float32) for b in (camera.basis_x, camera.basis_y, camera.basis_z)]
    with np.errstate(all="ignore"):
        rel = (pos - cpos).astype(np.float32)
        cam = np.stack([M.dot3(rel, b) for b in B], axis=1).astype(np.float32)
        if proj == "ortho":
            zoom, ocx, ocy = (f32(t) for t in ORTHO)
            x = ((cam[:, 0] - ocx).astype(np.float32) * zoom).astype(np.float32) + f32(width) / f32(2.0)
            y = ((-(cam[:, 1] - ocy)).astype(np.float32) * zoom).astype(np.float32) + f32(height) / f32(2.0)
            scr = np.stack([x, y, cam[:, 2]], axis=1).astype(np.float32)
        elif proj == "fixed":
            sx, sy = M.project_fixed(pos, camera, width, height)
            scr = np.stack([sx.astype(np.float32), sy.astype(np.float32), cam[:, 2] + M.K("mesh.distance")], axis=1).astype(np.float32)
        else:
            vs = f32(f32(min(width, height)) / M.K("project.viewport_div")) * M.K("project.viewport_frac")
            denom = cam[:, 2] + M.K("project.distance")
            us = f32(M.K("project.distance") - M.K("project.us_sub"))
            x = (cam[:, 0] * us) / denom * vs + f32(width) / f32(2.0)
            y = (cam[:, 1] * us) / denom * vs + f32(height) / f32(2.0)
            tiny = np.abs(denom) < M.K("project.denom_guard")
            scr = np.stack([np.where(tiny, f32(width) / f32(2.0), x), np.where(tiny, f32(height) / f32(2.0), y),
                            np.where(tiny, cam[:, 2], denom)], axis=1).astype(np.float32)
    return scr, cam[:, 2].copy()


def snap_camz(pos, camera, want):
    """Moves each position by a few ulps per coordinate until dot3(pos - camera.position, basis_z) has exactly the bits of want[i]
    (None: leave it), where that is possible.  Deterministic: the candidates are the lattice of offsets -R .. R ulps, nearest first."""
    cpos, bz = np.asarray(camera.position, np.float32), np.asarray(camera.basis_z, np.float32)
    out = np.array(pos, np.float32, copy=True)
    for i, wv in enumerate(want):
        if wv is None:
            continue
        sp = np.spacing(np.abs(out[i])).astype(np.float32)
        for R in (4, 10, 20):
            g = np.arange(-R, R + 1)
            offs = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
            offs = offs[np.argsort(np.abs(offs).sum(axis=1), kind="stable")]
            cand = (out[i][None, :] + offs.astype(np.float32) * sp[None, :]).astype(np.float32)
            cz = M.dot3((cand - cpos).astype(np.float32), bz).astype(np.float32)
            hit = np.nonzero(cz.view(np.uint32) == np.uint32(bits(wv)))[0]
            if len(hit):
                out[i] = cand[hit[0]]
                break
    return out                      # (where no candidate fits the position stays: the census counts what was reached)


# ------------------------------------------------------------------------------------------------ sheets
@dataclass
class Face:
    tri: tuple                      # three cell-local screen targets (x, y)
    z: tuple                        # three camera depths
    tag: str = ""
    blend: int = abi.OPAQUE
    alpha: int = 255
    world: object = None            # callable (x0, y0) -> [3, 3] f32 world positions of a searched face, instead of tri / z
    gradient: bool = False          # three different vertex colours: the back-face swap of the attributes shows
    textured: bool = False          # the identity-address texture, one corner of it per vertex: the swap of the UVs shows


def face_colour(i):
    """r, g, b = 4 q + 2 over the 5-bit digits q of i + 1 (coverage_sheets._vertex_colour): unique per face after RGB555 quantisation"""
    code = i + 1
    assert 0 < code < 32768
    return [4 * ((code >> s) & 31) + 2 for s in (0, 5, 10)]


def identity_texture():
    """8 x 8 texels, each holding its own address in the low bits of red and green (never black, no STP bit)"""
    y, x = np.mgrid[0:8, 0:8]
    return Texture15(8, 8, ((x + 8) | ((y + 8) << 5) | (20 << 10)).astype(np.uint16), abi.OPAQUE, "identity")


@dataclass
class Sheet:
    name: str
    family: str
    proj: str
    width: int
    height: int
    cell: int
    camera: Camera
    cull: bool
    vertices: np.ndarray
    faces: np.ndarray
    meta: list                      # Face per face, in face order
    cell_of: np.ndarray             # [n] cell of every face
    cell_tag: list                  # tag per cell
    cell_xy: np.ndarray             # [m, 2] origin of every cell
    textures: list = field(default_factory=list)
    _oracle: dict = field(default_factory=dict)
    _proj: tuple = None

    @property
    def n(self):
        return len(self.faces)

    def cell_faces(self, c):
        return [int(i) for i in np.nonzero(self.cell_of == c)[0]]

    def settings(self, zbuffer=False, fmt8=False, cull=None, xray=False):
        st = RasterSettings.benchmark()
        st.dithering = False
        st.backface_cull = self.cull if cull is None else cull
        st.use_zbuffer = zbuffer
        st.use_rgb555 = not fmt8
        st.xray_mode = xray
        st.use_fixed_point = self.proj == "fixed"
        st.ortho_projection = ORTHO if self.proj == "ortho" else None
        return st

    def projected(self):
        """(screen [nv, 3], camera depth [nv]) by `project`; computed once"""
        if self._proj is None:
            self._proj = project(self.vertices["pos"], self.camera, self.proj, self.width, self.height)
        return self._proj

    def oracle(self, O, fog_name=None, **mode):
        """dict(rc, px [H, W, 4], zb bits, tm, dump) of the reference restatement; computed once per mode, shared and read-only"""
        key = (fog_name,) + tuple(sorted(mode.items()))
        if key not in self._oracle:
            fb = O.Framebuffer(self.width, self.height)
            fb.clear(CLEAR)
            st = self.settings(**mode)
            with np.errstate(all="ignore"):
                if mode.get("fmt8"):
                    rc, tm, d = O.render_mesh(fb, self.vertices, self.faces, self.textures8(), self.camera, st, dump=True)
                else:
                    rc, tm, d = O.render_mesh_15(fb, self.vertices, self.faces, self.textures, self.camera, st, fog(fog_name) if fog_name else None, dump=True)
            px = fb.image().copy(); px.setflags(write=False)
            zb = fb.zbuffer.view(np.uint32).copy(); zb.setflags(write=False)
            self._oracle[key] = dict(rc=rc, px=px, zb=zb, tm=tm, dump=d)
        return self._oracle[key]

    def textures8(self):
        return [Texture.from_texture15(t) for t in self.textures]

    def decode(self, image):
        """[H, W] face index painted at every pixel of an RGB555-path frame, -1 where the clear colour is left (flat opaque faces only)"""
        img = np.asarray(image).reshape(self.height, self.width, 4).astype(np.int64)
        code = (img[..., 0] >> 3) | ((img[..., 1] >> 3) << 5) | ((img[..., 2] >> 3) << 10)
        clear = (img[..., 0] == CLEAR.r) & (img[..., 1] == CLEAR.g) & (img[..., 2] == CLEAR.b)
        return np.where(clear, -1, code - 1)

    def window(self, c):
        x0, y0 = (int(v) for v in self.cell_xy[c])
        return x0, y0, x0 + self.cell, y0 + self.cell

    def describe_cell(self, c):
        who = self.cell_faces(c)
        return f"cell {c} '{self.cell_tag[c]}' at {tuple(int(v) for v in self.cell_xy[c])}, faces " + ", ".join(
            f"{i} '{self.meta[i].tag}' z={tuple(float(z) for z in self.meta[i].z)}" for i in who[:4])

    def first_difference(self, got, want, what):
        """'' when the frames are equal, else a message naming the draw, the first offending cell and its faces"""
        g = np.asarray(got).reshape(self.height, self.width, -1)
        w = np.asarray(want).reshape(self.height, self.width, -1)
        bad = (g != w).any(axis=2)
        if not bad.any():
            return ""
        y, x = [int(v[0]) for v in np.nonzero(bad)]
        per_row = self.width // self.cell
        c = (y // self.cell) * per_row + x // self.cell
        where = self.describe_cell(c) if c < len(self.cell_tag) else "outside every cell"
        cells = len({(int(b) // self.cell) * per_row + int(a) // self.cell for b, a in zip(*np.nonzero(bad))})
        return f"[{self.name} {what}] {int(bad.sum())} pixels in {cells} cells differ, first at ({x}, {y}): got {g[y, x].tolist()}, oracle {w[y, x].tolist()}; {where}"


def _stride(n):
    s = max(1, int(n * 0.381966))
    while np.gcd(s, n) != 1:
        s += 1
    return s


def make_sheet(name, family, proj, cells, cell=8, camera=None, cull=True, snap=False, recolour=None):
    """cells: [(tag, [Face, ...])].  The cells are laid out in a scattered but fixed order (so kept and rejected faces interleave
    irregularly across the waves and blocks of k_setup), row by row; recolour: a permutation of the face colours (family D's second draw)."""
    camera = camera or Camera()
    n = len(cells)
    per_row = W // cell
    assert n <= per_row * (H // cell), (name, n)
    s = _stride(n)
    cells = [cells[(i * s) % n] for i in range(n)]
    height = max(64, -(-n // per_row) * cell)
    meta, cell_of, cell_tag, cell_xy, pos, snap_want = [], [], [], [], [], []
    for c, (tag, fcs) in enumerate(cells):
        x0, y0 = (c % per_row) * cell, (c // per_row) * cell
        cell_tag.append(tag); cell_xy.append((x0, y0))
        for fc in fcs:
            meta.append(fc); cell_of.append(c)
            if fc.world is not None:
                pos.append(np.asarray(fc.world(x0, y0, height), np.float32).reshape(3, 3))
                snap_want += [None] * 3
            else:
                t = np.asarray(fc.tri, np.float64)
                pos.append(place(proj, camera, t[:, 0] + x0, t[:, 1] + y0, np.asarray(fc.z, np.float32), W, height))
                snap_want += [z if snap and any(bits(z) == bits(v) for v in (NEAR, up(NEAR), down(NEAR))) else None for z in fc.z]
    pos = np.concatenate(pos).astype(np.float32)
    if snap:
        pos = snap_camz(pos, camera, snap_want)
    nf = len(meta)
    assert nf > 256, (name, nf)
    v = make_vertices(3 * nf)
    v["pos"] = pos
    v["normal"] = (0.0, 0.0, -1.0)
    col = np.repeat(np.array([face_colour(i) for i in range(nf)], np.uint8), 3, axis=0)
    if recolour is not None:
        col = np.repeat(np.array([face_colour(int(recolour[i])) for i in range(nf)], np.uint8), 3, axis=0)
    for i, fc in enumerate(meta):
        if fc.gradient:
            col[3 * i:3 * i + 3] = ((250, 10, 10), (10, 250, 10), (10, 10, 250))
    v["blend"] = abi.OPAQUE
    f = make_faces(nf)
    f["v"] = np.arange(3 * nf, dtype=np.uint32).reshape(nf, 3)
    f["blend_mode"] = [fc.blend for fc in meta]
    f["editor_alpha"] = [fc.alpha for fc in meta]
    for i, fc in enumerate(meta):
        if fc.textured:
            f["texture_id"][i] = 0
            v["uv"][3 * i:3 * i + 3] = ((0.0625, 0.0625), (0.9375, 0.0625), (0.0625, 0.9375))
            col[3 * i:3 * i + 3] = 128
    v["r"], v["g"], v["b"] = col[:, 0], col[:, 1], col[:, 2]
    v.setflags(write=False); f.setflags(write=False)
    textures = [identity_texture()] if any(fc.textured for fc in meta) else []
    return Sheet(name, family, proj, W, height, cell, camera, cull, v, f, meta, np.asarray(cell_of), cell_tag, np.asarray(cell_xy), textures)


# ------------------------------------------------------------------------------------------------ family N
N_VALUES = {"near": NEAR, "near+": up(NEAR), "near-": down(NEAR), "zero": f32(0.0), "-zero": f32(-0.0), "-near": -NEAR}
N_COMFORTABLE = (1.0, 3.0, 7.5, 0.5, 40.0, 2.25, 0.125)


def family_n(proj, rotated=False):
    cells = []
    for k, comfy in enumerate(N_COMFORTABLE * (2 if rotated else 1)):
        shape = SHAPES[k % 3]
        for slots in SLOTS:
            for vn, val in N_VALUES.items():
                z = [f32(comfy)] * 3
                for s in slots:
                    z[s] = val
                cells.append((f"N {vn} on {slots}", [Face(shape, tuple(z), f"{vn}{slots}")]))
        cells.append(("N comfortable", [Face(shape, (f32(comfy),) * 3, "comfortable")]))
    return make_sheet(("Nrot-" if rotated else "N-") + proj, "N", proj, cells, camera=rotated_camera() if rotated else None,
                      snap=rotated and proj != "ortho")      # (orthographic projection ignores the plane, and its wide x and y leave no exact 0.1f)


# ------------------------------------------------------------------------------------------------ family F
F_CENTRES = (12.0, 0.0, -1.0)


def family_f(proj):
    cells = []
    for k in range(2):
        for C in F_CENTRES:
            vals = {"at": f32(C), "above": up(C), "below": down(C)}
            if C == 0.0:
                vals["-zero"] = f32(-0.0)
            others = {"far": f32(C + 8.0 + k), "near": f32(C - (9.0 if C > 0 else 3.0) + 0.25 * k)}
            for slots in SLOTS:
                for vn, val in vals.items():
                    for on, o in others.items():
                        z = [o] * 3
                        for s in slots:
                            z[s] = val
                        cells.append((f"F {vn} {C} on {slots}, others {on}", [Face(SHAPES[(k + len(cells)) % 3], tuple(z), f"{C}:{vn}{slots}:{on}")]))
    return make_sheet("F-" + proj, "F", proj, cells)


# ------------------------------------------------------------------------------------------------ family A
INT_CASES = {
    "collinear": ((1, 1), (3, 3), (5, 5)), "collinear-reversed": ((5, 5), (3, 3), (1, 1)), "collinear-flat": ((1, 1), (5, 1), (3, 1)),
    "coincident-12": ((1, 1), (1, 1), (5, 5)), "coincident-23": ((1, 1), (5, 5), (5, 5)), "coincident-13": ((1, 1), (5, 5), (1, 1)),
    "coincident-123": ((2, 2), (2, 2), (2, 2)),
    "area+1": ((2, 2), (3, 2), (2, 3)), "area-1": ((2, 2), (2, 3), (3, 2)),
    "area+1-rotated": ((3, 2), (2, 3), (2, 2)), "area-1-rotated": ((2, 3), (3, 2), (2, 2)),
    "front": SHAPES[2], "back": (SHAPES[2][0], SHAPES[2][2], SHAPES[2][1]),
}
# (No "wrong sign" class.  Rounding is monotonic, so a * b < c * d gives rn(a * b) <= rn(c * d): the chain of PRODUCTS can lose the sign
#  of the exact area only by becoming 0, which is class "zero".  The DIFFERENCES in front of it are exact here, and only here: every float
#  and orthographic screen coordinate r is the result of a final `t + W / 2` or `t + H / 2` with an integer half size of at least 32, so r
#  is a multiple of ulp(t) and of its own ulp; either |r| >= 8, whose ulp is at least 2^-20, or |t| >= 24, whose ulp is at least 2^-19.
#  All coordinates are multiples of 2^-20, and a difference below 8 -- a cell -- of such values has at most 23 bits.  Raw f32 points near
#  the frame's origin, which no projection produces, do give areas of the opposite sign.)
SEARCHED = ("zero", "fma_a", "fma_b", "tiny", "tiny_back")
A_DEPTH = 3.0


def _area_1500(s):
    """the fill's own area (render.rs:1500) of [n, 3, 2] f32 screen points, as an f32 chain"""
    return ((s[:, 1, 1] - s[:, 2, 1]) * (s[:, 0, 0] - s[:, 2, 0]) + (s[:, 2, 0] - s[:, 1, 0]) * (s[:, 0, 1] - s[:, 2, 1])).astype(np.float32)


def searched_face(proj, kind, seed):
    """A near-collinear triple in the cell whose signed area realises `kind`: found among seeded random candidates by float64 arithmetic
    (products of two f32 values are exact there), confirmed with exact rationals."""
    def world(x0, y0, height):
        rng = np.random.default_rng(1000003 * seed + 131 * x0 + y0)
        for _ in range(200):
            n = 8192
            p1, p3 = rng.uniform(1.0, 6.5, (n, 2)), rng.uniform(1.0, 6.5, (n, 2))
            p2 = p1 + rng.uniform(0.2, 0.8, (n, 1)) * (p3 - p1)
            t = np.stack([p1, p2, p3], axis=1) + (x0, y0)
            w = place(proj, Camera(), t[..., 0].reshape(-1), t[..., 1].reshape(-1), np.full(3 * n, A_DEPTH, np.float32), W, height)
            scr = project(w, Camera(), proj, W, height)[0].reshape(n, 3, 3)[..., :2]
            inside = ((scr >= (x0, y0)) & (scr < (x0 + 7.5, y0 + 7.5))).all(axis=(1, 2))
            a = (scr[:, 1, 0] - scr[:, 0, 0]).astype(np.float64); b = (scr[:, 2, 1] - scr[:, 0, 1]).astype(np.float64)
            c = (scr[:, 2, 0] - scr[:, 0, 0]).astype(np.float64); d = (scr[:, 1, 1] - scr[:, 0, 1]).astype(np.float64)
            p64, q64 = a * b, c * d
            p, q = p64.astype(np.float32), q64.astype(np.float32)
            chain = (p - q).astype(np.float32)
            exact = np.sign(p64 - q64)
            if kind == "zero":
                m = (chain == 0) & (exact != 0)
            elif kind == "fma_a":
                m = ((p64 - q.astype(np.float64)).astype(np.float32) <= 0) != (chain <= 0)
            elif kind == "fma_b":
                m = ((p.astype(np.float64) - q64).astype(np.float32) <= 0) != (chain <= 0)
            else:
                ar = _area_1500(scr)
                m = (np.abs(ar) > 0) & (np.abs(ar) < AREA_EPS) & ((chain > 0) if kind == "tiny" else (chain < 0))
            for i in np.nonzero(m & inside)[0][:8]:
                fm = area_forms(*scr[i])
                ok = {"zero": fm["chain"] == 0 and fm["exact"] != 0,
                      "fma_a": (fm["fma_a"] <= 0) != (fm["chain"] <= 0), "fma_b": (fm["fma_b"] <= 0) != (fm["chain"] <= 0),
                      "tiny": fm["chain"] > 0, "tiny_back": fm["chain"] < 0}[kind]
                if ok:
                    return w.reshape(n, 3, 3)[i]
        raise AssertionError(f"no '{kind}' triple found in the cell at ({x0}, {y0}); widen the candidate set")
    return world


def _shifted(tri, dx, dy):
    """the triangle moved by dx and by dy, each where it still fits the cell"""
    dx = dx if max(p[0] for p in tri) + dx <= 7 else 0
    dy = dy if max(p[1] for p in tri) + dy <= 7 else 0
    return tuple((x + dx, y + dy) for x, y in tri)


def family_a(proj):
    cells = []
    z = (f32(A_DEPTH),) * 3
    for dx in range(4):
        for dy in range(3):
            for name, tri in INT_CASES.items():
                cells.append((f"A {name}", [Face(_shifted(tri, dx, dy), z, name)]))
    for k in range(8):
        cells.append(("A gradient front", [Face(SHAPES[k % 3], z, "gradient-front", gradient=True)]))
        s = SHAPES[k % 3]
        cells.append(("A gradient back", [Face((s[0], s[2], s[1]), z, "gradient-back", gradient=True)]))
        if k < 4:
            cells.append(("A textured front", [Face(s, z, "textured-front", textured=True)]))
            cells.append(("A textured back", [Face((s[0], s[2], s[1]), z, "textured-back", textured=True)]))
    if proj != "fixed":
        for k in range(16):
            for kind in SEARCHED:
                cells.append((f"A searched {kind}", [Face(None, z, kind, world=searched_face(proj, kind, k))]))
            cells.append(("A sub-pixel", [Face(((3.2 + 0.02 * k, 3.2), (3.7, 3.2 + 0.02 * k), (3.2, 3.7)), z, "subpixel")]))
    else:
        for k in range(10):                    # (integer screen coordinates: no rounding to search; more of the decisive integer cases)
            for name in ("collinear", "coincident-123", "area+1", "area-1", "coincident-12", "back", "front", "area-1-rotated", "collinear-reversed"):
                tri = INT_CASES[name]
                cells.append((f"A {name}", [Face(tuple((x + (k % 2), y + (k // 2) % 2) for x, y in tri), (f32(A_DEPTH + k),) * 3, name)]))
    return make_sheet("A-" + proj, "A", proj, cells)


# ------------------------------------------------------------------------------------------------ family K
@dataclass
class KCase:
    tag: str
    faces: list                     # (kind, depth triple): kind o opaque front, b opaque back face, v blend Average, a editor_alpha 128
    alt: str                        # the nearest alternative rule that must change the cell (a `mut` of the test module's decide)
    camz: bool = False              # the triples are camera depths as they are (else screen depths: perspective subtracts 5.0)


def key_mul(t):
    """the key with * (1.0f / 3.0f) in place of / 3.0f"""
    return f32(f32(f32(f32(t[0]) + f32(t[1])) + f32(t[2])) * f32(f32(1.0) / f32(3.0)))


def _flat(k):
    """m with key_of((m, m, m)) bit-equal to k, or None"""
    for m in (f32(k), up(k), down(k)):
        if bits(key_of((m, m, m))) == bits(k):
            return (m, m, m)
    return None


def k_numbers(seed):
    """searched depth triples in [8, 16) (where subtracting and adding 5.0 is exact): see the cases of k_cases"""
    rng = np.random.default_rng(seed)
    out = {}

    def rnd():
        return tuple(f32(x) for x in rng.uniform(8.0, 16.0, 3).astype(np.float32))
    while "ulp" not in out:                    # keys one ulp apart, the lower one even (so that dropping the last bit makes a tie)
        A = rnd(); kA = key_of(A); B = A
        if bits(kA) & 1:
            continue
        for _ in range(8):
            B = (B[0], B[1], up(B[2]))
            if key_of(B) != kA:
                break
        if bits(key_of(B)) - bits(kA) == 1:
            out["ulp"] = (A, B)
    while "tie_diff" not in out:               # equal keys from different triples
        A = rnd(); B = (up(up(A[0])), A[1], down(down(A[2])))
        if bits(key_of(A)) == bits(key_of(B)):
            out["tie_diff"] = (A, B)
    while "assoc" not in out:                  # (a + b) + c != (a + c) + b, and a flat neighbour on either key
        A = rnd(); k1, k2 = key_of(A), key_of((A[0], A[2], A[1]))
        if k1 != k2 and _flat(k1) and _flat(k2):
            out["assoc"] = (A, _flat(k1), _flat(k2))
    while "div3" not in out:                   # s / 3.0f != s * (1.0f / 3.0f)
        A = rnd()
        Y = _flat(key_of(A))
        if Y and key_mul(A) != key_mul(Y):     # equal keys by the rule, different ones by the alternative
            out["div3"] = (A, Y)
    return out


def k_cases(proj, seed):
    n = k_numbers(seed)
    A, B = n["ulp"]; TA, TB = n["tie_diff"]; X, Y1, Y2 = n["assoc"]; D3, D3Y = n["div3"]
    e = f32(9.0 + 0.25 * seed)
    c = [KCase("keys one ulp apart", [("o", A), ("o", B)], "drop_lsb"),
         KCase("equal keys, equal triples", [("o", (e, e, e)), ("o", (e, e, e))], "painter_tie_earlier"),
         KCase("equal keys, different triples", [("o", TA), ("o", TB)], "painter_tie_earlier"),
         KCase("three equal keys", [("o", TA), ("o", TB), ("o", TA)], "painter_tie_earlier"),
         KCase("non-associative sum, front face", [("o", X), ("o", Y1)], "assoc_other"),
         KCase("non-associative sum, back face", [("b", X), ("o", Y2)], "sum_before_swap"),
         KCase("/ 3.0f against * (1 / 3)", [("o", D3), ("o", D3Y)], "mul_third"),
         KCase("transparent (Average) over a nearer opaque", [("v", (e + 3, e + 3, e + 3)), ("o", (e, e, e))], "one_list"),
         KCase("transparent (alpha) over a nearer opaque", [("a", (e + 3, e + 3, e + 3)), ("o", (e, e, e))], "one_list"),
         KCase("transparent (Average) over a farther opaque", [("v", (e, e, e)), ("o", (e + 3, e + 3, e + 3))], "transparent_first"),
         KCase("transparent (alpha) over a farther opaque", [("a", (e, e, e)), ("o", (e + 3, e + 3, e + 3))], "transparent_first"),
         KCase("two transparent by key over an opaque between", [("a", (e, e, e)), ("a", (e + 2, e + 2, e + 2)), ("o", (e + 1, e + 1, e + 1))], "ascending"),
         KCase("two transparent with equal keys", [("a", TA), ("v", TB), ("o", (e, e, e))], "painter_tie_earlier"),
         KCase("four faces, two classes", [("a", (e, e, e)), ("o", (e + 1, e + 1, e + 1)), ("v", (e + 2, e + 2, e + 2)), ("o", (e, e + 1, e + 2))], "one_list")]
    if proj != "ortho":
        s = f32(0.2 + 0.05 * seed)
        while key_of((s, s, s)) == key_of((up(s),) * 3):         # (distinct keys without the + 5.0, equal ones with it)
            s = up(s)
        c += [KCase("camera depths equal after + 5.0", [("o", (s, s, s)), ("o", (up(s), up(s), up(s)))], "no_plus5", camz=True),
              KCase("large depths", [("o", (f32(900.0), f32(1.0), f32(1.0))), ("o", (f32(250.0), f32(250.0), f32(250.0)))], "ascending", camz=True)]
        if proj == "float":                    # as far out as x = cam.x * 4 / denom * vs stays finite for every cell of the frame (fixed point ends at 2^19)
            c += [KCase("depth 1e37 against 3e36", [("o", (f32(1e37), f32(1.0), f32(1.0))), ("o", (f32(3e36),) * 3)], "ascending", camz=True)]
    else:
        big, dn = f32(3e38), f32(4.2e-45 * (seed + 1))
        c += [KCase("sums overflow to +inf: a tie", [("o", (big, big, big)), ("o", (big, big, f32(1.0)))], "painter_tie_earlier"),
              KCase("+inf key against 1e38", [("o", (big, big, big)), ("o", (big, f32(1.0), f32(1.0)))], "ascending"),
              KCase("depth 3e38 against 9e37", [("o", (big, f32(1.0), f32(1.0))), ("o", (f32(9e37),) * 3)], "ascending"),
              KCase("negative keys", [("o", (-e, -e, -e)), ("o", (-e - 1, -e - 1, -e - 1))], "abs_key"),
              KCase("negative keys one ulp apart", [("o", tuple(-t for t in A)), ("o", tuple(-t for t in B))], "abs_key"),
              KCase("negative against positive", [("o", (-e, -e, -e)), ("o", (e / 2, e / 2, e / 2))], "abs_key"),
              KCase("-0.0 against +0.0: a tie", [("o", (f32(-0.0),) * 3), ("o", (f32(0.0),) * 3)], "neg_zero_less"),
              KCase("denormal against zero", [("o", (dn, dn, dn)), ("o", (f32(0.0),) * 3)], "flush_denormals"),
              KCase("negative denormal against -0.0", [("o", (-dn, -dn, -dn)), ("o", (f32(-0.0),) * 3)], "flush_denormals"),
              KCase("-inf key against -1e38", [("o", (-big, -big, -big)), ("o", (-big, f32(-1.0), f32(-1.0)))], "abs_key"),
              KCase("transparent negative keys", [("a", (-e, -e, -e)), ("a", (-e - 2, -e - 2, -e - 2)), ("o", (f32(0.0),) * 3)], "abs_key"),
              KCase("transparent -0.0 against +0.0", [("a", (f32(-0.0),) * 3), ("v", (f32(0.0),) * 3)], "neg_zero_less"),
              KCase("transparent +inf ties", [("a", (big, big, big)), ("a", (big, big, f32(2.0))), ("o", (big, big, big))], "painter_tie_earlier")]
    return c


def family_k(proj):
    cells = []
    for seed in range(4):
        for case in k_cases(proj, seed):
            for rev in (False, True):
                fcs = []
                for kind, t in (case.faces[::-1] if rev else case.faces):
                    t = tuple(f32(x) for x in t)
                    z = t if (proj == "ortho" or case.camz) else tuple(f32(x - f32(DIST)) for x in t)
                    tri = (SHAPES[0][0], SHAPES[0][2], SHAPES[0][1]) if kind == "b" else SHAPES[0]
                    fcs.append(Face(tri, z, kind, blend=abi.AVERAGE if kind == "v" else abi.OPAQUE, alpha=128 if kind == "a" else 255))
                if proj != "ortho" and len(cells) % 3 == 1:          # a near-rejected face among them (perspective only: nothing rejects here otherwise)
                    fcs.insert(len(cells) % 2, Face(SHAPES[0], (f32(0.05), f32(3.0), f32(3.0)), "rejected"))
                cells.append((f"K {case.tag}|{case.alt}|{'reversed' if rev else 'forward'}", fcs))
    return make_sheet("K-" + proj, "K", proj, cells, cull=False)


# ------------------------------------------------------------------------------------------------ family D
def d_pairs(proj, k):
    a = f32(8.0 + 0.37 * k); b = f32(a * f32(1.5))
    u = a                                       # the fill interpolates 1 / z: neighbours whose reciprocals round to one f32 would tie at every pixel
    while f32(1.0) / u == f32(1.0) / up(u):
        u = up(u)
    p = [("far apart", (a, b, b), (b, a, a)), ("one ulp apart", (u, up(u), up(u)), (up(u), u, u)),
         ("equal along an edge", (a, a, b), (a, a, f32(a + 1))), ("all tie", (a, b, b), (a, b, b))]
    if proj == "ortho":
        p += [("negative depths", (-a, -b, -b), (-b, -a, -a)), ("negative, one ulp apart", (-u, -up(u), -up(u)), (-up(u), -u, -u))]
    return p


def family_d(proj, second=False):
    cells = []
    for k in range(17 if proj != "ortho" else 12):
        for tag, t1, t2 in d_pairs(proj, k):
            for rev in (False, True):
                ts = (t2, t1) if rev else (t1, t2)
                fcs = [Face(SHAPE_D, t if proj == "ortho" else tuple(f32(x - f32(DIST)) for x in t), tag) for t in ts]
                cells.append((f"D {tag}|{'reversed' if rev else 'forward'}", fcs))
    n = sum(len(c[1]) for c in cells)
    recolour = None
    if second:                                  # the two faces of every cell swap their colours
        recolour = np.arange(n) ^ 1
    return make_sheet("D-" + proj + ("-second" if second else ""), "D", proj, cells, cell=16, cull=False, recolour=recolour)


# ------------------------------------------------------------------------------------------------ the sheets by name
FAMILIES = {"N": family_n, "Nrot": lambda p: family_n(p, rotated=True), "A": family_a, "F": family_f, "K": family_k, "D": family_d}
NAMES = [f"{fam}-{p}" for fam in FAMILIES for p in PROJS]


@functools.lru_cache(maxsize=None)
def sheet(name):
    """the sheet of that name ("K-ortho", "D-fixed-second", ...), built once per process"""
    fam, proj = name.split("-")[:2]
    if name.endswith("-second"):
        return family_d(proj, second=True)
    return FAMILIES[fam](proj)


def modes(sh):
    """the draws a sheet is compared in: [(label, fog name, settings keywords)]"""
    out = [("painter", None, {}), ("zbuffer", None, {"zbuffer": True})]
    if sh.family == "A":
        out += [("cull off", None, {"cull": False}), ("cull off zbuffer", None, {"cull": False, "zbuffer": True}), ("xray", None, {"xray": True})]
    if sh.family == "F":
        out = [(f"fog {n}", n, {}) for n in FOG_DISTANCES] + [("fog normal zbuffer", "normal", {"zbuffer": True})]
    if sh.family == "D":
        out = [("zbuffer", None, {"zbuffer": True})]
    return out


# ------------------------------------------------------------------------------------------------ family V
V_COMPOSITIONS = ("alone", "opaque_partner", "transparent_partner", "nan_transparent_alone", "nan_transparent_pair", "near_rejected", "backface_culled")


@functools.lru_cache(maxsize=None)
def v_mesh(comp, nf, nan_first, proj):
    """(vertices, faces): one face with a NaN depth on its second vertex, its partner(s) at the other end of the mesh, rejected fillers
    between them (near-rejected in perspective, back faces under orthographic projection; the sheet is drawn with culling on).
    backface_culled exists in fixed point only: a NaN z projects to finite screen coordinates there (Fixed32::from_f32 of NaN is 0),
    in float and orthographic projection it makes the area NaN, which is front-facing."""
    W_, H_ = 64, 64
    front, back = SHAPES[0], (SHAPES[0][0], SHAPES[0][2], SHAPES[0][1])
    nan = f32(np.nan)
    filler = (back, (f32(3.0),) * 3, abi.OPAQUE, 255) if proj == "ortho" else (front, (f32(3.0), f32(0.05), f32(3.0)), abi.OPAQUE, 255)
    partner_o = (front, (f32(4.0),) * 3, abi.OPAQUE, 255)
    partner_t = (front, (f32(4.0),) * 3, abi.OPAQUE, 128)
    nan_o = (front, (f32(3.0), nan, f32(3.0)), abi.OPAQUE, 255)
    nan_t = (front, (f32(3.0), nan, f32(3.0)), abi.AVERAGE, 255)
    special, others = {"alone": (nan_o, []), "opaque_partner": (nan_o, [partner_o]), "transparent_partner": (nan_o, [partner_t]),
                       "nan_transparent_alone": (nan_t, [partner_o]), "nan_transparent_pair": (nan_t, [partner_t]),
                       "near_rejected": ((front, (f32(0.05), nan, f32(3.0)), abi.OPAQUE, 255), [partner_o, partner_o]),
                       "backface_culled": ((back, (f32(3.0), nan, f32(3.0)), abi.OPAQUE, 255), [partner_o, partner_o])}[comp]
    rows = [filler] * nf                        # (tri, z, blend, alpha) per face
    ends = list(range(nf - 1, -1, -1)) if nan_first else list(range(nf))
    rows[0 if nan_first else nf - 1] = special
    for j, o in enumerate(others[:nf - 1]):
        rows[ends[j]] = o
    pos = []
    for i, (tri, z, _, _) in enumerate(rows):
        t = np.asarray(tri, np.float64)
        x0, y0 = 8 * (i % 8), 8 * ((i // 8) % 8)
        pos.append(place(proj, Camera(), t[:, 0] + x0, t[:, 1] + y0, np.asarray(z, np.float32), W_, H_))
    v = make_vertices(3 * nf)
    v["pos"] = np.concatenate(pos)
    v["normal"] = (0.0, 0.0, -1.0)
    col = np.repeat(np.array([face_colour(i) for i in range(nf)], np.uint8), 3, axis=0)
    v["r"], v["g"], v["b"] = col[:, 0], col[:, 1], col[:, 2]
    f = make_faces(nf)
    f["v"] = np.arange(3 * nf, dtype=np.uint32).reshape(nf, 3)
    f["blend_mode"] = [r[2] for r in rows]
    f["editor_alpha"] = [r[3] for r in rows]
    v.setflags(write=False); f.setflags(write=False)
    return v, f


def v_settings(proj, zbuffer):
    st = RasterSettings.benchmark()
    st.dithering = False
    st.backface_cull = True
    st.use_zbuffer = zbuffer
    st.use_fixed_point = proj == "fixed"
    st.ortho_projection = ORTHO if proj == "ortho" else None
    return st


@functools.lru_cache(maxsize=None)
def v_oracle(O, comp, nf, nan_first, proj, zbuffer):
    """(rc, pixels, z-buffer bits, timings, dump) of the reference restatement for one V draw on a 64 x 64 frame"""
    v, f = v_mesh(comp, nf, nan_first, proj)
    fb = O.Framebuffer(64, 64)
    fb.clear(CLEAR)
    with np.errstate(all="ignore"):
        rc, tm, d = O.render_mesh_15(fb, v, f, [], Camera(), v_settings(proj, zbuffer), dump=True)
    px = fb.pixels.copy(); px.setflags(write=False)
    zb = fb.zbuffer.view(np.uint32).copy(); zb.setflags(write=False)
    return rc, px, zb, tm, d


# ------------------------------------------------------------------------------------------------ the device side
def gpu_draw(ctx, sh, resident=False, band=None, fog_name=None, fb=None, **mode):
    """One frame of the sheet through the C ABI -> (framebuffer object, timings); fb: draw onto this framebuffer as it is."""
    from bonnie32_amd import rasterizer as R
    st = sh.settings(**mode)
    fmt8 = bool(mode.get("fmt8"))
    if fb is None:
        fb = R.Framebuffer(sh.width, sh.height, ctx)
        fb.clear(CLEAR)
    if band:
        fb.set_band(*band)
    fg = fog(fog_name) if fog_name else None
    if resident:
        rs = R.ResidentScene(fb, sh.vertices, sh.faces, textures8=sh.textures8()) if fmt8 else R.ResidentScene(fb, sh.vertices, sh.faces, sh.textures)
        tm = rs.render(sh.camera, st) if fmt8 else rs.render(sh.camera, st, fg)
    elif fmt8:
        tm = R.render_mesh(fb, sh.vertices, sh.faces, sh.textures8(), sh.camera, st)
    else:
        tm = R.render_mesh_15(fb, sh.vertices, sh.faces, sh.textures, sh.camera, st, fg)
    return fb, tm


@functools.lru_cache(maxsize=None)
def placed_n(proj):
    """(local vertices, Placement) for sheet N: rotating the local vertices about Y and moving them (place_vertices: rz = x * s + z * c,
    three roundings) gives world positions close to the sheet's, and camera depths with exactly the bits of 0.1f and its two neighbours
    wherever the sheet has them.  The angle is small and the offset has no z part, for the reason given at rotated_camera."""
    from bonnie32_amd.rasterizer import Placement
    sh = sheet("N-" + proj)
    s = f32(0.01); c = f32(np.sqrt(1.0 - float(s) ** 2))
    pl = Placement(cos_f=c, sin_f=s, world_pos=(0.5, -0.25, 0.0))
    P = sh.vertices["pos"].astype(np.float64)
    x, y, z = P[:, 0] - 0.5, P[:, 1] + 0.25, P[:, 2]
    L = np.stack([x * float(c) + z * float(s), y, -x * float(s) + z * float(c)], axis=1).astype(np.float32)
    targets = {bits(v) for v in (NEAR, up(NEAR), down(NEAR))}
    g = np.arange(-12, 13)
    ox, oz = (t.reshape(-1) for t in np.meshgrid(g, g, indexing="ij"))
    near_first = np.argsort(np.abs(ox) + np.abs(oz), kind="stable")
    ox, oz = ox[near_first].astype(np.float32), oz[near_first].astype(np.float32)
    for i, zv in enumerate(sh.vertices["pos"][:, 2]):
        if bits(zv) not in targets:
            continue
        cx = (L[i, 0] + ox * np.spacing(np.abs(L[i, 0]))).astype(np.float32)
        cz = (L[i, 2] + oz * np.spacing(np.abs(L[i, 2]))).astype(np.float32)
        rz = ((cx * s).astype(np.float32) + (cz * c).astype(np.float32)).astype(np.float32) + f32(0.0)
        hit = np.nonzero(rz.view(np.uint32) == np.uint32(bits(zv)))[0]
        if len(hit):
            L[i, 0], L[i, 2] = cx[hit[0]], cz[hit[0]]
    local = np.array(sh.vertices, copy=True)
    local["pos"] = L
    local.setflags(write=False)
    return local, pl
