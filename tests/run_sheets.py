"""Run sheets: console frames (b32_frame_begin / _add_scene[_placed] / _end, b32_frame_submit[_placed]) made of tiny resident meshes in
which every face has a cell of its own, or shares one screen triangle with the faces it is compared against, so that every decision that
is specific to MERGED runs -- which row of the MeshTable / PlaceTable a face reads, the member's own bound of texture ids and vertex indices,
the texel-pool base of a member, who wins a depth tie between members, where a run ends, which merged mesh the cache hands out -- is a cell
of the frame (tests/test_run_sheets.py).

The frame is 256 x 192, RasterSettings.game() with flat shading under one directional light (z-buffer, RGB555, fixed point), one identity
camera.  The expectation is always the oracle's sequential calls: one render_mesh_15 per draw onto one framebuffer with that draw's
ambient, culling and fog; a placed draw's vertices are placed on the host with the library's place_vertices.

  R  rows: 2, 31, 32, 33, 64, 65 members (the 32-member split falls inside); per member an ambient, a culling flag (one back face), one of
     three fogs or none with a colour of its own (one deep face that two of the fogs cull), a placement on every third member.  8 x 8 cells:
     65 members of three faces do not fit the frame's 192 cells of 16 x 16
  T  bases: members whose vertex counts, texture counts and texel pools differ (pools of 15, 64, 0, 142, 128 and 79 texels: every base is
     odd and no multiple of 32); first / last texel of every pool skippable; texture ids nt - 1, nt, NO_TEXTURE, 0xFFFFFFFE.  An upload
     pads every texture to 8 texels (layout_textures), so on the device the pools are 16, 72, 0, 144, 136 and 80 texels and the bases 16,
     88, 88, 232 and 368: never odd, but no multiple of 32 either -- one word of the skip mask holds texels of two members
  Z  ties: bit-equal depth triples of two and three members on one screen triangle, the same slot twice, once placed by the identity,
     one ulp nearer, the earlier member's face 70 behind 69 rejected faces, a tie across a run boundary
  B  the blend member: [A, B, C] [D, E, F] [G] [I, U] [J, K]; C's transparent faces over A's, B's and its own opaque faces
  L  large from small: 32 members give runs of 8192 / 8193 faces (2048 / 2049 with a blend member last); a 2049-deep transparent stack
  S  sequences that break the run rule at one place, and the base settings that never merge
  C  cache: 12 slots of different sizes, 66 two-member runs that share one tie cell

Source faces carry _pad = 0xFF in every second face: the merge overwrites that byte, a draw on its own ignores it.

This module only builds and caches; what the tests compare is always the oracle's frame."""
import copy
import functools
from dataclasses import dataclass, field

import numpy as np

from bonnie32_amd import abi
from bonnie32_amd.rasterizer import Placement
from bonnie32_amd.rtypes import Camera, Color, Light, RasterSettings, Texture, Texture15, make_faces, make_vertices
from tests import frontend_sheets as FS

f32 = np.float32
W, H = FS.W, FS.H
CLEAR = FS.CLEAR
CAM = Camera()
FRONT16 = ((1, 1), (14, 1), (1, 14))
FRONT8 = ((1, 1), (6, 1), (1, 6))
TINY = ((0, 0), (1, 0), (0, 1))                       # family L: owns the pixel at its origin
BLEND_MODES = (("average", abi.AVERAGE, 255), ("add", abi.ADD, 255), ("subtract", abi.SUBTRACT, 255), ("add-quarter", abi.ADD_QUARTER, 255),
               ("alpha-128", abi.OPAQUE, 128))
IDENTITY_PLACEMENT = dict(cos_f=1.0, sin_f=0.0, world_pos=(0.0, 0.0, 0.0))      # x * 1 - z * 0 + 0: the same bits through the placed code


def back(shape):
    return (shape[0], shape[2], shape[1])


def base_settings(**kw):
    st = RasterSettings.game()
    st.shading = abi.SHADE_FLAT
    st.lights = [Light.directional((0.2, 0.3, 1.0), 0.25)]
    for k, v in kw.items():
        setattr(st, k, v)
    return st


# ------------------------------------------------------------------------------------------------ members
@dataclass
class Member:
    name: str
    vertices: np.ndarray            # local space
    faces: np.ndarray
    textures: list
    tags: list                      # tag per face
    cells: list                     # cell per face (-1: none)
    fmt8: bool = False              # uploaded through the 8-bit-colour path (never merged)

    @property
    def nf(self):
        return len(self.faces)

    @property
    def blends(self):
        """the host's bound (b32raster.h: "the first mesh that has a transparent pass"): a face or a texture that can blend"""
        return bool(len(self.faces) and ((self.faces["blend_mode"] != abi.OPAQUE) | (self.faces["editor_alpha"] < 255)).any()) or \
            any(t.blend_mode != abi.OPAQUE for t in self.textures)


class Grid:
    """hands out the cells of a frame row by row"""

    def __init__(self, cell):
        self.cell, self.per_row, self.n, self.tags = cell, W // cell, 0, []

    def take(self, tag):
        assert self.n < self.per_row * (H // self.cell), "the frame is full"
        self.tags.append(tag)
        self.n += 1
        return self.n - 1

    def origin(self, c):
        return (c % self.per_row) * self.cell, (c // self.per_row) * self.cell


class MeshBuilder:
    def __init__(self, name, grid, spare_vertices=0):
        self.name, self.grid = name, grid
        self.pos = [np.zeros((spare_vertices, 3), np.float32)] if spare_vertices else []
        self.nv = spare_vertices
        self.col, self.uv = [(128, 128, 128)] * spare_vertices, [(0.0, 0.0)] * spare_vertices
        self.rows, self.textures = [], []

    def tri(self, cell, shape, z, rgb, tag="", tex=abi.NO_TEXTURE, uv=None, bt=1, blend=abi.OPAQUE, alpha=255, origin=None):
        """one face with three vertices of its own on the cell's screen triangle `shape` at the camera depths z -> its face index"""
        x0, y0 = origin if origin is not None else self.grid.origin(cell)
        t = np.asarray(shape, np.float64)
        z = np.asarray(z if np.ndim(z) else (z,) * 3, np.float32)
        self.pos.append(FS.place("fixed", CAM, t[:, 0] + x0, t[:, 1] + y0, z, W, H))
        self.col += [tuple(rgb)] * 3
        self.uv += list(uv) if uv is not None else [(0.0, 0.0)] * 3
        self.rows.append(((self.nv, self.nv + 1, self.nv + 2), tex, bt, blend, alpha, tag, cell))
        self.nv += 3
        return len(self.rows) - 1

    def build(self, localise=None, fmt8=False):
        v = make_vertices(self.nv)
        if self.nv:
            v["pos"] = np.concatenate(self.pos).astype(np.float32)
            v["uv"] = np.asarray(self.uv, np.float32)
            c = np.asarray(self.col, np.uint8)
            v["r"], v["g"], v["b"] = c[:, 0], c[:, 1], c[:, 2]
        v["normal"] = (0.0, 0.0, -1.0)
        if localise is not None:
            v = localise(v)
        f = make_faces(len(self.rows))
        for i, (idx, tex, bt, blend, alpha, _tag, _cell) in enumerate(self.rows):
            f["v"][i] = idx; f["texture_id"][i] = tex; f["black_transparent"][i] = bt; f["blend_mode"][i] = blend; f["editor_alpha"][i] = alpha
        f["_pad"][1::2] = 0xFF
        v.setflags(write=False); f.setflags(write=False)
        return Member(self.name, v, f, list(self.textures), [r[5] for r in self.rows], [r[6] for r in self.rows], fmt8)


def local_for(pl):
    """vertices whose placement by pl (place_vertices: three roundings per coordinate) lands next to the given world vertices"""
    def fn(v):
        c, s = float(pl.cos_f), float(pl.sin_f)
        P = v["pos"].astype(np.float64) - np.asarray(pl.world_pos, np.float64)
        out = np.array(v, copy=True)
        out["pos"] = np.stack([P[:, 0] * c + P[:, 2] * s, P[:, 1], -P[:, 0] * s + P[:, 2] * c], axis=1).astype(np.float32)
        return out
    return fn


# ------------------------------------------------------------------------------------------------ frames
@dataclass
class Draw:
    member: int
    ambient: float = 0.5
    cull: bool = True
    fog: tuple = None
    placement: Placement = None


@dataclass
class Frame:
    name: str
    family: str
    members: list
    draws: list
    cell: int
    cell_tags: list
    base: RasterSettings = field(default_factory=base_settings)
    claims: list = field(default_factory=list)          # (kind, ...) rows for the census
    routes_off: int = 0                                  # ROUTE_* bits this frame is drawn with (family S: ROUTE_BATCH)
    _cache: dict = field(default_factory=dict)

    def origin(self, c):
        per_row = W // self.cell
        return (c % per_row) * self.cell, (c // per_row) * self.cell

    def window(self, c):
        x0, y0 = self.origin(c)
        return slice(y0, y0 + self.cell), slice(x0, x0 + self.cell)

    def settings_of(self, d):
        st = copy.copy(self.base)
        st.ambient, st.backface_cull = d.ambient, d.cull
        return st

    def world_vertices(self, d):
        m = self.members[d.member]
        return d.placement.apply(m.vertices) if d.placement is not None else m.vertices

    def calls(self):
        """the sequential calls: dict(v, f, tex, st, fog, fmt8, draw) per draw"""
        return [dict(v=self.world_vertices(d), f=self.members[d.member].faces, tex=self.members[d.member].textures, st=self.settings_of(d),
                     fog=d.fog, fmt8=self.members[d.member].fmt8, draw=i) for i, d in enumerate(self.draws)]

    def oracle(self, O):
        if "frame" not in self._cache:
            self._cache["frame"] = render_calls(O, self.calls())
        return self._cache["frame"]

    def solo(self, O, i):
        """draw i alone on a cleared frame"""
        if ("solo", i) not in self._cache:
            self._cache[("solo", i)] = render_calls(O, [self.calls()[i]])
        return self._cache[("solo", i)]

    def cell_at(self, x, y):
        c = (y // self.cell) * (W // self.cell) + x // self.cell
        return c, (self.cell_tags[c] if c < len(self.cell_tags) else "outside every cell")

    def first_difference(self, got, want, what):
        """'' when the frames are equal, else a message naming the first offending cell"""
        g = np.asarray(got).reshape(H, W, -1)
        w = np.asarray(want).reshape(H, W, -1)
        bad = (g != w).any(axis=2)
        if not bad.any():
            return ""
        ys, xs = np.nonzero(bad)
        cells = sorted({self.cell_at(int(x), int(y))[0] for x, y in zip(xs, ys)})
        c, tag = self.cell_at(int(xs[0]), int(ys[0]))
        return (f"[{self.name} {what}] {int(bad.sum())} pixels in {len(cells)} cells differ, first at ({int(xs[0])}, {int(ys[0])}): got "
                f"{g[ys[0], xs[0]].tolist()}, oracle {w[ys[0], xs[0]].tolist()}; cell {c} '{tag}'")

    def changed_cells(self, a, b):
        """the cells in which two results (dicts with px and zb) differ"""
        bad = (a["px"] != b["px"]).any(axis=2) | (a["zb"].reshape(H, W) != b["zb"].reshape(H, W))
        ys, xs = np.nonzero(bad)
        return sorted({self.cell_at(int(x), int(y)) for x, y in zip(xs, ys)})


def render_calls(O, calls, fb=None):
    """the calls, in order, onto one oracle framebuffer -> dict(px [H, W, 4], zb bits, rcs, drawn per call)"""
    keep = fb is not None
    if fb is None:
        fb = O.Framebuffer(W, H)
        fb.clear(CLEAR)
    rcs, drawn = [], []
    with np.errstate(all="ignore"):
        for c in calls:
            if c["fmt8"]:
                rc, tm = O.render_mesh(fb, c["v"], c["f"], [Texture.from_texture15(t) for t in c["tex"]], CAM, c["st"])
            else:
                rc, tm = O.render_mesh_15(fb, c["v"], c["f"], c["tex"], CAM, c["st"], c["fog"])
            rcs.append(rc); drawn.append(tm.triangles_drawn)
    if keep:
        return fb
    px = fb.image().copy(); px.setflags(write=False)
    zb = fb.zbuffer.view(np.uint32).copy(); zb.setflags(write=False)
    return dict(px=px, zb=zb, rcs=rcs, drawn=drawn)


def colour(k):
    """different for neighbouring k, and at most 124: a vertex colour above 128 is overbright and saturates with its neighbours"""
    return (40 + 28 * (k % 4), 40 + 28 * ((k // 4) % 4), 40 + 28 * ((k // 16) % 4))


def stp_texture(mode):
    """2 x 2 white texels with the semi-transparency bit.  A textured face blends by its TEXTURE's mode, and only such texels (render.rs:
    1450-1452, 1681-1694); an untextured face's own blend mode reaches black pixels alone.  editor_alpha needs neither."""
    return Texture15(2, 2, np.full(4, 0xFFFF, np.uint16), mode, f"stp-{mode}")


def solid_call(call):
    """the call with nothing left that blends: opaque faces, full alpha, opaque texture modes"""
    c = dict(call)
    f = np.array(call["f"], copy=True); f["blend_mode"] = abi.OPAQUE; f["editor_alpha"] = 255
    c["f"], c["tex"] = f, [Texture15(t.width, t.height, t.pixels, abi.OPAQUE, t.name) for t in call["tex"]]
    return c


STP_UV = [(0.25, 0.75)] * 3


# ------------------------------------------------------------------------------------------------ family R
R_COUNTS = (2, 31, 32, 33, 64, 65)
R_FOGS = ((4.0, 10.0, 20.0), (2.0, 30.0, 25.0), (6.0, 8.0, 28.0), None)       # (start, falloff, cull distance); the deep face is at 26.5
R_DEEP = 26.5


def r_ambient(j):
    return 0.2 + 0.6 * ((j * 7) % 65) / 65.0


def r_fog(j):
    fg = R_FOGS[j % 4]
    return None if fg is None else fg + (Color(10 + 3 * j, 200 - 2 * j, 50 + j),)


def r_placement(j):
    if j % 3 != 2:
        return None
    s = f32(0.01 * (1 + j % 2))
    return Placement(cos_f=f32(np.sqrt(1.0 - float(s) ** 2)), sin_f=s, world_pos=(0.5 + 0.01 * j, -0.25 - 0.005 * j, 0.0))


@functools.lru_cache(maxsize=None)
def r_members():
    grid = Grid(8)
    out = []
    for j in range(max(R_COUNTS)):
        b = MeshBuilder(f"R{j}", grid, spare_vertices=j % 3)
        b.tri(grid.take(f"R member {j} front face"), FRONT8, 9.0, colour(j), "front")
        b.tri(grid.take(f"R member {j} back face"), back(FRONT8), 9.0, colour(j + 5), "back")
        b.tri(grid.take(f"R member {j} deep face"), FRONT8, R_DEEP, colour(j + 9), "deep")
        pl = r_placement(j)
        out.append(b.build(localise=local_for(pl) if pl is not None else None))
    return out, grid.tags


@functools.lru_cache(maxsize=None)
def family_r(n):
    members, tags = r_members()
    draws = [Draw(j, r_ambient(j), j % 3 != 1, r_fog(j), r_placement(j)) for j in range(n)]
    claims = []
    for j, d in enumerate(draws):
        claims.append(("drawn", j, 3 * j))
        claims.append(("absent" if d.cull else "drawn", j, 3 * j + 1))
        claims.append(("absent" if d.fog is not None and R_DEEP > d.fog[2] else "drawn", j, 3 * j + 2))
    return Frame(f"R-{n}", "R", members[:n], draws, 8, tags, claims=claims)


# ------------------------------------------------------------------------------------------------ family T
def _texels(w, h, seed, first=None, last=None):
    """opaque, never black texels (no STP bit), the first / last one replaced"""
    rng = np.random.default_rng(seed)
    px = (rng.integers(8, 32, w * h) | (rng.integers(8, 32, w * h) << 5) | (rng.integers(8, 32, w * h) << 10)).astype(np.uint16)
    if first is not None and len(px):
        px[0] = first
    if last is not None and len(px):
        px[-1] = last
    return px


def texel_uv(w, h, x, y):
    """all three vertices in the middle of texel (x, y): every fragment samples it (the sampler takes (u, 1 - v))"""
    return [((x + 0.5) / w, 1.0 - (y + 0.5) / h)] * 3


IDENTITY_UV = ((0.0625, 0.9375), (0.9375, 0.9375), (0.0625, 0.0625))
# textures of every T member: (width, height, blend mode, "identity" | "striking" | None)
T_TEXTURES = (
    [(3, 5, abi.OPAQUE, None)],
    [(1, 1, abi.OPAQUE, None), (0, 0, abi.OPAQUE, None), (7, 9, abi.OPAQUE, None)],
    [],
    [(3, 5, abi.OPAQUE, None), (8, 8, abi.OPAQUE, "identity"), (7, 9, abi.OPAQUE, None)],
    [(1, 1, abi.OPAQUE, None), (8, 8, abi.OPAQUE, "identity"), (7, 9, abi.OPAQUE, None)],
    [(8, 8, abi.AVERAGE, "striking"), (3, 5, abi.OPAQUE, None)],
)
FIRST_TEXEL, LAST_TEXEL = 0x8000, 0x0000      # first of a pool: drawn by a face with black_transparent off; last: skipped by one with it on


def t_pool_sizes(padded=False):
    """texels per member; padded: as an upload lays them out, every texture rounded up to 8 texels"""
    return [sum((w * h + 7) & ~7 if padded else w * h for w, h, _, _ in m) for m in T_TEXTURES]


@functools.lru_cache(maxsize=None)
def family_t():
    grid = Grid(16)
    members, claims = [], []
    for j, spec in enumerate(T_TEXTURES):
        b = MeshBuilder(f"T{j}", grid, spare_vertices=(5 * j) % 7)
        nonempty = [k for k, (w, h, _, _) in enumerate(spec) if w * h]
        for k, (w, h, mode, kind) in enumerate(spec):
            if kind == "identity":
                b.textures.append(FS.identity_texture())
                continue
            px = _texels(w, h, 100 * j + k, FIRST_TEXEL if nonempty and k == nonempty[0] else None, LAST_TEXEL if nonempty and k == nonempty[-1] else None)
            if kind == "striking":
                px[1:-1] = 0x7C1F | 0x8000                    # magenta with the STP bit: blends wherever it is sampled
            b.textures.append(Texture15(w, h, px, mode, f"T{j}.{k}"))
        nt = len(spec)
        here = len(claims)
        if nonempty:
            k0, k1 = nonempty[0], nonempty[-1]
            w0, h0 = spec[k0][:2]; w1, h1 = spec[k1][:2]
            c = grid.take(f"T member {j} first texel of its pool (0x8000, black_transparent off: drawn)")
            b.tri(c, FRONT16, 9.0, colour(j), "first", tex=k0, uv=texel_uv(w0, h0, 0, 0), bt=0)
            claims.append(("drawn", j, c))
            c = grid.take(f"T member {j} last texel of its pool (0x0000, black_transparent on: skipped)")
            b.tri(c, FRONT16, 9.0, colour(j + 1), "last", tex=k1, uv=texel_uv(w1, h1, w1 - 1, h1 - 1), bt=1)
            claims.append(("absent", j, c))
            wl, hl = spec[nt - 1][:2]
            c = grid.take(f"T member {j} texture id nt - 1 = {nt - 1} (the last valid own id)")
            b.tri(c, FRONT16, 9.0, (200, 200, 200), "own-last", tex=nt - 1, uv=texel_uv(wl, hl, wl // 2, hl // 2))
            claims.append(("textured", j, c))
        for k, (w, h, _, kind) in enumerate(spec):
            if kind == "identity":
                c = grid.take(f"T member {j} identity-address texture: which texel was sampled")
                b.tri(c, FRONT16, 9.0, (128, 128, 128), "identity", tex=k, uv=IDENTITY_UV)
                claims.append(("textured", j, c))
            if w * h == 0:
                c = grid.take(f"T member {j} zero-size texture {k}: samples transparent")
                b.tri(c, FRONT16, 9.0, colour(j + 2), "zero-size", tex=k)
                claims.append(("absent", j, c))
        for tag, tid in (("id = nt", nt), ("NO_TEXTURE", abi.NO_TEXTURE), ("0xFFFFFFFE", 0xFFFFFFFE)):
            c = grid.take(f"T member {j} texture id {tag}: untextured and opaque")
            b.tri(c, FRONT16, 9.0, colour(j + 3), tag, tex=tid)
            claims.append(("untextured", j, c))
        if j == len(T_TEXTURES) - 1:                                  # the blending member's own textured face: in the transparent pass
            c = grid.take(f"T member {j} striking Average texture on its own face")
            b.tri(c, FRONT16, 9.0, (200, 200, 200), "striking", tex=0, uv=texel_uv(8, 8, 3, 3))
            claims.append(("drawn", j, c))
        members.append(b.build())
        assert len(claims) > here
    draws = [Draw(j, 0.45 + 0.05 * j) for j in range(len(members))]
    fr = Frame("T", "T", members, draws, 16, grid.tags, claims=claims)
    bases = np.cumsum([0] + t_pool_sizes())[1:-1]
    assert all(b % 2 == 1 and b % 32 for b in bases), bases
    return fr


@functools.lru_cache(maxsize=None)
def family_t_error():
    """three runs; the middle run's second member has a face whose third vertex index is its own vertex count.  In merged space that is vertex
    0 of the next member, which lies where the face becomes a visible triangle in the error cell."""
    grid = Grid(16)
    members = []

    def plain(name, k):
        b = MeshBuilder(name, grid)
        b.tri(grid.take(f"{name} face"), FRONT16, 9.0, colour(k), "plain")
        return b.build()
    members += [plain("before-0", 0), plain("before-1", 1)]
    b = MeshBuilder("unused-blend-texture", grid)                    # ends the first run without drawing anything transparent
    b.tri(grid.take("run 1 ender face"), FRONT16, 9.0, colour(2), "plain")
    b.textures.append(Texture15(1, 1, np.array([0x7FFF], np.uint16), abi.AVERAGE, "unused"))
    members.append(b.build())
    members.append(plain("middle-0", 3))
    err_cell = grid.take("error cell: a triangle appears when the index nv is taken for the next member's vertex 0")
    b = MeshBuilder("bad-index", grid)
    b.tri(grid.take("bad-index member, valid face"), FRONT16, 9.0, colour(4), "plain")
    b.tri(err_cell, FRONT16, 9.0, colour(5), "index = nv")
    bad = b.build()                                                  # 6 vertices; the sixth is dropped: the second face's third index, 5, is nv
    third = bad.vertices["pos"][5].copy()
    bad = Member(bad.name, bad.vertices[:5].copy(), bad.faces, [], bad.tags, bad.cells)
    assert bad.faces["v"][1, 2] == len(bad.vertices)
    members.append(bad)
    b = MeshBuilder("middle-2", grid)
    b.pos.append(third[None, :]); b.nv = 1; b.col.append((128, 128, 128)); b.uv.append((0.0, 0.0))      # vertex 0: completes the bad face
    b.tri(grid.take("middle-2 face"), FRONT16, 9.0, colour(6), "plain")
    b.textures.append(Texture15(1, 1, np.array([0x7FFF], np.uint16), abi.AVERAGE, "unused"))
    members.append(b.build())
    members += [plain("after-0", 7), plain("after-1", 8)]
    fr = Frame("T-error", "T", members, [Draw(j) for j in range(len(members))], 16, grid.tags)
    fr.error_member, fr.error_cell, fr.error_run = 4, err_cell, (3, 4, 5)
    return fr


# ------------------------------------------------------------------------------------------------ family Z
def _one_ulp_pair(z):
    """(far, near): the first camera depth at or above z, and its lower neighbour, whose screen depths (depth + 5) differ by one ulp and
    have different reciprocals (the fill interpolates 1 / z: neighbours whose reciprocals round to one f32 would tie at every pixel)"""
    z = f32(z)
    while True:
        n = FS.down(z)
        zs, ns = f32(z + f32(5.0)), f32(n + f32(5.0))
        if FS.bits(zs) - FS.bits(ns) == 1 and f32(1.0) / zs != f32(1.0) / ns:
            return z, n
        z = FS.up(z)


def _z_member(name, grid, k, faces, fillers=0, filler_cell=None):
    """faces: [(cell, depth triple, tag)]; fillers: that many rejected faces in front (back faces and near-rejected ones in turn)"""
    b = MeshBuilder(name, grid, spare_vertices=k)
    for i in range(fillers):
        if i % 2:
            b.tri(filler_cell, FRONT16, (0.05, 3.0, 3.0), (250, 0, 0), "near-rejected")
        else:
            b.tri(filler_cell, back(FRONT16), 9.0, (250, 0, 0), "culled")
    for j, (cell, z, tag) in enumerate(faces):
        b.tri(cell, FRONT16, z, colour(7 * k + j + 1), tag)
    return b.build()


@functools.lru_cache(maxsize=None)
def family_z(variant):
    grid = Grid(16)
    far_z, near_z = _one_ulp_pair(9.0)
    Z = (far_z, 9.5, 10.25)
    near = (near_z, 9.5, 10.25)
    claims = []
    if variant in ("two", "three"):
        n = 2 if variant == "two" else 3
        tie, ulp, f70 = grid.take("Z tie of all members"), grid.take("Z last member nearer by one ulp at one vertex"), grid.take("Z first member's face 70 against the last member's face 0")
        fill = grid.take("Z rejected fillers (nothing drawn)")
        own = [grid.take(f"Z member {k} own face") for k in range(n)]
        members = []
        for k in range(n):
            last = k == n - 1
            faces = []
            if last:
                faces.append((f70, Z, "face 0 of the tie with face 70"))
            faces.append((tie, Z, "tie"))
            if k == 0:
                faces.append((f70, Z, "face 70"))                     # faces 0 .. 68 rejected, 69 the tie, 70 this one
            faces += [(ulp, near if last else Z, "one ulp"), (own[k], 9.0, "own")]
            members.append(_z_member(f"Z{k}", grid, k, faces, fillers=69 if k == 0 else 0, filler_cell=fill))
        assert members[0].tags[70] == "face 70" and members[-1].tags[0].startswith("face 0")
        draws = [Draw(k, 0.4 + 0.1 * k) for k in range(n)]
        claims = [("tie", tie, list(range(n))), ("no_tie", ulp, n - 1), ("tie", f70, [0, n - 1]), ("empty", fill)] + [("drawn", k, own[k]) for k in range(n)]
        return Frame(f"Z-{variant}", "Z", members, draws, 16, grid.tags, claims=claims)
    if variant in ("same", "placed"):
        tie, own = grid.take("Z the same slot twice: tie of the two draws"), grid.take("Z own face")
        other = grid.take("Z second member's face")
        a = _z_member("Za", grid, 1, [(tie, Z, "tie"), (own, 9.0, "own")])
        o = _z_member("Zo", grid, 0, [(other, 9.0, "own")])
        second = Draw(0, 0.8, placement=Placement(**IDENTITY_PLACEMENT) if variant == "placed" else None)
        draws = [Draw(0, 0.3), second, Draw(1, 0.5)]
        return Frame(f"Z-{variant}", "Z", [a, o], draws, 16, grid.tags, claims=[("tie", tie, [0, 1]), ("drawn", 2, other)])
    assert variant == "runs"
    tie = grid.take("Z tie between the last member of a run and the first member of the next")
    cells = [grid.take(f"Z member {k} own face") for k in range(4)]
    a = _z_member("Zr0", grid, 0, [(cells[0], 9.0, "own")])
    b = MeshBuilder("Zr1-ends-run", grid)
    b.tri(tie, FRONT16, Z, colour(3), "tie")
    b.tri(cells[1], FRONT16, 9.0, colour(4), "own")
    b.textures.append(Texture15(1, 1, np.array([0x7FFF], np.uint16), abi.AVERAGE, "unused"))
    c = _z_member("Zr2", grid, 2, [(tie, Z, "tie"), (cells[2], 9.0, "own")])
    d = _z_member("Zr3", grid, 3, [(cells[3], 9.0, "own")])
    return Frame("Z-runs", "Z", [a, b.build(), c, d], [Draw(k, 0.4 + 0.1 * k) for k in range(4)], 16, grid.tags, claims=[("tie", tie, [1, 2])])


Z_VARIANTS = ("two", "three", "same", "placed", "runs")


# ------------------------------------------------------------------------------------------------ family B
B_DEPTHS = (("in front", 8.0), ("behind", 12.0), ("at bit-equal depth", 10.0))        # the transparent face; the opaque one is at 10.0
B_ORDER = ("A", "B", "C", "D", "E", "F", "G", "I", "U", "J", "K")
B_RUNS = (("A", "B", "C"), ("D", "E", "F"), ("G",), ("I", "U"), ("J", "K"))


@functools.lru_cache(maxsize=None)
def family_b():
    grid = Grid(16)
    bl = {n: MeshBuilder(n, grid, spare_vertices=i % 3) for i, n in enumerate(B_ORDER)}
    claims = []
    k = 0
    d_front = d_behind = None
    for n in ("C", "F"):                                        # texture k blends by mode k + 1
        bl[n].textures += [stp_texture(mode) for mode in (abi.AVERAGE, abi.ADD, abi.SUBTRACT, abi.ADD_QUARTER)]
    for under in ("A", "B", "C"):
        for mname, mode, alpha in BLEND_MODES:
            for dname, z in B_DEPTHS:
                c = grid.take(f"B C's {mname} face {dname} of {under}'s opaque face")
                bl[under].tri(c, FRONT16, 10.0, colour(k), f"opaque under {mname} {dname}")
                bl["C"].tri(c, FRONT16, z, colour(k + 7), f"{mname} {dname} of {under}", blend=mode, alpha=alpha,
                              tex=mode - 1 if mode != abi.OPAQUE else abi.NO_TEXTURE, uv=STP_UV)
                claims.append(("blended" if z < 10.0 else "not_blended", B_ORDER.index("C"), c, B_ORDER.index(under)))
                if under == "A" and mname == "average" and dname == "in front":
                    d_front = c
                if under == "B" and mname == "add" and dname == "in front":
                    d_behind = c
                k += 1
    # D: an opaque face in front of one of C's transparent fragments, one behind another (and in front of the opaque face under it)
    bl["D"].tri(d_front, FRONT16, 7.0, colour(40), "opaque in front of C's transparent fragment")
    bl["D"].tri(d_behind, FRONT16, 9.0, colour(41), "opaque behind C's transparent fragment: drawn, the transparent pass wrote no depth")
    claims += [("wins", B_ORDER.index("D"), d_front), ("wins", B_ORDER.index("D"), d_behind)]
    for n in B_ORDER:
        c = grid.take(f"B member {n} own opaque face")
        bl[n].tri(c, FRONT16, 9.0, colour(k), "own"); k += 1
        if n in ("F", "G"):                                     # two blend members follow each other
            bl[n].tri(c, FRONT16, 8.0, colour(k), "own transparent", blend=abi.AVERAGE if n == "F" else abi.OPAQUE, alpha=255 if n == "F" else 128,
                      tex=0 if n == "F" else abi.NO_TEXTURE, uv=STP_UV); k += 1
    bl["U"].textures.append(Texture15(3, 5, _texels(3, 5, 7), abi.ADD, "unused"))       # no face uses it: host bound "may blend", device count 0
    members = [bl[n].build() for n in B_ORDER]
    draws = [Draw(i, 0.35 + 0.04 * i, cull=i % 4 != 3) for i in range(len(members))]
    fr = Frame("B", "B", members, draws, 16, grid.tags, claims=claims)
    fr.d_cells = (d_front, d_behind)
    return fr


# ------------------------------------------------------------------------------------------------ family L
def _tiny_origin(i):
    return 2 * (i % (W // 2)), 2 * (i // (W // 2))


@functools.lru_cache(maxsize=None)
def family_l(total, blend_last=False):
    """32 members whose faces add up to `total`: 2 x 2-pixel triangles, face i of the frame on grid position i"""
    per = total // 32
    counts = [per] * 32
    counts[7] += total - 32 * per
    grid = Grid(2)
    members, i = [], 0
    for j, n in enumerate(counts):
        b = MeshBuilder(f"L{j}", grid)
        for q in range(n):
            last = blend_last and j == 31 and q == n - 1
            b.tri(-1, TINY, 9.0 + (i % 5), colour(i), "tiny", origin=_tiny_origin(i), alpha=128 if last else 255)
            i += 1
        members.append(b.build())
    assert i == total and total <= (W // 2) * (H // 2)
    fr = Frame(f"L-{total}{'-blend' if blend_last else ''}", "L", members, [Draw(j, 0.3 + 0.02 * j) for j in range(32)], 2, [])
    fr.total = total
    return fr


STACK = 2049


@functools.lru_cache(maxsize=None)
def family_l_stack():
    """one opaque member, then a member that stacks 2049 transparent faces, at 2049 depths in scattered order, on one pixel pair"""
    grid = Grid(16)
    c, own = grid.take("L stack of 2049 transparent faces over one opaque face"), grid.take("L stack: opaque member's own face")
    a = MeshBuilder("Lstack-opaque", grid)
    a.tri(c, FRONT16, 20.0, (200, 180, 160), "under the stack")
    a.tri(own, FRONT16, 9.0, colour(3), "own")
    s = MeshBuilder("Lstack", grid)
    s.textures += [stp_texture(mode) for mode in (abi.AVERAGE, abi.ADD_QUARTER, abi.SUBTRACT)]
    x0, y0 = grid.origin(c)
    for i in range(STACK):
        k = (i * 1021) % STACK
        s.tri(c, TINY, 8.0 + k / 512.0, colour(i), f"layer {k}", origin=(x0 + 4, y0 + 4), blend=(abi.AVERAGE, abi.ADD_QUARTER, abi.SUBTRACT)[i % 3], tex=i % 3, uv=STP_UV)
    fr = Frame("L-stack", "L", [a.build(), s.build()], [Draw(0, 0.5), Draw(1, 0.6)], 16, grid.tags)
    fr.total = 2 + STACK
    return fr


# ------------------------------------------------------------------------------------------------ family S
@functools.lru_cache(maxsize=None)
def s_pool():
    """the members the S sequences are made of, each with cells of its own, on one grid"""
    grid = Grid(16)
    pool = {}
    for k in range(5):
        b = MeshBuilder(f"O{k}", grid)
        b.tri(grid.take(f"S opaque member {k} front face"), FRONT16, 9.0, colour(k), "front")
        b.tri(grid.take(f"S opaque member {k} back face"), back(FRONT16), 9.0, colour(k + 5), "back")
        pool[f"O{k}"] = b.build()
    for k in range(2):
        b = MeshBuilder(f"X{k}", grid)
        c = grid.take(f"S blend member {k}")
        b.tri(c, FRONT16, 10.0, colour(20 + k), "opaque")
        b.tri(c, FRONT16, 8.0, colour(24 + k), "transparent", alpha=128)
        pool[f"X{k}"] = b.build()
    b = MeshBuilder("E8", grid)
    b.tri(grid.take("S 8-bit-colour member"), FRONT16, 9.0, colour(30), "front")
    pool["E8"] = b.build(fmt8=True)
    pool["EMPTY"] = MeshBuilder("EMPTY", grid).build()
    return pool, grid.tags


# the zoom under which camera-space x and y of a face at camera depth 9 land on the columns perspective gives them (rows mirrored)
ORTHO_ZOOM = float((FS.M.K("project.distance") - FS.M.K("project.us_sub")) * min(W, H) / FS.M.K("project.viewport_div") * FS.M.K("project.viewport_frac")) / 14.0
S_SEQUENCES = {
    "8bit": (("O0", "O1", "E8", "O2", "O3"), {}),
    "empty": (("O0", "O1", "EMPTY", "O2", "O3"), {}),
    "wire": (("O0", "O1", "O2", "O3", "O4"), {"backface_wireframe": True}),        # the middle member culls: it has a wireframe phase
    "leftover": (("O0", "O1", "X0", "O2"), {}),
    "blend-first-and-last": (("X0", "O0", "O1", "X1"), {}),
    "painter": (("O0", "O1", "O2"), {"use_zbuffer": False}),
    "ortho": (("O0", "O1", "O2"), {"ortho_projection": (ORTHO_ZOOM, 0.0, 0.0)}),
    "xray": (("O0", "O1", "O2"), {"xray_mode": True}),
    "overlay": (("O0", "O1", "O2"), {"wireframe_overlay": True}),
    "batch-off": (("O0", "O1", "O2"), {}),
}
ROUTE_BATCH = 256


@functools.lru_cache(maxsize=None)
def family_s(name):
    pool, tags = s_pool()
    seq, kw = S_SEQUENCES[name]
    names = sorted(set(seq), key=seq.index)
    members = [pool[n] for n in names]
    draws = [Draw(names.index(n), 0.4 + 0.07 * i, cull=(i == 2) if name == "wire" else (i % 2 == 0)) for i, n in enumerate(seq)]
    return Frame(f"S-{name}", "S", members, draws, 16, tags, base=base_settings(**kw), routes_off=ROUTE_BATCH if name == "batch-off" else 0)


# ------------------------------------------------------------------------------------------------ family C
C_SLOTS = 12


@functools.lru_cache(maxsize=None)
def c_members():
    grid = Grid(8)
    tie = grid.take("C tie cell shared by every member")
    out = []
    for k in range(C_SLOTS):
        b = MeshBuilder(f"C{k}", grid, spare_vertices=k % 4)
        b.tri(tie, FRONT8, (9.0, 9.5, 10.25), colour(k), "tie")
        for q in range(2 + (k * 29) % 40):                       # 2 .. 41 own faces: the runs differ in size in no regular order
            b.tri(grid.take(f"C member {k} own face {q}"), FRONT8, 9.0 + q % 3, colour(k + q + 1), "own")
        out.append(b.build())
    return out, grid.tags, tie


def c_pairs():
    """the 66 unordered pairs in a fixed scattered order; run 1 (the first evicted) is a large one"""
    pairs = [(a, b) for a in range(C_SLOTS) for b in range(a + 1, C_SLOTS)]
    members = c_members()[0]
    pairs.sort(key=lambda p: -(members[p[0]].nf + members[p[1]].nf))
    return [pairs[0]] + [pairs[1 + (i * 23) % 65] for i in range(65)]


@functools.lru_cache(maxsize=None)
def family_c(a, b):
    members, tags, tie = c_members()
    fr = Frame(f"C-{a}-{b}", "C", [members[a], members[b]], [Draw(0, 0.4), Draw(1, 0.7)], 8, tags, claims=[("tie", tie, [0, 1])])
    fr.tie = tie
    return fr


# ------------------------------------------------------------------------------------------------ NaN keys in a run
NAN_KINDS = ("pair", "alone", "opaque")
NAN_Z = (3.0, float("nan"), 3.0)


def _ender(name, grid, k):
    """an opaque member that ends its run: its one texture blends, no face uses it"""
    b = MeshBuilder(name, grid)
    b.tri(grid.take(f"{name} face"), FRONT16, 9.0, colour(k), "plain")
    b.textures.append(Texture15(1, 1, np.array([0x7FFF], np.uint16), abi.AVERAGE, "unused"))
    return b.build()


@functools.lru_cache(maxsize=None)
def family_nan(kind):
    """three runs; the middle one holds faces with a NaN depth on their second vertex: two transparent ones in its last member ("pair": the
    reference panics on the key comparison), one ("alone": nothing to compare with), opaque ones in two members ("opaque": z-buffer mode
    never sorts them)"""
    grid = Grid(16)

    def plain(name, k, extra=None):
        b = MeshBuilder(name, grid)
        b.tri(grid.take(f"{name} face"), FRONT16, 9.0, colour(k), "plain")
        if extra:
            extra(b)
        return b.build()

    def nan_faces(n, transparent):
        def fn(b):
            for q in range(n):
                b.tri(grid.take(f"{b.name} NaN-depth face {q}"), FRONT16, NAN_Z, colour(11 + q), "nan", blend=abi.AVERAGE if transparent else abi.OPAQUE)
        return fn
    members = [plain("before-0", 0), plain("before-1", 1), _ender("before-2", grid, 2)]
    if kind == "opaque":
        members += [plain("middle-0", 3, nan_faces(1, False)), plain("middle-1", 4, nan_faces(2, False)), _ender("middle-2", grid, 5)]
    else:
        members += [plain("middle-0", 3), plain("middle-1", 4), plain("middle-2", 5, nan_faces(2 if kind == "pair" else 1, True))]
    members += [plain("after-0", 7), plain("after-1", 8)]
    fr = Frame(f"NaN-{kind}", "V", members, [Draw(j, 0.4 + 0.05 * j) for j in range(len(members))], 16, grid.tags)
    fr.error_member, fr.error_run = (5 if kind == "pair" else None), (3, 4, 5)
    return fr


# ------------------------------------------------------------------------------------------------ named mutations of the call sequence
def _with_rows(fr, row_of):
    calls = fr.calls()
    for j, c in enumerate(calls):
        d = fr.draws[row_of(j)]
        c["st"], c["fog"] = fr.settings_of(d), d.fog
    return calls


def _run_pool(fr):
    sizes = [sum(t.width * t.height for t in m.textures) for m in fr.members]
    pool = np.concatenate([t.pixels for m in fr.members for t in m.textures] + [np.zeros(64, np.uint16)])
    return sizes, pool


def mut_pool_base_rounded(O, fr, r):
    """every member's pool base rounded up to a multiple of r while the texels lie where they are"""
    sizes, pool = _run_pool(fr)
    calls = fr.calls()
    true_base = rounded = 0
    for c, m, size in zip(calls, fr.members, sizes):
        off, tex = 0, []
        for t in m.textures:
            n = t.width * t.height
            tex.append(Texture15(t.width, t.height, pool[rounded + off:rounded + off + n].copy(), t.blend_mode, t.name))
            off += n
        c["tex"] = tex
        true_base += size
        rounded = -(-(rounded + size) // r) * r
        assert rounded - true_base < 64
    return render_calls(O, calls)


def _flip_bt(fr, tags):
    calls = fr.calls()
    for c, m in zip(calls, fr.members):
        f = np.array(m.faces, copy=True)
        for i, t in enumerate(m.tags):
            if t in tags:
                f["black_transparent"][i] ^= 1
        c["f"] = f
    return calls


def _split(m, transparent):
    """the member's opaque or transparent faces alone"""
    tr = (m.faces["blend_mode"] != abi.OPAQUE) | (m.faces["editor_alpha"] < 255)
    return m.faces[tr if transparent else ~tr]


def mut_blend_not_last(O, fr):
    calls = fr.calls()
    c = B_ORDER.index("C")
    opaque, transp = dict(calls[c]), dict(calls[c])
    opaque["f"], transp["f"] = _split(fr.members[c], False), _split(fr.members[c], True)
    return render_calls(O, calls[:c] + [opaque, calls[c + 1], transp] + calls[c + 2:])


def mut_transparent_writes_depth(O, fr):
    """C's transparent pass leaves its depths behind: taken from a second framebuffer on which C's transparent faces are drawn as opaque"""
    calls = fr.calls()
    c = B_ORDER.index("C")
    opaque, transp = dict(calls[c]), dict(calls[c])
    opaque["f"], transp["f"] = _split(fr.members[c], False), _split(fr.members[c], True)
    solid = solid_call(transp)
    fb = O.Framebuffer(W, H); fb.clear(CLEAR)
    render_calls(O, calls[:c] + [opaque], fb)
    side = O.Framebuffer(W, H)
    side.pixels[:] = fb.pixels; side.zbuffer[:] = fb.zbuffer
    render_calls(O, [solid], side)
    render_calls(O, [transp], fb)
    fb.zbuffer[:] = side.zbuffer
    render_calls(O, calls[c + 1:], fb)
    return dict(px=fb.image().copy(), zb=fb.zbuffer.view(np.uint32).copy())


def mut_tie_by_face_index(O, fr):
    """every face a call of its own, in the order (face index, draw)"""
    calls = fr.calls()
    out = []
    for i in range(max(m.nf for m in fr.members)):
        for c in calls:
            if i < len(c["f"]):
                one = dict(c); one["f"] = c["f"][i:i + 1]
                out.append(one)
    return render_calls(O, out)


def mut_tex_unbounded(O, fr):
    calls = fr.calls()
    for j, c in enumerate(calls[:-1]):
        c["tex"] = fr.members[j].textures + fr.members[j + 1].textures
    return render_calls(O, calls)


def mut_vert_unbounded(O, fr):
    calls = fr.calls()
    j = fr.error_member
    calls[j]["v"] = np.concatenate([fr.members[j].vertices, fr.members[j + 1].vertices])
    return render_calls(O, calls)


def mut_placement_of_neighbour(O, fr):
    calls = fr.calls()
    n = len(calls)
    for j, c in enumerate(calls):
        pl = fr.draws[(j + 1) % n].placement
        c["v"] = pl.apply(fr.members[fr.draws[j].member].vertices) if pl is not None else fr.members[fr.draws[j].member].vertices
    return render_calls(O, calls)


# name -> (frame, family of the cells it must change, mutated result of (O, frame))
MUTATIONS = {
    "rows_shifted": ("R-33", lambda O, fr: render_calls(O, _with_rows(fr, lambda j: (j + 1) % len(fr.draws)))),
    "rows_mod_16": ("R-33", lambda O, fr: render_calls(O, _with_rows(fr, lambda j: j - 16 if j >= 16 else j))),
    "row_32_aliases_0": ("R-33", lambda O, fr: render_calls(O, _with_rows(fr, lambda j: 0 if j == 32 else j))),
    "placement_of_neighbour": ("R-33", mut_placement_of_neighbour),
    "tex_unbounded": ("T", mut_tex_unbounded),
    "pool_base_rounded_to_2": ("T", lambda O, fr: mut_pool_base_rounded(O, fr, 2)),
    "pool_base_rounded_to_32": ("T", lambda O, fr: mut_pool_base_rounded(O, fr, 32)),
    "mask_of_neighbour": ("T", lambda O, fr: render_calls(O, _flip_bt(fr, ("first", "last")))),
    "vert_unbounded": ("T-error", mut_vert_unbounded),
    "tie_later": ("Z-two", lambda O, fr: render_calls(O, fr.calls()[::-1])),
    "tie_by_face_index": ("Z-two", mut_tie_by_face_index),
    "blend_not_last": ("B", mut_blend_not_last),
    "transparent_writes_depth": ("B", mut_transparent_writes_depth),
}


# ------------------------------------------------------------------------------------------------ the frames by name
def frames():
    """name -> builder of every frame the GPU tests draw (family C apart)"""
    out = {f"R-{n}": functools.partial(family_r, n) for n in R_COUNTS}
    out["T"] = family_t
    out.update({f"Z-{v}": functools.partial(family_z, v) for v in Z_VARIANTS})
    out["B"] = family_b
    out.update({f"S-{n}": functools.partial(family_s, n) for n in S_SEQUENCES})
    return out


L_FRAMES = {"L-8192": (8192, False), "L-8193": (8193, False), "L-2048-blend": (2048, True), "L-2049-blend": (2049, True)}


def frame(name):
    if name in L_FRAMES:
        return family_l(*L_FRAMES[name])
    if name == "L-stack":
        return family_l_stack()
    if name == "T-error":
        return family_t_error()
    if name.startswith("NaN-"):
        return family_nan(name[4:])
    return frames()[name]()


# ------------------------------------------------------------------------------------------------ the device side
def upload(fb, fr):
    """one detached ResidentScene per member of the frame"""
    from bonnie32_amd import rasterizer as R
    return [R.ResidentScene(fb, m.vertices, m.faces, None if m.fmt8 else m.textures, textures8=[Texture.from_texture15(t) for t in m.textures] if m.fmt8 else None).detach()
            for m in fr.members]


def gpu_frame(ctx, fb, fr, slots, entry="begin", band=None, finish=True):
    """clear, then the frame through frame_begin / frame_add / frame_end or through frame_submit -> timings of the finish"""
    fb.clear(CLEAR)
    if band:
        fb.set_band(*band)
    if entry == "begin":
        ctx.frame_begin(CAM, fr.base)
        for d in fr.draws:
            ctx.frame_add(slots[d.member], ambient=d.ambient, backface_cull=d.cull, fog=d.fog, placement=d.placement)
        ctx.frame_end()
    else:
        placed = [d.placement for d in fr.draws]
        table = ctx.make_frame_table(CAM, fr.base, [slots[d.member] for d in fr.draws], fogs=[d.fog for d in fr.draws], ambients=[d.ambient for d in fr.draws],
                                     placements=placed if any(p is not None for p in placed) else None, backface_culls=[d.cull for d in fr.draws])
        ctx.frame_submit(table)
    return ctx.finish() if finish else None
