"""Blend stacks: sheets on which the ordered pass (k_blend, csrc/b32_blend.hip) decides every pixel by the ORDER of its fragments, and the
replay that restates that order on the CPU (tests/test_blend_stacks.py).

A layer is one screen-aligned quad of two faces (TL, TR, BR) and (TL, BR, BL) on integer screen coordinates (fixed-point projection); the
fill covers the closed triangle, so a layer with vertex rows r0 and r1 - 1 covers the pixel rows [r0, r1), and the pixels of the quad's
diagonal receive a fragment from either face.  Vertex colour 128 (the front is the texel), dithering off, a texture of its own per layer:
one texel per column, every channel a ramp 1 + (offset + slope * x / 8) mod 31 with a per-layer offset and slope (never black: black
fronts blend, and a black texel is skipped).  Layer k takes its mode from the cycle Average, Add, Subtract, AddQuarter; every fifth layer
(k mod 5 = 4) is a plain store: its texture has the mode, its texels lack bit 15.  The framebuffer is uploaded first with a back image
that varies along x.

  ladder   layer k covers the rows [k, H): row y holds the layers 0 .. y; odd layers cover only the left (columns [0, 40)) or the right
           (columns [24, W)) part, alternately, so the lanes of a wave receive different numbers of fragments.  200 layers, 64 x 208;
           "ladder70" is 70 wide: its second tile column has 6 pixels
  window   layer k covers the rows [k, k + 6): six consecutive layers per pixel, about 70 layers and 140 list entries per tile
  cap      1024 quads of 8 x 8 pixels on one 64 x 64 tile, 16 deep: 2048 transparent list entries; "cap2049" has one more face
  depth    transparent layers (plain and editor-alpha stores) over opaque occluders at a smaller, an equal and a greater depth
  depth8   the 8-bit path: pairs of sloped layers whose depths cross inside the quad
  xray     a ladder of opaque and transparent layers interleaved in face order

Key schedules (SCHEDULES): the painter's order is descending mean depth, ties in face order.  The layers of the ladder and the window are
always MEANT to be drawn in layer order, 0 first; the schedule decides where they stand in the mesh.  "along": the mesh holds them in layer
order and the depth falls with k; "against": the mesh holds them in reverse; "permuted": the mesh holds layer (77 i + 13) mod 200 at place
i; "equal": one depth for all, mesh in layer order, so that the order rests on the tie rule alone.  The two faces of a layer always tie.
All four give the same frame.

This module only builds and replays; what the tests compare is always the oracle's frame."""
import functools
from dataclasses import dataclass, field

import numpy as np

from bonnie32_amd import abi
from bonnie32_amd.rtypes import Camera, RasterSettings, Texture, Texture15, make_faces, make_vertices
from oracle import np_model as M
from tests import frontend_sheets as FS

MODES = (abi.AVERAGE, abi.ADD, abi.SUBTRACT, abi.ADD_QUARTER)
SCHEDULES = ("along", "against", "equal", "permuted")
N_LAYERS = 200
TILE = 64
BATCH = 64                           # surfaces k_blend stages per round of a tile (cs += 64)
LIST_CAP = 8                         # BLEND_LIST_CAP: fragments a lane notes per round
WAVES = 4                            # B32_BLEND_NT / 64: a lane owns column x of the rows w, w + 4, ...
SORT_CAP = 2048                      # BLEND_SORT_CAP
QUAD, LONE = (0, 1, 2, 3), (0, 1, 2)  # a layer's faces: (TL, TR, BR) and (TL, BR, BL), or the first alone


@dataclass
class Layer:
    k: int
    c0: int
    c1: int                          # columns [c0, c1)
    r0: int
    r1: int                          # rows [r0, r1)
    z: object                        # camera depth: one value, or four (TL, TR, BR, BL)
    mode: int = abi.OPAQUE           # the texture's blend mode
    plain: bool = False              # texels without bit 15: stored, not blended
    alpha: int = 255
    colour: tuple = None             # untextured, flat vertex colour (an opaque occluder) instead of a texture
    tex: int = None                  # texture index (filled in by the builder)
    faces: tuple = QUAD              # which of the quad's two triangles exist: (TL, TR, BR) and (TL, BR, BL); a lone face: (0, 1, 2)

    @property
    def transparent(self):
        return self.colour is None and (self.mode != abi.OPAQUE or self.alpha < 255)


def ramp_texels(k, width, plain):
    """layer k's texture row: per channel 1 + (offset + slope * x / 8) mod 31, offsets and slopes from k"""
    x = np.arange(width, dtype=np.int64)
    ch = []
    for c in range(3):
        off = (7 * k + 11 * c + 3) % 31
        slope = 3 + (5 * k + 7 * c) % 17
        ch.append(1 + (off + (slope * x) // 8) % 31)
    return ((0 if plain else 0x8000) | (ch[0] << 10) | (ch[1] << 5) | ch[2]).astype(np.uint16)


def back_image(height, width, step=8):
    """every byte value per channel along x, the phase moving per row and differing per channel (as sheet B of tests/pixel_swatches.py)"""
    y, x = np.mgrid[0:height, 0:width]
    img = np.zeros((height, width, 4), np.uint8)
    img[..., 0] = (3 * x + step * y) & 255
    img[..., 1] = (3 * x + step * y + 85) & 255
    img[..., 2] = (3 * x + step * y + 170) & 255
    img[..., 3] = 255
    return img


@dataclass
class Stack:
    name: str
    width: int
    height: int
    layers: list
    vertices: np.ndarray
    faces: np.ndarray
    textures: list
    layer_of_face: np.ndarray
    back: np.ndarray
    fmt8: bool = False
    zbuffer: bool = False
    xray: bool = False
    schedule: str = None
    _cache: dict = field(default_factory=dict)

    @property
    def n(self):
        return len(self.faces)

    def settings(self, zbuffer=None, xray=None):
        st = RasterSettings.benchmark()          # affine, fixed point, painter's, no lights
        st.dithering = False
        st.backface_cull = False
        st.use_zbuffer = self.zbuffer if zbuffer is None else zbuffer
        st.use_rgb555 = not self.fmt8
        st.xray_mode = self.xray if xray is None else xray
        return st

    def oracle(self, O, frames=1, **kw):
        """dict(px [H, W, 4], zb bits, tm, dump) of the C oracle after `frames` draws onto the back image; cached, read-only"""
        key = ("oracle", frames) + tuple(sorted(kw.items()))
        if key not in self._cache:
            fb = O.Framebuffer(self.width, self.height)
            fb.pixels[:] = self.back.reshape(-1)
            st = self.settings(**kw)
            for _ in range(frames):
                with np.errstate(all="ignore"):
                    rc, tm, d = (O.render_mesh if self.fmt8 else O.render_mesh_15)(fb, self.vertices, self.faces, self.textures, Camera(), st, dump=True)
                assert rc == 0
            px = fb.image().copy(); px.setflags(write=False)
            zb = fb.zbuffer.view(np.uint32).copy(); zb.setflags(write=False)
            self._cache[key] = dict(px=px, zb=zb, tm=tm, dump=d)
        return self._cache[key]

    def model(self, **kw):
        """dict(px, zb bits, tap, res) of the numpy model with its per-pixel tap on; cached"""
        key = ("model",) + tuple(sorted(kw.items()))
        if key not in self._cache:
            px = self.back.copy().reshape(-1)
            zb = np.full(self.width * self.height, np.finfo(np.float32).max, np.float32)
            tap = []
            st = self.settings(**kw)
            with np.errstate(all="ignore"):
                if self.fmt8:
                    res = M.render_mesh(px, self.width, self.height, self.vertices, self.faces, self.textures, Camera(), st, zbuffer=zb, tap=tap)
                else:
                    res = M.render_mesh_15(px, self.width, self.height, self.vertices, self.faces, self.textures, Camera(), st, None, zb, tap=tap)
            px = px.reshape(self.height, self.width, 4); px.setflags(write=False)
            self._cache[key] = dict(px=px, zb=zb.view(np.uint32), tap=tap, res=res)
        return self._cache[key]

    def intended_order(self):
        """the faces in the order the schedule means them to be drawn: layer after layer, the faces of a layer in face order"""
        return np.argsort(self.layer_of_face, kind="stable").astype(np.uint32)

    def describe(self, x, y):
        who = sorted((L for L in self.layers if L.c0 <= x < L.c1 and L.r0 <= y < L.r1), key=lambda L: L.k)
        return f"{len(who)} layers at the pixel, the last ones by layer number: " + ", ".join(
            f"{L.k} (mode {L.mode}{' plain' if L.plain else ''}{'' if L.alpha == 255 else f' alpha {L.alpha}'}{' opaque' if L.colour else ''})" for L in who[-6:])

    def first_difference(self, got, want, what):
        """'' when equal, else a message naming the first offending pixel and the layers stacked on it"""
        g = np.asarray(got).reshape(self.height, self.width, -1)
        w = np.asarray(want).reshape(self.height, self.width, -1)
        bad = (g != w).any(axis=2)
        if not bad.any():
            return ""
        y, x = [int(v[0]) for v in np.nonzero(bad)]
        return (f"[{self.name} {what}] {int(bad.sum())} pixels differ, rows {int(np.nonzero(bad.any(axis=1))[0][0])}..{int(np.nonzero(bad.any(axis=1))[0][-1])}, "
                f"first at ({x}, {y}): got {g[y, x].tolist()}, oracle {w[y, x].tolist()}; {self.describe(x, y)}")


def depth_schedule(schedule, n):
    """camera depth of layer k: multiples of 0.25 between 40 and 90 (exact in f32, also after the + 5.0 of the projection)"""
    return [60.0 if schedule == "equal" else 90.0 - 0.25 * k for k in range(n)]


def mesh_order(schedule, n):
    """which layer stands at place i of the mesh"""
    if schedule == "against":
        return list(range(n))[::-1]
    if schedule == "permuted":
        return [(77 * i + 13) % n for i in range(n)]
    return list(range(n))


def build(name, width, height, layers, fmt8=False, zbuffer=False, xray=False, schedule=None, shared_textures=None, tex_width=None):
    """The mesh of the layers, in layer order; a texture per textured layer (or `shared_textures`: (list, index of layer k))."""
    nl = len(layers)
    tw = tex_width or width                  # a texel per column of the sheet's content
    v = make_vertices(4 * nl)
    tx, ty, cz = [], [], []
    textures = [] if shared_textures is None else shared_textures[0]
    fv, flayer = [], []
    for i, L in enumerate(layers):
        a = 4 * i
        assert L.c1 - L.c0 >= 2 and L.r1 - L.r0 >= 2, (name, L)
        corners = ((L.c0, L.r0), (L.c1 - 1, L.r0), (L.c1 - 1, L.r1 - 1), (L.c0, L.r1 - 1))
        zs = [L.z] * 4 if np.ndim(L.z) == 0 else list(L.z)
        for j, (x, y) in enumerate(corners):
            tx.append(x); ty.append(y); cz.append(zs[j])
            v["uv"][a + j] = ((x + 0.5) / tw, 0.5)
        if L.colour is None:
            if shared_textures is None:
                textures.append(Texture15(tw, 1, ramp_texels(L.k, tw, L.plain), L.mode, f"layer{L.k}"))
                L.tex = len(textures) - 1
            else:
                L.tex = shared_textures[1](L)
            col = (128, 128, 128)
        else:
            col = L.colour
        v["r"][a:a + 4], v["g"][a:a + 4], v["b"][a:a + 4] = col
        for tri in ((0, 1, 2), (0, 2, 3)):
            if set(tri) <= set(L.faces):
                fv.append((a + tri[0], a + tri[1], a + tri[2])); flayer.append(i)
    v["pos"] = FS.place("fixed", Camera(), np.array(tx, np.float64), np.array(ty, np.float64), np.array(cz, np.float32), width, height)
    v["normal"] = (0.0, 0.0, -1.0)
    v["blend"] = abi.OPAQUE
    f = make_faces(len(fv))
    f["v"] = np.array(fv, np.uint32)
    for fi, i in enumerate(flayer):
        L = layers[i]
        f["texture_id"][fi] = abi.NO_TEXTURE if L.tex is None else L.tex
        f["blend_mode"][fi] = abi.OPAQUE
        f["editor_alpha"][fi] = L.alpha
        f["black_transparent"][fi] = 1
    if fmt8:
        textures = [Texture.from_texture15(t, stp_blend=t.blend_mode) for t in textures]
    v.setflags(write=False); f.setflags(write=False)
    return Stack(name, width, height, layers, v, f, textures, np.array([layers[i].k for i in flayer]), back_image(height, width),
                 fmt8=fmt8, zbuffer=zbuffer, xray=xray, schedule=schedule)


def check_placement(st, res):
    """every vertex landed on its integer target (the numpy model's projected coordinates)"""
    want = np.array([c for L in st.layers for c in ((L.c0, L.r0), (L.c1 - 1, L.r0), (L.c1 - 1, L.r1 - 1), (L.c0, L.r1 - 1))])
    assert np.array_equal(res["sx"], want[:, 0]) and np.array_equal(res["sy"], want[:, 1]), f"{st.name}: a vertex missed its target"


def _mode_of(k):
    return MODES[k % 4], k % 5 == 4


def _columns(k, width):
    if k % 2 == 0:
        return 0, width
    return (0, 40) if (k // 2) % 2 == 0 else (24, width)


@functools.lru_cache(maxsize=None)
def ladder(schedule="along", width=64, frame_width=None):
    """frame_width: the same 64 columns at the left of a wider frame (more tile columns: the cut grid keeps taller tiles)"""
    H = N_LAYERS + 8
    z = depth_schedule(schedule, N_LAYERS)
    layers = []
    for k in range(N_LAYERS):
        mode, plain = _mode_of(k)
        c0, c1 = _columns(k, width)
        layers.append(Layer(k, c0, c1, k, H, z[k], mode, plain, faces=LONE if k == 0 else QUAD))
    return build(f"ladder{'' if width == 64 else width}-{schedule}{f'-in{frame_width}' if frame_width else ''}", frame_width or width, H,
                 [layers[k] for k in mesh_order(schedule, N_LAYERS)], schedule=schedule, tex_width=width)


@functools.lru_cache(maxsize=None)
def window(schedule="along"):
    H = N_LAYERS + 6
    z = depth_schedule(schedule, N_LAYERS)
    layers = []
    for k in range(N_LAYERS):
        mode, plain = _mode_of(k)
        c0, c1 = _columns(k, 64)
        layers.append(Layer(k, c0, c1, k, k + 6, z[k], mode, plain, faces=LONE if k == 0 else QUAD))
    return build(f"window-{schedule}", 64, H, [layers[k] for k in mesh_order(schedule, N_LAYERS)], schedule=schedule)


CAP_TEXTURES = 20


@functools.lru_cache(maxsize=None)
def cap(extra, bare=False):
    """1024 quads of 8 x 8 pixels on the 64 cells of one 64 x 64 tile, 16 per cell: 2048 transparent faces, every one an entry of the
    tile's list; `extra` lone faces more; four opaque quads underneath (none when `bare`: 2048 faces in all).  Depths: 64 levels, scattered over the quads (many ties)."""
    textures = []
    for t in range(CAP_TEXTURES):
        mode, plain = _mode_of(t)
        textures.append(Texture15(64, 1, ramp_texels(t, 64, plain), mode, f"cap{t}"))
    layers = [Layer(k, 32 * (k % 2), 32 * (k % 2) + 32, 32 * (k // 2), 32 * (k // 2) + 32, 95.0, colour=(40 + 50 * k, 200 - 40 * k, 90 + 30 * k)) for k in range(0 if bare else 4)]
    for q in range(1024 + extra):
        k = 4 + q
        cell = (q * 37) % 64 if q < 1024 else 5 + 9 * (q - 1024)
        x0, y0 = 8 * (cell % 8), 8 * (cell // 8)
        L = Layer(k, x0, x0 + 8, y0, y0 + 8, 20.0 + 0.25 * ((q * 29) % 64), *_mode_of(q % CAP_TEXTURES))
        if q >= 1024:
            L.faces = LONE
        layers.append(L)
    return build(f"cap{SORT_CAP + extra}{'-bare' if bare else ''}", 64, 64, layers, shared_textures=(textures, lambda L: (L.k - 4) % CAP_TEXTURES))


def tile_entries(st, tx, ty, tile_h=TILE, transparent_only=True):
    """The faces whose clipped bounding box reaches tile (tx, ty), as the binning counts them (b32_setup.hip / b32_bin.hip: the box of the
    projected vertices, max + 1, clipped to the frame; a face with an empty box makes no entry).  The sheets hold no degenerate face."""
    res = st.model()["res"]
    sx, sy = res["sx"], res["sy"]
    out = []
    for fi in range(st.n):
        ids = st.faces["v"][fi]
        xs, ys = sx[ids], sy[ids]
        x0, x1 = max(int(xs.min()), 0), min(int(xs.max()) + 1, st.width)
        y0, y1 = max(int(ys.min()), 0), min(int(ys.max()) + 1, st.height)
        if x0 >= x1 or y0 >= y1:
            continue
        if x0 < (tx + 1) * TILE and x1 > tx * TILE and y0 < (ty + 1) * tile_h and y1 > ty * tile_h:
            out.append(fi)
    if transparent_only:
        tr = {L.k for L in st.layers if L.transparent}
        out = [fi for fi in out if int(st.layer_of_face[fi]) in tr]
    return out


# ------------------------------------------------------------------------------------------------ depth sheets
@functools.lru_cache(maxsize=None)
def depth(nan=None):
    """z-buffer mode, RGB555.  Three bands of columns hold an opaque occluder at camera depth 40 (nearer than the transparent layers of
    the cell, which are rejected), at the layers' own depth (`z < zb` and `!(z >= zb)` both reject), and at 80 (behind: they draw); every
    band is crossed by rows of transparent layers at depth 60, four deep, plain-mode stores and editor-alpha stores alternating, and two
    sloped layers whose depth crosses the occluder's inside the quad.  Depth is never written by the transparent pass: the z-buffer the
    frame leaves is the occluders'."""
    layers = []
    k = 0
    for b, zo in enumerate((40.0, 60.0, 80.0)):
        layers.append(Layer(k, 2 + 21 * b, 21 + 21 * b, 0, 64, zo, colour=(60 + 70 * b, 220 - 60 * b, 100 + 20 * b))); k += 1
    if nan:
        # one lone face with a NaN depth on its second vertex (fixed point projects it from 0, so its screen point is finite): every
        # fragment's depth is NaN.  Alone in the transparent list its NaN key is accepted (two members would be the reference's panic)
        layers.append(Layer(k, 0, 64, 10, 50, (60.0, float("nan"), 60.0, 60.0), abi.ADD, nan == "plain", 255 if nan == "plain" else 128, faces=LONE))
        return build(f"depth-nan-{nan}", 64, 64, layers, zbuffer=True)
    for row in range(7):
        for d in range(4):
            mode, plain = _mode_of(k)
            alpha = 255 if (row + d) % 2 == 0 else (128, 200, 77)[d % 3]
            z = 60.0
            if row >= 5:                                          # sloped: 50 on the left, 70 on the right (row 5), or top to bottom (row 6)
                z = (50.0, 70.0, 70.0, 50.0) if row == 5 else (50.0 + d, 50.0 + d, 70.0 - d, 70.0 - d)
            if row == 3:
                z = 60.0 + 0.25 * d                               # four depths: the painter's order of the pass is not the face order
            layers.append(Layer(k, 0, 64, 1 + 9 * row, 1 + 9 * row + 8, z, mode, plain, alpha)); k += 1
    return build("depth", 64, 64, layers, zbuffer=True)


@functools.lru_cache(maxsize=None)
def depth8():
    """The 8-bit path in z-buffer mode with blending texels: one list, drawn in face order (the reference sorts that list in painter's
    mode only), every store writes the running depth.  Pairs of sloped layers whose depths cross inside the quad -- the later one is
    rejected on one side of the crossing -- along x and along y, the nearer-on-the-left member first and second, over an opaque layer
    behind; plain (Opaque texel) and blending members."""
    layers = [Layer(0, 0, 64, 0, 96, 90.0, colour=(90, 160, 210))]
    k = 1
    for row in range(10):
        lo, hi = 40.0 + row, 70.0 - row
        za = (lo, hi, hi, lo) if row % 2 == 0 else (lo, lo, hi, hi)
        zb = (hi + 1.0, lo, lo, hi + 1.0) if row % 2 == 0 else (hi + 1.0, hi + 1.0, lo, lo)      # mean depth 0.5 above its partner's
        pair = [za, zb] if row % 4 < 2 else [zb, za]
        for z in pair:
            mode, plain = _mode_of(k + row)
            layers.append(Layer(k, 3, 61, 2 + 9 * row, 2 + 9 * row + 8, z, mode, plain)); k += 1
    return build("depth8", 64, 96, layers, fmt8=True, zbuffer=True)


@functools.lru_cache(maxsize=None)
def xray():
    """A ladder of 96 layers, every other one an opaque (untextured, flat) quad, in face order: x-ray blends every surface,
    (front + back) / 2, the opaque list first (painter's order), then the transparent one."""
    H = 104
    layers = []
    z = [90.0 - 0.25 * ((37 * k) % 96) for k in range(96)]         # scattered: neither list is in face order
    for k in range(96):
        c0, c1 = _columns(k + 1, 64) if k % 3 == 0 else (0, 64)
        if k % 2 == 0:
            layers.append(Layer(k, c0, c1, k, H, z[k], colour=((37 * k) % 256, (91 * k + 60) % 256, (53 * k + 140) % 256)))
        else:
            layers.append(Layer(k, c0, c1, k, H, z[k], *_mode_of(k // 2)))
    return build("xray", 64, H, layers, xray=True)


def face_depths(st, fi):
    """[H, W] f32: the depth the reference interpolates for face fi at every pixel it covers, FLT_MAX elsewhere -- the face drawn alone
    by the numpy model as an opaque, untextured face onto a cleared z-buffer, which stores exactly that depth (same vertices, same
    arithmetic as the face's own draw)"""
    f = st.faces[[fi]].copy()
    f["texture_id"], f["editor_alpha"], f["blend_mode"] = abi.NO_TEXTURE, 255, abi.OPAQUE
    px = np.zeros(st.width * st.height * 4, np.uint8)
    zb = np.full(st.width * st.height, np.finfo(np.float32).max, np.float32)
    with np.errstate(all="ignore"):
        M.render_mesh_15(px, st.width, st.height, st.vertices, f, [], Camera(), st.settings(zbuffer=True), None, zb)
    return zb.reshape(st.height, st.width)


# ------------------------------------------------------------------------------------------------ the replay
def blend_px(back, front, flag, mode, alpha, xray=False, fmt8=False):
    """One store per element: back, front [n, 3] int64; flag [n] (the fragment blends), mode, alpha [n]"""
    r = front.copy()
    for mval in (1, 2, 3, 4, 5):
        sel = flag & (mode == mval)
        if sel.any():
            r[sel] = M.blend8(front[sel], back[sel], mval) if fmt8 else M.blend555(front[sel], back[sel], mval)
    if xray:
        return (front + back) // 2
    a = alpha[:, None]
    if fmt8:
        assert (alpha == 255).all()
        return r
    return np.where(a < 255, (r * a + back * (255 - a)) // 255, r)


class Replay:
    """The tap of np_model.render_mesh_15 / render_mesh as per-surface fragment records, and the frame they give when they are applied
    again in any order.  A record: pix (flat pixel indices, ascending), front [n, 3], flag [n], mode [n], alpha."""

    def __init__(self, width, height, start, tap, xray=False, fmt8=False):
        self.width, self.height, self.xray, self.fmt8 = width, height, xray, fmt8
        self.start = np.asarray(start).reshape(height * width, 4)[:, :3].astype(np.int64)
        self.recs = []
        for t in tap:
            pix = t["y"].astype(np.int64) * width + t["x"].astype(np.int64)
            assert (np.diff(pix) > 0).all()
            m = t["m"].astype(np.int64)
            if fmt8:
                assert not t["dithered"]
                front, flag, mode = m, np.ones(len(pix), bool), t["texel"][:, 3].astype(np.int64)
            else:
                if t["dithered"]:
                    off = M.DITHER[t["y"] & 3, t["x"] & 3][:, None]
                    q = np.clip((m + off) >> M.K("dither.shift"), M.K("dither.clamp_lo"), M.K("dither.clamp_hi"))
                else:
                    q = m >> M.K("fill.nodither_shift")
                front = M.expand5(q)
                flag = ((t["texel"] & M.K("color15.semi_bit")) != 0) | (q == 0).all(axis=1)
                mode = np.full(len(pix), t["blend"], np.int64)
            self.recs.append(dict(face=int(t["face"]), pix=pix, front=front, flag=flag & (mode != 0), mode=mode,
                                  alpha=np.full(len(pix), t["alpha"], np.int64)))
        self.of_face = {r["face"]: i for i, r in enumerate(self.recs)}
        self.fragments = sum(len(r["pix"]) for r in self.recs)
        self._prefix = None

    def apply(self, state, r, keep=None, only=None):
        """record r onto state [H * W, 3]; keep: mask over the record's fragments; only: sorted flat pixel indices to restrict to"""
        rec = self.recs[r] if not isinstance(r, dict) else r
        pix = rec["pix"]
        if only is not None:
            pos = np.minimum(np.searchsorted(pix, only), len(pix) - 1) if len(pix) else np.zeros(0, np.int64)
            sel = pos[pix[pos] == only] if len(pix) else pos
            if keep is not None:
                sel = sel[keep[sel]]
        else:
            sel = np.arange(len(pix)) if keep is None else np.nonzero(keep)[0]
        if len(sel) == 0:
            return
        p = pix[sel]
        state[p] = blend_px(state[p], rec["front"][sel], rec["flag"][sel], rec["mode"][sel], rec["alpha"][sel], self.xray, self.fmt8)

    def frame(self, order=None):
        """[H * W, 3] after the records in `order` (default: the tap's own): entries are record indices or (index, keep mask)"""
        state = self.start.copy()
        for e in (range(len(self.recs)) if order is None else order):
            if isinstance(e, tuple):
                self.apply(state, e[0], keep=e[1])
            else:
                self.apply(state, e)
        return state

    def prefix(self):
        """[n + 1, H * W, 3] uint8: the frame after the first j records"""
        if self._prefix is None:
            P = np.zeros((len(self.recs) + 1,) + self.start.shape, np.uint8)
            state = self.start.copy()
            P[0] = state
            for j in range(len(self.recs)):
                self.apply(state, j)
                P[j + 1] = state
            self._prefix = P
        return self._prefix

    def mutant(self, a, b, repl):
        """Pixels of the final frame that change when the records [a, b) of the tap's order are replaced by the records `repl`.  Only the
        pixels that differ from the unchanged run are carried on, and the walk ends when none is left."""
        P = self.prefix()
        state = P[a].astype(np.int64)
        for r in repl:
            self.apply(state, r)
        dirty = np.nonzero((state != P[b]).any(axis=1))[0]
        for j in range(b, len(self.recs)):
            if len(dirty) == 0:
                return 0
            self.apply(state, j, only=dirty)
            dirty = dirty[(state[dirty] != P[j + 1][dirty]).any(axis=1)]
        return int(len(dirty))


def replay_of(st, **kw):
    key = ("replay",) + tuple(sorted(kw.items()))
    if key not in st._cache:
        m = st.model(**kw)
        st._cache[key] = Replay(st.width, st.height, st.back, m["tap"], xray=st.settings(**kw).xray_mode, fmt8=st.fmt8)
    return st._cache[key]


def layer_runs(st, rp):
    """[(layer, first record, end record)] in the tap's order: the records of a layer are adjacent in every schedule"""
    runs = []
    for i, r in enumerate(rp.recs):
        k = int(st.layer_of_face[r["face"]])
        if runs and runs[-1][0] == k:
            runs[-1][2] = i + 1
        else:
            runs.append([k, i, i + 1])
    assert len({k for k, _, _ in runs}) == len(runs), "a layer's records are not adjacent"
    return [tuple(r) for r in runs]


# ------------------------------------------------------------------------------------------------ the kernel's walk of one tile, restated
def tile_pixels(st, tx, ty):
    y, x = np.mgrid[ty * TILE:min((ty + 1) * TILE, st.height), tx * TILE:min((tx + 1) * TILE, st.width)]
    return np.sort((y * st.width + x).reshape(-1))


def tile_walk(st, rp, tx, ty, mutate=None):
    """The tile's pixels [n, 3] after its ordered list -- the drawn faces whose box reaches the tile, in draw order -- has been applied
    in batches of 64 entries.  mutate: None, "reverse_batches", "swap_64_65", or "skip_9th": in every batch every lane (column x of the
    rows w, w + 4, ... of the tile) loses the 9th fragment it would note -- rows ascending, surfaces in list order within a row."""
    pix = tile_pixels(st, tx, ty)
    order = [int(f) for f in st.model()["res"]["draw_order"]]
    entries = set(tile_entries(st, tx, ty, transparent_only=False))
    lst = [f for f in order if f in entries and f in rp.of_face]
    if mutate == "swap_64_65":
        lst[64], lst[65] = lst[65], lst[64]
    batches = [lst[i:i + BATCH] for i in range(0, len(lst), BATCH)]
    if mutate == "reverse_batches":
        batches = batches[::-1]
    state = rp.start.copy()
    for batch in batches:
        keeps = [None] * len(batch)
        if mutate == "skip_9th":
            fp, fj, fi = [], [], []
            for j, f in enumerate(batch):
                rec = rp.recs[rp.of_face[f]]
                idx = np.nonzero(np.isin(rec["pix"], pix))[0]
                fp.append(rec["pix"][idx]); fj.append(np.full(len(idx), j)); fi.append(idx)
            fp, fj, fi = np.concatenate(fp), np.concatenate(fj), np.concatenate(fi)
            row, col = fp // st.width - ty * TILE, fp % st.width
            lane = (row % WAVES) * st.width + col
            o = np.lexsort((fj, row // WAVES, lane))
            ls = lane[o]
            first = np.r_[0, np.nonzero(np.diff(ls))[0] + 1]
            rank = np.arange(len(o)) - np.repeat(first, np.diff(np.r_[first, len(o)]))
            lost = o[rank == LIST_CAP]
            for j in range(len(batch)):
                rec = rp.recs[rp.of_face[batch[j]]]
                keep = np.ones(len(rec["pix"]), bool)
                keep[fi[lost[fj[lost] == j]]] = False
                keeps[j] = keep
        for j, f in enumerate(batch):
            rp.apply(state, rp.of_face[f], keep=keeps[j], only=pix)
    return state[pix], len(lst)


# ------------------------------------------------------------------------------------------------ the device side
def gpu_draw(ctx, st, resident=False, band=None, frames=1, fb=None, **kw):
    """`frames` frames of the sheet through the C ABI onto the uploaded back image -> (framebuffer object, timings of the last frame)"""
    from bonnie32_amd import rasterizer as R
    s = st.settings(**kw)
    if fb is None:
        fb = R.Framebuffer(st.width, st.height, ctx)
        fb.upload(st.back)
    if band:
        fb.set_band(*band)
    cam = Camera()
    if resident or frames > 1:
        rs = R.ResidentScene(fb, st.vertices, st.faces, textures8=st.textures) if st.fmt8 else R.ResidentScene(fb, st.vertices, st.faces, st.textures)
        for _ in range(frames):
            tm = rs.render(cam, s)
    elif st.fmt8:
        tm = R.render_mesh(fb, st.vertices, st.faces, st.textures, cam, s)
    else:
        tm = R.render_mesh_15(fb, st.vertices, st.faces, st.textures, cam, s)
    return fb, tm


# ------------------------------------------------------------------------------------------------ census of the random pile scene
def pile_scene():
    """the scene of tests/test_gpu_parity.py::test_transparent_pile_on_the_sort_free_path (painter's mode), built the same way"""
    from bonnie32_amd import scenegen
    sc = scenegen.make_scene("C1", n_tris=1500, bbox_px=120.0, seed=4242, variant="blend")
    modes = np.array(MODES, dtype=sc.faces["blend_mode"].dtype)
    sc.faces["blend_mode"][:] = modes[np.arange(len(sc.faces)) % 4]
    sc.faces["editor_alpha"][::7] = 150
    sc.settings.use_zbuffer = False
    return sc


@functools.lru_cache(maxsize=None)
def pile_census():
    """Per-pixel fragment sequences of the pile scene from the numpy model's tap, replayed, and every fragment dropped in turn.
    -> dict(frame_ok, depth (mean, max fragments per pixel), by_distance: [(fragments at that distance from the top, of which a drop
    changes the final pixel)])"""
    sc = pile_scene()
    img = np.zeros((sc.height, sc.width, 4), np.uint8)
    img[...] = (sc.clear_color.r, sc.clear_color.g, sc.clear_color.b, 255)
    px = img.copy().reshape(-1)
    tap = []
    with np.errstate(all="ignore"):
        res = M.render_mesh_15(px, sc.width, sc.height, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, None, None, tap=tap)
    rp = Replay(sc.width, sc.height, img, tap)
    npix = sc.width * sc.height
    pix = np.concatenate([r["pix"] for r in rp.recs])
    o = np.argsort(pix, kind="stable")                                   # per pixel, in draw order
    pix = pix[o]
    front = np.concatenate([r["front"] for r in rp.recs])[o]
    flag = np.concatenate([r["flag"] for r in rp.recs])[o]
    mode = np.concatenate([r["mode"] for r in rp.recs])[o]
    alpha = np.concatenate([r["alpha"] for r in rp.recs])[o]
    length = np.bincount(pix, minlength=npix)
    first = np.cumsum(length) - length
    L = int(length.max())
    S = np.zeros((npix, L + 1, 3), np.uint8)                              # S[p, j]: pixel p after its first j fragments
    S[:, 0] = rp.start
    for j in range(L):
        sel = np.nonzero(length > j)[0]
        i = first[sel] + j
        S[sel, j + 1] = blend_px(S[sel, j].astype(np.int64), front[i], flag[i], mode[i], alpha[i])
        rest = np.nonzero(length <= j)[0]
        S[rest, j + 1] = S[rest, j]
    frame_ok = np.array_equal(S[:, L].reshape(sc.height, sc.width, 3), px.reshape(sc.height, sc.width, 4)[..., :3])
    by_distance = []
    for d in range(L):                                                   # drop the fragment d below the top
        sel = np.nonzero(length > d)[0]
        pos = length[sel] - 1 - d
        state = S[sel, pos].astype(np.int64)
        dirty = np.nonzero((state != S[sel, pos + 1]).any(axis=1))[0]    # indices into sel
        for t in range(d):
            if len(dirty) == 0:
                break
            p = sel[dirty]
            j = pos[dirty] + 1 + t
            i = first[p] + j
            state[dirty] = blend_px(state[dirty], front[i], flag[i], mode[i], alpha[i])
            dirty = dirty[(state[dirty] != S[p, j + 1]).any(axis=1)]
        by_distance.append((int(len(sel)), int(len(dirty))))
    covered = length[length > 0]
    return dict(frame_ok=frame_ok, fragments=int(res["fragments"]), mean_depth=float(covered.mean()), max_depth=L, by_distance=by_distance)
