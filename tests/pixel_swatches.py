"""Swatch sheets: frames in which every covered pixel is one chosen point of the value domain of the pixel pipeline -- modulate, shade,
dither, quantise, blend, editor alpha -- so that a frame comparison is an enumeration of the domain (tests/test_pixel_swatches.py).

Geometry of every sheet: 256 pixels wide, a stack of full-width quads ("strips") at one camera depth whose vertices sit on exact integer
screen coordinates (coverage_sheets.ScreenMap), each split along a diagonal into two triangles.  The fill covers the closed triangle, so a
quad between the vertex rows y0 and y1 covers the pixel rows y0..y1: a strip of 4 pixel rows (all 16 dither cells) has y1 = y0 + 3, and the
lowest quad that is not degenerate, y1 = y0 + 1, covers TWO pixel rows -- that is what "one row tall" can mean here, and both rows count.
The two triangles of a quad share exactly the lattice points of the diagonal inside the frame, one pixel per strip (0.1 to 0.2 % of the
stored pixels, measured per sheet by test_only_diagonal_pixels_are_stored_twice); an opaque strip stores the same value twice there, a
blending strip blends twice.  The census leaves no pixel out: the numpy model's tap reports the back every store really read, so the
second store counts as the second application that it is.  Texture coordinates run from half a column to one and a half a column
beyond (U_CENTRED), so a column samples the middle of its texel's span and never a texel boundary.

Sheet P, 256 x 1262, 646 faces, one texture (P2: 256 x 1266, a second bound texture and one strip that uses it) -- the opaque pipeline
of the RGB555 path.  The texture is 32 x 3: row 0 holds another 5-bit value per channel at every texel (r = c, g = (5 c + 1) & 31,
b = 31 - c, none 0x0000), row 1 the same with bit 15 set, row 2 the special texels 0x0000, 0x8000, white and white with bit 15 (the
extra rows keep the extra strips on the one bound texture, so that the fused one-texture path draws them too).  256 strips of 4 rows
with the flat vertex colour v = 0..255 on row 0, a texel spanning 8 columns; strips with bit-15 texels; untextured strips with unequal
vertex colours (dithered, `vert` sweeps through every byte along x) and with equal ones (NOT dithered, two rows each); strips over the
special texels with black_transparent on and off.  The interpolated byte is v - 1 at some pixels of a 4-row strip's third row (the
barycentrics are thirds there), for the 39 values of REPAIR_VALUES; those get a second strip half a dither period further down, where
the third dither row is the strip's exact first row.  Census (CPU): all 393 216 (channel, c5, vert, dither cell) = 3 x 32 x 256 x 16
occur with the byte that was really interpolated; `/ 128` reaches 508 before its clamp, the dither's `>> 3` gives -1 and 32 before
its clamp; with dithering off (the same mesh, P-nodither) all 24 576 (channel, c5, vert) occur.  The issue asked for a 32 x 1 texture;
the two extra rows are a deliberate departure, and the flipped v of Texture15::sample that selects a row (tex_row_v) is the one piece
of texture addressing these sheets depend on.  P-plain (256 x 1254, 638 faces) is the same sheet without row 2 and its strips: with
no texel that the black_transparent rule can skip the library may take CHEAP coverage, which the kernels of one-texture frames
(k_cover_plain, k_cover_plain_z) need; its census is the same, in full.

Sheet S, 256 x 110, 70 faces -- the shade factor.  Sheet P's strips at v in {0, 1, 127, 128, 129, 254, 255}; flat and Gouraud shading, no
lights, so the shade is min(ambient, 1.0) and, with Gouraud, bcx s + bcy s + bcz s, which falls short of s at some pixels (1216 pixels
differ between the two at ambient 1.0).  Ambient takes 0, 2^-10, 0.3, 0.5, 1, 1.5, 2, 3, -1 and also -0.0, +inf and NaN: the C oracle and
the numpy model agree on all twelve, flat and Gouraud (test_three_restatements_agree_on_the_shade_factor), so none is left out.
S-plain is the same without the special texels (for k_cover_lit, as P-plain).

Sheet B, 256 x 764, 764 faces, six textures (the texture above with blend mode Average, Add, Subtract, AddQuarter, Erase, Opaque), dithering
off, vertex colour 128 (the front is the texel) -- the transparent store of the RGB555 path.  The framebuffer is uploaded first: every byte
value per channel along x, the phase moving by 8 per row and differing per channel, arbitrary bytes and not only expanded 5-bit ones.
Per mode 16 strips of 2 rows with STP texels (a texel spans 8 columns: 32 rows put every back byte under every front value), a strip
of non-STP texels (stored, not blended), a strip of non-STP texels under vertex colour 3 (all-black: gets bit 15 and blends), strips over
the special texels; untextured faces with each mode as the FACE's mode (white has no STP bit: they blend only where the colour is black)
and a textured face with a face mode (its texture's mode counts: no blend); editor alpha 0, 1, 2, 127, 128, 254 over fronts that do not
blend and over Average and Subtract fronts, 16 strips each, and one strip of every other mode.  Census (CPU): all 122 880 (channel, mode,
front5, back byte) are blended; all 1280 (mode, back byte) through the all-black rule; all 368 640 (channel, alpha > 0, plain / Average
/ Subtract, front5, back byte) are lerped; alpha 0 stores nothing.  The same sheet runs in x-ray mode, with dithering on, and twice in
a row.  Deliberately not enumerated: alpha over Add, AddQuarter and Erase fronts beyond one strip each (the lerp sees only the blended
byte, and its domain is covered by the other three), and fronts that are no expanded 5-bit value (the path cannot produce them).

Sheets B8, the 8-bit path, Texture texels with their own blend byte: B8-modes, 256 x 1046, 1046 faces -- 256 x 1 textures (one texel per
column, r = t, g = t + 85, b = 255 - t), the back phase moving by 1 per row: 128 strips of 2 rows each for Average, Add, Subtract and
AddQuarter, two each for Opaque and Erase (skipped), every mode under alpha 0; B8-alpha, 256 x 1280, 1280 faces -- Opaque texels under alpha
1, 2, 127, 128, 254, 128 strips each, through the f32 lerp; B8-dither, 256 x 36 -- dithering on, 64 x 1 textures on strips of 4 rows.  Census
(CPU): all 786 432 (channel, mode, front byte, back byte), all 768 Opaque fronts, all 983 040 (channel, alpha, front byte, back byte), all
12 288 (channel, front byte, dither cell).  Every one of these three holds blending texels or an alpha below 255, so the library draws
it with the ordered walk of k_blend and never with the fused fill.  B8-opaque, 256 x 12, and B8-opaque-dither, 256 x 28, hold Opaque
texels, alpha 255 and one bound texture only and go through the fused fill (shade_tile_p64, k_cover_plain8): all 768 Opaque fronts,
`/ 128` up to 508 before the clamp, and all 12 288 (channel, front byte, dither cell) again.

This module only builds; what the tests compare is always the oracle's frame."""
import functools
from dataclasses import dataclass, field

import numpy as np

from bonnie32_amd import abi
from bonnie32_amd.rtypes import Camera, Color, IndexedTexture, RasterSettings, Texture, Texture15, make_faces, make_vertices
from oracle import np_model as M
from tests import coverage_sheets as CS

W = 256
MAX_ROWS = 1280
CLEAR = Color(20, 22, 28)
MODES = (abi.AVERAGE, abi.ADD, abi.SUBTRACT, abi.ADD_QUARTER, abi.ERASE)
ALPHAS = (0, 1, 2, 127, 128, 254)
S_VALUES = (0, 1, 127, 128, 129, 254, 255)
AMBIENTS = (0.0, 2.0 ** -10, 0.3, 0.5, 1.0, 1.5, 2.0, 3.0, -1.0)
ODD_AMBIENTS = (-0.0, float("inf"), float("nan"))
NONE, FLAT, GOURAUD = abi.SHADE_NONE, abi.SHADE_FLAT, abi.SHADE_GOURAUD


def tex_row_v(row, rows):
    """v coordinate of the middle of texture row `row` (Texture15::sample flips v: types.rs:671-681)"""
    return 1.0 - (row + 0.5) / rows


# ------------------------------------------------------------------------------------------------ the sheet
@dataclass
class Swatch:
    name: str
    height: int
    vertices: np.ndarray
    faces: np.ndarray
    textures: list                      # Texture15, or Texture on the 8-bit path
    strips: list                        # dict(y0, y1 (pixel rows, inclusive), kind, first face, + what the builder noted)
    fmt8: bool = False
    dithering: bool = True
    back: np.ndarray = None             # [H, W, 4] uploaded before the draw; None: cleared to CLEAR
    width: int = W
    _cache: dict = field(default_factory=dict)

    def settings(self, zbuffer=False, shading=NONE, ambient=0.3, xray=False, dithering=None):
        st = RasterSettings.benchmark()         # affine, fixed point, painter's, no lights
        st.backface_cull = False
        st.use_zbuffer = zbuffer
        st.use_rgb555 = not self.fmt8
        st.shading = shading
        st.ambient = ambient
        st.xray_mode = xray
        st.dithering = self.dithering if dithering is None else dithering
        return st

    def start_image(self):
        if self.back is not None:
            return self.back.copy()
        img = np.zeros((self.height, self.width, 4), np.uint8)
        img[...] = (CLEAR.r, CLEAR.g, CLEAR.b, 255)          # what Framebuffer::clear leaves (render.rs:27-45)
        return img

    def strip_of_row(self):
        own = np.full(self.height, -1, np.int64)
        for k, s in enumerate(self.strips):
            assert (own[s["y0"]:s["y1"] + 1] == -1).all(), f"{self.name}: strips overlap at rows {s['y0']}..{s['y1']}"
            own[s["y0"]:s["y1"] + 1] = k
        return own

    def diagonal(self):
        """[H, W] pixels that both triangles of their strip cover (the lattice points of the quad's diagonal inside the frame)"""
        if "diag" not in self._cache:
            d = np.zeros((self.height, self.width), bool)
            for s in self.strips:
                y0, y1 = s["y0"], s["y1"]
                ta = [(0, y0), (W, y0), (W, y1)]
                tb = [(0, y0), (W, y1), (0, y1)]
                d[y0:y1 + 1] |= CS.int_inside(ta, 0, y0, self.width, y1 + 1) & CS.int_inside(tb, 0, y0, self.width, y1 + 1)
            self._cache["diag"] = d
        return self._cache["diag"]

    # ---- the two restatements of the reference (CPU)
    def oracle(self, O, frames=1, **kw):
        """(pixels [H, W, 4], z-buffer bits [H * W], timings of the last frame) of the C oracle; cached per settings"""
        key = ("oracle", frames) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
        if key not in self._cache:
            fb = O.Framebuffer(self.width, self.height)
            fb.pixels[:] = self.start_image().reshape(-1)
            st = self.settings(**kw)
            for _ in range(frames):
                rc, tm = (O.render_mesh if self.fmt8 else O.render_mesh_15)(fb, self.vertices, self.faces, self.textures, Camera(), st)
                assert rc == 0
            px = fb.image().copy(); px.setflags(write=False)
            zb = fb.zbuffer.view(np.uint32).copy(); zb.setflags(write=False)
            self._cache[key] = (px, zb, tm)
        return self._cache[key]

    def model(self, **kw):
        """(pixels [H, W, 4], z-buffer bits, tap, result dict) of the numpy model with its per-pixel tap on; cached per settings"""
        key = ("model",) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
        if key not in self._cache:
            px = self.start_image().reshape(-1)
            zb = np.full(self.width * self.height, np.finfo(np.float32).max, np.float32)
            tap = []
            st = self.settings(**kw)
            with np.errstate(all="ignore"):
                if self.fmt8:
                    res = M.render_mesh(px, self.width, self.height, self.vertices, self.faces, self.textures, Camera(), st, zbuffer=zb, tap=tap)
                else:
                    res = M.render_mesh_15(px, self.width, self.height, self.vertices, self.faces, self.textures, Camera(), st, None, zb, tap=tap)
            px = px.reshape(self.height, self.width, 4); px.setflags(write=False)
            self._cache[key] = (px, zb.view(np.uint32), tap, res)
        return self._cache[key]

    def first_difference(self, got, want, what):
        g = np.asarray(got).reshape(self.height, self.width, -1)
        w = np.asarray(want).reshape(self.height, self.width, -1)
        bad = (g != w).any(axis=2)
        if not bad.any():
            return ""
        y, x = [int(v[0]) for v in np.nonzero(bad)]
        k = int(self.strip_of_row()[y])
        s = {a: b for a, b in self.strips[k].items() if a != "first"} if k >= 0 else "outside every strip"
        return f"[{self.name}: {what}] {int(bad.sum())} pixels differ, first at ({x}, {y}): got {g[y, x].tolist()}, oracle {w[y, x].tolist()}; strip {s}"


class _Builder:
    """Stacks full-width quads: TL (0, y0), TR (256, y0), BR (256, y1), BL (0, y1), split along TL-BR into (TL, TR, BR) and (TL, BR, BL).
    The fill covers the CLOSED triangle, so a quad between vertex rows y0 and y1 covers the pixel rows y0..y1: a strip of 4 pixel rows
    has y1 = y0 + 3; the lowest strip that is not degenerate has y1 = y0 + 1 and covers two pixel rows."""

    def __init__(self):
        self.y = 0
        self.quads = []

    def strip(self, rows, tex, colours, kind, u=(0.0, 1.0), v=0.5, blend=abi.OPAQUE, alpha=255, black_tr=1, **note):
        """colours: one (r, g, b) for a flat quad, or (left, right) for a sweep along x"""
        assert rows >= 2
        if np.ndim(colours[0]) == 0:
            colours = (colours, colours)
        self.quads.append(dict(y0=self.y, y1=self.y + rows - 1, tex=tex, left=tuple(colours[0]), right=tuple(colours[1]), u=u, v=v, blend=blend, alpha=alpha,
                               black_tr=black_tr, kind=kind, note=note))
        self.y += rows

    def finish(self, name, textures, fmt8=False, dithering=True, back=None):
        H = self.y
        assert H <= MAX_ROWS, (name, H)
        n = len(self.quads)
        sm = CS.ScreenMap(W, H)
        wx = sm.world([0, W], 0)
        ys = sorted({q[k] for q in self.quads for k in ("y0", "y1")})
        wy = dict(zip(ys, sm.world(ys, 1)))
        v = make_vertices(4 * n)
        f = make_faces(2 * n)
        strips = []
        for i, q in enumerate(self.quads):
            a = 4 * i
            for j, (xi, yk, side) in enumerate(((0, "y0", "left"), (1, "y0", "right"), (1, "y1", "right"), (0, "y1", "left"))):
                v["pos"][a + j] = (wx[xi], wy[q[yk]], CS.DEPTH)
                v["uv"][a + j] = (q["u"][xi], q["v"])
                v["r"][a + j], v["g"][a + j], v["b"][a + j] = q[side]
            f["v"][2 * i] = (a, a + 1, a + 2)
            f["v"][2 * i + 1] = (a, a + 2, a + 3)
            for k in (2 * i, 2 * i + 1):
                f["texture_id"][k] = abi.NO_TEXTURE if q["tex"] is None else q["tex"]
                f["blend_mode"][k], f["editor_alpha"][k], f["black_transparent"][k] = q["blend"], q["alpha"], q["black_tr"]
            strips.append(dict(y0=q["y0"], y1=q["y1"], kind=q["kind"], first=2 * i, tex=q["tex"], blend=q["blend"], alpha=q["alpha"], **q["note"]))
        v["normal"] = (0.0, 0.0, -1.0)
        v["blend"] = abi.OPAQUE
        if back is not None:
            assert back.shape == (H, W, 4)
        return Swatch(name, H, v, f, textures, strips, fmt8, dithering, back)


def check_placement(sw, res):
    """every vertex of the sheet landed on its integer target (the numpy model's projected coordinates)"""
    want_x = np.tile([0, W, W, 0], len(sw.strips))
    want_y = np.concatenate([[s["y0"], s["y0"], s["y1"], s["y1"]] for s in sw.strips])
    assert np.array_equal(res["sx"], want_x) and np.array_equal(res["sy"], want_y), f"{sw.name}: a vertex missed its target"


# ------------------------------------------------------------------------------------------------ textures
def _c15(r, g, b, stp=0):
    return (stp << 15) | (r << 10) | (g << 5) | b


def ramp15():
    """32 texels with another 5-bit value per channel each, every channel a bijection of 0..31, none 0x0000"""
    c = np.arange(32)
    px = _c15(c, (5 * c + 1) & 31, 31 - c)
    assert (px != 0).all() and all(len(set(((px >> s) & 31).tolist())) == 32 for s in (10, 5, 0))
    return px.astype(np.uint16)


def texture_p(blend=abi.OPAQUE, special=True):
    """32 x 3: row 0 the ramp, row 1 the ramp with bit 15 set, row 2 the texels with special meaning (0x0000, 0x8000, white, STP white)
    in turn.  (One row would do for the main strips; the extra rows keep every extra strip on the same single bound texture, so that
    the fused plain path draws them as well.)  special=False: 32 x 2, without row 2 -- no texel that the black_transparent rule can skip,
    which is what lets the library take CHEAP coverage when fragment counting is off (at most 1/64 skippable texels by default)."""
    r = ramp15()
    if not special:
        return Texture15(32, 2, np.concatenate([r, r | 0x8000]), blend, "swatch-ramp-plain")
    return Texture15(32, 3, np.concatenate([r, r | 0x8000, np.array([0x0000, 0x8000, 0x7FFF, 0xFFFF] * 8, np.uint16)]), blend, "swatch-ramp")


# u at the column centres: column x samples texel (x + 0.5) / 256 * width, never a texel boundary
U_CENTRED = (0.5 / W, 1.0 + 0.5 / W)


def _rot(v, k):
    return tuple(np.roll([v, (v + 85) & 255, (v + 170) & 255], k).tolist()) if k else (v, v, v)


# ------------------------------------------------------------------------------------------------ sheet P / S: the opaque pipeline
# Flat vertex colours v whose interpolation gives v - 1 somewhere on the third pixel row of a 4-row strip (barycentrics in thirds; on the
# other rows they are exact): bcx * v + bcy * v + bcz * v in f32 falls short of v there.  Found by the census of the sheet without the
# repair strips; the census of the sheet with them asserts that nothing is missing (tests/test_pixel_swatches.py).
REPAIR_VALUES = (15, 27, 30, 51, 54, 57, 60, 63, 99, 102, 105, 108, 111, 114, 117, 120, 123, 126, 195, 198, 201, 204, 207, 210, 213, 216, 219, 222, 225,
                 228, 231, 234, 237, 240, 243, 246, 249, 252, 255)


def _opaque_strips(b, values, full, special=True):
    v0, v1, v2 = (tex_row_v(r, 3 if special else 2) for r in range(3))
    for v in values:                                                    # the main part: textured, flat vertex colour v, 4 rows = 16 dither cells
        b.strip(4, 0, (v, v, v), "main", U_CENTRED, v0, value=v)
    for v in S_VALUES:                                                  # texels with bit 15 set
        b.strip(4, 0, (v, v, v), "stp", U_CENTRED, v1, value=v)
    for left, right in (((0, 255, 128), (255, 0, 127)), ((255, 255, 255), (0, 0, 0)), ((3, 130, 250), (4, 126, 255)), ((0, 0, 0), (255, 255, 255)),
                        ((128, 127, 129), (129, 128, 127))):
        b.strip(4, None, (left, right), "sweep-untextured")             # unequal vertex colours: dithered, vert sweeps through the interpolation
    b.strip(4, 0, ((0, 64, 255), (255, 190, 0)), "sweep-textured", U_CENTRED, v0)
    for v in (0, 1, 4, 63, 64, 65, 127, 128, 129, 254, 255):            # untextured, equal vertex colours: no dither although dithering is on
        b.strip(2, None, _rot(v, v % 3), "flat-untextured", value=v)
    if full:
        # 11 strips of two rows moved the stack by half a dither period: on these strips the third dither row is the strips' first row,
        # where the interpolation is exact
        assert b.y % 4 == 2
        for v in REPAIR_VALUES:
            b.strip(4, 0, (v, v, v), "main", U_CENTRED, v0, value=v)
    for black_tr in (1, 0) if special else ():                          # 0x0000 is skipped, or drawn as C15_BLACK_DRAWABLE; 0x8000 is black too
        for v in (128, 255):
            b.strip(2, 0, (v, v, v), "special", U_CENTRED, v2, black_tr=black_tr, value=v)


@functools.lru_cache(None)
def sheet_p(second=False, dithering=True, special=True):
    """second: one more bound texture and one strip that uses it (the fill's general shading path instead of the one-texture one);
    special=False ("-plain"): without the special texels and their strips (see texture_p)"""
    b = _Builder()
    _opaque_strips(b, range(256), True, special)
    textures = [texture_p(special=special)]
    if second:
        textures.append(Texture15(32, 1, ramp15()[::-1].copy(), abi.OPAQUE, "swatch-second"))
        b.strip(4, 1, (128, 200, 90), "second", U_CENTRED)
    return b.finish("P" + ("2" if second else "") + ("" if special else "-plain") + ("" if dithering else "-nodither"), textures, dithering=dithering)


def indexed_p():
    """texture_p as an indexed atlas: a CLUT of its distinct texels and one index per texel"""
    t = texture_p()
    clut, idx = np.unique(t.pixels, return_inverse=True)
    assert len(clut) <= 256
    clut = np.concatenate([clut, np.zeros(256 - len(clut), np.uint16)])
    it = IndexedTexture(t.width, t.height, idx.astype(np.uint8), clut, t.blend_mode)
    assert np.array_equal(it.to_texture15().pixels, t.pixels)
    return it


@functools.lru_cache(None)
def sheet_s(special=True):
    b = _Builder()
    _opaque_strips(b, S_VALUES, False, special)
    return b.finish("S" if special else "S-plain", [texture_p(special=special)])


# ------------------------------------------------------------------------------------------------ sheet B: the transparent store, RGB555
def back_image(height, step):
    """Every byte value per channel along x; the phase moves by `step` per row and differs per channel.  Arbitrary 8-bit values, not
    only expanded 5-bit ones (a clear colour or an editor-alpha store leaves such values)."""
    y, x = np.mgrid[0:height, 0:W]
    img = np.zeros((height, W, 4), np.uint8)
    img[..., 0] = (x + step * y) & 255
    img[..., 1] = (x + step * y + 85) & 255
    img[..., 2] = (x + step * y + 170) & 255
    img[..., 3] = 255
    return img


@functools.lru_cache(None)
def sheet_b():
    """Textures 0..4: the ramp texture with blend mode Average .. Erase; texture 5: the same, Opaque.  A front texel spans 8 columns, the
    back phase moves by 8 per row, so 16 strips of 2 rows put every back byte under every front texel."""
    b = _Builder()
    v_stp, v_plain, v_special = tex_row_v(1, 3), tex_row_v(0, 3), tex_row_v(2, 3)
    textures = [texture_p(m) for m in MODES] + [texture_p(abi.OPAQUE)]
    grey = (128, 128, 128)                                               # tex8 * 128 / 128: the front is the texel
    for t, mode in enumerate(MODES):
        for k in range(16):
            b.strip(2, t, grey, "stp", U_CENTRED, v_stp, mode=mode)
        b.strip(2, t, grey, "plain", U_CENTRED, v_plain, mode=mode)         # STP clear: stored, not blended
        b.strip(2, t, (3, 3, 3), "dark", U_CENTRED, v_plain, mode=mode)     # quantises to all-black: gets bit 15 and blends
        b.strip(2, t, grey, "special", U_CENTRED, v_special, mode=mode)     # 0x0000 skipped, 0x8000 black and skipped, white, STP white
        b.strip(2, t, grey, "special", U_CENTRED, v_special, mode=mode, black_tr=0)
    for mode in MODES:                                                   # the face's own mode counts on untextured faces only: white has no STP
        b.strip(2, None, ((0, 130, 255), (255, 120, 0)), "face-sweep", blend=mode, mode=mode)       # bit, so they blend where the colour is black
        b.strip(2, None, (2, 4, 1), "face-dark", blend=mode, mode=mode)
        b.strip(2, 5, grey, "face-textured", U_CENTRED, v_stp, blend=mode, mode=abi.OPAQUE)    # a textured face takes its texture's mode: no blend
    for alpha in ALPHAS:
        rows = 1 if alpha == 0 else 16
        for k in range(rows):
            b.strip(2, 5, grey, "alpha-plain", U_CENTRED, v_plain, alpha=alpha, mode=abi.OPAQUE)
        for t, mode in enumerate(MODES):
            if mode in (abi.AVERAGE, abi.SUBTRACT) or alpha == 0:
                for k in range(rows):
                    b.strip(2, t, grey, "alpha-stp", U_CENTRED, v_stp, alpha=alpha, mode=mode)
            else:
                b.strip(2, t, grey, "alpha-stp", U_CENTRED, v_stp, alpha=alpha, mode=mode)
        b.strip(2, None, ((0, 130, 255), (255, 120, 0)), "alpha-untextured", alpha=alpha, mode=abi.OPAQUE)
    return b.finish("B", textures, dithering=False, back=back_image(b.y, 8))


# ------------------------------------------------------------------------------------------------ sheet B8: the 8-bit path
def ramp8(n, blend):
    """n texels: r = t, g = t + 85, b = 255 - t (scaled to 0..255 for n < 256), with their own blend byte"""
    t = np.arange(n) * (256 // n)
    return np.stack([t, (t + 85) & 255, 255 - t, np.full(n, blend)], axis=1).astype(np.uint8)


OPAQUE_AND_MODES = (abi.OPAQUE,) + MODES


@functools.lru_cache(None)
def sheet_b8(part):
    """part "modes": Average, Add, Subtract, AddQuarter with front 0..255 against back 0..255 (a 256 x 1 texture, one texel per column; the
    back phase moves by 1 per row, so 128 strips of two rows put every back byte under every front byte), Opaque and Erase (skipped) on
    two strips each, every mode once more under alpha 0.  part "alpha": Opaque texels under every other alpha of the set, 128 strips each."""
    b = _Builder()
    grey = (128, 128, 128)
    if part == "modes":
        textures = [Texture(256, 1, ramp8(256, m), abi.OPAQUE, f"swatch8-{m}") for m in OPAQUE_AND_MODES]
        for t, m in enumerate(OPAQUE_AND_MODES):
            for k in range(128 if m in (abi.AVERAGE, abi.ADD, abi.SUBTRACT, abi.ADD_QUARTER) else 2):
                b.strip(2, t, grey, "mode", U_CENTRED, mode=m)
            b.strip(2, t, grey, "alpha", U_CENTRED, alpha=0, mode=m)
        b.strip(2, None, ((0, 130, 255), (255, 120, 0)), "untextured", mode=abi.OPAQUE)
    else:
        textures = [Texture(256, 1, ramp8(256, abi.OPAQUE), abi.OPAQUE, "swatch8-opaque")]
        for alpha in ALPHAS[1:]:
            for k in range(128):
                b.strip(2, 0, grey, "alpha", U_CENTRED, alpha=alpha, mode=abi.OPAQUE)
    return b.finish("B8-" + part, textures, fmt8=True, dithering=False, back=back_image(b.y, 1))


@functools.lru_cache(None)
def sheet_b8_dither():
    """The dithered part: a 64 x 1 texture (a texel spans 4 columns) on strips of 4 rows, so every texel meets the 16 dither cells; four
    textures whose ramps start at 0, 1, 2, 3 give every front byte; one strip each of Average and Add texels, and alpha 127."""
    b = _Builder()
    textures = []
    for k in range(4):
        px = ramp8(64, abi.OPAQUE).astype(np.int64)
        px[:, :3] = (px[:, :3] + k) & 255
        textures.append(Texture(64, 1, px.astype(np.uint8), abi.OPAQUE, f"swatch8-d{k}"))
        b.strip(4, k, (128, 128, 128), "dither", U_CENTRED, mode=abi.OPAQUE)
    for m in (abi.AVERAGE, abi.ADD):
        textures.append(Texture(64, 1, ramp8(64, m), abi.OPAQUE, f"swatch8-dm{m}"))
        b.strip(4, len(textures) - 1, (128, 128, 128), "dither-mode", U_CENTRED, mode=m)
    b.strip(4, 0, (255, 200, 129), "dither", U_CENTRED, mode=abi.OPAQUE)
    b.strip(4, 0, (128, 128, 128), "dither-alpha", U_CENTRED, alpha=127, mode=abi.OPAQUE)
    b.strip(4, None, ((0, 130, 255), (255, 120, 0)), "dither-untextured", mode=abi.OPAQUE)
    return b.finish("B8-dither", textures, fmt8=True, dithering=True, back=back_image(b.y, 7))


@functools.lru_cache(None)
def sheet_b8_opaque(dithering):
    """Opaque texels and alpha 255 only, ONE bound texture: nothing of the sheet blends, so the frame goes through the sort-free fused
    fill (shade8 from shade_tile_p64 / k_cover_plain8) and not through k_blend's ordered walk as every other B8 sheet does.  Dithering
    off: a 256 x 1 ramp under vertex colour 128 (every front byte per channel) and under (255, 200, 129) (the modulate's clamp).
    Dithering on: a 64 x 4 texture whose rows are ramps that start at 0, 1, 2, 3, one strip of 4 rows per texture row, so every front
    byte meets the 16 dither cells.  Untextured strips with unequal (dithered) and equal (never dithered) vertex colours in both."""
    b = _Builder()
    if dithering:
        px = np.concatenate([ramp8(64, abi.OPAQUE).astype(np.int64) + (k, k, k, 0) for k in range(4)])
        px[:, :3] &= 255
        textures = [Texture(64, 4, px.astype(np.uint8), abi.OPAQUE, "swatch8-opaque-d")]
        for k in range(4):
            b.strip(4, 0, (128, 128, 128), "dither", U_CENTRED, tex_row_v(k, 4), mode=abi.OPAQUE)
        b.strip(4, 0, (255, 200, 129), "bright", U_CENTRED, tex_row_v(0, 4), mode=abi.OPAQUE)
    else:
        textures = [Texture(256, 1, ramp8(256, abi.OPAQUE), abi.OPAQUE, "swatch8-opaque")]
        b.strip(2, 0, (128, 128, 128), "mode", U_CENTRED, mode=abi.OPAQUE)
        b.strip(2, 0, (255, 200, 129), "bright", U_CENTRED, mode=abi.OPAQUE)
    b.strip(4, None, ((0, 130, 255), (255, 120, 0)), "sweep-untextured", mode=abi.OPAQUE)
    b.strip(4, None, (200, 7, 131), "flat-untextured", mode=abi.OPAQUE)
    return b.finish("B8-opaque" + ("-dither" if dithering else ""), textures, fmt8=True, dithering=dithering, back=back_image(b.y, 7))


B8_SHEETS = {"B8-modes": lambda: sheet_b8("modes"), "B8-alpha": lambda: sheet_b8("alpha"), "B8-dither": sheet_b8_dither,
             "B8-opaque": lambda: sheet_b8_opaque(False), "B8-opaque-dither": lambda: sheet_b8_opaque(True)}
B8_BLENDING = ("B8-modes", "B8-alpha", "B8-dither")          # sheets with blending texels or alpha < 255: the ordered walk of k_blend
B8_OPAQUE = ("B8-opaque", "B8-opaque-dither")                # the fused fill


# ------------------------------------------------------------------------------------------------ the device side
def gpu_draw(ctx, sw, resident=False, textures=None, indexed=None, band=None, frames=1, **kw):
    """`frames` frames of the sheet through the C ABI, onto the uploaded back image (or the clear colour) -> (framebuffer object, timings)."""
    from bonnie32_amd import rasterizer as R
    st = sw.settings(**kw)
    fb = R.Framebuffer(sw.width, sw.height, ctx)
    if sw.back is not None:
        fb.upload(sw.back)
    else:
        fb.clear(CLEAR)
    if band:
        fb.set_band(*band)
    cam = Camera()
    if resident or indexed is not None or frames > 1:
        if sw.fmt8:
            rs = R.ResidentScene(fb, sw.vertices, sw.faces, textures8=sw.textures)
        elif indexed is not None:
            rs = R.ResidentScene(fb, sw.vertices, sw.faces, indexed_textures=indexed)
        else:
            rs = R.ResidentScene(fb, sw.vertices, sw.faces, sw.textures)
        if frames > 1:
            for _ in range(frames):
                rs.render_async(cam, st)
            tm = rs.finish()
        else:
            tm = rs.render(cam, st)
    elif sw.fmt8:
        tm = R.render_mesh(fb, sw.vertices, sw.faces, sw.textures, cam, st)
    else:
        tm = R.render_mesh_15(fb, sw.vertices, sw.faces, sw.textures, cam, st)
    return fb, tm
