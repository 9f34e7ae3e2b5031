"""Texel sheets: frames in which every covered pixel reports WHICH TEXEL it fetched, so that a frame comparison checks texture addressing
-- interpolation of u and v, the `1.0 - v` flip, the wrap, the clamp to the last texel, the row stride -- texel by texel
(tests/test_texel_sheets.py).  The sheets reuse the swatch plumbing of tests/pixel_swatches.py (the oracle, the model, gpu_draw).

Identity textures.  A texel's value is its own address.  On the RGB555 path it is code n = ty * width + tx + 977 * texture id (mod 21 952)
written in base 28 into the three 5-bit channels as 4 + digit: never 0x0000, never black, bit 15 clear.  Neighbours in x differ by 1 and
neighbours in y by `width` (mod 21 952, never 0 for the sizes used), also in the textures with more texels than codes.  Faces have
vertex colour 128, dithering is off and shading None, so the pipeline behind the fetch is tex8 * vert / 128, `>> 3` and the expansion to
bytes.  The issue expected `vert` to be 128 everywhere and proposed all 15 bits as the code; but the interpolated byte
bcx * 128 + bcy * 128 + bcz * 128 is 127 at many pixels of a quad whose area has an inexact reciprocal, and tex8 * 127 / 128 takes a channel
of 1, 2 or 3 down by one -- two neighbouring texels would show the same pixel.  Channels of 4..31 survive both 127 and 128 unchanged
(test_the_frame_is_a_map_of_texels), so the frame is an injective map of fetched addresses and TexelSheet.decode turns a pixel back into
the code for a failure message.  The 8-bit path stores the modulated byte itself, which is the texel's byte less 0, 1 or 2: there the code
n = linear index + 70 001 * id is written in base 64 as bytes 4 * digit + 3, and byte >> 2 survives (18 bits instead of the issue's 24).

Geometry.  Frames are 256 wide and at most 1280 high.  A strip is a quad on exact integer screen positions (coverage_sheets.ScreenMap, one
map per camera depth), split along TL-BR into two triangles; a strip of 2 pixel rows has y1 = y0 + 1, so the doubled area of its
triangles is the quad's width.  Widths: 256 (a power of two: the reciprocal of the area is exact) and 128 on 3 rows (the same area,
inset), and 200, 231, 240, 248, 250, 255, where it is not.  Every quad narrower than the frame is inset from the left edge by 1 to 3
pixels, so both of its vertex columns are drawn; a quad of width 256 cannot be inset on a frame of 256 columns (the issue's limit) and
runs from column 0 to the vertex column 256 just outside.  Along x one coordinate sweeps a span while the other is held at the middle
of a texel row / column or at a chosen edge value; "both" strips sweep both, "tall" strips sweep v along y over 9 rows.  The strips
take four vertex orders in turn (VERTEX_ORDERS): which corner is v1, v2, v3 decides how the interpolation associates, and a clockwise
face has two vertices and their uv swapped by the setup.

Spans per texture size (_spans): [0, 1] and [-1, 0] on a quad whose width is a multiple of the texture's width (height for v), so
that pixels sit exactly on texel boundaries; [-2, 2], [-3, 3]; [0, 1], [-1, 0] and [-2, 2] offset by half a texel.  The same in v.
Constant strips (CONSTANTS) hold one coordinate at +0.0, -0.0, a denormal, -1e-9 (its wrap is exactly 1.0: only the clamp keeps the fetch
inside), 1.0, the f32 neighbours of 0 and 1, 2^23 +- 1, 1e6, -1e6, 1e9, +-inf and NaN while the other sweeps [0, 1].  "far" strips
sweep one unit at 1e6, -1e6 and 2^23 - 1.

Sheets (sizes in SIZES_*):
  A        affine, 15 bound textures (13 sizes, a zero-width and a zero-height one, which sample transparent) and untextured strips
  A-plain  sheet A's strips on ONE texture without a skippable texel (the one-texture kernels, the LDS-staged texture)
  K        identity textures whose odd texels are 0x0000 / 0x8000 in turn (a checkerboard), each strip with black_transparent on and
           again with it off, over a backing layer of flat untextured quads at a greater depth: what shows through is decided by the
           coverage phase's address (a bit of the skip mask), what is drawn by the shading phase's.  The first textures are 3 x 5 and
           7 x 7, so every later one starts at a pool offset that is no multiple of 32 and mask words straddle textures.
  Z        perspective-correct: the left and right edge of a quad at different depths, ratios of z 1:1, 1:2, 1:16 and an edge at camera
           depth 0.125, just behind the near plane (0.1)
  Z-plain  the same on one texture
  F        a subset of A and Z for the float and the orthographic projection: the vertices are no integers there, the surfaces carry
           F_SLOW, and the barycentrics come from the accumulated walk.  (The orthographic projection mirrors the rows.)
  A8       sheet A's subset on the 8-bit path, Opaque texels (fused fill) or Average texels over an uploaded back (ordered walk)
  T        RGB555 textures that carry blend mode Average, half of their texels with bit 15, over an uploaded back (k_blend)
  I        one indexed texture of at most 16 x 16 with a CLUT of 256 distinct colours

This module only builds; what the tests compare is always the oracle's frame."""
import functools
from dataclasses import dataclass

import numpy as np

from bonnie32_amd import abi
from bonnie32_amd.rtypes import IndexedTexture, Texture, Texture15, make_faces, make_vertices
from tests import coverage_sheets as CS
from tests import pixel_swatches as PS

f32 = np.float32
W = PS.W
MAX_ROWS = PS.MAX_ROWS
GREY = (128, 128, 128)
BACKING = (200, 100, 50)
Z_BACKING = 300.0
MESH_DISTANCE = 5.0                                     # screen z = camera depth + 5 (render.rs:2344); the depths below are screen z

SIZES_A = ((1, 1), (2, 2), (1, 64), (64, 1), (3, 5), (7, 7), (30, 30), (31, 33), (32, 32), (33, 31), (100, 60), (255, 255), (256, 256))
SIZES_K = ((3, 5), (7, 7), (31, 33), (32, 32), (100, 60))
SIZES_Z = ((1, 1), (3, 5), (7, 7), (31, 33), (32, 32), (100, 60), (256, 256))
SIZES_F = ((3, 5), (31, 33), (32, 32), (100, 60), (255, 255))
SIZES_8 = ((1, 1), (3, 5), (7, 7), (31, 33), (32, 32), (100, 60), (255, 255))
DEPTH_PAIRS = ((100.0, 100.0), (100.0, 200.0), (10.0, 160.0), (5.125, 105.0))       # screen z of the left and the right edge

_up = lambda x: float(np.nextafter(f32(x), f32(np.inf)))
_down = lambda x: float(np.nextafter(f32(x), f32(-np.inf)))
CONSTANTS = (("+0", 0.0), ("-0", -0.0), ("denormal", 1e-40), ("-1e-9", -1e-9), ("1", 1.0), ("0+", _up(0.0)), ("0-", _down(0.0)), ("1-", _down(1.0)),
             ("1+", _up(1.0)), ("2^23-1", 8388607.0), ("2^23+1", 8388609.0), ("1e6", 1e6), ("-1e6", -1e6), ("1e9", 1e9), ("+inf", float("inf")),
             ("-inf", float("-inf")), ("nan", float("nan")))
FAR = (("1e6", 1e6, 1e6 + 1), ("-1e6", -1e6, -1e6 + 1), ("2^23", 8388607.0, 8388609.0))
WIDTHS = (256, 255, 250, 248, 240, 231, 200)
OTHER_WIDTHS = (250, 255, 231, 240, 256)


def width_for(n):
    """the widest quad width of the set that is a multiple of n: its pixels sit exactly on the boundaries of n texels over a unit span"""
    return next(w for w in WIDTHS if w % n == 0)


# ------------------------------------------------------------------------------------------------ textures
CODES15 = 28 ** 3                                       # codes of an RGB555 identity texel: three channels of 4..31
CODES8 = 64 ** 3                                        # codes of an 8-bit identity texel: three bytes 4 k + 3


def code15(n):
    """code n (mod 21 952) as a Color15 whose channels are all 4..31: see the module docstring"""
    n = np.asarray(n) % CODES15
    return (4 + n // 784) << 10 | (4 + (n // 28) % 28) << 5 | (4 + n % 28)


def identity15(w, h, tid, blend=abi.OPAQUE, checker=False, stp=False):
    y, x = np.mgrid[0:h, 0:w]
    px = code15(y * w + x + 977 * tid)
    if stp:
        px = np.where((x + y) % 2 == 1, px | 0x8000, px)
    if checker:                                             # odd texels: 0x0000 and 0x8000 in turn
        px = np.where((x + y) % 2 == 1, np.where(((x + y) // 2) % 2 == 0, 0x0000, 0x8000), px)
    return Texture15(w, h, px.astype(np.uint16).reshape(-1), blend, f"identity-{w}x{h}")


def identity8(w, h, tid, blend):
    y, x = np.mgrid[0:h, 0:w]
    c = ((y * w + x + 70001 * tid) % CODES8).reshape(-1)
    px = np.stack([4 * (c & 63) + 3, 4 * ((c >> 6) & 63) + 3, 4 * ((c >> 12) & 63) + 3, np.full(c.shape, blend)], axis=1).astype(np.uint8)
    return Texture(w, h, px, abi.OPAQUE, f"identity8-{w}x{h}")


def identity_indexed(w, h):
    clut = code15(np.arange(256) * 85 + 3).astype(np.uint16)
    assert len(set(clut.tolist())) == 256
    y, x = np.mgrid[0:h, 0:w]
    return IndexedTexture(w, h, ((y * w + x) % 256).astype(np.uint8).reshape(-1), clut, abi.OPAQUE)


# ------------------------------------------------------------------------------------------------ the sheet
@dataclass
class TexelSheet(PS.Swatch):
    affine: bool = True
    indexed: list = None                                    # sheet I: the IndexedTexture list the device is given

    def settings(self, affine=None, projection="fixed", **kw):
        st = super().settings(**kw)
        st.affine_textures = self.affine if affine is None else affine
        if projection == "float":
            st.use_fixed_point = False
        elif projection == "ortho":                         # x = cam x * zoom + W / 2, y = -cam y * zoom + H / 2 (math.rs:140-148): mirrored rows
            st.ortho_projection = (1.0 / CS.ScreenMap(self.width, self.height, CS.DEPTH).per_px, 0.0, 0.0)
        else:
            assert projection == "fixed"
        return st

    def decode(self, px):
        """the code n of the identity texel a pixel of a frame shows (RGB555: channels 4 + digit of n in base 28; 8-bit path: byte >> 2 is
        a digit in base 64); n is the texel's linear index + 977 * texture id (8-bit path: + 70 001 * id)"""
        p = [int(v) for v in px[:3]]
        if self.fmt8:
            return p[0] >> 2 | (p[1] >> 2) << 6 | (p[2] >> 2) << 12
        return ((p[0] >> 3) - 4) * 784 + ((p[1] >> 3) - 4) * 28 + (p[2] >> 3) - 4

    def first_difference(self, got, want, what):
        msg = super().first_difference(got, want, what)
        if msg:
            g = np.asarray(got).reshape(self.height, self.width, -1)
            w = np.asarray(want).reshape(self.height, self.width, -1)
            y, x = [int(v[0]) for v in np.nonzero((g != w).any(axis=2))]
            if g.shape[2] == 4:
                msg += f"; texel code got {self.decode(g[y, x])}, oracle {self.decode(w[y, x])} (linear index + id offset)"
        return msg


# the two triangles of a quad TL, TR, BR, BL (corners 0..3), always split along TL-BR: as listed, rotated, clockwise, clockwise rotated
VERTEX_ORDERS = (((0, 1, 2), (0, 2, 3)), ((1, 2, 0), (2, 3, 0)), ((0, 2, 1), (0, 3, 2)), ((2, 0, 1), (3, 0, 2)))


class _Builder:
    def __init__(self, fmt8=False):
        self.y = 0
        self.quads = []
        self.fmt8 = fmt8

    def strip(self, rows, qw, tex, kind, u=(0.0, 0.0), v=(0.5, 0.5), vy=None, z=(CS.DEPTH, CS.DEPTH), black_tr=1, colour=GREY, backing=False, **note):
        """u, v: (left, right) along x; vy: (top, bottom), v along y instead; z: screen z of the left and the right edge"""
        assert rows >= 2 and qw <= W
        x0 = 0 if qw == W else 1 + len(self.quads) % 3 if qw + 3 < W else W - 1 - qw
        q = dict(y0=self.y, y1=self.y + rows - 1, x0=x0, x1=x0 + qw, tex=tex, kind=kind, u=u, v=v, vy=vy, z=z, black_tr=black_tr, colour=colour, note=note)
        if backing:
            self.quads.append(dict(q, tex=None, kind="backing", z=(Z_BACKING, Z_BACKING), colour=BACKING, x0=0, x1=W, backs=True))
        self.quads.append(q)
        self.y += rows

    def finish(self, name, textures, affine=True, back=None, indexed=None):
        H = self.y
        assert H <= MAX_ROWS, (name, H)
        n = len(self.quads)
        maps = {}
        def world(t, axis, z):
            if z not in maps:
                maps[z] = CS.ScreenMap(W, H, z - MESH_DISTANCE)
            return float(maps[z].world([t], axis)[0])
        for z in sorted({z for q in self.quads for z in q["z"]}):          # one batch of solves per depth
            maps[z] = CS.ScreenMap(W, H, z - MESH_DISTANCE)
            for axis, keys in ((0, ("x0", "x1")), (1, ("y0", "y1"))):
                maps[z].world(sorted({q[k] for q in self.quads if z in q["z"] for k in keys}), axis)
        v = make_vertices(4 * n)
        f = make_faces(2 * n)
        strips = []
        for i, q in enumerate(self.quads):
            a = 4 * i
            for j, (xi, yi) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
                z = q["z"][xi]
                v["pos"][a + j] = (world(q[("x0", "x1")[xi]], 0, z), world(q[("y0", "y1")[yi]], 1, z), z - MESH_DISTANCE)
                v["uv"][a + j] = (q["u"][xi], q["v"][xi] if q["vy"] is None else q["vy"][yi])
                v["r"][a + j], v["g"][a + j], v["b"][a + j] = q["colour"]
            # which corner is v1, v2, v3 decides the association of (bcx c1 + bcy c2) + bcz c3, and a clockwise face has its second and
            # third vertex (and their uv) swapped by the setup: the strips take the four orders in turn
            order = 0 if q.get("backs") else len(strips) % 4
            first, second = VERTEX_ORDERS[order]
            f["v"][2 * i] = [a + c for c in first]
            f["v"][2 * i + 1] = [a + c for c in second]
            for k in (2 * i, 2 * i + 1):
                f["texture_id"][k] = abi.NO_TEXTURE if q["tex"] is None else q["tex"]
                f["blend_mode"][k], f["editor_alpha"][k], f["black_transparent"][k] = abi.OPAQUE, 255, q["black_tr"]
            if not q.get("backs"):
                strips.append(dict(y0=q["y0"], y1=q["y1"], x0=q["x0"], x1=q["x1"], kind=q["kind"], first=2 * i, tex=q["tex"], u=q["u"], v=q["v"], vy=q["vy"],
                                   z=q["z"], black_tr=q["black_tr"], blend=abi.OPAQUE, alpha=255, order=order, **q["note"]))
        v["normal"] = (0.0, 0.0, -1.0)
        v["blend"] = abi.OPAQUE
        if back is not None:
            back = PS.back_image(H, back)
        return TexelSheet(name, H, v, f, textures, strips, self.fmt8, False, back, W, affine=affine, indexed=indexed)


def check_placement(sw, res):
    """every vertex of the sheet landed on its integer target (the numpy model's projected coordinates); backing quads span the frame"""
    quads = {s["first"] // 2: s for s in sw.strips}
    for i in range(len(sw.faces) // 2):
        s = quads.get(i)
        sx, sy = res["sx"][4 * i:4 * i + 4], res["sy"][4 * i:4 * i + 4]
        if s is None:
            s = quads[i + 1]
            want_x = [0, W, W, 0]
        else:
            want_x = [s["x0"], s["x1"], s["x1"], s["x0"]]
        assert sx.tolist() == want_x and sy.tolist() == [s["y0"], s["y0"], s["y1"], s["y1"]], f"{sw.name}: quad {i} missed its target: {sx.tolist()} {sy.tolist()} {s}"


# ------------------------------------------------------------------------------------------------ strips
def mid(k, n):
    """the coordinate of the middle of texel k of n (in v this is row n - 1 - k after the flip)"""
    return (k + 0.5) / n


def _spans(n):
    h = 0.5 / n
    unit = width_for(n)
    return (("unit", unit, (0.0, 1.0)), ("neg-unit", unit, (-1.0, 0.0)), ("pm2", 250, (-2.0, 2.0)), ("pm3", 255 if n % 2 else 231, (-3.0, 3.0)),
            ("unit-half", 240, (h, 1.0 + h)), ("neg-unit-half", unit, (h - 1.0, h)), ("pm2-half", 256, (h - 2.0, h + 2.0)))


def _sweeps(b, tex, tw, th, spans=None, k=0, **kw):
    """the strips of one texture: every span in u with v at a row's middle, every span in v with u at a column's middle, both at once,
    a quad of the power-of-two area that is inset, and a tall strip with v along y"""
    for name, qw, span in _spans(tw):
        if spans is None or name in spans:
            b.strip(2, qw, tex, "sweep-u", u=span, v=(mid(k % th, th),) * 2, size=(tw, th), span=name, **kw)
            k += 1
    for name, qw, span in _spans(th):
        if spans is None or name in spans:
            b.strip(2, qw, tex, "sweep-v", u=(mid(k % tw, tw),) * 2, v=span, size=(tw, th), span=name, **kw)
            k += 1
    b.strip(2, OTHER_WIDTHS[k % 5], tex, "sweep-both", u=(-1.0, 2.0), v=(1.5, -0.5), size=(tw, th), span="both", **kw)
    if spans is None:
        b.strip(3, 128, tex, "sweep-u", u=(0.0, 1.0), v=(mid(0, th),) * 2, size=(tw, th), span="unit-128", **kw)
        b.strip(9, 250, tex, "tall", u=(-1.0, 1.0), vy=(1.0, 0.0), size=(tw, th), span="tall", **kw)


def _constants(b, tex, tw, th, names=None, **kw):
    for name, c in CONSTANTS:
        if names is None or name in names:
            b.strip(2, width_for(th), tex, "const-u", u=(c, c), v=(0.0, 1.0), size=(tw, th), const=name, **kw)
            b.strip(2, width_for(tw), tex, "const-v", u=(0.0, 1.0), v=(c, c), size=(tw, th), const=name, **kw)


def _far(b, tex, tw, th, **kw):
    for name, lo, hi in FAR:
        b.strip(2, 256, tex, "far-u", u=(lo, hi), v=(mid(0, th),) * 2, size=(tw, th), far=name, **kw)
        b.strip(2, 256, tex, "far-v", u=(mid(0, tw),) * 2, v=(lo, hi), size=(tw, th), far=name, **kw)


SHORT_SPANS = ("unit", "neg-unit", "pm3", "unit-half")
SHORT_CONSTANTS = ("-0", "-1e-9", "1", "1-", "2^23+1", "-1e6", "+inf", "nan")


@functools.lru_cache(None)
def sheet_a(single=None):
    """single: (tw, th) -- "A-plain", every strip on one texture"""
    b = _Builder()
    sizes = SIZES_A if single is None else (single,)
    textures = [identity15(w, h, t) for t, (w, h) in enumerate(sizes)]
    for t, (w, h) in enumerate(sizes):
        _sweeps(b, t, w, h, None if single or (w, h) in ((31, 33), (100, 60), (255, 255)) else ("unit", "neg-unit", "pm2", "pm3", "unit-half", "neg-unit-half"), k=t)
    for t, (w, h) in enumerate(sizes):
        if single or (w, h) in ((32, 32), (31, 33)):
            _constants(b, t, w, h)
        if single or (w, h) in ((64, 1), (1, 64), (100, 60)):
            _far(b, t, w, h)
        if (w, h) == (100, 60):                             # 100 texels over [-3, 3] on 250 pixels, once per vertex order
            for k in range(4):
                b.strip(2, 250, t, "sweep-u", u=(-3.0, 3.0), v=(mid(k, h),) * 2, size=(w, h), span="pm3-250")
    if single is None:
        textures += [Texture15(0, 5, np.zeros(0, np.uint16), abi.OPAQUE, "zero-width"), Texture15(5, 0, np.zeros(0, np.uint16), abi.OPAQUE, "zero-height")]
        for t in (len(sizes), len(sizes) + 1):
            b.strip(2, 250, t, "zero-size", u=(-1.0, 1.0), v=(0.25, 0.75), size=(0, 0))
        b.strip(2, 250, None, "untextured", u=(-1.0, 1.0), v=(0.25, 0.75), colour=(90, 160, 230))
        b.strip(2, 256, None, "untextured", u=(float("nan"),) * 2, v=(float("inf"),) * 2, colour=(90, 160, 230))
    return b.finish("A" if single is None else f"A-plain-{single[0]}x{single[1]}", textures)


@functools.lru_cache(None)
def sheet_k():
    b = _Builder()
    textures = [identity15(w, h, t, checker=True) for t, (w, h) in enumerate(SIZES_K)]
    for t, (w, h) in enumerate(SIZES_K):
        for black_tr in (1, 0):
            _sweeps(b, t, w, h, ("unit", "neg-unit", "pm2", "pm3", "unit-half", "neg-unit-half", "pm2-half"), k=t, black_tr=black_tr, backing=True)
            _constants(b, t, w, h, ("-1e-9", "1", "1-", "nan") if (w, h) in ((3, 5), (32, 32)) else (), black_tr=black_tr, backing=True)
    return b.finish("K", textures)


@functools.lru_cache(None)
def sheet_z(single=None):
    b = _Builder()
    sizes = SIZES_Z if single is None else (single,)
    textures = [identity15(w, h, t) for t, (w, h) in enumerate(sizes)]
    for z in DEPTH_PAIRS:
        for t, (w, h) in enumerate(sizes):
            _sweeps(b, t, w, h, SHORT_SPANS if single is None else ("unit", "neg-unit", "pm2", "pm3", "unit-half", "pm2-half"), k=t, z=z)
            if single or (w, h) == (32, 32):
                _constants(b, t, w, h, SHORT_CONSTANTS, z=z)
    return b.finish("Z" if single is None else f"Z-plain-{single[0]}x{single[1]}", textures, affine=False)


@functools.lru_cache(None)
def sheet_f(affine):
    """the literal replay: sheet A's (affine) or sheet Z's (perspective-correct) strips, cut down, for the float and orthographic projection"""
    b = _Builder()
    textures = [identity15(w, h, t) for t, (w, h) in enumerate(SIZES_F)]
    for z in ((100.0, 100.0),) if affine else DEPTH_PAIRS[1:]:
        for t, (w, h) in enumerate(SIZES_F):
            _sweeps(b, t, w, h, SHORT_SPANS, k=t, z=z)
        _constants(b, 2, 32, 32, SHORT_CONSTANTS, z=z)
    return b.finish("F-affine" if affine else "F-perspective", textures, affine=affine)


@functools.lru_cache(None)
def sheet_a8(blend):
    """blend: the blend byte of every texel -- Opaque: one frame of the fused fill; Average: the ordered walk of k_blend, over a back"""
    b = _Builder(fmt8=True)
    textures = [identity8(w, h, t, blend) for t, (w, h) in enumerate(SIZES_8)]
    for t, (w, h) in enumerate(SIZES_8):
        _sweeps(b, t, w, h, ("unit", "neg-unit", "pm2", "pm3", "unit-half", "neg-unit-half"), k=t)
    _constants(b, 4, 32, 32)
    _constants(b, 3, 31, 33, SHORT_CONSTANTS)
    _far(b, 5, 100, 60)
    textures += [Texture(0, 5, np.zeros((0, 4), np.uint8), abi.OPAQUE, "zero-width"), Texture(5, 0, np.zeros((0, 4), np.uint8), abi.OPAQUE, "zero-height")]
    for t in (len(SIZES_8), len(SIZES_8) + 1):
        b.strip(2, 250, t, "zero-size", u=(-1.0, 1.0), v=(0.25, 0.75), size=(0, 0))
    b.strip(2, 250, None, "untextured", u=(-1.0, 1.0), v=(0.25, 0.75), colour=(90, 160, 230))
    return b.finish("A8-opaque" if blend == abi.OPAQUE else "A8-blend", textures, back=None if blend == abi.OPAQUE else 3)


@functools.lru_cache(None)
def sheet_t():
    """RGB555 textures that carry blend mode Average; texels with x + y odd have bit 15 and blend with the uploaded back, the others are
    stored: every face is in the transparent pass"""
    b = _Builder()
    textures = [identity15(w, h, t, blend=abi.AVERAGE, stp=True) for t, (w, h) in enumerate(SIZES_K)]
    for t, (w, h) in enumerate(SIZES_K):
        _sweeps(b, t, w, h, ("unit", "neg-unit", "pm2", "pm3", "unit-half", "neg-unit-half"), k=t)
    _constants(b, 3, 32, 32, SHORT_CONSTANTS)
    return b.finish("T", textures, back=5)


@functools.lru_cache(None)
def sheet_i(w, h):
    b = _Builder()
    it = identity_indexed(w, h)
    _sweeps(b, 0, w, h)
    _constants(b, 0, w, h)
    _far(b, 0, w, h)
    return b.finish(f"I-{w}x{h}", [it.to_texture15()], indexed=[it])


PLAIN_SIZES = ((31, 33), (100, 60), (255, 255))             # 255 x 255 x 2 bytes does not fit the LDS stage: the same kernels from global memory
INDEXED_SIZES = ((16, 16), (7, 5))
SHEETS = {"A": sheet_a, "K": sheet_k, "Z": sheet_z, "F-affine": lambda: sheet_f(True), "F-perspective": lambda: sheet_f(False),
          "A8-opaque": lambda: sheet_a8(abi.OPAQUE), "A8-blend": lambda: sheet_a8(abi.AVERAGE), "T": sheet_t}
for _s in PLAIN_SIZES:
    SHEETS[f"A-plain-{_s[0]}x{_s[1]}"] = functools.partial(sheet_a, _s)
for _s in PLAIN_SIZES[:2]:
    SHEETS[f"Z-plain-{_s[0]}x{_s[1]}"] = functools.partial(sheet_z, _s)
for _s in INDEXED_SIZES:
    SHEETS[f"I-{_s[0]}x{_s[1]}"] = functools.partial(sheet_i, *_s)
