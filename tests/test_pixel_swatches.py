"""The pixel pipeline value by value: modulate, shade, dither, quantise, blend, editor alpha (tests/pixel_swatches.py builds the sheets).

Which pixels a triangle covers and what k_setup hands to the fill are tested elsewhere; this file tests the value a covered pixel is
given: shade15 and its packed two-pixel form shade15_pair_rgba, store_blend / blend_rgb555 / c15_to_rgba, shade8 / store8 and
dither_offset (b32_fill_common.h, b32_device.h, b32_blend.hip).  They are integer functions of small domains, so the sheets enumerate the
domains: every covered pixel of a sheet is one chosen point.

CPU tests (no mark): the C oracle and the numpy model draw the same frame of every sheet; a third restatement of the stages, written
here in plain integers from the reference lines the kernels cite, reproduces every pixel the model stored from the model's per-pixel
tap; a census over that tap proves that the whole domain is in the reference's own frame; one-point mutations of the third restatement
each change a pixel of the sheet meant for them.  GPU tests: the library's frame of every sheet is the oracle's, bit for bit, on every
path that shades or stores.

Two of the one-point changes the sheets were asked to see cannot be seen by the frames they were meant for, and
test_mutations_that_no_frame_can_see proves it over the domain concerned instead of pretending otherwise:
  `>> 3` replaced by `/ 8` on a negative dither sum: the sum is at least 0 - 4, so the shift gives -1 where the division gives 0, and the
      clamp to 0..31 that follows (render.rs:1177, :1191) makes both 0.  The sheet does reach the difference before the clamp.  The
      change that does matter to the packed form, a logical instead of an arithmetic shift of the 16-bit sum, is checked in its place.
  `min(.., 255)` after `/ 128` replaced by 254, on the RGB555 path WITHOUT a shading pass (sheet P): 254 and 255 quantise alike under
      every dither offset and under `>> 3`.  With a shade factor between the clamp and the dither the two can part (at a shade of about
      0.97, 254 gives 246 and 255 gives 247, which dither apart at offset +1); no ambient of sheet S is such a factor, and the proof
      claims nothing about shaded frames.  On the 8-bit path the modulated byte is stored as it is, so sheet B8-modes sees that clamp;
      on sheet P the clamp that can be seen is the dither's own (30 for 31)."""
import numpy as np
import pytest

from bonnie32_amd import abi
from tests import pixel_swatches as PS

gpu = pytest.mark.gpu
f32 = np.float32
NONE, FLAT, GOURAUD = PS.NONE, PS.FLAT, PS.GOURAUD

# PS1_DITHER_MATRIX, render.rs:1150-1155
DITHER = np.array([[-4, 0, -3, 1], [2, -2, 3, -1], [-3, 1, -4, 0], [3, -1, 2, -2]], np.int64)


# ------------------------------------------------------------------------------------------------ the third restatement
def _expand5(v):                                            # expand_5_to_8, render.rs:1161-1163 (u8 arithmetic)
    return ((v << 3) | (v >> 2)) & 255


def _f_as_u8(x):                                            # `f32 as u8`: truncates, saturates, NaN -> 0
    with np.errstate(invalid="ignore"):
        t = np.where(np.isnan(x), 0.0, np.trunc(x.astype(np.float64)))
    return np.clip(t, 0, 255).astype(np.int64)


def _shaded(mod, shade, clamp):
    """render.rs:1643-1645 (`shade.clamp(0.0, 2.0)`: NaN stays NaN; `.min(255.0)` drops it) / :1074-1081 on the 8-bit path (no clamp)"""
    with np.errstate(all="ignore"):
        s = shade.astype(f32)
        if clamp:
            s = np.where(s < f32(0.0), f32(0.0), np.where(s > f32(2.0), f32(2.0), s)).astype(f32)
        return _f_as_u8(np.fmin((mod.astype(f32) * s).astype(f32), f32(255.0)))


def _quantise(m, x, y, dithered, mut):
    """dither_and_quantize, render.rs:1173-1182, or `>> 3`, :1653 -> (5-bit value, value before the clamp)"""
    if not dithered:
        return m >> 3, m >> 3
    total = m + DITHER[y & 3, x & 3]
    if "div8" in mut:
        pre = np.where(total < 0, -((-total) // 8), total // 8)
    elif "lshr16" in mut:
        pre = (total & 0xFFFF) >> 3
    else:
        pre = total >> 3
    return np.clip(pre, 0, 30 if "clamp30" in mut else 31), pre


def restate15(rec, xray=False, mut=()):
    """rasterize_triangle_15's colour pipeline and its store for the pixels of one tap record, render.rs:1613-1702"""
    texel, vert, x, y, back = rec["texel"], rec["vert"], rec["x"], rec["y"], rec["back"]
    q, raw, pre, m_all = [], [], [], []
    for i, sh in enumerate((10, 5, 0)):
        tex8 = _expand5((texel >> sh) & 31)                                 # :1613-1616
        r = (tex8 * vert[:, i]) // 128                                      # :1624-1626
        m = np.minimum(r, 254 if "clamp254" in mut else 255)
        if rec["shade"] is not None:
            m = _shaded(m, rec["shade"][:, i], True)
        qi, pi = _quantise(m, x, y, rec["dithered"], mut)
        q.append(qi); raw.append(r); pre.append(pi); m_all.append(m)
    q = np.stack(q, axis=1)
    all_black = (q == 0).all(axis=1)                                        # :1659-1661
    semi = (texel & 0x8000) != 0
    if "nobit15" not in mut:
        semi = semi | all_black
    front = _expand5(q)                                                     # Color15::r8 / g8 / b8
    mode, alpha = rec["blend"], rec["alpha"]
    do_blend = semi & (mode != abi.OPAQUE)
    if xray:                                                                # set_pixel_xray_15, render.rs:507-526
        res = (front + back) // 2
    else:
        f5, b5 = front >> 3, back >> 3                                      # blend_rgb555, render.rs:1093-1145
        if mode == abi.AVERAGE:
            r5 = np.minimum((b5 + f5) // 2, 31)
        elif mode == abi.ADD:
            r5 = np.minimum(b5 + f5, 31)
        elif mode == abi.SUBTRACT:
            r5 = np.maximum(b5 - f5, 0)
        elif mode == abi.ADD_QUARTER:
            r5 = np.minimum((b5 + f5) // 4 if "quarter" in mut else b5 + f5 // 4, 31)
        elif mode == abi.ERASE:
            r5 = b5
        else:
            r5 = f5
        ps1 = np.where(do_blend[:, None], r5 << 3, front)                   # set_pixel_blended_15, :479-502
        if alpha < 255:                                                     # set_pixel_with_editor_alpha_15, :567-591 (u16 arithmetic)
            total = ps1 * alpha + back * (255 - alpha)
            assert total.max() < 65536
            res = total >> 8 if "shr8" in mut else total // 255
        else:
            res = ps1
    return dict(res=res, q=q, raw=np.stack(raw, axis=1), pre=np.stack(pre, axis=1), m=np.stack(m_all, axis=1), do_blend=do_blend,
                semi_by_black=all_black & ((texel & 0x8000) == 0), alpha_byte=np.full(len(x), 255))


def restate8(rec, mut=()):
    """rasterize_triangle's colour pipeline and store, render.rs:1355-1387, :340-370, types.rs:801-808, :886-936"""
    texel, vert, x, y, back = rec["texel"], rec["vert"], rec["x"], rec["y"], rec["back"]
    cols, m_all = [], []
    for i in range(3):
        m = np.minimum((texel[:, i] * vert[:, i]) // 128, 254 if "clamp254" in mut else 255)              # modulate
        if rec["shade"] is not None:
            m = _shaded(m, rec["shade"][:, i], False)
        m_all.append(m)
        if rec["dithered"]:                                                 # apply_dither, render.rs:1186-1197
            m = np.clip((m + DITHER[y & 3, x & 3]) >> 3, 0, 31) << 3
        cols.append(m)
    f = np.stack(cols, axis=1)
    mode = texel[:, 3][:, None]
    assert (mode != abi.ERASE).all(), "an Erase texel was stored"
    ps1 = np.select([mode == abi.AVERAGE, mode == abi.ADD, mode == abi.SUBTRACT, mode == abi.ADD_QUARTER],
                    [(back + f) // 2, np.minimum(back + f, 255), np.maximum(back - f, 0), np.minimum(back + f // 4, 255)], f)
    if rec["alpha"] < 255:                                                  # render.rs:356-366, in f32
        a = f32(rec["alpha"]) / f32(255.0)
        inv_a = f32(1.0) - a
        res = _f_as_u8(((ps1.astype(f32) * a).astype(f32) + (back.astype(f32) * inv_a).astype(f32)).astype(f32))
    else:
        res = ps1
    return dict(res=res, front=f, m=np.stack(m_all, axis=1), ps1=ps1, alpha_byte=np.full(len(x), 255))


def replay(sw, tap, xray=False, mut=(), check=True):
    """The frame the third restatement gives: every tap record in draw order, from the tapped inputs."""
    img = sw.start_image().astype(np.int64)
    for rec in tap:
        out = restate8(rec, mut) if sw.fmt8 else restate15(rec, xray, mut)
        if check:
            assert np.array_equal(img[rec["y"], rec["x"], :3], rec["back"]), f"{sw.name}: face {rec['face']} read another back than the replay holds"
            assert np.array_equal(out["m"], rec["m"]), f"{sw.name}: face {rec['face']}: the values before the dither differ"
        img[rec["y"], rec["x"], :3] = out["res"]
        img[rec["y"], rec["x"], 3] = out["alpha_byte"]
    return img.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the sheets and their variants
def _sheet(name):
    if name == "P":
        return PS.sheet_p()
    if name == "P-nodither":
        return PS.sheet_p(dithering=False)
    if name == "P2":
        return PS.sheet_p(second=True)
    if name == "S":
        return PS.sheet_s()
    if name == "P-plain":
        return PS.sheet_p(special=False)
    if name == "P-plain-nodither":
        return PS.sheet_p(special=False, dithering=False)
    if name == "S-plain":
        return PS.sheet_s(special=False)
    if name == "B":
        return PS.sheet_b()
    return PS.B8_SHEETS[name]()


SHEETS = ["P", "P-nodither", "P2", "P-plain", "P-plain-nodither", "B"] + list(PS.B8_SHEETS)
S_CASES = [(sh, a) for sh in (FLAT, GOURAUD) for a in PS.AMBIENTS + PS.ODD_AMBIENTS]
_ambient_id = lambda c: f"{'flat' if c[0] == FLAT else 'gouraud'}-{c[1]!r}"


def _agree(sw, oracle, what, **kw):
    """three-way agreement: C oracle == numpy model == the replay of the third restatement"""
    opx, ozb, otm = sw.oracle(oracle, **kw)
    mpx, mzb, tap, res = sw.model(**kw)
    PS.check_placement(sw, res)
    msg = sw.first_difference(mpx, opx, f"{what}: numpy model against the C oracle")
    assert not msg, msg
    assert np.array_equal(mzb, ozb)
    assert res["triangles_drawn"] == otm.triangles_drawn == len(sw.faces) and res["fragments"] == otm.fragments
    msg = sw.first_difference(replay(sw, tap, xray=kw.get("xray", False)), mpx, f"{what}: third restatement against the numpy model")
    assert not msg, msg
    return tap


# ------------------------------------------------------------------------------------------------ CPU: agreement
@pytest.mark.parametrize("name", SHEETS)
def test_three_restatements_agree(oracle, name):
    sw = _sheet(name)
    tap = _agree(sw, oracle, "painter's")
    stored = sum(len(r["x"]) for r in tap)
    print(f"{sw.name}: {sw.width} x {sw.height}, {len(sw.faces)} faces, {stored} stored pixels, {int(sw.diagonal().sum())} diagonal pixels")
    assert sw.width <= 256 and sw.height <= PS.MAX_ROWS


@pytest.mark.parametrize("name", ["P", "B", "B8-modes"])
def test_three_restatements_agree_in_zbuffer_mode(oracle, name):
    _agree(_sheet(name), oracle, "z-buffer", zbuffer=True)


def test_three_restatements_agree_on_xray_and_dithered_blends(oracle):
    _agree(PS.sheet_b(), oracle, "x-ray", xray=True)
    _agree(PS.sheet_b(), oracle, "dithered", dithering=True)


@pytest.mark.parametrize("case", S_CASES, ids=_ambient_id)
def test_three_restatements_agree_on_the_shade_factor(oracle, case):
    """Sheet S: no lights, so every shade is min(ambient, 1.0) (render.rs:1013-1071); -0.0, +inf and NaN are part of the cases because the
    two restatements do agree on them (this test is the check the sheet's docstring refers to)."""
    shading, ambient = case
    tap = _agree(PS.sheet_s(), oracle, f"shading {shading} ambient {ambient!r}", shading=shading, ambient=ambient)
    assert all(r["shade"] is not None for r in tap)
    _agree(PS.sheet_s(special=False), oracle, f"S-plain shading {shading} ambient {ambient!r}", shading=shading, ambient=ambient)


# ------------------------------------------------------------------------------------------------ CPU: the census
def _census_pixels(sw, tap, kinds):
    """(record, strip) of every tap record whose strip is of one of `kinds`.  Every stored pixel counts, none is left out: a diagonal
    pixel is stored by both triangles of its quad, and the tap holds the back each of the two stores really read, so the second one
    counts as the second application that it is."""
    strip = sw.strip_of_row()
    for rec in tap:
        s = sw.strips[int(strip[rec["y"][0]])]
        if s["kind"] in kinds:
            yield rec, s


@pytest.mark.parametrize("name", SHEETS + ["S"])
def test_only_diagonal_pixels_are_stored_twice(name):
    """the pixels with a second application are the lattice points of the quads' diagonals, at most 2 % of what is stored (the census
    leaves nothing out: see _census_pixels)"""
    sw = _sheet(name)
    px, zb, tap, res = sw.model() if name != "S" else sw.model(shading=FLAT, ambient=0.5)
    stored = np.zeros((sw.height, sw.width), np.int64)
    for rec in tap:
        np.add.at(stored, (rec["y"], rec["x"]), 1)
    assert np.array_equal(stored > 1, sw.diagonal() & (stored > 0)), "pixels stored twice are not the diagonals"
    assert (stored <= 2).all()
    share = int((stored > 1).sum()) / int((stored > 0).sum())
    print(f"{sw.name}: {int((stored > 1).sum())} of {int((stored > 0).sum())} stored pixels on a diagonal ({100 * share:.3f} %)")
    assert share <= 0.02


@pytest.mark.parametrize("special", [True, False], ids=["P", "P-plain"])
def test_census_sheet_p(special):
    """Every (c5, vert, dither cell) per channel -- 32 x 256 x 16 -- is a pixel of the reference's frame, with the byte `vert` that was
    actually interpolated; without dither every (c5, vert).  The modulate's `/ 128` exceeds 255 before its clamp and the dither's
    `>> 3` leaves 0..31 on both sides before its clamp.  The same holds for the sheet without the special texels."""
    sw = PS.sheet_p(special=special)
    tap = sw.model()[2]
    seen = np.zeros((3, 32, 256, 16), bool)
    raw_max, pre_min, pre_max = 0, 0, 0
    for rec, s in _census_pixels(sw, tap, ("main",)):
        assert rec["dithered"]
        out = restate15(rec)
        cell = ((rec["y"] & 3) * 4 + (rec["x"] & 3))
        for i, sh in enumerate((10, 5, 0)):
            seen[i, ((rec["texel"] >> sh) & 31), rec["vert"][:, i], cell] = True
        raw_max = max(raw_max, int(out["raw"].max())); pre_min = min(pre_min, int(out["pre"].min())); pre_max = max(pre_max, int(out["pre"].max()))
    print(f"{sw.name}: {int(seen.sum())} of {seen.size} (channel, c5, vert, cell); / 128 up to {raw_max}; dither sum >> 3 from {pre_min} to {pre_max}")
    assert seen.all(), f"{int((~seen).sum())} missing, first {np.argwhere(~seen)[:4].tolist()}"
    assert raw_max > 255 and pre_min < 0 and pre_max > 31
    # all 16 cells carry the matrix's own value (every value of -4..3 twice)
    assert sorted(DITHER.reshape(-1).tolist()) == sorted(list(range(-4, 4)) * 2)
    # dithering off: every (c5, vert)
    sw = PS.sheet_p(dithering=False, special=special)
    seen = np.zeros((3, 32, 256), bool)
    for rec, s in _census_pixels(sw, sw.model()[2], ("main",)):
        assert not rec["dithered"]
        for i, sh in enumerate((10, 5, 0)):
            seen[i, ((rec["texel"] >> sh) & 31), rec["vert"][:, i]] = True
    print(f"{sw.name}: {int(seen.sum())} of {seen.size} (channel, c5, vert)")
    assert seen.all()


def test_census_sheet_p_extras():
    """untextured faces with equal vertex colours do not dither although dithering is on, those with unequal ones do and sweep `vert`
    through every byte; texels with bit 15 are drawn like the others; 0x0000 is skipped, or drawn as black with black_transparent off"""
    sw = PS.sheet_p()
    px, zb, tap, res = sw.model()
    kinds = {}
    for rec, s in _census_pixels(sw, tap, ("flat-untextured", "sweep-untextured", "stp", "special")):
        kinds.setdefault(s["kind"], []).append((rec, s))
    assert all(not r["dithered"] for r, s in kinds["flat-untextured"]) and all(r["dithered"] for r, s in kinds["sweep-untextured"])
    swept = np.zeros((3, 256), bool)
    for r, s in kinds["sweep-untextured"]:
        for i in range(3):
            swept[i, r["vert"][:, i]] = True
    assert swept.all()
    assert all(((r["texel"] & 0x8000) != 0).all() for r, s in kinds["stp"])
    drawable = [r for r, s in kinds["special"] if (r["texel"] == 0x8000).any()]
    assert drawable and all(((r["texel"] & 0x7FFF) != 0).all() for r, s in kinds["special"] if sw.faces["black_transparent"][s["first"]])
    clear = np.array([PS.CLEAR.r, PS.CLEAR.g, PS.CLEAR.b, 255])
    for s in sw.strips:
        if s["kind"] == "special":
            rows = px[s["y0"]:s["y1"] + 1]
            left_clear = int((rows == clear).all(axis=2).sum())
            assert left_clear == (rows.shape[0] * 128 if sw.faces["black_transparent"][s["first"]] else 0), (s, left_clear)


def test_census_sheet_b():
    """Every (front5, back byte, mode) per channel is blended; every (front5, back byte, alpha) is lerped from a front that does not
    blend, and from Average and Subtract results; a non-STP texel that quantises to all-black gets bit 15 and blends, in every mode,
    over every back byte; alpha 0 stores nothing."""
    sw = PS.sheet_b()
    px, zb, tap, res = sw.model()
    blended = np.zeros((3, len(PS.MODES), 32, 256), bool)
    black = np.zeros((len(PS.MODES), 256), bool)
    lerped = np.zeros((3, len(PS.ALPHAS), 3, 32, 256), bool)             # [.., plain / Average / Subtract, ..]
    unblended = 0
    for rec, s in _census_pixels(sw, tap, ("stp", "dark", "plain", "alpha-plain", "alpha-stp")):
        assert rec["alpha"] == s["alpha"] and rec["blend"] == s["mode"] and rec["alpha"] > 0 and not rec["dithered"]
        out = restate15(rec)
        q, back, on = out["q"], rec["back"], out["do_blend"]
        if s["kind"] in ("stp", "dark"):
            assert on.all()
            mi = PS.MODES.index(s["mode"])
            for i in range(3):
                blended[i, mi, q[:, i], back[:, i]] = True
            if s["kind"] == "dark":
                assert out["semi_by_black"].all() and (q == 0).all()
                black[mi, back[:, 0]] = True
        elif s["kind"] == "plain":
            assert not on.any()
            unblended += len(rec["x"])
        else:
            which = 0 if s["kind"] == "alpha-plain" else {abi.AVERAGE: 1, abi.SUBTRACT: 2}.get(s["mode"])
            assert on.all() == (s["kind"] == "alpha-stp") and on.any() == (s["kind"] == "alpha-stp")
            if which is not None:
                for i in range(3):
                    lerped[i, PS.ALPHAS.index(s["alpha"]), which, q[:, i], back[:, i]] = True
    print(f"B: {int(blended.sum())} of {blended.size} (channel, mode, front5, back) blended; {int(black.sum())} of {black.size} (mode, back) by the all-black rule; "
          f"{int(lerped[:, 1:].sum())} of {lerped[:, 1:].size} (channel, alpha, plain / Average / Subtract, front5, back) lerped; {unblended} non-STP pixels stored unblended")
    assert blended.all() and black.all() and lerped[:, 1:].all() and not lerped[:, 0].any() and unblended > 0
    for s in sw.strips:                                                   # alpha 0: the strip's rows still hold the back image
        if s["alpha"] == 0:
            assert np.array_equal(px[s["y0"]:s["y1"] + 1], sw.back[s["y0"]:s["y1"] + 1])
    assert not np.array_equal((sw.back[..., :3] >> 3) << 3 | (sw.back[..., :3] >> 5), sw.back[..., :3]), "the back image holds expanded 5-bit values only"


def test_census_sheet_b8():
    """Every (front byte, back byte, mode) per channel for Average, Add, Subtract and AddQuarter; every front byte under Opaque; no Erase
    texel is stored; every (front byte, back byte, alpha) through the f32 lerp; every (front byte, dither cell) on the dithered part."""
    sw = PS.sheet_b8("modes")
    px, zb, tap, res = sw.model()
    four = (abi.AVERAGE, abi.ADD, abi.SUBTRACT, abi.ADD_QUARTER)
    seen = np.zeros((3, 4, 256, 256), bool)
    opaque = np.zeros((3, 256), bool)
    for rec, s in _census_pixels(sw, tap, ("mode",)):
        out = restate8(rec)
        f, back = out["front"], rec["back"]
        assert (rec["texel"][:, 3] == s["mode"]).all() and s["mode"] != abi.ERASE
        for i in range(3):
            if s["mode"] == abi.OPAQUE:
                opaque[i, f[:, i]] = True
            else:
                seen[i, four.index(s["mode"]), f[:, i], back[:, i]] = True
    print(f"B8-modes: {int(seen.sum())} of {seen.size} (channel, mode, front, back); {int(opaque.sum())} of {opaque.size} Opaque fronts")
    assert seen.all() and opaque.all()
    for s in sw.strips:
        if s["alpha"] == 0 or s["mode"] == abi.ERASE:
            assert np.array_equal(px[s["y0"]:s["y1"] + 1], sw.back[s["y0"]:s["y1"] + 1]), s
    sw = PS.sheet_b8("alpha")
    lerped = np.zeros((3, len(PS.ALPHAS), 256, 256), bool)
    for rec, s in _census_pixels(sw, sw.model()[2], ("alpha",)):
        out = restate8(rec)
        for i in range(3):
            lerped[i, PS.ALPHAS.index(rec["alpha"]), out["ps1"][:, i], rec["back"][:, i]] = True
    print(f"B8-alpha: {int(lerped[:, 1:].sum())} of {lerped[:, 1:].size} (channel, alpha, front, back)")
    assert lerped[:, 1:].all()
    sw = PS.sheet_b8_dither()
    cells = np.zeros((3, 256, 16), bool)
    for rec, s in _census_pixels(sw, sw.model()[2], ("dither",)):
        assert rec["dithered"]
        cell = ((rec["y"] & 3) * 4 + (rec["x"] & 3))
        for i in range(3):
            cells[i, rec["m"][:, i], cell] = True
    print(f"B8-dither: {int(cells.sum())} of {cells.size} (channel, front, cell)")
    assert cells.all()
    # the sheets of Opaque texels alone (the fused fill instead of the ordered walk): the same two domains
    sw = PS.sheet_b8_opaque(False)
    opaque = np.zeros((3, 256), bool)
    top = 0
    for rec, s in _census_pixels(sw, sw.model()[2], ("mode", "bright")):
        assert not rec["dithered"] and rec["alpha"] == 255 and (rec["texel"][:, 3] == abi.OPAQUE).all()
        if s["kind"] == "mode":
            for i in range(3):
                opaque[i, rec["m"][:, i]] = True
        top = max(top, int(((rec["texel"][:, :3] * rec["vert"]) // 128).max()))
    sw = PS.sheet_b8_opaque(True)
    cells = np.zeros((3, 256, 16), bool)
    for rec, s in _census_pixels(sw, sw.model()[2], ("dither",)):
        assert rec["dithered"] and rec["alpha"] == 255 and (rec["texel"][:, 3] == abi.OPAQUE).all()
        cell = ((rec["y"] & 3) * 4 + (rec["x"] & 3))
        for i in range(3):
            cells[i, rec["m"][:, i], cell] = True
    print(f"B8-opaque: {int(opaque.sum())} of {opaque.size} Opaque fronts, / 128 up to {top}; B8-opaque-dither: {int(cells.sum())} of {cells.size} (channel, front, cell)")
    assert opaque.all() and cells.all() and top > 255
    for name in PS.B8_OPAQUE:
        sw = _sheet(name)
        assert len(sw.textures) == 1 and (sw.faces["editor_alpha"] == 255).all() and all((t.pixels[:, 3] == abi.OPAQUE).all() for t in sw.textures)


def test_gouraud_shade_is_not_the_flat_one():
    """why sheet S runs Gouraud as well: the interpolated shade bcx * s + bcy * s + bcz * s falls short of s at some pixels, and the
    truncation then gives another byte than the flat shade does"""
    sw = PS.sheet_s()
    flat, gouraud = sw.model(shading=FLAT, ambient=1.0)[0], sw.model(shading=GOURAUD, ambient=1.0)[0]
    n = int((flat != gouraud).any(axis=2).sum())
    print(f"S: {n} pixels differ between flat and Gouraud at ambient 1.0")
    assert n > 0


# ------------------------------------------------------------------------------------------------ CPU: the sheets see the errors they are for
@pytest.mark.parametrize("name,mut,kw", [("B8-modes", "clamp254", {}), ("P", "clamp30", {}), ("P", "lshr16", {}), ("B", "quarter", {}), ("B", "shr8", {}), ("B", "nobit15", {}),
                                         ("B", "nobit15", {"dithering": True})])
def test_one_point_mutations_change_the_sheet(name, mut, kw):
    sw = _sheet(name)
    px, zb, tap, res = sw.model(**kw)
    n = int((replay(sw, tap, mut=(mut,), check=False) != px).any(axis=2).sum())
    print(f"{sw.name}: mutation {mut} changes {n} pixels")
    assert n > 0


def test_mutations_that_no_frame_can_see():
    """`>> 3` -> `/ 8` on the negative dither sum changes the value before the clamp at pixels of sheet P, and no stored value anywhere
    in the domain; a modulate clamp of 254 changes no 5-bit value either as long as no shading pass comes between the clamp and the
    dither, which is sheet P's case (see the module docstring; a shade factor of about 0.97 would show it)."""
    sw = PS.sheet_p()
    px, zb, tap, res = sw.model()
    changed = sum(int((restate15(rec, mut=("div8",))["pre"] != restate15(rec)["pre"]).sum()) for rec in tap if rec["dithered"])
    print(f"P: `/ 8` changes {changed} values before the clamp")
    assert changed > 0
    m, off = np.meshgrid(np.arange(256), np.arange(-4, 4))
    total = m + off
    assert np.array_equal(np.clip(total >> 3, 0, 31), np.clip(np.where(total < 0, -((-total) // 8), total // 8), 0, 31))
    assert np.array_equal(replay(sw, tap, mut=("div8",), check=False), px)
    for o in list(range(-4, 4)):
        assert min(max((254 + o) >> 3, 0), 31) == min(max((255 + o) >> 3, 0), 31)
    assert 254 >> 3 == 255 >> 3
    assert np.array_equal(replay(sw, tap, mut=("clamp254",), check=False), px)


# ------------------------------------------------------------------------------------------------ GPU: bit for bit on every path
def _same(sw, got, want, what):
    msg = sw.first_difference(got, want, what)
    assert not msg, msg


def _draws(gpu_ctx, sw, oracle, what, countings=(1, 0), residents=(False, True), check_z=False, **kw):
    want, wantz, etm = sw.oracle(oracle, **kw)
    for counting in countings:
        gpu_ctx.set_fragment_counting(counting)
        for resident in residents:
            fb, tm = PS.gpu_draw(gpu_ctx, sw, resident=resident, **kw)
            tag = f"{what} counting={counting} resident={resident}"
            _same(sw, fb.pixels, want, tag)
            if check_z:
                _same(sw, fb.zbuffer.view(np.uint32), wantz, tag + " depths")
            assert tm.triangles_drawn == etm.triangles_drawn
            if counting and not kw.get("zbuffer") and not sw.fmt8:
                assert tm.fragments == etm.fragments, tag


@gpu
@pytest.mark.parametrize("name", ["P", "P-nodither"])
def test_sheet_p_with_one_texture(gpu_ctx, oracle, name):
    """painter's mode, one texture, shading None, default routes: the tile lists are collected inside the fill, whose general
    instantiation picks the one-texture shading (shade_tile_plain, shade15_pair_rgba) at run time; the special texels make coverage
    EXACT with counting on and off.  The kernels of the one-texture frames proper: test_plain_sheet_p_on_the_one_texture_kernels.
    Fragment counting on and off, resident and immediate."""
    try:
        _draws(gpu_ctx, _sheet(name), oracle, "plain")
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", ["P", "P-nodither"])
def test_sheet_p_in_zbuffer_mode(gpu_ctx, oracle, name):
    try:
        _draws(gpu_ctx, _sheet(name), oracle, "z-buffer", check_z=True, zbuffer=True)
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
def test_sheet_p_with_a_second_texture(gpu_ctx, oracle):
    """two bound textures: the general shade_tile_p64 with shade15<true> instead of the one-texture form"""
    try:
        _draws(gpu_ctx, PS.sheet_p(second=True), oracle, "two textures")
        _draws(gpu_ctx, PS.sheet_p(second=True), oracle, "two textures, z-buffer", check_z=True, zbuffer=True)
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
def test_sheet_p_from_an_indexed_atlas(gpu_ctx, oracle):
    """ResidentScene(indexed_textures=...): the CLUT lookup in LDS gives the same texels"""
    sw = PS.sheet_p()
    want, _, etm = sw.oracle(oracle)
    try:
        for counting in (1, 0):
            gpu_ctx.set_fragment_counting(counting)
            fb, tm = PS.gpu_draw(gpu_ctx, sw, indexed=[PS.indexed_p()])
            _same(sw, fb.pixels, want, f"indexed counting={counting}")
            assert tm.triangles_drawn == etm.triangles_drawn
    finally:
        gpu_ctx.set_fragment_counting(1)


def _routed(gpu_ctx, sw, oracle, off, what, counting=0, advanced=(), still=(), check_z=False, **kw):
    """One resident draw with the routes of `off` switched off (b32_set_routes): the frame is the oracle's, the route counters named in
    `advanced` moved and those in `still` did not (b32_route_count).  The caller restores routes and counting."""
    want, wantz, etm = sw.oracle(oracle, **kw)
    gpu_ctx.set_fragment_counting(counting)
    gpu_ctx.set_routes(off)
    before = gpu_ctx.route_counts()
    fb, tm = PS.gpu_draw(gpu_ctx, sw, resident=True, **kw)
    after = gpu_ctx.route_counts()
    tag = f"{what} routes off: {off} counting={counting}"
    _same(sw, fb.pixels, want, tag)
    if check_z:
        _same(sw, fb.zbuffer.view(np.uint32), wantz, tag + " depths")
    assert tm.triangles_drawn == etm.triangles_drawn
    moved = sorted(k for k in after if after[k] != before[k])
    for k in advanced:
        assert after[k] > before[k], (tag, k, moved)
    for k in still:
        assert after[k] == before[k], (tag, k, moved)


BIN_ROUTES = ("direct_bin", "inline_bin", "counting_sort", "keyed")


def _only(route):
    return dict(advanced=(route,), still=tuple(r for r in BIN_ROUTES if r != route))


@gpu
def test_sheet_p_on_every_route(gpu_ctx, oracle):
    """the masks of test_sheet_on_every_route plus the counting-sort launches, and which way the tile lists were made each time: a
    resident mesh of 646 faces collects them inside the fill unless told otherwise"""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    sw = PS.sheet_p()
    try:
        for off, route in ((0, "inline_bin"), (C.ROUTE_SPAN_COVER, "inline_bin"), (C.ROUTE_DIRECT_BIN, "inline_bin"), (C.ROUTE_INLINE_BIN, "direct_bin"),
                           (C.ROUTE_CUT_TILES, "inline_bin"), (C.ROUTE_WIDE_GROUPS, "inline_bin"), (C.ROUTE_DIRECT_BIN | C.ROUTE_INLINE_BIN, "counting_sort"),
                           (C.ROUTE_SORT_FREE, "keyed")):
            _routed(gpu_ctx, sw, oracle, off, "P", **_only(route))
    finally:
        gpu_ctx.set_routes(0)
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", ["P-plain", "P-plain-nodither"])
def test_plain_sheet_p_on_the_one_texture_kernels(gpu_ctx, oracle, name):
    """The fused fill has kernels of its own for frames of ONE texture without a shading pass whose tile lists were NOT collected inside
    the fill (launch_p64, b32_fill.hip: `plain`): k_cover_plain -- the kernel the benchmark times -- in painter's mode with CHEAP coverage,
    k_cover_plain_z in z-buffer mode, the EXACT instantiation with fragment counting on.  CHEAP coverage needs a texture with (almost) no
    skippable texel, so this is sheet P without its special texels; in-fill collection and the 16-wave workgroups are switched off, and
    the route counters show that the setup kernel binned.  (Which kernel ran is not observable; the conditions are those of launch_p64.)"""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    sw = _sheet(name)
    assert all(((t.pixels & 0x7FFF) != 0).all() for t in sw.textures) and len(sw.textures) == 1
    try:
        for counting in (0, 1):
            for zbuffer in (False, True):
                _routed(gpu_ctx, sw, oracle, C.ROUTE_INLINE_BIN | C.ROUTE_WIDE_GROUPS, name, counting=counting, check_z=zbuffer, zbuffer=zbuffer, **_only("direct_bin"))
        _draws(gpu_ctx, sw, oracle, "default routes")
    finally:
        gpu_ctx.set_routes(0)
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("shading", [FLAT, GOURAUD], ids=["flat", "gouraud"])
def test_plain_sheet_s_on_the_lit_kernel(gpu_ctx, oracle, shading):
    """k_cover_lit: one texture, a shading pass, z-buffer mode, CHEAP coverage, tile lists binned by the setup kernel, 8-wave workgroups
    (launch_p64: `lit_plain`); painter's mode beside it"""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    sw = PS.sheet_s(special=False)
    try:
        for ambient in PS.AMBIENTS + PS.ODD_AMBIENTS:
            for zbuffer in (True, False):
                _routed(gpu_ctx, sw, oracle, C.ROUTE_INLINE_BIN | C.ROUTE_WIDE_GROUPS, f"S-plain ambient {ambient!r}", check_z=zbuffer, zbuffer=zbuffer, shading=shading,
                        ambient=ambient, **_only("direct_bin"))
    finally:
        gpu_ctx.set_routes(0)
        gpu_ctx.set_fragment_counting(1)


@gpu
def test_sheet_p_in_two_ragged_row_bands(gpu_ctx, oracle):
    """bands (0, 301) and (301, H), neither a multiple of a tile's rows nor of a strip's: the two partial frames assemble to the oracle's"""
    sw = PS.sheet_p()
    want, _, etm = sw.oracle(oracle)
    row = sw.width * 4
    try:
        for counting in (0, 1):
            gpu_ctx.set_fragment_counting(counting)
            assembled = np.zeros(sw.width * sw.height * 4, np.uint8)
            for y0, y1 in ((0, 301), (301, sw.height)):
                fb, tm = PS.gpu_draw(gpu_ctx, sw, resident=True, band=(y0, y1))
                assembled[y0 * row:y1 * row] = fb.pixels[y0 * row:y1 * row]
            _same(sw, assembled, want, f"bands counting={counting}")
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("shading", [FLAT, GOURAUD], ids=["flat", "gouraud"])
def test_sheet_s_at_every_ambient(gpu_ctx, oracle, shading):
    """the rclamp / rmin / f2u8_sat line of shade15<true>: painter's and z-buffer mode, resident and immediate, counting off (the lit
    plain path) and on"""
    sw = PS.sheet_s()
    try:
        for ambient in PS.AMBIENTS + PS.ODD_AMBIENTS:
            _draws(gpu_ctx, sw, oracle, f"ambient {ambient!r}", shading=shading, ambient=ambient)
            _draws(gpu_ctx, sw, oracle, f"z-buffer ambient {ambient!r}", countings=(0,), check_z=True, shading=shading, ambient=ambient, zbuffer=True)
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("zbuffer", [False, True], ids=["painter", "zbuffer"])
def test_sheet_b(gpu_ctx, oracle, zbuffer):
    """store_blend through k_blend: counting on and off, resident and immediate; in z-buffer mode the transparent pass writes no depth,
    and every face of the sheet is in it, so the z-buffer stays as new"""
    sw = PS.sheet_b()
    try:
        _draws(gpu_ctx, sw, oracle, "blend", check_z=True, zbuffer=zbuffer)
        assert (sw.oracle(oracle, zbuffer=zbuffer)[1] == np.float32(np.finfo(np.float32).max).view(np.uint32)).all()
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
def test_sheet_b_xray_and_dithered(gpu_ctx, oracle):
    sw = PS.sheet_b()
    try:
        _draws(gpu_ctx, sw, oracle, "x-ray", xray=True)
        _draws(gpu_ctx, sw, oracle, "x-ray z-buffer", countings=(0,), xray=True, zbuffer=True)
        _draws(gpu_ctx, sw, oracle, "dithered", dithering=True)
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
def test_sheet_b_with_two_frames_in_flight(gpu_ctx, oracle):
    """two frames enqueued back to back onto one framebuffer, then one finish: every pixel is blended twice, in order"""
    sw = PS.sheet_b()
    want, _, etm = sw.oracle(oracle, frames=2)
    try:
        for counting in (0, 1):
            gpu_ctx.set_fragment_counting(counting)
            fb, tm = PS.gpu_draw(gpu_ctx, sw, resident=True, frames=2)
            _same(sw, fb.pixels, want, f"two frames counting={counting}")
            assert tm.triangles_drawn == etm.triangles_drawn
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", PS.B8_BLENDING)
def test_sheet_b8(gpu_ctx, oracle, name):
    """shade8 / store8 in the ordered walk of k_blend: a sheet with blending texels or an editor alpha below 255 has no overwrite pass, its
    frames take the keyed pipeline whatever routes are on.  Fragment counting on and off, z-buffer mode on and off, resident and immediate."""
    sw = _sheet(name)
    try:
        for zbuffer in (False, True):
            before = gpu_ctx.route_counts()
            _draws(gpu_ctx, sw, oracle, "8-bit", check_z=zbuffer, zbuffer=zbuffer)
            after = gpu_ctx.route_counts()
            assert after["keyed"] > before["keyed"] and all(after[r] == before[r] for r in BIN_ROUTES if r != "keyed"), (before, after)
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", PS.B8_OPAQUE)
def test_sheet_b8_opaque_in_the_fused_fill(gpu_ctx, oracle, name):
    """shade8 from the fused fill (shade_tile_p64<FMT8>; k_cover_plain8 when the setup kernel binned, coverage is CHEAP and the workgroups
    have 8 waves), its dither included: tile lists collected in the fill, binned by the setup kernel, and made by the counting-sort
    launches, each shown by its route counter; fragment counting on and off, z-buffer mode on and off, then immediate draws."""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    sw = _sheet(name)
    try:
        for off, route in ((0, "inline_bin"), (C.ROUTE_INLINE_BIN, "direct_bin"), (C.ROUTE_INLINE_BIN | C.ROUTE_WIDE_GROUPS, "direct_bin"),
                           (C.ROUTE_DIRECT_BIN | C.ROUTE_INLINE_BIN, "counting_sort"), (C.ROUTE_DIRECT_BIN | C.ROUTE_INLINE_BIN | C.ROUTE_WIDE_GROUPS, "counting_sort")):
            for counting in (0, 1):
                for zbuffer in (False, True):
                    _routed(gpu_ctx, sw, oracle, off, name, counting=counting, check_z=zbuffer, zbuffer=zbuffer, **_only(route))
        gpu_ctx.set_routes(0)
        _draws(gpu_ctx, sw, oracle, "8-bit immediate", residents=(False,))
    finally:
        gpu_ctx.set_routes(0)
        gpu_ctx.set_fragment_counting(1)
