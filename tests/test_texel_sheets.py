"""Texture addressing texel by texel: wrap, flip, clamp, perspective (tests/texel_sheets.py builds the sheets).

Which pixels a triangle covers and what value a fetched texel becomes are tested elsewhere (test_coverage_sheets.py,
test_pixel_swatches.py); this file tests the stage between them, WHICH texel a fragment fetches: the interpolation of u and v
(render.rs:1565-1579), the `1.0 - v` flip and Texture15::sample / Texture::sample (types.rs:671-681, :1242-1253).  The device states that
arithmetic once, in interp_uv and texel_index (b32_fill_common.h), and reaches it through texel_address (texel_drawn, the EXACT trips
and their skip mask in b32_cover.h, k_blend), hit_prepare, texaddr (b32_shade_tile.h) and atlas_texel.  Every texel of a sheet's
textures carries its own address, so the frame is a map of fetched addresses.

CPU tests (no mark): every strip lands on its rows and the C oracle equals the numpy model on every sheet and setting; a restatement of
the address arithmetic, written once below, reproduces the model's tx / ty / texel at every stored pixel from the model's tap; a census
over that tap shows that the cases the sheets were built for are in the reference's own frame; one-point mutations of the restatement
each change a pixel of a named sheet.  GPU tests: the library's frame of every sheet is the oracle's, bit for bit, on every route and
kernel form that addresses texels.

One case the sheets were asked for cannot occur, and test_cases_that_no_frame_can_reach proves it instead of dropping it:
  the wrap returning exactly 1.0 in v: the wrap's argument is the f32 difference 1.0 - v.  It returns 1.0 only for an argument r with
      -2^-25 <= r < 0 (r + 1.0 rounds to 1.0).  For v <= 2 the difference 1.0 - v is exact (Sterbenz), so it is 0 or at least the spacing
      of v in magnitude: 2^-23 for v in (1, 2].  For larger v it is at least 1 in magnitude, and its remainder is 0 or a multiple
      of the spacing of v, 2^-22 or more.  So the clamp to th - 1 never decides in v; in u it does (strip const -1e-9)."""
from fractions import Fraction

import numpy as np
import pytest

from bonnie32_amd import abi
from oracle import np_model as M
from tests import test_pixel_swatches as TP
from tests import texel_sheets as TS

gpu = pytest.mark.gpu
f32 = np.float32
f64 = np.float64


# ------------------------------------------------------------------------------------------------ the restatement of the address arithmetic
def pool_of(sw):
    """the texel pool as the device lays it out: every texture after the one before -> (values, offsets); the 8-bit path's texels as
    r | g << 8 | b << 16 | blend << 24"""
    px, off, n = [], [], 0
    for t in sw.textures:
        p = t.pixels.astype(np.int64)
        if sw.fmt8:
            p = p[:, 0] | p[:, 1] << 8 | p[:, 2] << 16 | p[:, 3] << 24
        px.append(p.reshape(-1)); off.append(n); n += p.shape[0]
    return np.concatenate(px + [np.zeros(0, np.int64)]), off


def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _interp(b, c, mut):
    """(bcx * c1 + bcy * c2) + bcz * c3 in f32, render.rs:1565-1566"""
    (bx, by, bz), (c1, c2, c3) = b, [f32(v) for v in c]
    with np.errstate(all="ignore"):
        if "fma" in mut:                                    # a compiler's contraction: fma(bcz, c3, fma(bcx, c1, bcy * c2))
            return _fma(bz, c3, _fma(bx, c1, (by * c2).astype(f32)))
        if "assoc" in mut:
            return ((bx * c1).astype(f32) + ((by * c2).astype(f32) + (bz * c3).astype(f32)).astype(f32)).astype(f32)
        if "f64" in mut:
            return ((bx.astype(f64) * f64(c1) + by.astype(f64) * f64(c2)) + bz.astype(f64) * f64(c3)).astype(f32)
        return (((bx * c1).astype(f32) + (by * c2).astype(f32)).astype(f32) + (bz * c3).astype(f32)).astype(f32)


def _wrap(c, mut):
    """f32::rem_euclid(1.0): the remainder of the truncating division, + 1.0 when it is negative"""
    with np.errstate(all="ignore"):
        r = np.fmod(c, f32(1.0)).astype(f32)
        if "trunc" not in mut:
            r = np.where(r < 0, (r + f32(1.0)).astype(f32), r)
    return r


def _texel_index(w, n, mut):
    """(wrapped * n) as usize, .min(n - 1): types.rs:675-678"""
    with np.errstate(all="ignore"):
        t = (w * f32(n)).astype(f32)
        if "round" in mut:
            t = np.rint(t)
        i = M.as_usize(t)
    return i if "noclamp" in mut else np.minimum(i, n - 1)


def restate(sw, rec, mut=(), inside=False, affine=None):
    """The texel every pixel of one tap record fetches, from the tapped barycentrics bcx, bcy and the surface's vertices:
    render.rs:1538, :1565-1579, :1583 (`1.0 - v`), types.rs:671-681 -> dict(u, v, tx, ty, addr, value); value -1: outside the pool.
    inside: the pixels inside the triangle before the transparency rule instead of the stored ones."""
    p = "in_" if inside else ""
    bx, by = rec[p + "bcx"], rec[p + "bcy"]
    x, y = (rec["in_x"], rec["in_y"]) if inside else (rec["x"], rec["y"])
    sv, suv = rec["sv"], rec["suv"]
    tid = int(sw.faces["texture_id"][rec["face"]])
    tex = sw.textures[tid]
    tw, th = tex.width, tex.height
    pool, offs = pool_of(sw)
    with np.errstate(all="ignore"):
        if "bcz_edge" in mut:                               # the third edge function instead of the complement
            (x1, y1), (x2, y2) = sv[0][:2], sv[1][:2]
            area = (sv[1][1] - sv[2][1]) * (sv[0][0] - sv[2][0]) + (sv[2][0] - sv[1][0]) * (sv[0][1] - sv[2][1])
            w2 = ((y1 - y2) * (x.astype(f32) - x2)).astype(f32) + ((x2 - x1) * (y.astype(f32) - y2)).astype(f32)
            bz = (w2.astype(f32) * (f32(1.0) / f32(area))).astype(f32)
        else:
            bz = ((f32(1.0) - bx).astype(f32) - by).astype(f32)
        b = (bx, by, bz)
        persp = not (sw.affine if affine is None else affine) and "affine" not in mut
        if not persp:
            u, v = _interp(b, suv[:, 0], mut), _interp(b, suv[:, 1], mut)
        else:                                               # render.rs:1568-1579
            iz = [f32(1.0) / f32(sv[k][2]) for k in range(3)]
            inv_z = _interp(b, iz, mut)
            def over_z(c):
                t = [(b[k] * f32(suv[k][c])).astype(f32) for k in range(3)]
                if "fma" in mut:                            # contracted: fma(t3, iz3, fma(t1, iz1, t2 * iz2))
                    return _fma(t[2], iz[2], _fma(t[0], iz[0], (t[1] * iz[1]).astype(f32)))
                t = [(t[k] * iz[k]).astype(f32) for k in range(3)]
                return ((t[0] + t[1]).astype(f32) + t[2]).astype(f32)
            if "recip" in mut:
                rz = (f32(1.0) / inv_z).astype(f32)
                u, v = (over_z(0) * rz).astype(f32), (over_z(1) * rz).astype(f32)
            else:
                u, v = (over_z(0) / inv_z).astype(f32), (over_z(1) / inv_z).astype(f32)
        if "swap" in mut:
            tw, th = th, tw
        uw = _wrap(u, mut)
        if "noflip" in mut:
            vw = _wrap(v, mut)
        elif "flip_after" in mut:
            vw = (f32(1.0) - _wrap(v, mut)).astype(f32)
        else:
            vw = _wrap((f32(1.0) - v).astype(f32), mut)
        tx, ty = _texel_index(uw, tw, mut), _texel_index(vw, th, mut)
        addr = offs[tid] + ty * (th if "stride" in mut else tw) + tx
    ok = (addr >= 0) & (addr < len(pool))
    value = np.where(ok, pool[np.clip(addr, 0, max(len(pool) - 1, 0))] if len(pool) else -1, -1)
    return dict(u=u, v=v, uw=uw, vw=vw, tx=tx, ty=ty, addr=addr, value=value)


def _textured(sw, tap):
    """(record, strip) of every tap record of a textured strip whose texture has texels"""
    strip = sw.strip_of_row()
    for rec in tap:
        s = sw.strips[int(strip[rec["y"][0]])]
        if rec["tx"] is not None and (rec["tx"] >= 0).all() and s["kind"] != "backing":
            yield rec, s


def _raw_texel(sw, rec):
    """what the model fetched, as the pool holds it (the model replaces 0x0000 by BLACK_DRAWABLE when black is not transparent)"""
    t = sw.textures[int(sw.faces["texture_id"][rec["face"]])]
    p = t.pixels.astype(np.int64)
    if sw.fmt8:
        p = p[:, 0] | p[:, 1] << 8 | p[:, 2] << 16 | p[:, 3] << 24
    return p[rec["ty"] * t.width + rec["tx"]]


# ------------------------------------------------------------------------------------------------ CPU: placement and agreement
CASES = [("A", {}), ("A", dict(zbuffer=True)), ("A", dict(xray=True)), ("K", {}), ("K", dict(zbuffer=True)), ("Z", {}), ("Z", dict(zbuffer=True)),
         ("F-affine", dict(projection="float")), ("F-affine", dict(projection="ortho")), ("F-perspective", dict(projection="float")),
         ("F-perspective", dict(projection="ortho")), ("F-perspective", dict(projection="float", zbuffer=True)),
         ("A8-opaque", {}), ("A8-opaque", dict(zbuffer=True)), ("A8-blend", {}), ("T", {})]
CASES += [(n, kw) for n in TS.SHEETS if "plain" in n for kw in ({}, dict(zbuffer=True))] + [(n, {}) for n in TS.SHEETS if n.startswith("I-")]
_case_id = lambda c: c[0] + "".join(f"-{k}={v}" for k, v in c[1].items())


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_strips_land_on_their_rows_and_the_model_is_the_oracle(oracle, case):
    """every vertex on its integer target (fixed-point projection); C oracle == numpy model: pixels, depths, triangles, fragments; and the
    restatement of the address arithmetic below gives the model's tx, ty and texel at every stored pixel"""
    name, kw = case
    sw = TS.SHEETS[name]()
    assert sw.width <= 256 and sw.height <= TS.MAX_ROWS
    opx, ozb, otm = sw.oracle(oracle, **kw)
    mpx, mzb, tap, res = sw.model(**kw)
    if kw.get("projection", "fixed") == "fixed":
        TS.check_placement(sw, res)
        own = sw.strip_of_row()
        for rec in tap:                                     # a surface stores on the rows of its own strip only
            k = set(own[rec["y"]].tolist())
            assert len(k) == 1 and -1 not in k, (sw.name, rec["face"], k)
    msg = sw.first_difference(mpx, opx, f"{kw}: numpy model against the C oracle")
    assert not msg, msg
    assert np.array_equal(mzb, ozb)
    assert res["triangles_drawn"] == otm.triangles_drawn and res["fragments"] == otm.fragments
    stored = sum(len(r["x"]) for r in tap)
    print(f"{sw.name} {kw}: {sw.width} x {sw.height}, {len(sw.faces)} faces, {len(sw.textures)} textures, {otm.triangles_drawn} triangles drawn, {stored} stored pixels")
    assert stored > 0 and (kw.get("projection") == "ortho" or otm.triangles_drawn == len(sw.faces))
    for rec, s in _textured(sw, tap):                       # (in float and orthographic projection `s` is only roughly the record's strip)
        out = restate(sw, rec)
        assert np.array_equal(out["tx"], rec["tx"]) and np.array_equal(out["ty"], rec["ty"]), (sw.name, s)
        assert np.array_equal(out["value"], _raw_texel(sw, rec)), (sw.name, s)
        assert np.array_equal(out["u"].view(np.uint32), rec["u"].view(np.uint32)) and np.array_equal(out["v"].view(np.uint32), rec["v"].view(np.uint32))


def test_the_frame_does_not_depend_on_the_tap():
    sw = TS.sheet_k()
    px = sw.start_image().reshape(-1)
    zb = np.full(sw.width * sw.height, np.finfo(f32).max, f32)
    with np.errstate(all="ignore"):
        M.render_mesh_15(px, sw.width, sw.height, sw.vertices, sw.faces, sw.textures, TS.PS.Camera(), sw.settings(), None, zb, tap=None)
    assert np.array_equal(px.reshape(sw.height, sw.width, 4), sw.model()[0])


def test_the_frame_is_a_map_of_texels():
    """vertex colour 128, no dither, no shading: the stored pixel is the texel's three 5-bit channels (8-bit path: bytes) unchanged"""
    for name in ("A", "Z", "A8-opaque"):
        sw = TS.SHEETS[name]()
        px, zb, tap, res = sw.model()
        verts = set()
        for rec, s in _textured(sw, tap):
            raw = _raw_texel(sw, rec)
            m = rec["m"]                                    # the three values that are quantised (`>> 3`) or, on the 8-bit path, stored
            verts |= set(np.unique(rec["vert"]).tolist())
            if sw.fmt8:
                assert np.array_equal(m[:, 0] >> 2 | (m[:, 1] >> 2) << 6 | (m[:, 2] >> 2) << 12, (raw & 255) >> 2 | ((raw >> 8) & 255) >> 2 << 6 | ((raw >> 16) & 255) >> 2 << 12), s
            else:
                assert np.array_equal((m[:, 0] >> 3) << 10 | (m[:, 1] >> 3) << 5 | m[:, 2] >> 3, raw), s
            assert not rec["dithered"] and rec["shade"] is None
        print(f"{name}: the interpolated vertex byte takes the values {sorted(verts)}")
        assert verts == {127, 128}
        for t in sw.textures:
            p = t.pixels.astype(np.int64)
            if t.width * t.height:
                if not sw.fmt8:
                    assert (((p >> 10) & 31) >= 4).all() and (((p >> 5) & 31) >= 4).all() and ((p & 31) >= 4).all() and (p < 0x8000).all()
                    g = p.reshape(t.height, t.width)
                else:
                    assert (p[:, :3] & 3 == 3).all()
                    g = (p[:, 0] | p[:, 1] << 8 | p[:, 2] << 16).reshape(t.height, t.width)
                assert (g[:, 1:] != g[:, :-1]).all() and (g[1:] != g[:-1]).all(), "neighbouring texels carry the same code"
    sw = TS.sheet_a()
    for n in (0, 1, 27, 28, 783, 784, TS.CODES15 - 1):      # decode inverts the code for a failure message
        c = int(TS.code15(n))
        assert sw.decode([int(M.expand5((c >> s) & 31)) for s in (10, 5, 0)]) == n


# ------------------------------------------------------------------------------------------------ CPU: the census
def _exact_differs(s, rec, tw):
    """pixels of a sweep-u strip whose texel column differs from the one exact rational arithmetic gives: u is linear in x between the
    quad's vertex columns"""
    u0, u1 = (Fraction(float(f32(c))) for c in s["u"])
    n = 0
    for x, tx in zip(rec["x"].tolist(), rec["tx"].tolist()):
        u = u0 + (u1 - u0) * Fraction(x - s["x0"], s["x1"] - s["x0"])
        fr = u - (u.numerator // u.denominator)
        n += min(int(fr * tw), tw - 1) != tx
    return n


# strips on which the reference's f32 chain must pick another column than exact arithmetic somewhere: 100 texels over [-3, 3] on 250
# pixels (four strips, one per vertex order), 255 texels over 255 pixels (1 / 250 and 1 / 255 are inexact: the interpolated u misses
# boundaries it should sit on), 64 texels over one unit at 1e6 (a texel is 2^-6 wide, the spacing of u there 2^-4).  The other sweep-u
# strips of the three sizes are counted and printed, not asserted: which of them differ depends on the vertex order they were given.
EXACT_STRIPS = (((100, 60), "pm3-250"), ((255, 255), "unit"), ((64, 1), "far-1e6"))


def test_census_sheet_a():
    """What sheet A's reference frame holds, from the model's tap; every stored pixel is counted."""
    sw = TS.sheet_a()
    px, zb, tap, res = sw.model()
    own = sw.strip_of_row()
    cols = {t: np.zeros(max(x.width, 1), bool) for t, x in enumerate(sw.textures)}
    rows = {t: np.zeros(max(x.height, 1), bool) for t, x in enumerate(sw.textures)}
    n = dict(stored=0, textured=0, untextured=0, boundary_u=0, boundary_v=0, plus1_u=0, plus1_v=0, one_u=0, one_v=0, clamp_u=0, clamp_v=0, neg_u=0, neg_v=0,
             period_u=0, period_v=0, nan=0, inf=0)
    bound = {}
    consts = {name: 0 for name, c in TS.CONSTANTS}
    exact = {}
    for rec in tap:
        s = sw.strips[int(own[rec["y"][0]])]
        n["stored"] += len(rec["x"])
        if rec["tx"] is None:
            assert s["kind"] == "untextured"
            n["untextured"] += len(rec["x"])
            continue
        assert (rec["tx"] >= 0).all(), "a texture without texels stored a pixel"
        n["textured"] += len(rec["x"])
        tid, (tw, th) = s["tex"], s["size"]
        cols[tid][rec["tx"]] = True; rows[tid][rec["ty"]] = True
        out = restate(sw, rec)
        u, v = rec["u"], rec["v"]
        with np.errstate(all="ignore"):
            fv = (f32(1.0) - v).astype(f32)
            for c, w, size, k in ((u, out["uw"], tw, "u"), (fv, out["vw"], th, "v")):
                t = (w * f32(size)).astype(f32)
                on = (t == np.floor(t)) & np.isfinite(c)
                if s["kind"] == "sweep-" + k and s["span"] in ("unit", "neg-unit"):
                    n["boundary_" + k] += int(on.sum())
                    bound[(k, s["size"])] = bound.get((k, s["size"]), 0) + int(on.sum())
                n["plus1_" + k] += int((np.fmod(c, f32(1.0)) < 0).sum())
                n["one_" + k] += int((w == f32(1.0)).sum())
                n["clamp_" + k] += int((M.as_usize(t) > size - 1).sum())
                n["neg_" + k] += int((c < 0).sum())
                n["period_" + k] += int(((c == np.floor(c)) & (c != 0) & np.isfinite(c)).sum())
            n["nan"] += int((np.isnan(u) | np.isnan(v)).sum()); n["inf"] += int((np.isinf(u) | np.isinf(v)).sum())
        if "const" in s:
            c = f32(dict(TS.CONSTANTS)[s["const"]])
            held = u if s["kind"] == "const-u" else v
            same = np.isnan(held) if np.isnan(c) else held.view(np.uint32) == c.view(np.uint32)
            consts[s["const"]] += int(same.sum())
        if s["kind"] == "sweep-u" and s["size"] in ((31, 33), (100, 60), (255, 255)):
            exact[(s["size"], s["span"])] = exact.get((s["size"], s["span"]), 0) + _exact_differs(s, rec, tw)
        if s["kind"] == "far-u" and s["size"] == (64, 1):
            exact[(s["size"], "far-" + s["far"])] = exact.get((s["size"], "far-" + s["far"]), 0) + _exact_differs(s, rec, tw)
    print(f"A: {n}")
    print(f"A: pixels exactly on a texel boundary per (axis, size) of the unit spans: {bound}")
    print(f"A: pixels at which the held coordinate is the constant itself, bit for bit: {consts}")
    print(f"A: pixels whose texel column differs from exact rational arithmetic, per (size, span): {exact}")
    assert n["stored"] == n["textured"] + n["untextured"] == sum(len(r["x"]) for r in tap) and n["untextured"] > 0
    for t, x in enumerate(sw.textures):
        if x.width * x.height:
            assert cols[t].all() and rows[t].all(), f"texture {t} ({x.width} x {x.height}): columns {np.nonzero(~cols[t])[0][:8]} / rows {np.nonzero(~rows[t])[0][:8]} never fetched"
    for k in ("u", "v"):
        for size in TS.SIZES_A:
            assert bound[(k, size)] > 0, f"no pixel on a texel boundary in {k} for size {size}"
        assert n["plus1_" + k] > 0 and n["neg_" + k] > 0 and n["period_" + k] > 0
    # the wrap returns exactly 1.0 in u and only the clamp keeps the fetch inside; in v it cannot (test_cases_that_no_frame_can_reach)
    assert n["one_u"] > 0 and n["clamp_u"] >= n["one_u"] and n["one_v"] == 0 and n["clamp_v"] == 0
    assert n["nan"] > 0 and n["inf"] > 0
    # every constant is held by the vertices of two strips per size; the interpolation bcx c + bcy c + bcz c returns c itself at some pixel
    # for every finite one.  +-inf turn into NaN wherever a barycentric is 0 or negative and stay inf elsewhere.
    for name, c in TS.CONSTANTS:
        assert sum(1 for s in sw.strips if s.get("const") == name) >= 4
        assert consts[name] > 0, name
    for key in EXACT_STRIPS:
        assert exact[key] > 0, key
    for s in sw.strips:                                     # zero-size textures sample transparent: their rows keep the clear colour
        if s["kind"] == "zero-size":
            assert (px[s["y0"]:s["y1"] + 1, :, :3] == (TS.PS.CLEAR.r, TS.PS.CLEAR.g, TS.PS.CLEAR.b)).all()


def test_census_other_sheets():
    """K: both transparency settings skip / draw what they should and the backing shows through; Z: the depth ratios are in the frame and
    perspective-correct differs from affine; T: texels with bit 15 blend; every texel column and row of every texture is fetched"""
    for name in ("K", "Z", "T", "A8-opaque", "I-16x16", "A-plain-100x60", "Z-plain-31x33"):
        sw = TS.SHEETS[name]()
        px, zb, tap, res = sw.model()
        cols = {t: np.zeros(max(x.width, 1), bool) for t, x in enumerate(sw.textures)}
        rows = {t: np.zeros(max(x.height, 1), bool) for t, x in enumerate(sw.textures)}
        n = dict(stored=0, skipped=0, one_u=0, plus1=0)
        for rec in tap:
            n["stored"] += len(rec["x"])
            if rec["tx"] is None or (rec["tx"] < 0).any():
                continue
            tid = int(sw.faces["texture_id"][rec["face"]])
            cols[tid][rec["in_tx"]] = True; rows[tid][rec["in_ty"]] = True
            n["skipped"] += len(rec["in_x"]) - len(rec["x"])
            out = restate(sw, rec)
            n["one_u"] += int((out["uw"] == f32(1.0)).sum())
            with np.errstate(all="ignore"):
                n["plus1"] += int((np.fmod(rec["u"], f32(1.0)) < 0).sum())
        print(f"{name}: {n}")
        assert all(cols[t].all() and rows[t].all() for t, x in enumerate(sw.textures) if x.width * x.height), name
        assert n["plus1"] > 0
        if name == "T":
            recs = [r for r in tap if r["tx"] is not None]
            assert all(r["blend"] == abi.AVERAGE for r in recs) and any(((r["texel"] & 0x8000) != 0).any() for r in recs) and any(((r["texel"] & 0x8000) == 0).any() for r in recs)
        if name == "K":
            assert n["skipped"] > 0 and n["one_u"] > 0
            offs = pool_of(sw)[1]
            assert sum(o % 32 != 0 for o in offs[1:]) >= 3, offs
            # the backing's colour is what the frame holds left of an inset quad; it shows through a black_transparent quad only
            for s in sw.strips:
                if s["x0"] > 0:
                    quad = px[s["y0"]:s["y1"] + 1, s["x0"]:min(s["x1"], sw.width - 1) + 1]
                    through = int((quad == px[s["y0"], 0]).all(axis=2).sum())
                    assert (through > 0) == bool(s["black_tr"]), (s, through)
    sw = TS.sheet_z()
    persp, aff = sw.model()[0], sw.model(affine=True)[0]
    per_pair = {z: sum(int((persp[s["y0"]:s["y1"] + 1] != aff[s["y0"]:s["y1"] + 1]).any(axis=2).sum()) for s in sw.strips if s["z"] == z) for z in TS.DEPTH_PAIRS}
    print(f"Z: pixels at which perspective-correct and affine addressing differ, per (z left, z right): {per_pair}")
    assert all(v > 0 for z, v in per_pair.items() if z[0] != z[1])


def test_cases_that_no_frame_can_reach():
    """The wrap returns exactly 1.0 in v for no v at all (see the module docstring): checked over every f32 v near the candidates, and the
    argument covers the rest.  In u the case is real: -1e-9 wraps to 1.0."""
    assert _wrap(np.array([-1e-9], f32), ())[0] == f32(1.0)
    cand = []
    for c in (0.0, 1.0, 2.0, -1.0, 1e-9, 1.0 + 1e-9, 1e-40, 3.0, 1e6):
        x = f32(c)
        lo = x
        for _ in range(2000):
            lo = np.nextafter(lo, f32(-np.inf))
        v = [lo]
        for _ in range(4000):
            v.append(np.nextafter(v[-1], f32(np.inf)))
        cand.append(np.array(v, f32))
    v = np.concatenate(cand)
    w = _wrap((f32(1.0) - v).astype(f32), ())
    print(f"wrap(1.0 - v) == 1.0 at {int((w == f32(1.0)).sum())} of {len(v)} values of v around 0, 1, 2, -1, 3 and 1e6")
    assert not (w == f32(1.0)).any()
    # the argument's two steps: r + 1.0 == 1.0 needs r >= -2^-25; 1.0 - v is never in [-2^-25, 0)
    assert f32(-2.0 ** -25) + f32(1.0) == f32(1.0) and np.nextafter(f32(-2.0 ** -25), f32(-1.0)) + f32(1.0) < f32(1.0)
    assert f32(1.0) - np.nextafter(f32(1.0), f32(2.0)) == f32(-2.0 ** -23)


# ------------------------------------------------------------------------------------------------ CPU: the sheets see the errors they are for
MUTATIONS = [("A", "noflip"), ("A", "flip_after"), ("A", "trunc"), ("A", "noclamp"), ("A", "round"), ("A", "stride"), ("A", "swap"), ("A", "fma"), ("A", "assoc"),
             ("A", "f64"), ("A", "bcz_edge"), ("Z", "affine"), ("Z", "recip"), ("Z", "fma"), ("F-affine", "fma"), ("A8-opaque", "noclamp"), ("A8-opaque", "noflip"),
             ("K", "noclamp"), ("T", "flip_after"), ("I-16x16", "round"), ("A-plain-100x60", "fma"), ("Z-plain-31x33", "recip")]


@pytest.mark.parametrize("name,mut", MUTATIONS, ids=[f"{a}-{b}" for a, b in MUTATIONS])
def test_one_point_mutations_change_the_sheet(name, mut):
    """each one-point change of the restatement fetches another texel value at a stored pixel of the named sheet (the frame is a map of
    texel values, so the pixel changes with it)"""
    sw = TS.SHEETS[name]()
    px, zb, tap, res = sw.model()
    n, where = 0, {}
    for rec, s in _textured(sw, tap):
        d = int((restate(sw, rec, mut=(mut,))["value"] != _raw_texel(sw, rec)).sum())
        n += d
        if d:
            key = (s["kind"], s.get("span") or s.get("const") or s.get("far"))
            where[key] = where.get(key, 0) + d
    top = sorted(where.items(), key=lambda kv: -kv[1])[:4]
    print(f"{sw.name}: mutation {mut} changes {n} stored pixels; most on {top}")
    assert n > 0


def test_a_mask_address_one_texel_to_the_right_changes_sheet_k():
    """the coverage phase decides from a bit of the skip mask at the texel's address; one texel to the right, another surface wins the
    pixel: counted over every pixel inside a black_transparent triangle, drawn or not"""
    sw = TS.sheet_k()
    px, zb, tap, res = sw.model()
    pool, offs = pool_of(sw)
    skip = (pool & 0x7FFF) == 0
    n = 0
    for rec, s in _textured(sw, tap):
        if not s["black_tr"]:
            continue
        addr = restate(sw, rec, inside=True)["addr"]
        drawn = ~skip[addr]
        stored = np.zeros((sw.height, sw.width), bool); stored[rec["y"], rec["x"]] = True
        assert np.array_equal(drawn, stored[rec["in_y"], rec["in_x"]]), "the restated mask bit is not the model's decision"
        n += int((~skip[np.minimum(addr + 1, len(pool) - 1)] != drawn).sum())
    print(f"K: a mask address one texel to the right changes the decision at {n} pixels")
    assert n > 0


# ------------------------------------------------------------------------------------------------ GPU: bit for bit on every path
def _restore(ctx):
    ctx.set_routes(0)
    ctx.set_fragment_counting(1)


def _routed(gpu_ctx, sw, oracle, off, what, counting=0, advanced=(), still=(), check_z=False, **kw):
    """test_pixel_swatches._routed -- one resident draw with the routes of `off` switched off, the frame (and depths) the oracle's, the
    route counters of `advanced` moved and those of `still` not -- and, with counting on in painter's mode on the RGB555 path, the
    fragments the library reports are the oracle's.  The caller restores routes and counting."""
    want, wantz, etm = sw.oracle(oracle, **kw)
    gpu_ctx.set_fragment_counting(counting)
    gpu_ctx.set_routes(off)
    before = gpu_ctx.route_counts()
    fb, tm = TS.PS.gpu_draw(gpu_ctx, sw, resident=True, **kw)
    after = gpu_ctx.route_counts()
    tag = f"{what} routes off: {off} counting={counting}"
    TP._same(sw, fb.pixels, want, tag)
    if check_z:
        TP._same(sw, fb.zbuffer.view(np.uint32), wantz, tag + " depths")
    assert tm.triangles_drawn == etm.triangles_drawn
    if counting and not kw.get("zbuffer") and not sw.fmt8:
        assert tm.fragments == etm.fragments, tag
    moved = sorted(k for k in after if after[k] != before[k])
    for k in advanced:
        assert after[k] > before[k], (tag, k, moved)
    for k in still:
        assert after[k] == before[k], (tag, k, moved)


@gpu
@pytest.mark.parametrize("name", ["A", "K"])
@pytest.mark.parametrize("zbuffer", [False, True], ids=["painter", "zbuffer"])
def test_sheets_a_and_k(gpu_ctx, oracle, name, zbuffer):
    """default routes; fragment counting on and off, resident and immediate; depths too in z-buffer mode"""
    try:
        TP._draws(gpu_ctx, TS.SHEETS[name](), oracle, name, check_z=zbuffer, zbuffer=zbuffer)
    finally:
        _restore(gpu_ctx)


def _route_cases():
    from bonnie32_amd import rasterizer as R
    C = R.Context
    return ((0, "inline_bin"), (C.ROUTE_SPAN_COVER, "inline_bin"), (C.ROUTE_DIRECT_BIN, "inline_bin"), (C.ROUTE_INLINE_BIN, "direct_bin"), (C.ROUTE_CUT_TILES, "inline_bin"),
            (C.ROUTE_WIDE_GROUPS, "inline_bin"), (C.ROUTE_INLINE_BIN | C.ROUTE_WIDE_GROUPS, "direct_bin"), (C.ROUTE_DIRECT_BIN | C.ROUTE_INLINE_BIN, "counting_sort"),
            (C.ROUTE_SORT_FREE, "keyed"))


@gpu
@pytest.mark.parametrize("name", ["A", "K"])
def test_sheets_a_and_k_on_every_route(gpu_ctx, oracle, name):
    """every binning route with its counter asserted (inline_bin, direct_bin, counting_sort, keyed) and the masks ROUTE_SPAN_COVER,
    ROUTE_CUT_TILES, ROUTE_WIDE_GROUPS; counting off and on, so coverage is CHEAP where the textures allow it (sheet A) and EXACT
    (the skip mask; always on sheet K, whose textures are half skippable)"""
    sw = TS.SHEETS[name]()
    try:
        for off, route in _route_cases():
            for counting in (0, 1):
                _routed(gpu_ctx, sw, oracle, off, name, counting=counting, **TP._only(route))
        _routed(gpu_ctx, sw, oracle, 0, name + " z-buffer", check_z=True, zbuffer=True)
        from bonnie32_amd import rasterizer as R
        _routed(gpu_ctx, sw, oracle, R.Context.ROUTE_SORT_FREE, name + " z-buffer", check_z=True, zbuffer=True, **TP._only("keyed"))
    finally:
        _restore(gpu_ctx)


@gpu
@pytest.mark.parametrize("name", [n for n in TS.SHEETS if "plain" in n])
def test_plain_sheets_on_the_one_texture_kernels(gpu_ctx, oracle, name):
    """launch_p64's one-texture kernels (k_cover_plain, k_cover_plain_z; their EXACT instantiation with counting on): one texture without a
    skippable texel, in-fill collection and the 16-wave workgroups off, direct_bin asserted; painter's and z-buffer mode, counting off
    and on.  Then the keyed route with counting on: EXACT coverage of a one-texture frame stages the texture in LDS when it fits
    (k_cover<1>, texel_drawn<1>: 31 x 33 and 100 x 60 fit, 255 x 255 does not and is read from global memory).  Which kernel ran is not
    observable; the conditions are those of launch_p64 and launch_fill.  The Z-plain sheets ask for perspective-correct addressing
    under the same conditions."""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    sw = TS.SHEETS[name]()
    assert len(sw.textures) == 1 and ((sw.textures[0].pixels & 0x7FFF) != 0).all()
    try:
        for counting in (0, 1):
            for zbuffer in (False, True):
                _routed(gpu_ctx, sw, oracle, C.ROUTE_INLINE_BIN | C.ROUTE_WIDE_GROUPS, name, counting=counting, check_z=zbuffer, zbuffer=zbuffer, **TP._only("direct_bin"))
                _routed(gpu_ctx, sw, oracle, C.ROUTE_SORT_FREE, name, counting=counting, check_z=zbuffer, zbuffer=zbuffer, **TP._only("keyed"))
        gpu_ctx.set_routes(0)
        TP._draws(gpu_ctx, sw, oracle, name + " default routes")
    finally:
        _restore(gpu_ctx)


@gpu
@pytest.mark.parametrize("zbuffer", [False, True], ids=["painter", "zbuffer"])
def test_sheet_z(gpu_ctx, oracle, zbuffer):
    """perspective-correct addressing: default routes (counting on and off, resident and immediate), the setup kernel's bins, the keyed route"""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    sw = TS.sheet_z()
    try:
        TP._draws(gpu_ctx, sw, oracle, "Z", check_z=zbuffer, zbuffer=zbuffer)
        for counting in (0, 1):
            _routed(gpu_ctx, sw, oracle, C.ROUTE_SORT_FREE, "Z", counting=counting, check_z=zbuffer, zbuffer=zbuffer, **TP._only("keyed"))
            _routed(gpu_ctx, sw, oracle, C.ROUTE_INLINE_BIN, "Z", counting=counting, check_z=zbuffer, zbuffer=zbuffer, **TP._only("direct_bin"))
    finally:
        _restore(gpu_ctx)


@gpu
@pytest.mark.parametrize("name", ["F-affine", "F-perspective"])
@pytest.mark.parametrize("projection", ["float", "ortho"])
def test_sheet_f(gpu_ctx, oracle, name, projection):
    """the literal replay: float and orthographic projection, vertices off the integers, F_SLOW surfaces; painter's and z-buffer mode"""
    from bonnie32_amd import rasterizer as R
    sw = TS.SHEETS[name]()
    try:
        TP._draws(gpu_ctx, sw, oracle, f"{name} {projection}", projection=projection)
        TP._draws(gpu_ctx, sw, oracle, f"{name} {projection} z-buffer", countings=(0,), check_z=True, projection=projection, zbuffer=True)
        _routed(gpu_ctx, sw, oracle, R.Context.ROUTE_SORT_FREE, f"{name} {projection}", counting=1, projection=projection, **TP._only("keyed"))
    finally:
        _restore(gpu_ctx)


@gpu
def test_sheet_a8_opaque_in_the_fused_fill(gpu_ctx, oracle):
    """Texture::sample (texel_index on Color words) from the fused fill; with the setup kernel's bins and 8-wave workgroups k_cover_plain8's conditions (launch_p64)"""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    sw = TS.sheet_a8(abi.OPAQUE)
    try:
        for off, route in ((0, "inline_bin"), (C.ROUTE_INLINE_BIN | C.ROUTE_WIDE_GROUPS, "direct_bin"), (C.ROUTE_DIRECT_BIN | C.ROUTE_INLINE_BIN, "counting_sort")):
            for counting in (0, 1):
                for zbuffer in (False, True):
                    _routed(gpu_ctx, sw, oracle, off, "A8-opaque", counting=counting, check_z=zbuffer, zbuffer=zbuffer, **TP._only(route))
        gpu_ctx.set_routes(0)
        TP._draws(gpu_ctx, sw, oracle, "A8-opaque immediate", residents=(False,))
    finally:
        _restore(gpu_ctx)


@gpu
def test_sheet_a8_with_blending_texels(gpu_ctx, oracle):
    """Average texels: no overwrite pass, the ordered walk of k_blend (texel_drawn<0, FMT8>), shown by the keyed counter"""
    sw = TS.sheet_a8(abi.AVERAGE)
    try:
        for zbuffer in (False, True):
            before = gpu_ctx.route_counts()
            TP._draws(gpu_ctx, sw, oracle, "A8-blend", check_z=zbuffer, zbuffer=zbuffer)
            after = gpu_ctx.route_counts()
            assert after["keyed"] > before["keyed"] and all(after[r] == before[r] for r in TP.BIN_ROUTES if r != "keyed"), (before, after)
    finally:
        _restore(gpu_ctx)


@gpu
def test_sheet_t_in_the_transparent_pass(gpu_ctx, oracle):
    """textures with a blend mode over an uploaded back: every face is in the transparent pass, k_blend's texel_drawn<0>"""
    sw = TS.sheet_t()
    try:
        TP._draws(gpu_ctx, sw, oracle, "T")
        TP._draws(gpu_ctx, sw, oracle, "T z-buffer", countings=(0,), check_z=True, zbuffer=True)
    finally:
        _restore(gpu_ctx)


@gpu
@pytest.mark.parametrize("size", TS.INDEXED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sheet_i_from_an_indexed_atlas(gpu_ctx, oracle, size):
    """index bytes + CLUT staged in LDS (atlas_texel): the lds_atlas counter advances; with ROUTE_LDS_ATLAS off it stands still and the
    expanded texels give the same frame"""
    from bonnie32_amd import rasterizer as R
    sw = TS.sheet_i(*size)
    want, wantz, etm = sw.oracle(oracle)
    try:
        for off, moves in ((0, True), (R.Context.ROUTE_LDS_ATLAS, False)):
            for counting in (0, 1):
                gpu_ctx.set_routes(off)
                gpu_ctx.set_fragment_counting(counting)
                before = gpu_ctx.route_counts()["lds_atlas"]
                fb, tm = TS.PS.gpu_draw(gpu_ctx, sw, indexed=sw.indexed)
                after = gpu_ctx.route_counts()["lds_atlas"]
                TP._same(sw, fb.pixels, want, f"indexed routes off: {off} counting={counting}")
                assert tm.triangles_drawn == etm.triangles_drawn
                assert (after > before) == moves, (off, counting, before, after)
    finally:
        _restore(gpu_ctx)


@gpu
def test_sheet_a_in_xray_mode(gpu_ctx, oracle):
    """x-ray mode: every store averages with the back, in order -- the ordered walk"""
    try:
        TP._draws(gpu_ctx, TS.sheet_a(), oracle, "A x-ray", xray=True)
    finally:
        _restore(gpu_ctx)


@gpu
def test_sheet_k_in_two_bands_that_cut_a_strip(gpu_ctx, oracle):
    """bands (0, 151) and (151, H): row 151 is the second row of a strip; the partial frames assemble to the oracle's"""
    sw = TS.sheet_k()
    want, _, etm = sw.oracle(oracle)
    cut = 151
    assert any(s["y0"] < cut <= s["y1"] for s in sw.strips)
    row = sw.width * 4
    try:
        for counting in (0, 1):
            gpu_ctx.set_fragment_counting(counting)
            assembled = np.zeros(sw.width * sw.height * 4, np.uint8)
            for y0, y1 in ((0, cut), (cut, sw.height)):
                fb, tm = TS.PS.gpu_draw(gpu_ctx, sw, resident=True, band=(y0, y1))
                assembled[y0 * row:y1 * row] = fb.pixels[y0 * row:y1 * row]
            TP._same(sw, assembled, want, f"bands counting={counting}")
    finally:
        _restore(gpu_ctx)
