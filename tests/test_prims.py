"""The rest of the Framebuffer drawing methods (render.rs:631-971) through b32_draw_prims, mixed with the line family.

Expected images: `ref_prim`, a literal restatement of the reference methods (scalar loops, one function per method, f32 operands as
np.float32), pinned to the oracle's b32o_draw_line where the oracle has an entry and to hand-computed cases otherwise; and `np_prims`,
which applies a batch in order with every primitive vectorised over its pixels (runs of kinds 0..4 go through test_lines.np_lines),
pinned to `ref_prim` on CPU.  Every GPU case compares the device frame with np_prims byte for byte."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi
from tests.test_lines import ROOT, _oracle_line_fns, _project, _upload_zbuffer, np_lines, ref_line

f32 = np.float32
KINDS = tuple(range(11))


def _as_i32(v):                                                # Rust `f as i32`: toward zero, saturating, NaN -> 0
    v = float(v)
    if v != v:
        return 0
    return int(max(min(v, 2147483647.0), -2147483648.0)) if abs(v) < 2 ** 31 else (2147483647 if v > 0 else -2147483648)


# ---------------------------------------------------------------- literal restatement (render.rs:300-334, 631-971)
def _set_pixel(px, w, h, x, y, rgb, blend):                    # render.rs:300-309
    if 0 <= x < w and 0 <= y < h:
        i = (y * w + x) * 4
        px[i:i + 3] = rgb
        px[i + 3] = 0 if blend == abi.ERASE else 255


def _set_pixel_alpha(px, w, h, x, y, rgb, alpha):              # render.rs:646-667
    if 0 <= x < w and 0 <= y < h:
        i = (y * w + x) * 4
        a = int(alpha); inv = 255 - a
        for c in range(3):
            px[i + c] = (int(rgb[c]) * a + int(px[i + c]) * inv) // 255
        px[i + 3] = 255


def _blend_with(front, mode, back):                            # Color::blend_with, types.rs:886-929
    if mode == abi.OPAQUE:
        return front, 255
    if mode == abi.ERASE:
        return (0, 0, 0), 0                                    # Color::TRANSPARENT
    f = {abi.AVERAGE: lambda b, f: (b + f) // 2, abi.ADD: lambda b, f: min(b + f, 255), abi.SUBTRACT: lambda b, f: max(b - f, 0),
         abi.ADD_QUARTER: lambda b, f: min(b + f // 4, 255)}[mode]
    return tuple(f(int(b_), int(f_)) for b_, f_ in zip(back, front)), 255


def _set_pixel_blended(px, w, h, x, y, rgb, mode):             # render.rs:313-334
    if 0 <= x < w and 0 <= y < h:
        i = (y * w + x) * 4
        out, a = _blend_with(rgb, mode, tuple(int(v) for v in px[i:i + 3]))
        px[i:i + 3] = out
        px[i + 3] = a


def ref_draw_line_blended(px, w, h, x0, y0, x1, y1, rgb, blend, mode):   # render.rs:720-755
    dx = abs(x1 - x0); dy = -abs(y1 - y0)
    sx = 1 if x0 < x1 else -1; sy = 1 if y0 < y1 else -1
    err = dx + dy; x, y = x0, y0
    while True:
        if 0 <= x < w and 0 <= y < h:
            if mode == abi.OPAQUE:
                _set_pixel(px, w, h, x, y, rgb, blend)
            else:
                _set_pixel_blended(px, w, h, x, y, rgb, mode)
        if x == x1 and y == y1:
            break
        e2 = 2 * err
        if e2 >= dy:
            err += dy; x += sx
        if e2 <= dx:
            err += dx; y += sy


def ref_draw_circle(px, w, h, cx, cy, radius, rgb, blend, alpha=None):   # render.rs:631-642 (alpha: draw_circle_alpha :670-681)
    r_sq = radius * radius
    for y in range(max(cy - radius, 0), min(cy + radius, h - 1) + 1):
        for x in range(max(cx - radius, 0), min(cx + radius, w - 1) + 1):
            dx = x - cx; dy = y - cy
            if dx * dx + dy * dy <= r_sq:
                if alpha is None:
                    _set_pixel(px, w, h, x, y, rgb, blend)
                else:
                    _set_pixel_alpha(px, w, h, x, y, rgb, alpha)


def thick_corners(x0, y0, x1, y1, thickness):
    """draw_thick_line's four corners (render.rs:887-906), f32; None: len < 0.001."""
    dx = f32(x1 - x0); dy = f32(y1 - y0)
    ln = np.sqrt(dx * dx + dy * dy)
    if ln < f32(0.001):
        return None
    half = f32(thickness) * f32(0.5)
    ppx = -dy / ln * half
    ppy = dx / ln * half
    return [(f32(x0) + ppx, f32(y0) + ppy), (f32(x0) - ppx, f32(y0) - ppy), (f32(x1) - ppx, f32(y1) - ppy), (f32(x1) + ppx, f32(y1) + ppy)]


def thick_box(corners, w, h):
    """The bounding box of render.rs:909-918: f32::min / f32::max folds, `as i32`, clamped."""
    min_x, max_x, min_y, max_y = f32(np.inf), f32(-np.inf), f32(np.inf), f32(-np.inf)
    for cxy in corners:
        min_x = min(min_x, cxy[0]); max_x = max(max_x, cxy[0]); min_y = min(min_y, cxy[1]); max_y = max(max_y, cxy[1])
    return max(_as_i32(min_x), 0), min(_as_i32(max_x), w - 1), max(_as_i32(min_y), 0), min(_as_i32(max_y), h - 1)


def ref_draw_thick_line(px, w, h, x0, y0, x1, y1, thickness, rgb, blend):   # render.rs:875-938
    if thickness <= 1:
        ref_draw_line_blended(px, w, h, x0, y0, x1, y1, rgb, blend, abi.OPAQUE)
        return
    corners = thick_corners(x0, y0, x1, y1, thickness)
    if corners is None:
        return
    min_x, max_x, min_y, max_y = thick_box(corners, w, h)
    if min_x > max_x or min_y > max_y:
        return
    with np.errstate(over="ignore"):
        for py in range(min_y, max_y + 1):
            for px_ in range(min_x, max_x + 1):
                p = (f32(px_) + f32(0.5), f32(py) + f32(0.5))
                inside = True
                for i in range(4):
                    a = corners[i]; b = corners[(i + 1) % 4]
                    cross = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
                    if cross < f32(0.0):
                        inside = False
                        break
                if inside:
                    _set_pixel(px, w, h, px_, py, rgb, blend)


def ref_draw_rect(px, w, h, x0, y0, x1, y1, rgb, blend):      # render.rs:941-951
    min_x, max_x = (x0, x1) if x0 < x1 else (x1, x0)
    min_y, max_y = (y0, y1) if y0 < y1 else (y1, y0)
    for a, b_, c, d in ((min_x, min_y, max_x, min_y), (max_x, min_y, max_x, max_y), (max_x, max_y, min_x, max_y), (min_x, max_y, min_x, min_y)):
        ref_draw_line_blended(px, w, h, a, b_, c, d, rgb, blend, abi.OPAQUE)


def ref_draw_filled_rect(px, w, h, x0, y0, x1, y1, rgb, blend):   # render.rs:954-971
    min_x, max_x = (x0, x1) if x0 < x1 else (x1, x0)
    min_y, max_y = (y0, y1) if y0 < y1 else (y1, y0)
    for y in range(max(min_y, 0), min(max_y, h - 1) + 1):
        for x in range(max(min_x, 0), min(max_x, w - 1) + 1):
            _set_pixel(px, w, h, x, y, rgb, blend)


def to_lines(P):
    L = np.zeros(len(P), abi.LINE_DTYPE)
    for f in abi.LINE_DTYPE.names:
        if f != "_pad":
            L[f] = P[f]
    return L


def ref_prim(px, zb, w, h, p):
    """One reference call, literally."""
    kind = int(p["kind"])
    x0, y0, x1, y1, size = int(p["x0"]), int(p["y0"]), int(p["x1"]), int(p["y1"]), int(p["size"])
    rgb, blend = (int(p["r"]), int(p["g"]), int(p["b"])), int(p["blend"])
    if kind <= abi.LINE_3D_ALPHA:
        ref_line(px, zb, w, h, to_lines(np.atleast_1d(p))[0])
    elif kind == abi.PRIM_LINE_BLENDED:
        ref_draw_line_blended(px, w, h, x0, y0, x1, y1, rgb, blend, int(p["mode"]))
    elif kind == abi.PRIM_CIRCLE:
        ref_draw_circle(px, w, h, x0, y0, size, rgb, blend)
    elif kind == abi.PRIM_CIRCLE_ALPHA:
        ref_draw_circle(px, w, h, x0, y0, size, rgb, blend, alpha=int(p["alpha"]))
    elif kind == abi.PRIM_THICK_LINE:
        ref_draw_thick_line(px, w, h, x0, y0, x1, y1, size, rgb, blend)
    elif kind == abi.PRIM_RECT:
        ref_draw_rect(px, w, h, x0, y0, x1, y1, rgb, blend)
    else:
        ref_draw_filled_rect(px, w, h, x0, y0, x1, y1, rgb, blend)


# ---------------------------------------------------------------- vectorised model
def _walk(x0, y0, x1, y1, w, h):
    """The on-screen pixels of one Bresenham line (closed form, as np_lines), in step order; each pixel once."""
    adx, ady = abs(x1 - x0), abs(y1 - y0)
    sx = 1 if x0 < x1 else -1; sy = 1 if y0 < y1 else -1
    xm = adx >= ady
    N = max(adx, ady)
    m0, sm, lim = (x0, sx, w - 1) if xm else (y0, sy, h - 1)
    klo, khi = (-m0, lim - m0) if sm > 0 else (m0 - lim, m0)
    klo, khi = max(klo, 0), min(khi, N)
    if klo > khi:
        return np.zeros(0, np.int64)
    k = np.arange(klo, khi + 1, dtype=np.int64)
    dmaj, dmin = (adx, ady) if xm else (ady, adx)
    j = (2 * dmin * k + dmaj) // (2 * dmaj) if dmaj > 0 else np.zeros_like(k)
    maj = m0 + sm * k
    mnr = (y0 + sy * j) if xm else (x0 + sx * j)
    X, Y = (maj, mnr) if xm else (mnr, maj)
    on = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
    return Y[on] * w + X[on]


def _store(img, pix, p, op):
    rgb = np.array([int(p["r"]), int(p["g"]), int(p["b"])], np.int64)
    if op == "set":
        img[pix, :3] = rgb; img[pix, 3] = 0 if int(p["blend"]) == abi.ERASE else 255
    elif op == "alpha":
        a = int(p["alpha"])
        img[pix, :3] = (rgb * a + img[pix, :3].astype(np.int64) * (255 - a)) // 255; img[pix, 3] = 255
    else:
        mode = int(p["mode"])
        b = img[pix, :3].astype(np.int64)
        if mode == abi.ERASE:
            img[pix] = 0
            return
        out = {abi.AVERAGE: (b + rgb) // 2, abi.ADD: np.minimum(b + rgb, 255), abi.SUBTRACT: np.maximum(b - rgb, 0),
               abi.ADD_QUARTER: np.minimum(b + rgb // 4, 255)}[mode]
        img[pix, :3] = out; img[pix, 3] = 255


def _grid(x0, x1, y0, y1, w):
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    return xs.reshape(-1).astype(np.int64), ys.reshape(-1).astype(np.int64)


def np_prim(img, w, h, p):
    """One primitive of kind >= 5, vectorised over its pixels."""
    kind = int(p["kind"])
    x0, y0, x1, y1, size = int(p["x0"]), int(p["y0"]), int(p["x1"]), int(p["y1"]), int(p["size"])
    if kind == abi.PRIM_LINE_BLENDED or (kind == abi.PRIM_THICK_LINE and size <= 1):
        pix = _walk(x0, y0, x1, y1, w, h)
        _store(img, pix, p, "ps1" if kind == abi.PRIM_LINE_BLENDED and int(p["mode"]) != abi.OPAQUE else "set")
    elif kind in (abi.PRIM_CIRCLE, abi.PRIM_CIRCLE_ALPHA):
        bx0, bx1, by0, by1 = max(x0 - size, 0), min(x0 + size, w - 1), max(y0 - size, 0), min(y0 + size, h - 1)
        if bx0 > bx1 or by0 > by1:
            return
        X, Y = _grid(bx0, bx1, by0, by1, w)
        keep = (X - x0) ** 2 + (Y - y0) ** 2 <= size * size
        _store(img, (Y * w + X)[keep], p, "alpha" if kind == abi.PRIM_CIRCLE_ALPHA else "set")
    elif kind == abi.PRIM_THICK_LINE:
        corners = thick_corners(x0, y0, x1, y1, size)
        if corners is None:
            return
        bx0, bx1, by0, by1 = thick_box(corners, w, h)
        if bx0 > bx1 or by0 > by1:
            return
        X, Y = _grid(bx0, bx1, by0, by1, w)
        P0 = X.astype(f32) + f32(0.5); P1 = Y.astype(f32) + f32(0.5)
        keep = np.ones(len(X), bool)
        with np.errstate(over="ignore"):
            for i in range(4):
                a = corners[i]; b = corners[(i + 1) % 4]
                cross = (b[0] - a[0]) * (P1 - a[1]) - (b[1] - a[1]) * (P0 - a[0])
                keep &= ~(cross < f32(0.0))
        _store(img, (Y * w + X)[keep], p, "set")
    else:
        mnx, mxx, mny, mxy = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        bx0, bx1, by0, by1 = max(mnx, 0), min(mxx, w - 1), max(mny, 0), min(mxy, h - 1)
        if bx0 > bx1 or by0 > by1:
            return
        X, Y = _grid(bx0, bx1, by0, by1, w)
        keep = np.ones(len(X), bool) if kind == abi.PRIM_FILLED_RECT else (X == mnx) | (X == mxx) | (Y == mny) | (Y == mxy)
        _store(img, (Y * w + X)[keep], p, "set")


def np_prims(px, zb, w, h, prims):
    """The sequential result of `prims` (in order) on px (flat RGBA, modified in place)."""
    P = np.ascontiguousarray(prims, abi.PRIM_DTYPE).reshape(-1)
    img = px.reshape(-1, 4)
    kinds = P["kind"]
    i = 0
    while i < len(P):
        if kinds[i] <= abi.LINE_3D_ALPHA:
            j = i
            while j < len(P) and kinds[j] <= abi.LINE_3D_ALPHA:
                j += 1
            np_lines(px, zb, w, h, to_lines(P[i:j]))
            i = j
        else:
            np_prim(img, w, h, P[i])
            i += 1


def random_prims(rng, n, w, h, kinds=KINDS, max_len=48, max_r=12, zrange=(0.0, 4000.0)):
    P = np.zeros(n, abi.PRIM_DTYPE)
    P["x0"] = rng.integers(-30, w + 30, n); P["y0"] = rng.integers(-30, h + 30, n)
    P["x1"] = P["x0"] + rng.integers(-max_len, max_len + 1, n); P["y1"] = P["y0"] + rng.integers(-max_len, max_len + 1, n)
    P["z0"] = rng.uniform(*zrange, n).astype(f32); P["z1"] = rng.uniform(*zrange, n).astype(f32)
    P["r"], P["g"], P["b"] = (rng.integers(0, 256, n) for _ in range(3))
    P["blend"] = np.where(rng.random(n) < 0.15, abi.ERASE, abi.OPAQUE)
    P["kind"] = rng.choice(np.array(kinds, np.uint8), n)
    P["alpha"] = rng.choice(np.array([0, 1, 128, 140, 191, 255], np.uint8), n)
    P["mode"] = rng.integers(0, 6, n)
    circ = (P["kind"] == abi.PRIM_CIRCLE) | (P["kind"] == abi.PRIM_CIRCLE_ALPHA)
    P["size"] = np.where(circ, rng.integers(-1, max_r + 1, n), rng.choice(np.array([-5, 0, 1, 2, 3, 4, 7], np.int32), n))
    return P


def edge_prims(w, h, far=1 << 29):
    """The edge cases: radius -1 / 0 / 32767, thickness -5 / 0 / 1 / 2 / 3 / 2^30, equal end points, centres and corners `far` off screen,
    every blend mode and Erase colours (LINE_BLENDED Opaque with an Erase colour), alpha 0 / 255.  (The literal model walks every step of
    a line: it gets a smaller `far`.)"""
    recs = []
    B = far

    def add(kind, x0, y0, x1=0, y1=0, size=0, rgb=(200, 60, 30), blend=abi.OPAQUE, alpha=255, mode=0):
        p = np.zeros(1, abi.PRIM_DTYPE)
        p["x0"], p["y0"], p["x1"], p["y1"], p["size"] = x0, y0, x1, y1, size
        p["r"], p["g"], p["b"], p["blend"], p["kind"], p["alpha"], p["mode"] = *rgb, blend, kind, alpha, mode
        recs.append(p)

    for k in (abi.PRIM_CIRCLE, abi.PRIM_CIRCLE_ALPHA):
        for r in (-1, 0, 1, 5):
            add(k, w // 3 + 3 * r, h // 2, size=r, alpha=140)
        add(k, w // 2, h // 2, size=32767, rgb=(10, 20, 30), alpha=17)
        add(k, -B, h // 2, size=32767, alpha=200); add(k, w // 2, (1 << 30) - 1, size=9)
        add(k, w + 5, h // 3, size=9, alpha=0); add(k, -4, -4, size=6, alpha=255)
    for t in (-5, 0, 1, 2, 3, 1 << 30):
        add(abi.PRIM_THICK_LINE, 5, 7, w - 9, 7 + (t & 7), size=t, rgb=(20, 200, 90))
        add(abi.PRIM_THICK_LINE, 30, 3, 30, h - 4, size=t, blend=abi.ERASE)
        add(abi.PRIM_THICK_LINE, 11, 11, 11, 11, size=t)                      # equal end points
        add(abi.PRIM_THICK_LINE, -B, -7, B - 1, 9, size=t)
        add(abi.PRIM_THICK_LINE, -20, -30, 14, 12, size=t, rgb=(5, 5, 250))  # negative corners
    for k in (abi.PRIM_RECT, abi.PRIM_FILLED_RECT):
        add(k, w - 3, h - 2, 4, 6); add(k, 9, 9, 9, 9); add(k, -B, -B, B - 1, 2, blend=abi.ERASE); add(k, -5, h // 2, w + 5, h // 2 + 1)
    add(abi.PRIM_FILLED_RECT, (1 << 31) - 1, 0, -(1 << 31), h - 1)                  # (any i32)
    for mode in range(6):
        for blend in (abi.OPAQUE, abi.ERASE):
            add(abi.PRIM_LINE_BLENDED, 2, 2 + 3 * mode + blend, w - 2, h - 20 + mode, rgb=(250, 128, 3), blend=blend, mode=mode)
            add(abi.PRIM_LINE_BLENDED, 40 + mode, 4 + blend, 40 + mode, 4 + blend, rgb=(90, 90, 90), blend=blend, mode=mode)
    for a in (0, 255):
        add(abi.LINE_2D_ALPHA, 1, h - 1, w - 1, 1, alpha=a)
        add(abi.PRIM_CIRCLE_ALPHA, w // 2, h // 3, size=4, alpha=a, rgb=(255, 255, 255))
    return np.concatenate(recs)


def draw_ok(fb, base_px, zb, prims, before_z=None):
    """Draws `prims` on the GPU framebuffer (holding base_px / zb) and compares with np_prims."""
    want = base_px.copy()
    np_prims(want, zb, fb.width, fb.height, prims)
    fb.draw_prims(prims)
    got = fb.pixels
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    if before_z is not None:
        assert np.array_equal(fb.zbuffer.view(np.uint32), np.asarray(before_z, f32).view(np.uint32)), "the z-buffer changed"
    return got


# ---------------------------------------------------------------- CPU
def test_prim_layout_matches_c():
    """B32Prim compiled with gcc against the public header has the layout of abi.PRIM_DTYPE, and the kinds match."""
    fields = ("x0", "y0", "x1", "y1", "z0", "z1", "size", "r", "g", "b", "blend", "kind", "alpha", "mode", "_pad")
    kinds = ("B32_PRIM_LINE_BLENDED", "B32_PRIM_CIRCLE", "B32_PRIM_CIRCLE_ALPHA", "B32_PRIM_THICK_LINE", "B32_PRIM_RECT", "B32_PRIM_FILLED_RECT")
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void){ printf("%zu", sizeof(B32Prim));'
            + "".join(f' printf(" %zu", offsetof(B32Prim, {f}));' for f in fields)
            + "".join(f' printf(" %u", {k});' for k in kinds) + ' printf(" %u\\n", B32_ROUTE_PRIM_TILES); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == abi.PRIM_DTYPE.itemsize == 40
    assert out[1:1 + len(fields)] == [abi.PRIM_DTYPE.fields[f][1] for f in fields]
    assert out[1 + len(fields):-1] == [abi.PRIM_LINE_BLENDED, abi.PRIM_CIRCLE, abi.PRIM_CIRCLE_ALPHA, abi.PRIM_THICK_LINE, abi.PRIM_RECT,
                                       abi.PRIM_FILLED_RECT] == list(range(5, 11))
    assert out[-1] == 16384
    from bonnie32_amd import rasterizer as R
    assert R.Context.ROUTE_PRIM_TILES == 16384 and R.Context.ROUTES[-2:] == ("prim_tiles", "prim_scan")


def test_prim_model_pinned_to_oracle(oracle):
    """ref_prim's draw_rect edges, thickness <= 1 thick lines and Opaque LINE_BLENDED reproduce b32o_draw_line byte for byte."""
    L = _oracle_line_fns(oracle)
    W, H = 96, 64
    rng = np.random.default_rng(11)
    P = random_prims(rng, 1500, W, H, kinds=(abi.PRIM_LINE_BLENDED, abi.PRIM_THICK_LINE, abi.PRIM_RECT), max_len=90)
    P["blend"] = abi.OPAQUE; P["mode"] = abi.OPAQUE                 # (the oracle's lines always write alpha 255)
    P["size"] = np.where(P["kind"] == abi.PRIM_THICK_LINE, rng.integers(-3, 2, len(P)), P["size"])
    got = np.zeros(W * H * 4, np.uint8); want = np.zeros(W * H * 4, np.uint8)

    def line(a, b_, c, d, p):
        assert L.b32o_draw_line(want.ctypes.data, W, H, a, b_, c, d, int(p["r"]), int(p["g"]), int(p["b"])) == 0

    for p in P:
        ref_prim(got, None, W, H, p)
        x0, y0, x1, y1 = int(p["x0"]), int(p["y0"]), int(p["x1"]), int(p["y1"])
        if p["kind"] == abi.PRIM_RECT:
            mnx, mxx, mny, mxy = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
            for e in ((mnx, mny, mxx, mny), (mxx, mny, mxx, mxy), (mxx, mxy, mnx, mxy), (mnx, mxy, mnx, mny)):
                line(*e, p)
        else:
            line(x0, y0, x1, y1, p)
    assert np.array_equal(got, want)


def test_prim_model_hand_cases():
    """Cases computed by hand: a radius-1 circle (a 3x3 plus), the -0.0 perpendicular of a horizontal thick line, and the `as i32` box of
    a thick line with negative corners (truncation toward zero: -0.7 -> 0)."""
    W, H = 8, 6
    px = np.zeros(W * H * 4, np.uint8)
    ref_draw_circle(px, W, H, 3, 2, 1, (9, 8, 7), abi.OPAQUE)
    img = px.reshape(H, W, 4)
    assert [(y, x) for y, x in zip(*np.nonzero(img[:, :, 3]))] == [(1, 3), (2, 2), (2, 3), (2, 4), (3, 3)]
    assert tuple(img[2, 3]) == (9, 8, 7, 255)
    ref_draw_circle(px, W, H, 6, 4, -1, (1, 1, 1), abi.OPAQUE)   # negative radius: nothing
    ref_draw_circle(px, W, H, 6, 4, 0, (1, 2, 3), abi.ERASE)     # radius 0: the centre, alpha 0 (Erase)
    assert tuple(img[4, 6]) == (1, 2, 3, 0) and int((img[:, :, 3] > 0).sum()) == 5
    c = thick_corners(0, 2, 5, 2, 2)                             # dy = 0: px = -0.0 * ... = -0.0, py = 1
    ppx = -f32(0.0) / f32(5.0) * f32(1.0)
    assert ppx == 0.0 and np.signbit(ppx)
    assert c == [(f32(0.0), f32(3.0)), (f32(0.0), f32(1.0)), (f32(5.0), f32(1.0)), (f32(5.0), f32(3.0))]
    px = np.zeros(W * H * 4, np.uint8)
    ref_draw_thick_line(px, W, H, 0, 2, 5, 2, 2, (50, 60, 70), abi.OPAQUE)
    rows = np.nonzero(px.reshape(H, W, 4)[:, :, 3].any(1))[0]
    assert list(rows) == [1, 2] and px.reshape(H, W, 4)[1:3, :5, 3].all() and not px.reshape(H, W, 4)[:, 5:, 3].any()   # centres 0.5 .. 4.5
    c = thick_corners(-1, 0, 4, 0, 2)                            # corners (-1, +-1), (4, +-1): the box is x -1..4, y -1..1
    assert thick_box(c, W, H) == (0, 4, 0, 1)
    c = thick_corners(0, 0, 3, 4, 3)                             # px = -4/5*1.5 = -1.2, py = 0.9: min x = -1.2 -> -1 -> 0, min y = -0.9 -> 0
    assert -1.3 < c[0][0] < -1.1 and -1.0 < c[1][1] < -0.8 and max(q[0] for q in c) < 5.0 and max(q[1] for q in c) < 5.0
    assert thick_box(c, W, H) == (0, 4, 0, 4)
    px = np.zeros(W * H * 4, np.uint8)
    ref_draw_thick_line(px, W, H, 0, 0, 3, 4, 3, (1, 1, 1), abi.OPAQUE)
    assert px.reshape(H, W, 4)[0, 0, 3] == 255 and px.reshape(H, W, 4)[4, 0, 3] == 0
    assert _as_i32(f32(-0.7)) == 0 and _as_i32(f32(-1.7)) == -1 and _as_i32(f32(3e9)) == 2147483647 and _as_i32(f32(-3e9)) == -2147483648


def test_vectorised_prim_model_equals_literal_model():
    """np_prims (each primitive vectorised, runs of lines at once) == ref_prim called in order: random mixed batches of every kind and
    the edge cases."""
    W, H = 80, 48
    rng = np.random.default_rng(17)
    zb = rng.uniform(0.0, 1000.0, W * H).astype(f32)
    base = rng.integers(0, 256, W * H * 4).astype(np.uint8)
    batches = [random_prims(rng, 900, W, H, zrange=(-50.0, 1050.0)), edge_prims(W, H, far=3000)]
    mix = np.concatenate([random_prims(rng, 200, W, H), edge_prims(W, H, far=3000)])
    batches.append(mix[rng.permutation(len(mix))])
    for P in batches:
        for z in (zb, None):
            got = base.copy(); want = base.copy()
            np_prims(got, z, W, H, P)
            with np.errstate(invalid="ignore", over="ignore"):
                for p in P:
                    ref_prim(want, z, W, H, p)
            assert np.array_equal(got, want)


def test_cpp_mirror_prims_compile():
    """host/rasterizer.hpp: the new Framebuffer methods and the PrimBatch builder compile (header-only over the C ABI)."""
    hpp_dir = os.path.join(ROOT, "bonnie-32_amd", "host")
    src = ('#include "rasterizer.hpp"\nvoid f(b32::Framebuffer& fb) { b32::Color c{ 1, 2, 3, b32::BlendMode::Erase };\n'
           ' fb.draw_circle(1, 2, 3, c); fb.draw_circle_alpha(1, 2, 3, c, 140); fb.draw_thick_line(0, 0, 9, 9, 3, c); fb.draw_rect(0, 0, 4, 4, c);\n'
           ' fb.draw_filled_rect(0, 0, 4, 4, c); fb.draw_line_blended(0, 0, 4, 4, c, b32::BlendMode::Add);\n'
           ' fb.draw_prims(std::vector<B32Prim>{ b32::Framebuffer::prim(B32_PRIM_CIRCLE, 1, 1, 0, 0, c, 3) });\n'
           ' b32::PrimBatch b(fb); b.draw_line_3d_alpha(0, 0, 1.0f, 5, 5, 2.0f, c, 191); b.draw_circle_alpha(3, 3, 3, c, 140);\n'
           ' b.draw_circle(4, 4, 5, c); b.draw_thick_line(0, 0, 5, 9, 3, c); b.draw_rect(0, 0, 1, 1, c); b.draw_filled_rect(0, 0, 1, 1, c);\n'
           ' b.draw_line(0, 0, 1, 1, c); b.draw_line_alpha(0, 0, 1, 1, c, 9); b.draw_line_3d(0, 0, 1.0f, 1, 1, 1.0f, c);\n'
           ' b.draw_line_3d_overlay(0, 0, 1.0f, 1, 1, 1.0f, c); b.draw_line_blended(0, 0, 1, 1, c, b32::BlendMode::Subtract);\n'
           ' b.set_pixel(1, 1, c); b.set_pixel_alpha(1, 1, c, 3); b.set_pixel_blended(1, 1, c, b32::BlendMode::Erase);\n'
           ' if (b.size() == 16) b.flush(); }\nint main() { (void)&f; return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", hpp_dir, "-I", os.path.join(ROOT, "include"),
                        os.path.join(d, "t.cpp")], check=True)


def test_python_batch_builder_records():
    """PrimBatch records the Framebuffer methods in call order, with the pixel mappings of the header."""
    from bonnie32_amd import rasterizer as R
    b = R.PrimBatch(None)
    c = b32.Color(1, 2, 3, abi.ERASE)
    b.draw_circle_alpha(5, 6, 3, c, 140); b.draw_thick_line(0, 1, 2, 3, 4, c); b.set_pixel(7, 8, c); b.set_pixel_alpha(1, 2, c, 9)
    b.set_pixel_blended(3, 4, c, abi.ADD); b.draw_line_3d_alpha(0, 0, 1.5, 9, 9, 2.5, c, 191)
    P = b.records()
    assert list(P["kind"]) == [abi.PRIM_CIRCLE_ALPHA, abi.PRIM_THICK_LINE, abi.PRIM_FILLED_RECT, abi.LINE_2D_ALPHA, abi.PRIM_LINE_BLENDED, abi.LINE_3D_ALPHA]
    assert (P[0]["x0"], P[0]["y0"], P[0]["size"], P[0]["alpha"]) == (5, 6, 3, 140) and P[1]["size"] == 4
    assert (P[2]["x0"], P[2]["y0"], P[2]["x1"], P[2]["y1"]) == (7, 8, 7, 8) and P[4]["mode"] == abi.ADD and P[5]["z1"] == f32(2.5)
    assert (P["blend"] == abi.ERASE).all() and (P["r"] == 1).all()


# ---------------------------------------------------------------- GPU
def _zframe(oracle, scene="C1", **kw):
    from bonnie32_amd import scenegen
    sc = scenegen.make_scene(scene, **kw)
    sc.settings.use_zbuffer = True
    ofb = oracle.Framebuffer(sc.width, sc.height)
    ofb.clear(sc.clear_color)
    assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)[0] == 0
    return sc, ofb


def _render(fb, sc):
    from bonnie32_amd import rasterizer as R
    fb.clear(sc.clear_color)
    R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)


@pytest.mark.gpu
def test_gpu_prims_every_kind(gpu_ctx, oracle):
    """Random batches of every kind (and the edge cases) over a rendered z-buffer frame, at 320x240 and 2560x1920, small and copied."""
    from bonnie32_amd import rasterizer as R
    rng = np.random.default_rng(31)
    for scene, kw in (("C1", {}), ("C3", {"n_tris": 100_000})):
        sc, ofb = _zframe(oracle, scene, **kw)
        W, H = sc.width, sc.height
        fb = R.Framebuffer(W, H, gpu_ctx)
        for P in (random_prims(rng, 40, W, H), random_prims(rng, 3000, W, H, max_len=120, max_r=40), edge_prims(W, H)):
            _render(fb, sc)
            draw_ok(fb, ofb.pixels, ofb.zbuffer, P, ofb.zbuffer)


@pytest.mark.gpu
def test_gpu_prims_order(gpu_ctx):
    """Alpha circles and alpha lines on the same pixels in both orders, a late opaque shape hiding earlier blends, PS1 modes reading what
    came before: small and copied batches."""
    from bonnie32_amd import rasterizer as R
    W, H = 320, 240
    fb = R.Framebuffer(W, H, gpu_ctx)
    rng = np.random.default_rng(44)
    zb = rng.uniform(0.0, 2000.0, W * H).astype(f32)
    for n in (40, 600):
        P = random_prims(rng, n, W, H, kinds=(abi.LINE_2D_ALPHA, abi.LINE_3D_ALPHA, abi.PRIM_CIRCLE_ALPHA, abi.PRIM_LINE_BLENDED,
                                              abi.PRIM_CIRCLE, abi.PRIM_THICK_LINE), max_len=30, max_r=8)
        P["x0"] = rng.integers(140, 180, n); P["y0"] = rng.integers(100, 140, n)
        P["x1"] = rng.integers(140, 180, n); P["y1"] = rng.integers(100, 140, n)
        P["mode"] = rng.integers(1, 5, n)
        P[-1]["kind"] = abi.PRIM_FILLED_RECT; P[-1]["x0"], P[-1]["y0"], P[-1]["x1"], P[-1]["y1"] = 150, 110, 170, 130
        results = []
        for prims in (P, P[::-1].copy()):
            fb.clear(b32.Color(12, 200, 90))
            _upload_zbuffer(fb, zb)
            results.append(draw_ok(fb, fb.pixels, zb, prims, zb))
        assert not np.array_equal(results[0], results[1])
        img = results[0].reshape(H, W, 4)
        assert (img[110:131, 150:171, :3] == [P[-1]["r"], P[-1]["g"], P[-1]["b"]]).all()   # the late opaque rect hides the blends


def modeler_overlay(sc, w, h):
    """The modeler's overlay (modeler/viewport.rs:1943-1955 and the hover / selection around it) over the mesh: edges as LINE_3D_ALPHA 191,
    a CIRCLE_ALPHA r=3 alpha 140 dot per vertex, a hover CIRCLE r=5, THICK_LINE 3 selection edges -- in one batch."""
    from bonnie32_amd import rasterizer as R
    pos = sc.vertices["pos"]
    scr = [_project(sc.camera, p, w, h) for p in pos]
    b = R.PrimBatch(None)
    edges = set()
    for f in sc.faces["v"]:
        for a_, b_ in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            edges.add((min(a_, b_), max(a_, b_)))
    edges = sorted(edges)
    edge_c, dot_c = b32.Color(255, 200, 60), b32.Color(80, 220, 255)
    for a_, b_ in edges:
        if scr[a_] and scr[b_]:
            b.draw_line_3d_alpha(scr[a_][0], scr[a_][1], scr[a_][2], scr[b_][0], scr[b_][1], scr[b_][2], edge_c, 191)
    for s in scr:
        if s:
            b.draw_circle_alpha(s[0], s[1], 3, dot_c, 140)
    vis = [s for s in scr if s]
    b.draw_circle(vis[len(vis) // 2][0], vis[len(vis) // 2][1], 5, b32.Color(255, 255, 0))
    for a_, b_ in edges[:: max(1, len(edges) // 12)]:
        if scr[a_] and scr[b_]:
            b.draw_thick_line(scr[a_][0], scr[a_][1], scr[b_][0], scr[b_][1], 3, b32.Color(255, 128, 0))
    return b.records()


def _golden_scene(name="obj-crawler.b32scene"):
    """A real mesh object (the modeler's subject) from the golden scenes."""
    from bonnie32_amd import scenefile
    return scenefile.read_scene(os.path.join(ROOT, "tests", "golden", "scenes", "real", name))


@pytest.mark.gpu
def test_gpu_prims_modeler_overlay(gpu_ctx, oracle):
    """The modeler overlay on a real golden scene as one batch; then the same calls one method at a time through the Python mirror give
    the same frame."""
    from bonnie32_amd import rasterizer as R
    sc = _golden_scene()
    W, H = sc.width, sc.height
    ofb = oracle.Framebuffer(W, H)
    ofb.clear(sc.clear_color)
    assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)[0] == 0
    P = modeler_overlay(sc, W, H)
    assert (P["kind"] == abi.PRIM_CIRCLE_ALPHA).sum() > 200 and (P["kind"] == abi.LINE_3D_ALPHA).sum() > 500
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(sc.clear_color)
    R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
    got = draw_ok(fb, ofb.pixels, ofb.zbuffer, P, ofb.zbuffer)
    assert not np.array_equal(got, ofb.pixels)
    fb.upload(ofb.pixels)
    for p in P:                                                  # one call per method
        c = b32.Color(int(p["r"]), int(p["g"]), int(p["b"]), int(p["blend"]))
        k = int(p["kind"])
        if k == abi.LINE_3D_ALPHA:
            fb.draw_line_3d_alpha(int(p["x0"]), int(p["y0"]), float(p["z0"]), int(p["x1"]), int(p["y1"]), float(p["z1"]), c, int(p["alpha"]))
        elif k == abi.PRIM_CIRCLE_ALPHA:
            fb.draw_circle_alpha(int(p["x0"]), int(p["y0"]), int(p["size"]), c, int(p["alpha"]))
        elif k == abi.PRIM_CIRCLE:
            fb.draw_circle(int(p["x0"]), int(p["y0"]), int(p["size"]), c)
        else:
            fb.draw_thick_line(int(p["x0"]), int(p["y0"]), int(p["x1"]), int(p["y1"]), int(p["size"]), c)
    assert np.array_equal(fb.pixels, got)


@pytest.mark.gpu
def test_gpu_prims_lines_equal_draw_lines(gpu_ctx):
    """A batch of only kinds 0-4 through b32_draw_prims gives the bytes b32_draw_lines gives for the same records."""
    from bonnie32_amd import rasterizer as R
    W, H = 640, 480
    fb = R.Framebuffer(W, H, gpu_ctx)
    rng = np.random.default_rng(5)
    zb = rng.uniform(0.0, 3000.0, W * H).astype(f32)
    for n in (30, 5000):
        P = random_prims(rng, n, W, H, kinds=(0, 1, 2, 3, 4), max_len=200)
        out = []
        for via in ("prims", "lines"):
            fb.clear(b32.Color(20, 30, 40))
            _upload_zbuffer(fb, zb)
            fb.draw_prims(P) if via == "prims" else fb.draw_lines(to_lines(P))
            out.append(fb.pixels)
        assert np.array_equal(out[0], out[1])


@pytest.mark.gpu
def test_gpu_prims_routes_and_fallback(oracle):
    """100k mixed primitives on the tile route and scanned; more than 1024 on one tile (its list overflows); more than 1024 screen-sized
    ones (the long list overflows).  Each asserts the route it took."""
    from bonnie32_amd import rasterizer as R
    sc, ofb = _zframe(oracle, "C3", n_tris=100_000)
    W, H = sc.width, sc.height
    rng = np.random.default_rng(100)
    big = random_prims(rng, 100_000, W, H, max_len=40, max_r=10)
    dense = random_prims(rng, 3000, W, H, max_len=30, max_r=5)
    dense["x0"] = rng.integers(600, 664, len(dense)); dense["x1"] = rng.integers(600, 664, len(dense))
    dense["y0"] = rng.integers(800, 816, len(dense)); dense["y1"] = rng.integers(800, 816, len(dense))
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        for routes in (0, R.Context.ROUTE_PRIM_TILES):
            ctx.set_routes(routes)
            for P in (big, dense):
                _render(fb, sc)
                c0 = ctx.route_counts()
                draw_ok(fb, ofb.pixels, ofb.zbuffer, P, ofb.zbuffer)
                key = "prim_tiles" if routes == 0 else "prim_scan"
                assert ctx.route_counts()[key] == c0[key] + 1
        ctx.set_routes(0)
        W2, H2 = 320, 240                                        # the long list overflows: 1100 screen-sized primitives
        fb2 = R.Framebuffer(W2, H2, ctx)
        L = random_prims(rng, 1400, W2, H2, kinds=(abi.PRIM_FILLED_RECT, abi.PRIM_CIRCLE, abi.PRIM_CIRCLE_ALPHA, abi.LINE_2D_ALPHA))
        scr = (L["kind"] != abi.LINE_2D_ALPHA)
        L["size"] = np.where(scr, 2000, 0)
        L["x0"] = np.where(L["kind"] == abi.PRIM_FILLED_RECT, -10, L["x0"]); L["y0"] = np.where(L["kind"] == abi.PRIM_FILLED_RECT, -10, L["y0"])
        L["x1"] = np.where(L["kind"] == abi.PRIM_FILLED_RECT, W2 + 10, L["x1"]); L["y1"] = np.where(L["kind"] == abi.PRIM_FILLED_RECT, H2 + 10, L["y1"])
        assert scr.sum() > 1024
        fb2.clear(b32.Color(1, 2, 3))
        c0 = ctx.route_counts()["prim_tiles"]
        draw_ok(fb2, fb2.pixels, None, L)
        assert ctx.route_counts()["prim_tiles"] == c0 + 1
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_prims_bands_and_pipeline(gpu_ctx, oracle):
    """Only rows of the band are written; with two frames in flight, primitives between b32_frame_submit and b32_fb_download_async give
    exact delivered frames."""
    from bonnie32_amd import rasterizer as R, scenegen
    W, H = 640, 480
    fb = R.Framebuffer(W, H, gpu_ctx)
    rng = np.random.default_rng(4)
    zb = rng.uniform(0.0, 3000.0, W * H).astype(f32)
    for n in (40, 3000):
        P = random_prims(rng, n, W, H, max_len=200, max_r=30)
        fb.set_band(0, H)
        fb.clear(b32.Color(9, 9, 9))
        _upload_zbuffer(fb, zb)
        base = fb.pixels
        want = base.copy(); np_prims(want, zb, W, H, P)
        for band in ((0, 100), (100, 333), (333, 334), (334, H)):
            fb.set_band(*band)
            fb.draw_prims(P)
        fb.set_band(0, H)
        assert np.array_equal(fb.pixels, want)
        fb.upload(base)
        fb.set_band(100, 333)
        fb.draw_prims(P)
        fb.set_band(0, H)
        part = base.reshape(H, -1).copy(); part[100:333] = want.reshape(H, -1)[100:333]
        assert np.array_equal(fb.pixels, part.reshape(-1))
    ctx = R.Context(0)
    try:
        st = b32.RasterSettings.game()
        meshes = [scenegen.make_scene("C1", n_tris=800, seed=300 + i, variant="gouraud") for i in range(3)]
        W, H = meshes[0].width, meshes[0].height
        fb2 = R.Framebuffer(W, H, ctx)
        slots = [R.ResidentScene(fb2, m.vertices, m.faces, m.textures).detach() for m in meshes]
        table = ctx.make_frame_table(meshes[0].camera, st, slots)
        bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
        frames = [(random_prims(rng, 36, W, H), random_prims(rng, 700, W, H)) for _ in range(4)]
        want = []
        for small, large in frames:
            o = oracle.Framebuffer(W, H); o.clear(b32.Color(10, 10, 30))
            for m in meshes:
                assert oracle.render_mesh_15(o, m.vertices, m.faces, m.textures, meshes[0].camera, st)[0] == 0
            px = o.pixels.copy(); np_prims(px, o.zbuffer, W, H, small); np_prims(px, o.zbuffer, W, H, large)
            want.append(px)
        tickets = []
        for i, (small, large) in enumerate(frames):
            fb2.clear(b32.Color(10, 10, 30))
            ctx.frame_submit(table)
            for prims in (small, large):
                arr = prims.copy()
                fb2.draw_prims(arr)
                arr[:] = random_prims(rng, len(arr), W, H)        # the caller reuses its array at once
            tickets.append(ctx.download_async(bufs[i & 1][1]))
            if i >= 1:
                ctx.ticket_wait(tickets[i - 1])
                assert np.array_equal(bufs[(i - 1) & 1][0], want[i - 1]), f"frame {i - 1}"
        ctx.ticket_wait(tickets[-1])
        assert np.array_equal(bufs[(len(frames) - 1) & 1][0], want[-1])
        ctx.finish()
        for _, p in bufs:
            ctx.host_free(p)
        for s in slots:
            s.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_prims_validation(gpu_ctx):
    """An unknown kind, a bad mode, oversize extents or radii: the right error code, and the framebuffer unchanged (small and copied)."""
    from bonnie32_amd import rasterizer as R
    W, H = 200, 150
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(b32.Color(1, 2, 3))
    rng = np.random.default_rng(8)
    base = fb.pixels
    good = random_prims(rng, 30, W, H)
    B30 = 1 << 30
    cases = []
    for f, v, code in ((("kind",), 11, abi.B32_E_ARG), (("kind",), 255, abi.B32_E_ARG)):
        cases.append(({f[0]: v}, code))
    cases += [({"kind": abi.PRIM_LINE_BLENDED, "mode": 6}, abi.B32_E_ARG)]
    for k in (0, 3, abi.PRIM_LINE_BLENDED, abi.PRIM_THICK_LINE, abi.PRIM_RECT):
        cases += [({"kind": k, "x0": 0, "x1": B30, "size": 1}, abi.B32_E_UNSUPPORTED), ({"kind": k, "y0": -5, "y1": B30 - 5, "size": 4}, abi.B32_E_UNSUPPORTED)]
    for k in (abi.PRIM_CIRCLE, abi.PRIM_CIRCLE_ALPHA):
        cases += [({"kind": k, "x0": 5, "y0": 5, "size": 32768}, abi.B32_E_UNSUPPORTED), ({"kind": k, "x0": 5, "y0": 5, "size": -32768}, abi.B32_E_UNSUPPORTED),
                  ({"kind": k, "x0": B30, "y0": 5, "size": 1}, abi.B32_E_UNSUPPORTED), ({"kind": k, "x0": 5, "y0": -B30, "size": 1}, abi.B32_E_UNSUPPORTED)]
    for n in (30, 300):
        batch = np.concatenate([good] * (n // 30))
        for fields, code in cases:
            bad = batch.copy()
            for f, v in fields.items():
                bad[n // 2][f] = v
            with pytest.raises(R.B32Error) as e:
                fb.draw_prims(bad)
            assert e.value.code == code, fields
    ok = np.zeros(3, abi.PRIM_DTYPE)                             # accepted: FILLED_RECT takes any i32, radius +-32767, |centre| < 2^30
    ok["kind"] = [abi.PRIM_FILLED_RECT, abi.PRIM_CIRCLE, abi.PRIM_CIRCLE_ALPHA]
    ok["x0"] = [-(1 << 31), B30 - 1, -(B30 - 1)]; ok["x1"] = [(1 << 31) - 1, 0, 0]; ok["size"] = [0, 32767, -32767]
    fb.draw_prims(ok[1:])
    fb.draw_prims(good[:0])
    assert np.array_equal(fb.pixels, base)                       # nothing of a rejected batch (nor the off-screen circles) was drawn
    fb.draw_prims(ok[:1])
