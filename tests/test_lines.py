"""The Framebuffer line family (render.rs:684-872) through b32_draw_lines.

Expected images: the oracle's b32o_draw_line / b32o_draw_line_3d where it has an entry, and for the overlay and alpha kinds the literal
restatement below (`ref_line`), which is pinned to the oracle byte for byte on CPU.  Large batches use `np_lines`, a vectorised form of the
same walk (closed-form Bresenham, sequential fold per pixel), pinned to `ref_line` on CPU.  Every GPU case is compared with the sequential
CPU result, pixels and z-buffer."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FMAX = np.finfo(np.float32).max
KINDS = (abi.LINE_2D, abi.LINE_2D_ALPHA, abi.LINE_3D, abi.LINE_3D_OVERLAY, abi.LINE_3D_ALPHA)


# ---------------------------------------------------------------- CPU models
def _set_pixel(px, w, x, y, rgb, blend):                       # render.rs:300-309, Color::to_bytes (types.rs:829-832)
    i = (y * w + x) * 4
    px[i:i + 3] = rgb
    px[i + 3] = 0 if blend == abi.ERASE else 255


def _set_pixel_alpha(px, w, x, y, rgb, alpha):                 # render.rs:646-667
    i = (y * w + x) * 4
    a = int(alpha); inv = 255 - a
    for c in range(3):
        px[i + c] = (int(rgb[c]) * a + int(px[i + c]) * inv) // 255
    px[i + 3] = 255


def ref_line(px, zb, w, h, l):
    """One reference call, literally: draw_line_blended(Opaque) render.rs:715-755, draw_line_alpha :684-711, draw_line_3d_impl :768-817
    (allow_equal false / true), draw_line_3d_alpha :822-872.  px: flat RGBA bytes (modified), zb: flat f32 or None (= f32::MAX)."""
    x0, y0, x1, y1 = int(l["x0"]), int(l["y0"]), int(l["x1"]), int(l["y1"])
    kind, rgb, blend, alpha = int(l["kind"]), (int(l["r"]), int(l["g"]), int(l["b"])), int(l["blend"]), int(l["alpha"])
    z0, z1 = f32(l["z0"]), f32(l["z1"])
    if kind == abi.LINE_3D_ALPHA:
        z0, z1 = z0 * f32(0.995), z1 * f32(0.995)             # DEPTH_BIAS
    dx = abs(x1 - x0); dy = -abs(y1 - y0)
    sx = 1 if x0 < x1 else -1; sy = 1 if y0 < y1 else -1
    err = dx + dy; x, y = x0, y0
    total = f32(max(dx, max(-dy, 1)))
    step = f32(0.0)
    while True:
        if 0 <= x < w and 0 <= y < h:
            if kind in (abi.LINE_2D, abi.LINE_2D_ALPHA):
                passes = True
            else:
                t = step / total
                z = z0 + t * (z1 - z0)
                d = f32(FMAX) if zb is None else zb[y * w + x]
                passes = bool(z < d) if kind == abi.LINE_3D else bool(z <= d)
            if passes:
                if kind in (abi.LINE_2D_ALPHA, abi.LINE_3D_ALPHA):
                    _set_pixel_alpha(px, w, x, y, rgb, alpha)
                else:
                    _set_pixel(px, w, x, y, rgb, blend)
        if x == x1 and y == y1:
            break
        e2 = 2 * err
        if e2 >= dy:
            err += dy; x += sx; step = step + f32(1.0)
        if e2 <= dx:
            err += dx; y += sy
            if e2 < dy:
                step = step + f32(1.0)


def np_lines(px, zb, w, h, lines):
    """The sequential result of `lines` (in order) on px (flat RGBA, modified in place): every on-screen step from the closed form
    (tests/test_oracle_kats.py pins it to the loop), depth tests vectorised (the z-buffer is only read), then the colour writes folded
    per pixel in line order."""
    L = np.ascontiguousarray(lines, abi.LINE_DTYPE).reshape(-1)
    if not len(L):
        return
    x0, y0, x1, y1 = (L[k].astype(np.int64) for k in ("x0", "y0", "x1", "y1"))
    adx, ady = np.abs(x1 - x0), np.abs(y1 - y0)
    sx = np.where(x0 < x1, 1, -1); sy = np.where(y0 < y1, 1, -1)
    xm = adx >= ady
    N = np.maximum(adx, ady)
    m0 = np.where(xm, x0, y0); sm = np.where(xm, sx, sy); lim = np.where(xm, w - 1, h - 1)
    # steps whose major coordinate is on screen
    klo = np.where(sm > 0, -m0, m0 - lim); khi = np.where(sm > 0, lim - m0, m0)
    klo = np.maximum(klo, 0); khi = np.minimum(khi, N)
    cnt = np.maximum(khi - klo + 1, 0)
    idx = np.repeat(np.arange(len(L)), cnt)
    start = np.cumsum(cnt) - cnt
    k = klo[idx] + (np.arange(int(cnt.sum())) - start[idx])
    dmaj = np.where(xm, adx, ady)[idx]; dmin = np.where(xm, ady, adx)[idx]
    j = np.where(dmaj > 0, (2 * dmin * k + dmaj) // np.maximum(2 * dmaj, 1), 0)
    maj = m0[idx] + sm[idx] * k
    mnr = np.where(xm, y0, x0)[idx] + np.where(xm, sy, sx)[idx] * j
    X = np.where(xm[idx], maj, mnr); Y = np.where(xm[idx], mnr, maj)
    on = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
    idx, k, X, Y = idx[on], k[on], X[on], Y[on]
    kind = L["kind"][idx].astype(np.int64)
    z0 = L["z0"][idx].astype(f32); z1 = L["z1"][idx].astype(f32)
    bias = kind == abi.LINE_3D_ALPHA
    z0 = np.where(bias, z0 * f32(0.995), z0).astype(f32); z1 = np.where(bias, z1 * f32(0.995), z1).astype(f32)
    step = np.minimum(k, 1 << 24).astype(f32)
    t = (step / np.maximum(N[idx], 1).astype(f32)).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        z = (z0 + t * (z1 - z0)).astype(f32)
    pix = Y * w + X
    d = np.full(len(pix), FMAX, f32) if zb is None else zb[pix]
    with np.errstate(invalid="ignore"):
        keep = np.where(kind == abi.LINE_3D, z < d, np.where(kind >= abi.LINE_3D_OVERLAY, z <= d, True))
    idx, pix = idx[keep], pix[keep]
    if not len(pix):
        return
    order = np.argsort(pix, kind="stable")                      # per pixel, in line order
    pix, idx = pix[order], idx[order]
    first = np.r_[0, np.flatnonzero(np.diff(pix)) + 1]
    grp = np.repeat(first, np.diff(np.r_[first, len(pix)]))
    rank = np.arange(len(pix)) - grp
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2))
    img = px.reshape(-1, 4)
    rgb = np.stack([L["r"], L["g"], L["b"]], 1).astype(np.int64)
    alpha = L["alpha"].astype(np.int64)
    blend_kind = (L["kind"] == abi.LINE_2D_ALPHA) | (L["kind"] == abi.LINE_3D_ALPHA)
    abyte = np.where(L["blend"] == abi.ERASE, 0, 255)
    for r in range(rank.max() + 1):
        sel = by_rank[bounds[r]:bounds[r + 1]]
        p, li = pix[sel], idx[sel]
        bl = blend_kind[li]
        po, lo = p[~bl], li[~bl]
        img[po, :3] = rgb[lo]; img[po, 3] = abyte[lo]
        pb, lb = p[bl], li[bl]
        a = alpha[lb][:, None]
        img[pb, :3] = (rgb[lb] * a + img[pb, :3].astype(np.int64) * (255 - a)) // 255
        img[pb, 3] = 255


def random_lines(rng, n, w, h, max_len=64, kinds=KINDS, zrange=(0.0, 4000.0)):
    L = np.zeros(n, abi.LINE_DTYPE)
    L["x0"] = rng.integers(-40, w + 40, n); L["y0"] = rng.integers(-40, h + 40, n)
    L["x1"] = L["x0"] + rng.integers(-max_len, max_len + 1, n); L["y1"] = L["y0"] + rng.integers(-max_len, max_len + 1, n)
    L["z0"] = rng.uniform(*zrange, n).astype(f32); L["z1"] = rng.uniform(*zrange, n).astype(f32)
    L["r"], L["g"], L["b"] = (rng.integers(0, 256, n) for _ in range(3))
    L["blend"] = np.where(rng.random(n) < 0.1, abi.ERASE, abi.OPAQUE)
    L["kind"] = rng.choice(np.array(kinds, np.uint8), n)
    L["alpha"] = rng.choice(np.array([0, 1, 128, 191, 254, 255], np.uint8), n)
    return L


# ---------------------------------------------------------------- CPU
def test_line_layout_matches_c():
    """B32Line compiled with gcc against the public header has the layout of abi.LINE_DTYPE."""
    import subprocess, tempfile
    fields = ("x0", "y0", "x1", "y1", "z0", "z1", "r", "g", "b", "blend", "kind", "alpha", "_pad")
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void){ printf("%zu", sizeof(B32Line));'
            + "".join(f' printf(" %zu", offsetof(B32Line, {f}));' for f in fields)
            + ' printf(" %u %u %u %u %u\\n", B32_LINE_2D, B32_LINE_2D_ALPHA, B32_LINE_3D, B32_LINE_3D_OVERLAY, B32_LINE_3D_ALPHA); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = [int(v) for v in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == abi.LINE_DTYPE.itemsize == 32
    assert out[1:1 + len(fields)] == [abi.LINE_DTYPE.fields[f][1] for f in fields]
    assert out[1 + len(fields):] == list(KINDS)


def _oracle_line_fns(oracle):
    L = oracle.lib()
    P = C.c_void_p
    L.b32o_draw_line.restype = C.c_int
    L.b32o_draw_line.argtypes = [P, C.c_uint32, C.c_uint32] + [C.c_int32] * 4 + [C.c_uint8] * 3
    L.b32o_draw_line_3d.restype = C.c_int
    L.b32o_draw_line_3d.argtypes = [P, P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_float] + [C.c_uint8] * 3
    return L


def test_line_model_pinned_to_oracle(oracle):
    """ref_line with allow_equal = false and no alpha reproduces b32o_draw_line_3d / b32o_draw_line byte for byte (3 000 lines)."""
    L = _oracle_line_fns(oracle)
    W, H = 96, 64
    rng = np.random.default_rng(5)
    zb = rng.uniform(0.0, 1000.0, W * H).astype(f32)
    zb[rng.random(W * H) < 0.2] = FMAX
    lines = random_lines(rng, 3000, W, H, max_len=90, kinds=(abi.LINE_2D, abi.LINE_3D), zrange=(-100.0, 1100.0))
    lines["blend"] = abi.OPAQUE                                  # (the oracle's lines always write alpha 255)
    lines[::7]["z1"] = lines[::7]["z0"]
    for z in (zb, None):
        got = np.zeros(W * H * 4, np.uint8); want = np.zeros(W * H * 4, np.uint8)
        for l in lines:
            ref_line(got, z, W, H, l)
            if l["kind"] == abi.LINE_2D:
                rc = L.b32o_draw_line(want.ctypes.data, W, H, int(l["x0"]), int(l["y0"]), int(l["x1"]), int(l["y1"]), int(l["r"]), int(l["g"]), int(l["b"]))
            else:
                rc = L.b32o_draw_line_3d(want.ctypes.data, z.ctypes.data if z is not None else None, W, H, int(l["x0"]), int(l["y0"]), float(l["z0"]),
                                         int(l["x1"]), int(l["y1"]), float(l["z1"]), int(l["r"]), int(l["g"]), int(l["b"]))
            assert rc == 0
        assert np.array_equal(got, want)


def test_vectorised_model_equals_literal_model():
    """np_lines (whole batch at once) == ref_line called in order, every kind, Erase colours, NaN / inf depths, far endpoints."""
    W, H = 80, 48
    rng = np.random.default_rng(9)
    zb = rng.uniform(0.0, 1000.0, W * H).astype(f32)
    lines = random_lines(rng, 2500, W, H, max_len=70, zrange=(-50.0, 1050.0))
    lines[::11]["z0"] = np.nan; lines[5::13]["z1"] = np.inf; lines[3::17]["z0"] = -np.inf
    far = random_lines(rng, 40, W, H)
    far["x0"] = rng.integers(-(1 << 20), 1 << 20, 40); far["y1"] = rng.integers(-(1 << 16), 1 << 16, 40)
    lines = np.concatenate([lines, far])
    base = rng.integers(0, 256, W * H * 4).astype(np.uint8)
    for z in (zb, None):
        got = base.copy(); want = base.copy()
        np_lines(got, z, W, H, lines)
        with np.errstate(invalid="ignore", over="ignore"):
            for l in lines:
                ref_line(want, z, W, H, l)
        assert np.array_equal(got, want)


# ---------------------------------------------------------------- GPU
def _draw_check(fb, base_px, zb, lines, before_z=None):
    """Draws `lines` on the GPU framebuffer (holding base_px / zb) and compares pixels and z-buffer with the sequential CPU result."""
    want = base_px.copy()
    np_lines(want, zb, fb.width, fb.height, lines)
    fb.draw_lines(lines)
    got = fb.pixels
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    if before_z is not None:
        assert np.array_equal(fb.zbuffer.view(np.uint32), before_z.view(np.uint32)), "the z-buffer changed"
    return got


def _upload_zbuffer(fb, z):
    z = np.ascontiguousarray(z, f32).reshape(-1)
    assert fb.ctx.lib.b32_zbuffer_upload(fb.ctx.h, z.ctypes.data) == 0


def _real_game_scene():
    from bonnie32_amd import scenefile
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "scenes", "real", "*-game.b32scene")))
    assert paths
    return scenefile.read_scene(paths[0])


def _project(cam, p, w, h):
    """perspective_transform + a plain pinhole projection (the test needs plausible screen integers, not the reference's numerics)."""
    rel = np.asarray(p, np.float64) - np.asarray(cam.position)
    cx, cy, cz = (float(np.dot(rel, np.asarray(b))) for b in (cam.basis_x, cam.basis_y, cam.basis_z))
    if cz < 0.1:
        return None
    s = w * 0.75
    return int(cx / cz * s + w / 2), int(-cy / cz * s + h / 2), f32(cz)


def cylinder_lines(cam, w, h, center, radius, height, segments=12, rgb=(80, 255, 80)):
    """draw_wireframe_cylinder (game/renderer.rs:984-1050): bottom ring, top ring, every other vertical, all draw_line_3d."""
    ang = [(i / segments) * 2.0 * np.pi for i in range(segments)]
    bot = [_project(cam, (center[0] + radius * np.cos(a), center[1], center[2] + radius * np.sin(a)), w, h) for a in ang]
    top = [_project(cam, (center[0] + radius * np.cos(a), center[1] + height, center[2] + radius * np.sin(a)), w, h) for a in ang]
    segs = []
    for ring in ([p for p in bot if p], [p for p in top if p]):
        for i in range(len(ring)):
            segs.append((ring[i], ring[(i + 1) % len(ring)]))
    for i in range(0, segments, 2 if segments > 8 else 1):
        if bot[i] and top[i]:
            segs.append((bot[i], top[i]))
    L = np.zeros(len(segs), abi.LINE_DTYPE)
    for i, (a, b) in enumerate(segs):
        L[i]["x0"], L[i]["y0"], L[i]["z0"], L[i]["x1"], L[i]["y1"], L[i]["z1"] = a[0], a[1], a[2], b[0], b[1], b[2]
    L["r"], L["g"], L["b"], L["kind"] = rgb[0], rgb[1], rgb[2], abi.LINE_3D
    return L


def _room_cylinder(sc):
    cam = sc.camera
    fwd, up = np.asarray(cam.basis_z), np.asarray(cam.basis_y)
    center = np.asarray(cam.position) + 1800.0 * fwd - 500.0 * up
    return cylinder_lines(cam, sc.width, sc.height, center, 260.0, 900.0)


@pytest.mark.gpu
def test_gpu_lines_game_cylinder(gpu_ctx, oracle):
    from bonnie32_amd import rasterizer as R
    sc = _real_game_scene()
    ofb = oracle.Framebuffer(sc.width, sc.height)
    ofb.clear(sc.clear_color)
    rc, _ = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
    assert rc == 0
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    fb.clear(sc.clear_color)
    R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
    lines = _room_cylinder(sc)
    assert 20 <= len(lines) <= 64
    before = gpu_ctx.route_counts()["line_scan"]
    got = _draw_check(fb, ofb.pixels, ofb.zbuffer, lines, ofb.zbuffer)
    assert gpu_ctx.route_counts()["line_scan"] == before + 1
    assert not np.array_equal(got, ofb.pixels)                   # the cylinder is in view


@pytest.mark.gpu
def test_gpu_lines_equal_depths(gpu_ctx):
    from bonnie32_amd import rasterizer as R
    W, H = 256, 128
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(b32.Color(30, 40, 50))
    rng = np.random.default_rng(3)
    zrow = rng.uniform(1.0, 500.0, H).astype(f32); zcol = rng.uniform(-300.0, 500.0, W).astype(f32)
    zb = np.empty((H, W), f32)
    zb[:, :W // 2] = zrow[:, None]; zb[:, W // 2:] = zcol[None, W // 2:]         # left: constant rows, right: constant columns
    zb[0, :W // 2] = -np.inf; zb[1, :W // 2] = np.inf                      # (rows 0 / 1: lines at -inf / +inf)
    _upload_zbuffer(fb, zb)
    base = fb.pixels
    zf = zb.reshape(-1)
    L = []
    for y in range(H):                                           # horizontal lines at the row's depth
        L.append((4, y, W // 2 - 5, y, zrow[y] if y > 1 else zb[y, 0]))
    for x in range(W // 2, W, 3):                                # vertical lines at the column's depth
        L.append((x, 2, x, H - 3, zcol[x]))
    eq = np.zeros(len(L), abi.LINE_DTYPE)
    for i, (a, b_, c, d, z) in enumerate(L):
        eq[i]["x0"], eq[i]["y0"], eq[i]["x1"], eq[i]["y1"], eq[i]["z0"], eq[i]["z1"] = a, b_, c, d, z, z
    eq["r"], eq["g"], eq["b"] = 250, 20, 20
    for kind in (abi.LINE_3D, abi.LINE_3D_OVERLAY, abi.LINE_3D_ALPHA):
        fb.upload(base)
        lines = eq.copy(); lines["kind"] = kind; lines["alpha"] = 191
        got = _draw_check(fb, base, zf, lines, zf)
        changed = (got.reshape(H, W, 4) != base.reshape(H, W, 4)).any(2)
        on = np.zeros((H, W), bool)
        on[2:, 4:W // 2 - 4] = True
        for x in range(W // 2, W, 3):
            on[2:H - 2, x] = True
        if kind == abi.LINE_3D:
            assert not changed[on].any()                           # z == zbuffer: strictly-in-front draws none
        elif kind == abi.LINE_3D_OVERLAY:
            assert changed[on].all()                               # ... allow_equal draws all
    # NaN / +-inf / negative depths on a z-buffer of finite values
    fb.upload(base)
    sp = random_lines(rng, 600, W, H, kinds=(abi.LINE_3D, abi.LINE_3D_OVERLAY, abi.LINE_3D_ALPHA), zrange=(-600.0, 600.0))
    sp[::4]["z0"] = np.nan; sp[1::4]["z1"] = np.inf; sp[2::4]["z0"] = -np.inf; sp[3::8]["z1"] = -np.inf
    _draw_check(fb, base, zf, sp, zf)


@pytest.mark.gpu
def test_gpu_lines_order(gpu_ctx):
    from bonnie32_amd import rasterizer as R
    W, H = 320, 240
    fb = R.Framebuffer(W, H, gpu_ctx)
    rng = np.random.default_rng(21)
    zb = rng.uniform(0.0, 2000.0, W * H).astype(f32)
    for n in (48, 400):                                          # in the kernel argument / copied (tile route)
        L = random_lines(rng, n, W, H, max_len=30, zrange=(0.0, 1500.0))
        L["x0"] = rng.integers(140, 180, n); L["y0"] = rng.integers(100, 140, n)
        L["x1"] = rng.integers(140, 180, n); L["y1"] = rng.integers(100, 140, n)
        L["alpha"] = rng.choice(np.array([0, 191, 255], np.uint8), n)
        results = []
        for lines in (L, L[::-1].copy()):
            fb.clear(b32.Color(12, 200, 90))
            _upload_zbuffer(fb, zb)
            base = fb.pixels
            results.append(_draw_check(fb, base, zb, lines, zb))
        assert not np.array_equal(results[0], results[1])


@pytest.mark.gpu
def test_gpu_lines_geometry(gpu_ctx):
    from bonnie32_amd import rasterizer as R
    W, H = 200, 150
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(b32.Color(1, 2, 3))
    rng = np.random.default_rng(8)
    zb = rng.uniform(0.0, 100.0, W * H).astype(f32)
    _upload_zbuffer(fb, zb)
    base = fb.pixels
    B = 1 << 29
    geo = [(10, 10, 12, 140), (5, 70, 195, 72), (190, 140, 3, 7), (50, 50, 50, 50), (-5, -5, -5, -5), (120, 30, 120, 30),
           (-B, 75, B - 1, 80), (100, -B, 103, B - 1), (-B, -B, B - 1, B - 1), (B, 20, -B + 1, 100), (-B, 149, 300, 0),
           ((1 << 24) + 50, 10, -(1 << 24) + 10, 140)]             # (the last ones: far more than 2^24 steps, the depth parameter saturates)
    L = np.zeros(len(geo) * len(KINDS), abi.LINE_DTYPE)
    for i, (g, kind) in enumerate((g, k) for g in geo for k in KINDS):
        L[i]["x0"], L[i]["y0"], L[i]["x1"], L[i]["y1"] = g
        L[i]["kind"] = kind
    L["z0"] = rng.uniform(-10.0, 110.0, len(L)); L["z1"] = rng.uniform(-10.0, 110.0, len(L))
    L["r"], L["g"], L["b"], L["alpha"] = rng.integers(0, 256, len(L)), 200, rng.integers(0, 256, len(L)), 191
    got = _draw_check(fb, base, zb, L, zb)
    for big in (L, np.concatenate([L] * 8)):                   # (kernel argument / copied)
        bad = big.copy()
        bad[len(bad) // 2]["x1"] = bad[len(bad) // 2]["x0"] + (1 << 30)
        with pytest.raises(R.B32Error) as e:
            fb.draw_lines(bad)
        assert e.value.code == abi.B32_E_UNSUPPORTED
        bad = big.copy(); bad[-1]["kind"] = 5
        with pytest.raises(R.B32Error) as e:
            fb.draw_lines(bad)
        assert e.value.code == abi.B32_E_ARG
    fb.draw_lines(L[:0])
    assert np.array_equal(fb.pixels, got)                        # nothing of a rejected batch was drawn


def _big_zframe(oracle):
    from bonnie32_amd import scenegen
    sc = scenegen.make_scene("C3", n_tris=200_000)
    sc.settings.use_zbuffer = True
    ofb = oracle.Framebuffer(sc.width, sc.height)
    ofb.clear(sc.clear_color)
    rc, _ = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    assert rc == 0
    return sc, ofb


@pytest.mark.gpu
def test_gpu_lines_100k_tile_route_and_fallback(gpu_ctx, oracle):
    from bonnie32_amd import rasterizer as R
    sc, ofb = _big_zframe(oracle)
    W, H = sc.width, sc.height
    rng = np.random.default_rng(100)
    L = random_lines(rng, 100_000, W, H, max_len=48, zrange=(0.0, 6000.0))
    long_ = random_lines(rng, 300, W, H, max_len=1500)
    L = np.concatenate([L[:50_000], long_, L[50_000:]])
    dense = random_lines(rng, 20_000, W, H, max_len=40)          # 20 000 lines through one tile: its list overflows
    dense["x0"] = rng.integers(600, 664, len(dense)); dense["x1"] = rng.integers(600, 664, len(dense))
    dense["y0"] = rng.integers(800, 816, len(dense)); dense["y1"] = rng.integers(800, 816, len(dense))
    zb = ofb.zbuffer
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        for routes in (0, R.Context.ROUTE_LINE_TILES):
            ctx.set_routes(routes)
            for lines in (L, dense):
                fb.clear(sc.clear_color)
                R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
                c0 = ctx.route_counts()
                _draw_check(fb, ofb.pixels, zb, lines, zb)
                c1 = ctx.route_counts()
                assert c1["line_tiles" if routes == 0 else "line_scan"] == c0["line_tiles" if routes == 0 else "line_scan"] + 1
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_lines_bands(gpu_ctx):
    from bonnie32_amd import rasterizer as R
    W, H = 640, 480
    fb = R.Framebuffer(W, H, gpu_ctx)
    rng = np.random.default_rng(4)
    zb = rng.uniform(0.0, 3000.0, W * H).astype(f32)
    for n in (40, 3000):
        L = random_lines(rng, n, W, H, max_len=300)
        fb.set_band(0, H)
        fb.clear(b32.Color(9, 9, 9))
        _upload_zbuffer(fb, zb)
        base = fb.pixels
        want = base.copy(); np_lines(want, zb, W, H, L)
        for band in ((0, 100), (100, 333), (333, 334), (334, H)):
            fb.set_band(*band)
            fb.draw_lines(L)
        fb.set_band(0, H)
        assert np.array_equal(fb.pixels, want)
        fb.upload(base)
        fb.set_band(100, 333)                                    # one band alone: only its rows change
        fb.draw_lines(L)
        fb.set_band(0, H)
        part = base.reshape(H, -1).copy(); part[100:333] = want.reshape(H, -1)[100:333]
        assert np.array_equal(fb.pixels, part.reshape(-1))


@pytest.mark.gpu
def test_gpu_lines_pipeline(gpu_ctx, oracle):
    from bonnie32_amd import rasterizer as R, scenegen
    rng = np.random.default_rng(77)
    # painter's mode (the z-buffer is not valid: every depth f32::MAX), a deferred clear just before the lines
    sc = scenegen.make_scene("C1", variant="gouraud")
    W, H = sc.width, sc.height
    fb = R.Framebuffer(W, H, gpu_ctx)
    ofb = oracle.Framebuffer(W, H)
    ofb.clear(sc.clear_color)
    oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    fb.clear(sc.clear_color)
    R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    L = random_lines(rng, 500, W, H, max_len=80)
    _draw_check(fb, ofb.pixels, None, L)
    fb.clear(b32.Color(70, 10, 10, abi.ERASE))                  # deferred: flushed before the lines
    ofb2 = oracle.Framebuffer(W, H); ofb2.clear(b32.Color(70, 10, 10, abi.ERASE))
    _draw_check(fb, ofb2.pixels, None, L[:50])
    # the 8-bit render_mesh path, z-buffer mode
    sc8 = scenegen.make_scene("C1", variant="gouraud", seed=5)
    tex8 = [b32.Texture.from_texture15(t) for t in sc8.textures]
    st = b32.RasterSettings.game()
    ofb.clear(sc8.clear_color)
    assert oracle.render_mesh(ofb, sc8.vertices, sc8.faces, tex8, sc8.camera, st)[0] == 0
    fb.clear(sc8.clear_color)
    R.render_mesh(fb, sc8.vertices, sc8.faces, tex8, sc8.camera, st)
    _draw_check(fb, ofb.pixels, ofb.zbuffer, random_lines(rng, 300, W, H), ofb.zbuffer)
    # two frames in flight: b32_frame_submit -> b32_draw_lines -> b32_fb_download_async, the line array overwritten after each call
    ctx = R.Context(0)
    try:
        st = b32.RasterSettings.game()
        meshes = [scenegen.make_scene("C1", n_tris=800, seed=300 + i, variant="gouraud") for i in range(3)]
        fb2 = R.Framebuffer(W, H, ctx)
        slots = [R.ResidentScene(fb2, m.vertices, m.faces, m.textures).detach() for m in meshes]
        table = ctx.make_frame_table(meshes[0].camera, st, slots)
        bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
        frames = [(random_lines(rng, 36, W, H, kinds=(abi.LINE_3D,)), random_lines(rng, 700, W, H)) for _ in range(4)]
        want = []
        for small, big in frames:
            o = oracle.Framebuffer(W, H); o.clear(b32.Color(10, 10, 30))
            for m in meshes:
                assert oracle.render_mesh_15(o, m.vertices, m.faces, m.textures, meshes[0].camera, st)[0] == 0     # (one camera per frame)
            px = o.pixels.copy(); np_lines(px, o.zbuffer, W, H, small); np_lines(px, o.zbuffer, W, H, big)
            want.append(px)
        tickets = []
        for i, (small, big) in enumerate(frames):
            fb2.clear(b32.Color(10, 10, 30))
            ctx.frame_submit(table)
            for lines in (small, big):
                arr = lines.copy()
                fb2.draw_lines(arr)
                arr[:] = random_lines(rng, len(arr), W, H)        # the caller reuses its array at once
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
