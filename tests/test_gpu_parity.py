"""Parity tests proper: the HIP path through the C ABI against the CPU oracle, bit-exact (integer/byte outputs and
exact-order f32).  Every test needs a real MI355X and fails loudly if the HIP library or device is missing."""
import copy
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import scenegen
from tests.golden.make_golden import SCENES, SCENES8, needle_scene

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
HASHES = json.load(open(os.path.join(GOLD, "hashes.json")))


def gpu_render(ctx, sc, resident=False, indexed=False, band=None):
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    fb.clear(sc.clear_color)
    if band:
        fb.set_band(*band)
    if resident:
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, None if indexed else sc.textures, sc.indexed_textures if indexed else None)
        tm = rs.render(sc.camera, sc.settings, sc.fog)
    else:
        tm = R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
    return fb.pixels, tm


def cpu_render(oracle, sc):
    fb = oracle.Framebuffer(sc.width, sc.height); fb.clear(sc.clear_color)
    rc, tm, d = oracle.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog, dump=True)
    assert rc == 0
    return fb.pixels, tm, d


def test_device_f32_semantics(gpu_ctx):
    """No FMA contraction, correctly rounded / and sqrt, denormals kept: the premises of bit-exactness."""
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(1 << 16) * 1e3).astype(np.float32)
    b = rng.standard_normal(1 << 16).astype(np.float32)
    c = (rng.standard_normal(1 << 16) * 1e-3).astype(np.float32)
    a[:8] = [1e-40, 3e-39, 1.0, 16777216.0, 1e38, -1e-45, 0.1, 3.0]
    b[:8] = [0.5, 0.25, 3.0, 1.0, 10.0, 0.5, 0.2, 7.0]
    with np.errstate(all="ignore"):
        assert np.array_equal(gpu_ctx.selftest_f32(0, a, b, c), (a * b).astype(np.float32) + c)
        assert np.array_equal(gpu_ctx.selftest_f32(1, a, b, c), a / b)
        assert np.array_equal(gpu_ctx.selftest_f32(2, np.abs(a), b, c), np.sqrt(np.abs(a)))
        assert np.array_equal(gpu_ctx.selftest_f32(3, a, b, c), (a + b) / c)
    # Rust's `as i32` / `as u32` (NaN -> 0, saturating, toward zero) are gfx950's v_cvt_i32_f32 / v_cvt_u32_f32 as the kernels use them
    edge = np.array([np.nan, -np.nan, np.inf, -np.inf, 2147483648.0, 2147483520.0, -2147483648.0, -2147483904.0, 4294967296.0, 4294967040.0,
                     -0.0, 0.0, 0.99999994, -0.99999994, -1.0, 1.5, -1.5, 255.99998, 256.0, 1e-40, -1e-40, 3e9, -3e9, 1e30, -1e30, 16777217.0,
                     8388607.5, -8388607.5], dtype=np.float32)
    x = np.concatenate([edge, (rng.standard_normal(4096) * 3e9).astype(np.float32), (rng.standard_normal(4096) * 70000).astype(np.float32)])
    with np.errstate(all="ignore"):
        x64 = x.astype(np.float64)
        want_i = np.where(np.isnan(x64), 0, np.clip(np.trunc(np.nan_to_num(x64, nan=0.0, posinf=1e300, neginf=-1e300)), -2147483648.0, 2147483647.0)).astype(np.int64)
        want_u = np.where(np.isnan(x64), 0, np.clip(np.trunc(np.nan_to_num(x64, nan=0.0, posinf=1e300, neginf=-1e300)), 0.0, 4294967295.0)).astype(np.int64)
    assert np.array_equal(gpu_ctx.selftest_f32(5, x, x, x).view(np.int32).astype(np.int64), want_i)
    assert np.array_equal(gpu_ctx.selftest_f32(6, x, x, x).view(np.uint32).astype(np.int64), want_u)
    # Fixed32::mul_fixed (fixed.rs:161-165) on raw words: bits 12 .. 43 of the signed 64-bit product
    ia = np.concatenate([np.array([0, 1, -1, 4096, -4096, 2147483647, -2147483648, 2147483647, -2147483648, 123456789], dtype=np.int64),
                         rng.integers(-2**31, 2**31, 8192)])
    ib = np.concatenate([np.array([5, -1, -1, 4096, 4096, 2147483647, -2147483648, -2147483648, 1, -987654321], dtype=np.int64),
                         rng.integers(-2**31, 2**31, 4096), rng.integers(-5000, 5000, 4096)])
    prod = [(int(p) * int(q)) >> 12 for p, q in zip(ia, ib)]
    want_m = np.array([((v + 2**31) % 2**32) - 2**31 for v in prod], dtype=np.int64)
    got_m = gpu_ctx.selftest_f32(7, ia.astype(np.int32).view(np.float32), ib.astype(np.int32).view(np.float32), x[:len(ia)])
    assert np.array_equal(got_m.view(np.int32).astype(np.int64), want_m)
    # the wireframe tile kernel's depth parameter k / N (render.rs:784) by one reciprocal and a residual correction: bit-equal to the
    # IEEE division for EVERY pair 0 <= k <= N < 16384 it is used for (134 M quotients; the device counts the differing ones per N)
    N = np.arange(1, 16384, dtype=np.float32)
    assert not gpu_ctx.selftest_f32(8, N, N, N).any()
    # the z-buffer coverage's reciprocal (render.rs:1550: z = 1.0 / inv_z) by v_rcp_f32 + one fused residual correction (rcp_exact,
    # b32_device.h): bit-equal to the IEEE division for EVERY f32 operand -- all 2^32 of them, 65536 per lane; NaN results only have to be NaN
    base = (np.arange(65536, dtype=np.uint64) << 16).astype(np.uint32).view(np.float32)
    bad = gpu_ctx.selftest_f32(9, base, base, base)
    first = gpu_ctx.selftest_f32(10, base, base, base).view(np.uint32)
    assert not bad.any(), [hex(int(v)) for v in first[bad > 0][:8]]


def test_device_constants_are_the_reference_text(gpu_ctx):
    """Every numeric literal of the algorithm as DEVICE code holds it (b32_device_constants: a kernel writes out the K:: names the
    kernels compute with, the UNR table the projection indexes and the dither offsets the fill adds) equals the literal that
    tests/golden/pin_constants.py found in the reference's text (tests/golden/ref_constants.json)."""
    ref = json.load(open(os.path.join(GOLD, "ref_constants.json")))
    got, unr, dither = gpu_ctx.device_constants()
    scalar_keys = {k for k, e in ref.items() if not isinstance(e["value"], list)}
    assert set(got) == scalar_keys, sorted(set(got) ^ scalar_keys)
    for k in sorted(scalar_keys):
        e = ref[k]
        want = float(np.uint32(e["f32_bits"]).view(np.float32)) if isinstance(e["value"], float) else e["value"]
        assert got[k] == want, (k, got[k], e)
    assert unr.tolist() == ref["unr.table"]["value"]
    assert dither.tolist() == ref["dither.matrix"]["value"]


def test_project_fixed_stage(gpu_ctx, oracle):
    """fixed::project_fixed on the device vs the oracle, including saturating and wrapping inputs."""
    rng = np.random.default_rng(7)
    pos = (rng.standard_normal((20000, 3)) * np.array([3000, 3000, 4000])).astype(np.float32)
    pos[:200] *= 1e4
    pos[200:210] = [[3.0, 4.0, -5.0]] * 10
    cam = b32.Camera(position=(12.5, -7.25, 3.0), basis_x=(0.8, 0.0, -0.6), basis_y=(0.0, 1.0, 0.0), basis_z=(0.6, 0.0, 0.8))
    sx, sy, z = gpu_ctx.project_fixed_batch(pos, cam, 2560, 1920)
    from oracle import np_model as M
    ex, ey = M.project_fixed(pos, cam, 2560, 1920)
    assert np.array_equal(sx, ex) and np.array_equal(sy, ey)
    for i in range(0, 400):
        assert oracle.project_fixed(pos[i], cam, 2560, 1920)[:2] == (sx[i], sy[i])
    # The returned z is the per-vertex float depth of render.rs:2331-2345 (cam_pos.z + 5.0), bit for bit.  oracle.project_fixed's third
    # value is another quantity (the fixed-point depth the reference discards), so the expected depth is `sz` of the oracle's stage dump for
    # a draw of the same positions (no faces).  A second camera (translated, rotated about two axes), a second size, and positions with
    # zeros of both signs, denormals, 3e38 and cam-space depths on both sides of the near plane.

    def depth_bits_equal(a, b):
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    cy, sy_, cx, sx_ = (np.float32(t) for t in (np.cos(0.5), np.sin(0.5), np.cos(0.3), np.sin(0.3)))
    cam2 = b32.Camera(position=(-310.5, 44.125, -87.0), basis_x=(cy, 0.0, -sy_), basis_y=(sx_ * sy_, cx, sx_ * cy), basis_z=(cx * sy_, -sx_, cx * cy))
    extra = [[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, 1e-40], [1e-40, -1e-45, 1e-39], [3e38, 0.0, 0.0], [0.0, -3e38, 3e38], [3e38, 3e38, 3e38]]
    for c in (cam, cam2):                                          # cam-space z = 0.1 (the near plane, math.rs:155) and its neighbours
        o, bz = np.asarray(c.position, np.float32), np.asarray(c.basis_z, np.float32)
        for zc in (0.1, np.nextafter(np.float32(0.1), np.float32(0)), np.nextafter(np.float32(0.1), np.float32(1)), 0.0999, 0.1001, -0.1, 0.0):
            extra.append((o + bz * np.float32(zc)).astype(np.float32))
            extra.append((o + bz * np.float32(zc) + np.asarray(c.basis_x, np.float32) * np.float32(3.0)).astype(np.float32))
    pos2 = np.concatenate([pos, np.array(extra, np.float32)])
    verts = b32.make_vertices(len(pos2)); verts["pos"] = pos2
    for c in (cam, cam2):
        for w, h in ((2560, 1920), (333, 197)):
            gx, gy, gz = gpu_ctx.project_fixed_batch(pos2, c, w, h)
            ofb = oracle.Framebuffer(w, h)
            with np.errstate(all="ignore"):
                rc, _t, d = oracle.render_mesh_15(ofb, verts, b32.make_faces(0), [], c, b32.RasterSettings.game(), dump=True)
                mx, my = M.project_fixed(pos2, c, w, h)
                rel = (pos2 - np.asarray(c.position, np.float32)).astype(np.float32)
                mz = M.dot3(rel, np.asarray(c.basis_z, np.float32)) + M.K("mesh.distance")
            assert rc == 0
            assert np.array_equal(gx, d["sx"]) and np.array_equal(gy, d["sy"]) and np.array_equal(gx, mx) and np.array_equal(gy, my)
            assert depth_bits_equal(gz, d["sz"]), f"{int((gz.view(np.uint32) != d['sz'].view(np.uint32)).sum())} depths differ ({w}x{h})"
            assert depth_bits_equal(gz, mz.astype(np.float32))
            assert (gz[:len(pos)] == gz[:len(pos)]).all() and ((gz > 5.1) & (gz < 5.1001)).any() and ((gz < 5.1) & (gz > 5.0998)).any()
    assert np.array_equal(gpu_ctx.project_fixed_batch(pos, cam, 2560, 1920)[2].view(np.uint32), z.view(np.uint32))


REAL = [n for n in SCENES if n.startswith("real:")]       # the reference's own sample meshes and level rooms (tests/golden/scenes/real/*.b32scene)


@pytest.mark.parametrize("name", ["C1", "C1:gouraud", "C1:blend", "C1:blend5", "C1:float", "C1:persp", "cube", "fog-flat-point-nocull", "C2", "C2:blend"] + REAL)
def test_frame_parity_small(gpu_ctx, oracle, name):
    sc = SCENES[name]()
    exp, etm, d = cpu_render(oracle, sc)
    got, tm = gpu_render(gpu_ctx, sc)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ"
    assert hashlib.sha256(got).hexdigest() == HASHES[name]["sha256"]
    assert tm.triangles_drawn == etm.triangles_drawn
    if not sc.settings.use_zbuffer:           # (the store count of a z-buffer frame depends on the sequential order: not reported by the library)
        assert tm.fragments == etm.fragments
    assert np.array_equal(gpu_ctx.last_draw_order(len(sc.faces)), d["draw_order"])


@pytest.fixture
def fast_ctx(gpu_ctx):
    """Fragment counting off: CHEAP coverage + runner-up repair + per-tile LDS depth sort where eligible."""
    gpu_ctx.set_fragment_counting(0)
    yield gpu_ctx
    gpu_ctx.set_fragment_counting(1)


@pytest.mark.parametrize("name", ["C1", "C1:gouraud", "C1:blend", "C1:blend5", "C1:float", "C1:persp", "cube", "fog-flat-point-nocull", "C2", "C2:blend",
                                  "C3:100k", "C5:20k"] + REAL)
def test_fast_path_frame_parity(fast_ctx, oracle, name):
    """Same frames through the fast path (no global depth sort, inside-test-only coverage, top-2 visibility).  C2 has tile
    lists longer than the LDS sort capacity, so it also exercises the automatic redraw with the global sort."""
    sc = SCENES[name]()
    exp, etm, d = cpu_render(oracle, sc)
    for resident in (False, True):
        got, tm = gpu_render(fast_ctx, sc, resident=resident, indexed=resident and bool(sc.indexed_textures))
        assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ (resident={resident})"
        assert tm.triangles_drawn == etm.triangles_drawn
        assert np.array_equal(fast_ctx.last_draw_order(len(sc.faces)), d["draw_order"])      # lazily materialised global order


def test_fast_path_long_lists_and_skipped_winners(fast_ctx, oracle):
    """One 64x64 tile holding > 32768 surfaces (runner-up not representable -> list scan), with a texture where a third of
    the texels are skippable on some faces and none on others (black_transparent off)."""
    sc = scenegen.make_scene("C2", n_tris=90_000, width=64, height=64, bbox_px=30.0, seed=4242)
    sc.faces["black_transparent"][::4] = 0
    exp, etm, d = cpu_render(oracle, sc)
    assert etm.triangles_drawn > 33000
    got, tm = gpu_render(fast_ctx, sc, resident=True)
    assert np.array_equal(got, exp)
    # a texture with many skippable texels forces EXACT coverage even with counting off
    sc2 = scenegen.make_scene("C1", seed=99)
    sc2.textures[0].pixels[::3] = 0
    exp2, etm2, _ = cpu_render(oracle, sc2)
    got2, tm2 = gpu_render(fast_ctx, sc2)
    assert np.array_equal(got2, exp2) and tm2.fragments == etm2.fragments


def test_fast_path_full_size_c3(fast_ctx, oracle):
    """Headline configuration through the fast path, bands included."""
    sc = scenegen.make_scene("C3")
    exp, etm, d = cpu_render(oracle, sc)
    got, tm = gpu_render(fast_ctx, sc, resident=True, indexed=True)
    assert np.array_equal(got, exp)
    assert tm.triangles_drawn == etm.triangles_drawn and tm.tile_pairs > tm.triangles_drawn
    row = sc.width * 4
    assembled = np.empty_like(got)
    for y0, y1 in [(0, 333), (333, 960), (960, 1920)]:
        part, _ = gpu_render(fast_ctx, sc, resident=True, indexed=True, band=(y0, y1))
        assembled[y0 * row:y1 * row] = part[y0 * row:y1 * row]
    assert np.array_equal(assembled, exp)


@pytest.mark.parametrize("name", ["C1:zbuf", "C1:zbuf-blend", "C1:zbuf-blend5", "C1:zbuf-gouraud"] + [n for n in SCENES if n.startswith("real:") and n.endswith(("-game", "-game-640"))])
def test_zbuffer_mode_parity(gpu_ctx, oracle, name):
    """use_zbuffer=true (the reference's default / RasterSettings::game()): framebuffer AND z-buffer bit-exact, opaque list
    in face order, transparent pass depth-tested without z writes."""
    from bonnie32_amd import rasterizer as R
    sc = SCENES[name]()
    ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    rc, etm, d = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog, dump=True)
    assert rc == 0
    assert hashlib.sha256(ofb.pixels).hexdigest() == HASHES[name]["sha256"]
    try:
        for counting, resident in ((1, False), (1, True), (0, False), (0, True)):
            gpu_ctx.set_fragment_counting(counting)
            fb = R.Framebuffer(sc.width, sc.height, gpu_ctx); fb.clear(sc.clear_color)
            if resident:
                tm = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).render(sc.camera, sc.settings, sc.fog)
            else:
                tm = R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
            assert np.array_equal(fb.pixels, ofb.pixels), (counting, resident)
            assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))
            assert tm.triangles_drawn == etm.triangles_drawn
            assert np.array_equal(gpu_ctx.last_draw_order(len(sc.faces)), d["draw_order"])
    finally:
        gpu_ctx.set_fragment_counting(1)


def test_zbuffer_persists_across_calls_and_clear_resets(gpu_ctx, oracle):
    """fb.zbuffer is read-modify-write across render_mesh_15 calls (scene.rs:215/165) and Framebuffer::clear resets it."""
    from bonnie32_amd import rasterizer as R
    a = SCENES["C1:zbuf"](); b = SCENES["C1:zbuf-blend"](); c = scenegen.make_scene("C1", seed=5)    # c: painter's mode onto the same fb
    ofb = oracle.Framebuffer(a.width, a.height); ofb.clear(a.clear_color)
    fb = R.Framebuffer(a.width, a.height, gpu_ctx); fb.clear(a.clear_color)
    assert np.all(fb.zbuffer == np.finfo(np.float32).max)
    for sc in (a, b, c, a):
        oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
        R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
        assert np.array_equal(fb.pixels, ofb.pixels)
        assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))
    ofb.clear(a.clear_color); fb.clear(a.clear_color)
    assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))
    oracle.render_mesh_15(ofb, b.vertices, b.faces, b.textures, b.camera, b.settings)
    R.render_mesh_15(fb, b.vertices, b.faces, b.textures, b.camera, b.settings)
    assert np.array_equal(fb.pixels, ofb.pixels) and np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))


def test_zbuffer_mode_large_frame(gpu_ctx, oracle):
    sc = scenegen.make_scene("C3", n_tris=150_000)
    sc.settings.use_zbuffer = True
    ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    rc, etm = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx); fb.clear(sc.clear_color)
    R.ResidentScene(fb, sc.vertices, sc.faces, indexed_textures=sc.indexed_textures).render(sc.camera, sc.settings)
    assert np.array_equal(fb.pixels, ofb.pixels) and np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))


@pytest.mark.parametrize("bbox_px,n", [(3e3, 2000), (2e5, 300), (1.5e6, 80), (6e6, 30)])
@pytest.mark.parametrize("zbuf", [False, True])
def test_triangle_sizes_across_the_row_trim_thresholds(gpu_ctx, oracle, bbox_px, n, zbuf):
    """Row trimming (b32_fill.hip: row_trim) changes regime with the triangle's doubled area A: integer-exact below ~4900, a widening
    margin up to 2^20, switched off above.  Triangles from ~50 px to most of the 2560x1920 frame, EXACT and CHEAP coverage."""
    sc = scenegen.make_scene("C3", n_tris=n, bbox_px=bbox_px, seed=int(bbox_px) % 9973)
    sc.settings.use_zbuffer = zbuf
    want, etm, _ = cpu_render(oracle, sc)
    try:
        for counting in (1, 0):
            gpu_ctx.set_fragment_counting(counting)
            got, tm = gpu_render(gpu_ctx, sc, resident=True, indexed=True)
            assert np.array_equal(got, want)
            assert tm.triangles_drawn == etm.triangles_drawn
            if counting and not zbuf:
                assert tm.fragments == etm.fragments
    finally:
        gpu_ctx.set_fragment_counting(1)


def test_bounding_box_is_part_of_the_inside_test(gpu_ctx, oracle):
    """See needle_scene.  First the scene is checked to contain what it is for (pixels outside a triangle's box that would pass the
    toleranced test), then GPU == oracle in CHEAP and EXACT coverage, painter's and z-buffer."""
    sc = needle_scene()
    want, etm, d = cpu_render(oracle, sc)
    # count box-external pixels (up to 3 to the left / right, same rows) that pass bc >= -1e-4 for some drawn triangle
    F = np.float32
    sx, sy = d["sx"].astype(F), d["sy"].astype(F)
    leaks = 0
    for f in d["draw_order"][:150]:
        i1, i2, i3 = sc.faces["v"][f]
        x1, y1, x2, y2, x3, y3 = sx[i1], sy[i1], sx[i2], sy[i2], sx[i3], sy[i3]
        area = F(F((y2 - y3) * (x1 - x3)) + F((x3 - x2) * (y1 - y3)))
        if area < 0:                                             # rendered back-face: v2 / v3 swap (render.rs:2453-2479)
            x2, y2, x3, y3 = x3, y3, x2, y2
            area = F(F((y2 - y3) * (x1 - x3)) + F((x3 - x2) * (y1 - y3)))
        if abs(area) < 1:
            continue
        inv = F(F(1.0) / area)
        bx0, bx1 = int(max(min(x1, x2, x3), 0)), int(min(max(x1, x2, x3), sc.width - 1))
        by0, by1 = max(int(min(y1, y2, y3)), 0), min(int(max(y1, y2, y3)), sc.height - 1)
        ys = np.arange(by0, by1 + 1, dtype=np.float32)[:, None]
        xs = np.concatenate([np.arange(bx0 - 3, bx0), np.arange(bx1 + 1, bx1 + 4)]).astype(np.float32)[None, :]
        w0 = ((y2 - y3) * (xs - x3) + (x3 - x2) * (ys - y3)).astype(F)
        w1 = ((y3 - y1) * (xs - x3) + (x1 - x3) * (ys - y3)).astype(F)
        bx, by = (w0 * inv).astype(F), (w1 * inv).astype(F)
        bz = ((F(1.0) - bx).astype(F) - by).astype(F)
        leaks += int(((bx >= F(-0.0001)) & (by >= F(-0.0001)) & (bz >= F(-0.0001)) & (xs >= 0) & (xs < sc.width)).sum())
    assert leaks > 50, leaks
    for zbuf in (False, True):
        sc.settings.use_zbuffer = zbuf
        want, etm, _ = cpu_render(oracle, sc)
        try:
            for counting in (0, 1):
                gpu_ctx.set_fragment_counting(counting)
                for resident in (False, True):
                    got, tm = gpu_render(gpu_ctx, sc, resident=resident)
                    assert np.array_equal(got, want), (zbuf, counting, resident, int((got != want).sum()))
        finally:
            gpu_ctx.set_fragment_counting(1)


def test_thousands_of_textures(gpu_ctx, oracle):
    """One texture per face, 6 000 of them (the surface record keeps the slot in 16 bits: up to 65 534 textures per call), a few with a
    texture blend mode, sizes 1x1 .. 8x5, plus ids past the end of the list (drawn untextured, like `textures.get(id)`)."""
    n = 6000
    sc = scenegen.make_scene("C1", n_tris=n, seed=77, bbox_px=120.0)
    rng = np.random.default_rng(77)
    texs = []
    for i in range(n):
        w, h = int(rng.integers(1, 9)), int(rng.integers(1, 6))
        px = rng.integers(0, 0x10000, w * h).astype(np.uint16)
        texs.append(b32.Texture15(w, h, px, int(b32.abi.ADD) if i % 97 == 0 else int(b32.abi.OPAQUE)))
    sc.textures = texs
    sc.faces["texture_id"] = np.arange(n, dtype=np.uint32)
    sc.faces["texture_id"][::211] = n + 5                          # out of range: untextured
    want, etm, _ = cpu_render(oracle, sc)
    try:
        for counting in (1, 0):
            gpu_ctx.set_fragment_counting(counting)
            for resident in (False, True):
                got, tm = gpu_render(gpu_ctx, sc, resident=resident)
                assert np.array_equal(got, want), (counting, resident, int((got != want).sum()))
                assert tm.triangles_drawn == etm.triangles_drawn
    finally:
        gpu_ctx.set_fragment_counting(1)
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    with pytest.raises(R.B32Error) as e:                           # 65 535 and more: refused, nothing drawn
        R.render_mesh_15(fb, sc.vertices[:3], sc.faces[:1], [texs[0]] * 65535, sc.camera, sc.settings)
    assert e.value.code == b32.abi.B32_E_UNSUPPORTED


def test_c1_against_committed_frame(gpu_ctx):
    z = np.load(os.path.join(GOLD, "c1_frame.npz"))
    got, tm = gpu_render(gpu_ctx, SCENES["C1"]())
    assert np.array_equal(got, z["rgba"])
    assert np.array_equal(gpu_ctx.last_draw_order(2000), z["draw_order"])


@pytest.mark.parametrize("name", ["C3:100k", "C5:20k"])
def test_frame_parity_large_frame(gpu_ctx, oracle, name):
    """2560x1920 frames: resident scene, index atlas + CLUT expanded on the device; the fused kernel fetches the expanded texels through
    L1 / L2 (a 64 KB atlas does not fit beside two workgroups' tile planes: see test_index_atlas_and_clut_sampled_from_lds)."""
    sc = SCENES[name]()
    got, tm = gpu_render(gpu_ctx, sc, resident=True, indexed=True)
    assert hashlib.sha256(got).hexdigest() == HASHES[name]["sha256"]
    assert (tm.triangles_drawn, tm.fragments) == (HASHES[name]["triangles_drawn"], HASHES[name]["fragments"])


def test_full_size_c3_properties(gpu_ctx, oracle):
    """BASELINE size (1M tris @ 2560x1920): exact parity against the oracle plus size-independent properties:
    idempotence (same frame twice), band decomposition (union of band renders == whole frame), fragment count."""
    sc = scenegen.make_scene("C3")
    exp, etm, d = cpu_render(oracle, sc)
    got, tm = gpu_render(gpu_ctx, sc, resident=True, indexed=True)
    assert np.array_equal(got, exp)
    assert (tm.triangles_drawn, tm.fragments) == (etm.triangles_drawn, etm.fragments)
    assert np.array_equal(gpu_ctx.last_draw_order(len(sc.faces)), d["draw_order"])
    z = d["sz"][sc.faces["v"][d["draw_order"]]]          # painter's order: key is non-increasing along the draw order
    key = ((z[:, 0] + z[:, 1]) + z[:, 2]) / np.float32(3.0)
    assert (np.diff(key) <= 0).all()
    got2, _ = gpu_render(gpu_ctx, sc, resident=True, indexed=True)
    assert np.array_equal(got2, got)
    row = sc.width * 4
    frags = 0
    assembled = np.empty_like(got)
    for y0, y1 in [(0, 700), (700, 701), (701, 1300), (1300, 1920)]:      # ragged, tile-unaligned bands
        part, ptm = gpu_render(gpu_ctx, sc, resident=True, indexed=True, band=(y0, y1))
        assembled[y0 * row:y1 * row] = part[y0 * row:y1 * row]
        clear = np.tile(np.array([20, 22, 28, 255], np.uint8), sc.width)
        assert np.array_equal(part[:y0 * row].reshape(-1, row), np.tile(clear, (y0, 1)))      # rows outside the band untouched
        frags += ptm.fragments
    assert np.array_equal(assembled, exp) and frags == etm.fragments


def test_async_frames_are_never_silently_dropped(oracle):
    """A large scene's frame can run out of tile-list space (direct binning: fixed tile regions sized from the mesh) and then draws
    nothing until the host redraws it.  With frames enqueued back to back and a camera that moves (near: 58 000 surfaces spread over
    300 tiles; far: 11 600 surfaces inside eight tiles -> their regions overflow at the initial size) the middle frame of
    near, far, near  (no clear in between: read-modify-write) must not get lost:
      safe mode (default): enqueueing the next frame settles the pending one -> the result equals the oracle's three draws;
      deep mode (b32_set_async_depth(1)): no synchronisation between frames; the lost frame is REPORTED by b32_frame_finish
      (B32_E_FRAME_DROPPED), the most recent frame is intact, and after that report the context works normally again."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=120_000, width=640, height=480, bbox_px=60.0, seed=321)
    far = b32.Camera(position=(0.0, 0.0, -45000.0)); near = sc.camera
    ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    for cam in (near, far, near):
        assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, sc.settings)[0] == 0
    only_near = oracle.Framebuffer(sc.width, sc.height); only_near.clear(sc.clear_color)
    for cam in (near, near):
        oracle.render_mesh_15(only_near, sc.vertices, sc.faces, sc.textures, cam, sc.settings)
    assert not np.array_equal(only_near.pixels, ofb.pixels)
    # ---- safe mode, fresh context (tile regions at their initial size)
    ctx = R.Context(0)
    fb = R.Framebuffer(sc.width, sc.height, ctx); fb.clear(sc.clear_color)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    for cam in (near, far, near):
        rs.render_async(cam, sc.settings)
    got = fb.pixels                                   # (the download settles the last frame too)
    assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ"
    tm = rs.finish()
    # a download right after an overflowing frame shows the redrawn frame, never the cleared one
    ctx2 = R.Context(0)
    fb2 = R.Framebuffer(sc.width, sc.height, ctx2); fb2.clear(sc.clear_color)
    rs2 = R.ResidentScene(fb2, sc.vertices, sc.faces, sc.textures)
    rs2.render_async(far, sc.settings)
    o2 = oracle.Framebuffer(sc.width, sc.height); o2.clear(sc.clear_color)
    oracle.render_mesh_15(o2, sc.vertices, sc.faces, sc.textures, far, sc.settings)
    assert np.array_equal(fb2.pixels, o2.pixels)
    rs2.finish()
    # a clear between two frames: the overflowing frame must be redrawn BEFORE the clear, not on top of it
    ctx4 = R.Context(0)
    fb4 = R.Framebuffer(sc.width, sc.height, ctx4); fb4.clear(sc.clear_color)
    rs4 = R.ResidentScene(fb4, sc.vertices, sc.faces, sc.textures)
    rs4.render_async(far, sc.settings)
    fb4.clear(sc.clear_color)
    far_shifted = b32.Camera(position=(3000.0, 0.0, -45000.0))          # the far view again, elsewhere on screen
    rs4.render_async(far_shifted, sc.settings)
    o4 = oracle.Framebuffer(sc.width, sc.height); o4.clear(sc.clear_color)
    oracle.render_mesh_15(o4, sc.vertices, sc.faces, sc.textures, far_shifted, sc.settings)
    assert np.array_equal(fb4.pixels, o4.pixels)
    rs4.finish()
    # ---- deep mode, fresh context
    ctx3 = R.Context(0)
    ctx3.set_async_depth(1)
    fb3 = R.Framebuffer(sc.width, sc.height, ctx3); fb3.clear(sc.clear_color)
    rs3 = R.ResidentScene(fb3, sc.vertices, sc.faces, sc.textures)
    for cam in (near, far, near):
        rs3.render_async(cam, sc.settings)
    with pytest.raises(R.B32Error) as e:
        rs3.finish()
    assert e.value.code == b32.abi.B32_E_FRAME_DROPPED
    assert np.array_equal(fb3.pixels, only_near.pixels)           # the lost frame drew nothing, the others are intact
    fb3.clear(sc.clear_color)
    rs3.render_async(far, sc.settings)
    rs3.finish()                                                    # the most recent frame IS redrawn (regions grown), no error left over
    assert np.array_equal(fb3.pixels, o2.pixels)
    # ---- deep mode with three frame sets (b32_set_pipeline_depth): the dropped frame sits in a set that is revisited only three frames
    # later, or -- with fewer frames behind it -- only by b32_frame_finish reading the other sets' control blocks; reported either way
    for n_after in (1, 2, 3, 4):
        ctx5 = R.Context(0)
        ctx5.set_async_depth(1); ctx5.set_pipeline_depth(3)
        fb5 = R.Framebuffer(sc.width, sc.height, ctx5); fb5.clear(sc.clear_color)
        rs5 = R.ResidentScene(fb5, sc.vertices, sc.faces, sc.textures)
        for cam in (near, far) + (near,) * n_after:
            rs5.render_async(cam, sc.settings)
        with pytest.raises(R.B32Error) as e:
            rs5.finish()
        assert e.value.code == b32.abi.B32_E_FRAME_DROPPED, n_after
        assert np.array_equal(fb5.pixels, only_near.pixels), n_after          # (opaque painter's frames: drawing `near` again changes nothing)
        fb5.clear(sc.clear_color)
        rs5.render_async(far, sc.settings)
        rs5.finish()
        assert np.array_equal(fb5.pixels, o2.pixels), n_after
        ctx5.close()


def test_safe_mode_clear_supersedes_a_pending_frame(oracle):
    """Safe mode (the library default) settles a pending large-scene frame before anything writes the framebuffer -- except a
    b32_fb_clear of the whole band, which overwrites every pixel and depth that frame can have drawn: the frame is marked superseded
    and the next draw is enqueued behind it without a host synchronisation (the reference's loop is clear, draw, clear, draw).  A frame
    that overflowed its tile regions and drew nothing may therefore be left behind -- but only where it can never be seen: the final
    picture is the oracle's, b32_frame_finish reports no error, a download right after a draw still shows that draw (redrawn), and a
    mesh error (vertex index out of range) in a superseded frame is still reported by the next b32_frame_finish."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=120_000, width=640, height=480, bbox_px=60.0, seed=321)
    far = b32.Camera(position=(0.0, 0.0, -45000.0)); near = sc.camera
    far_shifted = b32.Camera(position=(3000.0, 0.0, -45000.0))

    def want(cam, zbuffer=False):
        o = oracle.Framebuffer(sc.width, sc.height); o.clear(sc.clear_color)
        st = copy.copy(sc.settings); st.use_zbuffer = zbuffer
        assert oracle.render_mesh_15(o, sc.vertices, sc.faces, sc.textures, cam, st)[0] == 0
        return o.pixels
    for zbuffer in (False, True):
        st = copy.copy(sc.settings); st.use_zbuffer = zbuffer
        ctx = R.Context(0)                                         # (fresh context: tile regions at their initial size, the far view overflows them)
        fb = R.Framebuffer(sc.width, sc.height, ctx)
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        before = ctx.route_counts()
        for cam in (far, far_shifted, near, far):
            fb.clear(sc.clear_color)
            rs.render_async(cam, st)
        got = fb.pixels                                            # the download settles (and redraws) the last frame only
        assert np.array_equal(got, want(far, zbuffer)), f"{int((got != want(far, zbuffer)).sum())} bytes differ (zbuffer={zbuffer})"
        rs.finish()                                                # no error: nothing observable was lost
        after = ctx.route_counts()
        assert after["redraw_region"] - before["redraw_region"] <= 2      # (not one redraw per overflowing frame)
        fb.clear(sc.clear_color); rs.render_async(far_shifted, st)
        assert np.array_equal(fb.pixels, want(far_shifted, zbuffer))     # no clear behind it: settled as ever
        rs.finish()
        ctx.close()
    # an error of a superseded frame is not lost
    bad = sc.faces.copy(); bad["v"][5, 1] = len(sc.vertices) + 7
    ctx = R.Context(0)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs_bad = R.ResidentScene(fb, sc.vertices, bad, sc.textures).detach()
    rs_ok = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    fb.clear(sc.clear_color); rs_bad.render_async(near, sc.settings)
    fb.clear(sc.clear_color); rs_ok.render_async(near, sc.settings)
    with pytest.raises(R.B32Error) as e:
        rs_ok.finish()
    assert e.value.code == b32.abi.B32_E_INDEX
    ctx.close()


def test_lost_setup_flag_aborts_one_frame_and_is_reported(oracle):
    """The failure path of the flag / join hand-over (two frames in flight: k_flag on the side stream behind the setup kernel, k_join on
    the main stream in front of the fill), forced by b32_debug_inject: the frame's flag never shows its epoch, the join gives up after its
    patience, raises the sticky error bit and Events::join_abort; the fill of THAT frame reads nothing of the setup kernel's output and
    writes only the folded clear; b32_frame_finish returns B32_E_HIP (never silent); the frames before and after it are drawn normally --
    also the next frame on the SAME frame set, whose tile counters the aborted fill left zeroed."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=200_000)                      # 1200 tiles, direct binning: frames run two in flight
    want, otm, _ = cpu_render(oracle, sc)
    red = b32.Color(200, 10, 10)
    ctx = R.Context(0); ctx.set_async_depth(1)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, indexed_textures=sc.indexed_textures)
    for _ in range(4):
        fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings, sc.fog)
    rs.finish()
    assert np.array_equal(fb.pixels, want)
    base = ctx.route_counts()
    assert base["flag_join"] >= 2 and base["event_join"] == 0
    # (a) the LAST frame loses its flag: nothing but its clear colour on the screen, and the error
    fb.clear(sc.clear_color); rs.render_async()
    ctx.debug_inject(1)
    fb.clear(red); rs.render_async()
    with pytest.raises(R.B32Error) as ei:
        rs.finish()
    assert ei.value.code == b32.abi.B32_E_HIP
    solid = np.tile(np.array([200, 10, 10, 255], np.uint8), sc.width * sc.height)
    got = fb.pixels
    assert np.array_equal(got, solid), f"{int((got != solid).sum())} bytes of the aborted frame are not its clear colour"
    # (b) a frame in the MIDDLE loses its flag; four more follow (both frame sets are used again) and the last one is right
    fb.clear(sc.clear_color); rs.render_async()
    ctx.debug_inject(1)
    fb.clear(red); rs.render_async()
    for _ in range(4):
        fb.clear(sc.clear_color); rs.render_async()
    with pytest.raises(R.B32Error) as ei:
        rs.finish()
    assert ei.value.code == b32.abi.B32_E_HIP
    assert np.array_equal(fb.pixels, want)
    # and the context is clean again
    fb.clear(sc.clear_color); rs.render_async()
    tm = rs.finish()
    assert np.array_equal(fb.pixels, want) and tm.triangles_drawn == otm.triangles_drawn
    assert ctx.lib.b32_debug_inject(ctx.h, 4) == b32.abi.B32_E_ARG
    ctx.close()


def test_narrow_band_runs_three_frame_sets_by_itself(oracle):
    """b32_set_pipeline_depth(0), the default: a band of at most a sixth of the frame's rows (one rank of a frame sharded over six or more GPUs)
    switches the context to three frame sets, a wider band or the whole frame back to two; frames drawn across the switches, pipelined, equal
    the oracle's rows of the band."""
    from bonnie32_amd import rasterizer as R, parallel
    sc = scenegen.make_scene("C3", n_tris=150_000)
    want, _, _ = cpu_render(oracle, sc)
    want = want.reshape(sc.height, sc.width, 4)
    ctx = R.Context(0); ctx.set_async_depth(1)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, indexed_textures=sc.indexed_textures)
    for N, r in ((8, 3), (2, 1), (8, 7), (1, 0), (6, 2)):
        y0, y1 = parallel.band_rows(sc.height, N, r)
        fb.set_band(y0, y1)
        p0 = ctx.route_counts()["pipelined"]
        fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings, sc.fog)
        for _ in range(6):
            fb.clear(sc.clear_color); rs.render_async()
        rs.finish()
        assert ctx.route_counts()["pipelined"] - p0 >= 4
        got = fb.pixels.reshape(sc.height, sc.width, 4)
        assert np.array_equal(got[y0:y1], want[y0:y1]), (N, r)
    ctx.close()


def test_batched_draws_poll_their_hand_over_and_a_lost_flag_is_reported(oracle):
    """The merged draws of a batched frame (b32_frame_begin / _add_scene / _end, frames back to back): the fused kernel polls the setup -> fill
    hand-over itself (FillArgs::join_seq, route counter `poll_join`) -- no event, no join kernel in front of it.  Frames equal the oracle's
    sequential calls; then b32_debug_inject(1) makes one draw's flag carry another value: its workgroups give up after 2 ms, that draw draws
    nothing, b32_frame_finish returns B32_E_HIP (never silent), and the frames after it are right again."""
    from bonnie32_amd import rasterizer as R
    meshes = _console_meshes(12, 5100)
    st = b32.RasterSettings.game()
    st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.point((0.0, -100.0, 1500.0), 3000.0, 1.2)]
    cam = b32.Camera(position=(15.0, -10.0, -40.0))
    W, H = meshes[0].width, meshes[0].height
    clear = b32.Color(10, 10, 30)
    ofb = oracle.Framebuffer(W, H); ofb.clear(clear)
    for sc in meshes:
        assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, st, None)[0] == 0
    ctx = R.Context(0); ctx.set_async_depth(1)
    fb = R.Framebuffer(W, H, ctx)
    slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in meshes]

    def frame():
        fb.clear(clear)
        ctx.frame_begin(cam, st)
        for rs in slots:
            ctx.frame_add(rs)
        ctx.frame_end()
    for _ in range(4):
        frame()
    ctx.finish()
    assert np.array_equal(fb.pixels, ofb.pixels) and np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))
    rc = ctx.route_counts()
    assert rc["poll_join"] >= 6 and rc["event_join"] == 0, rc
    frame()
    ctx.debug_inject(1)
    frame()                                   # its first pipelined draw loses its flag
    frame(); frame()
    with pytest.raises(R.B32Error) as ei:
        ctx.finish()
    assert ei.value.code == b32.abi.B32_E_HIP
    assert np.array_equal(fb.pixels, ofb.pixels), "the frames behind the lost flag are drawn in full"
    frame(); frame()
    ctx.finish()
    assert np.array_equal(fb.pixels, ofb.pixels) and np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))
    for rs in slots:
        rs.close()
    ctx.close()


@pytest.mark.parametrize("zbuffer", [False, True])
def test_frames_with_a_transparent_pass_two_in_flight(oracle, zbuffer):
    """Frames that fill the GPU (1200 tiles) and have a transparent pass, back to back: the next frame's setup kernel is released by k_blend's
    start instead of the fill's (FillArgs::start_defer), so the order between the frame sets now hangs on a word the BLEND kernel publishes.
    Six frames pipelined, painter's and z-buffer mode, camera moved between them so that a stale set would show: every second frame checked
    against the oracle."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=120_000, variant="blend", seed=31)
    if zbuffer:
        sc.settings = b32.RasterSettings(shading=0, lights=[], backface_wireframe=False)
    cams = []
    for k in range(3):
        cam = copy.deepcopy(sc.camera)
        cam.position = (cam.position[0] + 0.7 * k, cam.position[1] - 0.4 * k, cam.position[2])
        cams.append(cam)
    want = []
    for cam in cams:
        s2 = copy.copy(sc); s2.camera = cam
        want.append(cpu_render(oracle, s2)[0])
    ctx = R.Context(0); ctx.set_async_depth(1)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    for k in (0, 1, 2, 0, 1, 2, 1, 0):
        p0 = ctx.route_counts()["pipelined"]
        for _ in range(3):                                   # three frames in a row with this camera, the last one is looked at
            fb.clear(sc.clear_color); rs.render_async(cams[k], sc.settings, sc.fog)
        rs.finish()
        assert ctx.route_counts()["pipelined"] - p0 >= 2
        got = fb.pixels
        assert np.array_equal(got, want[k]), f"camera {k}: {int((got != want[k]).sum())} bytes differ"
    ctx.close()


def test_lost_start_signal_is_reported_and_the_frames_are_right(oracle):
    """The failure path of the device-side order between frame sets (round 6: the fused kernel publishes Events::fill_started, k_gate in front of
    the setup kernel that next writes the frame set waits for it instead of for a cross-stream event), forced by b32_debug_inject(2): one fill
    does not publish its start, the gate behind it gives up after 2 ms, raises the sticky error bit and lets its setup kernel go on (by then the
    main stream is long past the set's last reader); b32_frame_finish returns B32_E_HIP once -- never silent -- every frame is drawn, and the
    context is clean afterwards."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=200_000)
    want, otm, _ = cpu_render(oracle, sc)
    ctx = R.Context(0); ctx.set_async_depth(1)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, indexed_textures=sc.indexed_textures)
    for _ in range(4):
        fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings, sc.fog)
    rs.finish()
    assert np.array_equal(fb.pixels, want)
    p0 = ctx.route_counts()["pipelined"]
    ctx.debug_inject(2)
    for _ in range(5):
        fb.clear(sc.clear_color); rs.render_async()
    with pytest.raises(R.B32Error) as ei:
        rs.finish()
    assert ei.value.code == b32.abi.B32_E_HIP
    assert ctx.route_counts()["pipelined"] - p0 >= 4          # the frames behind the silent fill really took the gated route
    assert np.array_equal(fb.pixels, want)
    for _ in range(3):
        fb.clear(sc.clear_color); rs.render_async()
    tm = rs.finish()
    assert np.array_equal(fb.pixels, want) and tm.triangles_drawn == otm.triangles_drawn
    ctx.close()


def test_streams_of_one_priority_hand_over_by_event(oracle):
    """The other branch of the hand-over (b32_frame.hip: `join_ok`): when the caller's stream has the SIDE stream's priority the two may
    share a hardware queue, where k_join in front of k_flag would only end by its patience -- such frames keep the cross-stream event.
    A stream of the lowest priority made with the HIP runtime directly; frames of a large mesh two in flight on it, each against the
    oracle; the route counters say which hand-over ran."""
    from bonnie32_amd import rasterizer as R
    hip = C.CDLL("libamdhip64.so")
    least, greatest = C.c_int(), C.c_int()
    assert hip.hipDeviceGetStreamPriorityRange(C.byref(least), C.byref(greatest)) == 0
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithPriority(C.byref(stream), C.c_uint(1), least) == 0      # hipStreamNonBlocking
    sc = scenegen.make_scene("C3", n_tris=200_000, seed=7)
    want = cpu_render(oracle, sc)[0]
    ctx = R.Context(0); ctx.set_async_depth(1)
    ctx.set_stream(stream.value)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, indexed_textures=sc.indexed_textures)
    try:
        for i in range(7):
            fb.clear(b32.Color(9 * i, 3, 200) if i % 2 else sc.clear_color)      # (a frame that kept an older frame's pixels would show)
            rs.render_async(sc.camera, sc.settings, sc.fog)
            if i in (4, 6):
                got = fb.pixels
                assert np.array_equal(got, want), f"frame {i}: {int((got != want).sum())} bytes differ"
        rs.finish()
        rc = ctx.route_counts()
        assert rc["pipelined"] >= 3 and rc["event_join"] == rc["pipelined"] and rc["flag_join"] == 0, rc
    finally:
        ctx.close()
        hip.hipStreamDestroy(stream)


# Route-counter deltas of test_route_census_of_a_fixed_frame_sequence, group by group (counters that did not move are left out).  Recorded
# by running this test body on the commit BEFORE enqueue_frame was split into steps (profiles/frame_plan_refactor.md), on 256 CUs.
CENSUS_CUS = 256
CENSUS = {
    "small": {"inline_bin": 1},
    "large": {"direct_bin": 3, "pipelined": 2, "flag_join": 2},
    "large-narrow": {"direct_bin": 3, "pipelined": 2, "flag_join": 2},
    "batched": {"direct_bin": 3, "pipelined": 2, "flag_join": 2, "poll_join": 2},      # (a polled hand-over counts under flag_join too)
    "wire": {"direct_bin": 3, "pipelined": 2, "wire_tiles": 3, "flag_join": 2},
    "clear": {"direct_bin": 1},
    "keyed": {"keyed": 2, "redraw_pairs": 1},      # (the first keyed frame of the context outgrows its pair buffers and is redrawn)
}


def test_route_census_of_a_fixed_frame_sequence(oracle):
    """Every route draws the same pixels, and the other tests assert the route counters with `>=`: a frame sent down a neighbouring route
    would pass them.  One context on its own stream, a fixed sequence of 320x240 frames that reaches each branch of the frame's plan -- inline
    binning; direct binning with the flag / join hand-over of small frames, with and without the 16-wave form; the polled hand-over of a batched
    frame; wire binning on the side stream; a folded clear; the keyed route -- and after each group the EXACT delta of every counter of
    route_counts(), against the values the commit before the split gave; every frame bit for bit against the oracle."""
    import torch
    from bonnie32_amd import rasterizer as R
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count        # (b32_device_constants does not export it)
    if n_cu != CENSUS_CUS:
        pytest.skip(f"the census was recorded on {CENSUS_CUS} CUs, this device has {n_cu}: the routes depend on the count")
    small = scenegen.make_scene("C1", n_tris=300, seed=61)
    large = scenegen.make_scene("C2", n_tris=9000, seed=62)
    wired = copy.copy(large); wired.settings = copy.copy(large.settings)
    wired.settings.backface_cull = True; wired.settings.backface_wireframe = True
    rooms = [scenegen.make_scene("C1", n_tris=1500, seed=63 + i, variant="blend" if i == 2 else "gouraud", bbox_px=400.0) for i in range(3)]
    room_st = b32.RasterSettings.game()
    room_st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.point((0.0, -100.0, 1500.0), 3000.0, 1.2)]
    room_cam = b32.Camera(position=(15.0, -10.0, -40.0))
    room_clear = b32.Color(10, 10, 30)
    W, H = small.width, small.height
    ofb = oracle.Framebuffer(W, H); ofb.clear(room_clear)
    for sc in rooms:
        assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, room_cam, room_st, None)[0] == 0
    want = {"small": cpu_render(oracle, small)[0], "large": cpu_render(oracle, large)[0], "wire": cpu_render(oracle, wired)[0], "rooms": ofb.pixels}

    ctx = R.Context(0); ctx.set_async_depth(1)
    fb = R.Framebuffer(W, H, ctx)
    rs_small = R.ResidentScene(fb, small.vertices, small.faces, small.textures).detach()
    rs_large = R.ResidentScene(fb, large.vertices, large.faces, large.textures).detach()
    slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in rooms]
    seen = {}
    last = ctx.route_counts()

    def group(name, key):
        nonlocal last
        got = fb.pixels
        assert np.array_equal(got, want[key]), f"{name}: {int((got != want[key]).sum())} bytes differ from the oracle"
        now = ctx.route_counts()
        seen[name] = {k: now[k] - last[k] for k in now if now[k] != last[k]}
        print(f"census {name}: {seen[name]}")
        last = now

    def three(rs, sc):                                        # three frames with the finish deferred: the second and third may run two in flight
        for _ in range(3):
            fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings, sc.fog)
        rs.finish()
    try:
        fb.clear(small.clear_color); rs_small.render(small.camera, small.settings, small.fog)
        group("small", "small")
        three(rs_large, large)
        group("large", "large")
        ctx.set_routes(R.Context.ROUTE_WIDE_GROUPS)
        three(rs_large, large)
        group("large-narrow", "large")
        ctx.set_routes(0)
        for _ in range(3):
            fb.clear(room_clear)
            ctx.frame_begin(room_cam, room_st)
            for rs in slots:
                ctx.frame_add(rs)
            ctx.frame_end()
        ctx.finish()
        group("batched", "rooms")
        three(rs_large, wired)
        group("wire", "wire")
        fb.clear(b32.Color(200, 10, 10)); fb.clear(large.clear_color)
        rs_large.render(large.camera, large.settings, large.fog)
        group("clear", "large")
        ctx.set_routes(R.Context.ROUTE_SORT_FREE)
        fb.clear(large.clear_color); rs_large.render(large.camera, large.settings, large.fog)
        group("keyed", "large")
    finally:
        for rs in slots + [rs_small, rs_large]:
            rs.close()
        ctx.close()
    assert seen == CENSUS, seen


def test_superseded_frame_is_not_redrawn_over_an_executed_clear(oracle):
    """ADVICE r5 (b32_frame.hip): draw A (overflows its tile regions on a fresh context: nothing drawn), b32_fb_clear (safe mode marks A
    superseded, the clear stays deferred), b32_synchronize (flushes the clear WITHOUT settling: it now sits behind A on the stream), draw
    B.  A must be retired, not redrawn -- a redraw would put A's pixels on top of the executed clear and B would be drawn over them.
    Expected picture: the clear colour + B, exactly as the reference's sequence gives; A's capacities are still granted (B's view of the
    same far mesh needs them) and no error is reported.  The same with a download in place of draw B: the cleared frame, nothing of A."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=120_000, width=640, height=480, bbox_px=60.0, seed=321)
    far = b32.Camera(position=(0.0, 0.0, -45000.0)); far_shifted = b32.Camera(position=(3000.0, 0.0, -45000.0))
    red = b32.Color(200, 10, 10)
    for tail in ("draw", "download"):
        ctx = R.Context(0)
        fb = R.Framebuffer(sc.width, sc.height, ctx)
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        fb.clear(sc.clear_color); rs.render_async(far, sc.settings)          # A
        fb.clear(red)
        ctx.synchronize()
        want = oracle.Framebuffer(sc.width, sc.height); want.clear(red)
        if tail == "draw":
            rs.render_async(far_shifted, sc.settings)                         # B, on the red frame
            assert oracle.render_mesh_15(want, sc.vertices, sc.faces, sc.textures, far_shifted, sc.settings)[0] == 0
        got = fb.pixels
        assert np.array_equal(got, want.pixels), f"{tail}: {int((got != want.pixels).sum())} bytes differ"
        rs.finish()
        assert ctx.route_counts()["redraw_region"] <= (1 if tail == "draw" else 0)      # (A itself was never redrawn)
        ctx.close()


def test_safe_mode_settles_at_a_clear_when_the_framebuffer_is_read_elsewhere(oracle):
    """ADVICE r5 (b32_api.hip): with caller-bound framebuffer memory (b32_fb_bind_device) the pixels are read behind the library's back,
    so a b32_fb_clear must SETTLE the pending frame as it did before round 5, not supersede it: a clear / draw loop that never calls
    b32_frame_finish and whose first frame overflows its tile regions (fresh context, far view) would otherwise overflow the same way
    forever, unseen.  The bound memory here is another context's framebuffer (b32_band_attach: also the shared-framebuffer case); it is
    read through THAT context, not through the one that draws."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=120_000, width=640, height=480, bbox_px=60.0, seed=321)
    far = b32.Camera(position=(0.0, 0.0, -45000.0))
    owner = R.Context(0)
    ofb = R.Framebuffer(sc.width, sc.height, owner)
    ctx = R.Context(0)                                                         # safe mode (default), fresh capacities
    ctx.band_attach(owner, 1)
    fb = R.Framebuffer.__new__(R.Framebuffer); fb.ctx = ctx; fb.width, fb.height = sc.width, sc.height
    fb.set_band(0, sc.height)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    for _ in range(3):
        fb.clear(sc.clear_color)
        rs.render_async(far, sc.settings)
    ctx.synchronize()                                                          # (what an outside reader does: wait for the stream, nothing else)
    assert ctx.route_counts()["redraw_region"] == 1                            # the first frame was settled -- and redrawn -- at the second clear
    want = oracle.Framebuffer(sc.width, sc.height); want.clear(sc.clear_color)
    assert oracle.render_mesh_15(want, sc.vertices, sc.faces, sc.textures, far, sc.settings)[0] == 0
    got = ofb.pixels
    assert np.array_equal(got, want.pixels), f"{int((got != want.pixels).sum())} bytes differ"
    rs.finish()
    ctx.close(); owner.close()


def test_resized_root_must_export_again(gpu_ctx):
    """ADVICE r5 (b32_api.hip): the epoch words of an exported framebuffer sit behind its pixels at an offset that depends on its size.
    After any b32_fb_resize / _new of the root the old words are gone (inside the live pixels, or in freed memory): wait / release /
    status refuse until the root exports again, and the new export works at the new size."""
    from bonnie32_amd import rasterizer as R
    E = b32.abi.B32_E_ARG
    root = R.Context(0)
    fb = R.Framebuffer(640, 480, root)
    root.band_export()
    root.band_release(1); root.synchronize()
    assert root.band_status()[1] == 1
    fb.resize(320, 240)                                                        # fits the old allocation
    assert root.lib.b32_band_release(root.h, 2) == E and root.lib.b32_band_wait(root.h, 1, 1, 10) == E
    assert root.lib.b32_band_status(root.h, None, None, None) == E
    assert root.lib.b32_band_wait_all(root.h, 2, 1, 10, 1) == E
    share = root.band_export()
    assert np.frombuffer(share, np.uint32, 2, 64).tolist() == [320, 240]
    other = R.Context(0); other.band_attach(root, 1); other.band_publish(5); other.synchronize()
    root.band_wait(1, 5, 1_000_000); root.band_release(5); root.synchronize()
    epochs, released, timeouts = root.band_status()
    assert epochs[1] == 5 and released == 5 and timeouts == 0
    other.band_close()
    fb.resize(2048, 1024)                                                      # a new allocation
    assert root.lib.b32_band_status(root.h, None, None, None) == E
    root.band_export(); assert root.band_status()[1] == 0
    other.close(); root.close()


def test_pipeline_gate_argument_range():
    """b32_set_pipeline_gate: 0 = no hold, 1 .. 1000 = the fill's tail, 1001 .. 2000 = a share of the tiles behind its first round;
    anything above is refused and leaves the setting alone (include/b32raster.h)."""
    from bonnie32_amd import rasterizer as R
    ctx = R.Context(0)
    for ok in (0, 1, 1000, 1001, 1150, 2000):
        ctx.set_pipeline_gate(ok)
    for bad in (2001, 5000, 0xFFFFFFFF):
        with pytest.raises(R.B32Error) as e:
            ctx.set_pipeline_gate(bad)
        assert e.value.code == b32.abi.B32_E_ARG


def test_pipeline_depth_argument_range():
    """b32_set_pipeline_depth: two or three frame sets, or 0 = the library's own choice; anything else is refused (include/b32raster.h)."""
    from bonnie32_amd import rasterizer as R
    ctx = R.Context(0)
    for ok in (3, 2, 2, 3, 0, 0, 3, 0):
        ctx.set_pipeline_depth(ok)
    for bad in (1, 4, 0xFFFFFFFF):
        with pytest.raises(R.B32Error) as e:
            ctx.set_pipeline_depth(bad)
        assert e.value.code == b32.abi.B32_E_ARG


@pytest.mark.parametrize("mode", ["8bit", "zbuffer", "game"])
def test_capped_fill_forms_two_in_flight(oracle, mode):
    """The fills that run under the 112-VGPR cap beside the next frame's setup kernel (round 5: k_cover_plain8, k_cover_plain_z,
    k_cover_lit with k_setup<1, 2>), on a mesh large enough for direct binning and two frames in flight: the 8-bit path in painter's
    mode (render_mesh, render.rs:1971-2264), z-buffer mode without a shading pass, and RasterSettings::game() (types.rs:1455-1460).
    Five cameras back to back, a clear before each in painter's mode, none in the z-buffer modes (colour and depth accumulate)."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=60_000, width=1920, height=1440, bbox_px=120.0, seed=515, variant="gouraud")
    cams = [b32.Camera(position=(30.0 * i, -18.0 * i, -260.0 * i)) for i in range(5)]
    if mode == "8bit":
        st = b32.RasterSettings.benchmark(); st.use_rgb555 = False
        tex8 = [b32.Texture.from_texture15(t) for t in sc.textures]
    elif mode == "zbuffer":
        st = b32.RasterSettings.benchmark(); st.use_zbuffer = True
    else:
        st = b32.RasterSettings.game()
    ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    for cam in cams:
        if mode == "8bit":
            ofb.clear(sc.clear_color)
            assert oracle.render_mesh(ofb, sc.vertices, sc.faces, tex8, cam, st)[0] == 0
        else:
            assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, st)[0] == 0
    ctx = R.Context(0)
    ctx.set_async_depth(1)
    fb = R.Framebuffer(sc.width, sc.height, ctx); fb.clear(sc.clear_color)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, textures8=tex8) if mode == "8bit" else R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    if mode == "8bit": fb.clear(sc.clear_color)
    rs.render_async(cams[0], st); rs.finish()
    for cam in cams[1:]:
        if mode == "8bit": fb.clear(sc.clear_color)
        rs.render_async(cam, st)
    rs.finish()
    assert ctx.route_counts()["pipelined"] == 3
    assert np.array_equal(fb.pixels, ofb.pixels), f"{int((fb.pixels != ofb.pixels).sum())} bytes differ"
    if mode != "8bit":
        assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))


@pytest.mark.parametrize("depth", [2, 3])
def test_mixed_settings_back_to_back(oracle, depth):
    """Frames of one large resident mesh enqueued back to back with DIFFERENT settings from frame to frame -- default() (back-face
    wireframe), game(), z-buffer without a shading pass, wireframe overlay, flat shading -- so that consecutive frames take different
    forms of both kernels, frames with and without wire lists alternate on the frame sets, and the wire binning runs on the side stream
    for some frames and not at all for others.  All in z-buffer mode without a clear: every frame's colour, depth and wire pixels stay."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=60_000, width=1920, height=1440, bbox_px=120.0, seed=909, variant="gouraud")
    def zb():
        st = b32.RasterSettings.benchmark(); st.use_zbuffer = True; return st
    def overlay():
        st = b32.RasterSettings.game(); st.wireframe_overlay = True; return st
    def flat():
        st = b32.RasterSettings.game(); st.shading = b32.abi.SHADE_FLAT; return st
    seq = [b32.RasterSettings(), b32.RasterSettings.game(), zb(), b32.RasterSettings(), overlay(), flat(), b32.RasterSettings(), zb()]
    cams = [b32.Camera(position=(25.0 * i, -15.0 * i, -220.0 * i)) for i in range(len(seq))]
    ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    for cam, st in zip(cams, seq):
        assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, st)[0] == 0
    ctx = R.Context(0)
    ctx.set_async_depth(1); ctx.set_pipeline_depth(depth)
    fb = R.Framebuffer(sc.width, sc.height, ctx); fb.clear(sc.clear_color)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    rs.render_async(cams[0], seq[0]); rs.finish()
    for cam, st in zip(cams[1:], seq[1:]):
        rs.render_async(cam, st)
    rs.finish()
    assert ctx.route_counts()["pipelined"] >= 4
    assert np.array_equal(fb.pixels, ofb.pixels), f"{int((fb.pixels != ofb.pixels).sum())} bytes differ"
    assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))


@pytest.mark.parametrize("depth", [2, 3])
def test_wireframe_frames_two_in_flight(oracle, depth):
    """RasterSettings::default() (back-face wireframe, types.rs:1475-1495) on a large mesh, frames back to back: since round 5 the wire list
    k_setup writes is part of the frame set, so these frames run two in flight as well -- the next frame's setup kernel beside this
    frame's fill and wireframe kernels.  Five cameras in z-buffer mode without a clear in between: colour, depth and the wire pixels of
    every frame accumulate, so each frame's wire kernels must have read their OWN frame's list."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=60_000, width=1920, height=1440, bbox_px=120.0, seed=4242, variant="gouraud")
    st = b32.RasterSettings()                         # the reference's defaults
    cams = [b32.Camera(position=(35.0 * i, -20.0 * i, -280.0 * i)) for i in range(5)]
    ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    for cam in cams:
        assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, st)[0] == 0
    ctx = R.Context(0)
    ctx.set_async_depth(1); ctx.set_pipeline_depth(depth)
    fb = R.Framebuffer(sc.width, sc.height, ctx); fb.clear(sc.clear_color)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    rs.render_async(cams[0], st); rs.finish()
    for cam in cams[1:]:
        rs.render_async(cam, st)
    rs.finish()
    assert ctx.route_counts()["pipelined"] == 3
    assert np.array_equal(fb.pixels, ofb.pixels), f"{int((fb.pixels != ofb.pixels).sum())} bytes differ"
    assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))


@pytest.mark.parametrize("gate,routes_off,depth", [(1150, 0, 2), (300, 0, 2), (0, 0, 2), (1000, 0, 2), (2000, 0, 2), (300, 64, 2),
                                                   (1150, 0, 3), (0, 0, 3), (1000, 0, 3), (300, 64, 3)])
def test_two_frames_in_flight(oracle, gate, routes_off, depth):
    """Frames enqueued back to back run their setup kernel on the context's second stream, on the other frame set, beside the previous
    frame's fill (B32_ROUTE_PIPELINE, b32_set_pipeline_gate) -- or, with three frame sets (b32_set_pipeline_depth), beside the fill of
    the frame before that one.  Six frames of a large mesh (direct binning) with a moving camera in
    z-buffer mode without a clear in between -- colour AND depth accumulate, so every frame must have been drawn from its own records,
    in order -- then painter's frames with a clear each; and the same calls with a small mesh (whose frames stay on one stream)."""
    from bonnie32_amd import rasterizer as R
    for n_tris, deep in ((60_000, 1), (1500, 0)):
        big = n_tris > 8192          # (two frames in flight need a frame with more tiles than workgroup slots: 690 tiles of 64x64)
        sc = scenegen.make_scene("C3", n_tris=n_tris, width=1920 if big else 640, height=1440 if big else 480, bbox_px=120.0, seed=77 + n_tris, variant="gouraud")
        sc.settings.use_zbuffer = True
        cams = [b32.Camera(position=(40.0 * i, -25.0 * i, -300.0 * i)) for i in range(6)]
        ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
        for cam in cams:
            assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, sc.settings)[0] == 0
        ctx = R.Context(0)
        ctx.set_async_depth(deep); ctx.set_pipeline_gate(gate); ctx.set_routes(routes_off); ctx.set_pipeline_depth(depth)
        fb = R.Framebuffer(sc.width, sc.height, ctx); fb.clear(sc.clear_color)
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        rs.render_async(cams[0], sc.settings); rs.finish()            # (deep mode: list regions settled by a first synchronous frame)
        for cam in cams[1:]:
            rs.render_async(cam, sc.settings)
        tm = rs.finish()
        assert ctx.route_counts()["pipelined"] == (0 if (routes_off or n_tris < 8192) else 4)
        assert np.array_equal(fb.pixels, ofb.pixels) and np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))
        # painter's mode, a (folded) clear before every frame: the last camera's frame is what stays
        sc.settings.use_zbuffer = False
        o2 = oracle.Framebuffer(sc.width, sc.height); o2.clear(sc.clear_color)
        rc, otm, dump = oracle.render_mesh_15(o2, sc.vertices, sc.faces, sc.textures, cams[-1], sc.settings, None, dump=True)
        fb2 = R.Framebuffer(sc.width, sc.height, ctx)
        rs2 = R.ResidentScene(fb2, sc.vertices, sc.faces, sc.textures)
        for cam in cams:
            fb2.clear(sc.clear_color); rs2.render_async(cam, sc.settings)
        tm = rs2.finish()
        assert tm.triangles_drawn == otm.triangles_drawn and np.array_equal(fb2.pixels, o2.pixels)
        assert np.array_equal(ctx.last_draw_order(len(sc.faces)), dump["draw_order"])
        ctx.close()


def test_host_count_of_transparent_faces_bounds_the_device_classification(oracle):
    """A moderate mesh's frame is left in flight (never settled, never redrawn) when its tile regions hold every face and the HOST's count
    of faces that can be transparent fits what k_blend sorts per tile (enqueue_frame: direct_safe).  That count (upload_geometry: the
    face's own blend mode / editor alpha, or its texture's blend mode, render.rs:2403-2415) must bound what the setup kernel classifies
    on the device -- with nothing culled the two are equal."""
    from bonnie32_amd import rasterizer as R
    rng = np.random.default_rng(5)
    for trial in range(6):
        sc = scenegen.make_scene("C3", n_tris=20_000, width=640, height=480, bbox_px=50.0, seed=900 + trial, variant="blend" if trial % 2 else "bench")
        n = len(sc.faces)
        # three textures, one of them blending; texture ids partly out of range (untextured: only the face's own mode counts)
        base = sc.textures[0]
        sc.textures = [base, b32.Texture15(base.width, base.height, base.pixels.copy(), int(b32.abi.ADD)), b32.Texture15(8, 8, base.pixels[:64].copy(), int(b32.abi.OPAQUE))]
        sc.faces["texture_id"] = rng.integers(0, 5, n).astype(np.uint32)
        sc.faces["texture_id"][::17] = 0xFFFFFFFF
        sc.faces["editor_alpha"][::29] = int(rng.choice([0, 128, 254]))
        sc.faces["blend_mode"][::31] = int(b32.abi.SUBTRACT)
        sc.settings.backface_cull = bool(trial % 3 == 0)
        ctx = R.Context(0)
        fb = R.Framebuffer(sc.width, sc.height, ctx); fb.clear(sc.clear_color)
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        tm = rs.render(sc.camera, sc.settings)
        host, dev = ctx.transparent_counts()
        ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
        rc, otm, d = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, None, dump=True)
        assert rc == 0 and np.array_equal(fb.pixels, ofb.pixels) and tm.triangles_drawn == otm.triangles_drawn
        assert dev <= host, (trial, dev, host)
        if not sc.settings.backface_cull and tm.triangles_drawn == n:
            assert dev == host, (trial, dev, host)
        ctx.close()


def test_pending_frame_is_settled_before_its_scene_is_replaced(oracle):
    """Safe mode never loses a frame: a large mesh's frame whose tile regions overflowed is redrawn by the host from the RESIDENT scene, so
    it has to be settled before b32_scene_upload* / b32_set_band change what such a redraw would draw (found by the round-2 review: frame
    A was lost and mesh B -- with a transparent pass -- was drawn, and blended, twice)."""
    from bonnie32_amd import rasterizer as R
    a = scenegen.make_scene("C3", n_tris=120_000, width=640, height=480, bbox_px=60.0, seed=321)
    far = b32.Camera(position=(0.0, 0.0, -45000.0))                 # 11 600 surfaces inside eight tiles: their regions overflow at the initial size
    b = scenegen.make_scene("C3", n_tris=30_000, width=640, height=480, bbox_px=90.0, seed=99, variant="blend")
    ofb = oracle.Framebuffer(a.width, a.height); ofb.clear(a.clear_color)
    assert oracle.render_mesh_15(ofb, a.vertices, a.faces, a.textures, far, a.settings)[0] == 0
    assert oracle.render_mesh_15(ofb, b.vertices, b.faces, b.textures, b.camera, b.settings)[0] == 0
    for how in ("upload", "indexed", "band"):
        ctx = R.Context(0)
        fb = R.Framebuffer(a.width, a.height, ctx); fb.clear(a.clear_color)
        rs = R.ResidentScene(fb, a.vertices, a.faces, a.textures)
        rs.render_async(far, a.settings)                             # overflows; pending, not yet redrawn
        if how == "band":
            fb.set_band(0, a.height)                                 # (any band change settles the frame for the band it was enqueued with)
            assert ctx.route_counts()["redraw_region"] == 1
            rs.finish()
            want = oracle.Framebuffer(a.width, a.height); want.clear(a.clear_color)
            oracle.render_mesh_15(want, a.vertices, a.faces, a.textures, far, a.settings)
            assert np.array_equal(fb.pixels, want.pixels)
            ctx.close()
            continue
        rs2 = R.ResidentScene(fb, b.vertices, b.faces, b.textures) if how == "upload" else \
            R.ResidentScene(fb, b.vertices, b.faces, indexed_textures=b.indexed_textures)
        assert ctx.route_counts()["redraw_region"] == 1              # frame A was redrawn when mesh B was uploaded
        rs2.render_async(b.camera, b.settings)
        rs2.finish()
        got = fb.pixels
        assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ ({how})"
        ctx.close()


def test_clear_after_a_dropped_frame_in_deep_mode(oracle):
    """Deep asynchronous mode: draw (overflows, draws nothing yet) -> b32_fb_clear -> b32_frame_finish.  The redraw of the frame belongs
    BEFORE the clear that was issued after it: the framebuffer ends up cleared, not with the frame on top of the clear."""
    from bonnie32_amd import rasterizer as R
    a = scenegen.make_scene("C3", n_tris=120_000, width=640, height=480, bbox_px=60.0, seed=321)
    far = b32.Camera(position=(0.0, 0.0, -45000.0))
    red = b32.Color(200, 10, 10)
    ctx = R.Context(0); ctx.set_async_depth(1)
    fb = R.Framebuffer(a.width, a.height, ctx); fb.clear(a.clear_color)
    rs = R.ResidentScene(fb, a.vertices, a.faces, a.textures)
    rs.render_async(far, a.settings)
    fb.clear(red)
    rs.finish()
    assert ctx.route_counts()["redraw_region"] == 1
    want = oracle.Framebuffer(a.width, a.height); want.clear(red)
    assert np.array_equal(fb.pixels, want.pixels)
    # and the usual order afterwards: clear, draw
    fb.clear(a.clear_color); rs.render_async(far, a.settings); rs.finish()
    want.clear(a.clear_color); oracle.render_mesh_15(want, a.vertices, a.faces, a.textures, far, a.settings)
    assert np.array_equal(fb.pixels, want.pixels)
    ctx.close()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_band_ranks_share_one_gpu(world):
    """BASELINE config C4's data path with real processes (world = 8: C4's own partition, eight 240-row bands): `world` ranks (torch.distributed.run, gloo) share GPU 0, each binds the HIP
    context to its band of the 2560x1920 frame, renders C3 at 100 k triangles and the full 1 M-triangle C3, and the rows are gathered
    by bonnie32_amd.parallel.gather_bands and by the pipelined two-framebuffer flow of bench.py (gather_bands_async); rank 0 compares
    every assembled frame with the CPU oracle's (tests/band_worker.py).  What this cannot cover is the RCCL transport itself (one GPU
    per rank)."""
    import socket
    import subprocess
    import sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "tests", "band_worker.py")], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "BAND_WORKER_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("world,mode", [(2, "poll"), (8, "poll"), (8, "acquire")])
def test_band_ranks_share_one_gpu_through_the_c_abi(world, mode, oracle, tmp_path):
    """Config C4's exchange step behind the C boundary (include/b32raster.h "multi-GPU", b32_gather.hip), transport "shared framebuffer":
    this process is the root -- it owns the 2560x1920 framebuffer, exports it (b32_band_export), draws band 0 and makes its stream wait
    for the other ranks' epoch words (b32_band_wait); world - 1 worker PROCESSES (tests/band_worker_ipc.py: ctypes + numpy only, no
    torch) map the framebuffer (b32_band_import), draw their bands straight into it and publish every frame (b32_band_publish).  Six
    frames alternating between two scenes (a stale band would show), each compared with the CPU oracle's whole frame.  mode "poll": the
    workers read the root's release word from the host before the next frame; mode "acquire": they never touch the host between frames
    -- release / acquire order the frames on the device.  All ranks share GPU 0 (what is left untested is a peer mapping between two
    GPUs)."""
    import subprocess
    import sys
    from bonnie32_amd import rasterizer as R
    from bonnie32_amd.bands import band_rows
    W, H, NA, NB, FRAMES = 2560, 1920, 100_000, 60_000, 6
    scs = [scenegen.make_scene("C3", n_tris=n, width=W, height=H) for n in (NA, NB)]
    want = []
    for sc in scs:
        ofb = oracle.Framebuffer(W, H); ofb.clear(sc.clear_color)
        rc, otm = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog, fast=True)
        assert rc == 0
        want.append((ofb.pixels.copy(), otm.triangles_drawn))
    ctx = R.Context(0)
    ctx.set_async_depth(1)
    fb = R.Framebuffer(W, H, ctx)
    share = ctx.band_export()
    sf = tmp_path / "share.bin"
    sf.write_bytes(share)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "band_worker_ipc.py"), str(sf), str(r), str(world), str(NA), str(NB), str(FRAMES)] +
                              (["acquire"] if mode == "acquire" else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for r in range(1, world)]
    try:
        y0, y1 = band_rows(H, world, 0)
        fb.set_band(y0, y1)
        res = [R.ResidentScene(fb, sc.vertices, sc.faces, indexed_textures=sc.indexed_textures).detach() for sc in scs]
        for f in range(1, FRAMES + 1):
            sc, rs = scs[f % 2], res[f % 2]
            fb.clear(sc.clear_color)
            rs.render_async(sc.camera, sc.settings, sc.fog)
            for r in range(1, world):
                ctx.band_wait(r, f, 60_000_000)
            got = fb.pixels                                  # (b32_fb_download: behind this context's own band AND the waits on its stream)
            exp, drawn = want[f % 2]
            assert np.array_equal(got, exp), f"frame {f}: {int((got != exp).sum())} bytes differ (world={world}, mode={mode})"
            ctx.band_release(f)
        ctx.synchronize()
        epochs, released, timeouts = ctx.band_status()
        assert timeouts == 0 and released == FRAMES and all(e == FRAMES for e in epochs[1:world]), (epochs[:world], released, timeouts)
        for p in procs:
            out, err = p.communicate(timeout=120)
            assert p.returncode == 0 and "BAND_IPC_WORKER_OK" in out, (out[-1500:], err[-3000:])
    except AssertionError as e:
        logs = []
        for p in procs:
            if p.poll() is None:
                p.kill()
            out, err = p.communicate()
            logs.append((p.returncode, out[-600:], err[-1500:]))
        raise AssertionError(f"{e}\nworkers: {logs}\nstatus: {ctx.band_status()[0][:world]}")
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        ctx.close()


def test_band_exchange_argument_checks(gpu_ctx):
    """The multi-GPU entry points refuse what they cannot do, without touching the device: a root whose framebuffer is caller-bound
    memory cannot be exported, rank 0 / rank 64 cannot be imported or attached, publish / acquire need an imported context, wait /
    release an exported one, a context cannot attach to itself, and the RCCL transport without a communicator is an argument error."""
    from bonnie32_amd import rasterizer as R
    E = b32.abi.B32_E_ARG
    lib = gpu_ctx.lib
    root = R.Context(0)
    fb = R.Framebuffer(64, 48, root)
    share = root.band_export()
    assert len(share) == 96 and np.frombuffer(share, np.uint32, 2, 64).tolist() == [64, 48]
    other = R.Context(0)
    buf = C.create_string_buffer(share, 96)
    for rank in (0, 64, 1000):
        assert lib.b32_band_import(other.h, C.cast(buf, C.c_void_p), rank) == E
        assert lib.b32_band_attach(other.h, root.h, rank) == E
    assert lib.b32_band_attach(root.h, root.h, 1) == E
    assert lib.b32_band_publish(other.h, 1) == E and lib.b32_band_acquire(other.h, 1, 10) == E       # not a band rank (yet)
    assert lib.b32_band_wait(other.h, 1, 1, 10) == E and lib.b32_band_release(other.h, 1) == E       # not a root
    assert lib.b32_band_wait(root.h, 0, 1, 10) == E
    y = (C.c_uint32 * 2)(0, 24); y1 = (C.c_uint32 * 2)(24, 48)
    assert lib.b32_gather_bands_rccl(root.h, None, 0, 2, 0, y, y1) == E                               # no communicator
    assert lib.b32_gather_bands_rccl(root.h, C.c_void_p(1), 2, 2, 0, y, y1) == E                      # rank out of range
    # attach inside this process works, and a wait on a rank that never publishes times out COUNTED, not silently
    other.band_attach(root, 1)
    root.band_wait(1, 1, timeout_us=2000)
    root.synchronize()
    epochs, released, timeouts = root.band_status()
    assert epochs[1] == 0 and timeouts == 1
    other.band_publish(1); other.synchronize()
    root.band_wait(1, 1, timeout_us=2_000_000); root.synchronize()
    assert root.band_status()[0][1] == 1 and root.band_status()[2] == 1
    other.close(); root.close()


def test_band_wait_timeout_is_reported_by_frame_finish(oracle):
    """a band-exchange wait that gives up must not only be counted in the shared tail -- the waiting context's next
    b32_frame_finish returns B32_E_BAND_TIMEOUT (the presented frame may hold another rank's stale rows); the one after that is clean."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C1")
    root = R.Context(0); root.set_async_depth(1)
    fb = R.Framebuffer(sc.width, sc.height, root)
    root.band_export()
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings, sc.fog)
    root.band_wait_all(3, 1, timeout_us=3000, release_after=True)        # ranks 1 and 2 do not exist
    with pytest.raises(R.B32Error) as ei:
        rs.finish()
    assert ei.value.code == b32.abi.B32_E_BAND_TIMEOUT
    epochs, released, timeouts = root.band_status()
    assert timeouts == 2 and released == 1
    fb.clear(sc.clear_color); rs.render_async()
    tm = rs.finish()                                                      # the sticky bit was consumed
    want, otm, _ = cpu_render(oracle, sc)
    assert np.array_equal(fb.pixels, want) and tm.triangles_drawn == otm.triangles_drawn
    root.close()


def test_rccl_transport_loopback_on_one_gpu(oracle):
    """Transport (2) of the exchange step EXECUTED: a one-rank RCCL communicator made through the C ABI
    (b32_rccl_unique_id / _comm_create: the library's own dlopen of librccl and its resolved entry points), and
    b32_gather_bands_rccl_loopback -- the gather in which the root additionally sends its own band to itself -- enqueued on the
    context's stream right behind the frame's kernels: the upper half of the frame is drawn as a band, travels through ncclSend / ncclRecv
    (ncclUint8, grouped) into the lower half, and both halves must equal the oracle's rows of the upper half.  What stays unexecuted is a
    transfer between two physical GPUs."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=60_000, width=640, height=480)
    W, H = sc.width, sc.height
    want, otm, _ = cpu_render(oracle, sc)
    ctx = R.Context(0); ctx.set_async_depth(1)
    fb = R.Framebuffer(W, H, ctx)
    fb.upload(np.full(W * H * 4, 0xAB, np.uint8))
    fb.set_band(0, H // 2)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, indexed_textures=sc.indexed_textures)
    comm = ctx.rccl_comm_create(R.Context.rccl_unique_id(), 0, 1)
    E = b32.abi.B32_E_ARG
    y0 = (C.c_uint32 * 1)(0); y1 = (C.c_uint32 * 1)(H // 2)
    assert ctx.lib.b32_gather_bands_rccl_loopback(ctx.h, comm, 0, 1, 0, y0, y1, H // 4) == E             # destination overlaps the band
    assert ctx.lib.b32_gather_bands_rccl_loopback(ctx.h, comm, 0, 1, 0, y0, y1, H // 2 + 1) == E         # ... or leaves the framebuffer
    assert ctx.lib.b32_gather_bands_rccl_loopback(ctx.h, comm, 0, 1, 0, y0, y1, 0xFFFFFFFF) == E
    for frame in range(3):                                          # (the transfer of one frame behind the kernels of the same frame, three times)
        fb.clear(sc.clear_color)
        rs.render_async(sc.camera, sc.settings, sc.fog)
        ctx.gather_bands_rccl(comm, 0, 1, 0, [(0, H // 2)], loopback_dst_y0=H // 2)
    ctx.gather_bands_rccl(comm, 0, 1, 0, [(0, H // 2)])             # one rank, no loopback: nothing to do
    tm = rs.finish()
    got = fb.pixels.reshape(H, W, 4)
    top = want.reshape(H, W, 4)[:H // 2]
    assert np.array_equal(got[:H // 2], top), "the band itself"
    assert np.array_equal(got[H // 2:], top), "the band's rows after ncclSend / ncclRecv to self"
    assert tm.triangles_drawn == otm.triangles_drawn
    ctx.rccl_comm_destroy(comm)
    ctx.close()


@pytest.mark.parametrize("transport", ["shm", "rccl"])
def test_bench_c4_through_the_c_abi(transport):
    """BASELINE config C4 end to end through the product's own boundary: the driver's scaling command --
    `torch.distributed.run ... bench.py --gpus 4` -- with the four ranks sharing GPU 0 (gloo carries only the set-up bytes and the
    barriers).  `--transport shm`: every band rank maps rank 0's framebuffer (b32_band_import) and stores its rows of the 1 M-triangle
    frame into it, ordered by the device-side epoch words; the run-time self-check against the torch-gathered frame passes, no wait times
    out, and the timed frames' last one is bit-exact against the oracle (--check) and the committed hash.  `--transport rccl`: RCCL
    refuses ranks that share a GPU, so the set-up fails on every rank, the line SAYS it fell back to torch.distributed, and the frame
    is still right."""
    import socket
    import subprocess
    import sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=4", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "4", "--steps", "6", "--warmup", "2",
                        "--transport", transport, "--dist-backend", "gloo", "--check", "--full"], capture_output=True, text=True, timeout=1500, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert "parity vs oracle: bit-exact" in r.stderr, r.stderr[-3000:]
    assert line["n_gpus"] == 4 and line["bit_exact_vs_committed_hash"] is True
    t = line["transport"]
    assert t["requested"] == transport
    if transport == "shm":
        assert t["used"] == "shm" and t["self_check"] == "passed" and t["timeouts"] == 0 and t["fallback_reason"] is None, t
        assert "b32_band_export" in line["config"]["parallelism"]
    else:
        assert t["used"] == "torch" and t["self_check"] == "failed" and t["fallback_reason"], t
    assert line["weak_series"]["tris"] == 500000


def test_bench_dump_outputs_are_the_timed_frame(tmp_path):
    """bench.py --dump-outputs in a plain run (no --full): exactly --steps timed steps, no side measurement in the line, and the files
    hold what the last timed step returned -- at C1 the whole framebuffer, which must be the committed frame."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--config", "C1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 7 and line["ms_per_step"] > 0 and line["unit"] == "Mtriangles/s"
    assert not {"cpu_baseline", "configs", "roofline", "protocol", "weak_series"} & set(line)
    frame = np.load(out / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (240, 320, 4)
    px = frame.astype(np.uint8)
    assert np.array_equal(px, frame) and hashlib.sha256(px.tobytes()).hexdigest() == HASHES["C1"]["sha256"]
    assert np.array_equal(np.load(out / "frame_row_sums.npy"), px.sum(axis=1, dtype=np.float64))
    tm = np.load(out / "timings.npy")
    assert tm.dtype == np.float64 and tm[0] == HASHES["C1"]["triangles_drawn"]


def _console_meshes(n_meshes, seed0, blend_every=4):
    rng = np.random.default_rng(seed0)
    meshes = []
    for i in range(n_meshes):
        variant = "blend" if (blend_every and i % blend_every == blend_every - 1) else "gouraud"
        meshes.append(scenegen.make_scene("C1", n_tris=int(rng.integers(200, 2500)), seed=seed0 + i, variant=variant,
                                          bbox_px=float(rng.choice([150.0, 400.0, 900.0]))))
    return meshes


@pytest.mark.parametrize("zbuffer,counting,wire", [(True, 0, False), (True, 1, False), (False, 0, False), (True, 0, True)])
def test_batched_frame_equals_sequential_calls(oracle, zbuffer, counting, wire):
    """b32_frame_begin / _add_scene / _end: a console frame (scene.rs:112-261: clear, then one render_mesh_15 per room / asset part onto
    the same framebuffer, one camera and light list, per-mesh ambient, fog and backface culling) drawn as merged runs must leave the
    framebuffer AND the depth buffer of the oracle's sequential calls.  14 meshes, every fourth with a transparent pass (it ends its
    run), two of them double-sided (backface_cull off), three fog settings, ambients differing per room; z-buffer mode merges, painter's
    mode (order matters for every pixel) falls back to one draw per mesh through the same entry points; then the same frame again (merged
    meshes come from the cache), with one mesh re-uploaded (its run is rebuilt), and with batching switched off."""
    from bonnie32_amd import rasterizer as R
    meshes = _console_meshes(14, 4200)
    st = b32.RasterSettings.game()
    st.use_zbuffer = zbuffer
    st.backface_wireframe = wire      # (base settings with the back-face wireframe on: culled meshes are drawn one by one with their
                                      #  wireframe phase, double-sided ones -- no wireframe, render.rs:2577 -- still merge: soak seed 3101)
    st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.point((0.0, -100.0, 1500.0), 3000.0, 1.2)]
    fogs = [None, (1500.0, 3000.0, 5800.0, b32.Color(40, 50, 70)), (800.0, 2500.0, 5000.0, b32.Color(90, 20, 20))]
    per = [dict(ambient=0.2 + 0.05 * (i % 5), backface_cull=((i % 5 < 2) if wire else (i % 5 != 2)), fog=fogs[i % 3]) for i in range(len(meshes))]
    cam = b32.Camera(position=(15.0, -10.0, -40.0))
    W, H = meshes[0].width, meshes[0].height
    clear = b32.Color(10, 10, 30)

    def cpu_frame(ms):
        ofb = oracle.Framebuffer(W, H); ofb.clear(clear)
        drawn = 0
        for sc, p in zip(ms, per):
            s2 = copy.copy(st); s2.ambient = p["ambient"]; s2.backface_cull = p["backface_cull"]
            rc, tm = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, s2, p["fog"])
            assert rc == 0
            drawn += tm.triangles_drawn
        return ofb, drawn
    ofb, drawn = cpu_frame(meshes)
    ctx = R.Context(0)
    ctx.set_fragment_counting(counting)
    fb = R.Framebuffer(W, H, ctx)
    slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in meshes]

    def gpu_frame():
        fb.clear(clear)
        ctx.frame_begin(cam, st)
        for rs, p in zip(slots, per):
            ctx.frame_add(rs, **p)
        ctx.frame_end()
        return ctx.finish()
    for rep in range(2):
        gpu_frame()
        got = fb.pixels
        assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ (rep {rep})"
        if zbuffer:
            assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))
    bc = ctx.batch_counts()
    if wire:
        assert bc["merged_draws"] >= 2 and bc["single_draws"] >= 2 * 8, bc
    elif zbuffer:
        assert bc["merged_draws"] == 2 * 4 and bc["single_draws"] == 0 and bc["merged_built"] == 4, bc      # runs [0..3] [4..7] [8..11] [12, 13], built once
    else:
        assert bc["merged_draws"] == 0 and bc["single_draws"] == 2 * 14, bc
    # one mesh replaced: its run is rebuilt, the others are reused
    meshes2 = list(meshes)
    meshes2[5] = scenegen.make_scene("C1", n_tris=900, seed=777, variant="gouraud", bbox_px=500.0)
    slots[5].close()
    slots[5] = R.ResidentScene(fb, meshes2[5].vertices, meshes2[5].faces, meshes2[5].textures).detach()
    ofb2, _ = cpu_frame(meshes2)
    gpu_frame()
    assert np.array_equal(fb.pixels, ofb2.pixels)
    if zbuffer:
        assert np.array_equal(fb.zbuffer.view(np.uint32), ofb2.zbuffer.view(np.uint32))
        assert wire or ctx.batch_counts()["merged_built"] == 5
    # batching off: the same entry points, one draw per mesh
    ctx.set_routes(R.Context.ROUTE_BATCH)
    gpu_frame()
    assert np.array_equal(fb.pixels, ofb2.pixels)
    ctx.close()


def test_deferred_clear_is_never_observable(fast_ctx, oracle):
    """b32_fb_clear defers itself so that the frame that follows can fold it into its fused kernel (no clear launch).  Whatever else
    touches the framebuffer first must see the cleared frame: a download with no draw in between, a second clear with another
    colour, a band change, a z-buffer frame (depth reset too), a frame that draws nothing (empty mesh), tiles no surface reaches,
    and a bound device tensor read after b32_synchronize.  A sky pass, the star sprites, a clear_gradient and the presenter after a
    deferred clear are in test_sky_present.py: test_gpu_deferred_clear_before_sky_stars_gradient and
    test_gpu_present_sees_a_deferred_clear_and_a_pending_frame."""
    import torch
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=20_000, width=640, height=480, bbox_px=200.0, seed=12)
    sc.vertices["pos"][:, :2] *= np.float32(0.5)                      # the mesh covers the middle of the frame only: whole tiles stay empty
    red, blue = b32.Color(200, 10, 10), b32.Color(10, 10, 200)
    fb = R.Framebuffer(sc.width, sc.height, fast_ctx)
    ofb = oracle.Framebuffer(sc.width, sc.height)
    # clear, nothing else, download
    fb.clear(red); ofb.clear(red)
    assert np.array_equal(fb.pixels, ofb.pixels)
    # two clears, then a frame (folded), then the same again on top without a clear (read-modify-write)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    fb.clear(red); fb.clear(blue); ofb.clear(blue)
    for _ in range(2):
        rs.render(sc.camera, sc.settings)
        oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
        assert np.array_equal(fb.pixels, ofb.pixels)
    assert (ofb.pixels.reshape(-1, 4)[:, :3] == np.array([10, 10, 200], np.uint8)).all(axis=1).sum() > 100_000      # empty tiles really exist
    # clear of one band, band changed before the draw
    fb.set_band(100, 300); fb.clear(red); fb.set_band(0, sc.height)
    ofb.pixels.reshape(sc.height, -1)[100:300] = np.tile(np.array([200, 10, 10, 255], np.uint8), sc.width)
    rs.render(sc.camera, sc.settings)
    oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    assert np.array_equal(fb.pixels, ofb.pixels)
    # clear, then an empty mesh (no kernel runs), then a z-buffer frame after another clear (the depth buffer is reset as well)
    fb.clear(blue); ofb.clear(blue)
    R.render_mesh_15(fb, b32.make_vertices(0), b32.make_faces(0), [], sc.camera, sc.settings)
    assert np.array_equal(fb.pixels, ofb.pixels)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)      # (the drop-in call replaced the context's resident mesh)
    zs = b32.RasterSettings.game()
    for _ in range(2):
        fb.clear(red); ofb.clear(red)
        rs.render(sc.camera, zs)
        oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, zs)
        got = fb.pixels
        assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ (z-buffer frame)"
        assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))
    # a bound device tensor: the clear is in the tensor after b32_synchronize
    dev = torch.device("cuda", 0)
    ctx = R.Context(0)
    frame = torch.zeros(sc.width * sc.height * 4, dtype=torch.uint8, device=dev)
    fb2 = R.Framebuffer.__new__(R.Framebuffer); fb2.ctx = ctx
    fb2.bind_device(frame.data_ptr(), sc.width, sc.height)
    fb2.clear(red); ctx.synchronize(); torch.cuda.synchronize(dev)
    o2 = oracle.Framebuffer(sc.width, sc.height); o2.clear(red)
    assert np.array_equal(frame.cpu().numpy(), o2.pixels)
    ctx.close()


def test_framebuffer_new_on_a_reused_context(gpu_ctx, oracle):
    """Framebuffer::new (render.rs:18-25) gives zero pixels and an f32::MAX z-buffer; Framebuffer::resize to the same size keeps
    everything (render.rs:27-34).  A second Framebuffer of the same size on a reused context must not inherit the first one's frame."""
    from bonnie32_amd import rasterizer as R
    sc = SCENES["C1:zbuf"]()
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx); fb.clear(sc.clear_color)
    R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    drawn, zdrawn = fb.pixels, fb.zbuffer
    assert drawn.any() and (zdrawn != np.finfo(np.float32).max).any()
    fb.resize(sc.width, sc.height)                                   # same dimensions: no-op
    assert np.array_equal(fb.pixels, drawn) and np.array_equal(fb.zbuffer, zdrawn)
    fb2 = R.Framebuffer(sc.width, sc.height, gpu_ctx)                # new: zeroed, depth reset
    assert not fb2.pixels.any() and np.all(fb2.zbuffer == np.finfo(np.float32).max)
    ofb = oracle.Framebuffer(sc.width, sc.height)                    # (no clear: Framebuffer::new contents)
    oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    R.render_mesh_15(fb2, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    assert np.array_equal(fb2.pixels, ofb.pixels) and np.array_equal(fb2.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))


def test_texture_cache_is_semantically_per_call(gpu_ctx, oracle):
    """The drop-in call caches the uploaded textures by (pointer, size, blend mode, content hash): passing the same slice again skips
    the texel copies, but the call must behave as if it uploaded every time -- a texel changed IN PLACE (same pointer), a changed
    blend mode, another texture set and a return to the first one must all show up in the next frame."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=3000, width=320, height=240, bbox_px=300.0, seed=808)      # 256x256 atlas
    other = scenegen.make_scene("C1", n_tris=3000, bbox_px=300.0, seed=809)                           # 64x64 atlas, other content

    def both(textures):
        ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
        assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, textures, sc.camera, sc.settings)[0] == 0
        fb = R.Framebuffer(sc.width, sc.height, gpu_ctx); fb.clear(sc.clear_color)
        R.render_mesh_15(fb, sc.vertices, sc.faces, textures, sc.camera, sc.settings)
        got = fb.pixels
        assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ"
        return got
    a = both(sc.textures)
    assert np.array_equal(both(sc.textures), a)                     # second call: cache hit
    sc.textures[0].pixels[1000:30000] ^= 0x1234                     # same pointer, new content
    b = both(sc.textures)
    assert not np.array_equal(a, b)
    sc.textures[0].pixels[-1] ^= 1                                  # the very last texel (the hash's tail path)
    both(sc.textures)
    sc.textures[0].blend_mode = b32.abi.AVERAGE                     # same texels, other blend mode
    c_ = both(sc.textures)
    sc.textures[0].blend_mode = b32.abi.OPAQUE
    both(other.textures)                                            # another set in between
    assert np.array_equal(both(sc.textures), both(sc.textures))
    keep = [b32.Texture15(t.width, t.height, t.pixels.copy(), t.blend_mode) for t in sc.textures]     # same content at another address
    both(keep)


def test_raster_timings_are_filled_on_every_synchronous_call(gpu_ctx):
    """RasterTimings (types.rs:1499-1514): the reference fills every phase on every call (render.rs:2362, 2515-2516, 2544, 2572).  Here the
    phases come from the device-side phase clock with no profiling switched on: cull (the fused transform + cull + setup kernel), sort
    (the tile binning when it is a launch of its own; large meshes are binned by the setup kernel), draw (the fill kernels), wireframe (the line kernels); their sum cannot exceed the wall time of the call."""
    import time
    from bonnie32_amd import rasterizer as R
    gpu_ctx.set_profiling(0)
    for sc, wire in ((scenegen.make_scene("C3", n_tris=200_000), False), (SCENES["C1:default-settings"](), True), (SCENES["C1"](), False)):
        fb = R.Framebuffer(sc.width, sc.height, gpu_ctx); fb.clear(sc.clear_color)
        R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)          # warm-up (allocations)
        t0 = time.perf_counter()
        tm = R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
        wall = (time.perf_counter() - t0) * 1e3
        assert tm.cull_ms > 0 and tm.draw_ms > 0, tm
        assert (tm.wireframe_ms > 0) == wire, tm
        assert tm.sort_ms >= 0 and tm.cull_ms + tm.sort_ms + tm.draw_ms + tm.wireframe_ms <= wall, (tm, wall)
        if len(sc.faces) > 100_000:
            # a 200 k-triangle frame: tens of microseconds each (sort_ms is 0 when k_setup binned the faces itself: no binning launch)
            assert tm.cull_ms > 0.005 and tm.draw_ms > 0.01, tm
    tm = R.render_mesh_15(fb, b32.make_vertices(0), b32.make_faces(0), [], sc.camera, sc.settings)   # empty mesh: no kernel ran
    assert tm.triangles_drawn == 0 and tm.cull_ms == 0


def test_light_lists_change_between_async_frames(gpu_ctx, oracle):
    """Per-room light lists (scene.rs draws room after room, each with its own lights): up to 8 lights travel in the kernel arguments,
    longer lists through a device buffer; either way consecutive asynchronous frames with different lights must each use their own."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C1", variant="gouraud", seed=88, bbox_px=400.0)
    sc.settings.use_zbuffer = True
    mk = lambda k: [b32.Light.point((300.0 * i - 600.0, 100.0 * (i % 3), 1500.0 + 200.0 * i), 6000.0, 0.4 + 0.1 * i) for i in range(k)]
    lists = [mk(1), mk(8), mk(9), mk(3), mk(12), mk(2)]
    ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx); fb.clear(sc.clear_color)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    for i, ls in enumerate(lists):
        sc.settings.lights = ls
        cam = b32.Camera(position=(10.0 * i, -5.0 * i, 30.0 * i))
        assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, sc.settings)[0] == 0
        rs.render_async(cam, sc.settings)
    rs.finish()
    assert np.array_equal(fb.pixels, ofb.pixels) and np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))


@pytest.mark.parametrize("config,n_tris,width,height,expect_lds", [
    ("C1", 2000, 320, 240, True),        # 64x64 4-bit atlas, 16-wave workgroups (small mesh: lists collected in the fill)
    ("C2", 30_000, 320, 240, True),      # same atlas, direct binning
    ("C1", 40_000, 1280, 960, True),     # more tiles than CUs: two 8-wave workgroups per CU, 4.6 KB of atlas in the ~6 KB beside their planes
    ("C3", 20_000, 320, 240, True),      # 256x256 8-bit atlas (64.5 KB) beside ONE 16-wave workgroup's planes
    ("C3", 60_000, 1280, 960, False),    # the same atlas does not fit beside two workgroups' planes: expanded texels from global memory
])
def test_index_atlas_and_clut_sampled_from_lds(oracle, config, n_tris, width, height, expect_lds):
    """north_star's "LDS-staged 4/8-bit indexed texture tiles and palette" (B32_ROUTE_LDS_ATLAS): with ONE indexed texture the fused
    kernel stages CLUT + index bytes in LDS and performs Clut::lookup (types.rs:390-397) per shaded pixel whenever they fit beside the
    tile planes of the workgroup form in use.  Same frame as the oracle drawing the pre-expanded Texture15 (scene.rs:164), with the
    route on (counted) and switched off."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene(config, n_tris=n_tris, width=width, height=height, seed=4242 + n_tris, bbox_px=90.0 if width > 320 else None)
    at = sc.indexed_textures[0]
    at.indices[::53] = 255                                     # (some indices past a 16-entry palette: 0x0000 -> transparent texels)
    sc.textures = [at.to_texture15()]
    exp, etm, _ = cpu_render(oracle, sc)
    for off in (0, R.Context.ROUTE_LDS_ATLAS):
        ctx = R.Context(0); ctx.set_routes(off)
        for counting in (0, 1):
            ctx.set_fragment_counting(counting)
            before = ctx.route_counts()["lds_atlas"]
            got, tm = gpu_render(ctx, sc, resident=True, indexed=True)
            assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ (routes off {off}, counting {counting})"
            assert tm.triangles_drawn == etm.triangles_drawn
            assert (ctx.route_counts()["lds_atlas"] - before > 0) == (expect_lds and off == 0)
        # a Texture15 upload of the same texels never takes the route
        before = ctx.route_counts()["lds_atlas"]
        got, _ = gpu_render(ctx, sc, resident=True, indexed=False)
        assert np.array_equal(got, exp) and ctx.route_counts()["lds_atlas"] == before
        ctx.close()


def test_clut_indices_past_the_palette(gpu_ctx, oracle):
    """Clut::lookup (types.rs:390-397) returns 0x0000 for an index past the palette: a 4-bit CLUT (16 entries) under an atlas whose
    bytes run up to 255.  The device expansion of b32_scene_upload_indexed must give the texels of the oracle's expansion (and of
    the host mirror's IndexedAtlas::to_texture15), i.e. transparent texels wherever the index is out of range."""
    sc = scenegen.make_scene("C1", seed=123, bbox_px=300.0)
    at = sc.indexed_textures[0]
    assert at.clut.size == 16
    at.indices[:] = (scenegen.splitmix64(555, at.indices.size) % np.uint64(40)).astype(np.uint8)     # 60 % of the texels out of range
    at.indices[::97] = 255
    want15 = oracle.expand_indexed(at.indices, at.clut)
    assert np.array_equal(want15, at.to_texture15().pixels) and (want15 == 0).mean() > 0.5
    sc.textures = [at.to_texture15()]
    exp, etm, d = cpu_render(oracle, sc)
    try:
        for counting in (1, 0):
            gpu_ctx.set_fragment_counting(counting)
            got, tm = gpu_render(gpu_ctx, sc, resident=True, indexed=True)            # device-side CLUT expansion
            assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ (counting={counting})"
            assert tm.triangles_drawn == etm.triangles_drawn
            if counting:
                assert tm.fragments == etm.fragments
            got, tm = gpu_render(gpu_ctx, sc, resident=True, indexed=False)           # pre-expanded Texture15
            assert np.array_equal(got, exp)
    finally:
        gpu_ctx.set_fragment_counting(1)
    # a zero-length palette: every texel transparent, only untextured / black_transparent-off pixels remain
    at.clut = at.clut[:0]
    sc.textures = [at.to_texture15()]
    sc.faces["black_transparent"][::2] = 0
    exp, etm, _ = cpu_render(oracle, sc)
    got, tm = gpu_render(gpu_ctx, sc, resident=True, indexed=True)
    assert np.array_equal(got, exp) and tm.fragments == etm.fragments


def test_full_size_c5(gpu_ctx, oracle):
    """BASELINE configs[4] at full size: 1 M triangles of ~400 px at 64 discrete depths (massive painter's-key ties, ~13x overdraw,
    65 535 522 pixel stores).  Instrumented path (EXACT coverage, exact store count, draw order) and default path, against the
    oracle run here and against the committed hash (tests/golden/hashes.json, written in the build container)."""
    sc = scenegen.make_scene("C5")
    g = HASHES["C5"]
    exp, etm, d = cpu_render(oracle, sc)
    assert hashlib.sha256(exp).hexdigest() == g["sha256"] and (etm.triangles_drawn, etm.fragments) == (g["triangles_drawn"], g["fragments"])
    got, tm = gpu_render(gpu_ctx, sc, resident=True, indexed=True)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ"
    assert hashlib.sha256(got).hexdigest() == g["sha256"]
    assert (tm.triangles_drawn, tm.fragments) == (etm.triangles_drawn, etm.fragments) == (g["triangles_drawn"], 65535522)
    order = gpu_ctx.last_draw_order(len(sc.faces))
    assert np.array_equal(order, d["draw_order"]) and hashlib.sha256(order.tobytes()).hexdigest() == g["draw_order_sha256"]
    gpu_ctx.set_fragment_counting(0)
    try:
        got, tm = gpu_render(gpu_ctx, sc, resident=True, indexed=True)          # the path bench.py times
        assert hashlib.sha256(got).hexdigest() == g["sha256"] and tm.triangles_drawn == etm.triangles_drawn
    finally:
        gpu_ctx.set_fragment_counting(1)


def test_rmw_sequence_and_empty_mesh(gpu_ctx, oracle):
    """Several render_mesh_15 calls onto one framebuffer (scene.rs:215/165), then an empty mesh."""
    from bonnie32_amd import rasterizer as R
    a = scenegen.make_scene("C1", seed=1); b = scenegen.make_scene("C1", variant="blend", seed=2)
    ofb = oracle.Framebuffer(a.width, a.height); ofb.clear(a.clear_color)
    fb = R.Framebuffer(a.width, a.height, gpu_ctx); fb.clear(a.clear_color)
    for sc in (a, b, a):
        oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
        R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    assert np.array_equal(fb.pixels, ofb.pixels)
    tm = R.render_mesh_15(fb, b32.make_vertices(0), b32.make_faces(0), [], a.camera, a.settings)
    assert tm.triangles_drawn == 0 and np.array_equal(fb.pixels, ofb.pixels)
    # upload / download round trip and Framebuffer::resize zero-fill
    fb.upload(ofb.pixels[::-1].copy()); assert np.array_equal(fb.pixels, ofb.pixels[::-1])
    fb.resize(64, 48); assert not fb.pixels.any()


def test_edge_cases(gpu_ctx, oracle):
    """Off-screen / huge triangles (literal incremental-walk path), zero-area faces, untextured faces, out-of-range texture
    id, black_transparent off, zero-size texture, texture wider than the LDS budget (global-memory sampling)."""
    from bonnie32_amd import rasterizer as R
    rng = np.random.default_rng(11)
    n = 600
    v = b32.make_vertices(3 * n); f = b32.make_faces(n, texture_id=0)
    f["v"] = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    z = rng.uniform(1.0, 50.0, n).astype(np.float32)
    for k in range(3):
        v["pos"][k::3, 0] = rng.uniform(-200, 200, n) * (z / 8)
        v["pos"][k::3, 1] = rng.uniform(-200, 200, n) * (z / 8)
        v["pos"][k::3, 2] = z + rng.uniform(-0.5, 0.5, n)
    v["pos"][0:30] *= np.float32(400.0)                     # coordinates far beyond 2^22 after projection
    v["pos"][30:33] = v["pos"][33:36]                       # zero-area
    v["uv"] = rng.uniform(-3, 3, (3 * n, 2)).astype(np.float32)
    v["r"], v["g"], v["b"] = rng.integers(0, 256, (3, 3 * n), dtype=np.uint8)
    f["texture_id"][::5] = b32.abi.NO_TEXTURE
    f["texture_id"][1::7] = 9                                # out of range -> untextured (render.rs:2554-2556)
    f["texture_id"][2::11] = 1                               # zero-size texture
    f["black_transparent"][::3] = 0
    tex = b32.Texture15(512, 300, rng.integers(0, 0x10000, 512 * 300).astype(np.uint16))
    tex.pixels[::7] = 0; tex.pixels[3::13] = 0x8000
    empty = b32.Texture15(0, 0, np.zeros(0, np.uint16))
    st = b32.RasterSettings.benchmark(); st.backface_cull = False
    for (w, h) in [(320, 240), (333, 197)]:
        ofb = oracle.Framebuffer(w, h); ofb.clear(b32.Color(1, 2, 3))
        rc, etm = oracle.render_mesh_15(ofb, v, f, [tex, empty], b32.Camera(), st)
        assert rc == 0
        fb = R.Framebuffer(w, h, gpu_ctx); fb.clear(b32.Color(1, 2, 3))
        tm = R.render_mesh_15(fb, v, f, [tex, empty], b32.Camera(), st)
        assert np.array_equal(fb.pixels, ofb.pixels)
        assert (tm.triangles_drawn, tm.fragments) == (etm.triangles_drawn, etm.fragments)


def test_painters_sort_ties_are_stable(gpu_ctx, oracle):
    """C5-style scene: 64 discrete depths => massive key ties; equal keys must keep face order (stable sort_by)."""
    sc = scenegen.make_scene("C5", n_tris=30_000, width=640, height=480, bbox_px=200.0)
    exp, etm, d = cpu_render(oracle, sc)
    got, tm = gpu_render(gpu_ctx, sc)
    assert np.array_equal(gpu_ctx.last_draw_order(len(sc.faces)), d["draw_order"])
    assert np.array_equal(got, exp)


def test_error_behaviour(gpu_ctx, oracle):
    """Reference panics become error codes; the framebuffer is left untouched (the reference panics before drawing)."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C1")
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx); fb.clear(sc.clear_color)
    before = fb.pixels
    bad = sc.faces.copy(); bad["v"][17, 2] = len(sc.vertices)
    with pytest.raises(R.B32Error) as e:
        R.render_mesh_15(fb, sc.vertices, bad, sc.textures, sc.camera, sc.settings)
    assert e.value.code == b32.abi.B32_E_INDEX and np.array_equal(fb.pixels, before)
    vn = sc.vertices.copy(); vn["pos"][0, 2] = np.nan
    nc = b32.RasterSettings.benchmark(); nc.backface_cull = False      # keep the NaN face alive whatever its winding
    assert oracle.render_mesh_15(oracle.Framebuffer(sc.width, sc.height), vn, sc.faces, sc.textures, sc.camera, nc)[0] == b32.abi.B32_E_NAN_KEY
    with pytest.raises(R.B32Error) as e:
        R.render_mesh_15(fb, vn, sc.faces, sc.textures, sc.camera, nc)
    assert e.value.code == b32.abi.B32_E_NAN_KEY and np.array_equal(fb.pixels, before)
    st = b32.RasterSettings()                     # a light type outside LightType: refused by both sides, frame untouched
    st.lights = [b32.Light(7, position=(0, 0, 0), direction=(0, 0, 1), radius=50.0, angle=0.5)]
    assert oracle.render_mesh_15(oracle.Framebuffer(sc.width, sc.height), sc.vertices, sc.faces, sc.textures, sc.camera, st)[0] == b32.abi.B32_E_ARG
    with pytest.raises(R.B32Error) as e:
        R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, st)
    assert e.value.code == b32.abi.B32_E_ARG and np.array_equal(fb.pixels, before)


def test_smoke_entry():
    import __graft_entry__ as g
    g.smoke()


NEW_MODES = ["C1:ortho", "C1:xray", "C1:xray-zbuf", "C1:default-settings", "C1:wire-painter", "C1:wire-overlay", "cube:default",
             "wire-grid:far-first", "wire-grid:near-first", "C1:spot-gouraud", "C1:spot-flat-zbuf"]


@pytest.mark.parametrize("name", NEW_MODES)
@pytest.mark.parametrize("counting", [1, 0])
def test_editor_modes_parity(gpu_ctx, oracle, name, counting):
    """Orthographic projection (math.rs:140-148), x-ray (render.rs:507-526, 1671-1673) and both wireframe phases
    (render.rs:2574-2635) — the reference's default settings use the back-face wireframe with the z-buffer."""
    sc = SCENES[name]()
    fbo = oracle.Framebuffer(sc.width, sc.height); fbo.clear(sc.clear_color)
    rc, etm, d = oracle.render_mesh_15(fbo, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog, dump=True)
    assert rc == 0
    gpu_ctx.set_fragment_counting(counting)
    try:
        from bonnie32_amd import rasterizer as R
        fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
        fb.clear(sc.clear_color)
        tm = R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
        got = fb.pixels
        assert np.array_equal(got, fbo.pixels), f"{int((got != fbo.pixels).sum())} bytes differ"
        assert hashlib.sha256(got).hexdigest() == HASHES[name]["sha256"]
        assert tm.triangles_drawn == etm.triangles_drawn
        if sc.settings.use_zbuffer:
            assert np.array_equal(fb.zbuffer.view(np.uint32), fbo.zbuffer.view(np.uint32))
        if sc.settings.xray_mode:
            assert tm.fragments == etm.fragments
        assert np.array_equal(gpu_ctx.last_draw_order(len(sc.faces)), d["draw_order"])
    finally:
        gpu_ctx.set_fragment_counting(1)


@pytest.mark.parametrize("case", ["small", "medium", "long-lines", "crowded-tile", "overlay", "both-phases", "both-phases-long", "bands", "one-tile", "huge-lines", "thin-l"])
def test_wireframe_phases_through_screen_tiles(oracle, case):
    """B32_ROUTE_WIRE_TILES: the edges of the wireframe phases (render.rs:2574-2635) binned to 64x16 tiles, first occurrences found in an
    LDS table per tile, lines walked into an LDS bit plane.  Same frame as the oracle (and as the global kernels, route off):
      long-lines    triangles of ~2500 px: edges whose box covers more than 64 wire tiles (WIRE_BIG_TILES) stay with the global kernels, the
                    others go by tile
      crowded-tile  a far camera puts every edge into a few tiles: their lists overflow and the whole frame falls back
      both-phases   back-face wireframe AND front-face overlay in one frame (the overlay is drawn later: it wins where both hit);
                    -long: with edges of both kinds on both routes -- a big back-face edge (global kernels) must not paint over a small
                    overlay edge's pixels (tile kernel): found by the round-4 soak, fixed by the order of the launches
      huge-lines    triangles of ~40 000 px over a 256 x 192 frame (48 wire tiles, so no box is "big"): extents of 2^14 and more take the
                    tile kernel's general 64-bit walk instead of the incremental one
      one-tile      a 64 x 16 frame = one wire tile crossed by the edges of 250 big triangles: as many 16-step segments as one tile gets
                    (the kernel deals them out in passes of WIRE_SEG_CAP; a build with -DB32_WIRE_SEG_CAP=256 runs every case of this test
                    in several passes per tile)
      thin-l        long thin L-shaped triangles on a 2560 x 1920 frame: one edge along a tile row, one along a tile column (each within the
                    64-tile limit), the hypotenuse big -- the box AROUND the two small edges spans thousands of tiles; the face is binned
                    edge box by edge box instead (k_wire_bin), and the frame must stay on the tile route"""
    from bonnie32_amd import rasterizer as R
    cfg = {"thin-l": (3_000, 2560, 1920, 64.0), "small": (2_000, 320, 240, 64.0), "medium": (60_000, 1280, 960, 70.0), "long-lines": (6_000, 1280, 960, 2500.0),
           "crowded-tile": (40_000, 640, 480, 60.0), "overlay": (30_000, 1280, 960, 90.0), "both-phases": (30_000, 640, 480, 120.0), "both-phases-long": (8_000, 1280, 960, 1200.0),
           "bands": (50_000, 1280, 960, 150.0), "one-tile": (250, 64, 16, 150.0), "huge-lines": (400, 256, 192, 40000.0)}[case]
    sc = scenegen.make_scene("C3", n_tris=cfg[0], width=cfg[1], height=cfg[2], bbox_px=cfg[3], seed=31 + cfg[0], variant="gouraud")
    sc.settings = b32.RasterSettings()                                   # default(): z-buffer, Gouraud + light, back-face wireframe
    if case == "thin-l":
        # every face: v0 -> v1 runs 1800 px to the right within one or two tile rows, v0 -> v2 440 px down within one or two tile columns
        # (28 tile rows of 16 px): each edge's own box stays below the 64-tile limit; world coordinates from the screen ones at the face's own depth (camera at the origin, identity basis)
        rng = np.random.default_rng(17)
        pos = sc.vertices["pos"].reshape(-1, 3, 3)
        z = pos[:, :, 2].mean(axis=1, keepdims=True).astype(np.float32)
        vs = np.float32(min(sc.width, sc.height) / 2 * 0.75)
        k = (z + np.float32(5.0)) / np.float32(4.0) / vs
        x0 = rng.uniform(-1200, -900, (len(pos), 1)).astype(np.float32); y0 = rng.uniform(-900, -50, (len(pos), 1)).astype(np.float32)
        flip = rng.integers(0, 2, (len(pos), 1)).astype(bool)                   # half of them wound the other way (back faces: the wireframe's own)
        ax, ay = x0 + np.float32(1800.0), y0 + rng.uniform(-3, 3, (len(pos), 1)).astype(np.float32)
        bx_, by_ = x0 + rng.uniform(-3, 3, (len(pos), 1)).astype(np.float32), y0 + np.float32(440.0)
        sx = np.concatenate([x0, np.where(flip, bx_, ax), np.where(flip, ax, bx_)], axis=1); sy = np.concatenate([y0, np.where(flip, by_, ay), np.where(flip, ay, by_)], axis=1)
        pos[:, :, 0] = sx * k; pos[:, :, 1] = sy * k; pos[:, :, 2] = z
        sc.vertices["pos"] = pos.reshape(-1, 3)
    if case == "crowded-tile":
        sc.camera = b32.Camera(position=(0.0, 0.0, -60000.0))
    if case == "overlay":
        sc.settings.backface_wireframe = False; sc.settings.wireframe_overlay = True
    if case.startswith("both-phases") or case in ("one-tile", "huge-lines"):
        sc.settings.wireframe_overlay = True
    # shared and repeated edges: the second half of the mesh repeats the first half's triangles with other depths
    half = len(sc.faces) // 2
    sc.faces["v"][half:2 * half] = sc.faces["v"][:half]
    sc.faces["v"][half:2 * half:2] = sc.faces["v"][half:2 * half:2][:, [1, 2, 0]]   # ... every other one with its edges in another order
    bands = ((0, 301), (301, 700), (700, 960)) if case == "bands" else ((0, sc.height),)
    fbo = oracle.Framebuffer(sc.width, sc.height); fbo.clear(sc.clear_color)
    rc, etm = oracle.render_mesh_15(fbo, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
    assert rc == 0
    for off in (0, R.Context.ROUTE_WIRE_TILES):
        ctx = R.Context(0); ctx.set_routes(off)
        fb = R.Framebuffer(sc.width, sc.height, ctx)
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        for _ in range(2):                                               # (twice: the tile counters must come back to zero by themselves)
            for band in bands:
                fb.set_band(*band)
                fb.clear(sc.clear_color)
                tm = rs.render(sc.camera, sc.settings, sc.fog)
            fb.set_band(0, sc.height)
            got = fb.pixels
            assert np.array_equal(got, fbo.pixels), f"{case}: {int((got != fbo.pixels).sum())} bytes differ (routes off {off})"
            assert tm.triangles_drawn == etm.triangles_drawn
        assert (ctx.route_counts()["wire_tiles"] > 0) == (off == 0)
        ctx.close()
    if case == "thin-l":        # (sanity of the construction: the two small edges' boxes are far apart, so their union box is huge)
        px = sc.vertices["pos"].reshape(-1, 3, 3)
        assert np.ptp(px[:, :, 0] / px[:, :, 2], axis=1).min() * 720 * 4 > 1500


def test_editor_modes_large_frame_bands(gpu_ctx, oracle):
    """Default settings (z-buffer + Gouraud + back-face wireframe) at 1280x960 with 20 k triangles, drawn as three ragged
    screen bands (multi-GPU sharding): long lines cross tiles and bands, dedup table sized for 60 k edges."""
    sc = scenegen.make_scene("C3", n_tris=20_000, width=1280, height=960, bbox_px=2500.0, seed=99, variant="gouraud")
    sc.settings = b32.RasterSettings()
    fbo = oracle.Framebuffer(sc.width, sc.height); fbo.clear(sc.clear_color)
    rc, etm = oracle.render_mesh_15(fbo, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
    assert rc == 0
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    for band in ((0, 301), (301, 700), (700, 960)):
        fb.set_band(*band)
        fb.clear(sc.clear_color)
        tm = rs.render(sc.camera, sc.settings, sc.fog)
        assert tm.triangles_drawn == etm.triangles_drawn
    fb.set_band(0, sc.height)
    got = fb.pixels
    assert np.array_equal(got, fbo.pixels), f"{int((got != fbo.pixels).sum())} bytes differ"
    assert np.array_equal(fb.zbuffer.view(np.uint32), fbo.zbuffer.view(np.uint32))


def test_wire_edge_overflow_is_refused(gpu_ctx, oracle):
    """An edge >= 2^30 pixels long overflows the reference's i32 Bresenham state: both sides return B32_E_UNSUPPORTED."""
    sc = scenegen.wire_grid_scene()
    sc.settings.use_fixed_point = False
    sc.vertices["pos"][0] = (-3.0e9, 0.0, 1000.0)            # float projection keeps the huge coordinate; `as i32` saturates
    fbo = oracle.Framebuffer(sc.width, sc.height); fbo.clear(sc.clear_color)
    rc, _ = oracle.render_mesh_15(fbo, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
    assert rc == b32.abi.B32_E_UNSUPPORTED
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    with pytest.raises(R.B32Error) as ei:
        R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog)
    assert ei.value.code == b32.abi.B32_E_UNSUPPORTED


@pytest.mark.parametrize("name", list(SCENES8))
@pytest.mark.parametrize("counting", [1, 0])
def test_8bit_path_parity(gpu_ctx, oracle, name, counting):
    """render_mesh (render.rs:1971-2264) + rasterize_triangle (render.rs:1202-1433): the 8-bit-colour path, drop-in and
    resident forms, with and without fragment counting (EXACT / CHEAP coverage where the overwrite pass applies)."""
    sc = SCENES8[name]()
    fbo = oracle.Framebuffer(sc.width, sc.height); fbo.clear(sc.clear_color)
    rc, etm, d = oracle.render_mesh(fbo, sc.vertices, sc.faces, sc.textures8, sc.camera, sc.settings, dump=True)
    assert rc == 0
    from bonnie32_amd import rasterizer as R
    gpu_ctx.set_fragment_counting(counting)
    try:
        for resident in (False, True):
            fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
            fb.clear(sc.clear_color)
            if resident:
                tm = R.ResidentScene(fb, sc.vertices, sc.faces, textures8=sc.textures8).render(sc.camera, sc.settings)
            else:
                tm = R.render_mesh(fb, sc.vertices, sc.faces, sc.textures8, sc.camera, sc.settings)
            got = fb.pixels
            assert np.array_equal(got, fbo.pixels), f"{int((got != fbo.pixels).sum())} bytes differ (resident={resident})"
            assert hashlib.sha256(got).hexdigest() == HASHES[name]["sha256"]
            assert tm.triangles_drawn == etm.triangles_drawn
            if sc.settings.use_zbuffer:
                assert np.array_equal(fb.zbuffer.view(np.uint32), fbo.zbuffer.view(np.uint32))
            if tm.fragments:
                assert tm.fragments == etm.fragments
            assert np.array_equal(gpu_ctx.last_draw_order(len(sc.faces)), d["draw_order"])
    finally:
        gpu_ctx.set_fragment_counting(1)


def test_8bit_scene_rejects_15bit_draw(gpu_ctx):
    from bonnie32_amd import rasterizer as R
    sc = SCENES8["8:cube"]()
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, textures8=sc.textures8)
    rs.fmt8 = False                     # force the RGB555 entry point on an 8-bit scene
    with pytest.raises(R.B32Error) as e:
        rs.render(sc.camera, sc.settings)
    assert e.value.code == b32.abi.B32_E_ARG


@pytest.mark.parametrize("fmt8", [False, True])
def test_zbuffer_fast_path(fast_ctx, oracle, fmt8):
    """z-buffer mode without a transparent pass through the sort-free fused kernel (depth as the visibility priority):
    two meshes drawn onto the same framebuffer (the second one is depth-tested against the first), Gouraud lighting,
    a texture with skippable texels on faces that ignore / honour black_transparent, drawn as ragged bands."""
    from bonnie32_amd import rasterizer as R
    a = scenegen.make_scene("C3", n_tris=60_000, seed=5, variant="gouraud")
    b = scenegen.make_scene("C3", n_tris=40_000, seed=6, variant="gouraud", bbox_px=2000.0)
    for sc in (a, b):
        sc.settings = b32.RasterSettings.game()
        sc.settings.use_rgb555 = not fmt8
        sc.faces["black_transparent"][::3] = 0
    ofb = oracle.Framebuffer(a.width, a.height); ofb.clear(a.clear_color)
    fb = R.Framebuffer(a.width, a.height, fast_ctx)
    for band in ((0, 500), (500, 1301), (1301, 1920)):
        fb.set_band(*band); fb.clear(a.clear_color)
    for sc in (a, b):
        if fmt8:
            t8 = [b32.Texture.from_texture15(t) for t in sc.textures]
            rc, etm = oracle.render_mesh(ofb, sc.vertices, sc.faces, t8, sc.camera, sc.settings)
            rs = R.ResidentScene(fb, sc.vertices, sc.faces, textures8=t8)
        else:
            rc, etm = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
            rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        assert rc == 0
        for band in ((0, 500), (500, 1301), (1301, 1920)):
            fb.set_band(*band)
            tm = rs.render(sc.camera, sc.settings)
            assert tm.triangles_drawn == etm.triangles_drawn
    fb.set_band(0, a.height)
    got = fb.pixels
    assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ"
    assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))


@pytest.mark.parametrize("kind", ["bench", "fog-flat", "blend"])
def test_band_frames_of_a_resident_scene_use_packed_positions(fast_ctx, oracle, kind):
    """Multi-GPU band sharding: every rank culls and bins ALL the faces of the resident scene.  From the second band frame of an uploaded
    mesh on, k_setup does that from packed 12-byte positions and reads the whole vertex (UVs, colours; fog is applied to the colours
    after that) only for faces that reach the band.  Ragged bands rendered three times each (first: whole vertices; then: packed
    positions) must assemble to the oracle's frame, with the oracle's triangle count on every band."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=60_000, seed=808, variant="blend" if kind == "blend" else "bench", width=1280, height=960, bbox_px=700.0)
    if kind == "fog-flat":
        sc.fog = (1000.0, 3000.0, 5500.0, b32.Color(90, 100, 120))
        sc.settings.shading = b32.abi.SHADE_FLAT
        sc.settings.lights = [b32.Light.point((100.0, -50.0, 900.0), 2500.0, 1.5), b32.Light.directional((0.3, -1.0, 0.2), 0.5)]
        sc.settings.backface_cull = False
    exp, etm, d = cpu_render(oracle, sc)
    fb = R.Framebuffer(sc.width, sc.height, fast_ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    bands = ((0, 333), (333, 334), (334, 800), (800, 960))
    for rep in range(3):
        for band in bands:
            fb.set_band(*band); fb.clear(sc.clear_color)
            tm = rs.render(sc.camera, sc.settings, sc.fog)
            assert tm.triangles_drawn == etm.triangles_drawn
        fb.set_band(0, sc.height)
        got = fb.pixels
        assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ ({kind}, repetition {rep})"


def test_fast_path_transparent_lists(fast_ctx, oracle):
    """Scenes with a transparent pass on the sort-free path: binning splits each tile list by class and k_blend ranks the
    transparent part by 64-bit painter's priority in LDS (ties in depth -> face order).  The second scene has far more
    transparent entries per tile than that sort holds, so the frame is redrawn through the general path (nothing of the
    aborted attempt may have touched the framebuffer)."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C5", n_tris=30_000, variant="blend", seed=77)          # 64 depth levels: massive key ties
    sc.faces["blend_mode"][::3] = b32.abi.ADD
    exp, etm, d = cpu_render(oracle, sc)
    for z in (False, True):
        sc.settings.use_zbuffer = z
        ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
        rc, etm = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
        got, tm = gpu_render(fast_ctx, sc, resident=True)
        assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ (zbuffer={z})"
        assert tm.triangles_drawn == etm.triangles_drawn
    big = scenegen.make_scene("C2", n_tris=60_000, width=128, height=64, bbox_px=40.0, seed=78)
    big.faces["blend_mode"][:] = b32.abi.AVERAGE
    big.faces["blend_mode"][::2] = b32.abi.SUBTRACT
    exp, etm, d = cpu_render(oracle, big)
    got, tm = gpu_render(fast_ctx, big, resident=True)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ"
    assert tm.triangles_drawn == etm.triangles_drawn > 2 * 2048 * 2
    # (measured for tests/test_blend_stacks.py: with counting off this redrawn frame reports the oracle's store count; the C5 scene above
    #  reports 0 fragments in either mode, so nothing is compared there.  Exact for the same reason as in the pile test below: these
    #  textures are not cheap_ok, so plan_route takes EXACT coverage)
    assert tm.fragments == etm.fragments != 0


@pytest.mark.parametrize("zbuffer", [False, True])
def test_transparent_pile_on_the_sort_free_path(fast_ctx, oracle, zbuffer):
    """(Measured since, tests/test_blend_stacks.py::test_census_of_the_random_pile_scene: scenegen takes the square root of bbox_px, so this
    scene has triangles 11 pixels wide, 1.2 fragments per covered pixel and at most 5 -- not what the next sentences say; deep stacks,
    several batches and overflowing lists are pinned by tests/test_blend_stacks.py.)
    Every face in the transparent pass, large triangles on a small frame: ~70 blended fragments per pixel and ~150 list entries per
    (cut) tile, still under what k_blend ranks in LDS -- so the frame stays on the sort-free path, and the pixel-centric ordered pass
    runs several 64-surface batches per tile with every lane's fragment list overflowing round after round (all five blend modes,
    editor alpha on some faces: render.rs:479-502, 567-591, 1093-1145)."""
    sc = scenegen.make_scene("C1", n_tris=1500, bbox_px=120.0, seed=4242, variant="blend")
    modes = np.array([b32.abi.AVERAGE, b32.abi.ADD, b32.abi.SUBTRACT, b32.abi.ADD_QUARTER], dtype=sc.faces["blend_mode"].dtype)
    sc.faces["blend_mode"][:] = modes[np.arange(len(sc.faces)) % 4]
    sc.faces["editor_alpha"][::7] = 150
    sc.settings.use_zbuffer = zbuffer
    ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    rc, etm = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    assert rc == 0
    before = fast_ctx.route_counts()
    for resident in (False, True):
        got, tm = gpu_render(fast_ctx, sc, resident=resident)
        assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ (zbuffer={zbuffer}, resident={resident})"
        assert tm.triangles_drawn == etm.triangles_drawn
        # (measured for tests/test_blend_stacks.py: with counting off this scene reports the oracle's count in painter's mode, 0 in z-buffer
        #  mode.  It is exact because the scene's textures have too many skippable texels for CHEAP coverage -- scene.cheap_ok is false, so
        #  plan_route takes EXACT coverage, which counts every store.  If that heuristic changes, this line fails while the frame stays right.)
        if not zbuffer:
            assert tm.fragments == etm.fragments != 0
    after = fast_ctx.route_counts()
    assert after["redraw_global_sort"] == before["redraw_global_sort"] and after["keyed"] == before["keyed"], (before, after)


@pytest.mark.parametrize("name", ["C3:100k", "C1:blend5", "C2:blend"])
def test_every_route_of_the_sort_free_path_gives_the_same_frame(fast_ctx, oracle, name):
    """b32_set_routes switches internal routes off one at a time: binning inside k_setup (large meshes) -> counting-sort launches, list
    collection inside the fill kernel (small meshes) -> binning launch, cut tiles -> 64-row tiles, 16-wave workgroups -> 8 waves, the
    whole sort-free path -> keyed pipelines.  Every combination must give the oracle's frame, and b32_route_count must show the route
    that was asked for."""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    sc = SCENES[name]()
    exp, etm, d = cpu_render(oracle, sc)
    try:
        for off in (0, C.ROUTE_DIRECT_BIN, C.ROUTE_INLINE_BIN, C.ROUTE_DIRECT_BIN | C.ROUTE_INLINE_BIN, C.ROUTE_CUT_TILES, C.ROUTE_WIDE_GROUPS,
                    C.ROUTE_CUT_TILES | C.ROUTE_WIDE_GROUPS | C.ROUTE_DIRECT_BIN, C.ROUTE_SORT_FREE):
            fast_ctx.set_routes(off)
            before = fast_ctx.route_counts()
            got, tm = gpu_render(fast_ctx, sc, resident=True)
            after = fast_ctx.route_counts()
            assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ (routes off: {off})"
            assert tm.triangles_drawn == etm.triangles_drawn
            if off & C.ROUTE_DIRECT_BIN:
                assert after["direct_bin"] == before["direct_bin"]
            if off & C.ROUTE_INLINE_BIN:
                assert after["inline_bin"] == before["inline_bin"]
            if off & C.ROUTE_SORT_FREE:
                assert after["keyed"] > before["keyed"] and after["direct_bin"] == before["direct_bin"] and after["inline_bin"] == before["inline_bin"]
    finally:
        fast_ctx.set_routes(0)


@pytest.mark.parametrize("name", ["C3:100k", "C5:20k", "C3:blend-100k", "span-mix"])
def test_span_coverage_equals_the_per_pixel_inside_test(fast_ctx, oracle, name):
    """B32_ROUTE_SPAN_COVER: painter's CHEAP coverage decides a row by its exact integer interval instead of the reference's per-pixel
    toleranced test (render.rs:1536-1542; proof: tests/test_span_cover.py).  Same frame with the route on and off, the counter shows
    which ran; "span-mix" puts triangles beyond the eligibility limits (|area| > 8192: their batches keep the per-pixel form, where the
    tolerance admits pixels outside the integer triangle) into the same tiles as eligible ones, on a frame whose width is no multiple
    of the tile's."""
    from bonnie32_amd import rasterizer as R
    if name == "span-mix":
        sc = scenegen.make_scene("C3", n_tris=60_000, width=1000, height=700, seed=77)
        big = scenegen.make_scene("C5", n_tris=3_000, width=1000, height=700, bbox_px=40_000.0, seed=78)
        nv = len(sc.vertices)
        faces = big.faces.copy(); faces["v"] += nv
        sc.vertices = np.concatenate([sc.vertices, big.vertices]); sc.faces = np.concatenate([sc.faces, faces])
        rng = np.random.default_rng(5); perm = rng.permutation(len(sc.faces)); sc.faces = sc.faces[perm]
    elif name == "C3:blend-100k":        # a transparent pass beside it (the span form serves the opaque part of every tile list)
        sc = scenegen.make_scene("C3", n_tris=100_000, variant="blend")
    else:
        sc = SCENES[name]()
    exp, etm, d = cpu_render(oracle, sc)
    try:
        for off in (0, R.Context.ROUTE_SPAN_COVER):
            fast_ctx.set_routes(off)
            before = fast_ctx.route_counts()
            got, tm = gpu_render(fast_ctx, sc, resident=True)
            after = fast_ctx.route_counts()
            assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ (routes off: {off})"
            assert tm.triangles_drawn == etm.triangles_drawn
            assert (after["span_cover"] > before["span_cover"]) == (off == 0)
    finally:
        fast_ctx.set_routes(0)


@pytest.mark.parametrize("variant", ["bench", "blend"])
def test_direct_binning_of_a_spatially_ordered_mesh(fast_ctx, oracle, variant):
    """A real mesh is spatially ordered: the faces of one wave of k_setup mostly land in the same tile, and the list append groups them
    (one atomic per group of lanes asking for the same counter, base + rank for its members).  The synthetic scenes are spatially
    random and form almost no groups, so this one is sorted by screen tile (and, second pass, by scanline) first; large triangles
    make multi-tile spans whose later tiles are grouped too."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=120_000, width=1280, height=960, bbox_px=900.0, seed=4711, variant=variant)
    c = sc.vertices["pos"].reshape(-1, 3, 3).mean(axis=1)
    k = (c[:, 2] + 5.0) / 4.0
    vs = min(sc.width, sc.height) / 2 * 0.75
    px = c[:, 0] / k * vs + sc.width / 2; py = c[:, 1] / k * vs + sc.height / 2
    for order in (np.lexsort((px // 64, py // 64)), np.lexsort((px, py // 8))):
        v = sc.vertices.reshape(-1, 3)[order].reshape(-1).copy()
        f = sc.faces[order].copy(); f["v"] = np.arange(3 * len(order), dtype=np.uint32).reshape(-1, 3)
        ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
        rc, etm = oracle.render_mesh_15(ofb, v, f, sc.textures, sc.camera, sc.settings)
        assert rc == 0
        fb = R.Framebuffer(sc.width, sc.height, fast_ctx); fb.clear(sc.clear_color)
        before = fast_ctx.route_counts()
        tm = R.ResidentScene(fb, v, f, sc.textures).render(sc.camera, sc.settings)
        assert fast_ctx.route_counts()["direct_bin"] > before["direct_bin"]
        got = fb.pixels
        assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ"
        assert tm.triangles_drawn == etm.triangles_drawn and tm.tile_pairs > tm.triangles_drawn


def test_direct_binning_region_overflow_and_regrowth(fast_ctx, oracle):
    """Meshes above the in-kernel list collection are binned by k_setup itself into fixed tile regions sized from the mesh (three times
    the mean list, at least 512 entries).  Two thirds of this mesh sit in the four centre tiles of a 300-tile frame, so the first attempt
    overflows a region: nothing may be drawn by it, the frame is redrawn with regions sized from the longest list it reported, and the
    following frames (same context, the other variant with a transparent pass) run with the grown regions."""
    from bonnie32_amd import rasterizer as R
    for variant in ("bench", "blend"):
        sc = scenegen.make_scene("C1", n_tris=30_000, width=1280, height=960, bbox_px=300.0, seed=515, variant=variant)
        sc.vertices["pos"][: 60_000, :2] *= np.float32(0.15)        # (three vertices per face: the first 20 000 faces)
        exp, etm, d = cpu_render(oracle, sc)
        for rep in range(2):
            before = fast_ctx.route_counts()
            got, tm = gpu_render(fast_ctx, sc, resident=True)
            after = fast_ctx.route_counts()
            assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ ({variant}, attempt {rep})"
            assert tm.triangles_drawn == etm.triangles_drawn and tm.tile_pairs >= tm.triangles_drawn > 10_000
            redrawn = after["redraw_region"] - before["redraw_region"]
            assert after["direct_bin"] - before["direct_bin"] == 1 + redrawn and after["counting_sort"] == before["counting_sort"]
            if variant == "bench":
                assert redrawn == (1 if rep == 0 else 0)            # the first frame on this context overflows, the regions stay grown


@pytest.mark.parametrize("counting", [0, 1])
def test_more_tiles_than_the_span_histogram_holds(gpu_ctx, oracle, counting):
    """4160x4160 = 4225 screen tiles: beyond the LDS histogram of the sort-free binning (4096) and beyond one 12-bit radix
    pass, so the frame takes the keyed multi-pass tile sort + k_tile_ranges.  Also the blend variant (two classes per tile)."""
    from bonnie32_amd import rasterizer as R
    for variant in ("bench", "blend"):
        sc = scenegen.make_scene("C1", n_tris=6000, width=4160, height=4160, bbox_px=30000.0, seed=91, variant=variant)
        ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
        rc, etm = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
        assert rc == 0
        gpu_ctx.set_fragment_counting(counting)
        try:
            fb = R.Framebuffer(sc.width, sc.height, gpu_ctx); fb.clear(sc.clear_color)
            tm = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).render(sc.camera, sc.settings)
            got = fb.pixels
            assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ ({variant})"
            assert tm.triangles_drawn == etm.triangles_drawn
            if counting:
                assert tm.fragments == etm.fragments
        finally:
            gpu_ctx.set_fragment_counting(1)


@pytest.mark.parametrize("shading", [1, 2])
@pytest.mark.parametrize("zbuffer", [False, True])
def test_lit_frames_of_large_meshes(gpu_ctx, oracle, shading, zbuffer):
    """Lit frames of a mesh too large for the in-kernel list collection (100 000 faces at 2560x1920): flat and Gouraud shading
    (render.rs:1013-1071, 1466-1483), a directional, a point and a spot light, painter's and z-buffer mode, drop-in and resident (packed
    position / attribute / normal streams from the second frame on), whole frame and a band (surfaces outside the band carry no record
    and no shades) -- through the straight-line shading phase of the fused kernel.  Frame and triangles_drawn against the oracle."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=100_000, variant="gouraud", seed=31 + shading)
    st = copy.copy(sc.settings)
    st.shading = shading; st.use_zbuffer = zbuffer
    st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.point((200.0, -100.0, 2500.0), 4000.0, 1.3),
                 b32.Light.spot((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.6, 9000.0, 1.1)]
    sc.settings = st
    exp, etm, d = cpu_render(oracle, sc)
    got, tm = gpu_render(gpu_ctx, sc)
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ (drop-in)"
    assert tm.triangles_drawn == etm.triangles_drawn
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    for rep in range(3):                                     # (from the second resident frame on: packed position / attribute / normal streams)
        fb.clear(sc.clear_color)
        tm = rs.render(sc.camera, sc.settings, sc.fog)
        got = fb.pixels
        assert np.array_equal(got, exp), f"{int((got != exp).sum())} bytes differ (resident, frame {rep})"
        assert tm.triangles_drawn == etm.triangles_drawn
    row = sc.width * 4
    fb.set_band(700, 1300)
    for rep in range(2):
        fb.clear(b32.Color(1, 2, 3))
        fb.clear(sc.clear_color)
        rs.render(sc.camera, sc.settings, sc.fog)
    part = fb.pixels
    assert np.array_equal(part[700 * row:1300 * row], exp[700 * row:1300 * row])
    fb.set_band(0, sc.height)


def test_lit_stream_is_packed_on_the_first_lit_frame(oracle):
    """The packed vertex streams of a resident large mesh (k_pack_streams): positions + attributes from its second frame on; the 24-byte
    (u, v, rgba, normal) stream only once a frame with a shading pass is drawn -- the buffer is then reallocated and all three streams
    packed again (an unlit mesh no longer pays 72 MB per million faces for a stream nobody reads).  Unlit, unlit,
    unlit, Gouraud, Gouraud, unlit, flat: every frame against the oracle, in safe mode and back to back."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=60_000, width=1280, height=960, variant="gouraud", seed=77)
    lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.point((200.0, -100.0, 2500.0), 4000.0, 1.3)]
    want = {}
    for shading in (0, 1, 2):
        st = copy.copy(sc.settings); st.shading = shading; st.lights = lights
        o = oracle.Framebuffer(sc.width, sc.height); o.clear(sc.clear_color)
        assert oracle.render_mesh_15(o, sc.vertices, sc.faces, sc.textures, sc.camera, st)[0] == 0
        want[shading] = (st, o.pixels.copy())
    for deep in (0, 1):
        ctx = R.Context(0); ctx.set_async_depth(deep)
        fb = R.Framebuffer(sc.width, sc.height, ctx)
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        for i, shading in enumerate((0, 0, 0, 2, 2, 0, 1)):
            st, exp = want[shading]
            fb.clear(sc.clear_color)
            rs.render_async(sc.camera, st)
            got = fb.pixels
            assert np.array_equal(got, exp), f"frame {i} (shading {shading}, deep {deep}): {int((got != exp).sum())} bytes differ"
        rs.finish()
        ctx.close()


@pytest.mark.parametrize("name,ranks", [("C3:100k", 4), ("C1:zbuf", 3), ("C1:blend5", 2)])
def test_cpp_host_drives_band_ranks_through_the_c_abi(tmp_path, name, ranks):
    """tests/cpp/band_harness.cpp: compiled host code (g++, no Python, no torch) drives `ranks` contexts of ONE process through the C ABI
    -- b32_band_attach, b32_set_band, b32_band_publish / _wait / _release / _acquire -- over three frames; the root's framebuffer must
    carry the golden hash of the scene.  (Painter's frames, a z-buffer frame -- every rank keeps the depth rows of its band -- and a frame
    with a transparent pass.)"""
    import subprocess
    from bonnie32_amd import scenefile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "band_harness"
    lib_dir = os.path.join(root, "bonnie-32_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "bonnie-32_amd", "host"), "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "band_harness.cpp"), "-o", str(exe), "-L", lib_dir, "-lb32raster",
                    f"-Wl,-rpath,{lib_dir}"], check=True)
    H = json.load(open(os.path.join(GOLD, "hashes.json")))
    sc = SCENES[name]()
    path = str(tmp_path / "s.b32scene")
    scenefile.write_scene(path, sc)
    out = tmp_path / "out.rgba"
    r = subprocess.run([str(exe), path, str(out), str(ranks), "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert f"triangles_drawn {H[name]['triangles_drawn']}" in r.stdout and "timeouts 0" in r.stdout, r.stdout
    assert hashlib.sha256(out.read_bytes()).hexdigest() == H[name]["sha256"], name


def test_cpp_host_mirror_renders_scene_files(tmp_path):
    """The C++ mirror of the reference interface (host/rasterizer.hpp: b32::Framebuffer, b32::render_mesh_15 / render_mesh with
    reference-shaped Vertex / Face / Texture15 / RasterSettings / Light / fog) compiled with g++, linked against the C ABI and run on the
    GPU FROM `.b32scene` FILES (host/scenefile.hpp): every golden scene but the 1 M-triangle ones -- all the settings, light kinds, fog,
    orthographic views, both pixel formats -- must come out with the frame and depth-buffer hashes of tests/golden/hashes.json.  This is
    the proof that the file format is complete: the same files are what tests/rust/pin_oracle hands to the reference."""
    import subprocess
    from bonnie32_amd import scenefile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "mesh_harness"
    lib_dir = os.path.join(root, "bonnie-32_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "bonnie-32_amd", "host"), "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "mesh_harness.cpp"), "-o", str(exe), "-L", lib_dir, "-lb32raster",
                    f"-Wl,-rpath,{lib_dir}"], check=True)
    H = json.load(open(os.path.join(GOLD, "hashes.json")))
    names = [n for n in list(SCENES) + list(SCENES8) if n not in ("C3", "C5")]
    for name in names:
        sc = (SCENES.get(name) or SCENES8[name])()
        path = str(tmp_path / "s.b32scene")
        scenefile.write_scene(path, sc, expect=H[name])
        r = subprocess.run([str(exe), path, str(tmp_path / "out.rgba"), str(tmp_path / "out.z")], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr)
        assert hashlib.sha256((tmp_path / "out.rgba").read_bytes()).hexdigest() == H[name]["sha256"], name
        assert hashlib.sha256((tmp_path / "out.z").read_bytes()).hexdigest() == H[name]["zbuffer_sha256"], name
        assert f"triangles_drawn {H[name]['triangles_drawn']}" in r.stdout, name
    # the committed sample file (reference-authored cube: draw.rs:138-214, types.rs:702-711)
    r = subprocess.run([str(exe), os.path.join(GOLD, "scenes", "cube.b32scene"), str(tmp_path / "out.rgba")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer((tmp_path / "out.rgba").read_bytes(), np.uint8)
    assert np.array_equal(got, np.load(os.path.join(GOLD, "cube_frame.npz"))["rgba"]) and "triangles_drawn 10" in r.stdout


def test_frames_delivered_by_ticket_without_a_host_round_trip(oracle):
    """The console's render step as the reference runs it: every frame's pixels reach host memory (game/renderer.rs:179-214).
    b32_frame_submit (the frame's mesh table in one call) + b32_fb_download_async into page-locked memory + tickets: the host enqueues
    frame i + 1 while frame i is drawn and copied, the presenter waits for the previous frame's ticket.  Frames alternate between two
    cameras and clear colours; EVERY delivered frame is compared with the oracle's; polling never blocks; a ninth outstanding ticket
    reuses the first one's event; argument errors."""
    from bonnie32_amd import rasterizer as R
    rng = np.random.default_rng(11)
    meshes = [scenegen.make_scene("C1", n_tris=int(rng.integers(300, 2500)), seed=500 + i, variant=("blend" if i % 3 == 2 else "gouraud"),
                                  bbox_px=float(rng.choice([150.0, 400.0]))) for i in range(6)]
    st = b32.RasterSettings.game()
    st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.point((0.0, -100.0, 1500.0), 3000.0, 1.2)]
    fog = (1500.0, 3000.0, 5800.0, b32.Color(40, 50, 70))
    W, H = meshes[0].width, meshes[0].height
    cams = [meshes[0].camera, b32.Camera(position=(40.0, -25.0, 60.0))]
    clears = [b32.Color(10, 10, 30), b32.Color(90, 20, 20)]
    want = []
    for cam, cl in zip(cams, clears):
        o = oracle.Framebuffer(W, H); o.clear(cl)
        for sc in meshes:
            assert oracle.render_mesh_15(o, sc.vertices, sc.faces, sc.textures, cam, st, fog)[0] == 0
        want.append(o.pixels.copy())
    ctx = R.Context(0)                                            # the library's default (safe) mode
    fb = R.Framebuffer(W, H, ctx)
    slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in meshes]
    tables = [ctx.make_frame_table(cam, st, slots, fogs=[fog] * len(slots)) for cam in cams]
    bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
    tickets = [0, 0]
    E = b32.abi.B32_E_ARG
    d = C.c_int()
    assert ctx.lib.b32_ticket_poll(ctx.h, 1, C.byref(d)) == E and ctx.lib.b32_ticket_wait(ctx.h, 0) == E      # no such ticket (yet)
    assert ctx.lib.b32_fb_download_async(ctx.h, None, None) == E
    try:
        n_frames = 21
        for i in range(n_frames):
            fb.clear(clears[i & 1])
            ctx.frame_submit(tables[i & 1])
            tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
            assert isinstance(ctx.ticket_done(tickets[i & 1]), bool)              # (poll: no blocking, either answer is legal here)
            if i > 0:
                ctx.ticket_wait(tickets[(i - 1) & 1])
                got = bufs[(i - 1) & 1][0]
                assert np.array_equal(got, want[(i - 1) & 1]), f"frame {i - 1}: {int((got != want[(i - 1) & 1]).sum())} bytes differ"
        ctx.ticket_wait(tickets[(n_frames - 1) & 1])
        assert ctx.ticket_done(tickets[(n_frames - 1) & 1]) and ctx.ticket_done(1)   # (ticket 1: its event was reused long ago)
        assert np.array_equal(bufs[(n_frames - 1) & 1][0], want[(n_frames - 1) & 1])
        ctx.finish()
        assert ctx.batch_counts()["merged_draws"] > 0
        # pageable memory works too (the call may block)
        plain = np.zeros(W * H * 4, np.uint8)
        t = C.c_uint64()
        assert ctx.lib.b32_fb_download_async(ctx.h, plain.ctypes.data, C.byref(t)) == 0
        ctx.ticket_wait(t.value)
        assert np.array_equal(plain, want[(n_frames - 1) & 1])
    finally:
        for _, p in bufs:
            ctx.host_free(p)
        ctx.close()


def test_cpp_host_mirror_batched_frame(tmp_path, oracle):
    """b32::ResidentMesh + b32::render_frame of the C++ mirror (b32_frame_begin / _add_scene / _end behind them): six meshes from
    .b32scene files -- per-mesh ambient, backface culling and fog travel in the files -- drawn as one frame on the GPU; framebuffer and
    depth buffer must equal the oracle's sequential render_mesh_15 calls, and the frame must really have been drawn as merged runs."""
    import subprocess
    from bonnie32_amd import scenefile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "frame_harness"
    lib_dir = os.path.join(root, "bonnie-32_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "bonnie-32_amd", "host"), "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "frame_harness.cpp"), "-o", str(exe), "-L", lib_dir, "-lb32raster",
                    f"-Wl,-rpath,{lib_dir}"], check=True)
    meshes = _console_meshes(6, 9100, blend_every=3)
    base = b32.RasterSettings.game()
    base.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.point((0.0, -100.0, 1500.0), 3000.0, 1.2)]
    cam = b32.Camera(position=(5.0, -8.0, -30.0))
    fogs = [None, (1500.0, 3000.0, 5800.0, b32.Color(40, 50, 70))]
    W, H = meshes[0].width, meshes[0].height
    ofb = oracle.Framebuffer(W, H); ofb.clear(meshes[0].clear_color)
    paths = []
    for i, sc in enumerate(meshes):
        st = copy.copy(base); st.ambient = 0.15 + 0.1 * i; st.backface_cull = (i != 1)
        sc.settings = st; sc.camera = cam; sc.fog = fogs[i % 2]
        assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, st, sc.fog)[0] == 0
        paths.append(str(tmp_path / f"m{i}.b32scene"))
        scenefile.write_scene(paths[-1], sc)
    r = subprocess.run([str(exe), str(tmp_path / "out.rgba"), str(tmp_path / "out.z")] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer((tmp_path / "out.rgba").read_bytes(), np.uint8)
    gz = np.frombuffer((tmp_path / "out.z").read_bytes(), np.uint32)
    assert np.array_equal(got, ofb.pixels) and np.array_equal(gz, ofb.zbuffer.view(np.uint32))
    assert "merged_draws 2" in r.stdout, r.stdout
    # ... and the console loop of the mirror (b32::FrameLoop: every frame delivered to page-locked memory by ticket) presented the same frame three times
    assert "presented_frames 3" in r.stdout, r.stdout


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_hostile_geometry_every_path(gpu_ctx, oracle, seed):
    """Adversarial inputs through every scheduling path (sort-free fused painter's / z-buffer, transparent pass, instrumented,
    float projection, ortho): positions from 1e-3 to 1e30 and +-inf, coordinates that saturate the 4.12 conversion and the
    `as i32` / `as usize` casts, degenerate and sliver triangles, huge on-screen triangles (every tile), wild UVs (1e9, inf,
    NaN), vertices exactly on / behind the near plane.  NaN positions are excluded only where the reference itself panics
    (NaN sort key).  Bit-exact framebuffers and depth buffers, no hang."""
    from bonnie32_amd import rasterizer as R
    rng = np.random.default_rng(seed)
    n = 900
    v = b32.make_vertices(3 * n); f = b32.make_faces(n, texture_id=0)
    f["v"] = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    z = rng.uniform(0.5, 400.0, n).astype(np.float32)
    scale = (10.0 ** rng.uniform(-1, 2.5, n)).astype(np.float32)
    for k in range(3):
        v["pos"][k::3, 0] = rng.normal(0, 1, n) * scale * (z / 4)
        v["pos"][k::3, 1] = rng.normal(0, 1, n) * scale * (z / 4)
        v["pos"][k::3, 2] = z * (1 + rng.normal(0, 0.2, n))
    big = rng.choice(3 * n, 60, replace=False)
    v["pos"][big[:20], 0] = (10.0 ** rng.uniform(5, 30, 20)) * rng.choice([-1, 1], 20)
    v["pos"][big[20:30], 1] = 3.0e38                       # (+-inf would give inf * 0 = NaN keys: checked separately below)
    v["pos"][big[30:40], 1] = -3.0e38
    v["pos"][big[40:50], 2] = 10.0 ** rng.uniform(6, 30, 10)
    v["pos"][big[50:60], 2] = rng.choice([0.1, 0.100001, 0.0999, -3.0, 0.0], 10)          # near plane (math.rs:155)
    v["pos"][90:93] = v["pos"][93:96]                                                      # degenerate
    v["pos"][96:99, :2] = [[-9000, -7000], [9000, -7000], [0, 9000]]; v["pos"][96:99, 2] = 40.0   # covers the whole screen
    v["uv"] = rng.uniform(-3, 3, (3 * n, 2)).astype(np.float32)
    v["uv"][rng.choice(3 * n, 40, replace=False)] = [1e9, -1e9]
    v["uv"][rng.choice(3 * n, 10, replace=False), 0] = np.inf
    v["uv"][rng.choice(3 * n, 10, replace=False), 1] = np.nan
    v["r"], v["g"], v["b"] = rng.integers(0, 256, (3, 3 * n), dtype=np.uint8)
    f["black_transparent"][::3] = 0
    f["texture_id"][::9] = b32.abi.NO_TEXTURE
    tex = b32.Texture15(64, 32, rng.integers(1, 0x8000, 64 * 32).astype(np.uint16))
    tex.pixels[::97] = 0
    blend_faces = f.copy(); blend_faces["blend_mode"][::6] = b32.abi.ADD; blend_faces["editor_alpha"][1::10] = 90
    cam = b32.Camera(position=(3.0, -2.0, -1.0), basis_x=(0.8, 0.0, -0.6), basis_y=(0.0, 1.0, 0.0), basis_z=(0.6, 0.0, 0.8))
    W, H = 400, 300
    bench = b32.RasterSettings.benchmark
    variants = [
        ("painter", f, bench(), 0), ("painter-nocull", f, b32.RasterSettings(use_zbuffer=False, shading=0, lights=[], backface_wireframe=False, backface_cull=False), 0),
        ("zbuffer-gouraud", f, b32.RasterSettings.game(), 0), ("transparent", blend_faces, bench(), 0),
        ("transparent-z", blend_faces, b32.RasterSettings.game(), 0), ("instrumented", blend_faces, bench(), 1),
        ("float", f, b32.RasterSettings(use_zbuffer=False, shading=0, lights=[], backface_wireframe=False, use_fixed_point=False), 0),
        ("ortho", f, b32.RasterSettings(use_zbuffer=False, shading=0, lights=[], backface_wireframe=False, ortho_projection=(0.7, 1.0, -2.0)), 0),
        ("default+wire", f, b32.RasterSettings(), 0),
    ]
    # the same geometry through the 8-bit-colour path: opaque/erase texels (overwrite pipeline) and blending texels (ordered walk)
    tex8 = b32.Texture.from_texture15(tex)
    tex8b = b32.Texture.from_texture15(tex); tex8b.pixels[::5, 3] = 1 + (np.arange(len(tex8b.pixels[::5])) % 4)
    z8 = b32.RasterSettings(backface_wireframe=False, use_rgb555=False)
    p8 = b32.RasterSettings(use_zbuffer=False, shading=0, lights=[], backface_wireframe=False, use_rgb555=False)
    variants += [("8bit-painter", f, p8, 0, tex8), ("8bit-z-gouraud", f, z8, 0, tex8), ("8bit-blend-painter", blend_faces, p8, 0, tex8b),
                 ("8bit-blend-z", blend_faces, z8, 0, tex8b), ("8bit-instrumented", f, p8, 1, tex8)]
    refused = 0
    for name, faces, st, counting, *t8 in variants:
        ofb = oracle.Framebuffer(W, H); ofb.clear(b32.Color(9, 8, 7))
        if t8:
            rc, etm = oracle.render_mesh(ofb, v, faces, t8, cam, st)
            gpu_draw = lambda fb: R.render_mesh(fb, v, faces, t8, cam, st)
        else:
            rc, etm = oracle.render_mesh_15(ofb, v, faces, [tex], cam, st)
            gpu_draw = lambda fb: R.render_mesh_15(fb, v, faces, [tex], cam, st)
        gpu_ctx.set_fragment_counting(counting)
        try:
            fb = R.Framebuffer(W, H, gpu_ctx); fb.clear(b32.Color(9, 8, 7))
            if rc != 0:                                           # e.g. a wireframe edge longer than 2^30 px: both sides refuse
                with pytest.raises(R.B32Error) as e:
                    gpu_draw(fb)
                assert e.value.code == rc, name
                refused += 1
                continue
            tm = gpu_draw(fb)
            got = fb.pixels
            assert np.array_equal(got, ofb.pixels), f"{name}: {int((got != ofb.pixels).sum())} bytes differ"
            assert tm.triangles_drawn == etm.triangles_drawn, name
            if st.use_zbuffer:
                assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32)), name
            if counting:
                assert tm.fragments == etm.fragments, name
        finally:
            gpu_ctx.set_fragment_counting(1)
    assert refused <= 2, "the scene is meant to be drawn, not refused"
    # an infinite coordinate: inf * 0 = NaN camera depth -> NaN painter's key -> the reference panics; same verdict on both sides
    vi = v.copy(); vi["pos"][96, 1] = np.inf          # a vertex of the screen-filling triangle (never near-culled)
    nocull = b32.RasterSettings(use_zbuffer=False, shading=0, lights=[], backface_wireframe=False, backface_cull=False)
    assert oracle.render_mesh_15(oracle.Framebuffer(W, H), vi, f, [tex], cam, nocull)[0] == b32.abi.B32_E_NAN_KEY
    with pytest.raises(R.B32Error) as e:
        R.render_mesh_15(R.Framebuffer(W, H, gpu_ctx), vi, f, [tex], cam, nocull)
    assert e.value.code == b32.abi.B32_E_NAN_KEY


def test_four_million_triangles(fast_ctx, oracle):
    """Four times the BASELINE triangle count (C4's whole-node load on one GPU): capacities grow on demand (pair buffers are
    re-sized and the frame redrawn on overflow), ids and offsets stay within 32 bits, frame still bit-exact."""
    sc = scenegen.make_scene("C3", n_tris=4_000_000, seed=123)
    exp, etm, d = cpu_render(oracle, sc)
    got, tm = gpu_render(fast_ctx, sc, resident=True)
    assert np.array_equal(got, exp)
    assert tm.triangles_drawn == etm.triangles_drawn == 1938655


KEYED = ["C1", "C1:gouraud", "C1:blend", "C1:blend5", "C1:zbuf-blend5", "C1:float", "C1:persp", "cube", "fog-flat-point-nocull", "C2", "C2:blend", "C1:zbuf", "C1:zbuf-blend",
         "C1:zbuf-gouraud", "C3:100k", "C5:20k", "C1:default-settings", "C1:wire-painter"]


@pytest.mark.parametrize("name", KEYED)
@pytest.mark.parametrize("counting", [1, 0])
def test_keyed_pipelines_parity(keyed_ctx, oracle, name, counting):
    """The pipelines the sort-free path replaced (see conftest.keyed_ctx) against the oracle: still bit-exact, exact counts."""
    sc = SCENES[name]()
    fbo = oracle.Framebuffer(sc.width, sc.height); fbo.clear(sc.clear_color)
    rc, etm, d = oracle.render_mesh_15(fbo, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings, sc.fog, dump=True)
    assert rc == 0
    from bonnie32_amd import rasterizer as R
    keyed_ctx.set_fragment_counting(counting)
    try:
        fb = R.Framebuffer(sc.width, sc.height, keyed_ctx); fb.clear(sc.clear_color)
        tm = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).render(sc.camera, sc.settings, sc.fog)
        got = fb.pixels
        assert np.array_equal(got, fbo.pixels), f"{int((got != fbo.pixels).sum())} bytes differ"
        assert tm.triangles_drawn == etm.triangles_drawn
        if counting and not sc.settings.use_zbuffer:
            assert tm.fragments == etm.fragments
        if sc.settings.use_zbuffer:
            assert np.array_equal(fb.zbuffer.view(np.uint32), fbo.zbuffer.view(np.uint32))
        assert np.array_equal(keyed_ctx.last_draw_order(len(sc.faces)), d["draw_order"])
    finally:
        keyed_ctx.set_fragment_counting(1)


def test_keyed_full_size_c3(keyed_ctx, oracle):
    sc = scenegen.make_scene("C3")
    exp, etm, d = cpu_render(oracle, sc)
    for counting in (1, 0):
        keyed_ctx.set_fragment_counting(counting)
        got, tm = gpu_render(keyed_ctx, sc, resident=True, indexed=True)
        assert np.array_equal(got, exp)
        if counting:
            assert tm.fragments == etm.fragments
    keyed_ctx.set_fragment_counting(1)


def test_ordering_with_torch_streams(oracle):
    """Frames enqueued asynchronously on torch's stream must be ordered with torch's own work on that stream (the RCCL gather
    of bench.py reads the frame right after the fill): torch's default stream is handle 0, which b32_set_stream would read as
    "the context's own stream" -- Context.set_stream maps it to hipStreamLegacy."""
    import torch
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=300_000)
    exp, etm, d = cpu_render(oracle, sc)
    dev = torch.device("cuda", 0)
    for make in (lambda: torch.cuda.default_stream(dev), lambda: torch.cuda.Stream(device=dev)):
        stream = make()
        with torch.cuda.stream(stream):
            ctx = R.Context(0)
            ctx.set_stream(stream.cuda_stream)
            frame = torch.zeros(sc.width * sc.height * 4, dtype=torch.uint8, device=dev)
            fb = R.Framebuffer.__new__(R.Framebuffer); fb.ctx = ctx
            fb.bind_device(frame.data_ptr(), sc.width, sc.height)
            rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
            rs.render(sc.camera, sc.settings)
            for _ in range(6):
                fb.clear(sc.clear_color)
                rs.render_async()
                got = frame.cpu().numpy()              # no b32 synchronisation in between: stream order alone must do
                assert np.array_equal(got, exp)
            rs.finish()
            ctx.close()


def test_scene_slots_multi_mesh_frame(gpu_ctx, oracle):
    """Several resident scenes in one context (b32_scene_swap): a console-style frame -- clear, then room after room onto the same
    framebuffer with persistent depth (scene.rs:112-261) -- enqueued without uploads or host syncs between the meshes, three frames
    with a moving camera.  RGB555 and 8-bit scenes mixed, one mesh above the small-mesh limit (its pending frame is settled by the
    swap), one with a transparent pass."""
    from bonnie32_amd import rasterizer as R
    specs = [("gouraud", 700, False), ("blend", 1500, False), ("gouraud", 5000, False), ("bench", 300, True), ("gouraud", 2048, False)]
    meshes = []
    for i, (variant, n, f8) in enumerate(specs):
        sc = scenegen.make_scene("C1", n_tris=n, seed=900 + i, variant=variant, bbox_px=300.0)
        sc.tex8 = [b32.Texture.from_texture15(t) for t in sc.textures] if f8 else None
        meshes.append(sc)
    st15 = b32.RasterSettings.game(); st15.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.spot((0, 0, -100), (0, 0, 1), 0.6, 6000.0, 1.3)]
    st8 = b32.RasterSettings.game(); st8.use_rgb555 = False
    fog = (1500.0, 3000.0, 5800.0, b32.Color(40, 50, 70))
    W, H = meshes[0].width, meshes[0].height
    gpu_ctx.set_fragment_counting(0)
    try:
        fb = R.Framebuffer(W, H, gpu_ctx)
        slots = [R.ResidentScene(fb, sc.vertices, sc.faces, None if sc.tex8 else sc.textures, textures8=sc.tex8).detach() for sc in meshes]
        ofb = oracle.Framebuffer(W, H)
        for frame in range(3):
            cam = b32.Camera(); cam.position = (10.0 * frame, -5.0 * frame, 20.0 * frame)
            ofb.clear(b32.Color(10, 10, 30)); fb.clear(b32.Color(10, 10, 30))
            for sc, rs in zip(meshes, slots):
                if sc.tex8:
                    assert oracle.render_mesh(ofb, sc.vertices, sc.faces, sc.tex8, cam, st8)[0] == 0
                    rs.render_async(cam, st8)
                else:
                    assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, st15, fog)[0] == 0
                    rs.render_async(cam, st15, fog)
            slots[-1].finish()
            assert np.array_equal(fb.pixels, ofb.pixels), f"frame {frame}"
            assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))
        # an error in the middle of a frame is reported by the finish, the failing mesh draws nothing, the others are drawn
        bad = meshes[1].faces.copy(); bad["v"][7, 1] = 10 ** 6
        bad_rs = R.ResidentScene(fb, meshes[1].vertices, bad, meshes[1].textures).detach()
        cam = b32.Camera()
        ofb.clear(b32.Color(1, 2, 3)); fb.clear(b32.Color(1, 2, 3))
        order = [(meshes[0], slots[0]), (None, bad_rs), (meshes[4], slots[4])]
        for sc, rs in order:
            if sc is None:
                assert oracle.render_mesh_15(ofb, meshes[1].vertices, bad, meshes[1].textures, cam, st15, fog)[0] == b32.abi.B32_E_INDEX
            else:
                assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, st15, fog)[0] == 0
            rs.render_async(cam, st15, fog)
        with pytest.raises(R.B32Error) as e:
            slots[4].finish()
        assert e.value.code == b32.abi.B32_E_INDEX
        assert np.array_equal(fb.pixels, ofb.pixels)
        slots[0].render_async(cam, st15, fog); slots[0].finish()          # the error does not stick beyond the finish that reported it
        for rs in slots + [bad_rs]:
            rs.close()
    finally:
        gpu_ctx.set_fragment_counting(1)


def test_scene_slots_of_every_upload_kind_across_pipeline_depths(oracle):
    """Scene slots of all three upload kinds in one context -- RGB555, 8-bit, one indexed texture (its index atlas + CLUT sampled from
    LDS) -- drawn as pipelined console frames while the pipeline depth changes with buffers in every frame set, and while a larger
    slot uploaded late makes the current set grow beside sets of the old size.  2 500 triangles: just above the 2 048 faces below
    which a frame never takes another frame set; the RGB555 and indexed meshes can have a transparent pass, which sends a mesh of
    that size to the direct-binning route -- the one whose frames run their setup kernel on the side stream.  Every frame's pixels
    and depth against the oracle; what a slot carries (index atlas, format, texel pools) must come back with every swap."""
    from bonnie32_amd import rasterizer as R
    W, H, N = 320, 240, 2500
    rgb = scenegen.make_scene("C1", n_tris=N, seed=3101, variant="blend", width=W, height=H)
    s8 = scenegen.make_scene("C1", n_tris=N, seed=3102, variant="bench", width=W, height=H)
    s8.tex8 = [b32.Texture.from_texture15(t) for t in s8.textures]
    idx = scenegen.make_scene("C1", n_tris=N, seed=3103, variant="bench", width=W, height=H)
    idx.faces["blend_mode"][::40] = b32.abi.AVERAGE
    big = scenegen.make_scene("C1", n_tris=6000, seed=3104, variant="blend", width=W, height=H)
    assert len(idx.indexed_textures) == 1
    st15 = b32.RasterSettings.game(); st15.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.spot((0, 0, -100), (0, 0, 1), 0.6, 6000.0, 1.3)]
    st8 = b32.RasterSettings.game(); st8.use_rgb555 = False
    fog = (1500.0, 3000.0, 5800.0, b32.Color(40, 50, 70))
    ctx = R.Context(0)
    ctx.set_fragment_counting(0)
    fb = R.Framebuffer(W, H, ctx)
    slots = [(rgb, R.ResidentScene(fb, rgb.vertices, rgb.faces, rgb.textures).detach()),
             (idx, R.ResidentScene(fb, idx.vertices, idx.faces, None, indexed_textures=idx.indexed_textures).detach()),
             (s8, R.ResidentScene(fb, s8.vertices, s8.faces, None, textures8=s8.tex8).detach())]
    ofb = oracle.Framebuffer(W, H)
    before = ctx.route_counts()
    idx_frames = 0
    for frame in range(6):
        if frame == 5:      # the current frame set grows (ensure_work) while the other one holds buffers of the old size
            slots.insert(0, (big, R.ResidentScene(fb, big.vertices, big.faces, big.textures).detach()))
        cam = b32.Camera(); cam.position = (8.0 * frame, -4.0 * frame, 15.0 * frame)
        ofb.clear(b32.Color(10, 10, 30)); fb.clear(b32.Color(10, 10, 30))
        for sc, rs in slots:
            if sc is s8:
                assert oracle.render_mesh(ofb, sc.vertices, sc.faces, sc.tex8, cam, st8)[0] == 0
                rs.render_async(cam, st8)
            else:
                assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, cam, st15, fog)[0] == 0
                rs.render_async(cam, st15, fog)
            idx_frames += sc is idx
        slots[-1][1].finish()
        assert np.array_equal(fb.pixels, ofb.pixels), f"frame {frame}: {int((fb.pixels != ofb.pixels).sum())} bytes differ"
        assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32)), f"frame {frame}: depth"
        if frame == 2:
            ctx.set_pipeline_depth(3)
        if frame == 4:
            ctx.set_pipeline_depth(2)
    after = ctx.route_counts()
    assert after["pipelined"] > before["pipelined"]
    # the indexed slot was swapped out after its upload and in again for every draw: atlas_idx_bytes and the atlas travel with it
    assert idx_frames == 6 and after["lds_atlas"] - before["lds_atlas"] >= idx_frames
    for _, rs in slots:
        rs.close()
    ctx.close()


def test_randomised_mode_soak():
    """tools/soak.py for 20 s: random scenes x random settings (both pixel formats, z-buffer, x-ray, ortho, wireframes, fog, lights,
    editor alpha, ragged bands, counting on/off), bit-exact against the oracle.  (Longer runs of the same tool while building found two real bugs -- a record word not loaded for literal-walk surfaces, signed-zero depths -- and then passed ~60 000 scenes over sixteen seeds, spot lights and multi-mesh scene-slot frames included.)"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "soak.py"), "20", "3"], capture_output=True, text=True, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("soak:") and last.endswith(" 0 failures"), r.stdout[-3000:]
    assert int(last.split()[1]) > 50
    # orthographic + z-buffer + hostile coordinates: depths of exactly -0.0 / +0.0 meet in one pixel (the reference's `z < zbuffer`
    # sees them as equal, so one depth key for both, sign of the stored depth recomputed) -- found by this tool
    env = dict(os.environ, SOAK_FORCE="orthoz")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "soak.py"), "15", "21"], capture_output=True, text=True, cwd=root, env=env)
    last = r.stdout.strip().splitlines()[-1]
    assert r.returncode == 0 and last.startswith("soak:") and last.endswith(" 0 failures"), r.stdout[-3000:] + r.stderr[-2000:]
