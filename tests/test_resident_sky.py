"""The resident sky (b32_sky: b32_render_sky from the camera alone) and the star batches through the ordered tile pass (b32_draw_stars).

Expected results come from the oracle as it stands: Framebuffer.render_skybox_mesh on vertices whose positions were placed with numpy f32
(np.float32(cam) + off), and Framebuffer.draw_star_diamonds.  CPU tests pin the mirrors (mirrors/sky.py) and show that the placement rule
can be told from its shortcut; GPU tests compare the device with the oracle byte for byte."""
import contextlib
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi
from bonnie32_amd.mirrors.sky import sky_place, sky_project, star_per, star_records
from bonnie32_amd.records import pack_stars
from tests.test_lines import np_lines
from tests.test_prims import np_prims
from tests.test_sky_present import BOTTOM, CAM, TOP, np_sky, oracle_stars, same, sky_mesh, star_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
I_MAX, I_MIN = 2**31 - 1, -2**31


def cam_at(position):
    """test_sky_present.CAM's basis at another position."""
    return b32.Camera(position=tuple(position), basis_x=CAM.basis_x, basis_y=CAM.basis_y, basis_z=CAM.basis_z)


FAR_1 = cam_at((1000000.3, -2000000.7, 1500000.1))
FAR_2 = cam_at((30000001.0, -20000003.0, 15000001.0))
NEAR = cam_at((1234.567, -98.76, 4321.125))
ORIGIN = cam_at((0.0, 0.0, 0.0))
CAMS = {"cam": CAM, "far1": FAR_1, "far2": FAR_2}
STAR_SIZES = [0.2, 1.0, 1.99, 2.0, 2.99, 3.0, 7.5, float("nan"), float("inf")]

_SKIES = {}


def sky_offsets(name):
    """The skies the tests share, built once: name -> (offsets, faces); the offsets are sky_mesh at the origin."""
    if name not in _SKIES:
        if name == "one":                                                                  # a single face: the first one the 12 x 8 sphere draws
            v, f = sky_offsets("12x8")
            one = np.array([[0, 1, 2]], np.uint32)
            for face in f:
                img = np.zeros((120, 160, 4), np.uint8)
                np_sky(160, 120, sky_place(v[face], CAM.position), one, CAM, img)
                if img.any():
                    _SKIES[name] = (v[face].copy(), one)
                    break
        else:
            hs, vs = (int(x) for x in name.split("x"))
            _SKIES[name] = sky_mesh((0.0, 0.0, 0.0), hs, vs)
    v, f = _SKIES[name]
    v.setflags(write=False); f.setflags(write=False)
    return v, f


def recolour(verts, seed):
    out = verts.copy()
    col = np.random.default_rng(seed).integers(0, 256, (len(out), 3), dtype=np.uint8)
    out["r"], out["g"], out["b"] = col[:, 0], col[:, 1], col[:, 2]
    return out


def oracle_sky_frame(oracle, W, H, offsets, faces, cam, base=None):
    """clear_gradient (or `base`) + the oracle's render_skybox_mesh of the placed vertices -> flat pixels."""
    ofb = oracle.Framebuffer(W, H)
    if base is None:
        ofb.clear_gradient(TOP, BOTTOM)
    else:
        ofb.pixels[:] = base
    if len(offsets) and len(faces):
        assert ofb.render_skybox_mesh(sky_place(offsets, cam.position), faces, cam) == 0
    return ofb.pixels.copy()


def bands_of(H):
    return [(0, H // 3), (H // 3, H), (H, H)]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: layouts, bindings, the C++ mirror

NEW_SYMBOLS = ["b32_sky_create", "b32_sky_destroy", "b32_sky_update", "b32_render_sky", "b32_sky_project_batch", "b32_draw_stars",
               "b32_star_record_count", "b32_star_records_batch"]


@pytest.mark.parametrize("cc,ext", [("gcc", "c"), ("g++", "cpp")])
def test_star_layout_matches_c(cc, ext):
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(B32Star), '
            'offsetof(B32Star, cx), offsetof(B32Star, cy), offsetof(B32Star, r), offsetof(B32Star, g), offsetof(B32Star, b), offsetof(B32Star, _pad), '
            'sizeof(B32SkyVertex)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t." + ext), "w").write(prog)
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t." + ext)], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    fields = abi.STAR_DTYPE.fields
    assert out == [12, 0, 4, 8, 9, 10, 11, 16]
    assert out[:7] == [abi.STAR_DTYPE.itemsize] + [fields[n][1] for n in ("cx", "cy", "r", "g", "b", "_pad")]
    assert abi.SKY_VERTEX_DTYPE.itemsize == out[7]


def test_new_symbols_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    lib = abi.load_library()
    header = open(os.path.join(ROOT, "include", "b32raster.h")).read()
    bound = {n: a for n, _, a in abi.SYMBOLS}
    for n in NEW_SYMBOLS:
        assert n + "(" in header and n in bound and hasattr(lib, n), n
    assert len(bound["b32_sky_create"]) == 6 and len(bound["b32_star_records_batch"]) == 7 and len(bound["b32_draw_stars"]) == 4


def _gxx(args, **kw):
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bonnie-32_amd", "host"), "-I", os.path.join(ROOT, "include")] + args, **kw)


def test_cpp_mirror_sky_compiles():
    """host/rasterizer.hpp: b32::Sky, Framebuffer::draw_stars and FrameLoop::submit's trailing sky compile, and so do the calls of submit
    that existed before (no sky, with a pick, with a pick and a hover)."""
    src = ('#include "rasterizer.hpp"\n'
           'uint64_t f(b32::Framebuffer& fb, b32::FrameLoop& loop, const std::vector<std::pair<const b32::ResidentMesh*, b32::MeshParams>>& m, const b32::Camera& cam,\n'
           '           const b32::RasterSettings& st, const b32::FramePick& pick, const b32::FrameHover& hover) {\n'
           '    b32::Sky sky(fb, std::vector<B32SkyVertex>(3), std::vector<uint32_t>{ 0, 1, 2 });\n'
           '    sky.update(1, std::vector<B32SkyVertex>(2)); sky.render(fb, cam); (void)sky.project(cam, 320, 240);\n'
           '    fb.draw_stars({ B32Star{ 3, 4, 1, 2, 3, 0 } }, 3.0f);\n'
           '    b32::FrameSky fs; fs.sky = &sky; fs.stars.push_back(B32Star{ 1, 2, 3, 4, 5, 0 });\n'
           '    uint64_t t = loop.submit(b32::Color{}, m, cam, st) + loop.submit(b32::Color{}, m, cam, st, &pick) + loop.submit(b32::Color{}, m, cam, st, &pick, &hover);\n'
           '    return t + loop.submit(b32::Color{}, m, cam, st, nullptr, nullptr, &fs);\n}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        _gxx(["-fsyntax-only", os.path.join(d, "t.cpp")], check=True)


def build_sky_host(d):
    lib_dir = os.path.join(ROOT, "bonnie-32_amd", "csrc")
    exe = os.path.join(str(d), "sky_host")
    _gxx(["-O1", os.path.join(ROOT, "tests", "cpp", "sky_host.cpp"), "-o", exe, "-L", lib_dir, "-lb32raster", f"-Wl,-rpath,{lib_dir}"], check=True)
    return exe


def test_cpp_sky_host_builds(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = build_sky_host(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the star records

W_S, H_S = 33, 17
EDGE_X = [-2, -1, 0, W_S - 1, W_S, W_S + 1, I_MAX, I_MAX - 1, I_MIN]
EDGE_Y = [-2, -1, 0, H_S - 1, H_S, H_S + 1, I_MAX, I_MAX - 1, I_MIN]


def edge_stars(seed=5):
    """Every combination of the edge centres, each star with a colour of its own."""
    cx, cy = (a.reshape(-1) for a in np.meshgrid(np.array(EDGE_X, np.int64), np.array(EDGE_Y, np.int64), indexing="ij"))
    return pack_stars(cx, cy, np.random.default_rng(seed).integers(0, 256, (len(cx), 3)))


def star_arrays(stars):
    return stars["cx"], stars["cy"], np.stack([stars["r"], stars["g"], stars["b"]], axis=1)


def oracle_star_frame(oracle, W, H, stars, size):
    return oracle_stars(oracle, W, H, *star_arrays(stars), size).reshape(-1)


def mirror_star_frame(oracle, W, H, stars, size):
    px = oracle_stars(oracle, W, H, [], [], np.zeros((0, 3)), size).reshape(-1).copy()
    np_prims(px, None, W, H, star_records(stars, size))
    return px


@pytest.mark.parametrize("size", STAR_SIZES, ids=repr)
def test_star_records_drawn_equal_the_oracle(oracle, size):
    """star_records drawn by np_prims == the oracle's draw_star_diamonds, byte for byte: the edge centres on both axes (wrapping adds
    included) and a field of overlapping stars."""
    per = star_per(size)
    assert per == (9 if size >= 3 else (5 if size >= 2 else 1))
    for stars in (edge_stars(), pack_stars(*star_field(W_S, H_S))):
        recs = star_records(stars, size)
        assert len(recs) == len(stars) * per and (recs["kind"] == abi.PRIM_FILLED_RECT).all() and (recs["blend"] == abi.OPAQUE).all()
        assert (recs["x0"] == recs["x1"]).all() and (recs["y0"] == recs["y1"]).all()
        want = oracle_star_frame(oracle, W_S, H_S, stars, size)
        assert (want != oracle_star_frame(oracle, W_S, H_S, stars[:0], size)).any()
        same(mirror_star_frame(oracle, W_S, H_S, stars, size), want, f"size {size}")


def test_star_records_order_and_wrap():
    """The per-star order of the header, the dimmed colours, and INT32_MAX + 2 wrapping to a negative coordinate."""
    s = pack_stars([10, I_MAX], [8, I_MIN], [[200, 100, 50], [255, 1, 0]])
    r = star_records(s, 3.0)
    assert [(int(a), int(b)) for a, b in zip(r["x0"][:9] - 10, r["y0"][:9] - 8)] == [(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1), (-2, 0), (2, 0), (0, -2), (0, 2)]
    assert [int(v) for v in r["r"][:9]] == [200] + [int(f32(200) * f32(0.7))] * 4 + [int(f32(200) * f32(0.4))] * 4
    assert int(r["x0"][9 + 2]) == I_MIN and int(r["x0"][9 + 6]) == I_MIN + 1 and int(r["y0"][9 + 3]) == I_MAX and int(r["y0"][9 + 7]) == I_MAX - 1
    assert (r["alpha"] == 255).all() and not r["_pad"].any() and not r["size"].any() and not r["mode"].any()


def test_two_stars_sharing_pixels_both_orders(oracle):
    a = pack_stars([10, 11], [8, 8], [[250, 10, 10], [10, 10, 250]])
    images = []
    for stars in (a, a[::-1]):
        want = oracle_star_frame(oracle, W_S, H_S, stars, 3.0)
        same(mirror_star_frame(oracle, W_S, H_S, stars, 3.0), want, "shared pixels")
        images.append(want.reshape(H_S, W_S, 4))
    assert (images[0] != images[1]).any()
    assert list(images[0][8, 11, :3]) == [10, 10, 250] and list(images[1][8, 11, :3]) == [int(f32(250) * f32(0.7)), 7, 7]    # the later star wins


def test_star_record_count_host_only():
    import __graft_entry__ as g
    g.build()
    from bonnie32_amd import sky
    for size in STAR_SIZES:
        for n in (0, 1, 7, abi.STAR_MAX):
            assert sky.star_record_count(n, size) == n * star_per(size)
        assert sky.star_record_count(7, size) == len(star_records(np.zeros(7, abi.STAR_DTYPE), size))
    assert abi.load_library().b32_star_record_count(3, 3.0, None) == abi.B32_E_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the placement rule can be told from its shortcut

def np_sky_frame(W, H, verts, faces, cam):
    img = np.zeros((H, W, 4), np.uint8)
    np_sky(W, H, verts, faces, cam, img)
    return img


def test_placement_rounds_twice_far_from_the_origin():
    """(c + o) - c != o for most vertices of the 12 x 8 sphere under the far camera, and the frames differ: a kernel that projects the
    offsets themselves is caught.  Measured: 0.89 of the vertices; 22 pixels (far1), 478 pixels (far2)."""
    off, faces = sky_offsets("12x8")
    W, H = 160, 120
    c = np.asarray(FAR_1.position, f32)
    rel = sky_place(off, c)["pos"] - c[None, :]
    moved = (rel != off["pos"]).any(axis=1).mean()
    print("vertices whose (c + o) - c != o:", moved)
    assert moved > 0.5
    shortcut = np_sky_frame(W, H, off, faces, ORIGIN)
    for name, cam in (("far1", FAR_1), ("far2", FAR_2)):
        placed = np_sky_frame(W, H, sky_place(off, cam.position), faces, cam)
        differ = int((placed != shortcut).any(axis=2).sum())
        print(name, "pixels that differ from the shortcut:", differ)
        assert differ >= 1
    # near the origin the two agree: the near cameras alone prove nothing
    assert np.array_equal(np_sky_frame(W, H, sky_place(off, NEAR.position), faces, NEAR), shortcut)


def test_shared_skies_draw_on_the_oracle(oracle):
    """The skies the GPU tests share are the sizes they are named for and the oracle draws them: the spheres under every camera, the
    single face under CAM."""
    W, H = 160, 120
    for mesh, nv in (("12x8", 117), ("24x16", 425), ("one", 3)):
        off, faces = sky_offsets(mesh)
        assert len(off) == nv
        for name, cam in CAMS.items():
            covered = (oracle_sky_frame(oracle, W, H, off, faces, cam) != oracle_sky_frame(oracle, W, H, off[:0], faces, cam)).reshape(-1, 4).any(axis=1).mean()
            assert covered > (0.9 if mesh != "one" else 0.0) or (mesh == "one" and name != "cam"), (mesh, name, covered)


def test_sky_project_is_np_sky_projection():
    """mirrors/sky.sky_project == the projection inside np_sky / the oracle: drawing with it gives the oracle's picture (indirectly, the
    stage tap's reference is pinned)."""
    from tests.test_sky_present import sky_screen_points
    off, _ = sky_offsets("24x16")
    for cam in (CAM, FAR_1, FAR_2):
        sx, sy = sky_screen_points(160, 120, sky_place(off, cam.position), cam)
        xy = sky_project(off, cam, 160, 120)
        assert np.array_equal(np.isnan(sx), np.isnan(xy[:, 0])) and np.array_equal(np.isnan(sy), np.isnan(xy[:, 1]))
        ok = ~np.isnan(sx)
        assert ok.any() and (~ok).any()
        assert np.array_equal(sx[ok].view(np.uint32), xy[ok, 0].view(np.uint32)) and np.array_equal(sy[ok].view(np.uint32), xy[ok, 1].view(np.uint32))


def test_zero_offset_sign_cannot_be_seen():
    """generate_mesh((0, 0, 0), ..) turns an offset of -0.0 into +0.0 (0.0 + -0.0).  No projected coordinate can see it: c + -0.0 and
    c + +0.0 differ only for c == -0.0, by the sign of a zero, and (c + o) - c is +0.0 either way.  Every combination of zero signs in the
    offsets, camera components of both zero signs among them."""
    vals = np.array([-0.0, 0.0, 50.0, -70.0], f32)
    off = np.stack([a.reshape(-1) for a in np.meshgrid(vals, vals, vals, indexing="ij")], axis=1)
    flushed = np.where(off == 0, f32(0.0), off).astype(f32)
    assert (np.signbit(off) != np.signbit(flushed)).any()
    seen = 0
    for cx in (-0.0, 0.0, 2.5):
        for cy in (-0.0, 0.0, -1.0e6):
            for cz in (-0.0, 0.0, 3.0):
                cam = cam_at((cx, cy, cz))
                a, b = sky_project(off, cam, 160, 120), sky_project(flushed, cam, 160, 120)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
                seen += int((~np.isnan(a[:, 0])).sum())
    assert seen > 100


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the resident sky

def _sky_module():
    import __graft_entry__ as g
    g.build()
    from bonnie32_amd import rasterizer as R, sky
    return R, sky


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(160, 120), (7, 5), (640, 480)], ids=lambda s: "%dx%d" % s)
def test_gpu_resident_sky_equals_the_oracle(gpu_ctx, oracle, size):
    """b32_render_sky from the camera alone == the oracle's render_skybox_mesh of the vertices placed with numpy f32, whole and band by
    band, and == b32_render_skybox_mesh of the same placed vertices; the far cameras are the ones a shortcut (rel = offset) fails."""
    R, sky = _sky_module()
    W, H = size
    fb = R.Framebuffer(W, H, gpu_ctx)
    drawn = 0
    for mesh in ("12x8", "24x16", "one"):
        off, faces = sky_offsets(mesh)
        assert len(off) == {"12x8": 117, "24x16": 425, "one": 3}[mesh]
        with sky.ResidentSky(gpu_ctx, off, faces) as s:
            for name, cam in CAMS.items():
                want = oracle_sky_frame(oracle, W, H, off, faces, cam)
                drawn += int((want != oracle_sky_frame(oracle, W, H, off[:0], faces, cam)).any())
                fb.clear_gradient(TOP, BOTTOM)
                s.render(fb, cam)
                same(fb.pixels, want, f"{mesh} {name} whole")
                fb.clear_gradient(TOP, BOTTOM)
                for band in bands_of(H):
                    fb.set_band(*band)
                    s.render(fb, cam)
                fb.set_band(0, H)
                same(fb.pixels, want, f"{mesh} {name} bands")
                fb.clear_gradient(TOP, BOTTOM)
                fb.render_skybox_mesh(sky_place(off, cam.position), faces, cam)
                same(fb.pixels, want, f"{mesh} {name} b32_render_skybox_mesh of the placed vertices")
    assert drawn >= 6                                                                       # the spheres draw under every camera


@pytest.mark.gpu
def test_gpu_sky_stage_tap(gpu_ctx):
    """b32_sky_project_batch == mirrors/sky.sky_project bit for bit; the marker of a vertex behind the camera is the quiet NaN
    0x7FC00000 on both sides.  Where the arithmetic itself yields a NaN (NaN and infinite offsets: inf * 0, inf - inf) both sides must
    have one, but its payload and sign are the hardware's (IEEE leaves them open) and k_sky_fill reads `x != x` only."""
    R, sky = _sky_module()
    off, faces = sky_offsets("12x8")
    extra = np.zeros(16, abi.SKY_VERTEX_DTYPE)
    nan, inf = float("nan"), float("inf")
    extra["pos"] = [(nan, 1, 2), (1, nan, 2), (1, 2, nan), (inf, 0, 0), (-inf, 0, 0), (0, 0, inf), (0, 0, -inf), (3e38, 3e38, 3e38),
                    (-3e38, 0, 3e38), (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (-0.0, 0.0, 100.0), (0.0, -0.0, 100.0), (100.0, -0.0, 0.0),
                    (3e38, -0.0, 1.0), (5.0, 5.0, -5.0)]
    v = np.concatenate([off, extra])
    with sky.ResidentSky(gpu_ctx, v, faces) as s:
        for name, cam in CAMS.items():
            for W, H in ((160, 120), (7, 5), (16384, 1)):
                got, want = s.project_batch(cam, W, H), sky_project(v, cam, W, H)
                gn, wn = np.isnan(got), np.isnan(want)
                assert np.array_equal(gn, wn), f"{name} {W}x{H}: NaN positions"
                assert np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]), f"{name} {W}x{H}"
                marker = want.view(np.uint32) == 0x7FC00000
                assert marker.any() and (~wn).any()
                assert (got.view(np.uint32)[marker] == 0x7FC00000).all(), f"{name} {W}x{H}: markers"
        cam = CAM.pack()
        xy = np.zeros((len(v), 2), f32)
        for w, h in ((0, 5), (5, 0), (16385, 5), (5, 16385)):
            assert gpu_ctx.lib.b32_sky_project_batch(gpu_ctx.h, s._h, C.byref(cam), w, h, xy.ctypes.data) == abi.B32_E_ARG
        assert gpu_ctx.lib.b32_sky_project_batch(gpu_ctx.h, s._h, C.byref(cam), 5, 5, None) == abi.B32_E_ARG
        assert not xy.any()


@pytest.mark.gpu
def test_gpu_sky_update_ranges_and_stream_order(gpu_ctx, oracle):
    R, sky = _sky_module()
    W, H = 160, 120
    off, faces = sky_offsets("12x8")
    nv = len(off)
    fb = R.Framebuffer(W, H, gpu_ctx)
    cam = FAR_1
    bufs = [gpu_ctx.host_alloc(W * H * 4) for _ in range(2)]
    try:
        with sky.ResidentSky(gpu_ctx, off, faces) as s:
            def check(verts, what):
                fb.clear_gradient(TOP, BOTTOM)
                s.render(fb, cam)
                same(fb.pixels, oracle_sky_frame(oracle, W, H, verts, faces, cam), what)
            cur = recolour(off, 41)
            cur["pos"][:, 1] *= f32(0.7)                                                    # offsets change too
            s.update(0, cur)
            check(cur, "first = 0, count = nv")
            assert (oracle_sky_frame(oracle, W, H, cur, faces, cam) != oracle_sky_frame(oracle, W, H, off, faces, cam)).any()
            last = recolour(off, 42)[nv - 1:]
            s.update(nv - 1, last)
            cur[nv - 1:] = last
            check(cur, "first = nv - 1, count = 1")
            mid = recolour(off, 43)[30:50]
            s.update(30, mid)
            cur[30:50] = mid
            check(cur, "first = 30, count = 20")
            s.update(5, cur[:0])                                                            # count == 0
            assert gpu_ctx.lib.b32_sky_update(gpu_ctx.h, s._h, nv, 0, None) == abi.B32_OK
            bad = recolour(off, 44)
            for first, count, ptr in ((1, nv, bad.ctypes.data), (nv, 1, bad.ctypes.data), (0xFFFFFFFF, 2, bad.ctypes.data), (0, nv, None)):
                assert gpu_ctx.lib.b32_sky_update(gpu_ctx.h, s._h, first, count, ptr) == abi.B32_E_ARG
            check(cur, "after the rejected updates")
            # order on the stream: a render enqueued before the update sees the old vertices, one enqueued after it the new ones
            new = recolour(cur, 45)
            old_want, new_want = oracle_sky_frame(oracle, W, H, cur, faces, cam), oracle_sky_frame(oracle, W, H, new, faces, cam)
            assert (old_want != new_want).mean() > 0.3
            fb.clear_gradient(TOP, BOTTOM)
            s.render(fb, cam)
            t0 = gpu_ctx.download_async(bufs[0][1])
            arr = new.copy()
            s.update(0, arr)
            arr[:] = recolour(arr, 46)                                                      # the caller reuses its array at once
            s.render(fb, cam)
            t1 = gpu_ctx.download_async(bufs[1][1])
            gpu_ctx.ticket_wait(t0); gpu_ctx.ticket_wait(t1)
            same(bufs[0][0], old_want, "the render enqueued before the update")
            same(bufs[1][0], new_want, "the render enqueued after the update")
    finally:
        for _, p in bufs:
            gpu_ctx.host_free(p)


def cylinder_lines(W, H, z):
    """A ring of depth-tested segments (B32_LINE_3D) at depth z around the middle of the frame, and its verticals."""
    n = 16
    a = 2 * np.pi * np.arange(n + 1) / n
    x, y = (W / 2 + W / 3 * np.cos(a)).astype(np.int32), (H / 2 + H / 8 * np.sin(a)).astype(np.int32)
    L = np.zeros(3 * n, abi.LINE_DTYPE)
    for k, dy in enumerate((-H // 4, H // 4)):
        s = L[k * n:(k + 1) * n]
        s["x0"], s["y0"], s["x1"], s["y1"] = x[:-1], y[:-1] + dy, x[1:], y[1:] + dy
    s = L[2 * n:]
    s["x0"], s["y0"], s["x1"], s["y1"] = x[:-1], y[:-1] - H // 4, x[:-1], y[:-1] + H // 4
    L["z0"], L["z1"] = z, z
    L["r"], L["g"], L["b"], L["kind"], L["alpha"] = 40, 255, 90, abi.LINE_3D, 255
    return L


@pytest.mark.gpu
@pytest.mark.parametrize("deep", [0, 1], ids=["safe", "async_depth_1"])
def test_gpu_sky_and_stars_in_the_console_loop(oracle, deep):
    """Nine frames -- clear, sky.update (new colours every frame: the ring of four slots wraps twice), sky.render (two cameras in turn),
    draw_stars (200 stars of size 3), frame_submit of two meshes with the z-buffer, a depth-tested cylinder, download_async -- with the
    presenter one frame behind: every delivered frame is the oracle's."""
    from bonnie32_amd import scenegen
    R, sky = _sky_module()
    meshes = [scenegen.make_scene("C1", n_tris=n, seed=700 + i, variant="gouraud", bbox_px=bb) for i, (n, bb) in enumerate(((1500, 150.0), (700, 400.0)))]
    W, H = meshes[0].width, meshes[0].height
    st = b32.RasterSettings.game()
    assert st.use_zbuffer
    cams = [meshes[0].camera, b32.Camera(position=(40.0, -25.0, 60.0))]
    off, faces = sky_offsets("24x16")
    rng = np.random.default_rng(17)
    stars = pack_stars(rng.integers(-3, W + 3, 200), rng.integers(-3, H + 3, 200), rng.integers(0, 256, (200, 3)))
    black = b32.Color(0, 0, 0)
    n_frames = 9
    colours = [recolour(off, 900 + i) for i in range(n_frames)]
    want, hidden = [], 0
    lines = None
    for i in range(n_frames):
        cam = cams[i & 1]
        o = oracle.Framebuffer(W, H)
        o.clear(black)
        assert o.render_skybox_mesh(sky_place(colours[i], cam.position), faces, cam) == 0
        o.draw_star_diamonds(*star_arrays(stars), 3.0)
        for sc in meshes:
            assert oracle.render_mesh_15(o, sc.vertices, sc.faces, sc.textures, cam, st)[0] == 0
        if lines is None:
            depths = o.zbuffer[o.zbuffer < f32(3.0e38)]
            assert len(depths) > 1000
            lines = cylinder_lines(W, H, f32(np.median(depths)))
        px = o.pixels.copy()
        np_lines(px, o.zbuffer, W, H, lines)
        free = o.pixels.copy()
        np_lines(free, None, W, H, lines)
        hidden += int((free != px).any())
        assert (px != o.pixels).any()                                                      # part of the cylinder shows ...
        want.append(px)
    assert hidden >= 1                                                                      # ... and part of it is behind a mesh
    assert (want[0] != want[2]).mean() > 0.2 and (want[0] != want[1]).mean() > 0.2
    ctx = R.Context(0)
    bufs = []
    try:
        ctx.set_async_depth(deep)
        fb = R.Framebuffer(W, H, ctx)
        slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in meshes]
        tables = [ctx.make_frame_table(cam, st, slots) for cam in cams]
        bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
        tickets = [0, 0]
        with sky.ResidentSky(ctx, off, faces) as s:
            for i in range(n_frames):
                fb.clear(black)
                arr = colours[i].copy()
                s.update(0, arr)
                arr[:] = colours[(i + 1) % n_frames]                                        # the caller reuses its array at once
                s.render(fb, cams[i & 1])
                sky.draw_stars(fb, stars, 3.0)
                ctx.frame_submit(tables[i & 1])
                fb.draw_lines(lines)
                tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
                if i > 0:
                    ctx.ticket_wait(tickets[(i - 1) & 1])
                    same(bufs[(i - 1) & 1][0], want[i - 1], f"frame {i - 1}")
            ctx.ticket_wait(tickets[(n_frames - 1) & 1])
            same(bufs[(n_frames - 1) & 1][0], want[n_frames - 1], f"frame {n_frames - 1}")
            ctx.finish()
        for sl in slots:
            sl.close()
    finally:
        for _, p in bufs:
            ctx.host_free(p)
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the star batches

def gpu_star_frame(R, sky, ctx, W, H, stars, size, bands=None):
    fb = R.Framebuffer(W, H, ctx)
    fb.clear_gradient(TOP, BOTTOM)
    for band in bands or [(0, H)]:
        fb.set_band(*band)
        sky.draw_stars(fb, stars, size)
    fb.set_band(0, H)
    return fb.pixels


ROUTE_KEYS = ("prim_tiles", "prim_scan")


@contextlib.contextmanager
def route(R, ctx, key):
    """The tile route on ("prim_tiles") or switched off ("prim_scan"), switched on again whatever happens inside."""
    ctx.set_routes(0 if key == "prim_tiles" else R.Context.ROUTE_PRIM_TILES)
    try:
        yield
    finally:
        ctx.set_routes(0)


@pytest.mark.gpu
@pytest.mark.parametrize("size", STAR_SIZES, ids=repr)
def test_gpu_star_sizes_and_wrapping_centres(gpu_ctx, oracle, size):
    """The sizes either side of both thresholds, NaN and +inf; the edge centres with their wrapping adds; the field of overlapping
    stars -- on the tile route and with it switched off; the stage tap equals the mirror's records bit for bit, padding included."""
    R, sky = _sky_module()
    for stars in (edge_stars(), pack_stars(*star_field(W_S, H_S))):
        want = oracle_star_frame(oracle, W_S, H_S, stars, size)
        for key in ROUTE_KEYS:
            with route(R, gpu_ctx, key):
                c0 = gpu_ctx.route_counts()[key]
                same(gpu_star_frame(R, sky, gpu_ctx, W_S, H_S, stars, size), want, f"size {size} {key}")
                assert gpu_ctx.route_counts()[key] == c0 + 1                                 # 60 and 81 stars: more than PRIM_SMALL records
        got = sky.star_records_batch(gpu_ctx, stars, size)
        assert got.tobytes() == star_records(stars, size).tobytes()


@pytest.mark.gpu
def test_gpu_star_edge_centres_one_by_one(gpu_ctx, oracle):
    """Each edge centre alone (nothing another star draws can hide what it writes), size 3."""
    R, sky = _sky_module()
    stars = edge_stars()
    fb = R.Framebuffer(W_S, H_S, gpu_ctx)
    background = oracle_star_frame(oracle, W_S, H_S, stars[:0], 3.0)
    written = 0
    for i in range(len(stars)):
        want = oracle_star_frame(oracle, W_S, H_S, stars[i:i + 1], 3.0)
        written += int((want != background).reshape(-1, 4).any(axis=1).sum())
        fb.clear_gradient(TOP, BOTTOM)
        sky.draw_stars(fb, stars[i:i + 1], 3.0)
        same(fb.pixels, want, f"centre ({stars['cx'][i]}, {stars['cy'][i]})")
    assert written >= 4 * 5


@pytest.mark.gpu
def test_gpu_star_bands(gpu_ctx, oracle):
    R, sky = _sky_module()
    stars = pack_stars(*star_field(W_S, H_S))
    want = oracle_star_frame(oracle, W_S, H_S, stars, 3.0)
    background = oracle_star_frame(oracle, W_S, H_S, stars[:0], 3.0)
    same(gpu_star_frame(R, sky, gpu_ctx, W_S, H_S, stars, 3.0, [(0, 5), (5, 6), (6, 6), (6, H_S)]), want, "composite of the bands")
    alone = background.reshape(H_S, -1).copy(); alone[5:6] = want.reshape(H_S, -1)[5:6]
    assert (want.reshape(H_S, -1)[4:7] != background.reshape(H_S, -1)[4:7]).any(axis=1).all()
    same(gpu_star_frame(R, sky, gpu_ctx, W_S, H_S, stars, 3.0, [(5, 6)]), alone.reshape(-1), "band (5, 6) alone")
    same(gpu_star_frame(R, sky, gpu_ctx, W_S, H_S, stars[:5], 3.0, [(5, 6)]),                 # 45 records: the small form honours the band too
         np.where((np.arange(H_S * W_S * 4) // (W_S * 4) == 5), oracle_star_frame(oracle, W_S, H_S, stars[:5], 3.0), background), "band (5, 6), 5 stars")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 6, 64, 65, 2000])
def test_gpu_star_batch_sizes(gpu_ctx, oracle, n):
    """Either side of PRIM_SMALL (45 and 54 records), either side of the by-value form (64 and 65 stars), and 2000 stars."""
    R, sky = _sky_module()
    W, H = 160, 120
    rng = np.random.default_rng(100 + n)
    stars = pack_stars(rng.integers(-3, W + 3, n), rng.integers(-3, H + 3, n), rng.integers(0, 256, (n, 3)))
    if n >= 2:
        stars["cx"][n // 2] = stars["cx"][0] + 1; stars["cy"][n // 2] = stars["cy"][0]      # overlapping sprites: the order matters
    want = oracle_star_frame(oracle, W, H, stars, 3.0)
    for key in ROUTE_KEYS:
        with route(R, gpu_ctx, key):
            c0 = gpu_ctx.route_counts()
            same(gpu_star_frame(R, sky, gpu_ctx, W, H, stars, 3.0), want, f"n = {n} {key}")
            c1 = gpu_ctx.route_counts()
        tiled = 9 * n > 48 and key == "prim_tiles"
        assert c1["prim_tiles"] - c0["prim_tiles"] == (1 if tiled else 0) and c1["prim_scan"] - c0["prim_scan"] == (0 if tiled else 1)
    arr = stars.copy()
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear_gradient(TOP, BOTTOM)
    sky.draw_stars(fb, arr, 3.0)
    arr[:] = 0                                                                              # the array is reusable as soon as the call returns
    same(fb.pixels, want, f"n = {n}, array reused")
    assert sky.star_records_batch(gpu_ctx, stars, 3.0).tobytes() == star_records(stars, 3.0).tobytes()


@pytest.mark.gpu
def test_gpu_stars_overflow_one_tile_list(gpu_ctx, oracle):
    """120 stars of size 3 with distinct colours, all inside the first 64 x 16 tile: 1080 records, more than the 1024 a tile list holds."""
    R, sky = _sky_module()
    W, H = 160, 48
    rng = np.random.default_rng(9)
    n = 120
    col = rng.permutation(256 * 256)[:n]
    stars = pack_stars(rng.integers(2, 62, n), rng.integers(2, 14, n), np.stack([col % 256, col // 256, np.arange(n) + 100], axis=1))
    assert len(np.unique(star_arrays(stars)[2], axis=0)) == n and len(star_records(stars, 3.0)) == 1080
    want = oracle_star_frame(oracle, W, H, stars, 3.0)
    assert (want != oracle_star_frame(oracle, W, H, stars[::-1], 3.0)).any()
    for key in ROUTE_KEYS:
        with route(R, gpu_ctx, key):
            c0 = gpu_ctx.route_counts()[key]
            same(gpu_star_frame(R, sky, gpu_ctx, W, H, stars, 3.0), want, key)
            assert gpu_ctx.route_counts()[key] == c0 + 1


@pytest.mark.gpu
def test_gpu_deferred_clear_before_resident_sky_and_stars(gpu_ctx, oracle):
    """b32_fb_clear defers itself: b32_render_sky and b32_draw_stars that come first must see the cleared frame (draw_enter)."""
    R, sky = _sky_module()
    W, H = 160, 120
    red = b32.Color(200, 10, 10)
    ball, faces = sky_mesh((0.0, 0.0, 200.0), radius=50.0)                                  # a ball in front of the camera: most pixels stay cleared
    cam = b32.Camera()
    ofb = oracle.Framebuffer(W, H); ofb.clear(red)
    assert ofb.render_skybox_mesh(sky_place(ball, cam.position), faces, cam) == 0
    covered = (ofb.image()[:, :, :3] != (200, 10, 10)).any(axis=2).mean()
    assert 0.02 < covered < 0.6
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear_gradient(TOP, BOTTOM)
    with sky.ResidentSky(gpu_ctx, ball, faces) as s:
        fb.clear(red)
        s.render(fb, cam)
        same(fb.pixels, ofb.pixels, "clear + sky")
    stars = pack_stars(*star_field(W, H))
    for part in (stars, stars[:3]):                                                         # the tile route and the small form
        ofb.clear(red); ofb.draw_star_diamonds(*star_arrays(part), 3.0)
        fb.clear_gradient(TOP, BOTTOM)
        fb.clear(red); sky.draw_stars(fb, part, 3.0)
        same(fb.pixels, ofb.pixels, f"clear + {len(part)} stars")


@pytest.mark.gpu
def test_gpu_sky_and_star_contract(gpu_ctx, oracle):
    R, sky = _sky_module()
    lib, h = gpu_ctx.lib, gpu_ctx.h
    W, H = 160, 120
    off, faces = sky_offsets("12x8")
    nv, nf = len(off), len(faces)
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear_gradient(TOP, BOTTOM)
    base = fb.pixels
    cam = CAM.pack()
    out = C.c_void_p(0x1234)
    # NULL arguments
    assert lib.b32_sky_create(None, off.ctypes.data, nv, faces.ctypes.data, nf, C.byref(out)) == abi.B32_E_ARG
    assert lib.b32_sky_create(h, off.ctypes.data, nv, faces.ctypes.data, nf, None) == abi.B32_E_ARG
    assert lib.b32_sky_create(h, None, nv, faces.ctypes.data, nf, C.byref(out)) == abi.B32_E_ARG
    assert lib.b32_sky_create(h, off.ctypes.data, nv, None, nf, C.byref(out)) == abi.B32_E_ARG
    # a face index equal to nv: B32_E_INDEX, *out untouched
    bad = faces.copy(); bad[-1, 2] = nv
    assert lib.b32_sky_create(h, off.ctypes.data, nv, bad.ctypes.data, nf, C.byref(out)) == abi.B32_E_INDEX
    assert out.value == 0x1234
    lib.b32_sky_destroy(h, None)                                                            # no-op
    one = pack_stars([5], [5], [[1, 2, 3]])
    n_rec = C.c_uint32(77)
    recs = np.zeros(9, abi.PRIM_DTYPE)
    assert lib.b32_draw_stars(None, one.ctypes.data, 1, 3.0) == abi.B32_E_ARG
    assert lib.b32_draw_stars(h, None, 1, 3.0) == abi.B32_E_ARG
    assert lib.b32_star_records_batch(h, one.ctypes.data, 1, 3.0, recs.ctypes.data, 9, None) == abi.B32_E_ARG
    assert lib.b32_star_records_batch(h, None, 1, 3.0, recs.ctypes.data, 9, C.byref(n_rec)) == abi.B32_E_ARG
    assert lib.b32_star_records_batch(h, one.ctypes.data, 1, 3.0, recs.ctypes.data, 8, C.byref(n_rec)) == abi.B32_E_ARG     # cap too small
    assert lib.b32_star_records_batch(h, one.ctypes.data, 1, 3.0, None, 9, C.byref(n_rec)) == abi.B32_E_ARG
    assert not recs.view(np.uint8).any()
    # more stars than the pass can count (nothing is read: the batch is refused first)
    assert lib.b32_draw_stars(h, one.ctypes.data, abi.STAR_MAX + 1, 3.0) == abi.B32_E_UNSUPPORTED
    assert lib.b32_star_records_batch(h, one.ctypes.data, abi.STAR_MAX + 1, 1.0, recs.ctypes.data, 9, C.byref(n_rec)) == abi.B32_E_UNSUPPORTED
    # n == 0
    assert lib.b32_draw_stars(h, None, 0, 3.0) == abi.B32_OK
    assert lib.b32_star_records_batch(h, None, 0, 3.0, None, 0, C.byref(n_rec)) == abi.B32_OK and n_rec.value == 0
    other = R.Context(0)
    bare = R.Context(0)
    try:
        fb2 = R.Framebuffer(W, H, other)
        with sky.ResidentSky(gpu_ctx, off, faces) as a, sky.ResidentSky(gpu_ctx, recolour(off, 7), faces) as b, \
                sky.ResidentSky(gpu_ctx, off[:0], faces[:0]) as empty, sky.ResidentSky(gpu_ctx, off, faces[:0]) as faceless, \
                sky.ResidentSky(bare, off, faces) as unframed:
            assert lib.b32_render_sky(None, a._h, C.byref(cam)) == abi.B32_E_ARG
            assert lib.b32_render_sky(h, None, C.byref(cam)) == abi.B32_E_ARG
            assert lib.b32_render_sky(h, a._h, None) == abi.B32_E_ARG
            assert lib.b32_sky_update(None, a._h, 0, 1, off.ctypes.data) == abi.B32_E_ARG
            assert lib.b32_sky_update(h, None, 0, 1, off.ctypes.data) == abi.B32_E_ARG
            assert lib.b32_sky_project_batch(h, None, C.byref(cam), W, H, recs.ctypes.data) == abi.B32_E_ARG
            # a sky of another context
            xy = np.zeros((nv, 2), f32)
            assert lib.b32_render_sky(other.h, a._h, C.byref(cam)) == abi.B32_E_ARG
            assert lib.b32_sky_update(other.h, a._h, 0, 1, off.ctypes.data) == abi.B32_E_ARG
            assert lib.b32_sky_project_batch(other.h, a._h, C.byref(cam), W, H, xy.ctypes.data) == abi.B32_E_ARG
            assert not xy.any()
            with pytest.raises(R.B32Error):
                a.render(fb2, CAM)
            # a context with no framebuffer
            assert lib.b32_render_sky(bare.h, unframed._h, C.byref(cam)) == abi.B32_E_ARG
            assert lib.b32_draw_stars(bare.h, one.ctypes.data, 1, 3.0) == abi.B32_E_ARG
            # skies without vertices or without faces draw nothing
            empty.render(fb, CAM); faceless.render(fb, CAM); empty.update(0, off[:0])
            assert empty.project_batch(CAM, W, H).shape == (0, 2)
            sky.draw_stars(fb, one[:0], 3.0)
            same(fb.pixels, base, "no-ops")
            # two skies of one context are independent
            want_a, want_b = oracle_sky_frame(oracle, W, H, off, faces, CAM), oracle_sky_frame(oracle, W, H, recolour(off, 7), faces, CAM)
            assert (want_a != want_b).mean() > 0.3
            a.render(fb, CAM); same(fb.pixels, want_a, "sky a")
            b.render(fb, CAM); same(fb.pixels, want_b, "sky b")
            a.update(0, recolour(off, 8))
            b.render(fb, CAM); same(fb.pixels, want_b, "sky b after an update of sky a")
            a.render(fb, CAM); same(fb.pixels, oracle_sky_frame(oracle, W, H, recolour(off, 8), faces, CAM), "sky a after its update")
    finally:
        other.close()
        bare.close()


@pytest.mark.gpu
def test_gpu_cpp_sky_host(tmp_path, oracle):
    """tests/cpp/sky_host.cpp: four frames of b32::FrameLoop::submit(.., &sky) -- clear, b32::Sky::render, Framebuffer::draw_stars, one
    mesh, delivered by ticket -- with two cameras in turn; the delivered frames are the oracle's."""
    import __graft_entry__ as g
    g.build()
    from bonnie32_amd import scenefile, scenegen
    exe = build_sky_host(tmp_path)
    sc = scenegen.make_scene("C1", n_tris=900, seed=77, variant="gouraud", bbox_px=200.0)
    sc.settings = b32.RasterSettings.game()
    sc.fog = None
    W, H = sc.width, sc.height
    off, faces = sky_offsets("24x16")
    rng = np.random.default_rng(3)
    stars = pack_stars(rng.integers(-3, W + 3, 150), rng.integers(-3, H + 3, 150), rng.integers(0, 256, (150, 3)))
    cams = [sc.camera, b32.Camera(position=(40.0, -25.0, 60.0)), FAR_1, sc.camera]
    scenefile.write_scene(str(tmp_path / "m.b32scene"), sc)
    with open(tmp_path / "sky.bin", "wb") as f:
        f.write(np.array([len(off), len(faces), len(stars), len(cams)], np.uint32).tobytes() + f32(3.0).tobytes())
        f.write(off.tobytes() + np.ascontiguousarray(faces, np.uint32).tobytes() + stars.tobytes())
        for cam in cams:
            f.write(np.array([cam.position, cam.basis_x, cam.basis_y, cam.basis_z], f32).tobytes())
    r = subprocess.run([exe, str(tmp_path / "out.rgba"), str(tmp_path / "sky.bin"), str(tmp_path / "m.b32scene")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "presented_frames 4" in r.stdout, r.stdout
    got = np.frombuffer((tmp_path / "out.rgba").read_bytes(), np.uint8).reshape(len(cams), -1)
    for i, cam in enumerate(cams):
        o = oracle.Framebuffer(W, H)
        o.clear(sc.clear_color)
        assert o.render_skybox_mesh(sky_place(off, cam.position), faces, cam) == 0
        o.draw_star_diamonds(*star_arrays(stars), 3.0)
        assert oracle.render_mesh_15(o, sc.vertices, sc.faces, sc.textures, cam, sc.settings)[0] == 0
        same(got[i], o.pixels, f"frame {i}")
