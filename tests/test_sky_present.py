"""The steps around the mesh draw: clear_gradient, skybox sphere fill, star sprites, nearest upscale.
CPU tests pin the oracle against an independent numpy restatement; GPU tests compare the HIP path with the oracle."""
import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi

f32 = np.float32


def sky_mesh(cam_pos=(0.0, 0.0, 0.0), h_segments=24, v_segments=16, radius=10000.0, seed=3):
    """Same topology as Skybox::generate_mesh (world/geometry.rs:529-585: sphere rows of h_segments+1 vertices, faces
    [i0,i2,i1],[i1,i2,i3]); colours are arbitrary test data (the reference samples its gradient / clouds there with sin/powf)."""
    rng = np.random.default_rng(seed)
    verts = np.zeros((v_segments + 1) * (h_segments + 1), abi.SKY_VERTEX_DTYPE)
    k = 0
    for v in range(v_segments + 1):
        phi = np.pi * v / v_segments
        y, ring = np.cos(phi), np.sin(phi)
        for h in range(h_segments + 1):
            th = 2 * np.pi * h / h_segments
            verts["pos"][k] = (cam_pos[0] + ring * np.cos(th) * radius, cam_pos[1] + y * radius, cam_pos[2] + ring * np.sin(th) * radius)
            k += 1
    col = rng.integers(0, 256, (len(verts), 3), dtype=np.uint8)
    verts["r"], verts["g"], verts["b"] = col[:, 0], col[:, 1], col[:, 2]
    faces = []
    rw = h_segments + 1
    for v in range(v_segments):
        for h in range(h_segments):
            i0, i1, i2, i3 = v * rw + h, v * rw + h + 1, (v + 1) * rw + h, (v + 1) * rw + h + 1
            faces += [[i0, i2, i1], [i1, i2, i3]]
    return verts, np.array(faces, np.uint32)


def np_sky(width, height, verts, faces, cam, img):
    """numpy restatement of render.rs:81-134 + 251-298 (whole bbox at once per face)."""
    pos = verts["pos"].astype(np.float32)
    rel = (pos - np.asarray(cam.position, np.float32)).astype(np.float32)
    def dot(b):
        b = np.asarray(b, np.float32)
        return ((rel[:, 0] * b[0] + rel[:, 1] * b[1]).astype(np.float32) + rel[:, 2] * b[2]).astype(np.float32)
    cx, cy, cz = dot(cam.basis_x), dot(cam.basis_y), dot(cam.basis_z)
    vs = f32(f32(min(width, height)) / f32(2.0)) * f32(0.75)
    denom = cz + f32(5.0)
    with np.errstate(all="ignore"):
        sx = ((cx * f32(4.0)) / denom * vs + f32(width) / f32(2.0)).astype(np.float32)
        sy = ((cy * f32(4.0)) / denom * vs + f32(height) / f32(2.0)).astype(np.float32)
    behind = cz <= f32(0.1)
    col = np.stack([verts["r"], verts["g"], verts["b"]], axis=1).astype(np.float32)
    for f in faces:
        if behind[f].any():
            continue
        p0, p1, p2 = [(sx[i], sy[i]) for i in f]
        area = (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p2[0] - p0[0]) * (p1[1] - p0[1])
        if area >= 0:
            continue
        def usz(x):
            return int(max(0.0, min(float(np.trunc(x)), 1e18))) if x == x else 0
        min_x = usz(max(min(p0[0], p1[0], p2[0]), f32(0.0))); max_x = usz(min(max(p0[0], p1[0], p2[0]), f32(width) - f32(1.0)))
        min_y = usz(max(min(p0[1], p1[1], p2[1]), f32(0.0))); max_y = usz(min(max(p0[1], p1[1], p2[1]), f32(height) - f32(1.0)))
        if min_x > max_x or min_y > max_y:
            continue
        den = (p1[1] - p2[1]) * (p0[0] - p2[0]) + (p2[0] - p1[0]) * (p0[1] - p2[1])
        if abs(den) < f32(0.0001):
            continue
        inv = f32(1.0) / den
        ys, xs = np.mgrid[min_y:max_y + 1, min_x:max_x + 1]
        px = xs.astype(np.float32) + f32(0.5); py = ys.astype(np.float32) + f32(0.5)
        w0 = ((((p1[1] - p2[1]) * (px - p2[0])).astype(np.float32) + ((p2[0] - p1[0]) * (py - p2[1])).astype(np.float32)).astype(np.float32) * inv).astype(np.float32)
        w1 = ((((p2[1] - p0[1]) * (px - p2[0])).astype(np.float32) + ((p0[0] - p2[0]) * (py - p2[1])).astype(np.float32)).astype(np.float32) * inv).astype(np.float32)
        w2 = ((f32(1.0) - w0).astype(np.float32) - w1).astype(np.float32)
        m = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
        c0, c1, c2 = col[f[0]], col[f[1]], col[f[2]]
        for ch in range(3):
            val = (((c0[ch] * w0).astype(np.float32) + (c1[ch] * w1).astype(np.float32)).astype(np.float32) + (c2[ch] * w2).astype(np.float32)).astype(np.float32)
            val = np.clip(np.trunc(np.nan_to_num(val, nan=0.0)), 0, 255).astype(np.uint8)
            img[ys[m], xs[m], ch] = val[m]
        img[ys[m], xs[m], 3] = 255


CAM = b32.Camera(position=(10.0, -20.0, 5.0), basis_x=(0.8, 0.0, -0.6), basis_y=(0.0, 1.0, 0.0), basis_z=(0.6, 0.0, 0.8))


def test_sky_oracle_matches_numpy_restatement(oracle):
    W, H = 160, 120
    verts, faces = sky_mesh(CAM.position)
    fb = oracle.Framebuffer(W, H); fb.clear(b32.Color(1, 2, 3))
    assert fb.render_skybox_mesh(verts, faces, CAM) == 0
    img = np.zeros((H, W, 4), np.uint8); img[:] = (1, 2, 3, 255)
    np_sky(W, H, verts, faces, CAM, img)
    assert np.array_equal(fb.image(), img)
    assert (fb.image()[:, :, :3] != (1, 2, 3)).any(axis=2).mean() > 0.9          # the sphere surrounds the camera


def test_clear_gradient_oracle(oracle):
    fb = oracle.Framebuffer(7, 5)
    fb.clear_gradient(b32.Color(10, 200, 30), b32.Color(250, 0, 31))
    rows = fb.image()[:, 0, :]
    for y in range(5):
        t = f32(y) / f32(4)
        exp = [int(f32(f32(a) * (f32(1) - t)) + f32(f32(b) * t)) for a, b in ((10, 250), (200, 0), (30, 31))]
        assert list(rows[y, :3]) == exp and rows[y, 3] == 255
    assert (fb.image() == fb.image()[:, :1]).all()
    one = oracle.Framebuffer(3, 1); one.clear_gradient(b32.Color(9, 8, 7, abi.ERASE), b32.Color(1, 1, 1))
    assert list(one.image()[0, 0]) == [9, 8, 7, 0]                                    # h == 1: t = 0; Erase top -> alpha 0


def test_star_diamond_oracle(oracle):
    fb = oracle.Framebuffer(9, 9)
    fb.draw_star_diamonds([4], [4], [[200, 100, 50]], 3.0)
    im = fb.image()
    assert list(im[4, 4]) == [200, 100, 50, 255]
    assert list(im[4, 3]) == [int(f32(200) * f32(0.7)), int(f32(100) * f32(0.7)), int(f32(50) * f32(0.7)), 255]
    assert list(im[2, 4]) == [int(f32(200) * f32(0.4)), int(f32(100) * f32(0.4)), int(f32(50) * f32(0.4)), 255]
    assert im[:, :, 3].sum() == 9 * 255
    fb2 = oracle.Framebuffer(9, 9); fb2.draw_star_diamonds([0], [8], [[9, 9, 9]], 0.2)   # size.max(1.0) -> centre only, clipped
    assert fb2.image()[:, :, 3].sum() == 255


@pytest.mark.gpu
def test_gpu_sky_gradient_stars_present(gpu_ctx, oracle):
    from bonnie32_amd import rasterizer as R
    W, H = 640, 480
    verts, faces = sky_mesh(CAM.position, 48, 32)
    rng = np.random.default_rng(11)
    n = 400
    cx = rng.integers(-3, W + 3, n); cy = rng.integers(-3, H + 3, n); rgb = rng.integers(0, 256, (n, 3))
    cx[:50] = cx[50:100]; cy[:50] = cy[50:100] + 1                                       # overlapping sprites: order matters
    ofb = oracle.Framebuffer(W, H)
    ofb.clear_gradient(b32.Color(20, 40, 200), b32.Color(220, 180, 90))
    fb = R.Framebuffer(W, H, gpu_ctx)
    for band in ((0, 100), (100, 333), (333, H)):                                        # every step is band-aware
        fb.set_band(*band)
        fb.clear_gradient(b32.Color(20, 40, 200), b32.Color(220, 180, 90))
    fb.set_band(0, H)
    assert np.array_equal(fb.pixels, ofb.pixels)
    looking_down = b32.Camera(position=CAM.position, basis_x=(1.0, 0.0, 0.0), basis_y=(0.0, 0.0, 1.0), basis_z=(0.0, -1.0, 0.0))
    for cam in (CAM, looking_down):
        assert ofb.render_skybox_mesh(verts, faces, cam) == 0
        for band in ((0, 100), (100, 333), (333, H)):
            fb.set_band(*band)
            fb.render_skybox_mesh(verts, faces, cam)
        fb.set_band(0, H)
        got = fb.pixels
        assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ"
    ofb.draw_star_diamonds(cx, cy, rgb, 3.0)
    fb.draw_star_diamonds(cx, cy, rgb, 3.0)
    assert np.array_equal(fb.pixels, ofb.pixels)
    # a mesh drawn on top keeps working on the same framebuffer
    from bonnie32_amd import scenegen
    sc = scenegen.make_scene("C1", width=W, height=H, n_tris=3000, bbox_px=600.0)
    oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    R.render_mesh_15(fb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    assert np.array_equal(fb.pixels, ofb.pixels)
    # presenter: nearest upscale, GL_NEAREST sampling rule
    for dw, dh in ((2560, 1920), (1000, 777), (320, 240)):
        out = fb.present_nearest(dw, dh)
        sx = ((2 * np.arange(dw) + 1) * W) // (2 * dw); sy = ((2 * np.arange(dh) + 1) * H) // (2 * dh)
        assert np.array_equal(out, ofb.image()[sy][:, sx])
    with pytest.raises(R.B32Error):
        fb.render_skybox_mesh(verts, np.array([[0, 1, len(verts)]], np.uint32), CAM)      # index panic


# ---------------------------------------------------------------------------------------------------------------------------------
# The edges of the five kernels of b32_sky.hip.  Every device comparison below is bit-exact over the whole framebuffer.

SOUP_CAM = b32.Camera()                                                                    # origin, identity basis
LOOKING_DOWN = b32.Camera(position=CAM.position, basis_x=(1.0, 0.0, 0.0), basis_y=(0.0, 0.0, 1.0), basis_z=(0.0, -1.0, 0.0))
TOP, BOTTOM = b32.Color(20, 40, 200), b32.Color(220, 180, 90)
SKY_LIST_CAP = 4096                                                                        # b32_sky.hip: faces one tile lists per round


def sky_screen_points(W, H, verts, cam):
    """The f32 screen points of k_sky_project (math.rs:103-136), NaN where the vertex is behind the camera (render.rs:99-103)."""
    rel = (verts["pos"].astype(np.float32) - np.asarray(cam.position, np.float32)).astype(np.float32)
    with np.errstate(all="ignore"):
        def dot(b):
            b = np.asarray(b, np.float32)
            return ((rel[:, 0] * b[0] + rel[:, 1] * b[1]).astype(np.float32) + rel[:, 2] * b[2]).astype(np.float32)
        cx, cy, cz = dot(cam.basis_x), dot(cam.basis_y), dot(cam.basis_z)
        vs = f32(f32(min(W, H)) / f32(2.0)) * f32(0.75)
        denom = cz + f32(5.0)
        sx = ((cx * f32(4.0)) / denom * vs + f32(W) / f32(2.0)).astype(np.float32)
        sy = ((cy * f32(4.0)) / denom * vs + f32(H) / f32(2.0)).astype(np.float32)
        flat = np.abs(denom) < f32(0.001)
        sx = np.where(flat, f32(W) / f32(2.0), sx); sy = np.where(flat, f32(H) / f32(2.0), sy)
        behind = cz <= f32(0.1)
    return np.where(behind, f32(np.nan), sx).astype(np.float32), np.where(behind, f32(np.nan), sy).astype(np.float32)


def sky_face_facts(W, H, verts, faces, cam):
    """Per face, from the f32 screen points: `alive` (it survives the NaN and winding tests, render.rs:112-121, and its clamped,
    inclusive bounding box, render.rs:262-265, is non-empty), its signed `area`, the clamped box and whether the box was `infinite`
    before the clamp."""
    sx, sy = sky_screen_points(W, H, verts, cam)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    x0, x1, x2, y0, y1, y2 = sx[f[:, 0]], sx[f[:, 1]], sx[f[:, 2]], sy[f[:, 0]], sy[f[:, 1]], sy[f[:, 2]]
    with np.errstate(all="ignore"):
        alive = ~(np.isnan(x0) | np.isnan(x1) | np.isnan(x2))
        area = ((x1 - x0) * (y2 - y0)).astype(np.float32) - ((x2 - x0) * (y1 - y0)).astype(np.float32)
        alive &= ~(area >= 0)                                                              # (a NaN area is not culled)

        def usz(x):                                                                        # Rust `as usize`: NaN -> 0, saturating
            return np.trunc(np.clip(np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=1e18, neginf=0.0), 0.0, 1e18)).astype(np.int64)
        lo = lambda a, b, c: np.fmin(np.fmin(a, b), c)                                     # f32::min / max return the non-NaN operand
        hi = lambda a, b, c: np.fmax(np.fmax(a, b), c)
        min_x, max_x = usz(np.fmax(lo(x0, x1, x2), f32(0.0))), usz(np.fmin(hi(x0, x1, x2), f32(W) - f32(1.0)))
        min_y, max_y = usz(np.fmax(lo(y0, y1, y2), f32(0.0))), usz(np.fmin(hi(y0, y1, y2), f32(H) - f32(1.0)))
        infinite = np.isinf(lo(x0, x1, x2)) | np.isinf(hi(x0, x1, x2)) | np.isinf(lo(y0, y1, y2)) | np.isinf(hi(y0, y1, y2))
    alive &= (min_x <= max_x) & (min_y <= max_y)
    return dict(alive=alive, area=area, min_x=min_x, max_x=max_x, min_y=min_y, max_y=max_y, infinite=infinite)


def sky_tile_counts(W, H, verts, faces, cam):
    """How many faces each 64x64 tile of k_sky_fill lists (whole-framebuffer band), by the kernel's own rule: the face is alive and
    its box reaches the tile.  -> int array [tiles_y, tiles_x]."""
    ff = sky_face_facts(W, H, verts, faces, cam)
    alive, min_x, max_x, min_y, max_y = ff["alive"], ff["min_x"], ff["max_x"], ff["min_y"], ff["max_y"]
    counts = np.zeros(((H + 63) // 64, (W + 63) // 64), np.int64)
    for ty in range(counts.shape[0]):
        for tx in range(counts.shape[1]):
            x_lo, x_hi, y_lo, y_hi = tx * 64, min(tx * 64 + 64, W), ty * 64, min(ty * 64 + 64, H)
            counts[ty, tx] = int((alive & (max_x >= x_lo) & (min_x < x_hi) & (max_y >= y_lo) & (min_y < y_hi)).sum())
    return counts


def sky_soup(W, H, nf, seed, span=24.0, margin=8.0):
    """An ordered triangle soup built in screen space for SOUP_CAM: every vertex at z = 95 (denom = 100), x = (sx - W/2) / vs * 25;
    three random screen points per face in a span-pixel box whose centre is uniform over the framebuffer plus a margin; two vertices
    swapped where the projected face is not front-facing (render.rs:118-121).  -> (verts, faces, faces listed per tile)."""
    rng = np.random.default_rng(seed)
    centre = np.stack([rng.uniform(-margin, W + margin, nf), rng.uniform(-margin, H + margin, nf)], axis=1)
    pts = centre[:, None, :] + rng.uniform(-span / 2, span / 2, (nf, 3, 2))
    vs = min(W, H) / 2 * 0.75
    verts = np.zeros(3 * nf, abi.SKY_VERTEX_DTYPE)
    verts["pos"][:, 0] = ((pts[:, :, 0] - W / 2) / vs * 25).reshape(-1)
    verts["pos"][:, 1] = ((pts[:, :, 1] - H / 2) / vs * 25).reshape(-1)
    verts["pos"][:, 2] = 95.0
    col = rng.integers(0, 256, (3 * nf, 3), dtype=np.uint8)
    verts["r"], verts["g"], verts["b"] = col[:, 0], col[:, 1], col[:, 2]
    sx, sy = sky_screen_points(W, H, verts, SOUP_CAM)
    sx, sy = sx.reshape(nf, 3), sy.reshape(nf, 3)
    area = ((sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0])).astype(np.float32) - ((sx[:, 2] - sx[:, 0]) * (sy[:, 1] - sy[:, 0])).astype(np.float32)
    faces = np.arange(3 * nf, dtype=np.uint32).reshape(nf, 3)
    flip = area >= 0
    faces[flip] = faces[flip][:, [0, 2, 1]]
    return verts, faces, sky_tile_counts(W, H, verts, faces, SOUP_CAM)


def hostile_soup():
    """The 130x70 soup of 3 000 faces with 600 vertices replaced by values that project to +-inf, sit on the near limit, are NaN or
    infinite, and 100 faces [i, i, j] (area 0: culled)."""
    W, H = 130, 70
    verts, faces, _ = sky_soup(W, H, 3000, 7, span=5.0)                                   # small faces: part of the background stays
    rng = np.random.default_rng(70)
    pick = rng.choice(len(verts), 600, replace=False).reshape(6, 100)
    near = np.float32(0.1)
    verts["pos"][pick[0], 0] = 3e38                                                        # projects to +inf
    verts["pos"][pick[1], 1] = -3e38                                                       # ... -inf
    verts["pos"][pick[2], 2] = near                                                        # cz == 0.1: behind (render.rs:99)
    verts["pos"][pick[3], 2] = np.nextafter(near, np.float32(1.0))                         # one ulp in front of it
    verts["pos"][pick[4], 2] = 3e38
    verts["pos"][pick[5][:50], 0] = np.nan
    verts["pos"][pick[5][50:], 1] = np.inf
    faces = faces.copy()
    rep = rng.choice(len(faces), 100, replace=False)
    faces[rep, 1] = faces[rep, 0]
    HOSTILE_PICKS.update(on_limit=pick[2], past_limit=pick[3], repeated=rep)
    return W, H, verts, faces


HOSTILE_PICKS = {}                                                                         # which vertices / faces of hostile_soup got what
_INPUTS = {}


def sky_input(name):
    """The sky inputs the CPU and the GPU tests share: name -> (W, H, verts, faces, camera).  Built once."""
    if name not in _INPUTS:
        if name.startswith("soup"):                                                        # soup:WxH:nf:seed
            wh, nf, seed = name.split(":")[1:]
            W, H = map(int, wh.split("x"))
            verts, faces, _ = sky_soup(W, H, int(nf), int(seed))
            _INPUTS[name] = (W, H, verts, faces, SOUP_CAM)
        elif name == "hostile":
            _INPUTS[name] = hostile_soup() + (SOUP_CAM,)
        else:                                                                              # sphere:HSEGxVSEG:WxH:camera
            seg, wh, cam = name.split(":")[1:4]
            hs, vsg = map(int, seg.split("x")); W, H = map(int, wh.split("x"))
            if seg not in _INPUTS:
                _INPUTS[seg] = sky_mesh(CAM.position, hs, vsg)
            _INPUTS[name] = (W, H) + _INPUTS[seg] + ({"cam": CAM, "down": LOOKING_DOWN}[cam],)
    return _INPUTS[name]


_ORACLE_SKY = {}


def oracle_sky(oracle, name):
    """clear_gradient(TOP, BOTTOM) + the sky of sky_input(name) on the oracle, computed once -> read-only image [H, W, 4]."""
    if name not in _ORACLE_SKY:
        W, H, verts, faces, cam = sky_input(name)
        ofb = oracle.Framebuffer(W, H)
        ofb.clear_gradient(TOP, BOTTOM)
        assert ofb.render_skybox_mesh(verts, faces, cam) == 0
        img = ofb.image().copy(); img.setflags(write=False)
        _ORACLE_SKY[name] = img
    return _ORACLE_SKY[name]


def gradient_rows(oracle, W, H, top=TOP, bottom=BOTTOM):
    ofb = oracle.Framebuffer(W, H)
    ofb.clear_gradient(top, bottom)
    return ofb.image().copy()


def same(got, want, what=""):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape and np.array_equal(got, want), f"{what}: {int((got != want).sum())} bytes differ"


# three rounds of the list on one tile / the break inside the first partial chunk / 3x2 ragged tiles, one of them over the cap
SOUP_3ROUNDS, SOUP_PARTIAL, SOUP_RAGGED = "soup:64x64:9000:5", "soup:64x64:4550:5", "soup:130x70:9000:6"
SPHERE_SIZES = [(1, 1), (63, 65), (65, 63), (129, 1), (1, 129), (200, 150)]
TINY_TARGETS = [f"{w}x{h}:{c}" for w, h in ((64, 64), (1, 1)) for c in ("cam", "down")]
SKY_INPUTS = ([SOUP_3ROUNDS, SOUP_PARTIAL, SOUP_RAGGED, "hostile"]
              + ["sphere:128x64:" + t + ":smaller-nf-than-the-gpu-case(256x128)" for t in TINY_TARGETS]
              + [f"sphere:48x32:{w}x{h}:cam" for w, h in SPHERE_SIZES])


@pytest.mark.parametrize("name", SKY_INPUTS)
def test_sky_oracle_matches_numpy_on_edge_inputs(oracle, name):
    """Two independent references agree on every sky input the GPU tests use, so the device cannot "confirm" a reference bug.  The
    256x128 sphere (65 536 faces) is too slow for the numpy restatement: the 128x64 sphere of the same generator stands in for it."""
    name = name.split(":smaller-nf")[0]
    W, H, verts, faces, cam = sky_input(name)
    img = gradient_rows(oracle, W, H)
    with np.errstate(all="ignore"):
        np_sky(W, H, verts, faces, cam, img)
    same(oracle_sky(oracle, name), img, name)


def test_sky_soup_list_counts():
    """The inputs really reach the code they are meant for: every count comes from the inputs alone."""
    def counts(name):
        W, H, verts, faces, cam = sky_input(name)
        return sky_tile_counts(W, H, verts, faces, cam)
    assert counts(SOUP_3ROUNDS).shape == (1, 1) and counts(SOUP_3ROUNDS)[0, 0] > 2 * SKY_LIST_CAP          # at least three rounds
    assert SKY_LIST_CAP + 1 <= counts(SOUP_PARTIAL)[0, 0] <= SKY_LIST_CAP + 255                             # the break inside the first partial chunk
    ragged = counts(SOUP_RAGGED)
    assert ragged.shape == (2, 3) and ragged.max() > SKY_LIST_CAP and ragged.min() < SKY_LIST_CAP


def test_hostile_soup_reaches_the_paths_it_is_named_for():
    """Faces with a NaN area and faces whose bounding box is infinite before the clamp survive to be listed; a vertex exactly on
    the near limit removes its faces, one ulp past it does not; faces with a repeated index are culled unless their area is NaN."""
    W, H, verts, faces, cam = sky_input("hostile")
    ff = sky_face_facts(W, H, verts, faces, cam)
    alive = ff["alive"]
    assert (alive & np.isnan(ff["area"])).sum() >= 10
    assert (alive & ff["infinite"]).sum() >= 10
    uses = lambda vs: np.isin(faces, vs).any(axis=1)
    assert uses(HOSTILE_PICKS["on_limit"]).sum() >= 50 and not alive[uses(HOSTILE_PICKS["on_limit"])].any()
    assert alive[uses(HOSTILE_PICKS["past_limit"])].sum() >= 10
    rep = HOSTILE_PICKS["repeated"]
    assert not (alive[rep] & ~np.isnan(ff["area"][rep])).any()                                              # area 0 is culled, a NaN area is not
    assert sky_tile_counts(W, H, verts, faces, cam).min() > 0                                               # every tile lists some


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: k_sky_project + k_sky_fill

def gpu_sky(ctx, name, bands=None):
    """clear_gradient + the sky of sky_input(name) on the device, whole or band by band -> pixels."""
    from bonnie32_amd import rasterizer as R
    W, H, verts, faces, cam = sky_input(name)
    fb = R.Framebuffer(W, H, ctx)
    fb.clear_gradient(TOP, BOTTOM)
    for band in bands or [(0, H)]:
        fb.set_band(*band)
        fb.render_skybox_mesh(verts, faces, cam)
    fb.set_band(0, H)
    return fb.pixels


def reversed_order_changes(oracle, name):
    """The share of pixels that change when the faces are drawn in reversed order (on the oracle)."""
    W, H, verts, faces, cam = sky_input(name)
    ofb = oracle.Framebuffer(W, H)
    ofb.clear_gradient(TOP, BOTTOM)
    assert ofb.render_skybox_mesh(verts, faces[::-1], cam) == 0
    return float((ofb.image() != oracle_sky(oracle, name)).any(axis=2).mean())


@pytest.mark.gpu
@pytest.mark.parametrize("name", [SOUP_3ROUNDS, SOUP_PARTIAL])
def test_gpu_sky_list_overflow_one_tile(gpu_ctx, oracle, name):
    """One tile lists more faces than SKY_LIST_CAP: the walk runs in rounds, and the last face in order wins across them."""
    W, H, verts, faces, cam = sky_input(name)
    listed = int(sky_tile_counts(W, H, verts, faces, cam)[0, 0])
    if name == SOUP_3ROUNDS:
        assert listed > 2 * SKY_LIST_CAP
    else:
        assert SKY_LIST_CAP + 1 <= listed <= SKY_LIST_CAP + 255
    assert reversed_order_changes(oracle, name) > 0.5
    same(gpu_sky(gpu_ctx, name), oracle_sky(oracle, name), name)


@pytest.mark.gpu
def test_gpu_sky_list_overflow_ragged_tiles(gpu_ctx, oracle):
    """130x70 = 3x2 tiles, the right column 2 pixels wide, the bottom row 6 rows high; a band edge on the tile boundary, a one-row
    band and the rest; one tile over the cap and others under it."""
    W, H, verts, faces, cam = sky_input(SOUP_RAGGED)
    counts = sky_tile_counts(W, H, verts, faces, cam)
    assert counts.shape == (2, 3) and counts.max() > SKY_LIST_CAP and counts.min() < SKY_LIST_CAP
    assert reversed_order_changes(oracle, SOUP_RAGGED) > 0.5
    same(gpu_sky(gpu_ctx, SOUP_RAGGED), oracle_sky(oracle, SOUP_RAGGED), "whole")
    same(gpu_sky(gpu_ctx, SOUP_RAGGED, [(0, 64), (64, 65), (65, 70)]), oracle_sky(oracle, SOUP_RAGGED), "bands")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere:256x128:" + t for t in TINY_TARGETS])
def test_gpu_sky_real_mesh_on_a_tiny_target(gpu_ctx, oracle, name):
    """65 536 faces, most of them sub-pixel or with |denom| < 0.0001, on 64x64 and on 1x1."""
    same(gpu_sky(gpu_ctx, name), oracle_sky(oracle, name), name)


THREE_BANDS = {1: [(0, 0), (0, 1), (1, 1)], 63: [(0, 30), (30, 31), (31, 63)], 65: [(0, 30), (30, 64), (64, 65)],
               129: [(0, 64), (64, 100), (100, 129)], 150: [(0, 64), (64, 100), (100, 150)]}


@pytest.mark.gpu
@pytest.mark.parametrize("size", SPHERE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_sky_sizes(gpu_ctx, oracle, size):
    """Framebuffers narrower and lower than a tile, one pixel past a tile, one pixel in all: whole and in three bands."""
    name = f"sphere:48x32:{size[0]}x{size[1]}:cam"
    same(gpu_sky(gpu_ctx, name), oracle_sky(oracle, name), "whole")
    same(gpu_sky(gpu_ctx, name, THREE_BANDS[size[1]]), oracle_sky(oracle, name), "bands")


@pytest.mark.gpu
def test_gpu_sky_hostile_vertices(gpu_ctx, oracle):
    """Positions that project to +-inf (NaN area, NaN denom, saturating bounding boxes), cz exactly on the near limit and one ulp
    past it, NaN and infinite positions, faces with a repeated index.  The background survives where the oracle leaves it."""
    want = oracle_sky(oracle, "hostile")
    W, H = want.shape[1], want.shape[0]
    untouched = float((want == gradient_rows(oracle, W, H)).all(axis=2).mean())
    assert 0.0 < untouched < 1.0                                                            # both kinds of pixel exist
    same(gpu_sky(gpu_ctx, "hostile"), want, "whole")
    same(gpu_sky(gpu_ctx, "hostile", [(0, 64), (64, 65), (65, 70)]), want, "bands")


@pytest.mark.gpu
def test_gpu_sky_noops_and_index_error(gpu_ctx, oracle):
    from bonnie32_amd import rasterizer as R
    W, H = 65, 63
    verts, faces = sky_mesh(CAM.position)
    want = gradient_rows(oracle, W, H)
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear_gradient(TOP, BOTTOM)
    fb.render_skybox_mesh(verts[:0], faces, CAM)                                            # nv == 0
    same(fb.pixels, want, "nv == 0")
    fb.render_skybox_mesh(verts, faces[:0], CAM)                                            # nf == 0
    same(fb.pixels, want, "nf == 0")
    bad = faces.copy(); bad[len(bad) // 2, 1] = len(verts)                                  # the check runs before any launch
    with pytest.raises(R.B32Error):
        fb.render_skybox_mesh(verts, bad, CAM)
    same(fb.pixels, want, "index error")
    ofb = oracle.Framebuffer(W, H); ofb.clear_gradient(TOP, BOTTOM)
    assert ofb.render_skybox_mesh(verts, bad, CAM) == abi.B32_E_INDEX                       # (the oracle draws the faces before the bad one)
    assert (ofb.image() != want).any()


@pytest.mark.gpu
def test_gpu_deferred_clear_before_sky_stars_gradient(gpu_ctx, oracle):
    """b32_fb_clear defers itself; a sky pass, the star sprites and a clear_gradient that come first must see the cleared frame
    (flush_clear in front of launch_sky, launch_stars and launch_clear_gradient)."""
    from bonnie32_amd import rasterizer as R
    W, H = 130, 70
    red = b32.Color(200, 10, 10)
    red_px = np.array([200, 10, 10, 255], np.uint8)
    verts, faces = sky_mesh((0.0, 0.0, 200.0), radius=50.0)                                 # a ball in front of the camera: most pixels stay cleared
    ofb = oracle.Framebuffer(W, H); ofb.clear(red)
    assert ofb.render_skybox_mesh(verts, faces, SOUP_CAM) == 0
    cleared = float((ofb.image() == red_px).all(axis=2).mean())
    assert 0.2 < cleared < 0.95
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(red)
    fb.render_skybox_mesh(verts, faces, SOUP_CAM)
    same(fb.pixels, ofb.pixels, "clear + sky")
    rng = np.random.default_rng(4)
    cx, cy, rgb = rng.integers(-3, W + 3, 40), rng.integers(-3, H + 3, 40), rng.integers(0, 256, (40, 3))
    ofb.clear(red); ofb.draw_star_diamonds(cx, cy, rgb, 3.0)
    fb.clear(red); fb.draw_star_diamonds(cx, cy, rgb, 3.0)
    same(fb.pixels, ofb.pixels, "clear + stars")
    fb.clear(red); fb.clear_gradient(TOP, BOTTOM)                                           # the gradient is the later write
    same(fb.pixels, gradient_rows(oracle, W, H), "clear + gradient")
    fb.clear(red); fb.set_band(20, 41); fb.clear_gradient(TOP, BOTTOM); fb.set_band(0, H)
    want = gradient_rows(oracle, W, H); want[:20] = red_px; want[41:] = red_px
    same(fb.pixels, want, "clear + gradient of a sub-band")


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: k_clear_gradient

@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 2047, 2048, 2049, 4100])
def test_gpu_clear_gradient_widths(gpu_ctx, oracle, W):
    """The launch caps the grid at 8 blocks of 256 in x: the stride loop makes a second trip above 2048 and a third at 4100."""
    from bonnie32_amd import rasterizer as R
    for H in (1, 2, 3):
        fb = R.Framebuffer(W, H, gpu_ctx)
        for top, bottom in ((TOP, BOTTOM), (b32.Color(9, 8, 7, abi.ERASE), BOTTOM), (TOP, b32.Color(1, 2, 3, abi.ERASE))):
            fb.clear_gradient(top, bottom)
            same(fb.pixels, gradient_rows(oracle, W, H, top, bottom), f"{W}x{H} blends {top.blend}/{bottom.blend}")


@pytest.mark.gpu
@pytest.mark.parametrize("H", [241, 97])
def test_gpu_clear_gradient_lerp_rounding(gpu_ctx, oracle, H):
    """Color::lerp (types.rs:812-821) row by row: 32 random colour pairs and the extreme ones, every row compared."""
    from bonnie32_amd import rasterizer as R
    rng = np.random.default_rng(H)
    pairs = [(tuple(int(c) for c in rng.integers(0, 256, 3)), tuple(int(c) for c in rng.integers(0, 256, 3))) for _ in range(32)]
    pairs += [((a,) * 3, (b,) * 3) for a, b in ((0, 255), (255, 0), (255, 255), (1, 254))]
    fb = R.Framebuffer(3, H, gpu_ctx)
    for a, b in pairs:
        fb.clear_gradient(b32.Color(*a), b32.Color(*b))
        same(fb.pixels, gradient_rows(oracle, 3, H, b32.Color(*a), b32.Color(*b)), f"{a} -> {b}")


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(5, 7), (2049, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_clear_gradient_bands(gpu_ctx, oracle, size):
    """Every band is painted with its own colour pair; the empty band touches nothing."""
    from bonnie32_amd import rasterizer as R
    W, H = size
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear_gradient(b32.Color(3, 3, 3), b32.Color(250, 250, 250))
    want = gradient_rows(oracle, W, H, b32.Color(3, 3, 3), b32.Color(250, 250, 250))
    fb.set_band(1, 1); fb.clear_gradient(b32.Color(255, 0, 0), b32.Color(0, 255, 0)); fb.set_band(0, H)
    same(fb.pixels, want, "empty band")
    rng = np.random.default_rng(W)
    for y0, y1 in ((0, 1), (1, 1), (1, H - 1), (H - 1, H)):
        top, bottom = b32.Color(*(int(c) for c in rng.integers(0, 256, 3))), b32.Color(*(int(c) for c in rng.integers(0, 256, 3)))
        fb.set_band(y0, y1); fb.clear_gradient(top, bottom)
        want[y0:y1] = gradient_rows(oracle, W, H, top, bottom)[y0:y1]
    fb.set_band(0, H)
    same(fb.pixels, want, "composite")


@pytest.mark.gpu
def test_gpu_clear_gradient_resets_the_zbuffer_of_its_band(gpu_ctx, oracle):
    """clear_gradient resets the depths of the rows it paints (render.rs:58-77) and of no other row: a far mesh drawn afterwards
    appears in the cleared rows and stays hidden behind the near mesh below them."""
    from bonnie32_amd import rasterizer as R, scenegen
    near = scenegen.make_scene("C1", n_tris=2000, bbox_px=6000.0, seed=71)
    far = scenegen.make_scene("C1", n_tris=2000, bbox_px=6000.0, seed=72)
    near.vertices["pos"] *= f32(0.05)                                                       # depths 20 .. 300
    far.vertices["pos"] *= f32(2.0)                                                         # depths 800 .. 12 000: every far fragment is behind
    zs = b32.RasterSettings.game()
    W, H, cut = near.width, near.height, 100
    ofb = oracle.Framebuffer(W, H); ofb.clear(b32.Color(1, 2, 3))
    oracle.render_mesh_15(ofb, near.vertices, near.faces, near.textures, near.camera, zs)
    full = oracle.Framebuffer(W, H); full.clear_gradient(TOP, BOTTOM)
    ofb.image()[:cut] = full.image()[:cut]
    ofb.zbuffer.reshape(H, W)[:cut] = full.zbuffer.reshape(H, W)[:cut]
    before = ofb.image().copy()
    oracle.render_mesh_15(ofb, far.vertices, far.faces, far.textures, far.camera, zs)
    assert (ofb.image()[:cut] != before[:cut]).any(axis=2).mean() > 0.5                     # the far mesh appears in the cleared rows
    assert np.array_equal(ofb.image()[cut:], before[cut:])                                  # ... and stays hidden below them
    hidden = oracle.Framebuffer(W, H); hidden.clear(b32.Color(1, 2, 3))
    oracle.render_mesh_15(hidden, far.vertices, far.faces, far.textures, far.camera, zs)
    assert (hidden.image()[cut:, :, :3] != (1, 2, 3)).any(axis=2).mean() > 0.5              # (it would cover those rows if nothing hid it)
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(b32.Color(1, 2, 3))
    R.render_mesh_15(fb, near.vertices, near.faces, near.textures, near.camera, zs)
    fb.set_band(0, cut); fb.clear_gradient(TOP, BOTTOM); fb.set_band(0, H)
    R.render_mesh_15(fb, far.vertices, far.faces, far.textures, far.camera, zs)
    same(fb.pixels, ofb.pixels, "pixels")
    same(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32), "z-buffer")


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: k_stars

def star_field(W, H, n=60, seed=21):
    rng = np.random.default_rng(seed)
    cx, cy, rgb = rng.integers(-3, W + 4, n), rng.integers(-3, H + 4, n), rng.integers(0, 256, (n, 3))
    cx[:10] = cx[10:20]; cy[:10] = cy[10:20]                                               # same centres: order matters at every size
    cx[20:30] = cx[30:40]; cy[20:30] = cy[30:40] + 1
    return cx, cy, rgb


def oracle_stars(oracle, W, H, cx, cy, rgb, size):
    ofb = oracle.Framebuffer(W, H)
    ofb.clear_gradient(TOP, BOTTOM)
    ofb.draw_star_diamonds(cx, cy, rgb, size)
    return ofb.image().copy()


STAR_SIZES = [float("nan"), -5.0, 0.2, 1.0, 1.999, 2.0, 2.999, 3.0, 1e10, float("inf")]


@pytest.mark.gpu
@pytest.mark.parametrize("size", STAR_SIZES, ids=repr)
def test_gpu_star_sizes(gpu_ctx, oracle, size):
    """size.max(1.0) as i32 (render.rs:199-240): the near ring from 2, the far ring from 3; NaN, negative and huge sizes."""
    from bonnie32_amd import rasterizer as R
    W, H = 33, 17
    cx, cy, rgb = star_field(W, H)
    want = oracle_stars(oracle, W, H, cx, cy, rgb, size)
    assert (want != oracle_stars(oracle, W, H, cx[::-1], cy[::-1], rgb[::-1], size)).any()  # the order of the stars matters
    rings = 9 if size >= 3 else (5 if size >= 2 else 1)
    one = oracle_stars(oracle, W, H, [16], [8], [[200, 100, 50]], size)
    assert int((one != gradient_rows(oracle, W, H)).any(axis=2).sum()) == rings            # the case is on the side of the threshold it names
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear_gradient(TOP, BOTTOM)
    fb.draw_star_diamonds(cx, cy, rgb, size)
    same(fb.pixels, want, f"size {size}")


@pytest.mark.gpu
def test_gpu_star_wrapping_centres(gpu_ctx, oracle):
    """`cx + 2` on i32 wraps in a release build (render.rs:219-236): every combination of extreme and edge centres, each drawn
    alone, writes exactly what the oracle writes."""
    from bonnie32_amd import rasterizer as R
    W, H = 33, 17
    i_max, i_min = 2**31 - 1, -2**31
    xs = [i_max, i_max - 1, i_min, i_min + 1, -2, -1, 0, W - 1, W, W + 1]
    ys = [i_max, i_max - 1, i_min, i_min + 1, -2, -1, 0, H - 1, H, H + 1]
    fb = R.Framebuffer(W, H, gpu_ctx)
    background = gradient_rows(oracle, W, H)
    written = 0
    for cx in xs:
        for cy in ys:
            want = oracle_stars(oracle, W, H, [cx], [cy], [[250, 130, 60]], 3.0)
            written += int((want != background).any(axis=2).sum())
            fb.clear_gradient(TOP, BOTTOM)
            fb.draw_star_diamonds([cx], [cy], [[250, 130, 60]], 3.0)
            same(fb.pixels, want, f"centre ({cx}, {cy})")
    assert written >= 4 * 5                                                                 # each corner centre alone writes centre, two near and two far pixels


@pytest.mark.gpu
def test_gpu_star_bands(gpu_ctx, oracle):
    from bonnie32_amd import rasterizer as R
    W, H = 33, 17
    cx, cy, rgb = star_field(W, H)
    want = oracle_stars(oracle, W, H, cx, cy, rgb, 3.0)
    background = gradient_rows(oracle, W, H)
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear_gradient(TOP, BOTTOM)
    for band in ((0, 5), (5, 6), (6, 17)):
        fb.set_band(*band)
        fb.draw_star_diamonds(cx, cy, rgb, 3.0)
    fb.set_band(0, H)
    same(fb.pixels, want, "composite of the bands")
    fb.clear_gradient(TOP, BOTTOM)
    fb.set_band(5, 6); fb.draw_star_diamonds(cx, cy, rgb, 3.0); fb.set_band(0, H)
    alone = background.copy(); alone[5:6] = want[5:6]
    assert (want[4] != background[4]).any() and (want[5] != background[5]).any() and (want[6] != background[6]).any()
    same(fb.pixels, alone, "band (5, 6) alone")


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: b32_present_nearest

def nearest(img, dw, dh):
    """FilterMode::Nearest (game/renderer.rs:179-214): destination pixel centre -> source texel, in integers."""
    H, W = img.shape[:2]
    sx = ((2 * np.arange(dw) + 1) * W) // (2 * dw); sy = ((2 * np.arange(dh) + 1) * H) // (2 * dh)
    return img[sy][:, sx]


@pytest.mark.gpu
def test_gpu_present_sizes_and_errors(gpu_ctx, oracle):
    from bonnie32_amd import rasterizer as R
    W, H = 7, 5
    rng = np.random.default_rng(8)
    cx, cy, rgb = rng.integers(0, W, 30), rng.integers(0, H, 30), rng.integers(0, 256, (30, 3))
    src = oracle_stars(oracle, W, H, cx, cy, rgb, 3.0)
    assert len(np.unique(src.reshape(-1, 4), axis=0)) > 20                                  # (nearly) every pixel has a colour of its own
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear_gradient(TOP, BOTTOM)
    fb.draw_star_diamonds(cx, cy, rgb, 3.0)
    for dw, dh in ((1, 1), (7, 5), (21, 15), (13, 11), (32768, 1), (1, 32768)):
        same(fb.present_nearest(dw, dh), nearest(src, dw, dh), f"7x5 -> {dw}x{dh}")
    out = np.zeros(4 * 32769, np.uint8)
    for dw, dh in ((0, 1), (1, 0), (32769, 1), (1, 32769)):
        assert gpu_ctx.lib.b32_present_nearest(gpu_ctx.h, dw, dh, out.ctypes.data) == abi.B32_E_ARG
    assert not out.any()
    name = "sphere:48x32:640x480:cam"
    fb = R.Framebuffer(640, 480, gpu_ctx)
    fb.clear_gradient(TOP, BOTTOM)
    fb.render_skybox_mesh(*sky_input(name)[2:])
    same(fb.present_nearest(3, 2), nearest(oracle_sky(oracle, name), 3, 2), "640x480 -> 3x2")


@pytest.mark.gpu
def test_gpu_present_sees_a_deferred_clear_and_a_pending_frame(oracle):
    """present_nearest directly after a deferred clear (flush_clear) and directly after an enqueued frame (settle_pending)."""
    from bonnie32_amd import rasterizer as R, scenegen
    sc = scenegen.make_scene("C1", n_tris=1500, seed=81, variant="gouraud", bbox_px=400.0)
    W, H = sc.width, sc.height
    red, st = b32.Color(200, 10, 10), b32.RasterSettings.game()
    ofb = oracle.Framebuffer(W, H); ofb.clear(red)
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        fb.clear(red)
        same(fb.present_nearest(200, 100), nearest(ofb.image(), 200, 100), "clear, present")
        slot = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
        table = ctx.make_frame_table(sc.camera, st, [slot])
        assert oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, st)[0] == 0
        assert (ofb.image()[:, :, :3] != (200, 10, 10)).any(axis=2).mean() > 0.2
        fb.clear(red)
        ctx.frame_submit(table)
        same(fb.present_nearest(W, H), ofb.image(), "clear, frame, present")
        fb.clear(red)
        ctx.frame_submit(table)
        same(fb.present_nearest(401, 97), nearest(ofb.image(), 401, 97), "clear, frame, present (again)")
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the reference's frame order -- gradient, sky, stars, meshes -- in a pipelined loop

@pytest.mark.gpu
@pytest.mark.parametrize("deep", [0, 1], ids=["safe", "async_depth_1"])
def test_gpu_sky_inside_a_pipelined_frame_loop(oracle, deep):
    """clear_gradient, render_skybox_mesh, draw_star_diamonds, frame_submit, download_async, six frames alternating two cameras;
    every delivered frame is compared with the oracle's, the presenter one frame behind."""
    from bonnie32_amd import rasterizer as R, scenegen
    meshes = [scenegen.make_scene("C1", n_tris=n, seed=600 + i, variant="gouraud", bbox_px=bb) for i, (n, bb) in enumerate(((1800, 150.0), (900, 400.0)))]
    W, H = meshes[0].width, meshes[0].height
    st = b32.RasterSettings.game()
    st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7)]
    cams = [meshes[0].camera, b32.Camera(position=(40.0, -25.0, 60.0))]
    skies = [sky_mesh(cam.position) for cam in cams]
    rng = np.random.default_rng(13)
    cx, cy, rgb = rng.integers(-3, W + 3, 80), rng.integers(-3, H + 3, 80), rng.integers(0, 256, (80, 3))
    want = []
    for cam, (sv, sf) in zip(cams, skies):
        o = oracle.Framebuffer(W, H)
        o.clear_gradient(TOP, BOTTOM)
        assert o.render_skybox_mesh(sv, sf, cam) == 0
        o.draw_star_diamonds(cx, cy, rgb, 3.0)
        for sc in meshes:
            assert oracle.render_mesh_15(o, sc.vertices, sc.faces, sc.textures, cam, st)[0] == 0
        want.append(o.pixels.copy())
    assert (want[0] != want[1]).mean() > 0.3
    ctx = R.Context(0)
    bufs = []
    try:
        ctx.set_async_depth(deep)
        fb = R.Framebuffer(W, H, ctx)
        slots = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc in meshes]
        tables = [ctx.make_frame_table(cam, st, slots) for cam in cams]
        for _ in range(2):
            bufs.append(ctx.host_alloc(W * H * 4))
        tickets = [0, 0]
        n_frames = 6
        for i in range(n_frames):
            fb.clear_gradient(TOP, BOTTOM)
            fb.render_skybox_mesh(*skies[i & 1], cams[i & 1])
            fb.draw_star_diamonds(cx, cy, rgb, 3.0)
            ctx.frame_submit(tables[i & 1])
            tickets[i & 1] = ctx.download_async(bufs[i & 1][1])
            if i > 0:
                ctx.ticket_wait(tickets[(i - 1) & 1])
                same(bufs[(i - 1) & 1][0], want[(i - 1) & 1], f"frame {i - 1}")
        ctx.ticket_wait(tickets[(n_frames - 1) & 1])
        same(bufs[(n_frames - 1) & 1][0], want[(n_frames - 1) & 1], f"frame {n_frames - 1}")
        ctx.finish()
    finally:
        for _, p in bufs:
            ctx.host_free(p)
        ctx.close()
