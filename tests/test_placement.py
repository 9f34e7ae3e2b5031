"""Placed draws: facing and world offset per draw (render_asset_parts, scene.rs:112-171) applied inside the setup kernel.

The reference rotates an asset's local vertices about Y by the object's facing and translates them by its world position, per part, per
object and per frame, and only then calls render_mesh_15 / render_mesh.  `place_vertices` restates that on the host; the expected frame
of every GPU test here is the oracle's sequential render_mesh_15 / render_mesh calls on `place_vertices` output -- literally what the
reference does -- and every comparison is bit for bit: pixels, the depth buffer viewed as u32, and triangles_drawn."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import scenegen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden", "scenes", "real")
f32 = np.float32


# ================================================================== without a GPU
def _scalar_place(v, cos_f, sin_f, wp):
    """scene.rs:143-152 written out one separately rounded f32 operation at a time, vertex by vertex."""
    out = v.copy()
    c, s = f32(cos_f), f32(sin_f)
    wx, wy, wz = (f32(x) for x in wp)
    with np.errstate(all="ignore"):
        for i in range(len(v)):
            x, y, z = (f32(t) for t in v["pos"][i])
            xc = f32(x * c); zs = f32(z * s); rx = f32(xc - zs)
            xs = f32(x * s); zc = f32(z * c); rz = f32(xs + zc)
            out["pos"][i] = (f32(rx + wx), f32(y + wy), f32(rz + wz))
            nx, ny, nz = (f32(t) for t in v["normal"][i])
            a = f32(nx * c); b = f32(nz * s); d = f32(nx * s); e = f32(nz * c)
            out["normal"][i] = (f32(a - b), ny, f32(d + e))
    return out


def _same_bits(a, b):
    """bit-for-bit, except that any NaN equals any NaN (the payload of an invalid operation is not the reference's business)"""
    ua, ub = np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32)
    return bool(np.all((ua == ub) | (np.isnan(a) & np.isnan(b))))


def _random_vertices(rng, n, scale):
    v = np.zeros(n, b32.abi.VERTEX_DTYPE)
    v["pos"] = (rng.standard_normal((n, 3)) * scale).astype(f32)
    v["uv"] = rng.random((n, 2)).astype(f32)
    nrm = rng.standard_normal((n, 3)).astype(f32)
    v["normal"] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True).astype(f32)
    for k in ("r", "g", "b", "blend"):
        v[k] = rng.integers(0, 256, n).astype(np.uint8)
    return v


def test_place_vertices_is_the_scalar_f32_restatement():
    """place_vertices against scene.rs:143-152 evaluated step by step in f32 scalars: random values, zeros of both signs, large
    magnitudes (overflow to infinity and inf - inf included); uv and colour pass through."""
    rng = np.random.default_rng(20)
    v = _random_vertices(rng, 3000, 2000.0)
    special = [0.0, -0.0, 1.0, -1.0, 1e-40, -1e-45, 16777216.0, 1e30, -1e30, 3e38, -3e38]
    sv = np.zeros(len(special) ** 2, b32.abi.VERTEX_DTYPE)
    grid = np.array([(a, b) for a in special for b in special], f32)
    sv["pos"][:, 0] = grid[:, 0]; sv["pos"][:, 2] = grid[:, 1]; sv["pos"][:, 1] = grid[::-1, 0]
    sv["normal"][:, 0] = grid[:, 1]; sv["normal"][:, 2] = grid[:, 0]; sv["normal"][:, 1] = grid[::-1, 1]
    v = np.concatenate([v, sv])
    for cos_f, sin_f, wp in [(np.cos(f32(0.7)), np.sin(f32(0.7)), (100.5, -20.25, 3000.0)), (np.cos(f32(-2.9)), np.sin(f32(-2.9)), (-1e-3, 0.0, -0.0)),
                             (0.0, -1.0, (0.0, 0.0, 0.0)), (-0.0, 1.0, (1e30, -1e30, 3e38)), (0.6, 0.8, (np.inf, 0.0, -np.inf))]:
        got = b32.place_vertices(v, cos_f, sin_f, wp)
        want = _scalar_place(v, cos_f, sin_f, wp)
        assert _same_bits(got["pos"], want["pos"]) and _same_bits(got["normal"], want["normal"]), (cos_f, sin_f, wp)
        assert np.array_equal(got["uv"].view(np.uint32), v["uv"].view(np.uint32))
        assert all(np.array_equal(got[k], v[k]) for k in ("r", "g", "b", "blend"))
    assert b32.place_vertices(v[:0], 1.0, 0.0, (0, 0, 0)).shape == (0,)


def test_identity_placement_changes_only_the_sign_of_zero():
    """cos_f = 1, sin_f = 0, world_pos = 0 multiplies by one and adds zero: equal to the input except that a negative zero may come
    out positive -- which is why the reference's untransformed branch (and a NULL placement) is NOT this."""
    rng = np.random.default_rng(21)
    v = _random_vertices(rng, 2000, 500.0)
    zeros = np.array([0.0, -0.0], f32)
    v["pos"][:400] = zeros[rng.integers(0, 2, (400, 3))]
    v["normal"][200:600] = zeros[rng.integers(0, 2, (400, 3))]
    v["pos"][600:700, 0] = -0.0; v["normal"][700:800, 2] = -0.0
    got = b32.place_vertices(v, 1.0, 0.0, (0.0, 0.0, 0.0))
    changed = 0
    for k in ("pos", "normal"):
        a, g = v[k], got[k]
        assert np.array_equal(a, g)                                  # numerically equal everywhere (-0.0 == 0.0)
        diff = a.view(np.uint32) != g.view(np.uint32)
        assert np.all(a.view(np.uint32)[diff] == 0x80000000) and np.all(g.view(np.uint32)[diff] == 0)      # -0.0 in, +0.0 out: nothing else
        changed += int(diff.sum())
    assert changed > 0                                               # the difference exists: identity is not "no placement"
    assert np.array_equal(got["uv"].view(np.uint32), v["uv"].view(np.uint32))


def test_random_set_tells_a_fused_evaluation_apart():
    """x * cos - z * sin contracted into a fused multiply-add rounds differently for some inputs.  The fused forms are evaluated in
    float64 (the product of two f32 is exact there) and rounded once; the set must contain values where they differ from the separately
    rounded result, so that nothing built with FMA contraction can pass the comparisons of this file -- and place_vertices must be
    the separately rounded one."""
    rng = np.random.default_rng(22)
    v = _random_vertices(rng, 4000, 3000.0)
    c, s = np.cos(f32(0.9)), np.sin(f32(0.9))
    got = b32.place_vertices(v, c, s, (0.0, 0.0, 0.0))
    x, z = v["pos"][:, 0], v["pos"][:, 2]
    x64, z64, c64, s64 = x.astype(np.float64), z.astype(np.float64), np.float64(c), np.float64(s)
    unfused = (x * c).astype(f32) - (z * s).astype(f32)                 # (rx + 0.0 == rx for every rx but -0.0)
    fused_a = (x64 * c64 - (z * s).astype(f32).astype(np.float64)).astype(f32)       # fma(x, c, -(z * s))
    fused_b = ((x * c).astype(f32).astype(np.float64) - z64 * s64).astype(f32)       # fma(-z, s, x * c)
    assert np.array_equal(got["pos"][:, 0], unfused)
    n_a, n_b = int((fused_a != unfused).sum()), int((fused_b != unfused).sum())
    assert n_a >= 1 and n_b >= 1, (n_a, n_b)
    assert int((got["pos"][:, 0] != fused_a).sum()) == n_a and int((got["pos"][:, 0] != fused_b).sum()) == n_b


def test_placement_struct_and_symbols():
    """sizeof(B32Placement) == 20 on both sides of the boundary, and the placed entries resolve in the built library."""
    import subprocess
    import tempfile
    import __graft_entry__ as g
    g.build()
    lib = b32.abi.load_library()
    assert C.sizeof(b32.abi.B32Placement) == 20
    assert b32.abi.B32Placement.sin_f.offset == 4 and b32.abi.B32Placement.world_pos.offset == 8
    for name in ("b32_frame_add_scene_placed", "b32_frame_submit_placed", "b32_render_scene_15_placed_async"):
        assert name in {n for n, _, _ in b32.abi.SYMBOLS} and getattr(lib, name).argtypes is not None
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void){ printf("%zu %zu %zu\\n", sizeof(B32Placement), offsetof(B32Placement, sin_f), offsetof(B32Placement, world_pos)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [20, 4, 8]
    # NULL context: B32_E_ARG from every placed entry, no device needed
    E = b32.abi.B32_E_ARG
    assert lib.b32_frame_add_scene_placed(None, None, None, None) == E
    assert lib.b32_frame_submit_placed(None, None, None, None, None, None, None, 0) == E
    assert lib.b32_render_scene_15_placed_async(None, None, None, None, None) == E


def test_placement_helper_has_transform_rule():
    """scene.rs:125: facing.abs() > 0.0001 || any world_pos component's abs() > 0.0001, in f32."""
    P = b32.Placement
    eps = f32(0.0001)
    above, below = np.nextafter(eps, f32(1.0)), np.nextafter(eps, f32(0.0))
    assert not P(facing=0.0, world_pos=(0.0, 0.0, 0.0)).has_transform and P(facing=0.0).pack() is None
    assert not P(facing=eps, world_pos=(eps, -eps, eps)).has_transform              # exactly 0.0001: not greater
    assert not P(facing=-below, world_pos=(below, below, -below)).has_transform
    assert P(facing=above).has_transform and P(facing=-above).has_transform
    for k in range(3):
        for sign in (1.0, -1.0):
            wp = [0.0, 0.0, 0.0]; wp[k] = sign * above
            assert P(facing=0.0, world_pos=wp).has_transform
            wp[k] = sign * eps
            assert not P(facing=0.0, world_pos=wp).has_transform
    assert not P(facing=0.00010000000001).has_transform                            # rounds to the f32 0.0001
    p = P(facing=0.7, world_pos=(1.0, 2.0, 3.0))
    assert p.cos_f.dtype == f32 and p.cos_f == np.cos(f32(0.7)) and p.sin_f == np.sin(f32(0.7))
    c = p.pack()
    assert (c.cos_f, c.sin_f, tuple(c.world_pos)) == (float(p.cos_f), float(p.sin_f), (1.0, 2.0, 3.0))
    # explicit cos / sin: taken as they are (no trigonometry, no unit-length check), and always a transform
    q = P(cos_f=0.5, sin_f=0.25, world_pos=(0.0, 0.0, 0.0))
    assert q.has_transform and (q.pack().cos_f, q.pack().sin_f) == (0.5, 0.25)
    assert P(cos_f=1.0, sin_f=0.0, has_transform=False).pack() is None
    with pytest.raises(ValueError):
        P(world_pos=(1.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        P(cos_f=1.0)
    # apply(): the untransformed branch hands the local vertices over as they are, sign of zero included
    v = _random_vertices(np.random.default_rng(3), 16, 10.0); v["pos"][:4] = -0.0
    assert np.array_equal(P(facing=0.0).apply(v).view(np.uint8), v.view(np.uint8))
    assert np.array_equal(p.apply(v).view(np.uint8), b32.place_vertices(v, p.cos_f, p.sin_f, p.world_pos).view(np.uint8))


# ================================================================== on the GPU
def _real(name):
    from bonnie32_amd import scenefile
    return scenefile.read_scene(os.path.join(REAL, name + ".b32scene"))


class _Frame:
    """The frame of case 1: the dungeon room plus the three parts of the reference's sample asset, each uploaded once and placed
    `n_objects` times (render_scene, scene.rs:226-259: per object one render_asset_parts call, i.e. one placement for its three parts,
    per-part double_sided), base settings RasterSettings::game() with a directional, a point and a spot light, fog on some meshes."""

    def __init__(self, n_objects=11):
        self.room = _real("dungeon-room0-game")
        self.parts = [_real("asset3-part0-game"), _real("asset3-part1-game"), _real("asset3-part2-painter")]
        for m in [self.room] + self.parts:                             # the 8-bit-colour path's texels: the same RGB555 texels widened to Color
            m.textures8 = [b32.Texture.from_texture15(t) for t in m.textures]
        self.cam = self.room.camera
        self.W, self.H = self.room.width, self.room.height
        self.clear = b32.Color(12, 14, 40)
        self.n_objects = n_objects
        pos = np.array(self.cam.position, f32); bx = np.array(self.cam.basis_x, f32); bz = np.array(self.cam.basis_z, f32)
        self.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7),
                       b32.Light.point(tuple(pos + bz * f32(2500.0) + np.array([0.0, 900.0, 0.0], f32)), 6000.0, 1.3),
                       b32.Light.spot(tuple(pos + np.array([0.0, 1500.0, 0.0], f32)), tuple(bz + np.array([0.0, -0.25, 0.0], f32)), 0.6, 9000.0, 1.5)]
        self.fogs = [None, (2500.0, 5000.0, 12000.0, b32.Color(40, 50, 70)), (1500.0, 4000.0, 9000.0, b32.Color(90, 20, 20))]
        self._pos, self._bx, self._bz = pos, bx, bz

    def settings(self, zbuffer=True, rgb555=True, wire=False):
        st = b32.RasterSettings.game()
        st.use_zbuffer = zbuffer; st.use_rgb555 = rgb555; st.backface_wireframe = wire
        st.lights = list(self.lights)
        return st

    def placements(self, t=0.0):
        """One placement per object at time t: different facings, positions in front of the room's camera, object 2 far to the side
        (partly off-screen), object 5 behind the near plane (every face rejected).  (The room in front of them is the entry WITHOUT a
        placement in the same run.)"""
        out = []
        for k in range(self.n_objects):
            d = 900.0 + 250.0 * k + 30.0 * np.sin(0.9 * t + k)
            lat = -1500.0 + 300.0 * k + 90.0 * np.cos(0.7 * t + 2 * k)
            if k == 2:
                lat = 3300.0 + 100.0 * t
            if k == 5:
                d = -4000.0 + 10.0 * t
            wp = self._pos + self._bz * f32(d) + self._bx * f32(lat) + np.array([0.0, -700.0 - 40.0 * k + 30.0 * t, 0.0], f32)
            out.append(b32.Placement(facing=0.55 * k - 2.0 + 0.31 * t, world_pos=tuple(wp)))
        return out

    def entries(self, placements):
        """(mesh index 0 room / 1..3 part, per-mesh params, placement or None) in draw order: the room, then object by object."""
        e = [(0, dict(ambient=self.room.settings.ambient, backface_cull=True, fog=self.fogs[1]), None)]
        for k, pl in enumerate(placements):
            for p in range(3):
                cull = [k % 2 == 0, False, k % 3 == 0][p]            # per-part double_sided, varied from object to object
                e.append((1 + p, dict(ambient=0.25 + 0.05 * (k % 4), backface_cull=cull, fog=self.fogs[k % 3]), pl))
        return e

    def mesh(self, i):
        return self.room if i == 0 else self.parts[i - 1]

    def oracle_frame(self, oracle, st, entries):
        """The reference's frame: sequential render_mesh_15 / render_mesh calls on host-placed vertices.  Returns the framebuffer and
        triangles_drawn per mesh."""
        ofb = oracle.Framebuffer(self.W, self.H); ofb.clear(self.clear)
        drawn = []
        for i, p, pl in entries:
            m = self.mesh(i)
            v = m.vertices if pl is None else pl.apply(m.vertices)
            s2 = copy.copy(st); s2.ambient = p["ambient"]; s2.backface_cull = p["backface_cull"]
            s2.backface_wireframe = st.backface_wireframe and p["backface_cull"]        # scene.rs:136
            if st.use_rgb555:
                rc, tm = oracle.render_mesh_15(ofb, v, m.faces, m.textures, self.cam, s2, p["fog"])
            else:
                rc, tm = oracle.render_mesh(ofb, v, m.faces, m.textures8, self.cam, s2)
            assert rc == 0
            drawn.append(tm.triangles_drawn)
        return ofb, drawn

    def upload(self, R, fb, rgb555=True):
        """Room and parts, each uploaded ONCE."""
        if rgb555:
            return [R.ResidentScene(fb, m.vertices, m.faces, m.textures).detach() for m in [self.room] + self.parts]
        return [R.ResidentScene(fb, m.vertices, m.faces, textures8=m.textures8).detach() for m in [self.room] + self.parts]

    @staticmethod
    def last_draw_count(st, entries, drawn, batch_on):
        """triangles_drawn of the frame's LAST draw (what b32_frame_finish reports): the last mesh's, or -- when the frame's last draw
        is a merged run (z-buffer mode, RGB555, batching on; runs of at most 32 meshes, broken by meshes with a wireframe phase) -- the
        run's sum.  None of the fixtures has a transparent pass."""
        wire = [bool(st.backface_wireframe and p["backface_cull"]) for _, p, _ in entries]
        if not (st.use_zbuffer and st.use_rgb555 and batch_on):
            return drawn[-1]
        i, n, last = 0, len(entries), None
        while i < n:
            k = i
            while k < n and k - i < 32 and not wire[k]:
                k += 1
            if k - i < 2:
                last = drawn[i]; i += 1
            else:
                last = sum(drawn[i:k]); i = k
        return last


_ORACLE_CACHE = {}


def _case1_expect(oracle, fr, zbuffer, rgb555, wire):
    key = (zbuffer, rgb555, wire)
    if key not in _ORACLE_CACHE:
        st = fr.settings(zbuffer, rgb555, wire)
        entries = fr.entries(fr.placements(0.0))
        ofb, drawn = fr.oracle_frame(oracle, st, entries)
        _ORACLE_CACHE[key] = (ofb.pixels.copy(), ofb.zbuffer.copy(), drawn)
    return _ORACLE_CACHE[key]


def _submit(ctx, fr, st, slots, entries, how="add"):
    if how == "add":
        ctx.frame_begin(fr.cam, st)
        for i, p, pl in entries:
            ctx.frame_add(slots[i], placement=pl, **p)
        ctx.frame_end()
    else:
        table = ctx.make_frame_table(fr.cam, st, [slots[i] for i, _, _ in entries], fogs=[p["fog"] for _, p, _ in entries],
                                     ambients=[p["ambient"] for _, p, _ in entries], placements=[pl for _, _, pl in entries],
                                     backface_culls=[p["backface_cull"] for _, p, _ in entries])
        ctx.frame_submit(table)


def _assert_frame(fb, pixels, zbuffer, what=""):
    got = fb.pixels
    assert np.array_equal(got, pixels), f"{what}: {int((got != pixels).sum())} bytes differ"
    gz = fb.zbuffer.view(np.uint32)
    assert np.array_equal(gz, zbuffer.view(np.uint32)), f"{what}: {int((gz != zbuffer.view(np.uint32)).sum())} depths differ"


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "nopacked"])
@pytest.mark.parametrize("batch", [True, False], ids=["batch", "nobatch"])
@pytest.mark.parametrize("wire", [False, True], ids=["nowire", "wire"])
@pytest.mark.parametrize("rgb555", [True, False], ids=["rgb555", "rgba8"])
@pytest.mark.parametrize("zbuffer", [True, False], ids=["zbuffer", "painter"])
def test_batched_frame_of_placed_instances(oracle, zbuffer, rgb555, wire, batch, packed):
    """Case 1: a room (no placement) plus 11 objects of three resident parts each (33 placed draws of 3 uploads), per-part culling, three lights, fog on some meshes -- against the oracle's sequential calls on host-placed vertices.
    z-buffer mode draws merged runs (34 meshes: the 32-mesh split is inside the frame), painter's mode and the 8-bit-colour path draw
    mesh by mesh; the same frame through b32_frame_submit_placed; then a second frame with other placements on the same context."""
    from bonnie32_amd import rasterizer as R
    fr = _Frame()
    px, zb, drawn = _case1_expect(oracle, fr, zbuffer, rgb555, wire)
    assert len({d for d in drawn[1:]}) > 1 and sum(drawn[1:]) > 60 and drawn[1 + 3 * 5] == drawn[2 + 3 * 5] == drawn[3 + 3 * 5] == 0      # object 5: behind the near plane
    st = fr.settings(zbuffer, rgb555, wire)
    ctx = R.Context(0)
    ctx.set_routes((0 if batch else R.Context.ROUTE_BATCH) | (0 if packed else R.Context.ROUTE_PACKED_STREAMS))
    fb = R.Framebuffer(fr.W, fr.H, ctx)
    slots = fr.upload(R, fb, rgb555)
    entries = fr.entries(fr.placements(0.0))
    want_drawn = fr.last_draw_count(st, entries, drawn, batch)
    for how in ("add", "table"):
        fb.clear(fr.clear)
        _submit(ctx, fr, st, slots, entries, how)
        tm = ctx.finish()
        _assert_frame(fb, px, zb, how)
        assert tm.triangles_drawn == want_drawn, (how, tm.triangles_drawn, want_drawn)
    bc = ctx.batch_counts()
    if zbuffer and rgb555 and batch and not wire:
        assert bc["merged_draws"] == 4 and bc["single_draws"] == 0 and bc["merged_built"] == 2, bc        # runs [0..31] [32, 33], built once
    elif not (zbuffer and rgb555 and batch):
        assert bc["merged_draws"] == 0 and bc["single_draws"] == 2 * len(entries), bc
    else:
        assert bc["merged_draws"] > 0 and bc["single_draws"] > 0, bc
    # other placements, same context: nothing is uploaded, nothing merged again
    built = bc["merged_built"]
    entries2 = fr.entries(fr.placements(3.0))
    ofb2, drawn2 = fr.oracle_frame(oracle, st, entries2)
    fb.clear(fr.clear)
    _submit(ctx, fr, st, slots, entries2, "table")
    tm = ctx.finish()
    _assert_frame(fb, ofb2.pixels, ofb2.zbuffer, "moved")
    assert tm.triangles_drawn == fr.last_draw_count(st, entries2, drawn2, batch)
    assert not np.array_equal(ofb2.pixels, px) and ctx.batch_counts()["merged_built"] == built
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("deep", [0, 1], ids=["safe", "deep"])
def test_moving_objects_delivered_frames(oracle, deep):
    """Case 2: ten frames through b32_frame_submit_placed + b32_fb_download_async + tickets, EVERY placement changing every frame, every
    delivered frame compared with the oracle's; merged draws happen and no merged mesh is built after frame 0."""
    from bonnie32_amd import rasterizer as R
    fr = _Frame()
    st = fr.settings()
    n_frames = 10
    want = []
    for t in range(n_frames):
        ofb, _ = fr.oracle_frame(oracle, st, fr.entries(fr.placements(float(t))))
        want.append(ofb.pixels.copy())
    assert all(not np.array_equal(want[t], want[t + 1]) for t in range(n_frames - 1))
    ctx = R.Context(0)
    ctx.set_async_depth(deep)
    fb = R.Framebuffer(fr.W, fr.H, ctx)
    slots = fr.upload(R, fb)
    entries = fr.entries(fr.placements(0.0))
    table = ctx.make_frame_table(fr.cam, st, [slots[i] for i, _, _ in entries], fogs=[p["fog"] for _, p, _ in entries],
                                 ambients=[p["ambient"] for _, p, _ in entries], placements=[pl for _, _, pl in entries],
                                 backface_culls=[p["backface_cull"] for _, p, _ in entries])
    bufs = [ctx.host_alloc(fr.W * fr.H * 4) for _ in range(2)]
    tickets = [0, 0]
    built = []
    try:
        for t in range(n_frames):
            pls = fr.placements(float(t))
            ctx.set_table_placements(table, [None] + [pls[k] for k in range(fr.n_objects) for _ in range(3)])
            fb.clear(fr.clear)
            ctx.frame_submit(table)
            tickets[t & 1] = ctx.download_async(bufs[t & 1][1])
            built.append(ctx.batch_counts()["merged_built"])
            if t > 0:
                ctx.ticket_wait(tickets[(t - 1) & 1])
                got = bufs[(t - 1) & 1][0]
                assert np.array_equal(got, want[t - 1]), f"frame {t - 1}: {int((got != want[t - 1]).sum())} bytes differ"
        ctx.ticket_wait(tickets[(n_frames - 1) & 1])
        assert np.array_equal(bufs[(n_frames - 1) & 1][0], want[n_frames - 1])
        ctx.finish()
        bc = ctx.batch_counts()
        assert bc["merged_draws"] == 2 * n_frames and bc["frames"] == n_frames, bc
        assert built[0] == 2 and all(b == built[0] for b in built) and bc["merged_built"] == built[0], (built, bc)
    finally:
        for _, p in bufs:
            ctx.host_free(p)
        ctx.close()


@pytest.mark.gpu
def test_null_placement_is_the_existing_entry_and_identity_is_not(oracle):
    """Case 3: the placed entries with place = NULL give the bytes of the existing entries (frame and single draw); an explicit identity
    placement gives the oracle's frame on place_vertices(identity)."""
    from bonnie32_amd import rasterizer as R
    fr = _Frame(n_objects=3)
    st = fr.settings()
    none = b32.Placement(facing=0.0)                                  # has_transform false: pack() is None -> the placed entry gets NULL
    assert none.pack() is None
    plain = [(i, p, None) for i, p, _ in fr.entries([None] * 3)]
    nulls = [(i, p, none) for i, p, _ in plain]
    ident = b32.Placement(cos_f=1.0, sin_f=0.0, world_pos=(0.0, 0.0, 0.0))
    idents = [(i, p, ident) for i, p, _ in plain]
    ctx = R.Context(0)
    fb = R.Framebuffer(fr.W, fr.H, ctx)
    slots = fr.upload(R, fb)
    frames = {}
    for name, ent, how in (("existing", plain, "add"), ("existing_table", plain, "table"), ("null_add", nulls, "add"), ("null_table", nulls, "table"),
                           ("identity", idents, "table")):
        fb.clear(fr.clear)
        _submit(ctx, fr, st, slots, ent, how)
        tm = ctx.finish()
        frames[name] = (fb.pixels, fb.zbuffer.view(np.uint32).copy(), tm.triangles_drawn)
    for name in ("existing_table", "null_add", "null_table"):
        assert all(np.array_equal(a, b) for a, b in zip(frames[name][:2], frames["existing"][:2])) and frames[name][2] == frames["existing"][2], name
    o_plain, d_plain = fr.oracle_frame(oracle, st, plain)
    o_ident, d_ident = fr.oracle_frame(oracle, st, idents)
    assert np.array_equal(frames["existing"][0], o_plain.pixels) and np.array_equal(frames["existing"][1], o_plain.zbuffer.view(np.uint32))
    assert np.array_equal(frames["identity"][0], o_ident.pixels) and np.array_equal(frames["identity"][1], o_ident.zbuffer.view(np.uint32))
    assert frames["existing"][2] == sum(d_plain) and frames["identity"][2] == sum(d_ident)
    # the single draw
    sc = scenegen.make_scene("C1", variant="gouraud")
    sc.vertices["pos"][::7, 0] = -0.0; sc.vertices["normal"][::5, 2] = -0.0
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings); t0 = rs.finish(); a = (fb.pixels, fb.zbuffer.view(np.uint32).copy())
    fb.clear(sc.clear_color); rs.render_placed_async(None); t1 = rs.finish(); b = (fb.pixels, fb.zbuffer.view(np.uint32).copy())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and t0.triangles_drawn == t1.triangles_drawn
    fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings, placement=ident); t2 = rs.finish()
    ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    rc, otm = oracle.render_mesh_15(ofb, ident.apply(sc.vertices), sc.faces, sc.textures, sc.camera, sc.settings)
    assert rc == 0
    _assert_frame(fb, ofb.pixels, ofb.zbuffer, "identity, single draw")
    assert t2.triangles_drawn == otm.triangles_drawn
    ctx.close()


def _single_cases():
    def big(variant):
        def make():
            sc = scenegen.make_scene("C3", n_tris=20_000, width=640, height=480, bbox_px=200.0, seed=12, variant=variant)
            return sc, sc.settings, None
        return make

    def small(variant, **over):
        def make():
            sc = scenegen.make_scene("C1", variant=variant, seed=77)
            st = copy.copy(sc.settings)
            for k, v in over.items():
                if k not in ("lights", "fog"):
                    setattr(st, k, v)
            if over.get("lights"):
                st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7), b32.Light.point((300.0, -200.0, 2500.0), 4000.0, 1.2),
                             b32.Light.spot((0.0, 0.0, 0.0), (0.1, 0.0, 1.0), 0.5, 7000.0, 1.4)]
            return sc, st, (1200.0, 2500.0, 5200.0, b32.Color(40, 50, 70)) if over.get("fog") else None
        return make
    return {
        "big-gouraud-zbuffer": big("gouraud"),        # more than 8192 faces: direct binning, packed (lit) streams from the second frame on
        "big-painter-unlit": big("bench"),            # ... and the frame the plain kernel form would take without a placement
        "ortho": small("gouraud", ortho_projection=(0.05, 10.0, -5.0)),
        "float-projection": small("float"),
        "xray": small("gouraud", xray_mode=True),
        "transparent-pass": small("blend"),
        "flat-3-lights": small("gouraud", shading=b32.abi.SHADE_FLAT, lights=True),
        "gouraud-3-lights-fog": small("gouraud", shading=b32.abi.SHADE_GOURAUD, lights=True, fog=True),
        "painter-lit": small("gouraud", use_zbuffer=False, lights=True),
    }


_SINGLE = _single_cases()
_SINGLE_PLACEMENTS = [b32.Placement(facing=0.21, world_pos=(350.0, -120.0, 400.0)), b32.Placement(facing=-0.33, world_pos=(-500.0, 260.0, 900.0)),
                      b32.Placement(facing=3.0, world_pos=(100.0, 50.0, 7000.0)), b32.Placement(facing=0.05, world_pos=(0.0, 0.0, -300.0))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_SINGLE))
def test_single_placed_draws(oracle, name):
    """Case 4: b32_render_scene_15_placed_async, four frames with a different placement each on one context (so whatever the scene
    learned from the earlier frames -- packed streams, region capacities -- is in use while the placement changes)."""
    from bonnie32_amd import rasterizer as R
    sc, st, fog = _SINGLE[name]()
    ctx = R.Context(0)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    drawn, frames = [], []
    for n, pl in enumerate(_SINGLE_PLACEMENTS):
        ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
        rc, otm = oracle.render_mesh_15(ofb, pl.apply(sc.vertices), sc.faces, sc.textures, sc.camera, st, fog)
        assert rc == 0
        fb.clear(sc.clear_color)
        rs.render_async(sc.camera, st, fog, placement=pl)
        tm = rs.finish()
        _assert_frame(fb, ofb.pixels, ofb.zbuffer, f"{name}, placement {n}")
        assert tm.triangles_drawn == otm.triangles_drawn
        drawn.append(otm.triangles_drawn); frames.append(ofb.pixels.tobytes())
    assert max(drawn) > 100 and len(set(frames)) == len(frames), drawn        # every placement gives another picture
    if name.startswith("big"):
        assert len(sc.faces) > 8192 and ctx.route_counts()["direct_bin"] >= len(_SINGLE_PLACEMENTS), ctx.route_counts()
    ctx.close()


@pytest.mark.gpu
def test_single_placed_draw_of_an_8bit_colour_scene(oracle):
    """... and the 8-bit-colour path (render_mesh, scene.rs:166-168) through the same entry."""
    from bonnie32_amd import rasterizer as R
    fr = _Frame(n_objects=1)
    m = fr.parts[0]
    st = fr.settings(zbuffer=True, rgb555=False)
    ctx = R.Context(0)
    fb = R.Framebuffer(fr.W, fr.H, ctx)
    rs = R.ResidentScene(fb, m.vertices, m.faces, textures8=m.textures8)
    ofb = oracle.Framebuffer(fr.W, fr.H); ofb.clear(fr.clear)
    fb.clear(fr.clear)
    total = 0
    for k, pl in enumerate(_Frame(n_objects=4).placements(1.0)):
        rc, otm = oracle.render_mesh(ofb, pl.apply(m.vertices), m.faces, m.textures8, fr.cam, st)
        assert rc == 0
        rs.render_async(fr.cam, st, None, placement=pl)
        assert rs.finish().triangles_drawn == otm.triangles_drawn
        total += otm.triangles_drawn
    assert total > 10
    _assert_frame(fb, ofb.pixels, ofb.zbuffer, "8-bit colour")
    ctx.close()


@pytest.mark.gpu
def test_banded_placed_frame_equals_the_unbanded_one(oracle):
    """Case 5: the frame of case 1 in z-buffer mode drawn as two set_band halves on one GPU into one framebuffer."""
    from bonnie32_amd import rasterizer as R
    fr = _Frame()
    px, zb, _ = _case1_expect(oracle, fr, True, True, False)
    st = fr.settings()
    ctx = R.Context(0)
    fb = R.Framebuffer(fr.W, fr.H, ctx)
    slots = fr.upload(R, fb)
    entries = fr.entries(fr.placements(0.0))
    for y0, y1 in ((0, 100), (100, fr.H)):                            # (100: not a multiple of the tile height)
        fb.set_band(y0, y1)
        fb.clear(fr.clear)
        _submit(ctx, fr, st, slots, entries, "table")
        ctx.finish()
    fb.set_band(0, fr.H)
    _assert_frame(fb, px, zb, "two bands")
    assert ctx.batch_counts()["merged_draws"] == 4
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("zbuffer", [False, True], ids=["painter", "zbuffer"])
def test_placed_errors(oracle, zbuffer):
    """Case 6: a placement whose world_pos is infinite.  Where the reference panics on the NaN sort key of those placed vertices
    (painter's mode) the finish reports B32_E_NAN_KEY and the mesh draws nothing; where the oracle succeeds on them, the frame is the
    oracle's.  A placed add outside an open frame: B32_E_ARG."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C1", variant="gouraud")
    st = copy.copy(sc.settings); st.use_zbuffer = zbuffer; st.backface_cull = False
    pl = b32.Placement(facing=0.3, world_pos=(np.inf, 0.0, 100.0))
    good = b32.Placement(facing=0.3, world_pos=(10.0, 0.0, 100.0))
    ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    assert oracle.render_mesh_15(ofb, good.apply(sc.vertices), sc.faces, sc.textures, sc.camera, st)[0] == 0
    before = (ofb.pixels.copy(), ofb.zbuffer.copy())
    with np.errstate(all="ignore"):
        rc, otm = oracle.render_mesh_15(ofb, pl.apply(sc.vertices), sc.faces, sc.textures, sc.camera, st)
    if not zbuffer:
        assert rc == b32.abi.B32_E_NAN_KEY                            # (the case the issue is about really occurs)
    ctx = R.Context(0)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    for how in ("single", "frame"):
        fb.clear(sc.clear_color)
        rs.render_async(sc.camera, st, placement=good); rs.finish()
        if how == "single":
            rs.render_async(sc.camera, st, placement=pl)
        else:
            ctx.frame_begin(sc.camera, st); ctx.frame_add(rs, placement=pl); ctx.frame_end()
        if rc == b32.abi.B32_E_NAN_KEY:
            with pytest.raises(R.B32Error) as e:
                ctx.finish()
            assert e.value.code == b32.abi.B32_E_NAN_KEY
            _assert_frame(fb, before[0], before[1], how)             # the failing mesh drew nothing
        else:
            assert rc == 0 and ctx.finish().triangles_drawn == otm.triangles_drawn
            _assert_frame(fb, ofb.pixels, ofb.zbuffer, how)
    # argument errors
    E = b32.abi.B32_E_ARG
    p = good.pack()
    assert ctx.lib.b32_frame_add_scene_placed(ctx.h, rs._slot, None, C.byref(p)) == E          # no open frame
    ctx.frame_begin(sc.camera, st); ctx.frame_end()
    assert ctx.lib.b32_frame_add_scene_placed(ctx.h, rs._slot, None, C.byref(p)) == E          # closed again
    ctx.frame_begin(sc.camera, st)
    assert ctx.lib.b32_frame_add_scene_placed(ctx.h, None, None, C.byref(p)) == E              # no slot
    ctx.frame_end()
    assert ctx.lib.b32_frame_submit_placed(ctx.h, None, None, None, None, None, None, 1) == E
    assert ctx.lib.b32_render_scene_15_placed_async(ctx.h, None, None, None, C.byref(p)) == E
    ctx.finish()
    ctx.close()


@pytest.mark.gpu
def test_placement_beyond_the_learned_capacity_is_redrawn_with_its_placement(oracle):
    """What a scene learned from earlier frames (the tile regions' capacity of the direct binning) was learned from OTHER placements and
    stays a hint: a mesh of more than 65536 faces is drawn spread over the frame, then with a placement that moves it away until it falls
    into a few tiles -- lists far longer than any earlier frame's.  The frame overflows its regions, draws nothing, and b32_frame_finish
    redraws it with larger regions: the redraw must use the placement the frame was enqueued with.  Then back again."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=100_000, width=640, height=480, bbox_px=200.0, seed=31)
    assert len(sc.faces) > 65536
    places = [b32.Placement(facing=0.1, world_pos=(100.0, -50.0, 200.0)), b32.Placement(facing=-0.4, world_pos=(2500.0, 900.0, 60000.0)),
              b32.Placement(facing=0.25, world_pos=(-200.0, 80.0, 500.0))]
    ctx = R.Context(0)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    redraws = []
    for n, pl in enumerate(places):
        ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
        rc, otm = oracle.render_mesh_15(ofb, pl.apply(sc.vertices), sc.faces, sc.textures, sc.camera, sc.settings)
        assert rc == 0 and otm.triangles_drawn > 10_000
        fb.clear(sc.clear_color)
        rs.render_async(sc.camera, sc.settings, placement=pl)
        tm = rs.finish()
        _assert_frame(fb, ofb.pixels, ofb.zbuffer, f"placement {n}")
        assert tm.triangles_drawn == otm.triangles_drawn
        rc_ = ctx.route_counts()
        redraws.append(rc_["redraw_region"] + rc_["redraw_global_sort"] + rc_["redraw_pairs"])
    assert redraws[1] > redraws[0], (redraws, ctx.route_counts())        # the far placement really overflowed what frame 0 had sized
    ctx.close()


def test_cpp_host_mirror_has_the_placed_calls():
    """host/rasterizer.hpp: Placement, place_vertex, MeshParams::placement and render_placed_async compile (header-only over the C ABI)."""
    import subprocess
    import tempfile
    hpp = os.path.join(ROOT, "bonnie-32_amd", "host")
    src = ('#include "rasterizer.hpp"\nint main(){ b32::Placement p = b32::Placement::from_facing(0.5f, b32::Vec3{ 1, 2, 3 }); b32::Vertex v; v.pos = { 1, 0, 0 };\n'
           ' b32::Vertex w = b32::place_vertex(v, p); b32::MeshParams m{ 0.3f, true, false, std::nullopt, p }; (void)&b32::render_placed_async; (void)&b32::render_frame;\n'
           ' b32::Placement q = b32::Placement::from_facing(0.00005f, b32::Vec3{ 0, 0, 0.0001f });\n'
           ' return (p.has_transform && !q.has_transform && m.placement.has_value() && w.pos.y == 2.0f) ? 0 : 1; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", hpp, "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.cpp")], check=True)
