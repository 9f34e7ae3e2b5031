"""What only shows ACROSS the four record producers -- b32_draw_world, b32_draw_gizmos, b32_draw_mesh_overlay, b32_draw_room_overlay, each
with its stage tap b32_*_project_batch -- which share one host path to the ordered tile pass (produce_draw / produce_tap, b32_api.hip).

Each producer's own records, routes, bands and argument errors are pinned by its own module (test_world, test_gizmos, test_mesh_overlay,
test_room_overlay).  Here: a draw equals its tap's records drawn (so the tap shows what the draw's kernel makes, whichever launch form
the batch size picks); an empty band skips the producer's kernel in every draw and in no tap; and six calls in a row that rebind the
shared device buffers (the primitive pass's record buffer, the overlays' staged list, the counters) equal their replay one step at a time.

How a tap's records are drawn: b32_draw_prims for the world items and both overlays (their records are plain primitives).  A gizmo batch
holds triangle records, which b32_draw_prims refuses and only the gizmo pass draws, so its records go through tests.test_gizmos.cpu_records
(np_prims for lines and circles, np_tri for triangles) on the CPU and the result is uploaded.

Every GPU test uses ONE 128 x 96 framebuffer, loaded with the same random pixels and random z-buffer before each side of a comparison."""
import functools

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi
from bonnie32_amd import rasterizer as RM
from tests.test_gizmos import G, K_LINE, K_LINE_DEPTH, K_POINT, K_THICK, K_TRI, K_TRI_VIEW, cam_point, cpu_records, frame_gizmos, ref_gizmos
from tests.test_lines import _upload_zbuffer
from tests.test_mesh_overlay import case_overlays
from tests.test_prims import random_prims
from tests.test_room_hover import random_room
from tests.test_room_overlay import wild_overlay
from tests.test_world import IDENTITY_CAM, np_world, random_items

f32 = np.float32
W, H = 128, 96
ZMAX = 3000.0
CAM = IDENTITY_CAM


@functools.lru_cache(maxsize=None)
def frame():
    """Random pixels (alpha 255) and a random z-buffer across the depths the fixtures use: part of every depth-tested batch is hidden."""
    rng = np.random.default_rng(9100)
    px = rng.integers(0, 256, W * H * 4, dtype=np.uint8)
    px[3::4] = 255
    return px, rng.uniform(0.3 * ZMAX, 1.1 * ZMAX, W * H).astype(f32)


# ---------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def cube():
    """8 vertices, 6 quads, before the camera: (positions, polygons)."""
    c = np.array(cam_point(CAM, 40.0, -30.0, 0.6 * ZMAX))
    pos = np.array([c + 420.0 * np.array([sx, sy, sz]) for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], f32)
    polys = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
    return pos, polys


@functools.lru_cache(maxsize=None)
def room3():
    """A 3 x 3-sector room with materials, its camera and an overlay with every section on and all four lists."""
    faces, grid, cam, _, _ = random_room(41, 3, 3)
    rng = np.random.default_rng(42)
    mats = np.zeros(len(faces), abi.FACE_MATERIAL_DTYPE)
    mats["split_direction"] = rng.integers(0, 2, len(faces))
    mats["flags"] = np.where(rng.random(len(faces)) < 0.4, abi.MAT_HAS_HEIGHTS_2, 0)
    mats["heights_2"] = faces["heights"] + rng.choice(np.array([0.0, 128.0, -256.0], f32), (len(faces), 4))
    return faces, mats, grid, cam, wild_overlay(faces, grid, cam, W, H, 2, 43)


def world_items(n):
    """n items from test_world's generator; the first one a line across the middle of the frame, so that a batch of one draws."""
    I = random_items(np.random.default_rng(9200 + n), n, CAM, spread=(0.5 * ZMAX, 0.4 * ZMAX), depth=(-0.1 * ZMAX, 1.2 * ZMAX), seg=0.15 * ZMAX)
    I[:1] = RM.world_item(abi.LINE_2D, cam_point(CAM, -300.0, -200.0, 0.5 * ZMAX), cam_point(CAM, 300.0, 250.0, 0.5 * ZMAX), b32.Color(250, 240, 10))
    return I


def gizmo_items(n):
    I = frame_gizmos(np.random.default_rng(9300 + n), n, CAM, ZMAX)
    I[:1] = G(K_LINE, cam_point(CAM, -300.0, 200.0, 0.5 * ZMAX), cam_point(CAM, 300.0, -250.0, 0.5 * ZMAX), rgb=(10, 250, 240))
    return I


def gizmo_expanding():
    """10 items of every kind whose records exceed 48: few enough for the kernel argument, 55 records -- the tile route.  The expansion
    comes from THICK_LINE_DEPTH items of the largest thickness the ABI takes, abi.GIZMO_MAX_THICKNESS = 16 (a thickness of 40 is refused
    with B32_E_ARG before anything runs), so three of them carry it instead of one."""
    p = lambda x, y, z: cam_point(CAM, x, y, z * ZMAX)
    T = abi.GIZMO_MAX_THICKNESS
    items = [G(K_TRI, p(-500, -400, 0.5), p(500, -300, 0.5), p(0, 450, 0.5), rgb=(30, 90, 200)),
             G(K_THICK, p(-600, 100, 0.2), p(600, -150, 0.25), rgb=(240, 30, 30), size=T),
             G(K_LINE, p(-700, -500, 0.4), p(700, 500, 0.4)), G(K_LINE_DEPTH, p(-700, 500, 0.2), p(700, -500, 0.9), rgb=(0, 255, 0)),
             G(K_POINT, p(200, 100, 0.3), size=7), G(K_TRI_VIEW, p(100, 100, 0.7), p(600, 200, 0.7), p(300, 500, 0.7), rgb=(200, 200, 0), blend=abi.ERASE),
             G(K_THICK, p(0, -600, 0.25), p(50, 600, 0.22), rgb=(9, 9, 9), size=T), G(K_POINT, p(-300, -100, 0.3), rgb=(255, 255, 255), size=3),
             G(K_THICK, p(-400, -500, 0.6), p(450, 480, 0.15), rgb=(90, 200, 90), size=T), G(K_LINE_DEPTH, p(-100, 0, 0.35), p(400, 30, 0.3), rgb=(255, 0, 255))]
    return np.concatenate(items)


class Producer:
    """One producer with its arguments bound: draw(fb), tap(fb) -> records, counts(fb) (None: it counts nothing), and replay(fb, recs):
    the records drawn over fb's current content (plain: b32_draw_prims; `model`: cpu_records over the frame read back, uploaded)."""

    def __init__(self, name, draw, tap, counts, model=False):
        self.name, self.draw, self.tap, self.counts, self.model = name, draw, tap, counts, model

    def replay(self, fb, recs):
        if not self.model:
            fb.draw_prims(recs)
            return
        px, zb = fb.pixels, fb.zbuffer
        cpu_records(px, zb, W, H, recs)
        fb.upload(px)

    def __repr__(self):
        return self.name


def producers(fb, res):
    """name -> Producer over the framebuffer's context; res: the resident cube (slot, topology) and room."""
    world_counts, gizmo_counts = (lambda fb: fb.world_counts()), (lambda fb: fb.gizmo_counts())
    out = {}
    for n in (1, 48, 49):
        I = world_items(n)
        out[f"world-{n}"] = Producer(f"world-{n}", lambda fb, I=I: fb.draw_world(I, CAM), lambda fb, I=I: fb.world_project_batch(I, CAM, None, W, H), world_counts)
    for name, I in [(f"gizmo-{n}", gizmo_items(n)) for n in (1, 48, 49)] + [("gizmo-expanding", gizmo_expanding())]:
        out[name] = Producer(name, lambda fb, I=I: fb.draw_gizmos(I, CAM), lambda fb, I=I: fb.ctx.gizmo_project_batch(I, CAM, None, W, H), gizmo_counts, model=True)
    ov, sel = mesh_overlay()
    out["mesh-overlay"] = Producer("mesh-overlay", lambda fb: fb.draw_mesh_overlay(res["slot"], res["top"], ov, CAM, None, sel),
                                   lambda fb: fb.mesh_overlay_project_batch(res["slot"], res["top"], ov, CAM, None, sel, W, H), None)
    _, _, _, rcam, rov = room3()
    out["room-overlay"] = Producer("room-overlay", lambda fb: fb.draw_room_overlay(res["room"], rov, rcam),
                                   lambda fb: fb.room_overlay_project_batch(res["room"], rov, rcam, W, H), gizmo_counts)
    return out


def mesh_overlay():
    """Every section on, a selected-polygon list (which goes through the context's pair list and the staged list)."""
    pos, polys = cube()
    ov, sel = case_overlays(polys, len(pos), (0.0, 0.0, 0.6 * W, float(H)))[-1]
    assert ov.sections == abi.OVERLAY_ALL and ov.select_kind == abi.SELECT_POLYGONS
    return ov, sel


CASES = ["world-1", "world-48", "world-49", "gizmo-1", "gizmo-48", "gizmo-49", "gizmo-expanding", "mesh-overlay", "room-overlay"]
ONE_EACH = ["world-49", "gizmo-expanding", "mesh-overlay", "room-overlay"]


# ---------------------------------------------------------------- without a GPU: the fixtures are not trivial
def test_fixtures_draw_and_cross_the_launch_forms():
    """The mirrors' records of every fixture change the frame; the expanding gizmo batch has at most 48 items and more than 48 records; the
    overlays have more than 48 records and only plain kinds."""
    px, zb = frame()

    def changes(recs):
        got = px.copy()
        cpu_records(got, zb, W, H, recs)
        return not np.array_equal(got, px)

    for n in (1, 48, 49):
        recs, counts = np_world(world_items(n), CAM, None, W, H)
        assert changes(recs) and counts[0] > 0, n
        recs, counts = ref_gizmos(gizmo_items(n), CAM, None, W, H)
        assert changes(recs) and counts[0] > 0, n
    I = gizmo_expanding()
    recs, counts = ref_gizmos(I, CAM, None, W, H)
    assert len(I) == 10 and sorted(set(I["kind"])) == list(range(6)) and len(recs) == 55 and changes(recs) and counts[0] >= 8
    assert I["size"][I["kind"] == K_THICK].max() <= abi.GIZMO_MAX_THICKNESS
    pos, polys = cube()
    ov, sel = mesh_overlay()
    top = RM.Topology.from_polygons(polys)
    recs = RM.mesh_overlay_records(pos, top, ov, sel, CAM, W, H)
    assert len(recs) > 48 and changes(recs) and recs["kind"].max() <= abi.PRIM_FILLED_RECT
    faces, mats, grid, cam, rov = room3()
    recs = RM.room_overlay_records(faces, grid, rov, cam, W, H, mats)
    assert len(recs) > 48 and changes(recs) and recs["kind"].max() <= abi.PRIM_FILLED_RECT
    assert len(rov.vertices) and len(rov.edges) and len(rov.faces) and len(rov.points)


# ================================================================== GPU
@pytest.fixture(scope="module")
def stage(gpu_ctx):
    """(framebuffer, producers) with the cube and the room resident."""
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(W, H, gpu_ctx)
    pos, polys = cube()
    v = b32.make_vertices(len(pos))
    v["pos"] = pos
    faces, mats, grid, _, _ = room3()
    res = {"slot": R.ResidentScene(fb, v, b32.make_faces(1), []).detach(), "top": R.Topology.from_polygons(polys), "room": R.Room(gpu_ctx, faces, grid)}
    res["room"].set_materials(mats)
    yield fb, producers(fb, res)
    fb.set_band(0, H)
    res["slot"].close(); res["top"].close(); res["room"].close()


def _load(fb):
    px, zb = frame()
    fb.upload(px)
    _upload_zbuffer(fb, zb)


def _read(fb):
    return fb.pixels, fb.zbuffer.view(np.uint32).copy()


def _all_counts(fb):
    return fb.world_counts() + fb.gizmo_counts()


def _delta(fb, before):
    return tuple(a - b for a, b in zip(_all_counts(fb), before))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_tap_equals_draw(stage, name):
    """draw_X against the records of X_project_batch drawn (module docstring: b32_draw_prims, for gizmos the CPU model): pixels and z-buffer
    byte for byte, and the same counter deltas -- with at least one pixel drawn and one counter moved."""
    fb, prods = stage
    p = prods[name]
    px, zb = frame()
    _load(fb)
    c0 = _all_counts(fb)
    p.draw(fb)
    drawn_px, drawn_z = _read(fb)
    d_draw = _delta(fb, c0)
    _load(fb)
    c0 = _all_counts(fb)
    recs = p.tap(fb)
    d_tap = _delta(fb, c0)
    p.replay(fb, recs)
    tap_px, tap_z = _read(fb)
    assert not np.array_equal(drawn_px, px), "the case draws nothing"
    assert np.array_equal(drawn_px, tap_px), f"{int((drawn_px != tap_px).sum())} bytes differ"
    assert np.array_equal(drawn_z, tap_z) and np.array_equal(drawn_z, zb.view(np.uint32))
    if p.counts is not None:
        assert d_draw == d_tap and any(d_draw), (d_draw, d_tap)
    else:
        assert d_draw == d_tap == (0,) * 6                      # (the mesh overlay counts nothing)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ONE_EACH)
def test_gpu_empty_band(stage, name):
    """With the band at rows 40..40 a draw returns without error and leaves pixels, z-buffer, counters and route counters as they were;
    the tap under the same band returns the full records and moves the counters as without a band."""
    fb, prods = stage
    p = prods[name]
    px, zb = frame()
    try:
        _load(fb)
        c0 = _all_counts(fb)
        full = p.tap(fb)
        d_full = _delta(fb, c0)
        fb.set_band(40, 40)
        r0, c0 = fb.ctx.route_counts(), _all_counts(fb)
        p.draw(fb)
        assert _delta(fb, c0) == (0,) * 6 and fb.ctx.route_counts() == r0
        got = p.tap(fb)
        assert len(got) == len(full) > 0 and got.tobytes() == full.tobytes()
        assert _delta(fb, c0) == d_full and (any(d_full) or p.counts is None)
        fb.set_band(0, H)
        got_px, got_z = _read(fb)
        assert np.array_equal(got_px, px) and np.array_equal(got_z, zb.view(np.uint32))
    finally:
        fb.set_band(0, H)


@pytest.mark.gpu
def test_gpu_shared_buffers_in_sequence(stage):
    """Gizmos (records > 48), the mesh overlay with a selected-polygon list, the room overlay with vertex, edge and face lists, 49 world
    items, b32_draw_prims of 60 plain records and the room overlay again, on one stream with no read in between: the frame and the counters
    equal the same six steps replayed from each step's tap records with the framebuffer read between the steps."""
    fb, prods = stage
    steps = [prods[n] for n in ("gizmo-expanding", "mesh-overlay", "room-overlay", "world-49")]
    plain = random_prims(np.random.default_rng(9400), 60, W, H, zrange=(0.0, 1.2 * ZMAX))
    _load(fb)
    c0 = _all_counts(fb)
    for p in steps:
        p.draw(fb)
    fb.draw_prims(plain)
    prods["room-overlay"].draw(fb)
    seq_px, seq_z = _read(fb)
    d_seq = _delta(fb, c0)
    _load(fb)
    c0 = _all_counts(fb)
    for p in steps:
        p.replay(fb, p.tap(fb))
        _read(fb)
    fb.draw_prims(plain)
    _read(fb)
    prods["room-overlay"].replay(fb, prods["room-overlay"].tap(fb))
    step_px, step_z = _read(fb)
    assert np.array_equal(seq_px, step_px), f"{int((seq_px != step_px).sum())} bytes differ"
    assert np.array_equal(seq_z, step_z)
    assert d_seq == _delta(fb, c0) and any(d_seq[:3]) and any(d_seq[3:])
