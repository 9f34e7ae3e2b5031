"""The world editor's object overlays through b32_draw_object_overlays, and a slot's bounds through b32_scene_bounds
(editor/viewport_3d.rs:255-291 draw_asset_wireframe, :7658-7697 draw_rotated_bounding_box; asset/asset.rs:288-312 Asset::bounds).

Nothing else in the repository draws these, so the expectation is built here:
  `ref_object_overlays`  a literal scalar restatement of the three functions over an asset's parts, every operand an np.float32: it records
                         the calls the reference makes (draw_3d_line_clipped, draw_3d_line) item by item in call order; the clipped lines go
                         through tests.test_world.ref_world, draw_3d_line through tests.test_gizmos.ref_gizmos.
The mirror (rasterizer.object_overlay_records, vectorised, written from the Rust text) and csrc/b32_object_overlay_body.h -- the device
code -- compiled for the host are compared with it record for record and place for place, no-ops included.  Every GPU frame is compared
byte for byte with a frame composed on the CPU: tests.test_prims.np_prims draws the restatement's records over the oracle's frame.

Two stated departures from the reference are part of the expectation: an index >= nv (a panic there) leaves the no-op and counts as
dropped; the bounds hold both zeros as +0.0 (test_the_sign_of_a_zero_bound_reaches_no_record shows no record can tell).

One case of the issue's list cannot exist: a box edge whose screen clip "fails to converge".  For a frame rectangle (xmin = ymin = 0,
width and height >= 1) clip_line_to_rect takes at most four of its sixteen rounds
(tests.test_gizmos.test_clip_rounds_never_run_out_on_a_frame), and a zero-size framebuffer is refused before anything is projected."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi
from bonnie32_amd import rasterizer as RM
from bonnie32_amd.mirrors import overlays as OV          # (the mirror's own module: where its private rules are read and changed)
from tests.test_gizmos import G, K_LINE, cam_point, ref_clip_line_to_rect, ref_gizmos
from tests.test_prims import np_prims
from tests.test_world import IDENTITY_CAM, _cam_f32, look_at, noop_records, ref_clip, ref_world, ref_world_to_screen

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
F32_MAX, F32_MIN = f32(np.finfo(f32).max), f32(np.finfo(f32).min)
OP, OI = RM.ObjectPart, RM.ObjectItem
WIRE, BOX_MESH, BOX = abi.OBJECT_WIRE, abi.OBJECT_BOX_MESH, abi.OBJECT_BOX
GREEN, CYAN, YELLOW, BLUE = b32.Color(100, 255, 100), b32.Color(100, 200, 255), b32.Color(255, 200, 50), b32.Color(100, 150, 255)


# ================================================================== the literal restatement
def ref_min(a, b):                                               # f32::min: a NaN is ignored; of two zeros the first operand stays
    return b if np.isnan(a) else (a if np.isnan(b) else (b if b < a else a))


def ref_max(a, b):
    return b if np.isnan(a) else (a if np.isnan(b) else (b if b > a else a))


def polygons_of(top):
    st = top.poly_start
    return [[int(i) for i in top.poly_verts[int(st[p]):int(st[p + 1])]] for p in range(top.np)]


def ref_bounds(parts, zero=f32(0.0)):
    """Asset::bounds, asset.rs:288-312: (min, max, has_verts) over ALL parts.  Rust leaves the sign of min(-0.0, +0.0) to the operand
    order; the library keeps one zero, +0.0: a zero bound comes back as `zero`."""
    mn = [F32_MAX, F32_MAX, F32_MAX]
    mx = [F32_MIN, F32_MIN, F32_MIN]
    has_verts = False
    for obj in parts:
        for v in obj.vertices:
            has_verts = True
            for c in range(3):
                mn[c] = ref_min(mn[c], f32(v[c]))
                mx[c] = ref_max(mx[c], f32(v[c]))
    fix = lambda x: zero if x == f32(0.0) else x
    return tuple(fix(x) for x in mn), tuple(fix(x) for x in mx), has_verts


def ref_place(v, cos_f, sin_f, world_pos):                       # viewport_3d.rs:276-285 and :7681-7685
    x, y, z = (f32(c) for c in v)
    return (x * cos_f - z * sin_f + world_pos[0], y + world_pos[1], x * sin_f + z * cos_f + world_pos[2])


def ref_box_calls(mn, mx, it):
    """draw_rotated_bounding_box, viewport_3d.rs:7658-7697: the twelve (p0, p1) of its draw_3d_line calls."""
    corners = [(mn[0], mn[1], mn[2]), (mx[0], mn[1], mn[2]), (mx[0], mn[1], mx[2]), (mn[0], mn[1], mx[2]),
               (mn[0], mx[1], mn[2]), (mx[0], mx[1], mn[2]), (mx[0], mx[1], mx[2]), (mn[0], mx[1], mx[2])]
    world_corners = [ref_place(c, it.cos_f, it.sin_f, it.world_pos) for c in corners]
    edges = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
    return [(world_corners[a], world_corners[b]) for a, b in edges]


def _ref_calls(parts, items, zero=f32(0.0)):
    """Per record place, in order: ("clipped", p0, p1, colour), ("line", p0, p1, colour) or None (no call of the reference), and the calls
    that count as dropped without a record of their own."""
    places, dropped = [], 0
    with np.errstate(all="ignore"):
        for it in items:
            mine = parts[it.first_part:it.first_part + it.n_parts]
            if it.kind == WIRE:                                  # :263-290
                for part in mine:
                    if not part.visible:
                        continue
                    verts = part.vertices
                    for indices in polygons_of(part.topology):
                        for i in range(len(indices)):
                            i0, i1 = indices[i], indices[(i + 1) % len(indices)]
                            if i0 >= len(verts) or i1 >= len(verts):         # (the reference panics: the no-op, dropped)
                                places.append(None); dropped += 1
                                continue
                            p0 = ref_place(verts[i0], it.cos_f, it.sin_f, it.world_pos)
                            p1 = ref_place(verts[i1], it.cos_f, it.sin_f, it.world_pos)
                            places.append(("clipped", p0, p1, it.color))
                continue
            if it.kind == BOX_MESH:                              # :4231-4237, :4255-4268
                mn, mx, has_verts = ref_bounds(mine, zero)
                if not has_verts:                                # bounds() is None
                    places += [None] * 12; dropped += 1
                    continue
            else:                                                # :4215-4224
                mn, mx = it.box
            places += [("line", p0, p1, it.color) for p0, p1 in ref_box_calls(mn, mx, it)]
    return places, dropped


def ref_object_overlays(parts, items, camera, w, h, zero=f32(0.0)):
    """(the abi.PRIM_DTYPE records place for place, (drawn, dropped, rejected), the calls)."""
    places, dropped = _ref_calls(parts, items, zero)
    out = noop_records(len(places))
    counts = [0, dropped, 0]
    for tag, kind, model in (("clipped", abi.LINE_2D, ref_world), ("line", abi.GIZMO_LINE, ref_gizmos)):
        where = [i for i, c in enumerate(places) if c is not None and c[0] == tag]
        if not where:
            continue
        I = np.zeros(len(where), abi.WORLD_ITEM_DTYPE if tag == "clipped" else abi.GIZMO_ITEM_DTYPE)
        for k, i in enumerate(where):
            _, p0, p1, col = places[i]
            I["p0"][k], I["p1"][k] = p0, p1
            I["r"][k], I["g"][k], I["b"][k], I["blend"][k] = col.r, col.g, col.b, col.blend
        I["kind"] = kind
        if tag == "clipped":
            I["alpha"], I["flags"] = 255, abi.WORLD_CLIP_NEAR
        recs, c = model(I, camera, None, w, h)
        out[where] = recs
        for k in range(3):
            counts[k] += c[k]
    return out, tuple(counts), places


# ================================================================== cases
def verts(pos):
    return np.ascontiguousarray(pos, f32).reshape(-1, 3)


CUBE_POS = verts([[sx * 50.0, sy * 50.0, sz * 50.0] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)])
CUBE_POLYS = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
ODD_POS = verts([[60.0 * np.cos(k * 0.7), 20.0 + 7.0 * k, 60.0 * np.sin(k * 0.7)] for k in range(10)])
ODD_POLYS = [[], [0], [1, 2], [3, 4, 5], [0, 1, 2, 3, 4, 5, 6, 7], [2, 99, 4]]
HIDDEN_POS = verts([[130.0, -75.0, 10.0], [-20.0, 160.0, -140.0]])
NEAR_CAM = look_at((20.0, 30.0, -30.0), (0.0, 0.0, 40.0))       # inside the cube: parts of the asset lie behind it
FAR_CAM = look_at((300.0, 200.0, -400.0), (0.0, 0.0, 0.0))
PLACEMENTS = {"identity": (1.0, 0.0, (0.0, 0.0, 0.0)), "rotation": (float(np.cos(f32(0.7))), float(np.sin(f32(0.7))), (30.0, -20.0, 60.0)),
              "negative zeros": (1.0, -0.0, (-0.0, 0.0, -0.0)), "infinite offset": (1.0, 0.0, (np.inf, 0.0, 0.0))}


def named_asset():
    """Three parts: a cube of 8 vertices and 6 quads (24 half-edges); polygons of 0, 1, 2, 3 and 8 positions and one index >= nv; a HIDDEN
    part whose vertices extend the bounds."""
    return [OP(None, RM.Topology.from_polygons(CUBE_POLYS), True, CUBE_POS), OP(None, RM.Topology.from_polygons(ODD_POLYS), True, ODD_POS),
            OP(None, None, False, HIDDEN_POS)]


def three_calls(place, n_parts=3):
    return [OI(WIRE, place, 0, n_parts, CYAN), OI(BOX_MESH, place, 0, n_parts, YELLOW),
            OI(BOX, place, 0, 0, BLUE, box=((-40.0, -10.0, -70.0), (45.0, 90.0, 35.0)))]


def bounds_parts():
    """name -> parts of one BOX_MESH item"""
    ramp = np.linspace(-30.0, 30.0, 70).astype(f32)
    first = verts(np.stack([ramp, ramp * f32(0.5), -ramp], axis=1)); first[0] = (-900.0, 800.0, 700.0)
    last = verts(np.stack([ramp, ramp * f32(0.5), -ramp], axis=1)); last[-1] = (950.0, -850.0, -750.0)
    return {"nv == 0 in every part": [OP(None, None, True, verts([])), OP(None, None, False, verts([]))],
            "one vertex": [OP(None, None, True, verts([[12.5, -3.0, 40.0]]))],
            "only NaN vertices": [OP(None, None, True, verts([[np.nan] * 3] * 5))],
            "infinities": [OP(None, None, True, verts([[np.inf, -np.inf, 3.0], [-2.0, 5.0, np.inf], [1.0, np.nan, -4.0]]))],
            "only +inf": [OP(None, None, True, verts([[np.inf] * 3] * 2))],
            "the extreme at the first index": [OP(None, None, True, first)], "the extreme at the last index": [OP(None, None, True, last)],
            "zeros of both signs": [OP(None, None, True, verts([[-0.0, 0.0, -0.0], [0.0, -0.0, -5.0]]))]}


def random_asset(seed, n_parts=4, fine=False):
    """Parts of random polygons (0 .. 8 positions, a few indices out of range) over random vertices (a NaN, an infinity), some hidden."""
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(n_parts):
        nv = int(rng.integers(3, 60))
        pos = (rng.normal(size=(nv, 3)) * (90.0, 70.0, 110.0) + (3.0, 11.0, 37.0)).astype(f32)
        if not fine:
            pos[rng.integers(0, nv)][0] = np.nan; pos[rng.integers(0, nv)][2] = np.inf
        polys = [[int(rng.integers(0, nv + (0 if fine or rng.random() < 0.9 else 3))) for _ in range(int(rng.choice([0, 1, 2, 3, 3, 4, 4, 5, 8])))] for _ in range(int(rng.integers(1, 40)))]
        visible = bool(rng.random() < 0.75) or k == 0
        parts.append(OP(None, RM.Topology.from_polygons(polys), visible, pos))
    return parts


def random_items(seed, n_parts):
    rng = np.random.default_rng(seed + 500)
    items = []
    for _ in range(6):
        a = f32(rng.uniform(-3.2, 3.2))
        place = (float(np.cos(a)), float(np.sin(a)), tuple(float(v) for v in rng.normal(size=3) * (150.0, 60.0, 150.0)))
        first = int(rng.integers(0, n_parts)); n = int(rng.integers(0, n_parts - first + 1))
        kind = int(rng.integers(0, 3))
        lo, hi = rng.normal(size=3) * 80.0, rng.normal(size=3) * 80.0
        items.append(OI(kind, place, first, n, b32.Color(*[int(v) for v in rng.integers(0, 256, 3)]), box=(lo, hi)))
    return items


def named_cases():
    """(name, parts, items, camera, w, h)"""
    out = []
    asset = named_asset()
    for name, place in PLACEMENTS.items():
        out.append((f"asset, {name}, near camera", asset, three_calls(place), NEAR_CAM, 64, 48))
    out.append(("asset, rotation, far camera", asset, three_calls(PLACEMENTS["rotation"]), FAR_CAM, 64, 48))
    out.append(("asset, identity camera", asset, three_calls((1.0, 0.0, (5.0, -30.0, 20.0))), IDENTITY_CAM, 64, 48))
    for name, parts in bounds_parts().items():
        out.append((name, parts, [OI(BOX_MESH, PLACEMENTS["rotation"], 0, len(parts), YELLOW)], FAR_CAM, 64, 48))
    # render_asset_parts skips the transform when neither facing nor position exceeds 0.0001 (has_transform, scene.rs:125); these loops
    # have no such shortcut.  At the exact identity no record can tell (x * 1.0 - z * 0.0 + 0.0 is x, and what an infinity makes of it ends
    # as NaN either way), so the case is a facing of 0.0001 over a deep mesh in the largest frame the tap takes: 2.4 pixels.
    deep = [OP(None, RM.Topology.from_polygons([[0, 1, 2]]), True, verts([[0.0, 0.0, 40000.0], [900.0, 500.0, 40000.0], [0.0, 1000.0, 39000.0]]))]
    tiny = (float(np.cos(f32(0.0001))), float(np.sin(f32(0.0001))), (0.0, 0.0, 0.0))
    out.append(("a facing inside the has_transform threshold", deep, [OI(WIRE, tiny, 0, 1, GREEN), OI(BOX_MESH, tiny, 0, 1, YELLOW)], IDENTITY_CAM, 16384, 16384))
    out.append(("a box with min > max", asset, [OI(BOX, PLACEMENTS["rotation"], 0, 0, BLUE, box=((40.0, 40.0, 40.0), (-40.0, -45.0, -50.0)))], FAR_CAM, 64, 48))
    out.append(("the same slot in two items", asset, [OI(WIRE, PLACEMENTS["identity"], 0, 1, GREEN), OI(BOX_MESH, PLACEMENTS["identity"], 0, 1, YELLOW),
                                                      OI(WIRE, PLACEMENTS["rotation"], 0, 2, CYAN), OI(BOX_MESH, PLACEMENTS["rotation"], 0, 3, YELLOW)], FAR_CAM, 64, 48))
    out.append(("a wire item all of whose parts are hidden", asset, [OI(WIRE, PLACEMENTS["identity"], 2, 1, GREEN), OI(BOX_MESH, PLACEMENTS["identity"], 2, 1, YELLOW),
                                                                     OI(WIRE, PLACEMENTS["identity"], 1, 0, GREEN)], FAR_CAM, 64, 48))
    for seed in (11, 12, 13):
        parts = random_asset(seed)
        out.append((f"random asset {seed}", parts, random_items(seed, len(parts)), look_at((30.0, 60.0, -250.0), (0.0, 10.0, 40.0)), 64 if seed != 13 else 320, 48 if seed != 13 else 240))
    return out


@functools.lru_cache(maxsize=None)
def answers():
    """[(case, the restatement's (records, counts, calls))]: computed once, shared by the CPU and the GPU tests."""
    return [(c, ref_object_overlays(c[1], c[2], c[3], c[4], c[5])) for c in named_cases()]


def answer(name):
    return next((c, a) for c, a in answers() if c[0] == name)


# ================================================================== the device header compiled for the host
HOST_FLAGS = {"off": ["-O1", "-ffp-contract=off"], "fused": ["-O2", "-ffp-contract=fast", "-mfma"],
              "sanitized": ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@functools.lru_cache(maxsize=None)
def _host_dir():
    d = tempfile.mkdtemp(prefix="b32_object_overlay_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def host_exe(mode):
    exe = os.path.join(_host_dir(), "object_overlay_host_" + mode)
    subprocess.run(["g++", "-std=c++17"] + HOST_FLAGS[mode] + ["-I", os.path.join(ROOT, "bonnie-32_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "object_overlay_host.cpp"), "-o", exe], check=True)
    return exe


_host_calls = [0]


def host_overlay(parts, items, cam, w, h, mode="off", stride=3, part_heads=None, raw_items=None):
    """tests/cpp/object_overlay_host.cpp on one case: (rc, records, counts, rows, groups, the parts' 32 bytes of bounds).  part_heads: per
    part a dict that overrides flags / pad / slot (0 NULL, 1 holds, 2 does not) / has_topology; raw_items: the abi.OBJECT_ITEM_DTYPE
    array as it travels (padding and kinds included)."""
    _host_calls[0] += 1
    base = os.path.join(_host_dir(), f"case{_host_calls[0]}")
    I = RM.pack_object_items(items) if raw_items is None else np.ascontiguousarray(raw_items, abi.OBJECT_ITEM_DTYPE)
    with open(base + ".in", "wb") as fh:
        fh.write(np.array([w, h, len(parts), len(I)], np.uint32).tobytes())
        c = cam.pack()
        fh.write(np.array(list(c.position) + list(c.basis_x) + list(c.basis_y) + list(c.basis_z), f32).tobytes())
        for k, p in enumerate(parts):
            hd = dict(flags=0 if p.visible else abi.OBJECT_PART_HIDDEN, pad=0, slot=1, has_topology=int(p.topology is not None))
            hd.update((part_heads or {}).get(k, {}))
            nh = len(p.topology.poly_verts) if p.topology is not None else 0
            fh.write(np.array([hd["flags"], hd["pad"], hd["slot"], hd["has_topology"], nh, len(p.vertices), stride], np.uint32).tobytes())
            if nh:
                fh.write(np.stack([p.topology.he_v0, p.topology.he_v1], axis=1).astype(np.uint32).tobytes())
            wide = np.full((len(p.vertices), stride), 7.5, f32)      # (what stands behind a position in a B32Vertex is never read)
            wide[:, :3] = p.vertices
            fh.write(wide.tobytes())
        fh.write(I.tobytes())
    r = subprocess.run([host_exe(mode), base + ".in", base + ".out"], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    blob = open(base + ".out", "rb").read()
    os.remove(base + ".in"); os.remove(base + ".out")
    rc, rows = int(np.frombuffer(blob[:4], np.int32)[0]), int(np.frombuffer(blob[4:8], np.uint32)[0])
    total, groups = (int(v) for v in np.frombuffer(blob[8:24], np.uint64))
    if rc:
        return rc, None, None, rows, groups, None
    counts = tuple(int(v) for v in np.frombuffer(blob[24:48], np.uint64))
    bounds = np.frombuffer(blob[48:48 + 32 * len(parts)], abi.SCENE_BOUNDS_DTYPE)
    recs = np.frombuffer(blob[48 + 32 * len(parts):], abi.PRIM_DTYPE)
    assert len(recs) == total
    return rc, recs, counts, rows, groups, bounds


def same_bits(a, b):
    return np.asarray(a, f32).tobytes() == np.asarray(b, f32).tobytes()


# ================================================================== CPU
def test_restatement_hand_cases():
    """The restatement pinned by hand: the bounds' start values and NaN rule, where the identity camera puts a placed cube corner, the
    closing edge, the places of the no-ops, the box's edge order."""
    with np.errstate(all="ignore"):
        B = bounds_parts()
        assert ref_bounds(B["nv == 0 in every part"]) == ((F32_MAX,) * 3, (F32_MIN,) * 3, False)
        mn, mx, has = ref_bounds(B["only NaN vertices"])
        assert has and mn == (F32_MAX,) * 3 and mx == (F32_MIN,) * 3
        mn, mx, _ = ref_bounds(B["only +inf"])
        assert mn == (F32_MAX,) * 3 and mx == (f32(np.inf),) * 3                     # min starts at f32::MAX, not at +inf
        mn, mx, _ = ref_bounds(B["infinities"])
        assert mn == (f32(-2.0), f32(-np.inf), f32(-4.0)) and mx == (f32(np.inf), f32(5.0), f32(np.inf))
        assert ref_bounds(B["the extreme at the first index"])[0][0] == f32(-900.0) and ref_bounds(B["the extreme at the last index"])[1][0] == f32(950.0)
        mn, mx, _ = ref_bounds(named_asset())
        assert mn[1:] == (f32(-75.0), f32(-140.0)) and mx[:2] == (f32(130.0), f32(160.0))             # the hidden part extends them
        assert ref_bounds(named_asset()[:2])[0][1:] == (f32(-50.0), f32(ODD_POS[:, 2].min()))
    (_, parts, items, cam, w, h), (recs, counts, places) = answer("asset, identity camera")
    assert len(places) == (24 + 0 + 1 + 2 + 3 + 8 + 3) + 12 + 12
    # cube corner 4 (-50, -50, 50) -> (-45, -80, 70): sx = -45 * 4 / 75 * 18 + 32, sy = -80 * 4 / 75 * 18 + 24
    p = places[8][1]                                             # polygon 2 = [0, 4, 5, 1]: its first half-edge is (0, 4)
    assert tuple(float(v) for v in places[9][1]) == (-45.0, -80.0, 70.0) and tuple(float(v) for v in p) == (-45.0, -80.0, -30.0)
    r = recs[9]                                                  # (4, 5): both ends in front
    assert (int(r["x0"]), int(r["y0"]), int(r["x1"]), int(r["y1"])) == (int(f32(-45.0) * f32(4.0) / f32(75.0) * f32(18.0) + f32(32.0)), int(f32(-80.0) * f32(4.0) / f32(75.0) * f32(18.0) + f32(24.0)),
                                                                       int(f32(55.0) * f32(4.0) / f32(75.0) * f32(18.0) + f32(32.0)), int(f32(-80.0) * f32(4.0) / f32(75.0) * f32(18.0) + f32(24.0)))
    assert int(r["alpha"]) == 255 and (int(r["r"]), int(r["g"]), int(r["b"])) == (100, 200, 255)
    # the one-position polygon [0] is the edge (0, 0); the two-position one gives (1, 2) and (2, 1); the closing edge of the triangle is (5, 3)
    odd = places[24:24 + 17]
    same = lambda a, b: all(float(x) == float(y) for x, y in zip(a, b))
    assert same(odd[0][1], odd[0][2]) and same(odd[1][1], odd[2][2]) and same(odd[1][2], odd[2][1]) and same(odd[5][2], odd[3][1])
    assert odd[14] is None and odd[15] is None and odd[16] is not None               # (2, 99), (99, 4), (4, 2)
    box = places[24 + 17 + 12:]
    assert [tuple(float(v) for v in c[1]) for c in box[:2]] == [(-35.0, -40.0, -50.0), (50.0, -40.0, -50.0)]       # edges (0, 1), (1, 2) of the explicit box
    assert tuple(float(v) for v in box[8][2]) == (-35.0, 60.0, -50.0)                                              # the first vertical: corner 0 -> corner 4


def test_named_cases_exercise_what_the_issue_lists():
    """Counted from the restatement's calls, never from the code under test: half-edges that cross the near plane with the first and with
    the second end, some wholly behind it, box edges shortened by the screen clip."""
    (_, parts, items, cam, w, h), (recs, counts, places) = answer("asset, identity, near camera")
    camf = _cam_f32(cam)
    first = second = behind = shortened = 0
    with np.errstate(all="ignore"):
        for c in places:
            if c is None:
                continue
            p0, p1 = (tuple(f32(v) for v in q) for q in c[1:3])
            z0, z1 = (sum((q[k] - camf[0][k]) * camf[3][k] for k in range(3)) for q in (p0, p1))
            cl = ref_clip(p0, p1, camf)
            if c[0] == "clipped":
                behind += cl is None
                first += cl is not None and z0 <= f32(0.1)
                second += cl is not None and z1 <= f32(0.1)
            elif cl is not None:
                ends = [ref_world_to_screen(q, camf, w, h) for q in cl]
                if all(e is not None for e in ends):
                    sc = ref_clip_line_to_rect(ends[0][0], ends[0][1], ends[1][0], ends[1][1], f32(0), f32(0), f32(w), f32(h))
                    shortened += sc is not None and sc[4] > 0
    census = (int(first), int(second), int(behind), int(shortened), counts)
    assert first >= 1 and second >= 1 and behind >= 1 and shortened >= 1 and counts[0] >= 20 and counts[1] >= 3, census
    assert census == NEAR_CENSUS, census
    # an infinite offset: every call is made, none draws
    (_, _, _, _, _, _), (recs, counts, places) = answer("asset, infinite offset, near camera")
    assert counts[0] == 0 and counts[1] + counts[2] == len([c for c in places if c is not None]) + 2


# (half-edges clipped at their first end, at their second end, wholly behind the near plane, box edges shortened by the screen clip,
#  (drawn, dropped, rejected)) of "asset, identity, near camera", from the restatement
NEAR_CENSUS = (5, 5, 3, 3, (34, 31, 0))


def test_mirror_and_host_header_equal_the_restatement():
    """rasterizer.object_overlay_records and csrc/b32_object_overlay_body.h built for the host (g++ -O1 -ffp-contract=off) equal
    ref_object_overlays record for record and place for place, no-ops included; so do the drawn / dropped / rejected counts, the record
    count, and each part's bounds against mesh_bounds and the restatement, bit for bit.  Both vertex strides give the same records."""
    n_drawn = 0
    for (name, parts, items, cam, w, h), (want, counts, _) in answers():
        mirror, mcounts = RM.object_overlay_records(parts, items, cam, w, h, with_counts=True)
        assert len(mirror) == len(want) == RM.object_overlay_record_count(parts, items), name
        bad = np.nonzero(mirror != want)[0]
        assert not len(bad), f"{name} (mirror): place {bad[0]}: {mirror[bad[0]]} != {want[bad[0]]}"
        assert mcounts == counts, (name, mcounts, counts)
        for stride in (3, 9):
            rc, recs, hcounts, rows, groups, bounds = host_overlay(parts, items, cam, w, h, stride=stride)
            assert rc == 0 and recs.tobytes() == want.tobytes(), f"{name} (header, stride {stride}): places {np.nonzero(recs != want)[0][:8]} differ"
            assert hcounts == counts, (name, hcounts, counts)
        for k, p in enumerate(parts):
            mn, mx, has = RM.mesh_bounds([p.vertices])
            with np.errstate(all="ignore"):
                rmn, rmx, rhas = ref_bounds([p])
            assert same_bits(mn, rmn) and same_bits(mx, rmx) and has == rhas, (name, k)
            assert same_bits(bounds[k]["min"], mn) and same_bits(bounds[k]["max"], mx) and bool(bounds[k]["has_verts"]) == has, (name, k)
        n_drawn += int(((want["kind"] != abi.PRIM_CIRCLE)).sum())
    assert n_drawn > 400


def test_rows_cross_the_workgroup_boundary_on_the_host():
    """One polygon of 257 positions and one of 513 with an empty part between them: rows of 2 and 3 workgroups, none for the empty part."""
    parts, items = long_polygon_case()
    want, counts, _ = ref_object_overlays(parts, items, FAR_CAM, 64, 48)
    rc, recs, hcounts, rows, groups, _ = host_overlay(parts, items, FAR_CAM, 64, 48)
    assert rc == 0 and rows == 3 and groups == 2 + 3 + 1 and len(recs) == 257 + 513 + 12
    assert recs.tobytes() == want.tobytes() and hcounts == counts
    assert RM.object_overlay_records(parts, items, FAR_CAM, 64, 48).tobytes() == want.tobytes()


def long_polygon_case():
    ring = lambda n, r: verts([[r * np.cos(2 * np.pi * k / n), 15.0 * np.sin(9 * np.pi * k / n), r * np.sin(2 * np.pi * k / n)] for k in range(n)])
    parts = [OP(None, RM.Topology.from_polygons([list(range(257))]), True, ring(257, 120.0)), OP(None, RM.Topology.from_polygons([[], []]), True, verts([[1.0, 2.0, 3.0]])),
             OP(None, RM.Topology.from_polygons([list(range(513))]), True, ring(513, 80.0))]
    return parts, [OI(WIRE, PLACEMENTS["rotation"], 0, 3, GREEN), OI(BOX_MESH, PLACEMENTS["rotation"], 0, 3, YELLOW)]


# (seed of random_asset(.., fine=True), facing, world position, camera position): inputs at which a build of the device header with fused
# multiply-adds makes other records than the separately rounded one (found by a search over random placements and kept as data)
FUSED_INPUTS = ((691, 0.307, (796.34, -128.68, 198.51), (760.48, -171.22, 465.1)), (6643, -2.358, (-361.31, -95.63, 211.62), (-349.38, -61.48, 368.89)),
                (8638, 1.694, (107.52, -2.54, -74.84), (13.91, -48.81, -5.08)))


def fused_case(seed, facing, pos, cam_pos):
    parts = random_asset(seed, 6, fine=True)
    a = f32(facing)
    place = (float(np.cos(a)), float(np.sin(a)), pos)
    return parts, [OI(WIRE, place, 0, len(parts), CYAN), OI(BOX_MESH, place, 0, len(parts), YELLOW)], look_at(cam_pos, pos), 640, 480


def test_a_fused_evaluation_differs():
    """The same program built with FMA contraction (g++ -O2 -ffp-contract=fast -mfma) differs from the restatement on committed inputs
    (the placement's x * cos - z * sin contracts): nothing contracted can pass the comparisons of this file."""
    assert FUSED_INPUTS
    n = 0
    for args in FUSED_INPUTS:
        parts, items, cam, w, h = fused_case(*args)
        want, _, _ = ref_object_overlays(parts, items, cam, w, h)
        assert host_overlay(parts, items, cam, w, h, "off")[1].tobytes() == want.tobytes()
        n += int((host_overlay(parts, items, cam, w, h, "fused")[1] != want).sum())
    assert n >= 1


def test_the_sign_of_a_zero_bound_reaches_no_record():
    """Rust leaves the sign of min(-0.0, +0.0) to the operand order and the library keeps +0.0.  With the minima and maxima taking -0.0
    and taking +0.0, at a zero camera position and a zero placement (where nothing else is added to the zero), the 12 records are equal."""
    parts = bounds_parts()["zeros of both signs"] + [OP(None, None, True, verts([[0.0, 3.0, 9.0], [-0.0, -0.0, 2.0]]))]
    items = [OI(BOX_MESH, PLACEMENTS["identity"], 0, 2, YELLOW)]
    with np.errstate(all="ignore"):
        neg, pos = ref_bounds(parts, f32(-0.0)), ref_bounds(parts, f32(0.0))
    assert any(np.signbit(v) for v in neg[0] + neg[1]) and not any(np.signbit(v) and v == 0 for v in pos[0] + pos[1])
    for cam in (IDENTITY_CAM, b32.Camera(position=(0.0, 0.0, 0.0), basis_x=(0.8, 0.0, -0.6), basis_y=(0.0, 1.0, 0.0), basis_z=(0.6, 0.0, 0.8))):
        a, ca, _ = ref_object_overlays(parts, items, cam, 64, 48, zero=f32(-0.0))
        b, cb, _ = ref_object_overlays(parts, items, cam, 64, 48, zero=f32(0.0))
        assert len(a) == 12 and a.tobytes() == b.tobytes() and ca == cb and ca[0] >= 1
        assert RM.object_overlay_records(parts, items, cam, 64, 48).tobytes() == b.tobytes()


def _mutations(mp):
    """name -> (apply(monkeypatch), the named case it must change)"""
    def visible_only(parts):
        return [p for p in parts if p.visible]

    def open_loops(top):                                         # indices[i + 1] without the `% len`: the closing edge is gone
        v1 = top.he_v1.copy()
        last = np.cumsum(top.count)[top.count > 0] - 1
        v1[last] = NONE
        return top.he_v0, v1

    def skip_at_identity(P, cos_f, sin_f, world_pos):
        if abs(sin_f) <= 0.0001 and all(abs(v) <= 0.0001 for v in world_pos):     # (has_transform, scene.rs:125: not in these loops)
            return P
        return ORIGINAL["place"](P, cos_f, sin_f, world_pos)

    def other_sign(P, cos_f, sin_f, world_pos):
        return ORIGINAL["place"](P, cos_f, -sin_f, world_pos)

    edges = list(OV._OBJECT_BOX_EDGES)
    edges[3], edges[4] = edges[4], edges[3]
    inf = f32(np.inf)
    return {"bounds over visible parts only": (lambda: mp.setattr(OV, "_object_bounds_parts", visible_only), "asset, rotation, far camera"),
            "start values +-inf": (lambda: mp.setattr(OV, "_OBJECT_BOUNDS_START", (inf, -inf)), "only NaN vertices"),
            "(i + 1) % n dropped for the closing edge": (lambda: mp.setattr(OV, "_object_half_edges", open_loops), "asset, rotation, far camera"),
            "box edge order": (lambda: mp.setattr(OV, "_OBJECT_BOX_EDGES", tuple(edges)), "a box with min > max"),
            "placement skipped at identity": (lambda: mp.setattr(OV, "_object_place", skip_at_identity), "a facing inside the has_transform threshold"),
            "rotation sign": (lambda: mp.setattr(OV, "_object_place", other_sign), "asset, rotation, far camera"),
            "wire through draw_3d_line": (lambda: mp.setattr(OV, "_object_wire_lines", OV._np_draw_3d_lines), "asset, identity, near camera")}


ORIGINAL = {"place": OV._object_place}
MUTATIONS = ("bounds over visible parts only", "start values +-inf", "(i + 1) % n dropped for the closing edge", "box edge order",
             "placement skipped at identity", "rotation sign", "wire through draw_3d_line")


@pytest.mark.parametrize("mut", MUTATIONS)
def test_one_point_mutations_of_the_mirror_change_a_named_case(monkeypatch, mut):
    """Each one-point change of the mirror makes other records (or other counts) on the named case it is aimed at: the comparison with the
    restatement would catch it."""
    apply, name = _mutations(monkeypatch)[mut]
    (_, parts, items, cam, w, h), (want, counts, _) = answer(name)
    assert RM.object_overlay_records(parts, items, cam, w, h).tobytes() == want.tobytes()
    apply()
    got, gcounts = RM.object_overlay_records(parts, items, cam, w, h, with_counts=True)
    changed = int((got != want).sum()) if len(got) == len(want) else -1
    print(f"mutation {mut!r} on {name!r}: {changed} records change, counts {gcounts} against {counts}")
    assert changed != 0 or gcounts != counts


def test_argument_rules_on_the_host_and_in_the_mirror():
    """The plan refuses what the library refuses (B32_E_ARG): a part range outside the table, a visible part of a WIRE item without a
    topology, a NULL slot or one that does not hold its scene, an unknown kind or flag, non-zero padding; past 2^31 - 1 records it is
    B32_E_UNSUPPORTED.  A hidden part without a topology, a BOX whose range is empty and n_items == 0 are fine."""
    asset = named_asset()
    ok = three_calls(PLACEMENTS["identity"])
    E = abi.B32_E_ARG
    run = lambda items=ok, parts=asset, **kw: host_overlay(parts, items, FAR_CAM, 64, 48, "sanitized", **kw)[0]
    assert run() == 0 and run(items=[]) == 0 and run(items=[OI(BOX, PLACEMENTS["identity"], 3, 0, BLUE)]) == 0
    assert run(items=[OI(WIRE, PLACEMENTS["identity"], 2, 2, GREEN)]) == E and run(items=[OI(BOX_MESH, PLACEMENTS["identity"], 4, 0, GREEN)]) == E
    assert run(items=[OI(BOX, PLACEMENTS["identity"], 0xFFFFFFFF, 2, GREEN)]) == E
    assert run(part_heads={0: dict(has_topology=0)}) == E                           # visible, WIRE, no topology
    assert run(part_heads={2: dict(has_topology=0)}) == 0                           # hidden: none needed
    assert run(part_heads={1: dict(slot=0)}) == E and run(part_heads={1: dict(slot=2)}) == E
    assert run(part_heads={1: dict(flags=2)}) == E and run(part_heads={1: dict(flags=3)}) == E and run(part_heads={2: dict(pad=1)}) == E
    raw = RM.pack_object_items(ok)
    for field, value in (("kind", 3), ("kind", 255)):
        bad = raw.copy(); bad[field][1] = value
        assert run(raw_items=bad) == E
    for k in range(3):
        bad = raw.copy(); bad["_pad"][2][k] = 1
        assert run(raw_items=bad) == E
    with pytest.raises(ValueError):
        RM.object_overlay_record_count(asset, [OI(WIRE, PLACEMENTS["identity"], 2, 2, GREEN)])
    with pytest.raises(ValueError):
        RM.object_overlay_record_count([OP(None, None, True, CUBE_POS)], [OI(WIRE, PLACEMENTS["identity"], 0, 1, GREEN)])
    with pytest.raises(ValueError):
        RM.object_overlay_record_count(asset, [OI(3, PLACEMENTS["identity"], 0, 1, GREEN)])
    # 21 000 wire items over a table of 200 parts of 513 half-edges each: past 2^31 - 1 records before a vertex is read
    ring = long_polygon_case()[0][2]
    many = np.repeat(RM.pack_object_items([OI(WIRE, PLACEMENTS["identity"], 0, 200, GREEN)]), 21_000)
    assert 21_000 * 200 * 513 > 0x7FFFFFFF and run(parts=[ring] * 200, raw_items=many) == abi.B32_E_UNSUPPORTED


def test_host_program_under_the_sanitizers():
    """The stand-alone program once more with -fsanitize=address,undefined, run directly: it ends clean and gives the same records."""
    names = ("asset, identity, near camera", "asset, infinite offset, near camera", "nv == 0 in every part", "only NaN vertices", "the same slot in two items",
             "a wire item all of whose parts are hidden", "random asset 11")
    for name in names:
        (_, parts, items, cam, w, h), (want, counts, _) = answer(name)
        rc, recs, hcounts, _, _, _ = host_overlay(parts, items, cam, w, h, "sanitized", stride=9)
        assert rc == 0 and recs.tobytes() == want.tobytes() and hcounts == counts, name
    parts, items = long_polygon_case()
    assert host_overlay(parts, items, FAR_CAM, 64, 48, "sanitized")[1].tobytes() == host_overlay(parts, items, FAR_CAM, 64, 48)[1].tobytes()


def test_layout_and_pod_layout_match_c():
    """B32ObjectPart is 24 bytes and B32ObjectItem 60 with the fields where the C header puts them (compiled with gcc and g++); the kinds
    and the flag match; the record count follows the topologies and the kinds alone."""
    fields = ("place", "first_part", "n_parts", "box_min", "box_max", "r", "blend", "kind", "_pad")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void) { printf("%zu %zu %zu %zu", sizeof(B32ObjectPart), offsetof(B32ObjectPart, topology), '
           'offsetof(B32ObjectPart, flags), sizeof(B32ObjectItem));' + "".join(f' printf(" %zu", offsetof(B32ObjectItem, {f}));' for f in fields)
           + ' printf(" %u %u %u %u\\n", B32_OBJECT_PART_HIDDEN, B32_OBJECT_WIRE, B32_OBJECT_BOX_MESH, B32_OBJECT_BOX); return 0; }\n')
    D = abi.OBJECT_ITEM_DTYPE
    want = [24, abi.OBJECT_PART_DTYPE.fields["topology"][1], abi.OBJECT_PART_DTYPE.fields["flags"][1], 60, 0] + [D.fields[f][1] for f in fields[1:]] + [1, 0, 1, 2]
    with tempfile.TemporaryDirectory() as d:
        for cc, ext in (("gcc", "c"), ("g++", "cpp")):
            open(os.path.join(d, "t." + ext), "w").write(src)
            subprocess.run([cc, "-I", os.path.join(ROOT, "include"), os.path.join(d, "t." + ext), "-o", os.path.join(d, "t")], check=True)
            out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
            assert [int(x) for x in out] == want, cc
    assert (abi.OBJECT_PART_HIDDEN, abi.OBJECT_WIRE, abi.OBJECT_BOX_MESH, abi.OBJECT_BOX) == (1, 0, 1, 2)
    asset = named_asset()
    assert RM.object_overlay_record_count(asset, three_calls(PLACEMENTS["identity"])) == (24 + 17) + 12 + 12
    assert RM.object_overlay_record_count(asset, three_calls(PLACEMENTS["identity"], 1)) == 24 + 12 + 12
    assert RM.object_overlay_record_count(asset, [OI(WIRE, PLACEMENTS["identity"], 2, 1, GREEN)]) == 0
    # the camera and the placement never move a record: the same places under another camera
    a = RM.object_overlay_records(asset, three_calls(PLACEMENTS["identity"]), FAR_CAM, 64, 48)
    b = RM.object_overlay_records(asset, three_calls(PLACEMENTS["rotation"]), NEAR_CAM, 64, 48)
    assert len(a) == len(b) and not np.array_equal(a, b)


def test_cpp_mirror_object_overlays_compile():
    """host/rasterizer.hpp: b32::ObjectPart, b32::ObjectItem, b32::draw_object_overlays and b32::ResidentMesh::bounds compile (header-only
    over the C ABI)."""
    hpp_dir = os.path.join(ROOT, "bonnie-32_amd", "host")
    src = ('#include "rasterizer.hpp"\nvoid f(b32::Framebuffer& fb, const b32::ResidentMesh& m, const b32::Topology& t, const b32::Camera& cam) {\n'
           ' std::vector<b32::ObjectPart> parts{ { &m, &t, true }, { &m, nullptr, false } };\n'
           ' b32::ObjectItem wire; wire.kind = B32_OBJECT_WIRE; wire.place = b32::Placement::from_facing(0.5f, { 1.0f, 2.0f, 3.0f }); wire.n_parts = 2; wire.color = { 100, 200, 255 };\n'
           ' b32::ObjectItem box = wire; box.kind = B32_OBJECT_BOX_MESH; b32::ObjectItem given = wire; given.kind = B32_OBJECT_BOX; given.box_min = { -1, -2, -3 }; given.box_max = { 1, 2, 3 };\n'
           ' b32::draw_object_overlays(fb, parts, { wire, box, given }, cam);\n'
           ' b32::Vec3 mn, mx; (void)m.bounds(mn, mx); (void)sizeof(B32ObjectItem); (void)parts[0].pack().flags; }\n'
           'int main() { (void)&f; return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", hpp_dir, "-I", os.path.join(ROOT, "include"),
                        os.path.join(d, "t.cpp")], check=True)


# ================================================================== GPU
def _scene(R, fb, pos):
    """A detached resident scene with these positions (one degenerate face: the overlays read vertices only)."""
    v = b32.make_vertices(len(pos))
    if len(pos):
        v["pos"] = pos
    return R.ResidentScene(fb, v, b32.make_faces(1 if len(pos) else 0), []).detach()


class Resident:
    """The parts of a case with their vertices resident: one slot per distinct vertex array; .parts are ObjectParts for the device calls."""

    def __init__(self, R, fb, parts):
        self.scenes, self.parts = {}, []
        for p in parts:
            if id(p.vertices) not in self.scenes:
                self.scenes[id(p.vertices)] = _scene(R, fb, p.vertices)
            self.parts.append(OP(self.scenes[id(p.vertices)], p.topology, p.visible, p.vertices))

    def close(self):
        for s in self.scenes.values():
            s.close()
        for p in self.parts:
            if p.topology is not None:
                p.topology.close()


def _load(fb, px, zb):
    from tests.test_lines import _upload_zbuffer
    fb.upload(px)
    _upload_zbuffer(fb, zb)


def _reductions(ctx):
    return ctx.route_counts()["bounds_reductions"]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(64, 48), (320, 240)])
def test_gpu_stage_tap_equals_the_mirror(gpu_ctx, w, h):
    """b32_object_overlay_project_batch equals the mirror byte for byte on every named case and on the parts of one 257-position and one
    513-position polygon with an empty part between them (rows that cross the 256-lane workgroup); at a case's own frame size also the
    restatement.  The C record count agrees."""
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(w, h, gpu_ctx)
    cases = [(c[0], c[1], c[2], c[3], a[0] if (c[4], c[5]) == (w, h) else None) for c, a in answers()]
    cases.append(("long polygons", *long_polygon_case(), FAR_CAM, None))
    n = 0
    for name, parts, items, cam, want in cases:
        res = Resident(R, fb, parts)
        try:
            got = fb.object_overlay_project_batch(res.parts, items, cam, w, h)
            mirror = RM.object_overlay_records(parts, items, cam, w, h)
            assert len(got) == gpu_ctx.object_overlay_record_count(res.parts, items) == len(mirror), name
            assert got.tobytes() == mirror.tobytes(), f"{name}: places {np.nonzero(got != mirror)[0][:8]} differ from the mirror"
            if want is not None:
                assert got.tobytes() == want.tobytes(), name
            n += len(got)
        finally:
            res.close()
    assert n > 1500


@pytest.mark.gpu
def test_gpu_frames_bands_counts_and_zbuffer(gpu_ctx):
    """The golden Cave frame at 64 x 48, then b32_draw_object_overlays of the named asset (wireframe, mesh box, given box) placed before the
    camera: the pixels equal the oracle's frame with the restatement's records drawn by np_prims, the z-buffer is byte-equal before and
    after, b32_gizmo_counts moves by the restatement's drawn / dropped / rejected.  On the bands (0, 21), (21, 22), (22, H) only their rows
    are written; an empty band runs no kernel: no counter moves, no bounds are reduced."""
    from bonnie32_amd import rasterizer as R
    from tests.test_room_overlay import cave_frame
    w, h = 64, 48
    sc, px, zb = cave_frame(w, h)
    cam = sc.camera
    place = (PLACEMENTS["rotation"][0], PLACEMENTS["rotation"][1], tuple(float(v) for v in np.asarray(cam_point(cam, 0.0, 0.0, 260.0), f32)))
    parts, items = named_asset(), three_calls(place)
    want, counts, _ = ref_object_overlays(parts, items, cam, w, h)
    full = px.copy()
    np_prims(full, zb, w, h, want)
    assert not np.array_equal(full, px) and counts[0] >= 40
    fb = R.Framebuffer(w, h, gpu_ctx)
    res = Resident(R, fb, parts)
    try:
        _load(fb, px, zb)
        fb.set_band(21, 21)                                      # before anything else: the slots' bounds are still to be reduced
        r0, c0 = gpu_ctx.route_counts(), fb.gizmo_counts()
        fb.draw_object_overlays(res.parts, items, cam)
        assert gpu_ctx.route_counts() == r0 and fb.gizmo_counts() == c0
        fb.set_band(0, h)
        assert np.array_equal(fb.pixels, px)
        fb.draw_object_overlays(res.parts, items, cam)
        got = fb.pixels
        assert np.array_equal(got, full), f"{int((got != full).sum())} bytes differ"
        assert np.array_equal(fb.zbuffer.view(np.uint32), zb.view(np.uint32))
        assert tuple(a - b for a, b in zip(fb.gizmo_counts(), c0)) == counts
        assert _reductions(gpu_ctx) - r0["bounds_reductions"] == 3
        rows = lambda a: a.reshape(h, -1)
        for y0, y1 in ((0, 21), (21, 22), (22, h)):
            part = rows(px).copy(); part[y0:y1] = rows(full)[y0:y1]
            assert not np.array_equal(part[y0:y1], rows(px)[y0:y1])
            _load(fb, px, zb)
            fb.set_band(y0, y1)
            fb.draw_object_overlays(res.parts, items, cam)
            fb.set_band(0, h)
            assert np.array_equal(fb.pixels, part.reshape(-1)), (y0, y1)
            assert np.array_equal(fb.zbuffer.view(np.uint32), zb.view(np.uint32))
        _load(fb, px, zb)
        fb.draw_object_overlays(res.parts, [], cam)              # n_items == 0: a no-op
        assert np.array_equal(fb.pixels, px)
    finally:
        fb.set_band(0, h)
        res.close()
    ctx = R.Context(0)                                           # a fresh framebuffer: its z-buffer is not valid, its clear is deferred
    try:
        fb2 = R.Framebuffer(w, h, ctx)
        fb2.clear(b32.Color(3, 4, 5))
        res = Resident(R, fb2, parts)
        base = np.tile(np.array([3, 4, 5, 255], np.uint8), w * h)
        full = base.copy()
        np_prims(full, None, w, h, want)
        fb2.draw_object_overlays(res.parts, items, cam)
        assert np.array_equal(fb2.pixels, full) and not np.array_equal(full, base)
        assert (fb2.zbuffer == np.finfo(f32).max).all()
        res.close()
    finally:
        ctx.close()


def _bounds_positions(nv, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.normal(size=(nv, 3)) * (90.0, 70.0, 110.0)).astype(f32)
    if nv >= 1:
        pos[-1] = (4000.0, -3000.0, 0.0)                         # extremes at the last index ...
    if nv >= 2:
        pos[0] = (-4100.0, 3100.0, -0.0)                         # ... and at the first
    if nv >= 65:
        pos[63, 0] = np.nan; pos[64, 1] = 9000.0; pos[nv // 2, 2] = -9500.0
    return pos


@pytest.mark.gpu
def test_gpu_scene_bounds_bit_for_bit(gpu_ctx):
    """b32_scene_bounds == mesh_bounds bit for bit for 0, 1, 63, 64, 65, 257 and 1025 vertices, blocking and by ticket; the second call
    launches no reduction.  Both vertex layouts: the B32Vertex array right after the upload, and the packed positions, which a slot has
    once a mesh of more than 8192 faces has been drawn twice (frame_positions) -- there the first b32_scene_bounds comes after the frames."""
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(64, 48, gpu_ctx)
    for nv in (0, 1, 63, 64, 65, 257, 1025):
        pos = _bounds_positions(nv, 300 + nv)
        mn, mx, has = RM.mesh_bounds([pos])
        rs = _scene(R, fb, pos)
        try:
            r0 = _reductions(gpu_ctx)
            gmn, gmx, ghas = rs.bounds()
            assert same_bits(gmn, mn) and same_bits(gmx, mx) and ghas == has == (nv > 0), (nv, gmn, mn, gmx, mx)
            assert _reductions(gpu_ctx) == r0 + 1
            t, buf = rs.bounds_async()
            gpu_ctx.ticket_wait(t)
            rec = buf[0][:32].view(abi.SCENE_BOUNDS_DTYPE)[0].copy()
            gpu_ctx.host_free(buf[1])
            assert same_bits(rec["min"], mn) and same_bits(rec["max"], mx) and bool(rec["has_verts"]) == has and int(rec["_pad"]) == 0
            assert _reductions(gpu_ctx) == r0 + 1
        finally:
            rs.close()
    nv = 1025
    pos = _bounds_positions(nv, 77)
    pos[63, 0] = 5.0
    rng = np.random.default_rng(78)
    v = b32.make_vertices(nv); v["pos"] = pos
    f = b32.make_faces(8200); f["v"] = rng.integers(0, nv, (8200, 3))
    rs = R.ResidentScene(fb, v, f, []).detach()
    try:
        cam, st = look_at((0.0, 0.0, -20000.0), (0.0, 0.0, 0.0)), b32.RasterSettings.game()
        for _ in range(2):
            rs.render_async(cam, st); rs.finish()
        mn, mx, has = RM.mesh_bounds([pos])
        gmn, gmx, ghas = rs.bounds()
        assert same_bits(gmn, mn) and same_bits(gmx, mx) and ghas
    finally:
        rs.close()


@pytest.mark.gpu
def test_gpu_box_mesh_follows_every_edit_and_reduces_only_then(gpu_ctx):
    """OBJECT_BOX_MESH equals the mirror on the current arrays after b32_scene_patch_vertices moving the extreme vertex, b32_scene_pose, a
    fresh b32_scene_upload and b32_room_build_mesh into the slot; b32_scene_build_skeleton leaves the bounds (the tail is excluded).  The
    reduction counter advances by one exactly where the body's vertices changed: twenty items over one clean slot launch none, and the
    tail rebuild launches none either (tail_rebuilt keeps bounds_valid)."""
    from bonnie32_amd import rasterizer as R
    from tests.test_room_mesh import real_scene
    from tests.test_room_overlay import room_and_materials
    w, h = 64, 48
    fb = R.Framebuffer(w, h, gpu_ctx)
    sc = real_scene("cave-room0-game")
    rng = np.random.default_rng(91)
    v = b32.make_vertices(40); v["pos"] = (rng.normal(size=(40, 3)) * 60.0).astype(f32)
    rs = R.ResidentScene(fb, v, b32.make_faces(1), sc.textures).detach()
    items = [OI(BOX_MESH, PLACEMENTS["rotation"], 0, 1, YELLOW)]
    seen = set()

    def check(arr, moved, what):
        parts = [OP(rs, None, True, arr)]
        r0 = _reductions(gpu_ctx)
        got = fb.object_overlay_project_batch(parts, items, FAR_CAM, w, h)
        want = RM.object_overlay_records(parts, items, FAR_CAM, w, h)
        assert got.tobytes() == want.tobytes(), what
        assert _reductions(gpu_ctx) - r0 == moved, what
        gmn, gmx, _ = rs.bounds()
        mn, mx, _ = RM.mesh_bounds([arr])
        assert same_bits(gmn, mn) and same_bits(gmx, mx) and _reductions(gpu_ctx) - r0 == moved, what
        seen.add(got.tobytes())

    try:
        check(v, 1, "upload")
        r0 = _reductions(gpu_ctx)
        fb.draw_object_overlays([OP(rs, None, True, v)], items * 20, FAR_CAM)
        assert _reductions(gpu_ctx) == r0
        i = int(np.argmax(v["pos"][:, 0]))
        moved = v.copy(); moved["pos"][i] = (-700.0, 20.0, 30.0)
        rs.patch_vertices([i], moved[[i]])
        check(moved, 1, "patch"); check(moved, 0, "clean")
        bone_of = (np.arange(40) % 3).astype(np.uint16)
        bones = [RM.Bone.from_euler((10.0, 20.0, -30.0), (15.0, 0.0, 40.0)), RM.Bone.from_euler((-40.0, 5.0, 0.0), (0.0, 0.0, -25.0)), RM.Bone.from_euler((0.0, 90.0, 9.0), (33.0, 0.0, 0.0))]
        rs.set_rig(bone_of)
        rs.pose(bones)
        check(RM.pose_vertices(moved, bone_of, RM.pack_bones(bones)), 1, "pose")
        fresh = b32.make_vertices(25); fresh["pos"] = (rng.normal(size=(25, 3)) * (30.0, 200.0, 45.0)).astype(f32)
        one = b32.make_faces(1)
        tex, _keep = b32.rtypes.pack_textures(sc.textures)
        rs._swap()
        try:
            assert gpu_ctx.lib.b32_scene_upload(gpu_ctx.h, abi.ptr(fresh), len(fresh), abi.ptr(one), 1, C.cast(tex, C.c_void_p), len(sc.textures)) == 0
        finally:
            rs._swap()
        rs.n_vertices, rs.n_faces = len(fresh), 1
        check(fresh, 1, "upload into the slot")
        faces, mats, grid, _, _, _ = room_and_materials("cave")
        room = R.Room(gpu_ctx, faces, grid)
        room.set_materials(mats)
        room.build_mesh(rs)
        mesh_v, _ = b32.room_mesh(faces, mats, grid)
        check(mesh_v, 1, "room mesh")
        rs.build_skeleton([RM.SkelBone(pos=(5000.0, 9000.0, -7000.0), length=800.0, width=300.0)])
        assert rs.n_vertices > rs.n_body_vertices == len(mesh_v)
        check(mesh_v, 0, "skeleton tail")
        room.close()
        assert len(seen) == 5
    finally:
        rs.close()


@pytest.mark.gpu
def test_gpu_tap_equals_draw_and_batches_share_the_record_buffer(gpu_ctx):
    """The producer contract for this producer (tests/test_record_producers.py states it for the other four): a draw equals its tap's
    records drawn by b32_draw_prims, with the same counter deltas; and world, object-overlay, gizmo, room-overlay and object-overlay
    batches in a row on one context, with no read in between, equal the same steps replayed from each step's tap records."""
    from bonnie32_amd import rasterizer as R
    from tests.test_record_producers import CAM, H, W, ZMAX, frame, room3, world_items
    px, zb = frame()
    fb = R.Framebuffer(W, H, gpu_ctx)
    place = (PLACEMENTS["rotation"][0], PLACEMENTS["rotation"][1], tuple(float(v) for v in np.asarray(cam_point(CAM, 10.0, -5.0, 0.2 * ZMAX), f32)))
    parts, items = named_asset(), three_calls(place)
    assert int((RM.object_overlay_records(parts, items, CAM, W, H)["kind"] != abi.PRIM_CIRCLE).sum()) > 48
    res = Resident(R, fb, parts)
    faces, mats, grid, rcam, rov = room3()
    room = R.Room(gpu_ctx, faces, grid)
    room.set_materials(mats)
    rng = np.random.default_rng(9500)
    lines = np.concatenate([G(K_LINE, cam_point(CAM, *(rng.uniform(-1, 1, 2) * (600.0, 450.0)), 0.4 * ZMAX), cam_point(CAM, *(rng.uniform(-1, 1, 2) * (600.0, 450.0)), 0.5 * ZMAX),
                              rgb=tuple(int(c) for c in rng.integers(0, 256, 3))) for _ in range(60)])
    wi = world_items(49)
    obj = (lambda: fb.draw_object_overlays(res.parts, items, CAM), lambda: fb.object_overlay_project_batch(res.parts, items, CAM, W, H))
    steps = [(lambda: fb.draw_world(wi, CAM), lambda: fb.world_project_batch(wi, CAM, None, W, H)), obj,
             (lambda: fb.draw_gizmos(lines, CAM), lambda: gpu_ctx.gizmo_project_batch(lines, CAM, None, W, H)),
             (lambda: fb.draw_room_overlay(room, rov, rcam), lambda: fb.room_overlay_project_batch(room, rov, rcam, W, H)), obj]
    counts = lambda: fb.world_counts() + fb.gizmo_counts()
    read = lambda: (fb.pixels, fb.zbuffer.view(np.uint32).copy())
    try:
        _load(fb, px, zb)
        c0 = counts()
        obj[0]()
        drawn, d_draw = read(), tuple(a - b for a, b in zip(counts(), c0))
        _load(fb, px, zb)
        c0 = counts()
        recs = obj[1]()
        d_tap = tuple(a - b for a, b in zip(counts(), c0))
        fb.draw_prims(recs)
        tapped = read()
        assert not np.array_equal(drawn[0], px) and np.array_equal(drawn[0], tapped[0]) and np.array_equal(drawn[1], tapped[1])
        assert np.array_equal(drawn[1], zb.view(np.uint32)) and d_draw == d_tap and any(d_draw[3:]) and not any(d_draw[:3])
        _load(fb, px, zb)
        c0 = counts()
        for draw, _ in steps:
            draw()
        seq, d_seq = read(), tuple(a - b for a, b in zip(counts(), c0))
        _load(fb, px, zb)
        c0 = counts()
        for _, tap in steps:
            fb.draw_prims(tap())
            read()
        step = read()
        assert np.array_equal(seq[0], step[0]), f"{int((seq[0] != step[0]).sum())} bytes differ"
        assert np.array_equal(seq[1], step[1]) and d_seq == tuple(a - b for a, b in zip(counts(), c0)) and any(d_seq[:3]) and any(d_seq[3:])
    finally:
        room.close()
        res.close()


def _real_part(name):
    from tests.test_hover import merge_quads
    from tests.test_room_mesh import real_scene
    sc = real_scene(name)
    return sc, RM.Topology.from_polygons(merge_quads(sc.faces))


@pytest.mark.gpu
def test_gpu_four_delivered_drag_frames():
    """Four frames of clear -> b32_draw_object_overlays -> b32_fb_download_async, each with another placement, nothing blocking in between
    and only the last ticket waited for: every delivered frame equals the clear colour with the restatement's records drawn over it.  The
    slots are real golden asset parts: the three parts of asset3 (the third hidden: it still counts for the box) and obj-warrior with its
    442 polygons."""
    from bonnie32_amd import rasterizer as R
    W, H = 320, 240
    reals = [_real_part(n) for n in ("asset3-part0-game", "asset3-part1-game", "asset3-part2-painter", "obj-warrior")]
    assert reals[3][1].np == 442
    ctx = R.Context(0)
    bufs = []
    try:
        fb = R.Framebuffer(W, H, ctx)
        scenes = [R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach() for sc, _ in reals]
        parts = [OP(s, top, k != 2, sc.vertices) for k, (s, (sc, top)) in enumerate(zip(scenes, reals))]
        mn, mx, _ = RM.mesh_bounds([p.vertices for p in parts])
        centre, radius = (mn + mx) / f32(2.0), float(np.abs(mx - mn).max())
        cam = look_at(tuple(float(v) for v in centre + np.array([0.4, 0.5, -2.2], f32) * f32(radius)), tuple(float(v) for v in centre))
        bufs = [ctx.host_alloc(W * H * 4) for _ in range(4)]
        frames, tickets = [], []
        for i in range(4):
            a = f32(0.4 * i - 0.3)
            pa = (float(np.cos(a)), float(np.sin(a)), (0.12 * radius * i, -0.05 * radius * i, 0.2 * radius * i))
            pb = (float(np.cos(-a)), float(np.sin(-a)), (-0.3 * radius + 0.1 * radius * i, 0.0, 0.35 * radius))
            items = [OI(WIRE, pa, 0, 3, CYAN), OI(BOX_MESH, pa, 0, 3, YELLOW), OI(WIRE, pb, 3, 1, GREEN), OI(BOX_MESH, pb, 3, 1, YELLOW)]
            frames.append(items)
            # ---- everything enqueued without a host synchronisation in between
            fb.clear(b32.Color(20, 24, 30))
            fb.draw_object_overlays(parts, items, cam)
            tickets.append(ctx.download_async(bufs[i][1]))
        ctx.ticket_wait(tickets[-1])
        assert _reductions(ctx) == 4                             # one per slot, in the first frame
        seen = set()
        base = np.tile(np.array([20, 24, 30, 255], np.uint8), W * H)
        for i, items in enumerate(frames):
            want, counts, _ = ref_object_overlays(parts, items, cam, W, H)
            full = base.copy()
            np_prims(full, None, W, H, want)
            got = bufs[i][0][:W * H * 4]
            assert counts[0] > 1000 and np.array_equal(got, full), f"frame {i}: {int((got != full).sum())} bytes differ"
            seen.add(got.tobytes())
        assert len(seen) == 4
        for s in scenes:
            s.close()
    finally:
        for _, p in bufs:
            ctx.host_free(p)
        ctx.close()


@pytest.mark.gpu
def test_gpu_argument_errors(gpu_ctx):
    """Every argument error returns B32_E_ARG and leaves the frame byte-equal: NULL context or camera, a NULL array with a count, a part
    range outside the table, a slot that holds no scene, a visible part of a WIRE item without a topology, an unknown kind or flag,
    non-zero padding, a tap that is too small; b32_scene_bounds of a slot without a scene, without a context, without result pointers."""
    from bonnie32_amd import rasterizer as R
    W, H = 64, 48
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(b32.Color(1, 2, 3))
    base = fb.pixels
    res = Resident(R, fb, named_asset())
    lib, cam = gpu_ctx.lib, FAR_CAM.pack()
    E = abi.B32_E_ARG
    try:
        pa = RM.pack_object_parts(res.parts, gpu_ctx)
        ia = RM.pack_object_items(three_calls(PLACEMENTS["rotation"]))
        draw = lambda p=pa, i=ia, c=gpu_ctx.h, cm=C.byref(cam), np_=None, ni=None: lib.b32_draw_object_overlays(
            c, cm, abi.ptr(p) if p is not None else None, len(pa) if np_ is None else np_, abi.ptr(i) if i is not None else None, len(ia) if ni is None else ni)
        assert draw(c=None) == draw(cm=None) == draw(p=None) == draw(i=None) == E
        empty = C.c_void_p()
        assert lib.b32_scene_create(gpu_ctx.h, C.byref(empty)) == 0
        for field, k, value in (("slot", 1, 0), ("slot", 1, empty.value), ("topology", 0, 0), ("flags", 1, 2), ("_pad", 2, 7)):
            bad = pa.copy(); bad[field][k] = value
            assert draw(p=bad) == E, (field, k)
        for field, k, value in (("kind", 0, 3), ("first_part", 1, 2), ("n_parts", 0, 4), ("first_part", 2, 4)):
            bad = ia.copy(); bad[field][k] = value
            assert draw(i=bad) == E, (field, k)
        bad = ia.copy(); bad["_pad"][1][2] = 1
        assert draw(i=bad) == E
        n = C.c_uint32(77)
        out = np.zeros(100, abi.PRIM_DTYPE)
        tap = lambda w=W, h=H, cap=100, nn=C.byref(n): lib.b32_object_overlay_project_batch(gpu_ctx.h, C.byref(cam), abi.ptr(pa), len(pa), abi.ptr(ia), len(ia), w, h, abi.ptr(out), cap, nn)
        assert tap(w=0) == tap(h=0) == tap(cap=10) == tap(nn=None) == E and n.value == 77
        n64 = C.c_uint64(5)
        assert lib.b32_object_overlay_record_count(abi.ptr(pa), len(pa), abi.ptr(ia), len(ia), None) == E
        assert lib.b32_object_overlay_record_count(None, len(pa), abi.ptr(ia), len(ia), C.byref(n64)) == E and n64.value == 5
        mn, mx, has = (C.c_float * 3)(), (C.c_float * 3)(), C.c_uint32()
        assert lib.b32_scene_bounds(gpu_ctx.h, empty, mn, mx, C.byref(has)) == E and lib.b32_scene_bounds(None, res.parts[0].scene._slot, mn, mx, C.byref(has)) == E
        assert lib.b32_scene_bounds(gpu_ctx.h, res.parts[0].scene._slot, None, mx, C.byref(has)) == E
        t = C.c_uint64()
        assert lib.b32_scene_bounds_async(gpu_ctx.h, res.parts[0].scene._slot, None, C.byref(t)) == E
        lib.b32_scene_destroy(gpu_ctx.h, empty)
        assert np.array_equal(fb.pixels, base)
        assert draw() == abi.B32_OK and not np.array_equal(fb.pixels, base) and tap() == abi.B32_OK and n.value == 24 + 17 + 12 + 12
    finally:
        res.close()
    ctx = R.Context(0)                                           # a context without a framebuffer
    try:
        assert ctx.lib.b32_draw_object_overlays(ctx.h, C.byref(cam), None, 0, None, 0) == E
    finally:
        ctx.close()
