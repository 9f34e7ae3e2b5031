"""Picking: which placed resident mesh, and which of its triangles, lies under the cursor (b32_pick_meshes).

The reference answers that on the host every frame: check_mesh_hit (editor/viewport_3d.rs:7700-7756, called per visible part of every
enabled object, :7344-7400) and the face branch of the modeler's find_hovered_element (modeler/viewport.rs:2544-2594).
  `ref_pick`   a literal scalar restatement of those loops, every operand an np.float32, built on tests.test_world's restatements of the
               world_to_screen functions; pinned by hand-computed cases;
  `b32.pick_mesh` / rasterizer.PickMirror   the library's numpy host mirror, pinned to ref_pick on the CPU;
  the device   compared with the mirror.
Every comparison is exact: hit, triangle index, depth bits (any NaN equals any NaN) and the best item.  `closest` is updated with a strict
`<`, so ties go to the first in loop order and a NaN depth sticks when it comes first: the order cases below are built for that."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi, scenegen
from tests.test_world import IDENTITY_CAM, ORTHO, _cam_f32, ref_world_to_screen, ref_world_to_screen_with_ortho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden", "scenes", "real")
f32 = np.float32
NO_TRI = 0xFFFFFFFF
IDENT = (1.0, 0.0, (0.0, 0.0, 0.0))                            # (cos_f, sin_f, world_pos): the placement is applied even so
# tests/test_placement.py's list (test_place_vertices_is_the_scalar_f32_restatement), the infinite one included, behind the identity
PLACEMENTS = [IDENT,
              (np.cos(f32(0.7)), np.sin(f32(0.7)), (100.5, -20.25, 3000.0)), (np.cos(f32(-2.9)), np.sin(f32(-2.9)), (-1e-3, 0.0, -0.0)),
              (0.0, -1.0, (0.0, 0.0, 0.0)), (0.6, 0.8, (np.inf, 0.0, -np.inf))]
UNIT_ORTHO = (1.0, 0.0, 0.0)                                   # sx = x + w / 2, sy = -y + h / 2, depth = z under the identity camera


def _bits(x):
    return int(np.array([x], f32).view(np.uint32)[0])


def same_hit(a, b):
    """(hit, tri, depth) equal: depth bit for bit, except that any NaN equals any NaN."""
    return bool(a[0]) == bool(b[0]) and int(a[1]) == int(b[1]) and (_bits(a[2]) == _bits(b[2]) or (np.isnan(a[2]) and np.isnan(b[2])))


# ---------------------------------------------------------------- literal restatement
def point_in_triangle_2d(px, py, x1, y1, x2, y2, x3, y3):      # math.rs:687-706
    def sign(px, py, ax, ay, bx, by):
        return (px - bx) * (ay - by) - (ax - bx) * (py - by)
    d1 = sign(px, py, x1, y1, x2, y2)
    d2 = sign(px, py, x2, y2, x3, y3)
    d3 = sign(px, py, x3, y3, x1, y1)
    has_neg = (d1 < 0.0) or (d2 < 0.0) or (d3 < 0.0)
    has_pos = (d1 > 0.0) or (d2 > 0.0) or (d3 > 0.0)
    return not (has_neg and has_pos)


def interpolate_depth_in_triangle(px, py, x0, y0, d0, x1, y1, d1, x2, y2, d2):     # viewport_3d.rs:7485-7508
    area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    if abs(area) < f32(0.0001):
        return (d0 + d1 + d2) / f32(3.0)
    w0 = ((x1 - px) * (y2 - py) - (x2 - px) * (y1 - py)) / area
    w1 = ((x2 - px) * (y0 - py) - (x0 - px) * (y2 - py)) / area
    w2 = f32(1.0) - w0 - w1
    return w0 * d0 + w1 * d1 + w2 * d2


def ref_screen_verts(positions, placement, camera, w, h, ortho=None):
    """check_mesh_hit's screen_verts (viewport_3d.rs:7714-7728): every local vertex rotated, translated and projected; None stays None."""
    cam = _cam_f32(camera)
    cos_f, sin_f = f32(placement[0]), f32(placement[1])
    wx, wy, wz = (f32(v) for v in placement[2])
    out = []
    with np.errstate(all="ignore"):
        for p in positions:
            x, y, z = f32(p[0]), f32(p[1]), f32(p[2])
            rx = x * cos_f - z * sin_f
            rz = x * sin_f + z * cos_f
            world = (rx + wx, y + wy, rz + wz)
            out.append(ref_world_to_screen(world, cam, w, h) if ortho is None else ref_world_to_screen_with_ortho(world, cam, w, h, ortho))
    return out


def ref_candidates(screen_verts, tris, mx, my, cull_backfaces=False):
    """The body of the triangle loop: [(tri, depth)] of every hit in face order."""
    mx, my = f32(mx), f32(my)
    hits = []
    with np.errstate(all="ignore"):
        for t, (a, b, c) in enumerate(tris):
            if a >= len(screen_verts) or b >= len(screen_verts) or c >= len(screen_verts):     # screen_verts.get(..) == None
                continue
            v0, v1, v2 = screen_verts[a], screen_verts[b], screen_verts[c]
            if v0 is None or v1 is None or v2 is None:
                continue
            (x0, y0, d0), (x1, y1, d1), (x2, y2, d2) = v0, v1, v2
            if cull_backfaces:
                signed_area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
                if signed_area <= 0.0:                         # modeler/viewport.rs:2571-2574
                    continue
            if not point_in_triangle_2d(mx, my, x0, y0, x1, y1, x2, y2):
                continue
            hits.append((t, interpolate_depth_in_triangle(mx, my, x0, y0, d0, x1, y1, d1, x2, y2, d2)))
    return hits


def ref_closest(cands):
    """`if closest.map_or(true, |d| depth < d) { closest = Some(..) }` over (id, depth) in order."""
    closest = None
    for t, depth in cands:
        if closest is None or depth < closest[1]:
            closest = (t, depth)
    if closest is None:
        return False, NO_TRI, f32(0.0)
    return True, closest[0], closest[1]


def ref_pick(vertices, faces, placement, camera, w, h, mx, my, ortho=None, cull_backfaces=False):
    sv = ref_screen_verts(vertices["pos"], placement, camera, w, h, ortho)
    return ref_closest(ref_candidates(sv, [tuple(int(i) for i in f) for f in faces["v"]], mx, my, cull_backfaces))


def ref_best(hits):
    """The loop over the items, viewport_3d.rs:7370: hits = [(hit, tri, depth)] -> index or -1."""
    hit, best, _ = ref_closest([(i, h[2]) for i, h in enumerate(hits) if h[0]])
    return best if hit else -1


# ---------------------------------------------------------------- inputs
def cursors(w, h, n=200, seed=1):
    """Cursor k = (rng.random() * w, rng.random() * h), the two numbers drawn in that order; odd k truncated to integers."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        mx = rng.random() * w; my = rng.random() * h
        out.append((float(int(mx)), float(int(my))) if k & 1 else (mx, my))
    return out


def box_cursors(scene, n=200, seed=1):
    """The same recipe inside the projected bounding box of the mesh (identity placement, perspective)."""
    from bonnie32_amd.rasterizer import PickMirror
    m = PickMirror(scene.vertices, scene.faces, IDENT, scene.camera, scene.width, scene.height)
    xs = np.concatenate([v[m.ok] for v in m.x]); ys = np.concatenate([v[m.ok] for v in m.y])
    x0, x1, y0, y1 = float(xs.min()), float(xs.max()), float(ys.min()), float(ys.max())
    return [(x0 + cx / scene.width * (x1 - x0), y0 + cy / scene.height * (y1 - y0)) if not k & 1 else
            (float(int(x0 + cx / scene.width * (x1 - x0))), float(int(y0 + cy / scene.height * (y1 - y0))))
            for k, (cx, cy) in enumerate(_raw_cursors(scene.width, scene.height, n, seed))]


def _raw_cursors(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.random() * w, rng.random() * h) for _ in range(n)]


_SCENES = {}


def scene(name):
    """(scene, cursors, (least hits, least multi-candidate cursors) for the identity placement in perspective)."""
    if name not in _SCENES:
        if name in ("C1", "C2"):
            sc = scenegen.make_scene(name)
        else:
            from bonnie32_amd import scenefile
            sc = scenefile.read_scene(os.path.join(REAL, name + ".b32scene"))
        if name == "obj-warrior":
            _SCENES[name] = (sc, box_cursors(sc), (50, 0))
        else:
            _SCENES[name] = (sc, cursors(sc.width, sc.height), {"C1": (50, 15), "dungeon-room0-game": (150, 80)}.get(name, (0, 0)))
    return _SCENES[name]


def c1_head(n=256):
    sc, _, _ = scene("C1")
    return sc, sc.vertices.copy(), sc.faces[:n].copy()


def with_vertex(vertices, pos):
    v = np.concatenate([vertices, vertices[:1]])
    v["pos"][-1] = pos
    return v, len(v) - 1


def face_of(faces, a, b, c):
    f = faces[:1].copy()
    f["v"][0] = (a, b, c)
    return f


def order_cases():
    """name -> (vertices, faces, what(hit) must hold for every cursor with a hit in the plain list) on the first 256 faces of C1."""
    sc, v, f = c1_head()
    nan_v, nan_i = with_vertex(v, (np.nan, 0.0, 1000.0))
    inf_v, inf_i = with_vertex(v, (np.inf, 0.0, 1000.0))
    a = int(f["v"][0][0]); b = int(f["v"][0][1])
    return {
        "plain": (v, f),
        "copy_behind": (v, np.concatenate([f, f])),
        "reversed_copy_behind": (v, np.concatenate([f, f[::-1]])),
        "nan_face_first": (nan_v, np.concatenate([face_of(f, nan_i, a, b), f])),
        "nan_face_last": (nan_v, np.concatenate([f, face_of(f, nan_i, a, b)])),
        "inf_vertex_first": (inf_v, np.concatenate([face_of(f, inf_i, a, b), f])),
        "inf_vertex_last": (inf_v, np.concatenate([f, face_of(f, a, inf_i, b)])),
        "index_out_of_range": (v, np.concatenate([face_of(f, a, len(v), b), f[:100], face_of(f, NO_TRI, a, b), f[100:], face_of(f, a, b, len(v) + 7)])),
        "same_vertex_thrice_last": (v, np.concatenate([f, face_of(f, a, a, a)])),
    }


def zero_pair(order):
    """Two coincident triangles under the identity camera and UNIT_ORTHO whose camera z is -0.0 (`neg`) and +0.0 (`pos`): x < 0, y < 0 and
    a placement with world_pos.z = -0.0, so that rz + wz and the dot product keep the sign.  order: "neg_first" / "pos_first"."""
    v = b32.make_vertices(6)
    tri = np.array([(-40.0, -30.0), (-8.0, -30.0), (-40.0, -4.0)], f32)
    v["pos"][:3, :2] = tri; v["pos"][:3, 2] = -0.0
    v["pos"][3:, :2] = tri; v["pos"][3:, 2] = 0.0
    faces = b32.make_faces(2)
    neg, pos = (0, 1, 2), (3, 4, 5)
    faces["v"][0], faces["v"][1] = (neg, pos) if order == "neg_first" else (pos, neg)
    return v, faces, (1.0, 0.0, (0.0, 0.0, -0.0)), (160.0 - 30.0, 120.0 + 20.0)


# ================================================================== without a GPU
def test_pick_pod_layout_matches_c():
    """B32PickHit compiled against the public header has the layout of abi.PICK_HIT_DTYPE, and the built library exports both entries."""
    import __graft_entry__ as g
    g.build()
    lib = abi.load_library()
    fields = ("hit", "tri", "depth", "_pad")
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void){ printf("%zu", sizeof(B32PickHit));'
            + "".join(f' printf(" %zu", offsetof(B32PickHit, {f}));' for f in fields) + ' printf(" %u\\n", B32_PICK_CULL_BACKFACES); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == abi.PICK_HIT_DTYPE.itemsize == 16
    assert out[1:5] == [abi.PICK_HIT_DTYPE.fields[f][1] for f in fields] == [0, 4, 8, 12]
    assert out[5] == abi.PICK_CULL_BACKFACES == 1
    for name in ("b32_pick_meshes", "b32_pick_meshes_async"):
        assert name in {n for n, _, _ in abi.SYMBOLS} and getattr(lib, name).argtypes is not None
    E = abi.B32_E_ARG                                               # NULL context: no device needed
    assert lib.b32_pick_meshes(None, None, None, 0.0, 0.0, 0, None, None, 0, None, None) == E
    assert lib.b32_pick_meshes_async(None, None, None, 0.0, 0.0, 0, None, None, 0, None, None) == E


def _tri_mesh(points, tris):
    v = b32.make_vertices(len(points))
    v["pos"] = np.array(points, f32)
    f = b32.make_faces(len(tris))
    f["v"] = np.array(tris, np.uint32)
    return v, f


def test_ref_pick_hand_cases():
    """Identity camera, 320x240.  Under UNIT_ORTHO a vertex (x, y, z) lands at (x + 160, -y + 120) with depth z, so the triangle
    A = (0, 0, 2), B = (8, 0, 4), C = (0, -8, 6) is (160, 120), (168, 120), (160, 128) with signed area 8 * 8 - 0 = 64.
      cursor at A: the edge functions are (0, 64, 0): inside; w0 = 64 / 64, w1 = 0, w2 = 0: depth 2.
      cursor (164, 120), the middle of AB: (0, 32, 32): inside; w0 = w1 = 32 / 64: depth 0.5 * 2 + 0.5 * 4 + 0 * 6 = 3.
      cursor (164, 120 - u), u = 2^-17 (one ulp of 120): the edge function of AB is 0 - (-8) * (-u) = -8 u, the other two stay positive: outside;
      the same cursor with the winding reversed is outside too (the test has no winding), and (164, 120 + u) is inside.
      A face (i, i, i) of the vertex (3, 4, 7): every edge function is (px - x) * 0 - 0 * (py - y) = 0, so it is hit from EVERY cursor, area 0,
      depth ((7 + 7) + 7) / 3 = 7.
      |area| < 0.0001: (0, 0, 1), (2^-7, 0, 2), (0, -2^-7, 6) has area 2^-14 = 0.000061: the cursor at its first vertex gets the average
      (1 + 2 + 6) / 3 = 3, not the vertex's 1; scaled by 2 (area 2^-12 = 0.00024) it gets 1.
    Perspective (vs = 90): (10, 20, 95) lands at (196, 192), (-10, -20, 45) at (88, -24), (10, -20, 45) at (232, -24); the cursor at the first
    vertex reads depth 95; a vertex at z = 0.1 is None and takes its triangle with it."""
    W, H = 320, 240
    v, f = _tri_mesh([(0, 0, 2), (8, 0, 4), (0, -8, 6)], [(0, 1, 2)])
    pick = lambda v, f, mx, my, ortho=UNIT_ORTHO, cull=False: ref_pick(v, f, IDENT, IDENTITY_CAM, W, H, mx, my, ortho, cull)
    assert ref_screen_verts(v["pos"], IDENT, IDENTITY_CAM, W, H, UNIT_ORTHO) == [(160.0, 120.0, 2.0), (168.0, 120.0, 4.0), (160.0, 128.0, 6.0)]
    assert pick(v, f, 160.0, 120.0) == (True, 0, 2.0)
    assert pick(v, f, 164.0, 120.0) == (True, 0, 3.0)
    u = 2.0 ** -17
    assert float(np.nextafter(f32(120.0), f32(0.0))) == 120.0 - u
    assert pick(v, f, 164.0, 120.0 - u) == (False, NO_TRI, 0.0)
    assert pick(v, f, 164.0, 120.0 + u)[0] and pick(v, f, 164.0, 120.0 + u, cull=True)[0]
    rv, rf = _tri_mesh([(0, 0, 2), (8, 0, 4), (0, -8, 6)], [(0, 2, 1)])              # the other winding: area -64
    assert pick(rv, rf, 164.0, 120.0 - u) == (False, NO_TRI, 0.0)
    assert pick(rv, rf, 164.0, 120.0) == (True, 0, 3.0) and pick(rv, rf, 164.0, 120.0, cull=True) == (False, NO_TRI, 0.0)
    assert pick(v, f, 164.0, 120.0, cull=True) == (True, 0, 3.0)
    v3, f3 = _tri_mesh([(3, 4, 7)], [(0, 0, 0)])
    for cur in ((0.0, 0.0), (300.5, 200.25), (163.0, 116.0), (-5e6, 9e9)):
        assert pick(v3, f3, *cur) == (True, 0, 7.0)
        assert pick(v3, f3, *cur, ortho=None) == (True, 0, 7.0)                   # (and in perspective: z = 7 > 0.1)
        assert pick(v3, f3, *cur, cull=True) == (False, NO_TRI, 0.0)              # area 0 <= 0: culled
    s = 2.0 ** -7
    vt, ft = _tri_mesh([(0, 0, 1), (s, 0, 2), (0, -s, 6)], [(0, 1, 2)])
    assert pick(vt, ft, 160.0, 120.0) == (True, 0, 3.0)
    vt2, _ = _tri_mesh([(0, 0, 1), (2 * s, 0, 2), (0, -2 * s, 6)], [(0, 1, 2)])
    assert pick(vt2, ft, 160.0, 120.0) == (True, 0, 1.0)
    vp, fp = _tri_mesh([(10, 20, 95), (-10, -20, 45), (10, -20, 45), (0, 0, 0.1)], [(0, 1, 2), (0, 1, 3)])
    sv = ref_screen_verts(vp["pos"], IDENT, IDENTITY_CAM, W, H)
    assert sv[:3] == [(196.0, 192.0, 95.0), (88.0, -24.0, 45.0), (232.0, -24.0, 45.0)] and sv[3] is None
    assert pick(vp, fp, 196.0, 192.0, ortho=None) == (True, 0, 95.0)
    assert ref_candidates(sv, [(0, 1, 2), (0, 1, 3), (0, 1, 9)], 196.0, 192.0) == [(0, f32(95.0))]      # None and an index out of range: skipped
    # the placement is applied first: a quarter turn (cos 0, sin 1) takes (x, y, z) to (-z, y, x), then the offset
    assert ref_screen_verts([(5.0, 1.0, 2.0)], (0.0, 1.0, (10.0, 20.0, 30.0)), IDENTITY_CAM, W, H, UNIT_ORTHO) == [(168.0, 99.0, 35.0)]
    # the loops' strict `<`
    nan = f32(np.nan)
    assert ref_closest([(4, f32(2.0)), (7, f32(2.0)), (9, f32(1.0)), (11, f32(1.0))]) == (True, 9, 1.0)
    assert ref_closest([(4, f32(-0.0)), (7, f32(0.0))])[1] == 4 and _bits(ref_closest([(4, f32(-0.0)), (7, f32(0.0))])[2]) == 0x80000000
    assert ref_closest([(4, f32(0.0)), (7, f32(-0.0))])[1] == 4 and _bits(ref_closest([(4, f32(0.0)), (7, f32(-0.0))])[2]) == 0
    r = ref_closest([(2, nan), (3, f32(-5.0))]); assert r[1] == 2 and np.isnan(r[2])                  # NaN first: sticky
    assert ref_closest([(2, f32(5.0)), (3, nan), (4, f32(4.0))]) == (True, 4, 4.0)                    # NaN later: ignored
    assert ref_best([(False, NO_TRI, f32(0.0)), (True, 5, f32(3.0)), (True, 1, f32(3.0)), (True, 0, nan)]) == 1
    assert ref_best([(True, 0, nan), (True, 5, f32(3.0))]) == 0 and ref_best([(False, NO_TRI, f32(0.0))] * 3) == -1 and ref_best([]) == -1


def _mirror_equals_ref(sc, vertices, faces, placement, curs, orthos=(None, ORTHO), culls=(False, True)):
    """PickMirror == ref_pick for every cursor; returns {(ortho, cull): (cursors with a hit, cursors with more than one candidate)}."""
    from bonnie32_amd.rasterizer import PickMirror
    tris = [tuple(int(i) for i in f) for f in faces["v"]]
    stats = {}
    for ortho in orthos:
        sv = ref_screen_verts(vertices["pos"], placement, sc.camera, sc.width, sc.height, ortho)
        m = PickMirror(vertices, faces, placement, sc.camera, sc.width, sc.height, ortho)
        for cull in culls:
            n_hit = n_multi = 0
            for mx, my in curs:
                cands = ref_candidates(sv, tris, mx, my, cull)
                want = ref_closest(cands)
                got = m.pick(mx, my, cull)
                assert same_hit(got, want), (ortho, cull, mx, my, got, want)
                t, d = m.candidates(mx, my, cull)
                assert [int(x) for x in t] == [c[0] for c in cands]
                n_hit += bool(cands); n_multi += len(cands) > 1
            stats[(ortho, cull)] = (n_hit, n_multi)
    return stats


@pytest.mark.parametrize("name", ["C1", "dungeon-room0-game", "obj-warrior"])
def test_host_mirror_equals_ref_pick(name):
    """b32.pick_mesh == ref_pick on hit, tri and depth bits for the 200 cursors, perspective and ORTHO, culling off and on; the cursors
    cannot pass on misses: C1 has 78 cursors with a hit and 21 with more than one candidate, the dungeon room 200 and 110."""
    sc, curs, (least_hits, least_multi) = scene(name)
    stats = _mirror_equals_ref(sc, sc.vertices, sc.faces, IDENT, curs)
    n_hit, n_multi = stats[(None, False)]
    print(name, stats)
    assert n_hit >= least_hits and n_multi >= least_multi, stats
    mx, my = curs[0]
    assert same_hit(b32.pick_mesh(sc.vertices, sc.faces, IDENT, sc.camera, sc.width, sc.height, mx, my),
                    ref_pick(sc.vertices, sc.faces, IDENT, sc.camera, sc.width, sc.height, mx, my))
    # a placed copy: turned and moved, seen through the same camera (every third cursor)
    _mirror_equals_ref(sc, sc.vertices, sc.faces, (np.cos(f32(0.21)), np.sin(f32(0.21)), (35.0, -12.0, 40.0)), curs[::3], culls=(False,))


def test_order_cases_on_the_host():
    """The order cases against ref_pick, and what each of them is about."""
    sc, _, _ = scene("C1")
    from bonnie32_amd.rasterizer import PickMirror
    cases = order_cases()
    curs = cursors(sc.width, sc.height)
    plain = PickMirror(*cases["plain"], IDENT, sc.camera, sc.width, sc.height)
    base = [plain.pick(mx, my) for mx, my in curs]
    assert sum(h[0] for h in base) >= 10
    for name, (v, f) in cases.items():
        _mirror_equals_ref(sc, v, f, IDENT, curs[::2], orthos=(None,), culls=(False,))
        m = PickMirror(v, f, IDENT, sc.camera, sc.width, sc.height)
        for (mx, my), b in zip(curs, base):
            got = m.pick(mx, my)
            if name in ("copy_behind", "reversed_copy_behind") or (name in ("nan_face_last", "inf_vertex_last") and b[0]):
                assert same_hit(got, b), name                       # the first copy wins its tie; a NaN behind a number is ignored
            elif name == "nan_face_first":
                assert got[0] and got[1] == 0 and _bits(got[2]) == 0x7FC00000, name       # the sticky NaN, from every cursor
            elif name == "index_out_of_range" and b[0]:
                assert got[0] and got[1] == b[1] + (1 if b[1] < 100 else 2) and _bits(got[2]) == _bits(b[2]), name
            elif name == "same_vertex_thrice_last":
                assert got[0]                                       # hit from every cursor
    last = PickMirror(*cases["nan_face_last"], IDENT, sc.camera, sc.width, sc.height)
    miss = [c for c, b in zip(curs, base) if not b[0]]
    assert miss and all(last.pick(*c)[1] == 256 and np.isnan(last.pick(*c)[2]) for c in miss)      # ... unless it is the only hit


def test_signed_zero_tie_on_the_host():
    """Two coincident triangles at camera z -0.0 and +0.0 tie: the first in face order wins and ITS zero is reported."""
    for order, bits in (("neg_first", 0x80000000), ("pos_first", 0x00000000)):
        v, f, place, cur = zero_pair(order)
        sv = ref_screen_verts(v["pos"], place, IDENTITY_CAM, 320, 240, UNIT_ORTHO)
        zs = [_bits(s[2]) for s in sv]
        assert sorted(set(zs[0:3])) == [0x80000000] and sorted(set(zs[3:6])) == [0]        # the model really yields both zeros
        cands = ref_candidates(sv, [tuple(int(i) for i in t) for t in f["v"]], *cur)
        assert len(cands) == 2 and {_bits(c[1]) for c in cands} == {0, 0x80000000}
        want = ref_pick(v, f, place, IDENTITY_CAM, 320, 240, *cur, UNIT_ORTHO)
        assert want[0] and want[1] == 0 and _bits(want[2]) == bits
        assert same_hit(b32.pick_mesh(v, f, place, IDENTITY_CAM, 320, 240, *cur, UNIT_ORTHO), want)


def test_item_loop_on_the_host():
    """rasterizer.pick_best == the loop over the items: identical placements tie (the first wins), a NaN item first sticks, last is ignored."""
    from bonnie32_amd.rasterizer import pick_best
    rng = np.random.default_rng(5)
    nan = f32(np.nan)
    pool = [f32(1.5), f32(1.5), f32(-0.0), f32(0.0), nan, f32(np.inf), f32(-np.inf), f32(7.0)]
    for _ in range(300):
        n = int(rng.integers(0, 7))
        hits = [(bool(rng.integers(0, 2)), int(rng.integers(0, 50)), pool[int(rng.integers(0, len(pool)))]) for _ in range(n)]
        H = np.zeros(n, abi.PICK_HIT_DTYPE)
        for i, h in enumerate(hits):
            H[i] = (h[0], h[1], h[2], 0)
        assert pick_best(H) == ref_best(hits), hits
    H = np.zeros(3, abi.PICK_HIT_DTYPE)
    H["hit"] = 1; H["depth"] = 4.0
    assert pick_best(H) == 0
    H["depth"][0] = nan; assert pick_best(H) == 0
    H["depth"] = (4.0, 4.0, nan); assert pick_best(H) == 0
    H["hit"][0] = 0; assert pick_best(H) == 1


def test_random_set_tells_a_fused_evaluation_apart():
    """w0 * d0 + w1 * d1 + w2 * d2 contracted into fused multiply-adds rounds differently for some of the candidates of the random set.
    The fused form is evaluated in float64 (the product of two f32 is exact there) and rounded once per fused operation; the set must
    contain depths where it differs from the separately rounded result, so that nothing built with FMA contraction can pass the
    comparisons of this file -- and the mirror must be the separately rounded one."""
    from bonnie32_amd.rasterizer import PickMirror
    n_diff = n_all = 0
    for name in ("C1", "dungeon-room0-game"):
        sc, curs, _ = scene(name)
        m = PickMirror(sc.vertices, sc.faces, IDENT, sc.camera, sc.width, sc.height)
        for mx, my in curs:
            t, depth = m.candidates(mx, my)
            if not len(t):
                continue
            px, py = f32(mx), f32(my)
            (x0, x1, x2), (y0, y1, y2), (d0, d1, d2) = ([v[t] for v in g] for g in (m.x, m.y, m.d))
            area = m.area[t]
            w0 = ((x1 - px) * (y2 - py) - (x2 - px) * (y1 - py)) / area
            w1 = ((x2 - px) * (y0 - py) - (x0 - px) * (y2 - py)) / area
            w2 = f32(1.0) - w0 - w1
            unfused = (w0 * d0 + w1 * d1) + w2 * d2
            big = np.abs(area) >= f32(0.0001)
            assert np.array_equal(unfused[big].view(np.uint32), depth[big].view(np.uint32))
            D = np.float64
            inner = (w1.astype(D) * d1.astype(D) + (w0 * d0).astype(D)).astype(f32)           # fma(w1, d1, w0 * d0)
            fused = (w2.astype(D) * d2.astype(D) + inner.astype(D)).astype(f32)               # fma(w2, d2, inner)
            n_diff += int((fused[big].view(np.uint32) != unfused[big].view(np.uint32)).sum()); n_all += int(big.sum())
    assert n_all >= 300 and n_diff >= 10, (n_diff, n_all)


def test_cpp_mirror_pick_compiles():
    """host/rasterizer.hpp: the pick wrappers, the host mirror and FrameLoop's pick compile (header-only over the C ABI)."""
    hpp_dir = os.path.join(ROOT, "bonnie-32_amd", "host")
    src = ('#include "rasterizer.hpp"\nvoid f(b32::Framebuffer& fb, b32::ResidentMesh& a, const b32::Camera& cam, const std::vector<b32::Vertex>& v, const std::vector<b32::Face>& fc,\n'
           '       const b32::RasterSettings& st) {\n'
           ' std::vector<b32::PickItem> items{ { &a, b32::Placement::from_facing(0.5f, b32::Vec3{ 1, 2, 3 }) }, { &a, b32::Placement{} } };\n'
           ' b32::PickResult r = b32::pick_meshes(fb, items, cam, 10.0f, 20.0f); (void)(r.best + (int)r.hits.size());\n'
           ' r = b32::pick_meshes(fb, items, cam, 10.0f, 20.0f, b32::Vec3{ 1.0f, 0.0f, 0.0f }, true);\n'
           ' void* out = b32_host_alloc(16 + 16 * items.size()); const uint64_t t = b32::pick_meshes_async(fb, items, cam, 1.0f, 2.0f, out);\n'
           ' b32::check(b32_ticket_wait(fb.ctx(), t), "wait"); r = b32::pick_result(out); b32_host_free(out);\n'
           ' const B32PickHit h = b32::pick_mesh(v, fc, items[0].placement, cam, 320, 240, 1.0f, 2.0f, std::nullopt, false); (void)h.hit;\n'
           ' (void)b32::pick_best(r.hits);\n'
           ' b32::FrameLoop loop(fb); b32::FramePick pk{ items, 3.0f, 4.0f };\n'
           ' const uint64_t ft = loop.submit(b32::Color{}, { { &a, b32::MeshParams{ 0.5f, true, false, std::nullopt } } }, cam, st, &pk);\n'
           ' (void)loop.wait(ft); (void)loop.wait_pick(ft).best; }\n'
           'int main() { (void)&f; return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", hpp_dir, "-I", os.path.join(ROOT, "include"),
                        os.path.join(d, "t.cpp")], check=True)


# ================================================================== on the GPU
def _hit_of(rec):
    return bool(rec["hit"]), int(rec["tri"]), f32(rec["depth"])


def _check_picks(ctx, camera, w, h, items, curs, orthos=(None,), culls=(False,)):
    """items = [(detached ResidentScene, (vertices, faces), placement)]: every cursor through ONE b32_pick_meshes call for all items,
    against the mirror per item and the loop over the items.  Returns the mirror's hits per (ortho, cull): [[(hit, tri, depth)] per cursor]."""
    from bonnie32_amd.rasterizer import PickMirror, pick_best
    table = ctx.make_pick_table([(rs, pl) for rs, _, pl in items])
    out = {}
    for ortho in orthos:
        mirrors = [PickMirror(v, f, pl, camera, w, h, ortho) for _, (v, f), pl in items]
        for cull in culls:
            rows = []
            for mx, my in curs:
                best, hits = ctx.pick_meshes(table, camera, (mx, my), ortho, cull)
                want = [m.pick(mx, my, cull) for m in mirrors]
                for i, wnt in enumerate(want):
                    assert same_hit(_hit_of(hits[i]), wnt), (ortho, cull, mx, my, i, hits[i], wnt)
                    if not wnt[0]:
                        assert hits[i]["tri"] == NO_TRI and _bits(hits[i]["depth"]) == 0
                    if np.isnan(wnt[2]):
                        assert _bits(hits[i]["depth"]) == 0x7FC00000
                assert best == ref_best(want) == pick_best(hits), (ortho, cull, mx, my, best, want)
                rows.append(want)
            out[(ortho, cull)] = rows
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C1", "dungeon-room0-game", "obj-warrior"])
def test_gpu_pick_scenes(gpu_ctx, name):
    """b32_pick_meshes == b32.pick_mesh on the 200 cursors: five placements of the scene as five items of one call (the identity, and
    four of tests/test_placement.py's list, the infinite one among them), perspective and ORTHO, culling off and on."""
    from bonnie32_amd import rasterizer as R
    sc, curs, (least_hits, least_multi) = scene(name)
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    try:
        res = _check_picks(gpu_ctx, sc.camera, sc.width, sc.height, [(rs, (sc.vertices, sc.faces), pl) for pl in PLACEMENTS], curs,
                           orthos=(None, ORTHO), culls=(False, True))
    finally:
        rs.close()
    assert sum(row[0][0] for row in res[(None, False)]) >= least_hits
    per_placement = [sum(row[i][0] for rows in res.values() for row in rows) for i in range(len(PLACEMENTS))]
    print(name, per_placement)
    assert per_placement[0] >= least_hits and sum(p > 0 for p in per_placement) >= 2, per_placement


@pytest.mark.gpu
def test_gpu_pick_order_cases(gpu_ctx):
    """Every order case of the host tests on the device: the copy behind (the first copy wins), the reversed copy, the NaN face first
    (sticky) and last (ignored), an infinite vertex, an index out of range (skipped, no error), (i, i, i); the two zeros in both orders; and
    the same one level up, as items: identical placements tie, a NaN item first, a NaN item last."""
    from bonnie32_amd import rasterizer as R
    sc, curs, _ = scene("C1")
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    cases = order_cases()
    slots = {}
    try:
        for name, (v, f) in cases.items():
            slots[name] = R.ResidentScene(fb, v, f, sc.textures).detach()
            res = _check_picks(gpu_ctx, sc.camera, sc.width, sc.height, [(slots[name], (v, f), IDENT)], curs, culls=(False, True))
            if name == "nan_face_first":
                assert all(r[0][1] == 0 and np.isnan(r[0][2]) for r in res[(None, False)])
        item = lambda n: (slots[n], cases[n], IDENT)
        tie = _check_picks(gpu_ctx, sc.camera, sc.width, sc.height, [item("plain"), item("copy_behind"), item("plain")], curs)
        assert sum(r[0][0] for r in tie[(None, False)]) >= 10
        _check_picks(gpu_ctx, sc.camera, sc.width, sc.height, [item("nan_face_first"), item("plain")], curs[:60])       # best = 0, NaN, always
        _check_picks(gpu_ctx, sc.camera, sc.width, sc.height, [item("plain"), item("nan_face_first")], curs[:60])       # ignored behind a number
        for order, bits in (("neg_first", 0x80000000), ("pos_first", 0)):
            v, f, place, cur = zero_pair(order)
            z = R.ResidentScene(fb, v, f, []).detach()
            best, hits = gpu_ctx.pick_meshes([(z, place)], IDENTITY_CAM, cur, UNIT_ORTHO)
            z.close()
            assert best == 0 and hits[0]["hit"] == 1 and hits[0]["tri"] == 0 and _bits(hits[0]["depth"]) == bits, (order, hits)
    finally:
        for s in slots.values():
            s.close()


@pytest.mark.gpu
def test_gpu_pick_many_workgroups(gpu_ctx):
    """C2 (100 000 triangles: 98 workgroups, about twenty candidates per cursor), 50 cursors; again with the face list doubled, so that
    every winner ties with a triangle of another workgroup; again after two drawn frames, when the slot has its packed position stream."""
    from bonnie32_amd import rasterizer as R
    sc, curs, _ = scene("C2")
    curs = curs[:50]
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    twice = np.concatenate([sc.faces, sc.faces])
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    rs2 = R.ResidentScene(fb, sc.vertices, twice, sc.textures).detach()
    try:
        res = _check_picks(gpu_ctx, sc.camera, sc.width, sc.height, [(rs, (sc.vertices, sc.faces), IDENT)], curs, culls=(False, True))
        res2 = _check_picks(gpu_ctx, sc.camera, sc.width, sc.height, [(rs2, (sc.vertices, twice), IDENT), (rs, (sc.vertices, sc.faces), PLACEMENTS[1])], curs)
        hits = [r[0] for r in res[(None, False)]]
        assert sum(h[0] for h in hits) >= 40 and all(same_hit(a, r[0]) for a, r in zip(hits, res2[(None, False)]))
        assert len({h[1] // 1024 for h in hits if h[0]}) >= 10              # winners from many workgroups
        for _ in range(2):                                                  # (a large mesh packs its positions on its second frame)
            fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings); rs.finish()
        again = _check_picks(gpu_ctx, sc.camera, sc.width, sc.height, [(rs, (sc.vertices, sc.faces), IDENT)], curs)
        assert all(same_hit(a, r[0]) for a, r in zip(hits, again[(None, False)]))
    finally:
        rs.close(); rs2.close()


def _frame_items(fr, slots, placements):
    """The pick items of tests.test_placement._Frame: the room (identity) and every part of every object with its placement."""
    return [(slots[i], (fr.mesh(i).vertices, fr.mesh(i).faces), IDENT if pl is None else pl) for i, _, pl in fr.entries(placements)]


@pytest.mark.gpu
def test_gpu_pick_many_items(gpu_ctx):
    """24 placed items of 3 slots in one call (the table travels in the kernel argument), 34 of 4 slots (it lives in device memory): repeated
    slots, an object behind the camera that nothing hits, best against the loop over the items; n == 0."""
    from bonnie32_amd import rasterizer as R
    from tests.test_placement import _Frame
    fr = _Frame()
    fb = R.Framebuffer(fr.W, fr.H, gpu_ctx)
    slots = fr.upload(R, fb)
    try:
        items = _frame_items(fr, slots, fr.placements(0.0))
        assert len(items) == 34
        fr12 = _Frame(n_objects=12)                                       # the room and two parts of twelve objects: 25 items of 3 slots
        three = [it for it in _frame_items(fr12, slots, fr12.placements(0.0)) if it[0] is not slots[3]][:24]
        assert len(three) == 24 and len({id(it[0]) for it in three}) == 3
        curs = cursors(fr.W, fr.H, 60)
        res = _check_picks(gpu_ctx, fr.cam, fr.W, fr.H, three, curs, orthos=(None, ORTHO), culls=(False, True))
        rows = res[(None, False)]
        assert any(not any(r[i][0] for r in rows) for i in range(24)) and len({ref_best(r) for r in rows}) >= 3
        res34 = _check_picks(gpu_ctx, fr.cam, fr.W, fr.H, items, curs)
        assert len({ref_best(r) for r in res34[(None, False)]}) >= 3
        best, hits = gpu_ctx.pick_meshes([], fr.cam, (10.0, 10.0))
        assert best == -1 and len(hits) == 0
    finally:
        for s in slots:
            s.close()


@pytest.mark.gpu
def test_gpu_pick_errors(gpu_ctx):
    """A NULL or empty slot, NULL places with n > 0, an unknown flag, a zero-size framebuffer: B32_E_ARG; n > 65535: B32_E_UNSUPPORTED;
    NULL output pointers: B32_E_ARG."""
    from bonnie32_amd import rasterizer as R
    sc, _, _ = scene("C1")
    fb = R.Framebuffer(sc.width, sc.height, gpu_ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    lib, h = gpu_ctx.lib, gpu_ctx.h
    cam = sc.camera.pack()
    slots, places, n = gpu_ctx.make_pick_table([(rs, IDENT), (rs, IDENT)])
    hits = np.zeros(2, abi.PICK_HIT_DTYPE); best = C.c_int32(7); t = C.c_uint64()
    pl = C.cast(places, C.c_void_p)
    call = lambda *a: lib.b32_pick_meshes(h, C.byref(cam), None, 5.0, 5.0, *a)
    assert call(0, slots, pl, 2, hits.ctypes.data, C.byref(best)) == abi.B32_OK
    empty = C.c_void_p()
    assert lib.b32_scene_create(h, C.byref(empty)) == 0
    try:
        for bad in (None, empty):
            s2 = (C.c_void_p * 2)(slots[0], bad)
            assert call(0, s2, pl, 2, hits.ctypes.data, C.byref(best)) == abi.B32_E_ARG
        assert call(0, slots, None, 2, hits.ctypes.data, C.byref(best)) == abi.B32_E_ARG
        assert call(0, None, pl, 2, hits.ctypes.data, C.byref(best)) == abi.B32_E_ARG
        assert call(2, slots, pl, 2, hits.ctypes.data, C.byref(best)) == abi.B32_E_ARG
        assert call(0x80000000, slots, pl, 2, hits.ctypes.data, C.byref(best)) == abi.B32_E_ARG
        assert call(0, slots, pl, 65536, hits.ctypes.data, C.byref(best)) == abi.B32_E_UNSUPPORTED
        assert call(0, slots, pl, 2, None, None) == abi.B32_E_ARG
        assert call(0, slots, pl, 2, None, C.byref(best)) == abi.B32_OK                      # hits is nullable
        assert lib.b32_pick_meshes(h, None, None, 5.0, 5.0, 0, slots, pl, 2, hits.ctypes.data, C.byref(best)) == abi.B32_E_ARG
        buf, p = gpu_ctx.host_alloc(16 + 32)
        try:
            acall = lambda *a: lib.b32_pick_meshes_async(h, C.byref(cam), None, 5.0, 5.0, 0, slots, pl, 2, *a)
            assert acall(None, C.byref(t)) == abi.B32_E_ARG and acall(p, None) == abi.B32_E_ARG
            assert lib.b32_pick_meshes_async(h, C.byref(cam), None, 5.0, 5.0, 0, slots, pl, 65536, p, C.byref(t)) == abi.B32_E_UNSUPPORTED
            assert acall(p, C.byref(t)) == abi.B32_OK
            gpu_ctx.ticket_wait(t.value)
            assert buf[:8].view(np.int32)[1] == 2
        finally:
            gpu_ctx.host_free(p)
        with pytest.raises(R.B32Error):
            gpu_ctx.pick_meshes((slots, places, 70000), sc.camera, (1.0, 1.0))
        fresh = R.Context(0)                                                             # no framebuffer yet: zero-size
        try:
            assert fresh.lib.b32_pick_meshes(fresh.h, C.byref(cam), None, 5.0, 5.0, 0, None, None, 0, None, C.byref(best)) == abi.B32_E_ARG
        finally:
            fresh.close()
    finally:
        lib.b32_scene_destroy(h, empty)
        rs.close()


def _delivered_run(R, fr, mode, with_picks, n_frames=30):
    """clear, b32_frame_submit_placed, b32_pick_meshes_async, b32_fb_download_async per frame with moving placements and a moving cursor;
    tickets waited one frame behind, no blocking call in the loop.  mode "deep": deep asynchronous mode; "safe_clear_pending": safe mode
    and the pick enqueued between the clear and the draws, while the clear is still deferred."""
    ctx = R.Context(0)
    ctx.set_async_depth(1 if mode == "deep" else 0)
    fb = R.Framebuffer(fr.W, fr.H, ctx)
    slots = fr.upload(R, fb)
    st = fr.settings()
    entries = fr.entries(fr.placements(0.0))
    table = ctx.make_frame_table(fr.cam, st, [slots[i] for i, _, _ in entries], fogs=[p["fog"] for _, p, _ in entries],
                                 ambients=[p["ambient"] for _, p, _ in entries], placements=[pl for _, _, pl in entries],
                                 backface_culls=[p["backface_cull"] for _, p, _ in entries])
    ptable = ctx.make_pick_table([(slots[i], IDENT) for i, _, _ in entries])
    bufs = [ctx.host_alloc(fr.W * fr.H * 4) for _ in range(2)]
    pbufs = [ctx.host_alloc(16 + 16 * len(entries)) for _ in range(2)]
    tickets, ptickets, presults = [0, 0], [0, 0], [None, None]
    frames, picks, counts = [], [], []

    def pick(t):
        per_entry = [IDENT] + [pl for pl in fr.placements(float(t)) for _ in range(3)]
        ctx.set_pick_placements(ptable, per_entry)
        ptickets[t & 1], presults[t & 1] = ctx.pick_meshes_async(ptable, fr.cam, moving_cursor(fr, t), out=pbufs[t & 1])

    def collect(t):
        ctx.ticket_wait(tickets[t & 1])
        frames.append(bufs[t & 1][0].copy())
        if with_picks:
            ctx.ticket_wait(ptickets[t & 1])
            picks.append((presults[t & 1].best, presults[t & 1].hits))
    try:
        for t in range(n_frames):
            pls = fr.placements(float(t))
            ctx.set_table_placements(table, [None] + [pls[k] for k in range(fr.n_objects) for _ in range(3)])
            fb.clear(fr.clear)
            if with_picks and mode == "safe_clear_pending":
                pick(t)
            ctx.frame_submit(table)
            if with_picks and mode != "safe_clear_pending":
                pick(t)
            tickets[t & 1] = ctx.download_async(bufs[t & 1][1])
            counts.append(ctx.batch_counts())
            if t > 0:
                collect(t - 1)
        collect(n_frames - 1)
        ctx.finish()
        counts.append(ctx.batch_counts())
    finally:
        for _, p in bufs + pbufs:
            ctx.host_free(p)
        ctx.close()
    return frames, picks, counts


def moving_cursor(fr, t):
    return (fr.W * (0.5 + 0.42 * np.sin(0.37 * t)), fr.H * (0.5 + 0.4 * np.cos(0.23 * t)))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["deep", "safe_clear_pending"])
def test_gpu_pick_does_not_interfere_with_delivered_frames(mode):
    """30 delivered frames with one asynchronous pick each: the frames are byte-equal to the same run without picks, every pick equals the
    mirror's, every b32_batch_count is the same after every frame, and nothing in the loop blocks (tickets are waited one frame behind)."""
    from bonnie32_amd import rasterizer as R
    from bonnie32_amd.rasterizer import PickMirror
    from tests.test_placement import _Frame
    fr = _Frame()
    plain_frames, _, plain_counts = _delivered_run(R, fr, mode, False)
    frames, picks, counts = _delivered_run(R, fr, mode, True)
    assert len(frames) == len(plain_frames) == 30 and len(picks) == 30
    for t, (a, b) in enumerate(zip(frames, plain_frames)):
        assert np.array_equal(a, b), f"frame {t}: {int((a != b).sum())} bytes differ"
    assert all(not np.array_equal(frames[t], frames[t + 1]) for t in range(29)) and counts == plain_counts
    bests = []
    for t, (best, hits) in enumerate(picks):
        items = _frame_items(fr, [None] * 4, fr.placements(float(t)))
        mx, my = moving_cursor(fr, t)
        want = [PickMirror(v, f, pl, fr.cam, fr.W, fr.H).pick(mx, my) for _, (v, f), pl in items]
        assert len(hits) == len(want) and all(same_hit(_hit_of(h), w) for h, w in zip(hits, want)), t
        assert best == ref_best(want), t
        bests.append(best)
    assert sum(b >= 0 for b in bests) >= 20 and len(set(bests)) >= 3, bests


@pytest.mark.gpu
def test_gpu_nine_outstanding_tickets_of_mixed_kinds():
    """Picks and framebuffer downloads share the tickets: nine are issued without a wait in between (the ninth first waits for the oldest),
    then all are waited for; every pick and every frame is right."""
    from bonnie32_amd import rasterizer as R
    sc, curs, _ = scene("dungeon-room0-game")
    ctx = R.Context(0)
    fb = R.Framebuffer(sc.width, sc.height, ctx)
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings, sc.fog); rs.finish()
    want_px = np.asarray(fb.pixels).reshape(-1)
    table = ctx.make_pick_table([(rs, IDENT), (rs, PLACEMENTS[1])])
    want = [ctx.pick_meshes(table, sc.camera, curs[k]) for k in range(9)]
    fbufs = [ctx.host_alloc(sc.width * sc.height * 4) for _ in range(4)]
    try:
        issued = []
        for k in range(9):
            if k % 2 == 0:
                issued.append(("pick", k) + ctx.pick_meshes_async(table, sc.camera, curs[k]))
            else:
                issued.append(("frame", k, ctx.download_async(fbufs[k // 2][1]), fbufs[k // 2][0]))
        ts = [i[2] for i in issued]
        assert ts == list(range(ts[0], ts[0] + 9))
        assert ctx.ticket_done(ts[0])                                          # the ninth waited for it
        for kind, k, t, res in issued:
            ctx.ticket_wait(t)
            if kind == "pick":
                assert res.best == want[k][0] and res.hits.tobytes() == want[k][1].tobytes(), k
                res.close()
            else:
                assert np.array_equal(res, want_px), k
        assert sum(w[0] >= 0 for w in want) >= 5
    finally:
        for _, p in fbufs:
            ctx.host_free(p)
        rs.close(); ctx.close()


@pytest.mark.gpu
def test_cpp_pick_harness(tmp_path):
    """tests/cpp/pick_harness.cpp: a golden scene file through the C++ mirror's pick_meshes / pick_meshes_async on the device and its host
    restatement pick_mesh (compiled without contraction), all three against the Python mirror."""
    import __graft_entry__ as g
    g.build()
    from bonnie32_amd.rasterizer import PickMirror
    sc, curs, _ = scene("dungeon-room0-game")
    exe = tmp_path / "pick_harness"
    lib_dir = os.path.join(ROOT, "bonnie-32_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "bonnie-32_amd", "host"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "pick_harness.cpp"), "-o", str(exe), "-L", lib_dir, "-lb32raster", f"-Wl,-rpath,{lib_dir}"], check=True)
    place = (np.cos(f32(0.21)), np.sin(f32(0.21)), (35.0, -12.0, 40.0))
    curs = [(f32(mx), f32(my)) for mx, my in curs[:40]]
    mirrors = [PickMirror(sc.vertices, sc.faces, pl, sc.camera, sc.width, sc.height) for pl in (place, IDENT)]
    for cull in (0, 1):
        args = [repr(float(f32(x))) for x in (place[0], place[1]) + place[2]] + [repr(float(v)) for c in curs for v in c]
        r = subprocess.run([str(exe), os.path.join(REAL, "dungeon-room0-game.b32scene"), str(cull)] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.strip().splitlines()
        assert len(lines) == len(curs)
        for (mx, my), line in zip(curs, lines):
            dev, abest, host = (part.split() for part in line.replace("host:", "").split("|"))
            want = [m.pick(mx, my, bool(cull)) for m in mirrors]
            for k, wnt in enumerate(want):
                for src in (dev[1:], host):
                    got = (src[3 * k] == "1", int(src[3 * k + 1]), np.array([int(src[3 * k + 2], 16)], np.uint32).view(f32)[0])
                    assert same_hit(got, wnt), (line, k, wnt)
            assert int(dev[0]) == int(abest[0]) == ref_best(want), line
