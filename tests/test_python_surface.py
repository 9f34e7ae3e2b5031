"""The Python side's two promises, checked without a library or a device.

1. The surface: the public names of `bonnie32_amd` and `bonnie32_amd.rasterizer` and every public signature are what
   tests/golden/python_surface.json recorded (tools/python_surface.py made it; moving code between modules must not change it).
2. The layering: `records` and everything under `mirrors/` import and run without the library and without the binding."""
import ast
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bonnie-32_amd")
MIRRORS = ("screen", "query", "room", "overlays", "rig")


def _tool():
    spec = importlib.util.spec_from_file_location("python_surface", os.path.join(ROOT, "tools", "python_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_surface_is_the_recorded_one():
    tool = _tool()
    with open(tool.FIXTURE) as f:
        recorded = f.read()
    assert tool.dumps(tool.surface()) == recorded


def _lower_layer_files():
    files = [os.path.join(PKG, "records.py")] + sorted(os.path.join(PKG, "mirrors", n) for n in os.listdir(os.path.join(PKG, "mirrors")) if n.endswith(".py"))
    assert {os.path.join(PKG, "mirrors", m + ".py") for m in MIRRORS} <= set(files)
    return files


def test_lower_layers_do_not_import_the_binding():
    for path in _lower_layer_files():
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""] + [a.name for a in node.names]
            else:
                continue
            assert not any(n.split(".")[-1] == "rasterizer" for n in names), "%s:%d imports the binding" % (path, node.lineno)


# One call of every mirror family on the smallest inputs that reach each shared rule: a triangle hit and a miss, a placed mesh in ortho and
# in perspective, a vertex behind the near plane, a floor and a wall sector, a segment that crosses the near plane.
_CHILD = r'''
import ctypes
import sys
import numpy as np


def _no_library(*a, **k):
    raise AssertionError("the lower layers must not load the library")


ctypes.CDLL = _no_library            # before the package body runs: an import-time load in any layer fails here
sys.path.insert(0, %(root)r)
from bonnie32_amd import abi
abi.load_library = _no_library       # and a call-time load in a mirror function fails here
import importlib
from bonnie32_amd import records as K, rtypes as T
mods = {m: importlib.import_module("bonnie32_amd.mirrors." + m) for m in %(mirrors)r}
import bonnie32_amd.mirrors
assert "bonnie32_amd.rasterizer" not in sys.modules, "importing the lower layers pulled in the binding"
Q, RO, OV, RG = mods["query"], mods["room"], mods["overlays"], mods["rig"]

cam = T.Camera(position=(0.0, 0.0, -10.0))
W, H = 64, 48
v = T.make_vertices(4)
v["pos"] = [(-2, -2, 0), (2, -2, 0), (0, 2, 0), (0, 0, -30)]          # vertex 3 lies behind the near plane
f = T.make_faces(2)
f["v"] = [(0, 1, 2), (0, 1, 3)]
top = K.Topology.triangles(f)
place = K.Placement(facing=0.25, world_pos=(0.5, 0.0, 1.0))
ortho = (4.0, 0.0, 0.0)

hit = Q.pick_mesh(v, f, place, cam, W, H, W / 2, H / 2)                # perspective, placed: the cursor is on triangle 0
assert hit[0] and hit[1] == 0, hit
miss = Q.pick_mesh(v, f, place, cam, W, H, 1.0, 1.0, ortho=ortho)       # ortho, placed: nothing under the corner
assert not miss[0], miss
for o in (None, ortho):
    for pl in (None, place):
        r = Q.hover_mesh(v, top, pl, cam, W, H, W / 2, H / 2, ortho=o, see_through=True)      # (ortho flips y and with it the winding)
        assert int(r["face"]) != abi.HOVER_NONE, (o, pl, r)                 # triangle 0 covers the centre in all four
        Q.box_select_mesh(v, top, pl, cam, W, H, (0, 0, W, H), mode=abi.BOX_POLYGONS, ortho=o)
words, n = Q.box_select_mesh(v, top, None, cam, W, H, (0, 0, W, H))
assert n == 3, (words, n)                                                # the vertex behind the near plane does not project

sectors = [[{"floor": [0.0, 0.0, 0.0, 0.0], "walls_north": [[0.0, 0.0, 512.0, 512.0]]}]]
faces = RO.room_faces_from_sectors(sectors)
mats = RO.room_materials_from_sectors(sectors, lambda ref: None)
grid = ((-512.0, -300.0, 100.0), 1024.0)
assert sorted(faces["kind"]) == [abi.ROOM_FLOOR, abi.ROOM_WALL_NORTH]
rcam = T.Camera(position=(0.0, 200.0, -1500.0))
rh = RO.room_hover(faces, grid, rcam, W, H, W / 2, H / 2)
assert int(rh["face_rec"]) != abi.HOVER_NONE, rh
RO.room_hover(faces, grid, rcam, W, H, -500.0, -500.0)
RO.room_box_select(faces, grid, rcam, W, H, (0, 0, W, H), points=[(0.0, 0.0, 0.0)])
rv, rf = RO.room_mesh(faces, mats, grid)
assert (len(rv), len(rf)) == RO.room_mesh_counts(faces, mats) == (10, 4)

inside = T.Camera(position=(0.0, 0.0, 600.0))                            # stands in the sector: its outline crosses the near plane
for c in (rcam, inside):
    ov = K.RoomOverlay(sections=abi.ROOM_OVERLAY_ALL, hover=RO.room_hover(faces, grid, c, W, H, W / 2, H / 2), vertices=[0, 5], edges=[(0, 1), (1, 2)],
                       faces=[0, 1], points=[(0.0, 0.0, 600.0)], rect=(0.0, 0.0, float(W), float(H)))
    recs, counts = OV.room_overlay_records(faces, grid, ov, c, W, H, materials=mats, with_counts=True)
    assert len(recs) == OV.room_overlay_record_count(len(faces), ov) and sum(counts) > 0
mo = K.MeshOverlay(sections=abi.OVERLAY_ALL, hover_vertex=0, hover_edge=(0, 1), hover_face=0, select_kind=abi.SELECT_POLYGONS,
                   preview_mode=abi.PREVIEW_FACE, rect=(0.0, 0.0, float(W), float(H)))
for o in (None, ortho):
    recs = OV.mesh_overlay_records(v, top, mo, [0, 1], cam, W, H, ortho=o)
    assert len(recs) == OV.mesh_overlay_record_count(top, len(v), mo, [0, 1])
parts = [K.ObjectPart(topology=top, vertices=v)]
items = [K.ObjectItem(abi.OBJECT_WIRE, place, 0, 1), K.ObjectItem(abi.OBJECT_BOX_MESH, place, 0, 1),
         K.ObjectItem(abi.OBJECT_BOX, place, box=((-1, -1, -1), (1, 1, 1)))]
recs, counts = OV.object_overlay_records(parts, items, cam, W, H, with_counts=True)       # the wire's edges to vertex 3 cross the near plane
assert len(recs) == OV.object_overlay_record_count(parts, items) == 6 + 12 + 12 and counts[0] > 0

bones = [K.Bone.from_euler((1.0, 2.0, 3.0), (30.0, 0.0, 45.0)), K.Bone.from_euler((0.0, 1.0, 0.0), (0.0, 0.0, 0.0))]
posed = RG.pose_vertices(v, [0, 1, abi.BONE_NONE, 0], bones)
assert len(posed) == 4 and (posed["pos"][2] == v["pos"][2]).all()
skel = [K.SkelBone.from_rig((0, 0, 0), (10.0, 0.0, 20.0), 50.0, 0.0), K.SkelBone.from_rig((0, 50, 0), (0.0, 0.0, 0.0), 30.0, 10.0, parent=0)]
sv, sf = RG.skeleton_mesh(skel, K.SkeletonStyle(selected_bone=1), vertex_offset=4)
assert (len(sv), len(sf)) == (12, 16)
assert "bonnie32_amd.rasterizer" not in sys.modules
print("ok")
'''


def test_lower_layers_run_without_library_or_binding():
    src = _CHILD % {"root": ROOT, "mirrors": MIRRORS}
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
