"""bonnie-32_amd — MI355X-native (gfx950) implementation of bonnie-32's `src/rasterizer` hot path:
vertex transform + fixed-point snap, painter's-algorithm sort, affine textured fill with RGB555 dither
(reference: src/rasterizer/render.rs:2302-2638 `render_mesh_15`).

Layout:
  csrc/          hand-written HIP kernels + the C-ABI library (include/b32raster.h)
  abi.py         ctypes mirror of the C ABI, library loader (fails loudly if the .so is missing)
  rtypes.py      mirrors of the reference API types (Vertex/Face/Texture15/Camera/RasterSettings/...)
  records.py     value types and packers: caller input -> ABI records (Placement, Bone, Topology, the overlay structs, prim, ...)
  mirrors/       numpy / float32 restatements of the reference's editor rules -- what a host without the library walks, what the CPU tests
                 compare bit for bit, the CPU baselines of tools/*_time.py: screen.py (what the others share: placement, projection, the
                 triangle table and test), query.py (pick, hover, box), room.py, overlays.py, rig.py (bones, poses, patches, skeleton),
                 sky.py (sky placement and projection, star records)
  rasterizer.py  the binding: Context, Framebuffer, ResidentScene, Room + render_mesh_15 with the reference's signature, on the GPU;
                 re-exports every public name of records.py and mirrors/
  mirror_edit.py mirror editing (b32_scene_build_mirror): build_mirror(dst, src, mirror) over two ResidentScene; re-exports Mirror and mirror_mesh
  sky.py         the sky without a host wait (b32_sky, b32_draw_stars): ResidentSky and draw_stars; re-exports the mirror mirrors/sky.py
  scenegen.py    deterministic synthetic scenes of BASELINE.md (C1..C5 + parity variants)
  parallel.py    screen-band sharding across ranks + the RCCL gather of band rows
  build.py       hipcc recipe for csrc/
Imports go one way: rasterizer -> mirrors -> records -> abi / rtypes.
"""
from . import abi, rtypes  # noqa: F401
from . import rtypes as types  # noqa: F401  (alias: mirrors the reference module name src/rasterizer/types.rs)
from .rtypes import (Camera, Color, IndexedTexture, Light, RasterSettings, RasterTimings, Texture, Texture15,  # noqa: F401
                    make_faces, make_vertices)
from .records import Bone, MeshOverlay, ObjectItem, ObjectPart, Placement, RoomOverlay, Topology, place_vertices  # noqa: F401
from .mirrors.overlays import (mesh_bounds, mesh_overlay_record_count, mesh_overlay_records, object_overlay_record_count,  # noqa: F401
                               object_overlay_records, room_overlay_record_count, room_overlay_records)
from .mirrors.query import box_select_mesh, hover_mesh, hovered_element, pick_mesh  # noqa: F401
from .mirrors.rig import bone_world_transforms, pose_vertices  # noqa: F401
from .mirrors.room import (RoomMirror, room_box_select, room_faces_from_sectors, room_hover, room_hover_winner,  # noqa: F401
                           room_materials_from_sectors, room_mesh, room_mesh_counts)

__all__ = ["abi", "types", "Camera", "Color", "IndexedTexture", "Light", "RasterSettings", "RasterTimings",
           "Texture", "Texture15", "make_faces", "make_vertices", "Placement", "place_vertices", "pick_mesh",
           "Topology", "hover_mesh", "hovered_element", "box_select_mesh", "Bone", "bone_world_transforms", "pose_vertices",
           "Room", "RoomMirror", "room_faces_from_sectors", "room_materials_from_sectors", "room_mesh", "room_mesh_counts", "room_hover", "room_box_select", "room_hover_winner",
           "MeshOverlay", "mesh_overlay_records", "mesh_overlay_record_count", "RoomOverlay", "room_overlay_records", "room_overlay_record_count",
           "ObjectPart", "ObjectItem", "object_overlay_records", "object_overlay_record_count", "mesh_bounds"]


def __getattr__(name):
    """Room alone lives in the binding: looked up on first use, so that importing the package, records.py or mirrors/ does not import it."""
    if name == "Room":
        from .rasterizer import Room
        return Room
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
