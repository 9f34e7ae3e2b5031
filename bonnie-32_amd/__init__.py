"""bonnie-32_amd — MI355X-native (gfx950) implementation of bonnie-32's `src/rasterizer` hot path:
vertex transform + fixed-point snap, painter's-algorithm sort, affine textured fill with RGB555 dither
(reference: src/rasterizer/render.rs:2302-2638 `render_mesh_15`).

Layout:
  csrc/          hand-written HIP kernels + the C-ABI library (include/b32raster.h)
  abi.py         ctypes mirror of the C ABI, library loader (fails loudly if the .so is missing)
  rtypes.py      mirrors of the reference API types (Vertex/Face/Texture15/Camera/RasterSettings/...)
  rasterizer.py  Framebuffer + render_mesh_15 with the reference's signature, running on the GPU
  scenegen.py    deterministic synthetic scenes of BASELINE.md (C1..C5 + parity variants)
  parallel.py    screen-band sharding across ranks + the RCCL gather of band rows
  build.py       hipcc recipe for csrc/
"""
from . import abi, rtypes  # noqa: F401
from . import rtypes as types  # noqa: F401  (alias: mirrors the reference module name src/rasterizer/types.rs)
from .rtypes import (Camera, Color, IndexedTexture, Light, RasterSettings, RasterTimings, Texture, Texture15,  # noqa: F401
                    make_faces, make_vertices)
from .rasterizer import Bone, Placement, Topology, bone_world_transforms, pose_vertices, box_select_mesh, hover_mesh, hovered_element, pick_mesh, place_vertices, Room, RoomMirror, room_faces_from_sectors, room_materials_from_sectors, room_mesh, room_mesh_counts, room_hover, room_box_select, room_hover_winner, MeshOverlay, mesh_overlay_records, mesh_overlay_record_count, RoomOverlay, room_overlay_records, room_overlay_record_count, ObjectPart, ObjectItem, object_overlay_records, object_overlay_record_count, mesh_bounds  # noqa: F401  (host restatements of render_asset_parts' per-vertex transform and of check_mesh_hit: no GPU needed)

__all__ = ["abi", "types", "Camera", "Color", "IndexedTexture", "Light", "RasterSettings", "RasterTimings",
           "Texture", "Texture15", "make_faces", "make_vertices", "Placement", "place_vertices", "pick_mesh",
           "Topology", "hover_mesh", "hovered_element", "box_select_mesh", "Bone", "bone_world_transforms", "pose_vertices",
           "Room", "RoomMirror", "room_faces_from_sectors", "room_materials_from_sectors", "room_mesh", "room_mesh_counts", "room_hover", "room_box_select", "room_hover_winner",
           "MeshOverlay", "mesh_overlay_records", "mesh_overlay_record_count", "RoomOverlay", "room_overlay_records", "room_overlay_record_count",
           "ObjectPart", "ObjectItem", "object_overlay_records", "object_overlay_record_count", "mesh_bounds"]
