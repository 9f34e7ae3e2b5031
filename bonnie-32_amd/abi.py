"""ctypes mirror of include/b32raster.h (the C-ABI drop-in boundary for `render_mesh_15`,
reference: src/rasterizer/render.rs:2302-2310) and the loader of the HIP library.

The loader fails loudly when libb32raster.so is missing: there is no CPU fallback on the product path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libb32raster.so")

# ---- error codes -----------------------------------------------------------
B32_OK, B32_E_ARG, B32_E_INDEX, B32_E_NAN_KEY, B32_E_HIP, B32_E_UNSUPPORTED, B32_E_NO_DEVICE, B32_E_FRAME_DROPPED, B32_E_BAND_TIMEOUT = 0, -1, -2, -3, -4, -5, -6, -7, -8
NO_TEXTURE = 0xFFFFFFFF

# BlendMode (types.rs:1380-1388)
OPAQUE, AVERAGE, ADD, SUBTRACT, ADD_QUARTER, ERASE = range(6)
# ShadingMode (types.rs:1289-1294)
SHADE_NONE, SHADE_FLAT, SHADE_GOURAUD = range(3)
# LightType (types.rs:1297-1304)
LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_SPOT = range(3)

# ---- numpy dtypes with the exact C layout (used for bulk vertex/face arrays) ----
VERTEX_DTYPE = np.dtype([("pos", "<f4", 3), ("uv", "<f4", 2), ("normal", "<f4", 3),
                         ("r", "u1"), ("g", "u1"), ("b", "u1"), ("blend", "u1")])
FACE_DTYPE = np.dtype([("v", "<u4", 3), ("texture_id", "<u4"), ("black_transparent", "u1"),
                       ("blend_mode", "u1"), ("editor_alpha", "u1"), ("_pad", "u1")])
assert VERTEX_DTYPE.itemsize == 36 and FACE_DTYPE.itemsize == 20


class B32Texture15(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("blend_mode", C.c_uint32), ("_pad", C.c_uint32),
                ("pixels", C.c_void_p)]


class B32Texture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("blend_mode", C.c_uint32), ("_pad", C.c_uint32), ("pixels", C.c_void_p)]


# B32Line (Framebuffer line family, b32_draw_lines): kinds B32_LINE_*
LINE_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("z0", "<f4"), ("z1", "<f4"),
                       ("r", "u1"), ("g", "u1"), ("b", "u1"), ("blend", "u1"), ("kind", "u1"), ("alpha", "u1"), ("_pad", "u1", 2)])
assert LINE_DTYPE.itemsize == 32
LINE_2D, LINE_2D_ALPHA, LINE_3D, LINE_3D_OVERLAY, LINE_3D_ALPHA = range(5)

# B32Prim (the rest of the Framebuffer drawing methods, b32_draw_prims): kinds 0..4 = LINE_*, then B32_PRIM_*
PRIM_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("z0", "<f4"), ("z1", "<f4"), ("size", "<i4"),
                       ("r", "u1"), ("g", "u1"), ("b", "u1"), ("blend", "u1"), ("kind", "u1"), ("alpha", "u1"), ("mode", "u1"), ("_pad", "u1", 5)])
assert PRIM_DTYPE.itemsize == 40
PRIM_LINE_BLENDED, PRIM_CIRCLE, PRIM_CIRCLE_ALPHA, PRIM_THICK_LINE, PRIM_RECT, PRIM_FILLED_RECT = range(5, 11)

# B32WorldItem (world-space overlay items, b32_draw_world): kind = LINE_* / PRIM_* 0..8, flags = WORLD_CLIP_NEAR
WORLD_ITEM_DTYPE = np.dtype([("p0", "<f4", 3), ("p1", "<f4", 3), ("size", "<i4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("blend", "u1"),
                             ("kind", "u1"), ("alpha", "u1"), ("mode", "u1"), ("flags", "u1"), ("_pad", "u1", 4)])
assert WORLD_ITEM_DTYPE.itemsize == 40
WORLD_CLIP_NEAR = 1

# B32GizmoItem (the world editor's clipped lines and filled gizmos, b32_draw_gizmos): kind = GIZMO_*
GIZMO_ITEM_DTYPE = np.dtype([("p0", "<f4", 3), ("p1", "<f4", 3), ("p2", "<f4", 3), ("size", "<i4"), ("r", "u1"), ("g", "u1"), ("b", "u1"),
                             ("blend", "u1"), ("kind", "u1"), ("_pad", "u1", 3)])
assert GIZMO_ITEM_DTYPE.itemsize == 48
GIZMO_LINE, GIZMO_LINE_DEPTH, GIZMO_THICK_LINE_DEPTH, GIZMO_POINT, GIZMO_TRIANGLE, GIZMO_TRIANGLE_VIEW = range(6)
GIZMO_MAX_THICKNESS = 16
# the record kind of a filled triangle in the stage tap's output (library-internal: no drawing entry accepts it from the host);
# the third point's x and y are the bit patterns of z0 and z1
PRIM_TRIANGLE_INTERNAL = 11

# B32MeshOverlay (the modeler's selection overlays from resident vertices, b32_draw_mesh_overlay): sections = OVERLAY_* bits
OVERLAY_BRACKETS, OVERLAY_EDGES, OVERLAY_DOTS, OVERLAY_HOVER, OVERLAY_SELECTED, OVERLAY_PREVIEW = 1, 2, 4, 8, 16, 32
OVERLAY_ALL = 63
OVERLAY_NONE = 0xFFFFFFFF
SELECT_NONE, SELECT_VERTICES, SELECT_EDGES, SELECT_POLYGONS = range(4)
PREVIEW_VERTEX, PREVIEW_EDGE, PREVIEW_FACE = range(3)


class B32MeshOverlay(C.Structure):
    _fields_ = [("sections", C.c_uint32), ("hover_vertex", C.c_uint32), ("hover_edge_v0", C.c_uint32), ("hover_edge_v1", C.c_uint32),
                ("hover_face", C.c_uint32), ("select_kind", C.c_uint32), ("n_selected", C.c_uint32), ("preview_mode", C.c_uint32),
                ("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float)]


assert C.sizeof(B32MeshOverlay) == 48


# B32RoomOverlay (the world editor's room overlays from a resident room, b32_draw_room_overlay): sections = ROOM_OVERLAY_* bits
ROOM_OVERLAY_VERTICES, ROOM_OVERLAY_EDGES, ROOM_OVERLAY_HOVER, ROOM_OVERLAY_SELECTED, ROOM_OVERLAY_PREVIEW = 1, 2, 4, 8, 16
ROOM_OVERLAY_ALL = 31
ROOM_OVERLAY_HOVER_GIVEN, ROOM_OVERLAY_HOVER_RESIDENT = 0, 1     # hover_source


class B32RoomHover(C.Structure):
    _fields_ = [("vertex_rec", C.c_uint32), ("vertex_corner", C.c_uint32), ("vertex_dist", C.c_float), ("vertex_depth", C.c_float),
                ("edge_rec", C.c_uint32), ("edge_idx", C.c_uint32), ("edge_dist", C.c_float), ("edge_depth", C.c_float),
                ("face_rec", C.c_uint32), ("face_depth", C.c_float), ("_pad", C.c_uint32 * 2)]


class B32RoomOverlay(C.Structure):
    _fields_ = [("sections", C.c_uint32), ("hover_source", C.c_uint32), ("hover", B32RoomHover), ("primary_vertex", C.c_uint32),
                ("skip_first", C.c_uint32), ("skip_count", C.c_uint32), ("n_vertices", C.c_uint32), ("n_edges", C.c_uint32),
                ("n_faces", C.c_uint32), ("n_points", C.c_uint32), ("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float)]


assert C.sizeof(B32RoomHover) == 48 and C.sizeof(B32RoomOverlay) == 100

# B32ObjectPart / B32ObjectItem (the world editor's object overlays from resident asset parts, b32_draw_object_overlays): kind = OBJECT_*
OBJECT_PART_HIDDEN = 1
OBJECT_WIRE, OBJECT_BOX_MESH, OBJECT_BOX = range(3)
OBJECT_BOX_SLOTS = 12
OBJECT_PART_DTYPE = np.dtype([("slot", "<u8"), ("topology", "<u8"), ("flags", "<u4"), ("_pad", "<u4")])
OBJECT_ITEM_DTYPE = np.dtype([("cos_f", "<f4"), ("sin_f", "<f4"), ("world_pos", "<f4", 3), ("first_part", "<u4"), ("n_parts", "<u4"),
                              ("box_min", "<f4", 3), ("box_max", "<f4", 3), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("blend", "u1"),
                              ("kind", "u1"), ("_pad", "u1", 3)])
assert OBJECT_PART_DTYPE.itemsize == 24 and OBJECT_ITEM_DTYPE.itemsize == 60
SCENE_BOUNDS_DTYPE = np.dtype([("min", "<f4", 3), ("max", "<f4", 3), ("has_verts", "<u4"), ("_pad", "<u4")])     # b32_scene_bounds_async's 32 bytes
assert SCENE_BOUNDS_DTYPE.itemsize == 32

# B32PickHit (b32_pick_meshes): hit == 0 -> tri = 0xFFFFFFFF, depth = 0
PICK_HIT_DTYPE = np.dtype([("hit", "<u4"), ("tri", "<u4"), ("depth", "<f4"), ("_pad", "<u4")])
assert PICK_HIT_DTYPE.itemsize == 16
PICK_CULL_BACKFACES = 1
PICK_HEADER_BYTES = 16              # b32_pick_meshes_async's result: {int32 best; uint32 n; 8 bytes of padding}, then n B32PickHit
PICK_NO_TRI = 0xFFFFFFFF
# B32HoverParams / B32HoverResult (b32_hover_mesh) and B32BoxParams (b32_box_select)
HOVER_PARAMS_DTYPE = np.dtype([("mx", "<f4"), ("my", "<f4"), ("vertex_threshold", "<f4"), ("edge_threshold", "<f4"), ("flags", "<u4"),
                               ("mirror_axis", "<u4"), ("mirror_threshold", "<f4"), ("_pad", "<u4")])
HOVER_RESULT_DTYPE = np.dtype([("vertex", "<u4"), ("vertex_dist", "<f4"), ("edge_v0", "<u4"), ("edge_v1", "<u4"), ("edge_dist", "<f4"),
                               ("face", "<u4"), ("face_depth", "<f4"), ("_pad", "<u4")])
BOX_PARAMS_DTYPE = np.dtype([("x0", "<f4"), ("y0", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("mode", "<u4"), ("_pad", "<u4", 3)])
assert HOVER_PARAMS_DTYPE.itemsize == 32 and HOVER_RESULT_DTYPE.itemsize == 32 and BOX_PARAMS_DTYPE.itemsize == 32
HOVER_SEE_THROUGH = 1
HOVER_NONE = 0xFFFFFFFF
HOVER_VERTEX_THRESHOLD, HOVER_EDGE_THRESHOLD = 6.0, 4.0      # viewport.rs:2428-2429
BOX_VERTICES, BOX_POLYGONS = 0, 1
BOX_HEADER_BYTES = 16               # b32_box_select_async's result: {uint32 n_elements; uint32 n_selected; 8 bytes of padding}, then the words
# B32SectorFace / B32RoomGrid / B32RoomHoverParams / B32RoomHover (b32_room, b32_room_hover, b32_room_box_select)
SECTOR_FACE_DTYPE = np.dtype([("gx", "<u2"), ("gz", "<u2"), ("kind", "u1"), ("index", "u1"), ("_pad", "<u2"), ("heights", "<f4", 4)])
ROOM_GRID_DTYPE = np.dtype([("position", "<f4", 3), ("sector_size", "<f4")])
ROOM_HOVER_PARAMS_DTYPE = np.dtype([("mx", "<f4"), ("my", "<f4"), ("vertex_threshold", "<f4"), ("edge_threshold", "<f4")])
ROOM_HOVER_DTYPE = np.dtype([("vertex_rec", "<u4"), ("vertex_corner", "<u4"), ("vertex_dist", "<f4"), ("vertex_depth", "<f4"),
                             ("edge_rec", "<u4"), ("edge_idx", "<u4"), ("edge_dist", "<f4"), ("edge_depth", "<f4"),
                             ("face_rec", "<u4"), ("face_depth", "<f4"), ("_pad", "<u4", 2)])
assert SECTOR_FACE_DTYPE.itemsize == 24 and ROOM_GRID_DTYPE.itemsize == 16 and ROOM_HOVER_PARAMS_DTYPE.itemsize == 16 and ROOM_HOVER_DTYPE.itemsize == 48
# B32FaceMaterial (b32_room_set_materials, b32_room_build_mesh): one per B32SectorFace; flags = MAT_HAS_*
FACE_MATERIAL_DTYPE = np.dtype([("texture_id", "<u4"), ("tex_width", "<u4"), ("texture_id_2", "<u4"), ("tex_width_2", "<u4"),
                                ("uv", "<f4", (4, 2)), ("uv_2", "<f4", (4, 2)), ("colors", "u1", (4, 4)), ("colors_2", "u1", (4, 4)),
                                ("heights_2", "<f4", 4), ("normal_mode", "u1"), ("split_direction", "u1"), ("uv_projection", "u1"),
                                ("blend_mode", "u1"), ("black_transparent", "u1"), ("flags", "u1"), ("_pad", "u1", 2)])
assert FACE_MATERIAL_DTYPE.itemsize == 136
MAT_HAS_UV, MAT_HAS_UV_2, MAT_HAS_HEIGHTS_2 = 1, 2, 4
NORMAL_FRONT, NORMAL_BOTH, NORMAL_BACK = range(3)
SPLIT_NWSE, SPLIT_NESW = range(2)
UV_DEFAULT, UV_PROJECTED = range(2)
ROOM_FLOOR, ROOM_CEILING, ROOM_WALL_NORTH, ROOM_WALL_EAST, ROOM_WALL_SOUTH, ROOM_WALL_WEST, ROOM_WALL_NWSE, ROOM_WALL_NESW = range(8)
SECTOR_SIZE = 1024.0                # world/geometry.rs:10
ROOM_MAX_FACES = 1 << 24
ROOM_VERTEX_THRESHOLD, ROOM_EDGE_THRESHOLD = 6.0, 4.0        # viewport_3d.rs:7038-7039
# B32Bone (b32_scene_pose): get_bone_world_transform(i) with cos / sin taken on the host; rotate == 0: rotate_by_euler's early return
BONE_DTYPE = np.dtype([("pos", "<f4", 3), ("cos_x", "<f4"), ("sin_x", "<f4"), ("cos_z", "<f4"), ("sin_z", "<f4"), ("rotate", "<u4")])
assert BONE_DTYPE.itemsize == 32
BONE_NONE = 0xFFFF
MAX_BONES = 64
# B32VertexPatch / B32FacePatch (b32_scene_patch_vertices / _faces): the element's index, then the whole record
VERTEX_PATCH_DTYPE = np.dtype([("index", "<u4"), ("v", VERTEX_DTYPE)])
FACE_PATCH_DTYPE = np.dtype([("index", "<u4"), ("f", FACE_DTYPE)])
assert VERTEX_PATCH_DTYPE.itemsize == 40 and FACE_PATCH_DTYPE.itemsize == 24
# B32SkelBone / B32SkeletonStyle (b32_scene_build_skeleton, b32_skeleton_items): what the bone octahedra read per bone, and the editor state
SKEL_BONE_DTYPE = np.dtype([("pos", "<f4", 3), ("cos_x", "<f4"), ("sin_x", "<f4"), ("cos_z", "<f4"), ("sin_z", "<f4"), ("length", "<f4"),
                            ("width", "<f4"), ("parent", "<u4")])
SKELETON_STYLE_DTYPE = np.dtype([("selected_bone", "<i4"), ("hovered_bone", "<i4"), ("hovered_tip", "<i4"), ("mode", "<u4"), ("editor_alpha", "u1"),
                                 ("has_preview", "u1"), ("_pad", "u1", 2), ("preview_start", "<f4", 3), ("preview_end", "<f4", 3)])
assert SKEL_BONE_DTYPE.itemsize == 40 and SKELETON_STYLE_DTYPE.itemsize == 44
SKELETON_TRIANGLES, SKELETON_FROM_BONES = 0, 1
# B32Mirror (b32_scene_build_mirror, b32_mirror_counts): the selected object's vertex and face ranges inside the source's body
MIRROR_DTYPE = np.dtype([("axis", "<u4"), ("dim", "<f4"), ("v_first", "<u4"), ("v_count", "<u4"), ("f_first", "<u4"), ("f_count", "<u4"),
                         ("_pad", "<u4", 2)])
assert MIRROR_DTYPE.itemsize == 32
MIRROR_X, MIRROR_Y, MIRROR_Z = 1, 2, 3
MIRROR_DIM = 0.85                   # viewport.rs:1273
SKY_VERTEX_DTYPE = np.dtype([("pos", np.float32, 3), ("r", np.uint8), ("g", np.uint8), ("b", np.uint8), ("blend", np.uint8)])
# B32Star (b32_draw_stars): what draw_star_diamond is called with -- the cast screen point and the twinkled colour
STAR_DTYPE = np.dtype([("cx", "<i4"), ("cy", "<i4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("_pad", "u1")])
assert SKY_VERTEX_DTYPE.itemsize == 16 and STAR_DTYPE.itemsize == 12
STAR_MAX = (2**31 - 1) // 9         # more stars than this: B32_E_UNSUPPORTED


class B32IndexedTexture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("blend_mode", C.c_uint32), ("clut_len", C.c_uint32),
                ("indices", C.c_void_p), ("clut", C.c_void_p)]


class B32Camera(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("basis_x", C.c_float * 3), ("basis_y", C.c_float * 3),
                ("basis_z", C.c_float * 3)]


class B32Ortho(C.Structure):
    _fields_ = [("zoom", C.c_float), ("center_x", C.c_float), ("center_y", C.c_float)]


class B32Light(C.Structure):
    _fields_ = [("type", C.c_uint32), ("position", C.c_float * 3), ("direction", C.c_float * 3),
                ("radius", C.c_float), ("angle", C.c_float), ("intensity", C.c_float),
                ("r", C.c_uint8), ("g", C.c_uint8), ("b", C.c_uint8), ("enabled", C.c_uint8)]


class B32Settings(C.Structure):
    _fields_ = [("affine_textures", C.c_uint8), ("use_zbuffer", C.c_uint8), ("shading", C.c_uint8),
                ("backface_cull", C.c_uint8), ("backface_wireframe", C.c_uint8), ("dithering", C.c_uint8),
                ("wireframe_overlay", C.c_uint8), ("use_rgb555", C.c_uint8), ("use_fixed_point", C.c_uint8),
                ("xray_mode", C.c_uint8), ("has_ortho", C.c_uint8), ("_pad", C.c_uint8),
                ("ambient", C.c_float), ("ortho_zoom", C.c_float), ("ortho_center_x", C.c_float),
                ("ortho_center_y", C.c_float), ("n_lights", C.c_uint32), ("lights", C.c_void_p)]


class B32Fog(C.Structure):
    _fields_ = [("start", C.c_float), ("falloff", C.c_float), ("cull_distance", C.c_float),
                ("r", C.c_uint8), ("g", C.c_uint8), ("b", C.c_uint8), ("blend", C.c_uint8)]


class B32MeshParams(C.Structure):
    _fields_ = [("ambient", C.c_float), ("backface_cull", C.c_uint8), ("backface_wireframe", C.c_uint8), ("has_fog", C.c_uint8),
                ("_pad", C.c_uint8), ("fog", B32Fog)]


class B32Placement(C.Structure):
    _fields_ = [("cos_f", C.c_float), ("sin_f", C.c_float), ("world_pos", C.c_float * 3)]


assert C.sizeof(B32Placement) == 20


class B32Timings(C.Structure):
    _fields_ = [("transform_ms", C.c_float), ("fog_ms", C.c_float), ("cull_ms", C.c_float), ("sort_ms", C.c_float),
                ("draw_ms", C.c_float), ("wireframe_ms", C.c_float), ("triangles_drawn", C.c_uint32),
                ("tile_pairs", C.c_uint32), ("fragments", C.c_uint64)]


# Every symbol include/b32raster.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("b32_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("b32_destroy", None, [_P]),
    ("b32_strerror", C.c_char_p, [C.c_int]),
    ("b32_last_hip_error", C.c_int, [_P]),
    ("b32_set_stream", C.c_int, [_P, _P]),
    ("b32_synchronize", C.c_int, [_P]),
    ("b32_fb_resize", C.c_int, [_P, C.c_uint32, C.c_uint32]),
    ("b32_fb_new", C.c_int, [_P, C.c_uint32, C.c_uint32]),
    ("b32_set_async_depth", C.c_int, [_P, C.c_int]),
    ("b32_route_count", C.c_ulonglong, [_P, C.c_int]),
    ("b32_set_routes", C.c_int, [_P, C.c_uint32]),
    ("b32_set_cheap_threshold", C.c_int, [_P, C.c_uint32]),
    ("b32_fb_clear", C.c_int, [_P, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint8]),
    ("b32_fb_upload", C.c_int, [_P, _P]),
    ("b32_fb_download", C.c_int, [_P, _P]),
    ("b32_host_alloc", C.c_void_p, [C.c_size_t]),
    ("b32_host_free", None, [C.c_void_p]),
    ("b32_fb_download_async", C.c_int, [_P, _P, C.POINTER(C.c_uint64)]),
    ("b32_ticket_poll", C.c_int, [_P, C.c_uint64, C.POINTER(C.c_int)]),
    ("b32_ticket_wait", C.c_int, [_P, C.c_uint64]),
    ("b32_zbuffer_download", C.c_int, [_P, _P]),
    ("b32_zbuffer_upload", C.c_int, [_P, _P]),
    ("b32_fb_bind_device", C.c_int, [_P, _P, C.c_uint32, C.c_uint32]),
    ("b32_fb_size", C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("b32_set_band", C.c_int, [_P, C.c_uint32, C.c_uint32]),
    ("b32_render_mesh_15", C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _P, _P, _P, _P]),
    ("b32_scene_upload", C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32]),
    ("b32_scene_upload_indexed", C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32]),
    ("b32_render_scene_15", C.c_int, [_P, _P, _P, _P, _P]),
    ("b32_render_scene_15_async", C.c_int, [_P, _P, _P, _P]),
    ("b32_frame_finish", C.c_int, [_P, _P]),
    ("b32_scene_create", C.c_int, [_P, C.POINTER(_P)]),
    ("b32_scene_destroy", None, [_P, _P]),
    ("b32_scene_swap", C.c_int, [_P, _P]),
    ("b32_scene_set_rig", C.c_int, [_P, _P, _P]),
    ("b32_scene_pose", C.c_int, [_P, _P, _P, C.c_uint32]),
    ("b32_scene_read_vertices", C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P]),
    ("b32_scene_patch_vertices", C.c_int, [_P, _P, _P, C.c_uint32]),
    ("b32_scene_patch_faces", C.c_int, [_P, _P, _P, C.c_uint32]),
    ("b32_scene_patch_texels", C.c_int, [_P, _P] + [C.c_uint32] * 5 + [_P, C.c_uint32]),
    ("b32_scene_patch_indexed", C.c_int, [_P, _P] + [C.c_uint32] * 5 + [_P, C.c_uint32, _P, C.c_uint32]),
    ("b32_scene_read_texels", C.c_int, [_P, _P, C.c_uint32, _P]),
    ("b32_scene_build_skeleton", C.c_int, [_P, _P, _P, C.c_uint32, _P]),
    ("b32_skeleton_counts", C.c_int, [_P, C.c_uint32, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("b32_skeleton_items", C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("b32_scene_build_mirror", C.c_int, [_P, _P, _P, _P]),
    ("b32_mirror_counts", C.c_int, [C.c_uint32, C.c_uint32, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("b32_frame_begin", C.c_int, [_P, _P, _P]),
    ("b32_frame_add_scene", C.c_int, [_P, _P, _P]),
    ("b32_frame_end", C.c_int, [_P]),
    ("b32_frame_submit", C.c_int, [_P, _P, _P, C.POINTER(_P), _P, C.c_uint32]),
    ("b32_batch_count", C.c_ulonglong, [_P, C.c_int]),
    ("b32_frame_add_scene_placed", C.c_int, [_P, _P, _P, _P]),
    ("b32_frame_submit_placed", C.c_int, [_P, _P, _P, C.POINTER(_P), _P, _P, _P, C.c_uint32]),
    ("b32_render_scene_15_placed_async", C.c_int, [_P, _P, _P, _P, _P]),
    ("b32_pick_meshes", C.c_int, [_P, _P, _P, C.c_float, C.c_float, C.c_uint32, C.POINTER(_P), _P, C.c_uint32, _P, C.POINTER(C.c_int32)]),
    ("b32_pick_meshes_async", C.c_int, [_P, _P, _P, C.c_float, C.c_float, C.c_uint32, C.POINTER(_P), _P, C.c_uint32, _P, C.POINTER(C.c_uint64)]),
    ("b32_topology_create", C.c_int, [_P, _P, C.c_uint32, _P, C.POINTER(_P)]),
    ("b32_topology_destroy", None, [_P, _P]),
    ("b32_hover_mesh", C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    ("b32_hover_mesh_async", C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint64)]),
    ("b32_box_select", C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint32)]),
    ("b32_box_select_async", C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint64)]),
    ("b32_room_create", C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(_P)]),
    ("b32_room_update", C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P]),
    ("b32_room_destroy", None, [_P, _P]),
    ("b32_room_set_materials", C.c_int, [_P, _P, _P]),
    ("b32_room_update_materials", C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P]),
    ("b32_room_mesh_counts", C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("b32_room_build_mesh", C.c_int, [_P, _P, _P]),
    ("b32_scene_read_faces", C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P]),
    ("b32_room_hover", C.c_int, [_P, _P, _P, _P, _P]),
    ("b32_room_hover_async", C.c_int, [_P, _P, _P, _P, _P, C.POINTER(C.c_uint64)]),
    ("b32_room_hover_winner", C.c_int, [_P]),
    ("b32_room_box_select", C.c_int, [_P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, _P, C.c_uint32, _P, C.POINTER(C.c_uint32)]),
    ("b32_room_box_select_async", C.c_int, [_P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, _P, C.c_uint32, _P, C.POINTER(C.c_uint64)]),
    ("b32_fb_clear_gradient", C.c_int, [_P] + [C.c_uint8] * 8),
    ("b32_fb_clear_transparent", C.c_int, [_P]),
    ("b32_render_skybox_mesh", C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, _P]),
    ("b32_draw_star_diamonds", C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_float]),
    ("b32_sky_create", C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(_P)]),
    ("b32_sky_destroy", None, [_P, _P]),
    ("b32_sky_update", C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P]),
    ("b32_render_sky", C.c_int, [_P, _P, _P]),
    ("b32_sky_project_batch", C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P]),
    ("b32_draw_stars", C.c_int, [_P, _P, C.c_uint32, C.c_float]),
    ("b32_star_record_count", C.c_int, [C.c_uint32, C.c_float, C.POINTER(C.c_uint64)]),
    ("b32_star_records_batch", C.c_int, [_P, _P, C.c_uint32, C.c_float, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("b32_present_nearest", C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    ("b32_draw_lines", C.c_int, [_P, _P, C.c_uint32]),
    ("b32_draw_prims", C.c_int, [_P, _P, C.c_uint32]),
    ("b32_draw_world", C.c_int, [_P, _P, _P, _P, C.c_uint32]),
    ("b32_draw_floor_grid", C.c_int, [_P, _P, C.c_float, C.c_float, C.c_float, _P, _P, _P]),
    ("b32_floor_grid_items", C.c_int, [C.c_float, C.c_float, C.c_float, _P, _P, _P, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("b32_world_project_batch", C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P]),
    ("b32_world_counts", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("b32_draw_gizmos", C.c_int, [_P, _P, _P, _P, C.c_uint32]),
    ("b32_gizmo_project_batch", C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("b32_gizmo_counts", C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("b32_octahedron_items", C.c_int, [_P, C.c_float, _P, _P]),
    ("b32_draw_mesh_overlay", C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    ("b32_mesh_overlay_project_batch", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("b32_mesh_overlay_record_count", C.c_int, [_P, C.c_uint32, _P, _P, C.POINTER(C.c_uint32)]),
    ("b32_draw_room_overlay", C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    ("b32_room_overlay_project_batch", C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("b32_room_overlay_record_count", C.c_int, [_P, _P, _P, _P, C.POINTER(C.c_uint32)]),
    ("b32_draw_object_overlays", C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32]),
    ("b32_object_overlay_project_batch", C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("b32_object_overlay_record_count", C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("b32_scene_bounds", C.c_int, [_P, _P, _P, _P, C.POINTER(C.c_uint32)]),
    ("b32_scene_bounds_async", C.c_int, [_P, _P, _P, C.POINTER(C.c_uint64)]),
    ("b32_render_mesh", C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, _P, _P, _P]),
    ("b32_scene_upload_rgba", C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32]),
    ("b32_render_scene", C.c_int, [_P, _P, _P, _P]),
    ("b32_render_scene_async", C.c_int, [_P, _P, _P]),
    ("b32_project_fixed_batch", C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, _P, _P]),
    ("b32_last_draw_order", C.c_int, [_P, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("b32_last_surface_shading", C.c_int, [_P, _P, _P, _P, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("b32_selftest_f32", C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_uint32]),
    ("b32_last_kernel_times", C.c_int, [_P, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_uint32]),
    ("b32_device_constants", C.c_int, [_P, C.POINTER(C.c_char_p), _P, _P, C.c_uint32, C.POINTER(C.c_uint32), _P, _P]),
    ("b32_set_profiling", C.c_int, [_P, C.c_int]),
    ("b32_set_profiling_stride", C.c_int, [_P, C.c_uint32]),
    ("b32_set_pipeline_gate", C.c_int, [_P, C.c_uint32]),
    ("b32_set_pipeline_depth", C.c_int, [_P, C.c_uint32]),
    ("b32_last_shader_clock", C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("b32_transparent_counts", C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("b32_set_fragment_counting", C.c_int, [_P, C.c_int]),
    ("b32_debug_inject", C.c_int, [_P, C.c_uint32]),
    ("b32_build_digest", C.c_char_p, []),
    ("b32_band_export", C.c_int, [_P, C.c_void_p]),
    ("b32_band_import", C.c_int, [_P, C.c_void_p, C.c_uint32]),
    ("b32_band_attach", C.c_int, [_P, _P, C.c_uint32]),
    ("b32_band_close", C.c_int, [_P]),
    ("b32_band_publish", C.c_int, [_P, C.c_uint32]),
    ("b32_band_wait", C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("b32_band_release", C.c_int, [_P, C.c_uint32]),
    ("b32_band_wait_all", C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]),
    ("b32_band_acquire", C.c_int, [_P, C.c_uint32, C.c_uint32]),
    ("b32_band_status", C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("b32_gather_bands_rccl", C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("b32_gather_bands_rccl_loopback", C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]),
    ("b32_rccl_unique_id", C.c_int, [C.c_void_p]),
    ("b32_rccl_comm_create", C.c_int, [_P, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("b32_rccl_comm_destroy", C.c_int, [C.c_void_p]),
]

_lib = None


def load_library(path=None):
    """dlopen libb32raster.so and type every entry point. Raises if the library was not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("B32_LIB") or LIB_PATH          # B32_LIB: an experiment build (tools/exp_variants.py); never set by the product
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} is missing: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()'). "
            "The bonnie-32 rasterizer path has no CPU fallback.")
    lib = C.CDLL(p)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    if path is None:
        _lib = lib
    return lib


def check_build_digest(lib=None):
    """The loaded library must have been compiled from THIS source tree (b32_build_digest() == build.csrc_digest()): a stale .so that
    travelled with the snapshot would otherwise be timed / tested in place of the sources next to it.  Returns the digest.  An
    experiment build named by B32_LIB (tools/exp_variants.py) is exempt: it is never the product."""
    from . import build as B
    lib = lib or load_library()
    have = (lib.b32_build_digest() or b"").decode("ascii", "replace")
    want = B.csrc_digest()
    if have != want and not os.environ.get("B32_LIB"):
        raise RuntimeError(f"libb32raster.so was built from other sources (library {have}, tree {want}): run __graft_entry__.build()")
    return have


def ptr(a):
    """Address of a C-contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data
