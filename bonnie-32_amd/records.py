"""Value types and packers: what turns caller input into the records and structs of the C ABI (abi.py).  Imports neither mirrors/ nor the
binding, and loads no library at import: Topology.handle reaches it through its `ctx`, octahedron_items (host only) at the call."""
import ctypes as C

import numpy as np

from . import abi
from . import rtypes as T


class B32Error(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        msg = abi.load_library().b32_strerror(code).decode()
        super().__init__(f"{where}: {msg} (code {code})" if where else f"{msg} (code {code})")


def _chk(rc, where=""):
    if rc != abi.B32_OK:
        raise B32Error(rc, where)


def _positions(vertices):
    """(n, 3) f32 positions of an abi.VERTEX_DTYPE array or of anything that already is one."""
    return np.ascontiguousarray(vertices["pos"] if getattr(vertices, "dtype", None) is not None and vertices.dtype.names else vertices, np.float32).reshape(-1, 3)


def place_vertices(vertices, cos_f, sin_f, world_pos):
    """The per-vertex arithmetic of render_asset_parts (scene.rs:140-156) in numpy float32: rotate about Y by (cos_f, sin_f), then
    translate by world_pos; normals are rotated and not renormalised; uv and colour are unchanged.  Every operation is one separately
    rounded f32 operation in the reference's order (numpy does not fuse).  This is what a caller without a GPU does per object and per
    frame, and what the tests hand to the oracle; on the device the same arithmetic runs inside the setup kernel (B32Placement)."""
    v = np.array(vertices, dtype=abi.VERTEX_DTYPE, copy=True)
    c, s = np.float32(cos_f), np.float32(sin_f)
    w = np.asarray(world_pos, np.float32).reshape(3)
    with np.errstate(all="ignore"):
        x, y, z = v["pos"][:, 0].copy(), v["pos"][:, 1].copy(), v["pos"][:, 2].copy()
        rx = x * c - z * s
        rz = x * s + z * c
        v["pos"][:, 0] = rx + w[0]; v["pos"][:, 1] = y + w[1]; v["pos"][:, 2] = rz + w[2]
        nx, nz = v["normal"][:, 0].copy(), v["normal"][:, 2].copy()
        v["normal"][:, 0] = nx * c - nz * s
        v["normal"][:, 2] = nx * s + nz * c
    return v


class Placement:
    """facing + world offset of one placed object (render_asset_parts, scene.rs:112-159).  Placement(facing=..., world_pos=...) takes
    cos / sin in f32 on the host and decides `has_transform` as scene.rs:125 does (|facing| or any |world_pos| component above 0.0001,
    compared in f32); without a transform the reference draws the local vertices as they are, so pack() is None -- "draw exactly as
    without a placement".  Placement(cos_f=..., sin_f=..., world_pos=...) takes the caller's own cos / sin (Rust's f32::cos is the
    target's libm and may differ from numpy's in the last bit) and always transforms unless has_transform says otherwise."""

    def __init__(self, facing=None, world_pos=(0.0, 0.0, 0.0), cos_f=None, sin_f=None, has_transform=None):
        f32 = np.float32
        self.world_pos = tuple(f32(x) for x in world_pos)
        if (cos_f is None) != (sin_f is None) or (facing is None and cos_f is None):
            raise ValueError("Placement needs facing, or cos_f and sin_f")
        if cos_f is None:
            self.cos_f, self.sin_f = f32(np.cos(f32(facing))), f32(np.sin(f32(facing)))
        else:
            self.cos_f, self.sin_f = f32(cos_f), f32(sin_f)
        if has_transform is None:
            eps = f32(0.0001)
            has_transform = True if facing is None else bool(abs(f32(facing)) > eps or any(abs(x) > eps for x in self.world_pos))
        self.has_transform = bool(has_transform)

    def pack(self):
        """abi.B32Placement, or None when the reference takes its untransformed branch."""
        if not self.has_transform:
            return None
        return _pack_triple(self)

    def apply(self, vertices):
        """The vertices render_asset_parts hands to render_mesh_15 / render_mesh for this placement (host restatement)."""
        if not self.has_transform:
            return np.array(vertices, dtype=abi.VERTEX_DTYPE, copy=True)
        return place_vertices(vertices, self.cos_f, self.sin_f, self.world_pos)


def _placement_triple(placement):
    """(cos_f, sin_f, world_pos) as f32 of a Placement, an abi.B32Placement or such a triple.  Picking always applies the placement
    (viewport_3d.rs:7716-7718 has no has_transform shortcut), so Placement.has_transform is not consulted."""
    f32 = np.float32
    if isinstance(placement, (Placement, abi.B32Placement)):
        c, s, w = placement.cos_f, placement.sin_f, tuple(placement.world_pos)
    else:
        c, s, w = placement
    return f32(c), f32(s), tuple(f32(x) for x in w)


def _pack_triple(placement):
    """The abi.B32Placement of whatever _placement_triple reads: always a transform."""
    c, s, w = _placement_triple(placement)
    return abi.B32Placement(float(c), float(s), (C.c_float * 3)(*[float(x) for x in w]))


def _pack_placement(placement):
    """A draw's placement as the library takes it: None and an abi.B32Placement as they are, a Placement by its pack() (None: no transform)."""
    if placement is None or isinstance(placement, abi.B32Placement):
        return placement
    return placement.pack()


def _pack_ortho(ortho):
    if ortho is None:
        return None
    zoom, cx, cy = ortho
    return abi.B32Ortho(float(zoom), float(cx), float(cy))


# ---- bones (b32_scene_set_rig, b32_scene_pose): the modeler's rotate_by_euler(v.pos, bone_rot) + bone_pos
_RADS_PER_DEG = np.float32(np.pi / 180.0)                  # f32::to_radians: self * (consts::PI / 180.0)


class Bone:
    """get_bone_world_transform(i) (modeler/state.rs:2585-2614) as the device takes it: bone_pos, cos / sin of bone_rot.x and .z in
    radians, and `rotate` -- False where rotate_by_euler (state.rs:30-54) takes its early return and hands the vector back as it is.
    Bone.from_euler(pos, rot_deg) takes to_radians as x * f32(pi / 180), cos / sin in f32, and decides `rotate` with the reference's
    test (|rot.x| < 0.001 && |rot.z| < 0.001, strict, in f32).  Bone(pos, cos_x=..., sin_x=..., cos_z=..., sin_z=...) takes the caller's own
    libm values (Rust's f32::cos is the target's libm and may differ from numpy's in the last bit), as Placement does."""

    def __init__(self, pos=(0.0, 0.0, 0.0), cos_x=1.0, sin_x=0.0, cos_z=1.0, sin_z=0.0, rotate=True):
        f32 = np.float32
        self.pos = tuple(f32(x) for x in pos)
        self.cos_x, self.sin_x, self.cos_z, self.sin_z = f32(cos_x), f32(sin_x), f32(cos_z), f32(sin_z)
        self.rotate = bool(rotate)

    @classmethod
    def from_euler(cls, pos, rot_deg):
        f32 = np.float32
        rx, rz = f32(rot_deg[0]), f32(rot_deg[2])
        if abs(rx) < f32(0.001) and abs(rz) < f32(0.001):
            return cls(pos, rotate=False)
        ax, az = rx * _RADS_PER_DEG, rz * _RADS_PER_DEG
        return cls(pos, cos_x=np.cos(ax), sin_x=np.sin(ax), cos_z=np.cos(az), sin_z=np.sin(az), rotate=True)

    def record(self):
        r = np.zeros((), abi.BONE_DTYPE)
        r["pos"] = self.pos
        r["cos_x"], r["sin_x"], r["cos_z"], r["sin_z"] = self.cos_x, self.sin_x, self.cos_z, self.sin_z
        r["rotate"] = 1 if self.rotate else 0
        return r


def _pack_table(rows, dtype):
    """A table as a contiguous array of `dtype`: from such an array, or from a sequence of objects with a record() of it."""
    if isinstance(rows, np.ndarray) and rows.dtype == dtype:
        return np.ascontiguousarray(rows).reshape(-1)
    out = np.zeros(len(rows), dtype)
    for i, b in enumerate(rows):
        out[i] = b.record()
    return out


def pack_bones(bones):
    """A bone table as a contiguous abi.BONE_DTYPE array: from such an array, or from a sequence of Bone."""
    return _pack_table(bones, abi.BONE_DTYPE)


# ---- the bone octahedra (b32_scene_build_skeleton, b32_skeleton_items): skeleton_to_triangles / draw_skeleton / draw_bone_dots
class SkelBone:
    """What the reference reads per bone when it draws the skeleton (modeler/skeleton.rs:412-477, state.rs:2629-2638): the position of
    get_bone_world_transform(i), cos / sin of the WORLD rotation's .x and .z in radians (always read: get_bone_tip_position has no early
    return), length, width = display_width() and the parent (None: a root).  SkelBone.from_rig(pos, rot_deg, length, width, parent) takes
    to_radians as x * f32(pi / 180), cos / sin in f32 and resolves display_width (state.rs:369-375: width > 0 ? width :
    (length * 0.15).clamp(20, 200)).  SkelBone(pos, cos_x=..., ...) takes the caller's own libm values, as Bone does."""

    def __init__(self, pos=(0.0, 0.0, 0.0), cos_x=1.0, sin_x=0.0, cos_z=1.0, sin_z=0.0, length=20.0, width=40.0, parent=None):
        f32 = np.float32
        self.pos = tuple(f32(x) for x in pos)
        self.cos_x, self.sin_x, self.cos_z, self.sin_z = f32(cos_x), f32(sin_x), f32(cos_z), f32(sin_z)
        self.length, self.width = f32(length), f32(width)
        self.parent = None if parent is None or parent < 0 else int(parent)

    @staticmethod
    def display_width(length, width):
        f32 = np.float32
        length, width = f32(length), f32(width)
        if width > f32(0.0):
            return width
        with np.errstate(all="ignore"):
            w = length * f32(0.15)
        return f32(20.0) if w < f32(20.0) else (f32(200.0) if w > f32(200.0) else w)        # f32::clamp: a NaN stays

    @classmethod
    def from_rig(cls, pos, rot_deg, length, width, parent=None):
        f32 = np.float32
        with np.errstate(all="ignore"):
            ax, az = f32(rot_deg[0]) * _RADS_PER_DEG, f32(rot_deg[2]) * _RADS_PER_DEG
            return cls(pos, cos_x=np.cos(ax), sin_x=np.sin(ax), cos_z=np.cos(az), sin_z=np.sin(az), length=length,
                       width=cls.display_width(length, width), parent=parent)

    def record(self):
        r = np.zeros((), abi.SKEL_BONE_DTYPE)
        r["pos"] = self.pos
        r["cos_x"], r["sin_x"], r["cos_z"], r["sin_z"] = self.cos_x, self.sin_x, self.cos_z, self.sin_z
        r["length"], r["width"] = self.length, self.width
        r["parent"] = abi.BONE_NONE if self.parent is None else self.parent
        return r


def pack_skel_bones(bones):
    """A skeleton as a contiguous abi.SKEL_BONE_DTYPE array: from such an array, or from a sequence of SkelBone."""
    return _pack_table(bones, abi.SKEL_BONE_DTYPE)


class SkeletonStyle:
    """The editor state the skeleton's colours depend on: selected_bone / hovered_bone / hovered_tip (None: none), editor_alpha, mode
    (abi.SKELETON_TRIANGLES: skeleton_to_triangles; abi.SKELETON_FROM_BONES: skeleton_to_triangles_from_bones -- root / default colours,
    editor_alpha on every bone, no preview) and the creation preview as (start, end) or None."""

    def __init__(self, selected_bone=None, hovered_bone=None, hovered_tip=None, editor_alpha=255, mode=abi.SKELETON_TRIANGLES, preview=None):
        self.selected_bone, self.hovered_bone, self.hovered_tip = selected_bone, hovered_bone, hovered_tip
        self.editor_alpha, self.mode, self.preview = int(editor_alpha), int(mode), preview

    def pack(self):
        r = np.zeros(1, abi.SKELETON_STYLE_DTYPE)
        for k in ("selected_bone", "hovered_bone", "hovered_tip"):
            v = getattr(self, k)
            r[k] = -1 if v is None or v < 0 else v
        r["mode"], r["editor_alpha"] = self.mode, self.editor_alpha
        if self.preview is not None:
            r["has_preview"] = 1
            r["preview_start"], r["preview_end"] = np.asarray(self.preview[0], np.float32), np.asarray(self.preview[1], np.float32)
        return r


class Mirror:
    """Mirror editing (MirrorSettings, modeler/state.rs:777-850) as b32_scene_build_mirror takes it: the axis (abi.MIRROR_X / _Y / _Z, or
    "x" / "y" / "z"), the selected object's vertices [v_first, v_first + v_count) and faces [f_first, f_first + f_count) inside the source's
    body, and the twins' colour factor (the reference's 0.85)."""
    AXES = {"x": abi.MIRROR_X, "y": abi.MIRROR_Y, "z": abi.MIRROR_Z}

    def __init__(self, axis=abi.MIRROR_X, v_first=0, v_count=0, f_first=0, f_count=0, dim=abi.MIRROR_DIM):
        self.axis = self.AXES[axis.lower()] if isinstance(axis, str) else int(axis)
        self.v_first, self.v_count, self.f_first, self.f_count = int(v_first), int(v_count), int(f_first), int(f_count)
        self.dim = np.float32(dim)

    def pack(self):
        r = np.zeros(1, abi.MIRROR_DTYPE)
        r["axis"], r["dim"] = self.axis, self.dim
        r["v_first"], r["v_count"], r["f_first"], r["f_count"] = self.v_first, self.v_count, self.f_first, self.f_count
        return r


def pack_mirror(mirror):
    """A mirror as a one-element abi.MIRROR_DTYPE array: from such an array (or record), or from a Mirror."""
    if isinstance(mirror, Mirror):
        return mirror.pack()
    return np.ascontiguousarray(mirror, abi.MIRROR_DTYPE).reshape(-1)[:1].copy()


class Topology:
    """The modeler's polygons over a slot's vertices (b32_topology): poly_start (np + 1, non-decreasing, [0] == 0) into poly_verts.  The
    constructor derives what b32_topology_create derives: the half-edges (v[k], v[(k + 1) % n]) in loop order (Face::edges,
    mesh_editor.rs:92-95) with the id of their normalised edge, and the fan triangles in loop order (Face::triangulate,
    mesh_editor.rs:99-112) with their polygon.  handle(ctx) is the device object (created on first use, released by close())."""

    def __init__(self, poly_start, poly_verts):
        self.poly_start = np.ascontiguousarray(poly_start, np.uint32).reshape(-1)
        self.poly_verts = np.ascontiguousarray(poly_verts, np.uint32).reshape(-1)
        if len(self.poly_start) < 1 or self.poly_start[0] != 0 or (np.diff(self.poly_start.astype(np.int64)) < 0).any() or int(self.poly_start[-1]) != len(self.poly_verts):
            raise ValueError("Topology: poly_start must start at 0, not decrease and end at len(poly_verts)")
        self.np = len(self.poly_start) - 1
        st = self.poly_start.astype(np.int64)
        self.count = np.diff(st)
        self.poly_of = np.repeat(np.arange(self.np, dtype=np.int64), self.count)       # polygon of every position of poly_verts
        k = np.arange(len(self.poly_verts), dtype=np.int64) - st[:-1][self.poly_of]
        pv = self.poly_verts.astype(np.int64)
        self.he_v0 = pv
        self.he_v1 = pv[st[:-1][self.poly_of] + (k + 1) % np.maximum(self.count[self.poly_of], 1)] if len(pv) else pv
        key = (np.minimum(self.he_v0, self.he_v1) << 32) | np.maximum(self.he_v0, self.he_v1)
        uniq, self.he_edge = np.unique(key, return_inverse=True) if len(pv) else (key, np.zeros(0, np.int64))
        self.ne = len(uniq)
        fan_poly = np.repeat(np.arange(self.np, dtype=np.int64), np.maximum(self.count - 2, 0))
        j = np.arange(len(fan_poly), dtype=np.int64) - np.concatenate([[0], np.cumsum(np.maximum(self.count - 2, 0))])[:-1][fan_poly] + 1
        base = st[:-1][fan_poly]
        self.fan = np.stack([pv[base], pv[base + j], pv[base + j + 1]], 1) if len(fan_poly) else np.zeros((0, 3), np.int64)
        self.fan_poly = fan_poly
        self._handles = []

    def first_half_edges(self):
        """Per half-edge: 1 + how many edges began before it when it is the first half-edge of its normalised edge in loop order, else 0
        (what b32_topology_create derives for the edge preview of b32_draw_mesh_overlay)."""
        first = np.zeros(len(self.poly_verts), np.int64)
        if self.ne:
            _, idx = np.unique(self.he_edge, return_index=True)
            first[np.sort(idx)] = np.arange(1, self.ne + 1)
        return first

    @classmethod
    def from_polygons(cls, polygons):
        """polygons: a list of vertex-index lists."""
        start = np.concatenate([[0], np.cumsum([len(p) for p in polygons])]).astype(np.uint32)
        verts = np.array([i for p in polygons for i in p], np.uint32)
        return cls(start, verts)

    @classmethod
    def triangles(cls, faces):
        """The trivial topology of a triangle list (FACE_DTYPE faces or an (n, 3) index array): poly_start = 0, 3, 6, ..."""
        fv = np.ascontiguousarray(faces["v"] if getattr(faces, "dtype", None) is not None and faces.dtype.names else faces, np.uint32).reshape(-1, 3)
        return cls(np.arange(len(fv) + 1, dtype=np.uint32) * 3, fv.reshape(-1))

    def handle(self, ctx):
        for c, h in self._handles:
            if c is ctx:
                return h
        h = C.c_void_p()
        _chk(ctx.lib.b32_topology_create(ctx.h, abi.ptr(self.poly_start), self.np, abi.ptr(self.poly_verts) if len(self.poly_verts) else None, C.byref(h)),
             "b32_topology_create")
        self._handles.append((ctx, h))
        return h

    def close(self):
        for c, h in self._handles:
            if getattr(c, "h", None):
                c.lib.b32_topology_destroy(c.h, h)
        self._handles = []


# ---- records of the tile pass and items of the device producers (b32_draw_prims, b32_draw_world, b32_draw_gizmos)
def prim(kind, x0, y0, x1, y1, color: T.Color, z0=0.0, z1=0.0, size=0, alpha=255, mode=0):
    """One abi.PRIM_DTYPE record."""
    p = np.zeros(1, abi.PRIM_DTYPE)
    p["x0"], p["y0"], p["x1"], p["y1"], p["z0"], p["z1"], p["size"] = x0, y0, x1, y1, z0, z1, size
    p["r"], p["g"], p["b"], p["blend"], p["kind"], p["alpha"], p["mode"] = color.r, color.g, color.b, color.blend, kind, alpha, mode
    return p


def pack_sky_vertices(vertices):
    """abi.SKY_VERTEX_DTYPE records (b32_sky_create, b32_sky_update) of a structured array as it is."""
    return np.ascontiguousarray(vertices, abi.SKY_VERTEX_DTYPE).reshape(-1)


def pack_stars(stars, cy=None, rgb=None):
    """abi.STAR_DTYPE records (b32_draw_stars): a structured array as it is, or the three arrays draw_star_diamonds takes (cx, cy, rgb)."""
    if cy is None:
        return np.ascontiguousarray(stars, abi.STAR_DTYPE).reshape(-1)
    cx = np.asarray(stars, np.int32).reshape(-1)
    c = np.asarray(rgb, np.uint8).reshape(-1, 3)
    s = np.zeros(len(cx), abi.STAR_DTYPE)
    s["cx"], s["cy"] = cx, np.asarray(cy, np.int32).reshape(-1)
    s["r"], s["g"], s["b"] = c[:, 0], c[:, 1], c[:, 2]
    return s


def noop_prims(n):
    """n records that draw nothing (a circle of radius -1): what a call the reference does not make leaves in its place."""
    r = np.zeros(n, abi.PRIM_DTYPE)
    r["kind"], r["size"] = abi.PRIM_CIRCLE, -1
    return r


def world_item(kind, p0, p1, color: T.Color, size=0, alpha=255, mode=0, flags=0):
    """One abi.WORLD_ITEM_DTYPE record."""
    it = np.zeros(1, abi.WORLD_ITEM_DTYPE)
    it["p0"], it["p1"], it["size"] = np.asarray(p0, np.float32), np.asarray(p1, np.float32), size
    it["r"], it["g"], it["b"], it["blend"] = color.r, color.g, color.b, color.blend
    it["kind"], it["alpha"], it["mode"], it["flags"] = kind, alpha, mode, flags
    return it


def floor_grid_items(y, spacing, extent, grid_color: T.Color, x_axis_color: T.Color, z_axis_color: T.Color):
    """The segments of draw_floor_grid (draw.rs:81-135) in call order, as LINE_2D items with WORLD_CLIP_NEAR: what b32_floor_grid_items
    builds in the library.  ValueError where the reference would not terminate; more than 2^20 segments: OverflowError."""
    f32 = np.float32
    y, spacing, extent = f32(y), f32(spacing), f32(extent)
    if not (np.isfinite(y) and np.isfinite(spacing) and np.isfinite(extent) and spacing > 0):
        raise ValueError("draw_floor_grid does not terminate for these arguments")
    rows = []
    for pas in (0, 1):                                            # 0: X-parallel lines (fixed Z), 1: Z-parallel lines (fixed X)
        u = -extent
        while u <= extent:
            col = ((z_axis_color if pas == 0 else x_axis_color) if abs(u) < f32(0.001) else grid_color)
            v = -extent
            while v < extent:
                v_end = min(f32(v + spacing), extent)
                if len(rows) >= 1 << 20:
                    raise OverflowError("more than 2^20 floor grid segments")
                rows.append(((v, y, u), (v_end, y, u), col) if pas == 0 else ((u, y, v), (u, y, v_end), col))
                nxt = f32(v + spacing)
                if not nxt > v:
                    raise ValueError("draw_floor_grid does not terminate: x + spacing == x")
                v = nxt
            nxt = f32(u + spacing)
            if not nxt > u:
                raise ValueError("draw_floor_grid does not terminate: z + spacing == z")
            u = nxt
    items = np.zeros(len(rows), abi.WORLD_ITEM_DTYPE)
    if rows:
        items["p0"] = np.array([r[0] for r in rows], f32); items["p1"] = np.array([r[1] for r in rows], f32)
        for f in ("r", "g", "b", "blend"):
            items[f] = [getattr(r[2], f) for r in rows]
    items["kind"], items["alpha"], items["flags"] = abi.LINE_2D, 255, abi.WORLD_CLIP_NEAR
    return items


def gizmo_record_count(kind, size):
    """Records an item becomes in the tile pass: `size` parallel lines for a thick line of thickness > 1, else one."""
    return size if (kind == abi.GIZMO_THICK_LINE_DEPTH and size > 1) else 1


def gizmo_item(kind, p0, p1=(0.0, 0.0, 0.0), p2=(0.0, 0.0, 0.0), color: T.Color = None, size=0):
    """One abi.GIZMO_ITEM_DTYPE record."""
    it = np.zeros(1, abi.GIZMO_ITEM_DTYPE)
    it["p0"], it["p1"], it["p2"], it["size"] = np.asarray(p0, np.float32), np.asarray(p1, np.float32), np.asarray(p2, np.float32), size
    it["r"], it["g"], it["b"], it["blend"] = color.r, color.g, color.b, color.blend
    it["kind"] = kind
    return it


def octahedron_items(center, size, color: T.Color):
    """b32_octahedron_items: the editor's draw_filled_octahedron (viewport_3d.rs:6223-6292) as 20 items in call order -- the eight faces
    as GIZMO_TRIANGLE, then the twelve edges as GIZMO_LINE in the darker edge colour.  Host only."""
    out = np.zeros(20, abi.GIZMO_ITEM_DTYPE)
    ctr = (C.c_float * 3)(*[float(v) for v in center])
    col = (C.c_uint8 * 4)(color.r, color.g, color.b, color.blend)
    _chk(abi.load_library().b32_octahedron_items(ctr, float(size), col, out.ctypes.data), "octahedron_items")
    return out


# ---- the overlay calls' structs and the lists that travel beside them (b32_draw_mesh_overlay, b32_draw_room_overlay, b32_draw_object_overlays)
class MeshOverlay:
    """B32MeshOverlay: which sections to draw (abi.OVERLAY_* bits), the hovered element (a masked hover result: None = none), the kind of
    the selection (abi.SELECT_*; the list itself travels beside the struct), the preview's mode (abi.PREVIEW_*) and rectangle."""

    def __init__(self, sections=0, hover_vertex=None, hover_edge=None, hover_face=None, select_kind=abi.SELECT_NONE, preview_mode=abi.PREVIEW_VERTEX,
                 rect=(0.0, 0.0, 0.0, 0.0)):
        self.sections, self.select_kind, self.preview_mode, self.rect = sections, select_kind, preview_mode, tuple(rect)
        self.hover_vertex = abi.OVERLAY_NONE if hover_vertex is None else int(hover_vertex)
        self.hover_edge = (abi.OVERLAY_NONE, abi.OVERLAY_NONE) if hover_edge is None else (int(hover_edge[0]), int(hover_edge[1]))
        self.hover_face = abi.OVERLAY_NONE if hover_face is None else int(hover_face)

    def selected_list(self, selected):
        """The list as the C entry takes it: a flat uint32 array (pairs flattened) and n_selected."""
        sel = np.ascontiguousarray(selected if selected is not None else [], np.uint32).reshape(-1)
        return sel, (len(sel) // 2 if self.select_kind == abi.SELECT_EDGES else len(sel))

    def pack(self, selected=None):
        sel, n = self.selected_list(selected)
        return abi.B32MeshOverlay(self.sections, self.hover_vertex, self.hover_edge[0], self.hover_edge[1], self.hover_face, self.select_kind, n,
                                  self.preview_mode, *[float(v) for v in self.rect]), sel


class RoomOverlay:
    """B32RoomOverlay and the lists that travel beside it: which sections to draw (abi.ROOM_OVERLAY_* bits), the hover (an
    abi.ROOM_HOVER_DTYPE record, raw; hover_source = abi.ROOM_OVERLAY_HOVER_RESIDENT: the room's last hover, read on the device -- the
    mirror still reads `hover`), the primary vertex key, the skip range of includes_face, the rectangle as stored, and the lists:
    vertices (keys 4 * rec + corner, strictly ascending), edges ((rec, edge_idx) pairs), faces (recs), points ((m, 3) positions)."""

    def __init__(self, sections=0, hover=None, hover_source=abi.ROOM_OVERLAY_HOVER_GIVEN, primary_vertex=None, skip=(0, 0), rect=(0.0, 0.0, 0.0, 0.0),
                 vertices=None, edges=None, faces=None, points=None):
        self.sections, self.hover_source, self.skip, self.rect = int(sections), int(hover_source), (int(skip[0]), int(skip[1])), tuple(rect)
        if hover is None:
            hover = np.zeros((), abi.ROOM_HOVER_DTYPE)
            for k in ("vertex_rec", "vertex_corner", "edge_rec", "edge_idx", "face_rec"):
                hover[k] = abi.HOVER_NONE
        self.hover = np.array(hover, abi.ROOM_HOVER_DTYPE).reshape(())
        self.primary_vertex = abi.HOVER_NONE if primary_vertex is None else int(primary_vertex)
        self.vertices = np.ascontiguousarray(vertices if vertices is not None else [], np.uint32).reshape(-1)
        self.edges = np.ascontiguousarray(edges if edges is not None else [], np.uint32).reshape(-1, 2)
        self.faces = np.ascontiguousarray(faces if faces is not None else [], np.uint32).reshape(-1)
        self.points = np.ascontiguousarray(points if points is not None else [], np.float32).reshape(-1, 3)

    def pack(self):
        """(abi.B32RoomOverlay, the four list pointers or None)"""
        h = abi.B32RoomHover.from_buffer_copy(self.hover.tobytes())
        o = abi.B32RoomOverlay(self.sections, self.hover_source, h, self.primary_vertex, self.skip[0], self.skip[1], len(self.vertices), len(self.edges),
                               len(self.faces), len(self.points), *[float(v) for v in self.rect])
        return o, tuple(abi.ptr(a) if len(a) else None for a in (self.vertices, self.edges, self.faces, self.points))


class ObjectPart:
    """One MeshPart of an asset: `scene`, the detached ResidentScene that holds its mesh; `topology`, its polygons (None when the part is
    hidden or only boxes read it); `visible`, part.visible; `vertices`, the host's copy (abi.VERTEX_DTYPE or (n, 3) positions) -- read by
    the mirror only, never by the device calls."""

    def __init__(self, scene=None, topology=None, visible=True, vertices=None):
        self.scene, self.topology, self.visible = scene, topology, bool(visible)
        self.vertices = None if vertices is None else _positions(vertices)


class ObjectItem:
    """One reference call: kind abi.OBJECT_WIRE (draw_asset_wireframe), abi.OBJECT_BOX_MESH (asset.bounds() -> draw_rotated_bounding_box) or
    abi.OBJECT_BOX (draw_rotated_bounding_box with box = (min, max)); the asset is parts[first_part : first_part + n_parts] of the call's
    table; the placement (a Placement, an abi.B32Placement or (cos_f, sin_f, world_pos)) is always applied."""

    def __init__(self, kind, placement, first_part=0, n_parts=0, color=None, box=None):
        self.kind, self.first_part, self.n_parts = int(kind), int(first_part), int(n_parts)
        self.cos_f, self.sin_f, self.world_pos = _placement_triple(placement)
        self.color = color if color is not None else T.Color(255, 200, 50)
        f32 = np.float32
        self.box = (tuple(f32(v) for v in box[0]), tuple(f32(v) for v in box[1])) if box is not None else ((f32(0),) * 3, (f32(0),) * 3)


def pack_object_items(items):
    """The abi.OBJECT_ITEM_DTYPE array of a sequence of ObjectItem."""
    out = np.zeros(len(items), abi.OBJECT_ITEM_DTYPE)
    for i, it in enumerate(items):
        r = out[i]
        r["cos_f"], r["sin_f"], r["world_pos"] = it.cos_f, it.sin_f, it.world_pos
        r["first_part"], r["n_parts"], r["box_min"], r["box_max"] = it.first_part, it.n_parts, it.box[0], it.box[1]
        r["r"], r["g"], r["b"], r["blend"], r["kind"] = it.color.r, it.color.g, it.color.b, it.color.blend, it.kind
    return out
