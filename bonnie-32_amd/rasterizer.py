"""Host-side mirror of the reference rasterizer interface, running on the MI355X through the C ABI.

Same names and argument meaning as the reference:
    Framebuffer::{new, resize, clear}       src/rasterizer/render.rs:18-45
    render_mesh_15(fb, vertices, faces, textures, camera, settings, fog) -> RasterTimings   render.rs:2302-2310
Errors the reference turns into panics come back as B32Error (index out of range, NaN sort key).

There is no CPU path here: if libb32raster.so or a HIP device is missing, construction raises.
"""
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
        return abi.B32Placement(float(self.cos_f), float(self.sin_f), (C.c_float * 3)(*[float(x) for x in self.world_pos]))

    def apply(self, vertices):
        """The vertices render_asset_parts hands to render_mesh_15 / render_mesh for this placement (host restatement)."""
        if not self.has_transform:
            return np.array(vertices, dtype=abi.VERTEX_DTYPE, copy=True)
        return place_vertices(vertices, self.cos_f, self.sin_f, self.world_pos)


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


def pack_bones(bones):
    """A bone table as a contiguous abi.BONE_DTYPE array: from such an array, or from a sequence of Bone."""
    if isinstance(bones, np.ndarray) and bones.dtype == abi.BONE_DTYPE:
        return np.ascontiguousarray(bones).reshape(-1)
    out = np.zeros(len(bones), abi.BONE_DTYPE)
    for i, b in enumerate(bones):
        out[i] = b.record()
    return out


def rotate_by_euler(v, rot_deg):
    """rotate_by_euler (modeler/state.rs:30-54) for one vector in f32: (x, y, z)."""
    f32 = np.float32
    b = Bone.from_euler((0.0, 0.0, 0.0), rot_deg)
    x, y, z = (f32(c) for c in v)
    if not b.rotate:
        return x, y, z
    with np.errstate(all="ignore"):
        y1 = y * b.cos_x + z * b.sin_x
        z1 = (-y) * b.sin_x + z * b.cos_x
        x2 = x * b.cos_z + y1 * b.sin_z
        y2 = (-x) * b.sin_z + y1 * b.cos_z
    return x2, y2, z1


def bone_world_transforms(local_positions, local_rotations, parents, indices=None):
    """get_bone_world_transform (modeler/state.rs:2585-2614) for the bones `indices` (default: every bone) of a skeleton given as
    local positions, local rotations (degrees) and parents (None or a negative number: a root).  Per bone the chain from the root down to
    it is walked: position += rotate_by_euler(local_position, rotation so far), then rotation += local_rotation, all in f32.  An index
    past the skeleton gives (0, 0), as in the reference.  Returns (positions, rotations), two (len(indices), 3) f32 arrays; feed row i to
    Bone.from_euler."""
    f32 = np.float32
    lp = np.asarray(local_positions, f32).reshape(-1, 3)
    lr = np.asarray(local_rotations, f32).reshape(-1, 3)
    n = len(lp)
    idxs = range(n) if indices is None else indices
    pos = np.zeros((len(idxs), 3), f32); rot = np.zeros((len(idxs), 3), f32)
    with np.errstate(all="ignore"):
        for row, i in enumerate(idxs):
            if i < 0 or i >= n:
                continue
            chain = []
            cur = i
            while cur is not None and cur >= 0:
                chain.append(cur)
                if len(chain) > n:
                    raise ValueError("bone_world_transforms: the parents form a cycle")
                cur = parents[cur]
                if cur is not None and cur >= n:
                    raise IndexError("bone_world_transforms: parent out of range")
            p = [f32(0.0)] * 3; r = [f32(0.0)] * 3
            for k in reversed(chain):
                q = rotate_by_euler(lp[k], r)
                p = [p[0] + q[0], p[1] + q[1], p[2] + q[2]]
                r = [r[0] + lr[k][0], r[1] + lr[k][1], r[2] + lr[k][2]]
            pos[row] = p; rot[row] = r
    return pos, rot


def pose_vertices(vertices, bone_of_vertex, bones):
    """What b32_scene_pose leaves in a slot, in numpy float32: per vertex rotate_by_euler(pos, bone_rot) + bone_pos and the normal rotated
    alike (not renormalised), each operation separately rounded in the reference's order (numpy does not fuse).  A bone index past the
    table (abi.BONE_NONE included) leaves the vertex as it is; a bone with rotate == 0 only translates and leaves the normal's bits.
    uv and colour are unchanged.  This is what a host without the library does per frame before it uploads."""
    v = np.array(vertices, dtype=abi.VERTEX_DTYPE, copy=True).reshape(-1)
    tab = pack_bones(bones)
    bo = np.asarray(bone_of_vertex).reshape(-1).astype(np.int64)
    if len(bo) != len(v):
        raise ValueError("pose_vertices: one bone index per vertex")
    if not len(tab) or not len(v):
        return v
    has = (bo >= 0) & (bo < len(tab))
    t = tab[np.where(has, bo, 0)]
    rot = has & (t["rotate"] != 0)
    tr = has & ~rot
    cx, sx, cz, sz = t["cos_x"], t["sin_x"], t["cos_z"], t["sin_z"]

    def turned(a):
        x, y, z = a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()
        y1 = y * cx + z * sx
        z1 = (-y) * sx + z * cx
        x2 = x * cz + y1 * sz
        y2 = (-x) * sz + y1 * cz
        return x2, y2, z1

    with np.errstate(all="ignore"):
        rp = turned(v["pos"]); rn = turned(v["normal"])
        for k in range(3):
            rest = v["pos"][:, k].copy()
            v["pos"][:, k] = np.where(rot, rp[k] + t["pos"][:, k], np.where(tr, rest + t["pos"][:, k], rest))
            v["normal"][:, k] = np.where(rot, rn[k], v["normal"][:, k])
    return v


# ---- editing a resident scene in place (b32_scene_patch_*): the reference composition in numpy.  The mirrors patch host arrays; what they
# return is given to the oracle or to a fresh upload, which a patched slot must be indistinguishable from
def patch_indices(indices, limit):
    """The `index` column of a patch as the library accepts it: strictly ascending and below `limit`, else ValueError."""
    idx = np.asarray(indices, np.int64).reshape(-1)
    if len(idx) and (idx[0] < 0 or idx[-1] >= limit or np.any(np.diff(idx) <= 0)):
        raise ValueError("patch: indices must be strictly ascending and inside the body")
    return idx


def patch_vertices(vertices, indices, records, rest=None, bone_of_vertex=None, bones=()):
    """b32_scene_patch_vertices on host arrays.  Without `rest`: a copy of `vertices` with records written at `indices`.  With `rest` (a
    rigged slot: the (n, 6) float32 rest stream, position then normal): the records are in rest space; returns (vertices, rest) where the
    rest stream got position and normal and the vertices the records posed by `bones` (pose_vertices; an empty table copies)."""
    v = np.array(vertices, dtype=abi.VERTEX_DTYPE, copy=True).reshape(-1)
    idx = patch_indices(indices, len(v))
    recs = np.asarray(records, abi.VERTEX_DTYPE).reshape(-1)
    if len(recs) != len(idx):
        raise ValueError("patch_vertices: one record per index")
    if rest is None:
        v[idx] = recs
        return v
    r = np.array(rest, dtype=np.float32, copy=True).reshape(-1, 6)
    r.view(np.uint32)[idx, 0:3] = recs["pos"].view(np.uint32)
    r.view(np.uint32)[idx, 3:6] = recs["normal"].view(np.uint32)
    bo = np.asarray(bone_of_vertex).reshape(-1)
    v[idx] = pose_vertices(recs, bo[idx], bones)
    return v, r


def rest_stream(vertices):
    """The rest stream b32_scene_set_rig takes from a slot's vertices: (n, 6) float32, position then normal."""
    v = np.asarray(vertices, abi.VERTEX_DTYPE).reshape(-1)
    return np.concatenate([v["pos"], v["normal"]], axis=1).astype(np.float32)


def patch_faces(faces, indices, records):
    """b32_scene_patch_faces on a host array: a copy of `faces` with the whole records written at `indices`."""
    f = np.array(faces, dtype=abi.FACE_DTYPE, copy=True).reshape(-1)
    idx = patch_indices(indices, len(f))
    recs = np.asarray(records, abi.FACE_DTYPE).reshape(-1)
    if len(recs) != len(idx):
        raise ValueError("patch_faces: one record per index")
    f[idx] = recs
    return f


def _patch_rect(shape, x, y, block):
    h, w = block.shape[:2]
    if h == 0 or w == 0:
        return None
    if x < 0 or y < 0 or x + w > shape[1] or y + h > shape[0]:
        raise ValueError("patch: the rectangle leaves the texture")
    return slice(y, y + h), slice(x, x + w)


def patch_texels(texels, x, y, block):
    """b32_scene_patch_texels on a host array: `texels` is one texture as (height, width) Color15 or (height, width, 4) Color bytes,
    `block` the rectangle's texels, (h, w[, 4]); any view will do, its rows need not be contiguous.  Returns the patched copy."""
    t = np.array(texels, copy=True)
    block = np.asarray(block, t.dtype)
    at = _patch_rect(t.shape, x, y, block)
    if at is not None:
        t[at] = block
    return t


def clut_lookup(clut, indices):
    """Clut::lookup (types.rs:390-397) for an array of indices: an index at or past the palette is 0x0000."""
    clut = np.asarray(clut, np.uint16).reshape(-1)
    idx = np.asarray(indices, np.int64)
    pad = np.concatenate([clut, np.zeros(1, np.uint16)])
    return pad[np.where(idx < len(clut), idx, len(clut))]


def patch_indexed(texels, atlas, x, y, index_block, clut):
    """b32_scene_patch_indexed on host arrays: `texels` (height, width) Color15 and `atlas` (height, width) index bytes of one texture
    (atlas may be None), `index_block` the rectangle's indices (h, w).  Returns (texels, atlas) patched: the texels get
    clut_lookup(clut, index_block), the atlas the indices.  (A palette-only change is the whole atlas with the new CLUT.)"""
    block = np.asarray(index_block, np.uint8)
    t = patch_texels(np.asarray(texels, np.uint16), x, y, clut_lookup(clut, block))
    a = None if atlas is None else patch_texels(np.asarray(atlas, np.uint8), x, y, block)
    return t, a


def kept_clut(clut):
    """The CLUT a slot keeps beside its index atlas: 256 entries, zero behind a shorter palette."""
    out = np.zeros(256, np.uint16)
    c = np.asarray(clut, np.uint16).reshape(-1)[:256]
    out[:len(c)] = c
    return out


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
    if isinstance(bones, np.ndarray) and bones.dtype == abi.SKEL_BONE_DTYPE:
        return np.ascontiguousarray(bones).reshape(-1)
    out = np.zeros(len(bones), abi.SKEL_BONE_DTYPE)
    for i, b in enumerate(bones):
        out[i] = b.record()
    return out


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


class SkeletonMirror:
    """skeleton_to_triangles, skeleton_to_triangles_from_bones, draw_skeleton and draw_bone_dots in numpy float32, one separately
    rounded operation at a time in the reference's order: what b32_scene_build_skeleton leaves behind a slot's body and what
    b32_skeleton_items returns.  The rules are methods and attributes so that a test can change one of them and watch a case move."""
    f32 = np.float32
    DEGENERATE, UP_LIMIT, RING_AT, DEFAULT_WIDTH, DIM_ALPHA = np.float32(0.001), np.float32(0.9), np.float32(0.2), np.float32(40.0), 30
    COLOURS = {"default": (200, 200, 200), "selected": (80, 255, 80), "hovered": (100, 180, 255), "tip_hovered": (255, 180, 80),
               "root": (255, 220, 100), "creating": (255, 150, 50), "hierarchy_line": (100, 100, 100)}
    DOTS = {"tip": (5, (220, 220, 230)), "tip_selected": (8, (80, 255, 80)), "tip_hovered": (11, (255, 180, 80)),
            "base": (5, (150, 150, 160)), "base_selected": (8, (80, 255, 80)), "base_hovered": (11, (100, 180, 255))}
    RING = ((0, 1), (1, 1), (0, -1), (1, -1))                   # ring[i] = centre + sign * perp[which] * width
    DOT_ORDER = ("tip", "base")

    # -- Vec3 (math.rs:23-49)
    def length(self, v):
        return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])

    def normalize(self, v):
        l = self.length(v)
        if l == 0.0:
            return [self.f32(0.0)] * 3
        return [v[0] / l, v[1] / l, v[2] / l]

    @staticmethod
    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    # -- the rules
    def tip(self, b):
        """get_bone_tip_position, state.rs:2629-2638"""
        d = self.normalize([b["sin_z"] * b["cos_x"], b["cos_z"] * b["cos_x"], -b["sin_x"]])
        return [b["pos"][k] + d[k] * b["length"] for k in range(3)]

    def degenerate(self, length):
        return length < self.DEGENERATE

    def y_up(self, dir_y):
        return abs(dir_y) < self.UP_LIMIT

    def dimmed(self, style, i):
        return style.selected_bone is not None and style.selected_bone >= 0 and style.selected_bone != i

    def bone_style(self, style, i, root):
        """(rgb, alpha) of bone i, skeleton.rs:430-454 / :546-550"""
        plain = self.COLOURS["root" if root else "default"]
        if style.mode != abi.SKELETON_TRIANGLES:
            return plain, style.editor_alpha
        if style.selected_bone == i:
            rgb = self.COLOURS["selected"]
        elif style.hovered_tip == i:
            rgb = self.COLOURS["tip_hovered"]
        elif style.hovered_bone == i:
            rgb = self.COLOURS["hovered"]
        else:
            rgb = plain
        return rgb, (min(style.editor_alpha, self.DIM_ALPHA) if self.dimmed(style, i) else style.editor_alpha)

    def octahedron(self, base, tip, width, rgb, alpha, v_start):
        """generate_bone_octahedron, skeleton.rs:565-660: (6 vertices, 8 faces) or None"""
        f32 = self.f32
        direction = [tip[k] - base[k] for k in range(3)]
        length = self.length(direction)
        if self.degenerate(length):
            return None
        inv = f32(1.0) / length
        dn = [direction[k] * inv for k in range(3)]
        up = [f32(0.0), f32(1.0), f32(0.0)] if self.y_up(dn[1]) else [f32(1.0), f32(0.0), f32(0.0)]
        perp1 = self.normalize(self.cross(dn, up))
        perp2 = self.normalize(self.cross(dn, perp1))
        along = length * f32(self.RING_AT)
        centre = [base[k] + dn[k] * along for k in range(3)]
        perps = (perp1, perp2)
        ring = [[centre[k] + perps[which][k] * width if sign > 0 else centre[k] - perps[which][k] * width for k in range(3)] for which, sign in self.RING]
        v = np.zeros(6, abi.VERTEX_DTYPE)
        v["pos"][0], v["normal"][0] = base, [dn[k] * f32(-1.0) for k in range(3)]
        v["pos"][1], v["normal"][1] = tip, dn
        for i in range(4):
            v["pos"][2 + i], v["normal"][2 + i] = ring[i], self.normalize([ring[i][k] - centre[k] for k in range(3)])
        v["r"], v["g"], v["b"] = rgb
        f = np.zeros(8, abi.FACE_DTYPE)
        for i in range(4):
            nxt = (i + 1) % 4
            f["v"][i] = (v_start, v_start + 2 + i, v_start + 2 + nxt)
            f["v"][4 + i] = (v_start + 1, v_start + 2 + nxt, v_start + 2 + i)
        f["texture_id"], f["blend_mode"], f["editor_alpha"] = abi.NO_TEXTURE, abi.OPAQUE, alpha
        return v, f

    def mesh(self, bones, style, vertex_offset=0):
        """(vertices, faces) of the tail: abi.VERTEX_DTYPE / abi.FACE_DTYPE, face indices from vertex_offset on."""
        tab = pack_skel_bones(bones)
        vs, fs = [], []
        at = int(vertex_offset)
        with np.errstate(all="ignore"):
            octs = [(b["pos"], self.tip(b), b["width"]) + self.bone_style(style, i, b["parent"] == abi.BONE_NONE) for i, b in enumerate(tab)]
            if style.mode == abi.SKELETON_TRIANGLES and style.preview is not None:
                octs.append((np.asarray(style.preview[0], np.float32), np.asarray(style.preview[1], np.float32), self.DEFAULT_WIDTH,
                             self.COLOURS["creating"], 255))
            for base, tip, width, rgb, alpha in octs:
                o = self.octahedron([self.f32(x) for x in base], [self.f32(x) for x in tip], self.f32(width), rgb, alpha, at)
                if o is not None:
                    vs.append(o[0]); fs.append(o[1]); at += 6
        v = np.concatenate(vs) if vs else np.zeros(0, abi.VERTEX_DTYPE)
        f = np.concatenate(fs) if fs else np.zeros(0, abi.FACE_DTYPE)
        for k in ("pos", "normal"):                                 # the one departure: a NaN is the quiet NaN 0x7FC00000
            w = v[k].view(np.uint32)
            w[np.isnan(v[k])] = 0x7FC00000
        return v, f

    def items(self, bones, style):
        """The calls of draw_skeleton (skeleton.rs:70-79) and then of draw_bone_dots (:110-143) as abi.WORLD_ITEM_DTYPE items."""
        tab = pack_skel_bones(bones)
        rows = []                                                   # (kind, p0, p1, size, rgb, flags)
        zero = np.zeros(3, np.float32)
        for i, b in enumerate(tab):
            if b["parent"] != abi.BONE_NONE:
                rows.append((abi.LINE_2D, tab[b["parent"]]["pos"] if b["parent"] < len(tab) else zero, b["pos"], 0, self.COLOURS["hierarchy_line"], abi.WORLD_CLIP_NEAR))
        with np.errstate(all="ignore"):
            for i, b in enumerate(tab):
                for what in self.DOT_ORDER:
                    if what == "tip":
                        key = "tip_hovered" if style.hovered_tip == i else ("tip_selected" if style.selected_bone == i else "tip")
                        p = np.array(self.tip(b), np.float32)
                    else:
                        key = "base_hovered" if style.hovered_bone == i else ("base_selected" if style.selected_bone == i else "base")
                        p = b["pos"]
                    rows.append((abi.PRIM_CIRCLE, p, zero, self.DOTS[key][0], self.DOTS[key][1], 0))
        items = np.zeros(len(rows), abi.WORLD_ITEM_DTYPE)
        for k, (kind, p0, p1, size, rgb, flags) in enumerate(rows):
            items[k]["p0"], items[k]["p1"], items[k]["size"], items[k]["kind"], items[k]["flags"] = p0, p1, size, kind, flags
            items[k]["r"], items[k]["g"], items[k]["b"] = rgb
        items["alpha"] = 255
        return items


def skeleton_mesh(bones, style, vertex_offset=0):
    """SkeletonMirror().mesh: the tail b32_scene_build_skeleton writes behind a body of vertex_offset vertices."""
    return SkeletonMirror().mesh(bones, style, vertex_offset)


def skeleton_items(bones, style):
    """SkeletonMirror().items: what b32_skeleton_items returns, for Framebuffer.draw_world."""
    return SkeletonMirror().items(bones, style)


def _placement_triple(placement):
    """(cos_f, sin_f, world_pos) as f32 of a Placement, an abi.B32Placement or such a triple.  Picking always applies the placement
    (viewport_3d.rs:7716-7718 has no has_transform shortcut), so Placement.has_transform is not consulted."""
    f32 = np.float32
    if isinstance(placement, (Placement, abi.B32Placement)):
        c, s, w = placement.cos_f, placement.sin_f, tuple(placement.world_pos)
    else:
        c, s, w = placement
    return f32(c), f32(s), tuple(f32(x) for x in w)


class PickMirror:
    """check_mesh_hit (editor/viewport_3d.rs:7700-7756) and the face branch of find_hovered_element (modeler/viewport.rs:2544-2594) for one
    placed mesh in numpy float32: what b32_pick_meshes computes per item, and what a host without this library walks per mouse move.
    The constructor does what the reference does once per mesh and frame (place and project every vertex: screen_verts); pick() is the
    triangle loop for one cursor.  Every operation is one separately rounded f32 operation in the reference's order."""

    def __init__(self, vertices, faces, placement, camera, w, h, ortho=None):
        f32 = np.float32
        pos = np.ascontiguousarray(vertices["pos"] if getattr(vertices, "dtype", None) is not None and vertices.dtype.names else vertices, f32).reshape(-1, 3)
        fv = np.ascontiguousarray(faces["v"] if getattr(faces, "dtype", None) is not None and faces.dtype.names else faces).reshape(-1, 3).astype(np.int64)
        c, s, wp = _placement_triple(placement)
        cp, bx, by, bz = (tuple(f32(x) for x in getattr(camera, n)) for n in ("position", "basis_x", "basis_y", "basis_z"))
        with np.errstate(all="ignore"):
            x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
            rx = x * c - z * s
            rz = x * s + z * c
            rel = (rx + wp[0] - cp[0], y + wp[1] - cp[1], rz + wp[2] - cp[2])
            cam_x, cam_y, cam_z = ((rel[0] * b[0] + rel[1] * b[1]) + rel[2] * b[2] for b in (bx, by, bz))
            hw, hh = f32(w) / f32(2.0), f32(h) / f32(2.0)
            if ortho is not None:                                  # world_to_screen_with_ortho_depth, math.rs:595-599: never None
                zoom, ocx, ocy = (f32(v) for v in ortho)
                sx = (cam_x - ocx) * zoom + hw
                sy = -(cam_y - ocy) * zoom + hh
                some = np.ones(len(pos), bool)
            else:                                                  # world_to_screen_with_depth, math.rs:621-652
                vs = (f32(min(w, h)) / f32(2.0)) * f32(0.75)
                denom = cam_z + f32(5.0)
                sx = (cam_x * f32(4.0) / denom) * vs + hw
                sy = (cam_y * f32(4.0) / denom) * vs + hh
                some = ~(cam_z <= f32(0.1))
            inside = (fv >= 0).all(1) & (fv < len(pos)).all(1)     # screen_verts.get(..): an index out of range skips the triangle
            i = np.where(inside[:, None], fv, 0) if len(pos) else np.zeros_like(fv)
            if not len(pos):
                sx = sy = cam_z = np.zeros(1, f32); some = np.zeros(1, bool)
            self.ok = inside & some[i[:, 0]] & some[i[:, 1]] & some[i[:, 2]]
            self.x = [sx[i[:, k]] for k in range(3)]; self.y = [sy[i[:, k]] for k in range(3)]; self.d = [cam_z[i[:, k]] for k in range(3)]
            x0, x1, x2 = self.x; y0, y1, y2 = self.y
            self.area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
            self.front = ~(self.area <= f32(0.0))                  # modeler/viewport.rs:2571-2574 (a NaN area is not culled)

    def candidates(self, mx, my, cull_backfaces=False):
        """(triangle indices in face order, their depths) of every triangle the cursor hits."""
        f32 = np.float32
        px, py = f32(mx), f32(my)
        x0, x1, x2 = self.x; y0, y1, y2 = self.y
        with np.errstate(all="ignore"):
            d1 = (px - x1) * (y0 - y1) - (x0 - x1) * (py - y1)     # point_in_triangle_2d, math.rs:687-706
            d2 = (px - x2) * (y1 - y2) - (x1 - x2) * (py - y2)
            d3 = (px - x0) * (y2 - y0) - (x2 - x0) * (py - y0)
            has_neg = (d1 < 0) | (d2 < 0) | (d3 < 0)
            has_pos = (d1 > 0) | (d2 > 0) | (d3 > 0)
            hit = self.ok & ~(has_neg & has_pos)
            if cull_backfaces:
                hit &= self.front
            t = np.nonzero(hit)[0]
            x0, x1, x2 = (v[t] for v in self.x); y0, y1, y2 = (v[t] for v in self.y); e0, e1, e2 = (v[t] for v in self.d)
            area = self.area[t]                                    # interpolate_depth_in_triangle, viewport_3d.rs:7485-7508
            w0 = ((x1 - px) * (y2 - py) - (x2 - px) * (y1 - py)) / area
            w1 = ((x2 - px) * (y0 - py) - (x0 - px) * (y2 - py)) / area
            w2 = f32(1.0) - w0 - w1
            depth = np.where(np.abs(area) < f32(0.0001), (e0 + e1 + e2) / f32(3.0), w0 * e0 + w1 * e1 + w2 * e2).astype(f32)
        return t, depth

    def pick(self, mx, my, cull_backfaces=False):
        """(hit, tri, depth): the closest hit by the reference's strict `<` in face order -- the first of equal depths, a NaN depth only when
        it is the first hit (reported as the quiet NaN 0x7FC00000); no hit: (False, 0xFFFFFFFF, 0.0)."""
        t, depth = self.candidates(mx, my, cull_backfaces)
        return _closest_in_order(t, depth)


def _closest_in_order(ids, depth):
    """`closest = None; for (id, depth): if closest is None or depth < closest.depth: closest = (depth, id)` without the loop."""
    f32 = np.float32
    if not len(ids):
        return False, abi.PICK_NO_TRI, f32(0.0)
    if np.isnan(depth[0]):
        return True, int(ids[0]), np.array([0x7FC00000], np.uint32).view(f32)[0]
    num = ~np.isnan(depth)
    j = int(np.nonzero(num & (depth == depth[num].min()))[0][0])
    return True, int(ids[j]), depth[j]


def pick_mesh(vertices, faces, placement, camera, w, h, mx, my, ortho=None, cull_backfaces=False):
    """Host mirror of one item of b32_pick_meshes (see PickMirror): (hit, tri, depth)."""
    return PickMirror(vertices, faces, placement, camera, w, h, ortho).pick(mx, my, cull_backfaces)


def pick_best(hits):
    """The loop over the items (viewport_3d.rs:7370) on a PICK_HIT_DTYPE array: the index of the closest hit item, or -1."""
    hits = np.asarray(hits, abi.PICK_HIT_DTYPE)
    i = np.nonzero(hits["hit"])[0]
    hit, best, _ = _closest_in_order(i, hits["depth"][i])
    return best if hit else -1


class PickResult:
    """What b32_pick_meshes_async delivers into `buf` (16 + 16 * n bytes) once its ticket is done."""

    def __init__(self, buf, n, owner=None):
        self.buf, self.n, self._owner = buf, n, owner

    @property
    def best(self):
        return int(self.buf[:4].view(np.int32)[0])

    @property
    def hits(self):
        return self.buf[abi.PICK_HEADER_BYTES:abi.PICK_HEADER_BYTES + 16 * self.n].view(abi.PICK_HIT_DTYPE).copy()

    def close(self):
        if self._owner is not None:
            ctx, p = self._owner
            ctx.host_free(p)
            self._owner = None


# ---- hover and box selection (b32_hover_mesh, b32_box_select): the modeler's find_hovered_element / apply_box_selection for one mesh
def _project_f32(x, y, z, camera, w, h, ortho):
    """world_to_screen_with_ortho (math.rs:538-575) on f32 arrays: (sx, sy, cam_z, some)."""
    f32 = np.float32
    cp, bx, by, bz = (tuple(f32(v) for v in getattr(camera, n)) for n in ("position", "basis_x", "basis_y", "basis_z"))
    rel = (x - cp[0], y - cp[1], z - cp[2])
    cam_x, cam_y, cam_z = ((rel[0] * b[0] + rel[1] * b[1]) + rel[2] * b[2] for b in (bx, by, bz))
    hw, hh = f32(w) / f32(2.0), f32(h) / f32(2.0)
    if ortho is not None:
        zoom, ocx, ocy = (f32(v) for v in ortho)
        return (cam_x - ocx) * zoom + hw, -(cam_y - ocy) * zoom + hh, cam_z, np.ones(len(x), bool)
    vs = (f32(min(w, h)) / f32(2.0)) * f32(0.75)
    denom = cam_z + f32(5.0)
    return (cam_x * f32(4.0) / denom) * vs + hw, (cam_y * f32(4.0) / denom) * vs + hh, cam_z, ~(cam_z <= f32(0.1))


def _world_f32(pos, placement):
    """The positions the modeler's loops project: as they are (placement None) or placed as in PickMirror."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    if placement is None:
        return x, y, z
    c, s, wp = _placement_triple(placement)
    return (x * c - z * s) + wp[0], y + wp[1], (x * s + z * c) + wp[2]


def _positions(vertices):
    return np.ascontiguousarray(vertices["pos"] if getattr(vertices, "dtype", None) is not None and vertices.dtype.names else vertices, np.float32).reshape(-1, 3)


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


class _FanMirror(PickMirror):
    """PickMirror's triangle loop over already projected vertices (the fan triangles of a Topology)."""

    def __init__(self, sx, sy, cam_z, some, fv):
        f32 = np.float32
        n = len(sx)
        inside = (fv >= 0).all(1) & (fv < n).all(1)
        i = np.where(inside[:, None], fv, 0) if n else np.zeros_like(fv)
        if not n:
            sx = sy = cam_z = np.zeros(1, f32); some = np.zeros(1, bool)
        with np.errstate(all="ignore"):
            self.ok = inside & some[i[:, 0]] & some[i[:, 1]] & some[i[:, 2]]
            self.x = [sx[i[:, k]] for k in range(3)]; self.y = [sy[i[:, k]] for k in range(3)]; self.d = [cam_z[i[:, k]] for k in range(3)]
            x0, x1, x2 = self.x; y0, y1, y2 = self.y
            self.area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
            self.front = ~(self.area <= f32(0.0))


class HoverMirror:
    """find_hovered_element (modeler/viewport.rs:2379-2601) for one mesh in numpy float32: what b32_hover_mesh computes, and what a host
    without this library walks per mouse move.  The constructor does what the reference does once per mesh and frame (project every
    vertex, the front pass of viewport.rs:2435-2473); hover() answers one cursor with vectorised f32 operations, each separately rounded in
    the reference's order.  placement None: the vertices as they are; else it is always applied (as in PickMirror).
    local_vertices: the rest vertices of a rigged mesh whose posed vertices are `vertices` -- the mirror plane is tested on the LOCAL
    position (viewport.rs:2482-2486) while the posed one is projected."""

    def __init__(self, vertices, topology, placement, camera, w, h, ortho=None, local_vertices=None):
        f32 = np.float32
        self.pos = _positions(vertices)
        self.local = self.pos if local_vertices is None else _positions(local_vertices)
        if len(self.local) != len(self.pos):
            raise ValueError("HoverMirror: local_vertices must have one entry per vertex")
        self.top = t = topology
        nv = self.nv = len(self.pos)
        with np.errstate(all="ignore"):
            self.sx, self.sy, self.cz, self.some = _project_f32(*_world_f32(self.pos, placement), camera, w, h, ortho)
            sx, sy, some = self.sx, self.sy, self.some
            # the front pass: polygons with n >= 3 whose first three vertices exist and project, signed area > 0.0
            st = t.poly_start.astype(np.int64)
            big = np.nonzero(t.count >= 3)[0]
            pv = t.poly_verts.astype(np.int64)
            i3 = np.stack([pv[st[big] + k] for k in range(3)], 1) if len(big) else np.zeros((0, 3), np.int64)
            ok3 = (i3 < nv).all(1)
            j3 = np.where(ok3[:, None], i3, 0)
            if nv:
                ok3 &= some[j3].all(1)
                x, y = sx[j3], sy[j3]
                area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
                ok3 &= area > f32(0.0)
            else:
                ok3[:] = False
        front_poly = np.zeros(t.np, bool)
        front_poly[big[ok3]] = True
        on_front = front_poly[t.poly_of]                                        # per position of poly_verts == per half-edge
        self.vfront = np.zeros(nv, bool)
        self.vfront[pv[on_front & (pv < nv)]] = True
        efront = np.zeros(t.ne, bool)
        efront[t.he_edge[on_front]] = True
        self.he_front = efront[t.he_edge] if t.ne else np.zeros(0, bool)
        self.he_in = (t.he_v0 < nv) & (t.he_v1 < nv)
        self.he_a = np.where(self.he_in, t.he_v0, 0); self.he_b = np.where(self.he_in, t.he_v1, 0)
        self.faces = _FanMirror(sx, sy, self.cz, some, t.fan)

    def _editable(self, axis, threshold):
        if not axis:
            return np.ones(self.nv, bool)
        with np.errstate(all="ignore"):
            return self.local[:, axis - 1] >= -np.float32(threshold)           # state.rs:797-806 (a NaN fails)

    def hover(self, mx, my, see_through=False, mirror_axis=0, mirror_threshold=1.0, vertex_threshold=abi.HOVER_VERTEX_THRESHOLD,
              edge_threshold=abi.HOVER_EDGE_THRESHOLD):
        """One abi.HOVER_RESULT_DTYPE record: all three branches, raw (hovered_element() masks them)."""
        f32 = np.float32
        px, py = f32(mx), f32(my)
        t = self.top
        r = np.zeros((), abi.HOVER_RESULT_DTYPE)
        r["vertex"] = r["edge_v0"] = r["edge_v1"] = r["face"] = abi.HOVER_NONE
        edit = self._editable(mirror_axis, mirror_threshold)
        with np.errstate(all="ignore"):
            # vertices, viewport.rs:2475-2505
            ok = self.some & edit
            if not see_through:
                ok = ok & self.vfront
            dx, dy = px - self.sx, py - self.sy
            dist = np.sqrt(dx * dx + dy * dy)
            c = np.nonzero(ok & (dist < f32(vertex_threshold)))[0]
            if len(c):
                j = c[np.argmin(dist[c])]
                r["vertex"] = j; r["vertex_dist"] = dist[j]
            # half-edges, viewport.rs:2507-2542
            if self.nv and len(self.he_in):
                a, b = self.he_a, self.he_b
                ok = self.he_in & edit[a] & edit[b] & self.some[a] & self.some[b]
                if not see_through:
                    ok = ok & self.he_front
                x0, y0, x1, y1 = self.sx[a], self.sy[a], self.sx[b], self.sy[b]
                ex, ey = x1 - x0, y1 - y0
                len_sq = ex * ex + ey * ey
                tt = ((px - x0) * ex + (py - y0) * ey) / len_sq
                tt = np.where(tt < f32(0.0), f32(0.0), tt)                      # f32::clamp: a NaN and -0.0 stay
                tt = np.where(tt > f32(1.0), f32(1.0), tt)
                qx, qy = px - (x0 + tt * ex), py - (y0 + tt * ey)
                p0x, p0y = px - x0, py - y0
                dist = np.where(len_sq < f32(0.001), np.sqrt(p0x * p0x + p0y * p0y), np.sqrt(qx * qx + qy * qy)).astype(f32)
                c = np.nonzero(ok & (dist < f32(edge_threshold)))[0]
                if len(c):
                    j = c[np.argmin(dist[c])]
                    r["edge_v0"] = min(t.he_v0[j], t.he_v1[j]); r["edge_v1"] = max(t.he_v0[j], t.he_v1[j]); r["edge_dist"] = dist[j]
            # faces, viewport.rs:2544-2594
            if len(t.fan):
                pv = t.poly_verts.astype(np.int64)
                bad = pv >= self.nv
                bad[~bad] = ~edit[pv[~bad]]
                bad_poly = np.zeros(t.np, bool)
                bad_poly[t.poly_of[bad]] = True
                tri, depth = self.faces.candidates(px, py, not see_through)
                keep = ~bad_poly[t.fan_poly[tri]]
                hit, j, d = _closest_in_order(tri[keep], depth[keep])
                if hit:
                    r["face"] = t.fan_poly[j]; r["face_depth"] = d
        return r


def hover_mesh(vertices, topology, placement, camera, w, h, mx, my, ortho=None, **params):
    """Host mirror of b32_hover_mesh (see HoverMirror): one abi.HOVER_RESULT_DTYPE record."""
    return HoverMirror(vertices, topology, placement, camera, w, h, ortho).hover(mx, my, **params)


def hovered_element(result):
    """find_hovered_element's return tuple (viewport.rs:2596-2600) of a hover result: the vertex; the edge only without a vertex; the face
    only without either.  (vertex | None, (v0, v1) | None, polygon | None)."""
    v = int(result["vertex"]); e = (int(result["edge_v0"]), int(result["edge_v1"])); f = int(result["face"])
    v = None if v == abi.HOVER_NONE else v
    e = None if v is not None or e[0] == abi.HOVER_NONE else e
    f = None if v is not None or e is not None or f == abi.HOVER_NONE else f
    return v, e, f


def box_select_mesh(vertices, topology, placement, camera, w, h, rect, mode=abi.BOX_VERTICES, ortho=None):
    """Host mirror of b32_box_select -- apply_box_selection (modeler/viewport.rs:1624-1779) for one rectangle (x0, y0, x1, y1):
    (words, n_selected), bit i of word i // 32 set iff element i is selected.  mode BOX_VERTICES: every vertex that projects into the
    rectangle (inclusive); BOX_POLYGONS: every polygon whose centre (viewport.rs:1749) does."""
    f32 = np.float32
    pos = _positions(vertices)
    x0, y0, x1, y1 = (f32(v) for v in rect)
    with np.errstate(all="ignore"):
        wx, wy, wz = _world_f32(pos, placement)
        some = None
        if mode == abi.BOX_POLYGONS:
            t = topology
            st = t.poly_start.astype(np.int64); pv = t.poly_verts.astype(np.int64)
            acc = [np.zeros(t.np, f32) for _ in range(3)]
            cnt = np.zeros(t.np, np.int64)
            for k in range(int(t.count.max()) if t.np else 0):                  # fold(Vec3::ZERO, acc + p) in order
                m = np.nonzero(t.count > k)[0]
                i = pv[st[m] + k]
                m = m[i < len(pos)]; i = i[i < len(pos)]
                for a, wc in zip(acc, (wx, wy, wz)):
                    a[m] = a[m] + wc[i]
                cnt[m] += 1
            inv = f32(1.0) / np.maximum(cnt, 1).astype(f32)
            wx, wy, wz = acc[0] * inv, acc[1] * inv, acc[2] * inv
            some = cnt > 0
        sx, sy, _, ok = _project_f32(wx, wy, wz, camera, w, h, ortho)
        sel = ok & (sx >= x0) & (sx <= x1) & (sy >= y0) & (sy <= y1)
        if some is not None:
            sel &= some
    n = len(sel)
    bits = np.zeros(((n + 31) // 32) * 32, np.uint8)
    bits[:n] = sel
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    return words, int(sel.sum())


class HoverResult:
    """What b32_hover_mesh_async delivers into `buf` (32 bytes) once its ticket is done."""

    def __init__(self, buf, owner=None):
        self.buf, self._owner = buf, owner

    @property
    def record(self):
        return self.buf[:32].view(abi.HOVER_RESULT_DTYPE)[0].copy()

    def close(self):
        if self._owner is not None:
            ctx, p = self._owner
            ctx.host_free(p)
            self._owner = None


class BoxResult:
    """What b32_box_select_async delivers into `buf` once its ticket is done: n_elements, n_selected and the words."""

    def __init__(self, buf, owner=None):
        self.buf, self._owner = buf, owner

    @property
    def n_elements(self):
        return int(self.buf[:4].view(np.uint32)[0])

    @property
    def n_selected(self):
        return int(self.buf[4:8].view(np.uint32)[0])

    @property
    def words(self):
        nw = (self.n_elements + 31) // 32
        return self.buf[abi.BOX_HEADER_BYTES:abi.BOX_HEADER_BYTES + 4 * nw].view(np.uint32).copy()

    close = HoverResult.close


# ---- room hover and box selection (b32_room_hover, b32_room_box_select): the world editor's find_hovered_elements / find_selections_in_rect
_ROOM_KEYS = (("floor", abi.ROOM_FLOOR), ("ceiling", abi.ROOM_CEILING), ("walls_north", abi.ROOM_WALL_NORTH), ("walls_east", abi.ROOM_WALL_EAST),
              ("walls_south", abi.ROOM_WALL_SOUTH), ("walls_west", abi.ROOM_WALL_WEST), ("walls_nwse", abi.ROOM_WALL_NWSE), ("walls_nesw", abi.ROOM_WALL_NESW))
# corner k's (x, z) selectors per kind, 0 = base, 1 = base + S (viewport_3d.rs:6603-6657, :7099-7170, :7183-7279)
_ROOM_XSEL = np.array([[0, 1, 1, 0], [0, 1, 1, 0], [0, 1, 1, 0], [1, 1, 1, 1], [1, 0, 0, 1], [0, 0, 0, 0], [0, 1, 1, 0], [1, 0, 0, 1]], bool)
_ROOM_ZSEL = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 0, 0], [0, 1, 1, 0], [1, 1, 1, 1], [1, 0, 0, 1], [0, 1, 1, 0], [0, 1, 1, 0]], bool)
# wall_center_in_rect's own (x0, z0, x1, z1) per direction, as selectors (viewport_3d.rs:7633-7640); rows 0 and 1 are unused
_ROOM_CENTRE_SEL = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0], [1, 0, 1, 1], [0, 1, 1, 1], [0, 0, 0, 1], [0, 0, 1, 1], [1, 0, 0, 1]], bool)


def room_faces_from_sectors(sectors):
    """A room's sector grid as abi.SECTOR_FACE_DTYPE records in the reference's one loop order (iter_sectors, world/geometry.rs:2828-2835):
    gx outer, gz inner; inside a sector floor, ceiling, the north, east, south and west walls by i, then the nwse and the nesw walls.
    sectors[gx][gz] is None or a mapping with the optional keys floor, ceiling (one face) and walls_north, walls_east, walls_south,
    walls_west, walls_nwse, walls_nesw (lists of faces); a face is four heights or a mapping with "heights"."""
    rows = []
    for gx, col in enumerate(sectors):
        for gz, sec in enumerate(col):
            if sec is None:
                continue
            for key, kind in _ROOM_KEYS:
                got = sec.get(key)
                if got is None:
                    continue
                faces = [got] if kind < 2 else list(got)
                for i, face in enumerate(faces):
                    h = face["heights"] if hasattr(face, "keys") else face
                    rows.append((gx, gz, kind, i, 0, tuple(float(np.float32(v)) for v in h)))
    out = T.make_sector_faces(len(rows))
    for j, r in enumerate(rows):
        out[j] = r
    return out


# ---- a room's render mesh (b32_room_build_mesh): Room::to_render_data_with_textures, world/geometry.rs:2839-3352
_BLEND_NAMES = {"Opaque": abi.OPAQUE, "Average": abi.AVERAGE, "Add": abi.ADD, "Subtract": abi.SUBTRACT, "AddQuarter": abi.ADD_QUARTER, "Erase": abi.ERASE}
_NORMAL_NAMES = {"Front": abi.NORMAL_FRONT, "Both": abi.NORMAL_BOTH, "Back": abi.NORMAL_BACK}
_SPLIT_NAMES = {"NwSe": abi.SPLIT_NWSE, "NeSw": abi.SPLIT_NESW}
_PROJECTION_NAMES = {"Default": abi.UV_DEFAULT, "Projected": abi.UV_PROJECTED}
# SplitDirection::triangle_1_corners / triangle_2_corners by [split][triangle][j]
_ROOM_TRI = np.array([[[0, 1, 2], [0, 2, 3]], [[0, 1, 3], [1, 2, 3]]], np.intp)


def _enum(v, names):
    return names[v] if isinstance(v, str) else int(v)


def _vec2s(uv):
    return [(u["x"], u["y"]) if hasattr(u, "keys") else tuple(u) for u in uv]


def _colors(cols):
    return [(c["r"], c["g"], c["b"], _enum(c.get("blend", abi.OPAQUE), _BLEND_NAMES)) if hasattr(c, "keys") else tuple(c) for c in cols]


def room_materials_from_sectors(sectors, resolve):
    """The twin of room_faces_from_sectors: one abi.FACE_MATERIAL_DTYPE record per face in the same loop order, the Options resolved as
    the reference's getters do (geometry.rs:1193-1210).  A face is a mapping with the optional keys texture, texture_2, uv, uv_2 (four
    {x, y} or pairs), colors, colors_2 (four {r, g, b, blend} or quadruples), heights_2, normal_mode, split_direction, uv_projection,
    blend_mode (names or numbers) and black_transparent -- the field names of HorizontalFace / VerticalFace; four bare heights are a face
    with every default.  resolve(texture_ref) -> (texture_id, width) or None: the reference's resolve_texture, `.unwrap_or((0, 64))`."""
    rows = []
    for gx, col in enumerate(sectors):
        for gz, sec in enumerate(col):
            if sec is None:
                continue
            for key, kind in _ROOM_KEYS:
                got = sec.get(key)
                if got is None:
                    continue
                rows += [(kind, face if hasattr(face, "keys") else {}) for face in ([got] if kind < 2 else list(got))]
    out = T.make_face_materials(len(rows))
    for j, (kind, face) in enumerate(rows):
        m = out[j]
        m["texture_id"], m["tex_width"] = resolve(face.get("texture")) or (0, 64)
        flags = 0
        if face.get("uv") is not None:
            m["uv"] = _vec2s(face["uv"]); flags |= abi.MAT_HAS_UV
        if face.get("colors") is not None:
            m["colors"] = _colors(face["colors"])
        m["colors_2"] = m["colors"]
        m["texture_id_2"], m["tex_width_2"] = m["texture_id"], m["tex_width"]
        if kind < 2:                                                          # HorizontalFace only
            if face.get("texture_2") is not None:
                m["texture_id_2"], m["tex_width_2"] = resolve(face["texture_2"]) or (0, 64)
            uv2 = face.get("uv_2") if face.get("uv_2") is not None else face.get("uv")        # get_uv_2: uv_2.or(uv)
            if uv2 is not None:
                m["uv_2"] = _vec2s(uv2); flags |= abi.MAT_HAS_UV_2
            if face.get("colors_2") is not None:
                m["colors_2"] = _colors(face["colors_2"])
            if face.get("heights_2") is not None:
                m["heights_2"] = [np.float32(v) for v in face["heights_2"]]; flags |= abi.MAT_HAS_HEIGHTS_2
            m["split_direction"] = _enum(face.get("split_direction", abi.SPLIT_NWSE), _SPLIT_NAMES)
        else:
            m["uv_projection"] = _enum(face.get("uv_projection", abi.UV_DEFAULT), _PROJECTION_NAMES)
        m["normal_mode"] = _enum(face.get("normal_mode", abi.NORMAL_FRONT), _NORMAL_NAMES)
        m["blend_mode"] = _enum(face.get("blend_mode", abi.OPAQUE), _BLEND_NAMES)
        m["black_transparent"] = 1 if face.get("black_transparent", True) else 0
        m["flags"] = flags
    return out


def _room_mesh_layout(faces, materials):
    """(sides, vertices per record, faces per record): where a record's output lies depends on (kind, normal_mode) alone."""
    sides = np.where(materials["normal_mode"] == abi.NORMAL_BOTH, 2, 1).astype(np.int64)
    return sides, np.where(faces["kind"] < 2, 6, 4) * sides, 2 * sides


def room_mesh_counts(faces, materials):
    """(n_vertices, n_faces) of room_mesh / b32_room_mesh_counts."""
    f = np.ascontiguousarray(faces, abi.SECTOR_FACE_DTYPE).reshape(-1)
    m = np.ascontiguousarray(materials, abi.FACE_MATERIAL_DTYPE).reshape(-1)
    _, nv, nf = _room_mesh_layout(f, m)
    return int(nv.sum()), int(nf.sum())


def room_mesh(faces, materials, grid):
    """Room::to_render_data_with_textures (world/geometry.rs:2839-3352) in numpy float32, every operation separately rounded in the
    reference's order: (abi.VERTEX_DTYPE array, abi.FACE_DTYPE array) -- what b32_room_build_mesh leaves in a slot, and what a host
    without it computes per drag.  As on the device, a float that is a NaN is written as 0x7FC00000."""
    f32 = np.float32
    f = np.ascontiguousarray(faces, abi.SECTOR_FACE_DTYPE).reshape(-1)
    m = np.ascontiguousarray(materials, abi.FACE_MATERIAL_DTYPE).reshape(-1)
    if len(f) != len(m):
        raise ValueError("room_mesh: one material per face")
    g = _room_grid(grid)[0]
    n = len(f)
    px, py, pz = (f32(v) for v in g["position"]); S = f32(g["sector_size"])
    sides, nv_rec, nf_rec = _room_mesh_layout(f, m)
    kind = np.minimum(f["kind"], 7).astype(np.intp)
    flat = kind < 2
    mode = m["normal_mode"]
    rec = np.arange(n)[:, None]
    neg = f32(-1.0)
    with np.errstate(all="ignore"):
        bx = px + f["gx"].astype(f32) * S
        bz = pz + f["gz"].astype(f32) * S
        bxs, bzs = bx + S, bz + S
        # ---- floors and ceilings: slot s is corner s % 3 of rendered triangle s / 3
        s12 = np.arange(12)
        t, j = (s12 // 3)[None, :], (s12 % 3)[None, :]
        second = t >= sides[:, None]
        back = (mode[:, None] == abi.NORMAL_BACK) | ((mode[:, None] == abi.NORMAL_BOTH) & ((t & 1) == 1))
        c = _ROOM_TRI[np.minimum(m["split_direction"], 1).astype(np.intp)[:, None], second.astype(np.intp), j]
        has_h2 = (m["flags"] & abi.MAT_HAS_HEIGHTS_2) != 0
        hsets = np.stack([f["heights"], np.where(has_h2[:, None], m["heights_2"], f["heights"])], axis=1).astype(f32)   # (n, 2, 4)
        hsel = hsets[rec, second.astype(np.intp)]                                  # (n, 12, 4)
        east, south = (c == 1) | (c == 2), c >= 2
        hpos = np.stack([np.where(east, bxs[:, None], bx[:, None]), py + np.take_along_axis(hsel, c[..., None], 2)[..., 0],
                         np.where(south, bzs[:, None], bz[:, None])], axis=-1)
        y0 = py + hsets[..., 0]
        e1 = ((bxs - bx)[:, None], (py + hsets[..., 1]) - y0, (bz - bz)[:, None])
        e2 = ((bx - bx)[:, None], (py + hsets[..., 3]) - y0, (bzs - bz)[:, None])
        fl = (kind == 0)[:, None]
        a = tuple(np.where(fl, u, v) for u, v in zip(e2, e1))                      # floor: edge2.cross(edge1); ceiling: edge1.cross(edge2)
        b = tuple(np.where(fl, u, v) for u, v in zip(e1, e2))
        nx = a[1] * b[2] - a[2] * b[1]
        ny = a[2] * b[0] - a[0] * b[2]
        nz = a[0] * b[1] - a[1] * b[0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        nrm = np.stack([np.where(ln == 0, f32(0.0), q / ln) for q in (nx, ny, nz)], axis=-1).astype(f32)       # (n, 2, 3)
        hnrm = nrm[rec, second.astype(np.intp)]
        hnrm = np.where(back[..., None], hnrm * neg, hnrm)
        w1, w2 = m["tex_width"], m["tex_width_2"]
        first = ~second | (((m["flags"] & abi.MAT_HAS_UV_2) == 0) & (w1 == w2))[:, None]
        has = np.where(first, ((m["flags"] & abi.MAT_HAS_UV) != 0)[:, None], ((m["flags"] & abi.MAT_HAS_UV_2) != 0)[:, None])
        sc = f32(32.0) / np.where(first, w1[:, None], w2[:, None]).astype(f32)
        uo, vo = f["gx"].astype(f32)[:, None] * sc, f["gz"].astype(f32)[:, None] * sc
        duv = np.stack([np.where(east, uo + sc, uo), np.where(south, vo + sc, vo)], axis=-1)
        ouv = np.where(first[..., None], m["uv"][rec, c], m["uv_2"][rec, c])
        huv = np.where(has[..., None], ouv, duv)
        hcol = np.where(second[..., None], m["colors_2"][rec, c], m["colors"][rec, c])
        # ---- walls: slot s is corner s % 4 of side s / 4; a diagonal's corner i is the hover's corner i ^ 1
        side, i = (s12 // 4)[None, :], np.broadcast_to((s12 % 4)[None, :], (n, 12))
        wback = (mode[:, None] == abi.NORMAL_BACK) | (side != 0)
        k = np.where((kind >= 6)[:, None], i ^ 1, i)
        wpos = np.stack([np.where(_ROOM_XSEL[kind[:, None], k], bxs[:, None], bx[:, None]), py + f["heights"][rec, k],
                         np.where(_ROOM_ZSEL[kind[:, None], k], bzs[:, None], bz[:, None])], axis=-1)
        d = f32(1.0) / np.sqrt(f32(2.0))
        z = f32(0.0)
        table = np.array([[z, z, z], [z, z, z], [z, z, 1], [-1, z, z], [z, z, -1], [1, z, z], [d, z, -d], [d, z, d]], f32)
        wnrm = np.broadcast_to(table[kind][:, None, :], (n, 12, 3))
        wnrm = np.where(wback[..., None], wnrm * neg, wnrm)
        ws = (f32(32.0) / w1.astype(f32))[:, None]
        along = np.where((kind == 3) | (kind == 5), f["gz"], f["gx"]).astype(f32)[:, None] * ws
        right = (i == 1) | (i == 2)
        wuv = np.stack([np.where(right, along + ws, along), np.where(i < 2, ws, f32(0.0))], axis=-1)
        wuv = np.where(((m["flags"] & abi.MAT_HAS_UV) != 0)[:, None, None], m["uv"][rec, i], wuv)
        proj = ((-(py + f["heights"][rec, i])) / S) * ws
        wuv[..., 1] = np.where((m["uv_projection"] == abi.UV_PROJECTED)[:, None], proj, wuv[..., 1])
        wcol = m["colors"][rec, i]
    fl3 = flat[:, None, None]
    valid = s12[None, :] < nv_rec[:, None]
    v = T.make_vertices(int(nv_rec.sum()))
    for name, hh, ww in (("pos", hpos, wpos), ("uv", huv, wuv), ("normal", hnrm, wnrm)):
        arr = np.ascontiguousarray(np.where(fl3, hh, ww)[valid], f32)
        arr.view(np.uint32)[np.isnan(arr)] = 0x7FC00000
        v[name] = arr
    col = np.where(fl3, hcol, wcol)[valid]
    v["r"], v["g"], v["b"], v["blend"] = col[:, 0], col[:, 1], col[:, 2], col[:, 3]
    # ---- faces: slot k < 2 * sides; indices are absolute
    first_v = (np.cumsum(nv_rec) - nv_rec).astype(np.int64)[:, None]
    k4 = np.arange(4)[None, :]
    hsecond = k4 >= sides[:, None]
    hback = (mode[:, None] == abi.NORMAL_BACK) | ((mode[:, None] == abi.NORMAL_BOTH) & ((k4 & 1) == 1))
    flip = np.where(hback, (kind == 0)[:, None], (kind != 0)[:, None])
    hb = first_v + 3 * k4
    hidx = np.stack([hb, np.where(flip, hb + 2, hb + 1), np.where(flip, hb + 1, hb + 2)], axis=-1)
    htex = np.where(hsecond, m["texture_id_2"][:, None], m["texture_id"][:, None])
    wside, ww = k4 // 2, k4 % 2
    wb = first_v + 4 * wside
    wbk = (mode[:, None] == abi.NORMAL_BACK) | (wside != 0)
    widx = np.stack([wb, np.where(wbk, wb + 1 + ww, wb + 2 + ww), np.where(wbk, wb + 2 + ww, wb + 1 + ww)], axis=-1)
    fvalid = k4 < nf_rec[:, None]
    out = np.zeros(int(nf_rec.sum()), abi.FACE_DTYPE)
    out["v"] = np.where(fl3, hidx, widx)[fvalid].astype(np.uint32)
    out["texture_id"] = np.where(flat[:, None], htex, m["texture_id"][:, None])[fvalid]
    out["black_transparent"] = np.broadcast_to((m["black_transparent"] != 0)[:, None], (n, 4))[fvalid]
    out["blend_mode"] = np.broadcast_to(m["blend_mode"][:, None], (n, 4))[fvalid]
    out["editor_alpha"] = 255
    return v, out


def _room_grid(grid):
    """(position, sector_size) or an abi.ROOM_GRID_DTYPE record -> one abi.ROOM_GRID_DTYPE record."""
    if isinstance(grid, np.ndarray) and grid.dtype == abi.ROOM_GRID_DTYPE:
        return grid.reshape(-1)[:1].copy()
    g = np.zeros(1, abi.ROOM_GRID_DTYPE)
    pos, size = grid if len(grid) == 2 else (grid, abi.SECTOR_SIZE)
    g["position"][0] = pos; g["sector_size"] = size
    return g


class RoomMirror:
    """find_hovered_elements' three sector loops (editor/viewport_3d.rs:7050-7281) and find_selections_in_rect (:7512-7655) for one room in
    numpy float32: what b32_room_hover / b32_room_box_select compute, and what a host without this library walks per mouse move.  The
    constructor does what the reference does once per frame (derive and project every corner); hover() and box_select() answer one
    cursor / rectangle with vectorised f32 operations, each separately rounded in the reference's order."""

    def __init__(self, faces, grid, camera, w, h):
        f32 = np.float32
        self.faces = f = np.ascontiguousarray(faces, abi.SECTOR_FACE_DTYPE).reshape(-1)
        self.grid = g = _room_grid(grid)[0]
        self.camera, self.w, self.h = camera, w, h
        self.n = len(f)
        px, py, pz = (f32(v) for v in g["position"]); S = f32(g["sector_size"])
        with np.errstate(all="ignore"):
            self.bx = bx = px + f["gx"].astype(f32) * S
            self.bz = bz = pz + f["gz"].astype(f32) * S
            kind = np.minimum(f["kind"], 7)
            x = np.where(_ROOM_XSEL[kind], (bx + S)[:, None], bx[:, None])
            z = np.where(_ROOM_ZSEL[kind], (bz + S)[:, None], bz[:, None])
            y = py + f["heights"]
            sx, sy, d, some = _project_f32(x.reshape(-1), y.reshape(-1).astype(f32), z.reshape(-1), camera, w, h, None)
        self.sx, self.sy, self.d, self.some = (a.reshape(-1, 4) for a in (sx, sy, d, some))

    @staticmethod
    def _triangle(px, py, x0, y0, e0, x1, y1, e1, x2, y2, e2):
        """(inside, depth): point_in_triangle_2d (math.rs:687-706), interpolate_depth_in_triangle (viewport_3d.rs:7485-7508)."""
        f32 = np.float32
        d1 = (px - x1) * (y0 - y1) - (x0 - x1) * (py - y1)
        d2 = (px - x2) * (y1 - y2) - (x1 - x2) * (py - y2)
        d3 = (px - x0) * (y2 - y0) - (x2 - x0) * (py - y0)
        has_neg = (d1 < 0) | (d2 < 0) | (d3 < 0)
        has_pos = (d1 > 0) | (d2 > 0) | (d3 > 0)
        area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
        w0 = ((x1 - px) * (y2 - py) - (x2 - px) * (y1 - py)) / area
        w1 = ((x2 - px) * (y0 - py) - (x0 - px) * (y2 - py)) / area
        w2 = f32(1.0) - w0 - w1
        depth = np.where(np.abs(area) < f32(0.0001), (e0 + e1 + e2) / f32(3.0), w0 * e0 + w1 * e1 + w2 * e2).astype(f32)
        return ~(has_neg & has_pos), depth

    def hover(self, mx, my, vertex_threshold=abi.ROOM_VERTEX_THRESHOLD, edge_threshold=abi.ROOM_EDGE_THRESHOLD):
        """One abi.ROOM_HOVER_DTYPE record: all three loops, raw (room_hover_winner() is the reference's answer)."""
        f32 = np.float32
        px, py = f32(mx), f32(my)
        r = np.zeros((), abi.ROOM_HOVER_DTYPE)
        for k in ("vertex_rec", "vertex_corner", "edge_rec", "edge_idx", "face_rec"):
            r[k] = abi.HOVER_NONE
        if not self.n:
            return r
        sx, sy, d, some = self.sx, self.sy, self.d, self.some
        with np.errstate(all="ignore"):
            # vertices, viewport_3d.rs:7050-7068
            dx, dy = px - sx, py - sy
            dist = np.sqrt(dx * dx + dy * dy)
            c = np.nonzero((some & (dist < f32(vertex_threshold))).reshape(-1))[0]
            hit, j, depth = _closest_in_order(c, d.reshape(-1)[c])
            if hit:
                r["vertex_rec"], r["vertex_corner"] = j >> 2, j & 3
                r["vertex_dist"] = dist.reshape(-1)[j]; r["vertex_depth"] = depth
            # edges (k, (k + 1) % 4), viewport_3d.rs:7078-7096
            x0, y0, e0 = sx, sy, d
            x1, y1, e1 = (np.roll(a, -1, axis=1) for a in (sx, sy, d))
            ok = some & np.roll(some, -1, axis=1)
            ex, ey = x1 - x0, y1 - y0
            len_sq = ex * ex + ey * ey
            tt = ((px - x0) * ex + (py - y0) * ey) / len_sq
            tt = np.where(tt < f32(0.0), f32(0.0), tt)                          # f32::clamp: a NaN and -0.0 stay
            tt = np.where(tt > f32(1.0), f32(1.0), tt)
            qx, qy = px - (x0 + tt * ex), py - (y0 + tt * ey)
            p0x, p0y = px - x0, py - y0
            dist = np.where(len_sq < f32(1e-6), np.sqrt(p0x * p0x + p0y * p0y), np.sqrt(qx * qx + qy * qy)).astype(f32)
            edepth = np.where(len_sq < f32(0.0001), (e0 + e1) * f32(0.5), e0 + tt * (e1 - e0)).astype(f32)
            c = np.nonzero((ok & (dist < f32(edge_threshold))).reshape(-1))[0]
            hit, j, depth = _closest_in_order(c, edepth.reshape(-1)[c])
            if hit:
                r["edge_rec"], r["edge_idx"] = j >> 2, j & 3
                r["edge_dist"] = dist.reshape(-1)[j]; r["edge_depth"] = depth
            # faces, check_quad_hit_with_depth, viewport_3d.rs:7436-7481
            col = lambda a, k: a[:, k]
            in_a, dep_a = self._triangle(px, py, *(col(a, k) for k in (0, 1, 2) for a in (sx, sy, d)))
            in_b, dep_b = self._triangle(px, py, *(col(a, k) for k in (0, 2, 3) for a in (sx, sy, d)))
            all4 = some.all(axis=1)
            c = np.nonzero(all4 & (in_a | in_b))[0]
            hit, j, depth = _closest_in_order(c, np.where(in_a, dep_a, dep_b)[c])
            if hit:
                r["face_rec"] = j; r["face_depth"] = depth
        return r

    def centres(self):
        """The (x, y, z) the rubber band projects per record: face_center_in_rect / wall_center_in_rect, viewport_3d.rs:7597-7655."""
        f32 = np.float32
        f, g = self.faces, self.grid
        py = f32(g["position"][1]); S = f32(g["sector_size"])
        h = f["heights"]
        with np.errstate(all="ignore"):
            avg = (((h[:, 0] + h[:, 1]) + h[:, 2]) + h[:, 3]) / f32(4.0)
            kind = np.minimum(f["kind"], 7)
            sel = _ROOM_CENTRE_SEL[kind]
            bx, bz = self.bx, self.bz
            x0, z0, x1, z1 = (np.where(sel[:, k], (b + S), b) for k, b in ((0, bx), (1, bz), (2, bx), (3, bz)))
            flat = kind < 2
            cx = np.where(flat, bx + S / f32(2.0), (x0 + x1) / f32(2.0))
            cz = np.where(flat, bz + S / f32(2.0), (z0 + z1) / f32(2.0))
            return cx.astype(f32), (py + avg).astype(f32), cz.astype(f32)

    def box_select(self, rect, points=None):
        """(words, n_selected) for the rectangle (x0, y0, x1, y1): element i is record i, then point i - n of `points` ((m, 3) positions)."""
        f32 = np.float32
        x0, y0, x1, y1 = (f32(v) for v in rect)
        pts = np.zeros((0, 3), f32) if points is None else np.ascontiguousarray(points, f32).reshape(-1, 3)
        cx, cy, cz = self.centres() if self.n else (np.zeros(0, f32),) * 3
        with np.errstate(all="ignore"):
            x, y, z = (np.concatenate([a, pts[:, k]]) for k, a in enumerate((cx, cy, cz)))
            sx, sy, _, ok = _project_f32(x, y, z, self.camera, self.w, self.h, None)   # world_to_screen, math.rs:503-534
            sel = ok & (sx >= x0) & (sx <= x1) & (sy >= y0) & (sy <= y1)
        n = len(sel)
        bits = np.zeros(((n + 31) // 32) * 32, np.uint8)
        bits[:n] = sel
        words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
        return words, int(sel.sum())


def room_hover(faces, grid, camera, w, h, mx, my, **params):
    """Host mirror of b32_room_hover (see RoomMirror): one abi.ROOM_HOVER_DTYPE record."""
    return RoomMirror(faces, grid, camera, w, h).hover(mx, my, **params)


def room_box_select(faces, grid, camera, w, h, rect, points=None):
    """Host mirror of b32_room_box_select (see RoomMirror): (words, n_selected)."""
    return RoomMirror(faces, grid, camera, w, h).box_select(rect, points)


def room_hover_winner(result):
    """find_hovered_elements' answer (viewport_3d.rs:7283-7336) of a room hover record: 0 vertex, 1 edge, 2 face, -1 nothing.  The
    candidates (depth, type) are sorted by depth (a stable insertion sort in which a NaN compares equal to everything, as
    partial_cmp(..).unwrap_or(Equal) in the standard library's sort of so few elements); tolerance = closest * 0.01; the lowest type among
    those with |d - closest| < tolerance wins, else the closest one's type."""
    f32 = np.float32
    cand = [(f32(result[d]), t) for t, (i, d) in enumerate((("vertex_rec", "vertex_depth"), ("edge_rec", "edge_depth"), ("face_rec", "face_depth")))
            if int(result[i]) != abi.HOVER_NONE]
    if not cand:
        return -1
    for i in range(1, len(cand)):
        c, j = cand[i], i
        while j > 0 and c[0] < cand[j - 1][0]:
            cand[j] = cand[j - 1]; j -= 1
        cand[j] = c
    with np.errstate(all="ignore"):
        closest = cand[0][0]
        tolerance = closest * f32(0.01)
        near = [t for d, t in cand if np.abs(d - closest) < tolerance]
    return min(near) if near else cand[0][1]


# ---- the world editor's room overlays (editor/viewport_3d.rs:4273-4658, :4862-5362) from a room's records: b32_draw_room_overlay and its mirror
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


ROOM_OVERLAY_COLORS = {"selected_vertex": (100, 255, 100), "hover_vertex": (255, 200, 150), "selected_edge": (100, 255, 100), "hover_edge": (255, 200, 100),
                       "hover_face": (150, 200, 255), "selected": (255, 200, 80), "preview": (100, 220, 255)}
# the draw_3d_line calls of a hovered / selected face as (corner set, from, to): viewport_3d.rs:4513-4532 / :4895-4918 and the walls' five
_ROOM_FACE_LINES = {abi.SPLIT_NWSE: ((1, 0, 1), (1, 1, 2), (2, 2, 3), (2, 3, 0), (1, 0, 2), (2, 0, 2)),
                    abi.SPLIT_NESW: ((1, 0, 1), (1, 0, 3), (2, 1, 2), (2, 2, 3), (1, 1, 3), (2, 1, 3))}
_ROOM_WALL_LINES = ((0, 1), (1, 2), (2, 3), (3, 0), (0, 2))
# the preview's own (x0, z0, x1, z1) per wall direction as selectors, viewport_3d.rs:5305-5311 (rows 0 and 1 are unused): WallSouth and
# WallWest run the other way round than at every other site
_ROOM_PREVIEW_SEL = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0], [1, 0, 1, 1], [0, 1, 1, 1], [0, 0, 0, 1], [0, 0, 1, 1], [1, 0, 0, 1]], bool)


def _f32_min(a, b):
    """f32::min: a NaN loses."""
    a, b = np.float32(a), np.float32(b)
    return b if np.isnan(a) else (a if np.isnan(b) else (b if b < a else a))


def _f32_max(a, b):
    a, b = np.float32(a), np.float32(b)
    return b if np.isnan(a) else (a if np.isnan(b) else (b if b > a else a))


def room_overlay_layout(n, overlay):
    """First record of every part, the total, and the preview's rectangle and gate (viewport_3d.rs:5252-5258): {"vertices", "edges", "hover",
    "sel_faces", "sel_edges", "preview", "points", "total", "rect", "gate"} -- a function of n, the struct and the lists' lengths alone."""
    o = overlay
    if (o.sections & ~abi.ROOM_OVERLAY_ALL) or o.hover_source > 1:
        raise ValueError("RoomOverlay: unknown section bit or hover source")
    if len(o.edges) and int(o.edges[:, 1].max()) > 3:
        raise ValueError("RoomOverlay: edge_idx > 3")
    if len(o.vertices) > 1 and not (np.diff(o.vertices.astype(np.int64)) > 0).all():
        raise ValueError("RoomOverlay: vertex keys not strictly ascending")
    lay, at = {}, 0
    lay["vertices"] = at
    at += len(o.vertices) + 1 if o.sections & abi.ROOM_OVERLAY_VERTICES else 0
    lay["edges"] = at
    at += len(o.edges) if o.sections & abi.ROOM_OVERLAY_EDGES else 0
    lay["hover"] = at
    at += 7 if o.sections & abi.ROOM_OVERLAY_HOVER else 0
    lay["sel_faces"] = at
    at += 6 * len(o.faces) if o.sections & abi.ROOM_OVERLAY_SELECTED else 0
    lay["sel_edges"] = at
    at += len(o.edges) if o.sections & abi.ROOM_OVERLAY_SELECTED else 0
    x0, y0, x1, y1 = o.rect
    rect = (_f32_min(x0, x1), _f32_min(y0, y1), _f32_max(x0, x1), _f32_max(y0, y1))
    with np.errstate(all="ignore"):
        gate = bool(o.sections & abi.ROOM_OVERLAY_PREVIEW) and bool((rect[2] - rect[0]) > np.float32(3.0) or (rect[3] - rect[1]) > np.float32(3.0))
    lay["preview"] = at
    at += 4 * n if gate else 0
    lay["points"] = at
    at += 3 * len(o.points) if gate else 0
    lay["total"], lay["rect"], lay["gate"] = at, rect, gate
    return lay


def room_overlay_record_count(n, overlay):
    """How many records b32_draw_room_overlay makes for a room of n records (b32_room_overlay_record_count)."""
    return room_overlay_layout(n, overlay)["total"]


def _np_near_clip_project(P0, P1, camera, w, h):
    """The near clip of draw.rs:19-42 (viewport_3d.rs:5794-5816 is the same text) and world_to_screen on both ends for m segments at once
    in f32: (x0, y0, x1, y1 as f32, ok) -- ok: neither both behind nor an end that does not project."""
    f32 = np.float32
    pos, bx, by, bz = (np.array([f32(v) for v in getattr(camera, k)], f32) for k in ("position", "basis_x", "basis_y", "basis_z"))
    vdot = lambda r, b: (r[:, 0] * b[0] + r[:, 1] * b[1]) + r[:, 2] * b[2]
    NEAR = f32(0.1)
    vs = (f32(min(w, h)) / f32(2.0)) * f32(0.75)
    hw, hh = f32(w) / f32(2.0), f32(h) / f32(2.0)
    with np.errstate(all="ignore"):
        def project(P):
            rel = P - pos
            cx, cy, cz = vdot(rel, bx), vdot(rel, by), vdot(rel, bz)
            denom = cz + f32(5.0)
            return (cx * f32(4.0) / denom) * vs + hw, (cy * f32(4.0) / denom) * vs + hh, cz

        z0, z1 = vdot(P0 - pos, bz), vdot(P1 - pos, bz)
        b0, b1 = z0 <= NEAR, z1 <= NEAR
        t = (NEAR - z0) / (z1 - z0)
        Q = (P0 + (P1 - P0) * t[:, None]).astype(f32)
        C0 = np.where((b0 & ~b1)[:, None], Q, P0); C1 = np.where((~b0 & b1)[:, None], Q, P1)
        x0, y0, d0 = project(C0); x1, y1, d1 = project(C1)
        ok = ~(b0 & b1) & ~(d0 <= NEAR) & ~(d1 <= NEAR)
    return x0, y0, x1, y1, ok


def _np_draw_3d_lines_clipped(P0, P1, camera, w, h):
    """draw_3d_line_clipped (draw.rs:12-67) for m segments at once in f32: the near clip, world_to_screen, the cast -- no screen clip.
    Returns what _np_draw_3d_lines returns."""
    x0, y0, x1, y1, ok = _np_near_clip_project(P0, P1, camera, w, h)
    ix0, iy0, ix1, iy1 = (_ov_i32(v).astype(np.int64) for v in (x0, y0, x1, y1))
    lim = 1 << 30
    state = np.where(ok, np.where((np.abs(ix1 - ix0) >= lim) | (np.abs(iy1 - iy0) >= lim), 2, 0), 1)
    return ix0, iy0, ix1, iy1, state


def _np_draw_3d_lines(P0, P1, camera, w, h):
    """draw_3d_line (viewport_3d.rs:5687-5695, :5783-5882) for m segments at once in f32: the near clip, world_to_screen, the 16 rounds of
    clip_line_to_rect, the cast.  Returns (x0, y0, x1, y1 as int64, state): state 0 drawn, 1 dropped, 2 rejected (an extent >= 2^30)."""
    f32 = np.float32
    m = len(P0)
    x0, y0, x1, y1, ok = _np_near_clip_project(P0, P1, camera, w, h)
    with np.errstate(all="ignore"):
        xmax, ymax, one, zero = f32(w), f32(h), f32(1.0), f32(0.0)

        def outcode(x, y):
            return np.where(x < zero, 1, np.where(x >= xmax, 2, 0)) | np.where(y < zero, 8, np.where(y >= ymax, 4, 0))

        c0, c1 = outcode(x0, y0), outcode(x1, y1)
        live = np.ones(m, bool); accept = np.zeros(m, bool)
        for _ in range(16):                         # lanes that have returned keep their state
            acc = live & ((c0 | c1) == 0); rej = live & ((c0 & c1) != 0)
            accept |= acc; live &= ~(acc | rej)
            if not live.any():
                break
            co = np.where(c0 != 0, c0, c1)
            bot, top, right = (co & 4) != 0, (co & 8) != 0, (co & 2) != 0
            dx, dy = x1 - x0, y1 - y0
            xh = np.where(bot, x0 + dx * (ymax - one - y0) / dy, x0 + dx * (zero - y0) / dy)
            yv = np.where(right, y0 + dy * (xmax - one - x0) / dx, y0 + dy * (zero - x0) / dx)
            horiz = bot | top
            nx = np.where(horiz, xh, np.where(right, xmax - one, zero)).astype(f32)
            ny = np.where(horiz, np.where(bot, ymax - one, zero), yv).astype(f32)
            first = live & (co == c0); second = live & ~(co == c0)
            x0 = np.where(first, nx, x0); y0 = np.where(first, ny, y0); x1 = np.where(second, nx, x1); y1 = np.where(second, ny, y1)
            c0 = np.where(first, outcode(x0, y0), c0); c1 = np.where(second, outcode(x1, y1), c1)
    ix0, iy0, ix1, iy1 = (_ov_i32(v).astype(np.int64) for v in (x0, y0, x1, y1))
    lim = 1 << 30
    state = np.where(ok & accept, np.where((np.abs(ix1 - ix0) >= lim) | (np.abs(iy1 - iy0) >= lim), 2, 0), 1)
    return ix0, iy0, ix1, iy1, state


def room_overlay_records(faces, grid, overlay, camera, w, h, materials=None, with_counts=False):
    """The numpy / float32 mirror of b32_draw_room_overlay: the abi.PRIM_DTYPE records, place for place, that the device makes from the
    room's records (abi.SECTOR_FACE_DTYPE), its materials (abi.FACE_MATERIAL_DTYPE or None: none set) and `overlay` (a RoomOverlay, whose
    `hover` is read whatever its hover_source) -- the sections of draw_viewport_3d at viewport_3d.rs:4273-4658 and :4862-5362.
    with_counts: also (drawn, dropped, rejected), what the call adds to b32_gizmo_counts."""
    f32 = np.float32
    o = overlay
    F = np.ascontiguousarray(faces, abi.SECTOR_FACE_DTYPE).reshape(-1)
    M = None if materials is None else np.ascontiguousarray(materials, abi.FACE_MATERIAL_DTYPE).reshape(-1)
    n = len(F)
    G = _room_grid(grid)
    g = G[0]
    px, py, pz = (f32(v) for v in g["position"]); S = f32(g["sector_size"])
    lay = room_overlay_layout(n, o)
    out = noop_prims(lay["total"])
    counts = np.zeros(3, np.int64)
    col = ROOM_OVERLAY_COLORS
    lim = 1 << 30

    def corner(rec, xsel, zsel, H, k):
        """(m, 3) positions: the lattice place the selectors name, with height H[i, k[i]]"""
        with np.errstate(all="ignore"):
            bx = px + F["gx"][rec].astype(f32) * S
            bz = pz + F["gz"][rec].astype(f32) * S
            return np.stack([np.where(xsel, bx + S, bx), py + H[np.arange(len(rec)), k], np.where(zsel, bz + S, bz)], axis=1).astype(f32)

    def corners(rec, k, H=None):
        """corner k of records rec as every site but the preview places it (viewport_3d.rs:6603-6657)"""
        kind = F["kind"][rec].astype(np.int64)
        return corner(rec, _ROOM_XSEL[kind, k], _ROOM_ZSEL[kind, k], F["heights"][rec] if H is None else H, k)

    def screen(P):
        with np.errstate(all="ignore"):
            sx, sy, _cz, some = _project_f32(P[:, 0], P[:, 1], P[:, 2], camera, w, h, None)
        return sx, sy, some

    def tally(state):
        counts[:] += np.bincount(state, minlength=3)[:3]

    def lines(idx, P0, P1, rgb):
        """draw_3d_line per row into out[idx]"""
        if not len(idx):
            return
        x0, y0, x1, y1, state = _np_draw_3d_lines(P0, P1, camera, w, h)
        tally(state)
        i = idx[state == 0]
        d = state == 0
        out["x0"][i], out["y0"][i], out["x1"][i], out["y1"][i] = x0[d], y0[d], x1[d], y1[d]
        out["size"][i] = 0
        out["r"][i], out["g"][i], out["b"][i] = rgb
        out["kind"][i], out["alpha"][i] = abi.LINE_2D, 0           # (as b32_draw_gizmos leaves it: LINE_2D reads no alpha)

    def circles(idx, P, radius, rgb):
        if not len(idx):
            return
        sx, sy, some = screen(P)
        x, y = _ov_i32(sx).astype(np.int64), _ov_i32(sy).astype(np.int64)
        state = np.where(some, np.where((np.abs(x) >= lim) | (np.abs(y) >= lim), 2, 0), 1)
        tally(state)
        d = state == 0
        i = idx[d]
        out["x0"][i], out["y0"][i], out["size"][i] = x[d], y[d], np.broadcast_to(radius, len(idx))[d]
        out["r"][i], out["g"][i], out["b"][i] = rgb
        out["kind"][i], out["alpha"][i] = abi.PRIM_CIRCLE, 255

    def thick(idx, rec, e, rgb):
        """draw_edge_highlight's fb.draw_thick_line(.., 3, color) per row (:4373-4384)"""
        if not len(idx):
            return
        ax, ay, asome = screen(corners(rec, e))
        bx_, by_, bsome = screen(corners(rec, (e + 1) % 4))
        x0, y0, x1, y1 = (_ov_i32(v).astype(np.int64) for v in (ax, ay, bx_, by_))
        state = np.where(asome & bsome, np.where((np.abs(x1 - x0) >= lim) | (np.abs(y1 - y0) >= lim), 2, 0), 1)
        tally(state)
        d = state == 0
        i = idx[d]
        out["x0"][i], out["y0"][i], out["x1"][i], out["y1"][i], out["size"][i] = x0[d], y0[d], x1[d], y1[d], 3
        out["r"][i], out["g"][i], out["b"][i] = rgb
        out["kind"][i], out["alpha"][i] = abi.PRIM_THICK_LINE, 255

    def face_lines(first, rec, rgb):
        """the six slots of faces `rec` (all < n) from out[first[i]] on"""
        if not len(rec):
            return
        kind = F["kind"][rec]
        flat = kind < 2
        H1 = F["heights"][rec]
        H2, nesw = H1, np.zeros(len(rec), bool)
        if M is not None:
            H2 = np.where(((M["flags"][rec] & abi.MAT_HAS_HEIGHTS_2) != 0)[:, None], M["heights_2"][rec], H1)
            nesw = M["split_direction"][rec] == abi.SPLIT_NESW
        for j in range(6):
            for split in (abi.SPLIT_NWSE, abi.SPLIT_NESW):
                sel = flat & (nesw == (split == abi.SPLIT_NESW))
                which, a, b = _ROOM_FACE_LINES[split][j]
                H = (H1 if which == 1 else H2)[sel]
                r = rec[sel]
                lines(first[sel] + j, corners(r, np.full(len(r), a), H), corners(r, np.full(len(r), b), H), rgb)
            if j < 5:
                a, b = _ROOM_WALL_LINES[j]
                r = rec[~flat]
                lines(first[~flat] + j, corners(r, np.full(len(r), a)), corners(r, np.full(len(r), b)), rgb)

    hov = o.hover
    winner = room_hover_winner(hov)

    if o.sections & abi.ROOM_OVERLAY_VERTICES:
        keys = o.vertices.astype(np.int64)
        m = len(keys)
        hk = None
        if winner == 0 and int(hov["vertex_rec"]) < n:
            hk = int(hov["vertex_rec"]) * 4 + (int(hov["vertex_corner"]) & 3)
        rank = int(np.searchsorted(keys, hk, "left")) if hk is not None else m
        place = lay["vertices"] + np.arange(m) + (np.arange(m) >= rank)
        ok = (keys >> 2) < n
        k = keys[ok]
        circles(place[ok], corners(k >> 2, k & 3), np.where(k == o.primary_vertex, 5, 4), col["selected_vertex"])
        if hk is not None and not (rank < m and keys[rank] == hk):
            circles(np.array([lay["vertices"] + rank]), corners(np.array([hk >> 2]), np.array([hk & 3])), 4, col["hover_vertex"])

    pairs = o.edges.astype(np.int64)
    pair_ok = pairs[:, 0] < n if len(pairs) else np.zeros(0, bool)
    if (o.sections & abi.ROOM_OVERLAY_EDGES) and len(pairs):
        thick(lay["edges"] + np.nonzero(pair_ok)[0], pairs[pair_ok, 0], pairs[pair_ok, 1], col["selected_edge"])

    if o.sections & abi.ROOM_OVERLAY_HOVER:
        if winner == 1 and int(hov["edge_rec"]) < n:
            thick(np.array([lay["hover"]]), np.array([int(hov["edge_rec"])]), np.array([int(hov["edge_idx"]) & 3]), col["hover_edge"])
        fr = int(hov["face_rec"])
        if winner == 2 and fr < n and not (o.skip[0] <= fr < o.skip[0] + o.skip[1]):
            face_lines(np.array([lay["hover"] + 1]), np.array([fr]), col["hover_face"])

    if o.sections & abi.ROOM_OVERLAY_SELECTED:
        rec = o.faces.astype(np.int64)
        ok = rec < n
        face_lines((lay["sel_faces"] + 6 * np.arange(len(rec)))[ok], rec[ok], col["selected"])
        if len(pairs):
            r, e = pairs[pair_ok, 0], pairs[pair_ok, 1]
            lines(lay["sel_edges"] + np.nonzero(pair_ok)[0], corners(r, e), corners(r, (e + 1) % 4), col["selected"])

    if lay["gate"]:
        words, _ = RoomMirror(F, G, camera, w, h).box_select(lay["rect"], o.points)
        sel = np.unpackbits(words.view(np.uint8), bitorder="little")[:n + len(o.points)].astype(bool) if len(words) else np.zeros(0, bool)
        rec = np.nonzero(sel[:n])[0]
        kind = F["kind"][rec].astype(np.int64)
        flat = kind < 2
        for j in range(4):
            ka, kb = np.full(len(rec), j), np.full(len(rec), (j + 1) % 4)
            ends = []
            for k in (ka, kb):
                first_end = (k == 0) | (k == 3)                      # corners 0 and 3 stand at (x0, z0), 1 and 2 at (x1, z1)
                ps = _ROOM_PREVIEW_SEL[kind]
                xsel = np.where(flat, _ROOM_XSEL[kind, k], np.where(first_end, ps[:, 0], ps[:, 2]))
                zsel = np.where(flat, _ROOM_ZSEL[kind, k], np.where(first_end, ps[:, 1], ps[:, 3]))
                ends.append(corner(rec, xsel, zsel, F["heights"][rec], k))
            lines(lay["preview"] + 4 * rec + j, ends[0], ends[1], col["preview"])
        pt = np.nonzero(sel[n:])[0]
        P = o.points[pt]
        size = f32(64.0)
        for j in range(3):
            d = np.zeros(3, f32); d[j] = size
            with np.errstate(all="ignore"):
                lines(lay["points"] + 3 * pt + j, (P - d).astype(f32), (P + d).astype(f32), col["preview"])
    return (out, tuple(int(v) for v in counts)) if with_counts else out


# ---- the world editor's object overlays (editor/viewport_3d.rs:255-291, :7658-7697; asset/asset.rs:288-312) from resident asset parts:
# b32_draw_object_overlays, b32_scene_bounds and their mirror
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


def pack_object_parts(parts, ctx):
    """The abi.OBJECT_PART_DTYPE array of a sequence of ObjectPart for `ctx` (slots and topology handles)."""
    out = np.zeros(len(parts), abi.OBJECT_PART_DTYPE)
    for i, p in enumerate(parts):
        if p.scene is None or p.scene._slot is None:
            raise ValueError("ObjectPart: the scene must be detached into a slot")
        out[i]["slot"] = p.scene._slot.value or 0
        out[i]["topology"] = (p.topology.handle(ctx).value or 0) if p.topology is not None else 0
        out[i]["flags"] = 0 if p.visible else abi.OBJECT_PART_HIDDEN
    return out


_OBJECT_BOUNDS_START = (np.float32(np.finfo(np.float32).max), np.float32(np.finfo(np.float32).min))      # f32::MAX, f32::MIN (asset.rs:291-292)
# draw_rotated_bounding_box's corners as (x, y, z) selectors of max (viewport_3d.rs:7669-7678) and its edges (:7688-7692)
_OBJECT_BOX_CORNERS = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1], [0, 1, 0], [1, 1, 0], [1, 1, 1], [0, 1, 1]], bool)
_OBJECT_BOX_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))


def mesh_bounds(parts_vertices):
    """Asset::bounds (asset/asset.rs:288-312) over the vertices of ALL parts (a sequence of abi.VERTEX_DTYPE arrays or (n, 3) positions):
    (min, max, has_verts) in f32.  Minima start at f32::MAX and maxima at f32::MIN, f32::min / f32::max ignore a NaN, and a zero comes
    back as +0.0 (the library's one key for both zeros): what b32_scene_bounds returns for one part, and what OBJECT_BOX_MESH folds."""
    f32 = np.float32
    mn = np.full(3, _OBJECT_BOUNDS_START[0], f32); mx = np.full(3, _OBJECT_BOUNDS_START[1], f32)
    has_verts = False
    for v in parts_vertices:
        pos = _positions(v)
        if not len(pos):
            continue
        has_verts = True
        mn = np.fmin(mn, np.fmin.reduce(pos, axis=0)); mx = np.fmax(mx, np.fmax.reduce(pos, axis=0))
    zero = f32(0.0)
    return np.where(mn == zero, zero, mn).astype(f32), np.where(mx == zero, zero, mx).astype(f32), has_verts


def _object_bounds_parts(parts):
    """The parts Asset::bounds reads: all of them, hidden ones included (asset.rs:295)."""
    return list(parts)


def _object_half_edges(topology):
    """(v0, v1) of draw_asset_wireframe's loop, viewport_3d.rs:271-273: the topology's half-edges in loop order."""
    return topology.he_v0, topology.he_v1


def _object_place(P, cos_f, sin_f, world_pos):
    """viewport_3d.rs:276-285 and :7681-7685 on (m, 3) positions in f32."""
    with np.errstate(all="ignore"):
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        return np.stack([(x * cos_f - z * sin_f) + world_pos[0], y + world_pos[1], (x * sin_f + z * cos_f) + world_pos[2]], axis=1).astype(np.float32)


_object_wire_lines = _np_draw_3d_lines_clipped      # draw_asset_wireframe draws through draw_3d_line_clipped (:287)


def object_overlay_layout(parts, items):
    """First record of every item and the total: a WIRE item owns the sum of nh over its visible parts, a box 12 -- a function of the
    topologies and the kinds alone.  ValueError for what the library answers B32_E_ARG."""
    first, at = [], 0
    for it in items:
        if it.kind not in (abi.OBJECT_WIRE, abi.OBJECT_BOX_MESH, abi.OBJECT_BOX):
            raise ValueError("ObjectItem: unknown kind")
        if it.first_part < 0 or it.n_parts < 0 or it.first_part + it.n_parts > len(parts):
            raise ValueError("ObjectItem: part range outside the table")
        first.append(at)
        if it.kind == abi.OBJECT_WIRE:
            for p in parts[it.first_part:it.first_part + it.n_parts]:
                if p.visible:
                    if p.topology is None:
                        raise ValueError("ObjectItem: a visible part of a WIRE item needs a topology")
                    at += len(p.topology.poly_verts)
        else:
            at += abi.OBJECT_BOX_SLOTS
    return first, at


def object_overlay_record_count(parts, items):
    """How many records b32_draw_object_overlays makes (b32_object_overlay_record_count)."""
    return object_overlay_layout(parts, items)[1]


def object_overlay_records(parts, items, camera, w, h, with_counts=False):
    """The numpy / float32 mirror of b32_draw_object_overlays: the abi.PRIM_DTYPE records, place for place, that the device makes from the
    parts' vertices (ObjectPart.vertices) and topologies for `items` (ObjectItem) -- draw_asset_wireframe (viewport_3d.rs:255-291),
    Asset::bounds (asset.rs:288-312) and draw_rotated_bounding_box (viewport_3d.rs:7658-7697), one call after another.
    with_counts: also (drawn, dropped, rejected), what the call adds to b32_gizmo_counts."""
    f32 = np.float32
    first, total = object_overlay_layout(parts, items)
    out = noop_prims(total)
    counts = np.zeros(3, np.int64)

    def lines(where, x0, y0, x1, y1, state, color, alpha):
        """the calls' records at the places `where`: those that draw are filled in, every call is counted"""
        draw = state == 0
        idx = where[draw]
        for f, v in (("x0", x0), ("y0", y0), ("x1", x1), ("y1", y1)):
            out[f][idx] = v[draw]
        out["kind"][idx] = abi.LINE_2D; out["size"][idx] = 0; out["alpha"][idx] = alpha
        out["r"][idx], out["g"][idx], out["b"][idx], out["blend"][idx] = color.r, color.g, color.b, color.blend
        counts[:] += np.bincount(state, minlength=3)[:3]

    for it, at in zip(items, first):
        mine = parts[it.first_part:it.first_part + it.n_parts]
        if it.kind == abi.OBJECT_WIRE:
            for p in mine:
                if not p.visible:
                    continue
                v0, v1 = (np.asarray(v, np.int64) for v in _object_half_edges(p.topology))
                nv = len(p.vertices)
                good = (v0 >= 0) & (v0 < nv) & (v1 >= 0) & (v1 < nv)
                counts[1] += int((~good).sum())                  # an index >= nv: the no-op, dropped
                g = np.nonzero(good)[0]
                if len(g):
                    P0 = _object_place(p.vertices[v0[g]], it.cos_f, it.sin_f, it.world_pos)
                    P1 = _object_place(p.vertices[v1[g]], it.cos_f, it.sin_f, it.world_pos)
                    lines(at + g, *_object_wire_lines(P0, P1, camera, w, h), it.color, 255)
                at += len(v0)
            continue
        if it.kind == abi.OBJECT_BOX_MESH:
            mn, mx, has_verts = mesh_bounds([p.vertices for p in _object_bounds_parts(mine)])
            if not has_verts:                                    # bounds() is None: no call; the item counts once, as dropped
                counts[1] += 1
                continue
        else:
            mn, mx = np.array(it.box[0], f32), np.array(it.box[1], f32)
        corners = _object_place(np.where(_OBJECT_BOX_CORNERS, mx, mn).astype(f32), it.cos_f, it.sin_f, it.world_pos)
        ea = np.array([e[0] for e in _OBJECT_BOX_EDGES]); eb = np.array([e[1] for e in _OBJECT_BOX_EDGES])
        lines(at + np.arange(abi.OBJECT_BOX_SLOTS), *_np_draw_3d_lines(corners[ea], corners[eb], camera, w, h), it.color, 0)
    return (out, tuple(int(v) for v in counts)) if with_counts else out


class Room:
    """A resident room (b32_room): its grid and its abi.SECTOR_FACE_DTYPE records on the device.  update() is a height drag."""

    def __init__(self, ctx, faces, grid=((0.0, 0.0, 0.0), abi.SECTOR_SIZE)):
        self.ctx = getattr(ctx, "ctx", ctx)
        f = np.ascontiguousarray(faces, abi.SECTOR_FACE_DTYPE).reshape(-1)
        g = _room_grid(grid)
        self.n = len(f)
        self._h = C.c_void_p()
        _chk(self.ctx.lib.b32_room_create(self.ctx.h, g.ctypes.data, f.ctypes.data if len(f) else None, len(f), C.byref(self._h)), "b32_room_create")

    def update(self, first=0, faces=None, grid=None):
        """b32_room_update: records [first, first + len(faces)) and / or the grid."""
        f = np.zeros(0, abi.SECTOR_FACE_DTYPE) if faces is None else np.ascontiguousarray(faces, abi.SECTOR_FACE_DTYPE).reshape(-1)
        g = _room_grid(grid) if grid is not None else None
        _chk(self.ctx.lib.b32_room_update(self.ctx.h, self._h, g.ctypes.data if g is not None else None, int(first), len(f),
                                          f.ctypes.data if len(f) else None), "b32_room_update")

    def set_materials(self, materials):
        """b32_room_set_materials: one abi.FACE_MATERIAL_DTYPE record per face (room_materials_from_sectors)."""
        m = np.ascontiguousarray(materials, abi.FACE_MATERIAL_DTYPE).reshape(-1)
        if len(m) != self.n:
            raise ValueError("set_materials: one material per face")
        _chk(self.ctx.lib.b32_room_set_materials(self.ctx.h, self._h, m.ctypes.data if len(m) else None), "b32_room_set_materials")

    def update_materials(self, first, materials):
        """b32_room_update_materials: records [first, first + len(materials)); ordered on the stream like update()."""
        m = np.ascontiguousarray(materials, abi.FACE_MATERIAL_DTYPE).reshape(-1)
        _chk(self.ctx.lib.b32_room_update_materials(self.ctx.h, self._h, int(first), len(m), m.ctypes.data if len(m) else None), "b32_room_update_materials")

    def mesh_counts(self):
        """b32_room_mesh_counts: (n_vertices, n_faces) of the mesh build_mesh would write now."""
        nv, nf = C.c_uint32(), C.c_uint32()
        _chk(self.ctx.lib.b32_room_mesh_counts(self._h, C.byref(nv), C.byref(nf)), "b32_room_mesh_counts")
        return int(nv.value), int(nf.value)

    def build_mesh(self, scene=None):
        """b32_room_build_mesh: the room's render mesh into `scene` (a ResidentScene, detached or not; None: the context's resident
        scene), whose textures stay and whose geometry is replaced.  One launch, no upload, no host synchronisation."""
        _chk(self.ctx.lib.b32_room_build_mesh(self.ctx.h, self._h, scene._handle() if scene is not None else None), "b32_room_build_mesh")
        if scene is not None:
            scene.n_vertices, scene.n_faces = self.mesh_counts()

    def close(self):
        if self._h and getattr(self.ctx, "h", None):
            self.ctx.lib.b32_room_destroy(self.ctx.h, self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class RoomHoverResult:
    """What b32_room_hover_async delivers into `buf` (48 bytes) once its ticket is done."""

    def __init__(self, buf, owner=None):
        self.buf, self._owner = buf, owner

    @property
    def record(self):
        return self.buf[:48].view(abi.ROOM_HOVER_DTYPE)[0].copy()

    close = HoverResult.close


def _pack_placement(placement):
    if placement is None or isinstance(placement, abi.B32Placement):
        return placement
    return placement.pack()


class Context:
    """One b32_ctx: one GPU, one stream, one device-resident framebuffer and scene."""

    def __init__(self, device=0):
        self.lib = abi.load_library()
        h = C.c_void_p()
        _chk(self.lib.b32_create(device, C.byref(h)), "b32_create")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.b32_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        """Run on a caller-owned hipStream_t.  torch reports its default stream as handle 0, which the C ABI reads as "the
        context's own (non-blocking) stream" -- work enqueued there is NOT ordered with torch's default stream.  So 0 is mapped
        to hipStreamLegacy (handle 1), the legacy default stream torch actually uses."""
        HIP_STREAM_LEGACY = 1
        _chk(self.lib.b32_set_stream(self.h, stream_ptr if stream_ptr else HIP_STREAM_LEGACY), "b32_set_stream")

    def use_own_stream(self):
        _chk(self.lib.b32_set_stream(self.h, None), "b32_set_stream")

    def synchronize(self):
        _chk(self.lib.b32_synchronize(self.h), "b32_synchronize")

    def set_profiling(self, level):
        _chk(self.lib.b32_set_profiling(self.h, level), "b32_set_profiling")

    def set_profiling_stride(self, every):
        """b32_set_profiling_stride: HIP events on every `every`-th frame only (an event pair per frame costs the stream microseconds)."""
        _chk(self.lib.b32_set_profiling_stride(self.h, int(every)), "b32_set_profiling_stride")

    def set_async_depth(self, deep):
        """b32_set_async_depth: 0 = safe (default), 1 = large-scene frames back to back, a dropped one is reported by finish()."""
        _chk(self.lib.b32_set_async_depth(self.h, int(deep)), "b32_set_async_depth")

    ROUTES = ("direct_bin", "inline_bin", "counting_sort", "keyed", "redraw_region", "redraw_global_sort", "redraw_pairs", "pipelined", "lds_atlas", "wire_tiles", "span_cover",
              "flag_join", "event_join", "poll_join", "line_tiles", "line_scan", "prim_tiles", "prim_scan")
    WORLD_ROUTES = ("world_tiles", "world_scan")      # b32_route_count 18, 19: b32_draw_world batches (they count under prim_tiles / prim_scan too)
    OBJECT_ROUTES = ("bounds_reductions",)            # b32_route_count 20: reductions of a slot's bounds launched (object overlays, b32_scene_bounds)

    ROUTE_SORT_FREE, ROUTE_CUT_TILES, ROUTE_INLINE_BIN, ROUTE_DIRECT_BIN, ROUTE_WIDE_GROUPS, ROUTE_PACKED_STREAMS, ROUTE_PIPELINE, ROUTE_TEX_CACHE, ROUTE_BATCH, ROUTE_LDS_ATLAS, ROUTE_WIRE_TILES, ROUTE_SPAN_COVER, ROUTE_STAGGER, ROUTE_LINE_TILES, ROUTE_PRIM_TILES = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384

    # ---- a frame of several meshes (scene.rs:112-261): b32_frame_begin / _add_scene / _end
    def frame_begin(self, camera, settings):
        """One camera, base settings and light list for the frame; the meshes follow with frame_add (resident scenes in slots)."""
        cam = camera.pack()
        st, keep = settings.pack()
        self._frame_keep = (cam, st, keep)
        _chk(self.lib.b32_frame_begin(self.h, C.byref(cam), C.byref(st)), "b32_frame_begin")

    def frame_add(self, scene, ambient=None, backface_cull=None, backface_wireframe=None, fog=None, placement=None):
        """Append a detached ResidentScene with its per-mesh parameters (None: the base settings' value; fog None: no fog).
        placement: a Placement (or abi.B32Placement) for this draw of the slot -- the same slot may be added any number of times."""
        st = self._frame_keep[1]
        p = abi.B32MeshParams()
        p.ambient = float(st.ambient if ambient is None else ambient)
        p.backface_cull = int(st.backface_cull if backface_cull is None else bool(backface_cull))
        p.backface_wireframe = int(st.backface_wireframe if backface_wireframe is None else bool(backface_wireframe))
        fg = T.pack_fog(fog)
        p.has_fog = 0 if fg is None else 1
        if fg is not None:
            p.fog = fg
        scene.detach()
        if placement is not None:
            pl = _pack_placement(placement)
            _chk(self.lib.b32_frame_add_scene_placed(self.h, scene._slot, C.byref(p), C.byref(pl) if pl is not None else None), "b32_frame_add_scene_placed")
            return
        _chk(self.lib.b32_frame_add_scene(self.h, scene._slot, C.byref(p)), "b32_frame_add_scene")

    def frame_end(self):
        _chk(self.lib.b32_frame_end(self.h), "b32_frame_end")

    def frame_submit(self, table):
        """b32_frame_submit: the frame recorded by make_frame_table, in one call."""
        if len(table) == 8:                               # a placed table: b32_frame_submit_placed
            cam, st, _keep, slots, params, n, places, has_place = table
            _chk(self.lib.b32_frame_submit_placed(self.h, C.byref(cam), C.byref(st), slots, C.cast(params, C.c_void_p), C.cast(places, C.c_void_p),
                                                  C.cast(has_place, C.c_void_p), n), "b32_frame_submit_placed")
            return
        cam, st, _keep, slots, params, n = table
        _chk(self.lib.b32_frame_submit(self.h, C.byref(cam), C.byref(st), slots, C.cast(params, C.c_void_p), n), "b32_frame_submit")

    @staticmethod
    def set_table_placements(table, placements):
        """Rewrites the placements of a placed frame table in place (objects that move every frame: nothing else is packed again)."""
        places, has_place = table[6], table[7]
        for i, pl in enumerate(placements):
            p = _pack_placement(pl)
            has_place[i] = 0 if p is None else 1
            if p is not None:
                places[i] = p

    @staticmethod
    def make_frame_table(camera, settings, scenes, fogs=None, ambients=None, placements=None, backface_culls=None):
        """Packs camera, base settings and a list of detached ResidentScenes (+ per-mesh fog / ambient) once, for frame_submit.
        placements: one Placement (or None) per entry -- the table then goes through b32_frame_submit_placed, and the same scene may
        appear any number of times; backface_culls: per-entry culling (per part: double_sided, scene.rs:133-137)."""
        cam = camera.pack()
        st, keep = settings.pack()
        n = len(scenes)
        slots = (C.c_void_p * n)()
        params = (abi.B32MeshParams * n)()
        for i, sc in enumerate(scenes):
            sc.detach()
            slots[i] = sc._slot
            params[i].ambient = float(st.ambient if ambients is None or ambients[i] is None else ambients[i])
            params[i].backface_cull = int(st.backface_cull); params[i].backface_wireframe = int(st.backface_wireframe)
            fg = T.pack_fog(fogs[i]) if fogs is not None else None
            params[i].has_fog = 0 if fg is None else 1
            if fg is not None:
                params[i].fog = fg
            if backface_culls is not None and backface_culls[i] is not None:
                params[i].backface_cull = int(bool(backface_culls[i]))
                params[i].backface_wireframe = int(st.backface_wireframe and bool(backface_culls[i]))
        if placements is None:
            return cam, st, keep, slots, params, n
        table = (cam, st, keep, slots, params, n, (abi.B32Placement * n)(), (C.c_uint8 * n)())
        Context.set_table_placements(table, placements)
        return table

    # ---- the presenter's copy without a host round trip per frame (b32_fb_download_async + tickets)
    def host_alloc(self, nbytes):
        """b32_host_alloc: page-locked host memory as a numpy uint8 array (freed by host_free)."""
        p = self.lib.b32_host_alloc(int(nbytes))
        if not p:
            raise MemoryError("b32_host_alloc")
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(int(nbytes),))
        return arr, p

    def host_free(self, p):
        self.lib.b32_host_free(p)

    def download_async(self, host_ptr):
        t = C.c_uint64()
        _chk(self.lib.b32_fb_download_async(self.h, host_ptr, C.byref(t)), "b32_fb_download_async")
        return int(t.value)

    def ticket_wait(self, ticket):
        _chk(self.lib.b32_ticket_wait(self.h, int(ticket)), "b32_ticket_wait")

    def ticket_done(self, ticket):
        d = C.c_int()
        _chk(self.lib.b32_ticket_poll(self.h, int(ticket), C.byref(d)), "b32_ticket_poll")
        return bool(d.value)

    # ---- picking (b32_pick_meshes): which placed resident mesh, and which of its triangles, is under the cursor
    @staticmethod
    def make_pick_table(items):
        """Packs [(detached ResidentScene, placement)] once; set_pick_placements rewrites the placements in place."""
        n = len(items)
        slots = (C.c_void_p * max(n, 1))()
        places = (abi.B32Placement * max(n, 1))()
        for i, (sc, _) in enumerate(items):
            slots[i] = sc._slot if sc is not None else None
        table = (slots, places, n)
        Context.set_pick_placements(table, [pl for _, pl in items])
        return table

    @staticmethod
    def set_pick_placements(table, placements):
        for i, pl in enumerate(placements):
            c, s, w = _placement_triple(pl)
            table[1][i] = abi.B32Placement(float(c), float(s), (C.c_float * 3)(*[float(x) for x in w]))

    def _pick_args(self, items, camera, mouse, ortho, cull_backfaces):
        slots, places, n = items if isinstance(items, tuple) else self.make_pick_table(items)
        cam = camera.pack() if hasattr(camera, "pack") else camera
        o = _pack_ortho(ortho)
        return (self.h, C.byref(cam), C.byref(o) if o is not None else None, float(mouse[0]), float(mouse[1]),
                abi.PICK_CULL_BACKFACES if cull_backfaces else 0, slots, C.cast(places, C.c_void_p), n), n

    def pick_meshes(self, items, camera, mouse, ortho=None, cull_backfaces=False):
        """b32_pick_meshes: items = [(detached ResidentScene, Placement)] or a make_pick_table table -> (best, hits); best = -1 when
        nothing is hit, hits = one abi.PICK_HIT_DTYPE record per item."""
        args, n = self._pick_args(items, camera, mouse, ortho, cull_backfaces)
        hits = np.zeros(n, abi.PICK_HIT_DTYPE)
        best = C.c_int32(-1)
        _chk(self.lib.b32_pick_meshes(*args, hits.ctypes.data if n else None, C.byref(best)), "b32_pick_meshes")
        return int(best.value), hits

    def pick_meshes_async(self, items, camera, mouse, ortho=None, cull_backfaces=False, out=None):
        """b32_pick_meshes_async -> (ticket, PickResult).  out: an (array, pointer) pair from host_alloc of at least 16 + 16 * n bytes to
        deliver into (reused from frame to frame); None: page-locked memory of the result's own, released by PickResult.close()."""
        args, n = self._pick_args(items, camera, mouse, ortho, cull_backfaces)
        need = abi.PICK_HEADER_BYTES + 16 * n
        own = out is None
        arr, ptr = self.host_alloc(need) if own else out
        if len(arr) < need:
            raise ValueError("pick_meshes_async: the result buffer is too small")
        t = C.c_uint64()
        rc = self.lib.b32_pick_meshes_async(*args, ptr, C.byref(t))
        if rc != abi.B32_OK and own:
            self.host_free(ptr)
        _chk(rc, "b32_pick_meshes_async")
        return int(t.value), PickResult(arr, n, (self, ptr) if own else None)

    # ---- hover and box selection (b32_hover_mesh, b32_box_select): one detached ResidentScene and a Topology
    def _hover_args(self, scene, topology, camera, mouse, ortho, placement, see_through, mirror_axis, mirror_threshold, vertex_threshold, edge_threshold):
        prm = np.zeros(1, abi.HOVER_PARAMS_DTYPE)
        prm["mx"], prm["my"] = mouse
        prm["vertex_threshold"], prm["edge_threshold"] = vertex_threshold, edge_threshold
        prm["flags"] = abi.HOVER_SEE_THROUGH if see_through else 0
        prm["mirror_axis"], prm["mirror_threshold"] = mirror_axis, mirror_threshold
        return self._mesh_args(scene, topology, camera, ortho, placement) + (prm,)

    def _mesh_args(self, scene, topology, camera, ortho, placement):
        cam = camera.pack() if hasattr(camera, "pack") else camera
        o = _pack_ortho(ortho)
        pl = None
        if placement is not None:
            c, s, w = _placement_triple(placement)
            pl = abi.B32Placement(float(c), float(s), (C.c_float * 3)(*[float(x) for x in w]))
        top = topology.handle(self) if topology is not None else None
        return (self.h, C.byref(cam), C.byref(o) if o is not None else None, scene._slot, top, C.byref(pl) if pl is not None else None), (cam, o, pl)

    def hover_mesh(self, scene, topology, camera, mouse, ortho=None, placement=None, see_through=False, mirror_axis=0, mirror_threshold=1.0,
                   vertex_threshold=abi.HOVER_VERTEX_THRESHOLD, edge_threshold=abi.HOVER_EDGE_THRESHOLD):
        """b32_hover_mesh: one abi.HOVER_RESULT_DTYPE record (all three branches, raw; hovered_element() masks them)."""
        args, _keep, prm = self._hover_args(scene, topology, camera, mouse, ortho, placement, see_through, mirror_axis, mirror_threshold,
                                            vertex_threshold, edge_threshold)
        out = np.zeros(1, abi.HOVER_RESULT_DTYPE)
        _chk(self.lib.b32_hover_mesh(*args, prm.ctypes.data, out.ctypes.data), "b32_hover_mesh")
        return out[0]

    def hover_mesh_async(self, scene, topology, camera, mouse, ortho=None, placement=None, out=None, **params):
        """b32_hover_mesh_async -> (ticket, HoverResult).  out: an (array, pointer) pair from host_alloc of at least 32 bytes; None:
        page-locked memory of the result's own, released by HoverResult.close()."""
        p = dict(see_through=False, mirror_axis=0, mirror_threshold=1.0, vertex_threshold=abi.HOVER_VERTEX_THRESHOLD, edge_threshold=abi.HOVER_EDGE_THRESHOLD)
        p.update(params)
        args, _keep, prm = self._hover_args(scene, topology, camera, mouse, ortho, placement, **p)
        own = out is None
        arr, ptr = self.host_alloc(32) if own else out
        if len(arr) < 32:
            raise ValueError("hover_mesh_async: the result buffer is too small")
        t = C.c_uint64()
        rc = self.lib.b32_hover_mesh_async(*args, prm.ctypes.data, ptr, C.byref(t))
        if rc != abi.B32_OK and own:
            self.host_free(ptr)
        _chk(rc, "b32_hover_mesh_async")
        return int(t.value), HoverResult(arr, (self, ptr) if own else None)

    @staticmethod
    def _box_params(rect, mode):
        prm = np.zeros(1, abi.BOX_PARAMS_DTYPE)
        prm["x0"], prm["y0"], prm["x1"], prm["y1"] = rect
        prm["mode"] = mode
        return prm

    def box_select(self, scene, topology, camera, rect, mode=abi.BOX_VERTICES, ortho=None, placement=None, n_elements=None):
        """b32_box_select: (words, n_selected) for the rectangle (x0, y0, x1, y1).  n_elements: the slot's vertex count in mode BOX_VERTICES
        (default: the uploaded scene's), the topology's polygon count in mode BOX_POLYGONS."""
        args, _keep = self._mesh_args(scene, topology, camera, ortho, placement)
        prm = self._box_params(rect, mode)
        n = (topology.np if mode == abi.BOX_POLYGONS else scene.n_body_vertices) if n_elements is None else n_elements
        words = np.zeros((n + 31) // 32, np.uint32)
        cnt = C.c_uint32()
        _chk(self.lib.b32_box_select(*args, prm.ctypes.data, words.ctypes.data if len(words) else None, C.byref(cnt)), "b32_box_select")
        return words, int(cnt.value)

    def box_select_async(self, scene, topology, camera, rect, mode=abi.BOX_VERTICES, ortho=None, placement=None, out=None, n_elements=None):
        """b32_box_select_async -> (ticket, BoxResult); out as for hover_mesh_async, of at least 16 + 4 * ceil(n_elements / 32) bytes."""
        args, _keep = self._mesh_args(scene, topology, camera, ortho, placement)
        prm = self._box_params(rect, mode)
        n = (topology.np if mode == abi.BOX_POLYGONS else scene.n_body_vertices) if n_elements is None else n_elements
        need = abi.BOX_HEADER_BYTES + 4 * ((n + 31) // 32)
        own = out is None
        arr, ptr = self.host_alloc(need) if own else out
        if len(arr) < need:
            raise ValueError("box_select_async: the result buffer is too small")
        t = C.c_uint64()
        rc = self.lib.b32_box_select_async(*args, prm.ctypes.data, ptr, C.byref(t))
        if rc != abi.B32_OK and own:
            self.host_free(ptr)
        _chk(rc, "b32_box_select_async")
        return int(t.value), BoxResult(arr, (self, ptr) if own else None)

    # ---- room hover and box selection (b32_room_hover, b32_room_box_select): one Room
    @staticmethod
    def _room_hover_params(mouse, vertex_threshold, edge_threshold):
        prm = np.zeros(1, abi.ROOM_HOVER_PARAMS_DTYPE)
        prm["mx"], prm["my"] = mouse
        prm["vertex_threshold"], prm["edge_threshold"] = vertex_threshold, edge_threshold
        return prm

    def room_hover(self, room, camera, mouse, vertex_threshold=abi.ROOM_VERTEX_THRESHOLD, edge_threshold=abi.ROOM_EDGE_THRESHOLD):
        """b32_room_hover: one abi.ROOM_HOVER_DTYPE record (all three loops, raw; room_hover_winner() is the reference's answer)."""
        cam = camera.pack() if hasattr(camera, "pack") else camera
        prm = self._room_hover_params(mouse, vertex_threshold, edge_threshold)
        out = np.zeros(1, abi.ROOM_HOVER_DTYPE)
        _chk(self.lib.b32_room_hover(self.h, C.byref(cam), room._h, prm.ctypes.data, out.ctypes.data), "b32_room_hover")
        return out[0]

    def room_hover_async(self, room, camera, mouse, vertex_threshold=abi.ROOM_VERTEX_THRESHOLD, edge_threshold=abi.ROOM_EDGE_THRESHOLD, out=None):
        """b32_room_hover_async -> (ticket, RoomHoverResult).  out: an (array, pointer) pair from host_alloc of at least 48 bytes; None:
        page-locked memory of the result's own, released by RoomHoverResult.close()."""
        cam = camera.pack() if hasattr(camera, "pack") else camera
        prm = self._room_hover_params(mouse, vertex_threshold, edge_threshold)
        own = out is None
        arr, ptr = self.host_alloc(48) if own else out
        if len(arr) < 48:
            raise ValueError("room_hover_async: the result buffer is too small")
        t = C.c_uint64()
        rc = self.lib.b32_room_hover_async(self.h, C.byref(cam), room._h, prm.ctypes.data, ptr, C.byref(t))
        if rc != abi.B32_OK and own:
            self.host_free(ptr)
        _chk(rc, "b32_room_hover_async")
        return int(t.value), RoomHoverResult(arr, (self, ptr) if own else None)

    def room_hover_winner(self, record):
        """b32_room_hover_winner of one abi.ROOM_HOVER_DTYPE record."""
        rec = np.ascontiguousarray(record, abi.ROOM_HOVER_DTYPE).reshape(1)
        return int(self.lib.b32_room_hover_winner(rec.ctypes.data))

    @staticmethod
    def _room_points(points):
        pts = np.zeros((0, 3), np.float32) if points is None else np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        return pts, (pts.ctypes.data if len(pts) else None)

    def room_box_select(self, room, camera, rect, points=None):
        """b32_room_box_select: (words, n_selected) for the rectangle (x0, y0, x1, y1); element i is record i, then point i - n."""
        cam = camera.pack() if hasattr(camera, "pack") else camera
        pts, pp = self._room_points(points)
        words = np.zeros((room.n + len(pts) + 31) // 32, np.uint32)
        cnt = C.c_uint32()
        _chk(self.lib.b32_room_box_select(self.h, C.byref(cam), room._h, *[float(v) for v in rect], pp, len(pts),
                                          words.ctypes.data if len(words) else None, C.byref(cnt)), "b32_room_box_select")
        return words, int(cnt.value)

    def room_box_select_async(self, room, camera, rect, points=None, out=None):
        """b32_room_box_select_async -> (ticket, BoxResult); out as for room_hover_async, of at least 16 + 4 * ceil(n_elements / 32) bytes."""
        cam = camera.pack() if hasattr(camera, "pack") else camera
        pts, pp = self._room_points(points)
        need = abi.BOX_HEADER_BYTES + 4 * ((room.n + len(pts) + 31) // 32)
        own = out is None
        arr, ptr = self.host_alloc(need) if own else out
        if len(arr) < need:
            raise ValueError("room_box_select_async: the result buffer is too small")
        t = C.c_uint64()
        rc = self.lib.b32_room_box_select_async(self.h, C.byref(cam), room._h, *[float(v) for v in rect], pp, len(pts), ptr, C.byref(t))
        if rc != abi.B32_OK and own:
            self.host_free(ptr)
        _chk(rc, "b32_room_box_select_async")
        return int(t.value), BoxResult(arr, (self, ptr) if own else None)

    def finish(self) -> T.RasterTimings:
        """b32_frame_finish of whatever this context has in flight."""
        tm = abi.B32Timings()
        _chk(self.lib.b32_frame_finish(self.h, C.byref(tm)), "b32_frame_finish")
        return T.RasterTimings.from_c(tm)

    def batch_counts(self):
        return {n: int(self.lib.b32_batch_count(self.h, i)) for i, n in enumerate(("merged_draws", "single_draws", "merged_built", "frames"))}

    def set_pipeline_gate(self, permille):
        """b32_set_pipeline_gate: hold a pipelined setup kernel until the previous fill's tile cursor has come that far (include/b32raster.h)."""
        _chk(self.lib.b32_set_pipeline_gate(self.h, int(permille)), "b32_set_pipeline_gate")

    def last_shader_clock(self):
        """b32_last_shader_clock: (GHz, ms) the fused kernel of the last finished frame ran at / over; (0, 0) if it had none."""
        g, m = C.c_float(), C.c_float()
        _chk(self.lib.b32_last_shader_clock(self.h, C.byref(g), C.byref(m)), "b32_last_shader_clock")
        return float(g.value), float(m.value)

    def transparent_counts(self):
        """b32_transparent_counts: (host-side bound counted at upload, surfaces the last finished frame's setup kernel classified transparent)."""
        a, b = C.c_uint32(), C.c_uint32()
        _chk(self.lib.b32_transparent_counts(self.h, C.byref(a), C.byref(b)), "b32_transparent_counts")
        return int(a.value), int(b.value)

    def set_pipeline_depth(self, sets):
        """b32_set_pipeline_depth: 2 or 3 frame sets -- the setup kernel one or two frames ahead of the fill (include/b32raster.h)."""
        _chk(self.lib.b32_set_pipeline_depth(self.h, int(sets)), "b32_set_pipeline_depth")

    def mesh_overlay_record_count(self, topology, nv, overlay, selected=None):
        """b32_mesh_overlay_record_count (host only; the topology's device object is only read for its host copy of poly_start)."""
        o, sel = overlay.pack(selected)
        n = C.c_uint32()
        _chk(self.lib.b32_mesh_overlay_record_count(topology.handle(self) if topology is not None else None, nv, C.byref(o),
                                                    abi.ptr(sel) if len(sel) else None, C.byref(n)), "mesh_overlay_record_count")
        return int(n.value)

    def room_overlay_record_count(self, room, overlay):
        """b32_room_overlay_record_count (host only)."""
        o, (_v, e, f, _p) = overlay.pack()
        n = C.c_uint32()
        _chk(self.lib.b32_room_overlay_record_count(room._h, C.byref(o), e, f, C.byref(n)), "room_overlay_record_count")
        return int(n.value)

    def object_overlay_record_count(self, parts, items):
        """b32_object_overlay_record_count (host only; slots and topologies are only read for their counts)."""
        pa, ia = pack_object_parts(parts, self), pack_object_items(items)
        n = C.c_uint64()
        _chk(self.lib.b32_object_overlay_record_count(abi.ptr(pa) if len(pa) else None, len(pa), abi.ptr(ia) if len(ia) else None, len(ia), C.byref(n)),
             "object_overlay_record_count")
        return int(n.value)

    def gizmo_project_batch(self, items, camera: T.Camera, ortho, width, height):
        """b32_gizmo_project_batch (stage tap): the abi.PRIM_DTYPE records b32_draw_gizmos hands to the tile pass for a width x height
        framebuffer -- one per item, `size` of them for a thick line of thickness > 1 -- in item order; synchronous."""
        arr = np.ascontiguousarray(items, dtype=abi.GIZMO_ITEM_DTYPE).reshape(-1)
        # (a thickness beyond the cap is refused before anything is written)
        cap = int(sum(gizmo_record_count(int(k), min(int(s), abi.GIZMO_MAX_THICKNESS)) for k, s in zip(arr["kind"], arr["size"])))
        out = np.zeros(cap, abi.PRIM_DTYPE)
        cam = camera.pack()
        o = _pack_ortho(ortho)
        n = C.c_uint32()
        _chk(self.lib.b32_gizmo_project_batch(self.h, C.byref(cam), C.byref(o) if o is not None else None, arr.ctypes.data if len(arr) else None,
                                              len(arr), int(width), int(height), out.ctypes.data if cap else None, cap, C.byref(n)),
             "gizmo_project_batch")
        return out[:int(n.value)]

    def set_routes(self, off_mask):
        """b32_set_routes: switch internal routes off (ROUTE_* bits); results are identical on every route."""
        _chk(self.lib.b32_set_routes(self.h, int(off_mask)), "b32_set_routes")

    def set_cheap_threshold(self, den):
        """b32_set_cheap_threshold: CHEAP coverage while every texture has at most 1/den skippable texels (default 64)."""
        _chk(self.lib.b32_set_cheap_threshold(self.h, int(den)), "b32_set_cheap_threshold")

    def route_counts(self):
        """b32_route_count: how many frames of this context took each internal route (tests assert the targeted one ran)."""
        return {n: int(self.lib.b32_route_count(self.h, i)) for i, n in enumerate(self.ROUTES + self.WORLD_ROUTES + self.OBJECT_ROUTES)}

    def debug_inject(self, what):
        """b32_debug_inject: fault injection (1 = the next flag / join hand-over loses its flag; 2 = the next fused kernel does not publish its start)."""
        _chk(self.lib.b32_debug_inject(self.h, int(what)), "b32_debug_inject")

    def set_fragment_counting(self, on):
        _chk(self.lib.b32_set_fragment_counting(self.h, int(on)), "b32_set_fragment_counting")

    def last_kernel_times(self):
        names = (C.c_char_p * 8)()
        ms = (C.c_float * 8)()
        n = self.lib.b32_last_kernel_times(self.h, names, ms, 8)
        return {names[i].decode(): float(ms[i]) for i in range(n)}

    # ---- multi-GPU band exchange behind the C ABI (include/b32raster.h "multi-GPU", b32_gather.hip)
    BAND_SHARE_BYTES = 96

    def band_export(self) -> bytes:
        """b32_band_export (root): the 96-byte share of this context's library-owned framebuffer + epoch words, for the other ranks."""
        buf = C.create_string_buffer(self.BAND_SHARE_BYTES)
        _chk(self.lib.b32_band_export(self.h, C.cast(buf, C.c_void_p)), "b32_band_export")
        return buf.raw

    def band_import(self, share: bytes, rank):
        """b32_band_import (band rank, another process): map the root's framebuffer and draw into it; returns (width, height)."""
        assert len(share) == self.BAND_SHARE_BYTES
        buf = C.create_string_buffer(share, self.BAND_SHARE_BYTES)
        rc = self.lib.b32_band_import(self.h, C.cast(buf, C.c_void_p), int(rank))
        _chk(rc, f"b32_band_import (hip error {self.lib.b32_last_hip_error(self.h)})" if rc else "b32_band_import")
        w, h = np.frombuffer(share, np.uint32, 2, 64)
        return int(w), int(h)

    def band_attach(self, root: "Context", rank):
        _chk(self.lib.b32_band_attach(self.h, root.h, int(rank)), "b32_band_attach")

    def band_close(self):
        _chk(self.lib.b32_band_close(self.h), "b32_band_close")

    def band_publish(self, frame_no):
        _chk(self.lib.b32_band_publish(self.h, int(frame_no)), "b32_band_publish")

    def band_wait(self, rank, frame_no, timeout_us=2_000_000):
        _chk(self.lib.b32_band_wait(self.h, int(rank), int(frame_no), int(timeout_us)), "b32_band_wait")

    def band_wait_all(self, nranks, frame_no, timeout_us=2_000_000, release_after=True):
        _chk(self.lib.b32_band_wait_all(self.h, int(nranks), int(frame_no), int(timeout_us), 1 if release_after else 0), "b32_band_wait_all")

    def band_release(self, frame_no):
        _chk(self.lib.b32_band_release(self.h, int(frame_no)), "b32_band_release")

    def band_acquire(self, frame_no, timeout_us=2_000_000):
        _chk(self.lib.b32_band_acquire(self.h, int(frame_no), int(timeout_us)), "b32_band_acquire")

    def band_status(self):
        """b32_band_status: (published frame per rank [64], released frame of the root, waits that timed out)."""
        ep = (C.c_uint32 * 64)(); root = C.c_uint32(); to = C.c_uint32()
        _chk(self.lib.b32_band_status(self.h, ep, C.byref(root), C.byref(to)), "b32_band_status")
        return list(ep), int(root.value), int(to.value)

    # transport (2): RCCL behind the C ABI.  The communicator is made by the library itself (the librccl it loaded), so the host needs
    # no RCCL binding of its own.
    @staticmethod
    def rccl_unique_id() -> bytes:
        """b32_rccl_unique_id: ncclGetUniqueId on ONE rank; hand the 128 bytes to every other rank."""
        from . import abi
        buf = C.create_string_buffer(128)
        _chk(abi.load_library().b32_rccl_unique_id(C.cast(buf, C.c_void_p)), "b32_rccl_unique_id")
        return buf.raw

    def rccl_comm_create(self, unique_id: bytes, rank, nranks):
        """b32_rccl_comm_create: ncclCommInitRank on this context's device (collective); returns the opaque ncclComm_t."""
        assert len(unique_id) == 128
        buf = C.create_string_buffer(unique_id, 128)
        comm = C.c_void_p()
        rc = self.lib.b32_rccl_comm_create(self.h, C.cast(buf, C.c_void_p), int(rank), int(nranks), C.byref(comm))
        _chk(rc, f"b32_rccl_comm_create (ncclResult {self.lib.b32_last_hip_error(self.h)})" if rc else "b32_rccl_comm_create")
        return comm

    def rccl_comm_destroy(self, comm):
        _chk(self.lib.b32_rccl_comm_destroy(comm), "b32_rccl_comm_destroy")

    def gather_bands_rccl(self, comm, rank, nranks, root, bands, loopback_dst_y0=None):
        """b32_gather_bands_rccl: bands = [(y0, y1)] of every rank; enqueued on the context's stream behind the frame's kernels.
        loopback_dst_y0 (test tap): the root also sends its own band to itself, received at that row."""
        y0 = (C.c_uint32 * nranks)(*[b[0] for b in bands]); y1 = (C.c_uint32 * nranks)(*[b[1] for b in bands])
        if loopback_dst_y0 is None:
            rc = self.lib.b32_gather_bands_rccl(self.h, comm, int(rank), int(nranks), int(root), y0, y1)
        else:
            rc = self.lib.b32_gather_bands_rccl_loopback(self.h, comm, int(rank), int(nranks), int(root), y0, y1, int(loopback_dst_y0))
        _chk(rc, f"b32_gather_bands_rccl (ncclResult {self.lib.b32_last_hip_error(self.h)})" if rc == -4 else "b32_gather_bands_rccl")

    # ---- stage taps -----------------------------------------------------------------
    def project_fixed_batch(self, pos, camera: T.Camera, width, height):
        pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        n = len(pos)
        sx = np.zeros(n, np.int32); sy = np.zeros(n, np.int32); z = np.zeros(n, np.float32)
        cam = camera.pack()
        _chk(self.lib.b32_project_fixed_batch(self.h, pos.ctypes.data, n, C.byref(cam), width, height,
                                              sx.ctypes.data, sy.ctypes.data, z.ctypes.data), "project_fixed_batch")
        return sx, sy, z

    def device_constants(self):
        """({fixture key: value}, UNR table, 4x4 dither matrix [y & 3][x & 3]) read back from device code (b32_device_constants)."""
        cap = 256
        names = (C.c_char_p * cap)()
        bits = np.zeros(cap, np.uint32); isf = np.zeros(cap, np.uint8)
        n = C.c_uint32()
        unr = np.zeros(257, np.uint8); dither = np.zeros(16, np.int32)
        _chk(self.lib.b32_device_constants(self.h, names, bits.ctypes.data, isf.ctypes.data, cap, C.byref(n), unr.ctypes.data,
                                           dither.ctypes.data), "b32_device_constants")
        out = {}
        for i in range(min(n.value, cap)):
            out[names[i].decode()] = float(bits[i:i + 1].view(np.float32)[0]) if isf[i] else int(bits[i])
        return out, unr, dither.reshape(4, 4)

    def selftest_f32(self, op, a, b, c):
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
        c = np.ascontiguousarray(c, np.float32)
        out = np.zeros_like(a)
        _chk(self.lib.b32_selftest_f32(self.h, op, a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data, a.size))
        return out

    def last_draw_order(self, cap):
        buf = np.zeros(max(cap, 1), np.uint32)
        n = C.c_uint32()
        _chk(self.lib.b32_last_draw_order(self.h, buf.ctypes.data, cap, C.byref(n)), "last_draw_order")
        return buf[:min(n.value, cap)].copy()

    def last_surface_shading(self, cap):
        """b32_last_surface_shading: (face_idx [n], shades f32 [n or 0, 9], colors u32 [n, 3]) of the last finished frame's surviving
        surfaces, in ascending face index -- the shades of an unlit frame come back empty."""
        cap = max(int(cap), 1)
        faces = np.zeros(cap, np.uint32); shades = np.zeros((cap, 9), np.float32); colors = np.zeros((cap, 3), np.uint32)
        n = C.c_uint32(); ns = C.c_uint32()
        _chk(self.lib.b32_last_surface_shading(self.h, faces.ctypes.data, shades.ctypes.data, colors.ctypes.data, cap, C.byref(n), C.byref(ns)),
             "last_surface_shading")
        if n.value > cap:
            raise ValueError(f"last_surface_shading: {n.value} surfaces, room for {cap}")
        return faces[:n.value].copy(), shades[:ns.value].copy(), colors[:n.value].copy()


class Framebuffer:
    """Framebuffer (render.rs:10-45), device resident. `pixels` downloads the RGBA8 bytes."""

    def __init__(self, width, height, ctx: Context = None, device=0):
        self.ctx = ctx or Context(device)
        # Framebuffer::new (render.rs:18-25): zero pixels and an f32::MAX z-buffer even when the ctx already held a frame of this size
        _chk(self.ctx.lib.b32_fb_new(self.ctx.h, width, height), "fb_new")
        self.width, self.height = width, height
        self.set_band(0, height)          # a new Framebuffer owns all its rows (a band set earlier on this ctx does not carry over)

    @staticmethod
    def new(width, height, ctx=None):
        return Framebuffer(width, height, ctx)

    def resize(self, width, height):
        _chk(self.ctx.lib.b32_fb_resize(self.ctx.h, width, height), "fb_resize")
        self.width, self.height = width, height

    def bind_device(self, device_ptr, width, height):
        """Draw into caller-owned device memory (e.g. torch uint8 tensor .data_ptr())."""
        _chk(self.ctx.lib.b32_fb_bind_device(self.ctx.h, device_ptr, width, height), "fb_bind_device")
        self.width, self.height = width, height

    def set_band(self, y0, y1):
        _chk(self.ctx.lib.b32_set_band(self.ctx.h, y0, y1), "set_band")

    def clear(self, color: T.Color):
        _chk(self.ctx.lib.b32_fb_clear(self.ctx.h, color.r, color.g, color.b, color.blend), "fb_clear")

    def clear_gradient(self, top: T.Color, bottom: T.Color):
        """Framebuffer::clear_gradient (render.rs:58-77)"""
        _chk(self.ctx.lib.b32_fb_clear_gradient(self.ctx.h, top.r, top.g, top.b, top.blend, bottom.r, bottom.g, bottom.b, bottom.blend), "fb_clear_gradient")

    def clear_transparent(self):
        """Framebuffer::clear_transparent (render.rs:47-56)"""
        _chk(self.ctx.lib.b32_fb_clear_transparent(self.ctx.h), "fb_clear_transparent")

    def render_skybox_mesh(self, vertices, faces, camera: T.Camera):
        """Step 1 of Framebuffer::render_skybox (render.rs:81-134): `vertices` (abi.SKY_VERTEX_DTYPE) and `faces` ([n,3] u32) are
        what Skybox::generate_mesh returned on the host."""
        v = np.ascontiguousarray(vertices, dtype=abi.SKY_VERTEX_DTYPE)
        f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1, 3)
        cam = camera.pack()
        _chk(self.ctx.lib.b32_render_skybox_mesh(self.ctx.h, v.ctypes.data if len(v) else None, len(v),
                                                 f.ctypes.data if len(f) else None, len(f), C.byref(cam)), "render_skybox_mesh")

    def draw_star_diamonds(self, cx, cy, rgb, size):
        """draw_star_diamond (render.rs:199-240) for every star, in order."""
        cx = np.ascontiguousarray(cx, np.int32); cy = np.ascontiguousarray(cy, np.int32)
        rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
        _chk(self.ctx.lib.b32_draw_star_diamonds(self.ctx.h, cx.ctypes.data, cy.ctypes.data, rgb.ctypes.data, len(cx), float(size)), "draw_star_diamonds")

    # ---- the line family (render.rs:684-872): each call is a batch of one; draw_lines takes a whole abi.LINE_DTYPE array in order
    def draw_lines(self, lines):
        """b32_draw_lines: every line of `lines` (abi.LINE_DTYPE) as the reference calls in array order; enqueued, no host synchronisation."""
        arr = np.ascontiguousarray(lines, dtype=abi.LINE_DTYPE).reshape(-1)
        _chk(self.ctx.lib.b32_draw_lines(self.ctx.h, arr.ctypes.data if len(arr) else None, len(arr)), "draw_lines")

    @staticmethod
    def _line(kind, x0, y0, x1, y1, z0, z1, color: T.Color, alpha):
        l = np.zeros(1, abi.LINE_DTYPE)
        l["x0"], l["y0"], l["x1"], l["y1"], l["z0"], l["z1"] = x0, y0, x1, y1, z0, z1
        l["r"], l["g"], l["b"], l["blend"], l["kind"], l["alpha"] = color.r, color.g, color.b, color.blend, kind, alpha
        return l

    def draw_line(self, x0, y0, x1, y1, color: T.Color):
        """Framebuffer::draw_line (render.rs:715-755)"""
        self.draw_lines(self._line(abi.LINE_2D, x0, y0, x1, y1, 0.0, 0.0, color, 255))

    def draw_line_alpha(self, x0, y0, x1, y1, color: T.Color, alpha):
        """Framebuffer::draw_line_alpha (render.rs:684-711)"""
        self.draw_lines(self._line(abi.LINE_2D_ALPHA, x0, y0, x1, y1, 0.0, 0.0, color, alpha))

    def draw_line_3d(self, x0, y0, z0, x1, y1, z1, color: T.Color):
        """Framebuffer::draw_line_3d (render.rs:757-762): z < zbuffer"""
        self.draw_lines(self._line(abi.LINE_3D, x0, y0, x1, y1, z0, z1, color, 255))

    def draw_line_3d_overlay(self, x0, y0, z0, x1, y1, z1, color: T.Color):
        """Framebuffer::draw_line_3d_overlay (render.rs:764-766): z <= zbuffer"""
        self.draw_lines(self._line(abi.LINE_3D_OVERLAY, x0, y0, x1, y1, z0, z1, color, 255))

    def draw_line_3d_alpha(self, x0, y0, z0, x1, y1, z1, color: T.Color, alpha):
        """Framebuffer::draw_line_3d_alpha (render.rs:822-872): depths * 0.995, z <= zbuffer, set_pixel_alpha"""
        self.draw_lines(self._line(abi.LINE_3D_ALPHA, x0, y0, x1, y1, z0, z1, color, alpha))

    # ---- the other drawing methods (render.rs:631-971), in one ordered batch with the line family: b32_draw_prims
    def draw_prims(self, prims):
        """b32_draw_prims: every record of `prims` (abi.PRIM_DTYPE) as the reference calls in array order; enqueued, no host synchronisation."""
        arr = np.ascontiguousarray(prims, dtype=abi.PRIM_DTYPE).reshape(-1)
        _chk(self.ctx.lib.b32_draw_prims(self.ctx.h, arr.ctypes.data if len(arr) else None, len(arr)), "draw_prims")

    def prim_batch(self):
        """A PrimBatch on this framebuffer: the same drawing methods, recorded; flush() draws them all with one b32_draw_prims call."""
        return PrimBatch(self)

    def draw_line_blended(self, x0, y0, x1, y1, color: T.Color, mode):
        """Framebuffer::draw_line_blended (render.rs:720-755): Opaque -> set_pixel, else set_pixel_blended"""
        self.draw_prims(prim(abi.PRIM_LINE_BLENDED, x0, y0, x1, y1, color, mode=mode))

    def draw_circle(self, cx, cy, radius, color: T.Color):
        """Framebuffer::draw_circle (render.rs:631-642)"""
        self.draw_prims(prim(abi.PRIM_CIRCLE, cx, cy, 0, 0, color, size=radius))

    def draw_circle_alpha(self, cx, cy, radius, color: T.Color, alpha):
        """Framebuffer::draw_circle_alpha (render.rs:670-681)"""
        self.draw_prims(prim(abi.PRIM_CIRCLE_ALPHA, cx, cy, 0, 0, color, size=radius, alpha=alpha))

    def draw_thick_line(self, x0, y0, x1, y1, thickness, color: T.Color):
        """Framebuffer::draw_thick_line (render.rs:875-938)"""
        self.draw_prims(prim(abi.PRIM_THICK_LINE, x0, y0, x1, y1, color, size=thickness))

    def draw_rect(self, x0, y0, x1, y1, color: T.Color):
        """Framebuffer::draw_rect (render.rs:941-951)"""
        self.draw_prims(prim(abi.PRIM_RECT, x0, y0, x1, y1, color))

    def draw_filled_rect(self, x0, y0, x1, y1, color: T.Color):
        """Framebuffer::draw_filled_rect (render.rs:954-971)"""
        self.draw_prims(prim(abi.PRIM_FILLED_RECT, x0, y0, x1, y1, color))

    # ---- world-space overlays (rasterizer/draw.rs:12-135, math.rs:503-652): projected on the device, b32_draw_world
    def draw_world(self, items, camera: T.Camera, ortho=None):
        """b32_draw_world: every item of `items` (abi.WORLD_ITEM_DTYPE) projected on the device and drawn as the reference's calls in array
        order; enqueued, no host synchronisation.  ortho: None (perspective) or (zoom, center_x, center_y)."""
        arr = np.ascontiguousarray(items, dtype=abi.WORLD_ITEM_DTYPE).reshape(-1)
        cam = camera.pack()
        o = _pack_ortho(ortho)
        _chk(self.ctx.lib.b32_draw_world(self.ctx.h, C.byref(cam), C.byref(o) if o is not None else None,
                                         arr.ctypes.data if len(arr) else None, len(arr)), "draw_world")

    def world_batch(self):
        """A WorldBatch on this framebuffer: world-space calls recorded; flush(camera, ortho) draws them with one b32_draw_world call."""
        return WorldBatch(self)

    def draw_3d_line_clipped(self, camera: T.Camera, p0, p1, color: T.Color):
        """draw_3d_line_clipped (draw.rs:12-67)"""
        self.draw_world(world_item(abi.LINE_2D, p0, p1, color, flags=abi.WORLD_CLIP_NEAR), camera)

    def draw_floor_grid(self, camera: T.Camera, y, spacing, extent, grid_color: T.Color, x_axis_color: T.Color, z_axis_color: T.Color):
        """draw_floor_grid (draw.rs:81-135)"""
        cam = camera.pack()
        cols = [(C.c_uint8 * 4)(c.r, c.g, c.b, c.blend) for c in (grid_color, x_axis_color, z_axis_color)]
        _chk(self.ctx.lib.b32_draw_floor_grid(self.ctx.h, C.byref(cam), float(y), float(spacing), float(extent), *cols), "draw_floor_grid")

    def world_counts(self):
        """b32_world_counts: (drawn, dropped, rejected) items this context has projected so far; synchronises."""
        v = [C.c_uint64() for _ in range(3)]
        _chk(self.ctx.lib.b32_world_counts(self.ctx.h, *[C.byref(x) for x in v]), "world_counts")
        return tuple(int(x.value) for x in v)

    def world_project_batch(self, items, camera: T.Camera, ortho=None, width=None, height=None):
        """b32_world_project_batch (stage tap): the abi.PRIM_DTYPE records b32_draw_world hands to the tile pass."""
        arr = np.ascontiguousarray(items, dtype=abi.WORLD_ITEM_DTYPE).reshape(-1)
        out = np.zeros(len(arr), abi.PRIM_DTYPE)
        cam = camera.pack()
        o = _pack_ortho(ortho)
        _chk(self.ctx.lib.b32_world_project_batch(self.ctx.h, C.byref(cam), C.byref(o) if o is not None else None,
                                                  arr.ctypes.data if len(arr) else None, len(arr), width or self.width, height or self.height,
                                                  out.ctypes.data if len(arr) else None), "world_project_batch")
        return out

    # ---- the world editor's clipped lines and filled gizmos (editor/viewport_3d.rs:5687-6357): projected on the device, b32_draw_gizmos
    def draw_gizmos(self, items, camera: T.Camera, ortho=None):
        """b32_draw_gizmos: every item of `items` (abi.GIZMO_ITEM_DTYPE) drawn as the editor's helper calls in array order; enqueued, no
        host synchronisation.  ortho: None or (zoom, center_x, center_y), read by GIZMO_TRIANGLE_VIEW only."""
        arr = np.ascontiguousarray(items, dtype=abi.GIZMO_ITEM_DTYPE).reshape(-1)
        cam = camera.pack()
        o = _pack_ortho(ortho)
        _chk(self.ctx.lib.b32_draw_gizmos(self.ctx.h, C.byref(cam), C.byref(o) if o is not None else None,
                                          arr.ctypes.data if len(arr) else None, len(arr)), "draw_gizmos")

    def gizmo_batch(self):
        """A GizmoBatch on this framebuffer: the editor's helper calls recorded; flush(camera, ortho) draws them with one b32_draw_gizmos call."""
        return GizmoBatch(self)

    def gizmo_counts(self):
        """b32_gizmo_counts: (drawn, dropped, rejected) gizmo items this context has projected so far; synchronises."""
        v = [C.c_uint64() for _ in range(3)]
        _chk(self.ctx.lib.b32_gizmo_counts(self.ctx.h, *[C.byref(x) for x in v]), "gizmo_counts")
        return tuple(int(x.value) for x in v)

    # ---- the modeler's selection overlays from a slot's resident vertices (modeler/viewport.rs:1782-2247): b32_draw_mesh_overlay
    def _overlay_args(self, scene, topology, overlay, camera, ortho, selected):
        cam = camera.pack()
        o = _pack_ortho(ortho)
        ov, sel = overlay.pack(selected)
        top = topology.handle(self.ctx) if topology is not None else None
        return (self.ctx.h, C.byref(cam), C.byref(o) if o is not None else None, scene._slot, top, C.byref(ov), abi.ptr(sel) if len(sel) else None), (cam, o, ov, sel)

    def draw_mesh_overlay(self, scene, topology, overlay, camera: T.Camera, ortho=None, selected=None):
        """b32_draw_mesh_overlay: the sections of `overlay` (a MeshOverlay) made into records on the device from the vertices of `scene` (a
        detached ResidentScene, posed or not) and drawn in the reference's order; enqueued, no host synchronisation, nothing read back."""
        args, _keep = self._overlay_args(scene, topology, overlay, camera, ortho, selected)
        _chk(self.ctx.lib.b32_draw_mesh_overlay(*args), "draw_mesh_overlay")

    def mesh_overlay_project_batch(self, scene, topology, overlay, camera: T.Camera, ortho=None, selected=None, width=None, height=None):
        """b32_mesh_overlay_project_batch (stage tap): the abi.PRIM_DTYPE records b32_draw_mesh_overlay hands to the tile pass."""
        n = mesh_overlay_record_count(topology, scene.n_body_vertices, overlay, selected)
        out = np.zeros(n, abi.PRIM_DTYPE)
        got = C.c_uint32()
        args, _keep = self._overlay_args(scene, topology, overlay, camera, ortho, selected)
        _chk(self.ctx.lib.b32_mesh_overlay_project_batch(*args, width or self.width, height or self.height, abi.ptr(out) if n else None, n,
                                                         C.byref(got)), "mesh_overlay_project_batch")
        return out[:int(got.value)]

    # ---- the world editor's room overlays from a resident room (editor/viewport_3d.rs:4273-4658, :4862-5362): b32_draw_room_overlay
    def draw_room_overlay(self, room, overlay, camera: T.Camera):
        """b32_draw_room_overlay: the sections of `overlay` (a RoomOverlay) made into records on the device from the records of `room` (a
        Room) as they are there -- and, with hover_source = abi.ROOM_OVERLAY_HOVER_RESIDENT, from its last hover without waiting for it --
        and drawn in the reference's order; enqueued, no host synchronisation, nothing read back."""
        cam = camera.pack()
        o, lists = overlay.pack()
        _chk(self.ctx.lib.b32_draw_room_overlay(self.ctx.h, C.byref(cam), room._h, C.byref(o), *lists), "draw_room_overlay")

    def room_overlay_project_batch(self, room, overlay, camera: T.Camera, width=None, height=None):
        """b32_room_overlay_project_batch (stage tap): the abi.PRIM_DTYPE records b32_draw_room_overlay hands to the tile pass."""
        n = room_overlay_record_count(room.n, overlay)
        out = np.zeros(n, abi.PRIM_DTYPE)
        got = C.c_uint32()
        cam = camera.pack()
        o, lists = overlay.pack()
        _chk(self.ctx.lib.b32_room_overlay_project_batch(self.ctx.h, C.byref(cam), room._h, C.byref(o), *lists, width or self.width, height or self.height,
                                                         abi.ptr(out) if n else None, n, C.byref(got)), "room_overlay_project_batch")
        return out[:int(got.value)]

    # ---- the world editor's object overlays from resident asset parts (viewport_3d.rs:255-291, :7658-7697; asset.rs:288-312)
    def draw_object_overlays(self, parts, items, camera: T.Camera):
        """b32_draw_object_overlays: the wireframes and bounding boxes of `items` (ObjectItem) over the asset parts `parts` (ObjectPart with
        detached scenes) made into records on the device and drawn in array order; enqueued, no host synchronisation, nothing read back."""
        cam = camera.pack()
        pa, ia = pack_object_parts(parts, self.ctx), pack_object_items(items)
        _chk(self.ctx.lib.b32_draw_object_overlays(self.ctx.h, C.byref(cam), abi.ptr(pa) if len(pa) else None, len(pa),
                                                   abi.ptr(ia) if len(ia) else None, len(ia)), "draw_object_overlays")

    def object_overlay_project_batch(self, parts, items, camera: T.Camera, width=None, height=None):
        """b32_object_overlay_project_batch (stage tap): the abi.PRIM_DTYPE records b32_draw_object_overlays hands to the tile pass."""
        n = self.ctx.object_overlay_record_count(parts, items)
        out = np.zeros(n, abi.PRIM_DTYPE)
        got = C.c_uint32()
        cam = camera.pack()
        pa, ia = pack_object_parts(parts, self.ctx), pack_object_items(items)
        _chk(self.ctx.lib.b32_object_overlay_project_batch(self.ctx.h, C.byref(cam), abi.ptr(pa) if len(pa) else None, len(pa),
                                                           abi.ptr(ia) if len(ia) else None, len(ia), width or self.width, height or self.height,
                                                           abi.ptr(out) if n else None, n, C.byref(got)), "object_overlay_project_batch")
        return out[:int(got.value)]

    def present_nearest(self, dst_w, dst_h):
        """The presenter's nearest-neighbour upscale (game/renderer.rs:179-214) -> uint8 [dst_h, dst_w, 4]."""
        out = np.empty((dst_h, dst_w, 4), np.uint8)
        _chk(self.ctx.lib.b32_present_nearest(self.ctx.h, dst_w, dst_h, out.ctypes.data), "present_nearest")
        return out

    def upload(self, pixels):
        px = np.ascontiguousarray(pixels, dtype=np.uint8).reshape(-1)
        assert px.size == self.width * self.height * 4
        _chk(self.ctx.lib.b32_fb_upload(self.ctx.h, px.ctypes.data), "fb_upload")

    @property
    def pixels(self):
        out = np.empty(self.width * self.height * 4, np.uint8)
        _chk(self.ctx.lib.b32_fb_download(self.ctx.h, out.ctypes.data), "fb_download")
        return out

    @property
    def zbuffer(self):
        """Framebuffer::zbuffer (render.rs:12): f32 per pixel, f32::MAX where nothing was drawn in z-buffer mode."""
        out = np.empty(self.width * self.height, np.float32)
        _chk(self.ctx.lib.b32_zbuffer_download(self.ctx.h, out.ctypes.data), "zbuffer_download")
        return out

    def image(self):
        return self.pixels.reshape(self.height, self.width, 4)


def _geom(vertices, faces):
    v = np.ascontiguousarray(vertices, dtype=abi.VERTEX_DTYPE)
    f = np.ascontiguousarray(faces, dtype=abi.FACE_DTYPE)
    return v, f


def render_mesh_15(fb: Framebuffer, vertices, faces, textures, camera: T.Camera, settings: T.RasterSettings,
                   fog=None) -> T.RasterTimings:
    """render_mesh_15 (render.rs:2302-2310): host slices in, draws into the device framebuffer."""
    v, f = _geom(vertices, faces)
    tex_arr, _keep = T.pack_textures(textures)
    cam = camera.pack()
    st, _kl = settings.pack()
    fg = T.pack_fog(fog)
    tm = abi.B32Timings()
    rc = fb.ctx.lib.b32_render_mesh_15(fb.ctx.h, v.ctypes.data if len(v) else None, len(v),
                                       f.ctypes.data if len(f) else None, len(f),
                                       C.cast(tex_arr, C.c_void_p), len(textures), C.byref(cam), C.byref(st),
                                       C.byref(fg) if fg is not None else None, C.byref(tm))
    _chk(rc, "render_mesh_15")
    return T.RasterTimings.from_c(tm)


def render_mesh(fb: Framebuffer, vertices, faces, textures, camera: T.Camera, settings: T.RasterSettings) -> T.RasterTimings:
    """render_mesh (render.rs:1971-1978), the 8-bit-colour path every caller takes when `settings.use_rgb555` is false
    (scene.rs:163-169).  `textures` are rtypes.Texture (Color texels with per-texel blend modes)."""
    v, f = _geom(vertices, faces)
    tex_arr, _keep = T.pack_textures8(textures)
    cam = camera.pack()
    st, _kl = settings.pack()
    tm = abi.B32Timings()
    rc = fb.ctx.lib.b32_render_mesh(fb.ctx.h, v.ctypes.data if len(v) else None, len(v),
                                    f.ctypes.data if len(f) else None, len(f),
                                    C.cast(tex_arr, C.c_void_p), len(textures), C.byref(cam), C.byref(st), C.byref(tm))
    _chk(rc, "render_mesh")
    return T.RasterTimings.from_c(tm)


# aliases named in BASELINE.json's north_star (the reference's real entry point is render_mesh_15)
draw_mesh = render_mesh_15


def prim(kind, x0, y0, x1, y1, color: T.Color, z0=0.0, z1=0.0, size=0, alpha=255, mode=0):
    """One abi.PRIM_DTYPE record."""
    p = np.zeros(1, abi.PRIM_DTYPE)
    p["x0"], p["y0"], p["x1"], p["y1"], p["z0"], p["z1"], p["size"] = x0, y0, x1, y1, z0, z1, size
    p["r"], p["g"], p["b"], p["blend"], p["kind"], p["alpha"], p["mode"] = color.r, color.g, color.b, color.blend, kind, alpha, mode
    return p


def _pack_ortho(ortho):
    if ortho is None:
        return None
    zoom, cx, cy = ortho
    return abi.B32Ortho(float(zoom), float(cx), float(cy))


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


class WorldBatch:
    """World-space overlay calls recorded in call order (the modeler's frame: hierarchy lines, depth-tested edges, a dot per vertex);
    flush(camera, ortho) projects and draws them with ONE b32_draw_world call.  Positions are (x, y, z) in world space."""

    def __init__(self, fb: "Framebuffer"):
        self.fb = fb
        self._items = []                                          # one tuple per call; the array is built once, in items()

    def __len__(self):
        return len(self._items)

    def _add(self, kind, p0, p1, color: T.Color, size=0, alpha=255, mode=0, flags=0):
        self._items.append((tuple(p0), tuple(p1), size, color.r, color.g, color.b, color.blend, kind, alpha, mode, flags, (0, 0, 0, 0)))

    def line_clipped(self, p0, p1, color: T.Color):
        """draw_3d_line_clipped (draw.rs:12-67)"""
        self._add(abi.LINE_2D, p0, p1, color, flags=abi.WORLD_CLIP_NEAR)

    def line_clipped_3d(self, p0, p1, color: T.Color):
        """the same clip with depth (editor/viewport_3d.rs:5783-5840): world_to_screen_with_depth, draw_line_3d"""
        self._add(abi.LINE_3D, p0, p1, color, flags=abi.WORLD_CLIP_NEAR)

    def line(self, p0, p1, color: T.Color):
        """world_to_screen_with_ortho on each end, draw_line"""
        self._add(abi.LINE_2D, p0, p1, color)

    def line_alpha(self, p0, p1, color: T.Color, alpha):
        self._add(abi.LINE_2D_ALPHA, p0, p1, color, alpha=alpha)

    def line_3d(self, p0, p1, color: T.Color):
        """world_to_screen_with_ortho_depth on each end, draw_line_3d"""
        self._add(abi.LINE_3D, p0, p1, color)

    def line_3d_overlay(self, p0, p1, color: T.Color):
        self._add(abi.LINE_3D_OVERLAY, p0, p1, color)

    def line_3d_alpha(self, p0, p1, color: T.Color, alpha):
        """... draw_line_3d_alpha (modeler/viewport.rs:1927-1951)"""
        self._add(abi.LINE_3D_ALPHA, p0, p1, color, alpha=alpha)

    def line_blended(self, p0, p1, color: T.Color, mode):
        self._add(abi.PRIM_LINE_BLENDED, p0, p1, color, mode=mode)

    def thick_line(self, p0, p1, thickness, color: T.Color):
        self._add(abi.PRIM_THICK_LINE, p0, p1, color, size=thickness)

    def circle(self, p, radius, color: T.Color):
        """world_to_screen_with_ortho, draw_circle"""
        self._add(abi.PRIM_CIRCLE, p, (0.0, 0.0, 0.0), color, size=radius)

    def circle_alpha(self, p, radius, color: T.Color, alpha):
        """world_to_screen_with_ortho, draw_circle_alpha (modeler/viewport.rs:1876-1880)"""
        self._add(abi.PRIM_CIRCLE_ALPHA, p, (0.0, 0.0, 0.0), color, size=radius, alpha=alpha)

    def items(self):
        """The recorded batch (abi.WORLD_ITEM_DTYPE, call order)."""
        return np.array(self._items, abi.WORLD_ITEM_DTYPE)

    def flush(self, camera: T.Camera, ortho=None):
        """Draws everything recorded (one b32_draw_world call) and starts an empty batch."""
        items, self._items = self.items(), []
        self.fb.draw_world(items, camera, ortho)


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


class GizmoBatch:
    """The world editor's overlay helpers (editor/viewport_3d.rs:5687-6357) recorded in call order; flush(camera, ortho) projects and
    draws them with ONE b32_draw_gizmos call.  Positions are (x, y, z) in world space."""

    def __init__(self, fb: "Framebuffer" = None):
        self.fb = fb
        self._items = []

    def __len__(self):
        return len(self._items)

    def _add(self, kind, p0, p1, p2, color: T.Color, size=0):
        self._items.append((tuple(p0), tuple(p1), tuple(p2), size, color.r, color.g, color.b, color.blend, kind, (0, 0, 0)))

    def line(self, p0, p1, color: T.Color):
        """draw_3d_line (viewport_3d.rs:5687-5695): near clip, world_to_screen, the Cohen-Sutherland clip to the frame, Bresenham"""
        self._add(abi.GIZMO_LINE, p0, p1, _ZERO3, color)

    def line_depth(self, p0, p1, color: T.Color):
        """draw_3d_line_depth (:5698-5706)"""
        self._add(abi.GIZMO_LINE_DEPTH, p0, p1, _ZERO3, color)

    def thick_line_depth(self, p0, p1, color: T.Color, thickness):
        """draw_3d_thick_line_depth (:5709-5781)"""
        self._add(abi.GIZMO_THICK_LINE_DEPTH, p0, p1, _ZERO3, color, size=thickness)

    def point(self, p, radius, color: T.Color):
        """draw_3d_point (:5958-5976)"""
        self._add(abi.GIZMO_POINT, p, _ZERO3, _ZERO3, color, size=radius)

    def triangle(self, p0, p1, p2, color: T.Color):
        """the editor's project_vertex three times, then draw_filled_triangle_3d (:6239-6245, :6295-6357)"""
        self._add(abi.GIZMO_TRIANGLE, p0, p1, p2, color)

    def triangle_view(self, p0, p1, p2, color: T.Color):
        """the modeler's project_vertex three times (modeler/viewport.rs:4592-4607: takes the flush's ortho), then its fill"""
        self._add(abi.GIZMO_TRIANGLE_VIEW, p0, p1, p2, color)

    def octahedron(self, center, size, color: T.Color):
        """draw_filled_octahedron (viewport_3d.rs:6223-6292): eight faces, twelve edges"""
        for it in octahedron_items(center, size, color):
            self._items.append(tuple(tuple(v) if isinstance(v, np.ndarray) else v for v in it.tolist()))

    def items(self):
        """The recorded batch (abi.GIZMO_ITEM_DTYPE, call order)."""
        return np.array(self._items, abi.GIZMO_ITEM_DTYPE)

    def flush(self, camera: T.Camera, ortho=None):
        """Draws everything recorded (one b32_draw_gizmos call) and starts an empty batch."""
        items, self._items = self.items(), []
        self.fb.draw_gizmos(items, camera, ortho)


_ZERO3 = (0.0, 0.0, 0.0)


# ---- the modeler's selection overlays (modeler/viewport.rs:1782-2247) from vertex positions: b32_draw_mesh_overlay and its mirror
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


OVERLAY_COLORS = {"brackets": (0, 200, 230), "edges": (80, 80, 80), "dots": (40, 40, 50), "hover": (255, 200, 150), "selected": (100, 180, 255),
                  "preview": (255, 220, 100)}


def _poly_slots(mode, cnt):
    """Records of a polygon of cnt positions: hovered (0), selected (1), previewed (2)."""
    cnt = np.asarray(cnt, np.int64)
    return cnt + (cnt >= 4) if mode == 0 else (2 * cnt + 1 if mode == 1 else cnt + 1)


def mesh_overlay_layout(topology, nv, overlay, selected=None):
    """First record of every part, and the total: {"brackets", "edges", "dots", "hover_vertex", "hover_edge", "hover_face", "selected",
    "preview", "total"} -- a function of the topology, nv, the struct and the list alone (overlay_layout, b32_overlay_body.h)."""
    o = overlay
    sel, n_sel = o.selected_list(selected)
    if (o.sections & ~abi.OVERLAY_ALL) or o.select_kind > 3 or o.preview_mode > 2:
        raise ValueError("MeshOverlay: unknown section bit, select_kind or preview_mode")
    polygons = (o.sections & abi.OVERLAY_EDGES) or ((o.sections & abi.OVERLAY_HOVER) and o.hover_face != abi.OVERLAY_NONE) or \
        ((o.sections & abi.OVERLAY_SELECTED) and o.select_kind == abi.SELECT_POLYGONS and n_sel) or ((o.sections & abi.OVERLAY_PREVIEW) and o.preview_mode != 0)
    if polygons and topology is None:
        raise ValueError("MeshOverlay: a section that walks polygons needs a topology")
    t = topology
    np_, nh, ne = (t.np, len(t.poly_verts), t.ne) if t is not None else (0, 0, 0)
    lay, at = {}, 0
    lay["brackets"] = at
    at += 24 if (o.sections & abi.OVERLAY_BRACKETS) and nv else 0
    lay["edges"] = at
    at += nh if o.sections & abi.OVERLAY_EDGES else 0
    lay["dots"] = at
    at += nv if o.sections & abi.OVERLAY_DOTS else 0
    lay["hover_vertex"] = lay["hover_edge"] = lay["hover_face"] = at
    if o.sections & abi.OVERLAY_HOVER:
        at += 1 if o.hover_vertex != abi.OVERLAY_NONE else 0
        lay["hover_edge"] = at
        at += 3 if o.hover_edge != (abi.OVERLAY_NONE, abi.OVERLAY_NONE) else 0
        lay["hover_face"] = at
        if o.hover_face != abi.OVERLAY_NONE and o.hover_face < np_:
            at += int(_poly_slots(0, t.count[o.hover_face]))
    lay["selected"] = at
    if o.sections & abi.OVERLAY_SELECTED:
        if o.select_kind == abi.SELECT_VERTICES:
            at += n_sel
        elif o.select_kind == abi.SELECT_EDGES:
            at += 4 * n_sel
        elif o.select_kind == abi.SELECT_POLYGONS and n_sel:
            at += int(_poly_slots(1, t.count[sel[sel < np_].astype(np.int64)]).sum())
    lay["preview"] = at
    if o.sections & abi.OVERLAY_PREVIEW:
        at += nv if o.preview_mode == 0 else (2 * ne if o.preview_mode == 1 else nh + np_)
    lay["total"] = at
    return lay


def mesh_overlay_record_count(topology, nv, overlay, selected=None):
    """How many records b32_draw_mesh_overlay makes (b32_mesh_overlay_record_count): known before anything is projected."""
    return mesh_overlay_layout(topology, nv, overlay, selected)["total"]


def _ov_i32(f):
    """Rust's `as i32` on an f32 array: NaN -> 0, saturating, truncation toward zero."""
    f = np.asarray(f, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isnan(f), 0.0, np.clip(np.trunc(f), -2147483648.0, 2147483647.0))
    return r.astype(np.int64).astype(np.int32)


def _ov_inc(v):
    """`as i32 + 1` of a release build: wraps."""
    return (v.astype(np.int64) + 1).astype(np.uint32).view(np.int32) if isinstance(v, np.ndarray) else _ov_inc(np.asarray([v], np.int32))[0]


def _ov_depth(z):
    z = np.asarray(z, np.float32).copy()
    z[np.isnan(z)] = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    return z


def _ov_lines(out, idx, ok, kind, x0, y0, x1, y1, z0, z1, rgb, alpha=255):
    """Line records at out[idx[ok]]; an extent that reaches 2^30 leaves the no-op."""
    lim = 1 << 30
    ok = ok & (np.abs(x1.astype(np.int64) - x0) < lim) & (np.abs(y1.astype(np.int64) - y0) < lim)
    i = idx[ok]
    for name, v in (("x0", x0), ("y0", y0), ("x1", x1), ("y1", y1)):
        out[name][i] = v[ok]
    depth = abi.LINE_3D <= kind <= abi.LINE_3D_ALPHA
    out["z0"][i] = _ov_depth(z0[ok]) if depth else 0.0
    out["z1"][i] = _ov_depth(z1[ok]) if depth else 0.0
    out["size"][i] = 0
    out["r"][i], out["g"][i], out["b"][i] = rgb
    out["kind"][i], out["alpha"][i] = kind, alpha


def _ov_circles(out, idx, ok, kind, sx, sy, radius, rgb, alpha=255):
    """Circle records at out[idx[ok]]; a centre that reaches 2^30 leaves the no-op."""
    lim = 1 << 30
    x, y = _ov_i32(sx), _ov_i32(sy)
    ok = ok & (np.abs(x.astype(np.int64)) < lim) & (np.abs(y.astype(np.int64)) < lim)
    i = idx[ok]
    out["x0"][i], out["y0"][i], out["size"][i] = x[ok], y[ok], radius
    out["r"][i], out["g"][i], out["b"][i] = rgb
    out["kind"][i], out["alpha"][i] = kind, alpha


def _ov_segs(out, idx, ok, sx0, sy0, sx1, sy1, rgb, ox=False, oy=False):
    x0, y0, x1, y1 = _ov_i32(sx0), _ov_i32(sy0), _ov_i32(sx1), _ov_i32(sy1)
    if ox:
        x0, x1 = _ov_inc(x0), _ov_inc(x1)
    if oy:
        y0, y1 = _ov_inc(y0), _ov_inc(y1)
    zero = np.zeros(len(x0), np.float32)
    _ov_lines(out, idx, ok, abi.LINE_2D, x0, y0, x1, y1, zero, zero, rgb)


def _ov_inside(x, y, rect):
    x0, y0, x1, y1 = (np.float32(v) for v in rect)
    with np.errstate(invalid="ignore"):
        return (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)


def _ov_polygons(out, mode, polys, first, top, pos, nv, tab, project, rect, rgb):
    """The polygons `polys` (all < np) into their records at out[first[i] ...], all polygons at once, one position of the loop at a time:
    the streamed outline of overlay_polygon (b32_overlay_body.h) -- hovered (mode 0), selected (1), previewed (2)."""
    f32 = np.float32
    sx, sy, some = tab
    polys = np.asarray(polys, np.int64)
    first = np.asarray(first, np.int64)
    m = len(polys)
    if not m:
        return
    start, cnt = top.poly_start.astype(np.int64)[polys], top.count[polys]
    pv = top.poly_verts.astype(np.int64)
    acc = np.zeros((m, 3), f32)
    count = np.zeros(m, np.int64)
    go = np.ones(m, bool)
    csx = csy = np.zeros(m, f32)
    maxc = int(cnt.max()) if m else 0
    if mode != 0:
        for j in range(maxc):
            act = j < cnt
            vi = np.where(act, pv[np.minimum(start + j, len(pv) - 1)] if len(pv) else 0, nv)
            ok = act & (vi < nv)
            p = pos[np.where(ok, vi, 0)] if nv else np.zeros((m, 3), f32)
            acc[ok] = acc[ok] + p[ok]
            count += ok
    if mode == 2:
        with np.errstate(all="ignore"):
            inv = f32(1.0) / count.astype(f32)
            c = acc * inv[:, None]
            csx, csy, _cz, csome = project(c[:, 0], c[:, 1], c[:, 2])
        go = (count != 0) & csome & _ov_inside(csx, csy, rect)
    n = np.zeros(m, np.int64)
    k = np.zeros(m, np.int64)
    pts = {name: [np.zeros(m, f32), np.zeros(m, f32)] for name in ("first", "third", "prev")}
    for j in range(maxc):
        act = go & (j < cnt)
        vi = np.where(act, pv[np.minimum(start + j, len(pv) - 1)] if len(pv) else 0, nv)
        ok = act & (vi < nv)
        vc = np.where(ok, vi, 0)
        ok = ok & (some[vc] if nv else False)
        ex, ey = (sx[vc], sy[vc]) if nv else (np.zeros(m, f32), np.zeros(m, f32))
        isfirst = ok & (n == 0)
        emit = ok & (n > 0)
        _ov_segs(out, first + k, emit, pts["prev"][0], pts["prev"][1], ex, ey, rgb)
        k += emit
        if mode == 1:
            _ov_segs(out, first + k, emit, pts["prev"][0], pts["prev"][1], ex, ey, rgb, ox=True)
            k += emit
        for name, sel in (("first", isfirst), ("third", ok & (n == 2)), ("prev", ok)):
            pts[name][0] = np.where(sel, ex, pts[name][0])
            pts[name][1] = np.where(sel, ey, pts[name][1])
        n += ok
    done = n >= 3
    # fewer than three projected vertices: what the walk wrote is taken back
    back = ~done
    for d in range(2):
        i = (first + d)[back & (k > d)]
        out[i] = noop_prims(len(i))
    _ov_segs(out, first + k, done, pts["prev"][0], pts["prev"][1], pts["first"][0], pts["first"][1], rgb)
    k += done
    if mode == 1:
        _ov_segs(out, first + k, done, pts["prev"][0], pts["prev"][1], pts["first"][0], pts["first"][1], rgb, ox=True)
        k += done
        with np.errstate(all="ignore"):
            inv = f32(1.0) / n.astype(f32)                                              # n = screen_positions.len() (:2088)
            c = acc * inv[:, None]
            csx, csy, _cz, csome = project(c[:, 0], c[:, 1], c[:, 2])
        _ov_circles(out, first + k, done & csome, abi.PRIM_CIRCLE, csx, csy, 4, rgb)
    elif mode == 2:
        _ov_circles(out, first + k, done, abi.PRIM_CIRCLE, csx, csy, 4, rgb)
    else:
        _ov_segs(out, first + k, n >= 4, pts["first"][0], pts["first"][1], pts["third"][0], pts["third"][1], rgb)


def noop_prims(n):
    """n records that draw nothing (a circle of radius -1): what a call the reference does not make leaves in its place."""
    r = np.zeros(n, abi.PRIM_DTYPE)
    r["kind"], r["size"] = abi.PRIM_CIRCLE, -1
    return r


def mesh_overlay_records(vertices, topology, overlay, selected, camera, w, h, ortho=None):
    """The numpy / float32 mirror of b32_draw_mesh_overlay: the abi.PRIM_DTYPE records, place for place, that the device makes from
    `vertices` (abi.VERTEX_DTYPE or (n, 3) positions, posed or not) -- draw_selected_object_brackets, draw_mesh_selection_overlays and
    draw_box_selection_preview (modeler/viewport.rs:1782-2247) for the sections of `overlay`."""
    f32 = np.float32
    o, t = overlay, topology
    pos = _positions(vertices)
    nv = len(pos)
    sel, n_sel = o.selected_list(selected)
    lay = mesh_overlay_layout(t, nv, o, selected)
    out = noop_prims(lay["total"])
    col = OVERLAY_COLORS

    def project(x, y, z):
        with np.errstate(all="ignore"):
            return _project_f32(np.asarray(x, f32), np.asarray(y, f32), np.asarray(z, f32), camera, w, h, ortho)

    sx, sy, cz, some = project(pos[:, 0], pos[:, 1], pos[:, 2])
    tab = (sx, sy, some)
    allv = np.arange(nv, dtype=np.int64)

    def ends(v0, v1):
        """Both indices < nv and both ends projected; the indices clipped for the gathers."""
        v0, v1 = np.asarray(v0, np.int64), np.asarray(v1, np.int64)
        ok = (v0 < nv) & (v1 < nv)
        a, b = np.where(ok, v0, 0), np.where(ok, v1, 0)
        if nv:
            ok = ok & some[a] & some[b]
        return ok, a, b

    if (o.sections & abi.OVERLAY_BRACKETS) and nv:
        with np.errstate(all="ignore"):
            mn, mx = np.empty(3, f32), np.empty(3, f32)
            for c in range(3):
                v = pos[:, c][~np.isnan(pos[:, c])]
                lo = min(np.finfo(f32).max, v.min()) if len(v) else np.finfo(f32).max
                hi = max(np.finfo(f32).min, v.max()) if len(v) else np.finfo(f32).min
                mn[c] = (f32(lo) + f32(0.0)) - f32(4.0)                                 # (the sign of a zero disappears in the margin)
                mx[c] = (f32(hi) + f32(0.0)) + f32(4.0)
            size = mx - mn
            blen = f32(min(min(size[0], size[1]), size[2]) if not np.isnan(size).any() else np.nanmin(size)) * f32(0.25)
            ci, di = np.arange(24) // 3, np.arange(24) % 3
            hi_ = np.stack([np.isin(ci, (1, 2, 5, 6)), ci >= 4, np.isin(ci, (2, 3, 6, 7))], 1)
            corner = np.where(hi_, mx[None, :], mn[None, :]).astype(f32)
            dirs = np.where(np.arange(3)[None, :] == di[:, None], np.where(hi_, f32(-1.0), f32(1.0)), f32(0.0)).astype(f32)
            end = corner + dirs * blen
            ax, ay, az, asome = project(corner[:, 0], corner[:, 1], corner[:, 2])
            bx, by, bz, bsome = project(end[:, 0], end[:, 1], end[:, 2])
        _ov_lines(out, lay["brackets"] + np.arange(24), asome & bsome, abi.LINE_3D, _ov_i32(ax), _ov_i32(ay), _ov_i32(bx), _ov_i32(by), az, bz, col["brackets"])

    if o.sections & abi.OVERLAY_EDGES:
        ok, a, b = ends(t.he_v0, t.he_v1)
        if nv:
            _ov_lines(out, lay["edges"] + np.arange(len(a)), ok, abi.LINE_3D_ALPHA, _ov_i32(sx[a]), _ov_i32(sy[a]), _ov_i32(sx[b]), _ov_i32(sy[b]),
                      cz[a], cz[b], col["edges"], 191)
    if o.sections & abi.OVERLAY_DOTS:
        _ov_circles(out, lay["dots"] + allv, some, abi.PRIM_CIRCLE_ALPHA, sx, sy, 3, col["dots"], 140)

    if o.sections & abi.OVERLAY_HOVER:
        if o.hover_vertex != abi.OVERLAY_NONE and o.hover_vertex < nv:
            v = np.array([o.hover_vertex])
            _ov_circles(out, np.array([lay["hover_vertex"]]), some[v], abi.PRIM_CIRCLE, sx[v], sy[v], 5, col["hover"])
        if o.hover_edge != (abi.OVERLAY_NONE, abi.OVERLAY_NONE) and nv:
            ok, a, b = ends([o.hover_edge[0]], [o.hover_edge[1]])
            for d, (ox, oy) in enumerate(((False, False), (True, False), (False, True))):
                _ov_segs(out, np.array([lay["hover_edge"] + d]), ok, sx[a], sy[a], sx[b], sy[b], col["hover"], ox=ox, oy=oy)
        if o.hover_face != abi.OVERLAY_NONE and t is not None and o.hover_face < t.np:
            _ov_polygons(out, 0, [o.hover_face], [lay["hover_face"]], t, pos, nv, tab, project, o.rect, col["hover"])

    if (o.sections & abi.OVERLAY_SELECTED) and n_sel:
        at = lay["selected"]
        if o.select_kind == abi.SELECT_VERTICES:
            v = sel.astype(np.int64)
            ok = v < nv
            vc = np.where(ok, v, 0)
            if nv:
                _ov_circles(out, at + np.arange(n_sel), ok & some[vc], abi.PRIM_CIRCLE, sx[vc], sy[vc], 4, col["selected"])
        elif o.select_kind == abi.SELECT_EDGES and nv:
            pairs = sel[:2 * n_sel].reshape(-1, 2)
            ok, a, b = ends(pairs[:, 0], pairs[:, 1])
            idx = at + 4 * np.arange(n_sel)
            _ov_segs(out, idx, ok, sx[a], sy[a], sx[b], sy[b], col["selected"])
            _ov_segs(out, idx + 1, ok, sx[a], sy[a], sx[b], sy[b], col["selected"], ox=True)
            _ov_circles(out, idx + 2, ok, abi.PRIM_CIRCLE, sx[a], sy[a], 3, col["selected"])
            _ov_circles(out, idx + 3, ok, abi.PRIM_CIRCLE, sx[b], sy[b], 3, col["selected"])
        elif o.select_kind == abi.SELECT_POLYGONS:
            polys = sel[sel < t.np].astype(np.int64)
            slots = _poly_slots(1, t.count[polys])
            first = at + np.concatenate([[0], np.cumsum(slots)])[:-1]
            _ov_polygons(out, 1, polys, first, t, pos, nv, tab, project, o.rect, col["selected"])

    if o.sections & abi.OVERLAY_PREVIEW:
        at = lay["preview"]
        if o.preview_mode == abi.PREVIEW_VERTEX:
            _ov_circles(out, at + allv, some & _ov_inside(sx, sy, o.rect), abi.PRIM_CIRCLE, sx, sy, 6, col["preview"])
        elif o.preview_mode == abi.PREVIEW_EDGE and nv:
            rank = t.first_half_edges()
            h = np.nonzero(rank)[0]
            ok, a, b = ends(t.he_v0[h], t.he_v1[h])
            with np.errstate(all="ignore"):
                mid_x, mid_y = (sx[a] + sx[b]) / f32(2.0), (sy[a] + sy[b]) / f32(2.0)
            ok = ok & _ov_inside(mid_x, mid_y, o.rect)
            idx = at + 2 * (rank[h] - 1)
            _ov_segs(out, idx, ok, sx[a], sy[a], sx[b], sy[b], col["preview"])
            _ov_segs(out, idx + 1, ok, sx[a], sy[a], sx[b], sy[b], col["preview"], ox=True)
        elif o.preview_mode == abi.PREVIEW_FACE:
            polys = np.arange(t.np, dtype=np.int64)
            _ov_polygons(out, 2, polys, at + t.poly_start.astype(np.int64)[:-1] + polys, t, pos, nv, tab, project, o.rect, col["preview"])
    return out


class PrimBatch:
    """Framebuffer's drawing methods, recorded in call order; flush() draws them with ONE b32_draw_prims call (callers that draw a dot per
    vertex pay one launch per frame, not one per circle).  set_pixel / set_pixel_alpha / set_pixel_blended map to a 1x1 FILLED_RECT, a
    one-point LINE_2D_ALPHA and a one-point LINE_BLENDED."""

    def __init__(self, fb: "Framebuffer"):
        self.fb = fb
        self._recs = []

    def __len__(self):
        return len(self._recs)

    def _add(self, *args, **kw):
        self._recs.append(prim(*args, **kw))

    def draw_line(self, x0, y0, x1, y1, color: T.Color):
        self._add(abi.LINE_2D, x0, y0, x1, y1, color)

    def draw_line_alpha(self, x0, y0, x1, y1, color: T.Color, alpha):
        self._add(abi.LINE_2D_ALPHA, x0, y0, x1, y1, color, alpha=alpha)

    def draw_line_3d(self, x0, y0, z0, x1, y1, z1, color: T.Color):
        self._add(abi.LINE_3D, x0, y0, x1, y1, color, z0=z0, z1=z1)

    def draw_line_3d_overlay(self, x0, y0, z0, x1, y1, z1, color: T.Color):
        self._add(abi.LINE_3D_OVERLAY, x0, y0, x1, y1, color, z0=z0, z1=z1)

    def draw_line_3d_alpha(self, x0, y0, z0, x1, y1, z1, color: T.Color, alpha):
        self._add(abi.LINE_3D_ALPHA, x0, y0, x1, y1, color, z0=z0, z1=z1, alpha=alpha)

    def draw_line_blended(self, x0, y0, x1, y1, color: T.Color, mode):
        self._add(abi.PRIM_LINE_BLENDED, x0, y0, x1, y1, color, mode=mode)

    def draw_circle(self, cx, cy, radius, color: T.Color):
        self._add(abi.PRIM_CIRCLE, cx, cy, 0, 0, color, size=radius)

    def draw_circle_alpha(self, cx, cy, radius, color: T.Color, alpha):
        self._add(abi.PRIM_CIRCLE_ALPHA, cx, cy, 0, 0, color, size=radius, alpha=alpha)

    def draw_thick_line(self, x0, y0, x1, y1, thickness, color: T.Color):
        self._add(abi.PRIM_THICK_LINE, x0, y0, x1, y1, color, size=thickness)

    def draw_rect(self, x0, y0, x1, y1, color: T.Color):
        self._add(abi.PRIM_RECT, x0, y0, x1, y1, color)

    def draw_filled_rect(self, x0, y0, x1, y1, color: T.Color):
        self._add(abi.PRIM_FILLED_RECT, x0, y0, x1, y1, color)

    def set_pixel(self, x, y, color: T.Color):
        self._add(abi.PRIM_FILLED_RECT, x, y, x, y, color)

    def set_pixel_alpha(self, x, y, color: T.Color, alpha):
        self._add(abi.LINE_2D_ALPHA, x, y, x, y, color, alpha=alpha)

    def set_pixel_blended(self, x, y, color: T.Color, mode):
        self._add(abi.PRIM_LINE_BLENDED, x, y, x, y, color, mode=mode)

    def records(self):
        """The recorded batch (abi.PRIM_DTYPE, call order)."""
        return np.concatenate(self._recs) if self._recs else np.zeros(0, abi.PRIM_DTYPE)

    def flush(self):
        """Draws everything recorded (one b32_draw_prims call) and starts an empty batch."""
        recs, self._recs = self.records(), []
        self.fb.draw_prims(recs)


class ResidentScene:
    """A mesh + textures kept in HBM across frames: upload once, draw many times."""

    def __init__(self, fb: Framebuffer, vertices, faces, textures=None, indexed_textures=None, textures8=None):
        self.fb = fb
        self.ctx = fb.ctx
        v, f = _geom(vertices, faces)
        self.fmt8 = textures8 is not None
        if textures8 is not None:                       # the 8-bit-colour path (render_mesh)
            arr, keep = T.pack_textures8(textures8)
            rc = self.ctx.lib.b32_scene_upload_rgba(self.ctx.h, v.ctypes.data if len(v) else None, len(v),
                                                    f.ctypes.data if len(f) else None, len(f),
                                                    C.cast(arr, C.c_void_p), len(textures8))
        elif indexed_textures is not None:
            arr, keep = T.pack_indexed_textures(indexed_textures)
            rc = self.ctx.lib.b32_scene_upload_indexed(self.ctx.h, v.ctypes.data if len(v) else None, len(v),
                                                       f.ctypes.data if len(f) else None, len(f),
                                                       C.cast(arr, C.c_void_p), len(indexed_textures))
        else:
            textures = textures or []
            arr, keep = T.pack_textures(textures)
            rc = self.ctx.lib.b32_scene_upload(self.ctx.h, v.ctypes.data if len(v) else None, len(v),
                                               f.ctypes.data if len(f) else None, len(f),
                                               C.cast(arr, C.c_void_p), len(textures))
        _chk(rc, "scene_upload")
        self.n_faces = len(f)
        self.n_vertices = len(v)
        self._packed = None
        self._slot = None

    # n_vertices / n_faces are what the slot holds and draws; assigning them (an upload, Room.build_mesh) names a new body and drops
    # the tail of bone octahedra, as the library does
    @property
    def n_vertices(self):
        return self.n_body_vertices + self._tail_v

    @n_vertices.setter
    def n_vertices(self, n):
        self.n_body_vertices, self._tail_v = int(n), 0

    @property
    def n_faces(self):
        return self.n_body_faces + self._tail_f

    @n_faces.setter
    def n_faces(self, n):
        self.n_body_faces, self._tail_f = int(n), 0

    def detach(self):
        """Move this scene into its own slot (b32_scene_swap) so that other scenes can be uploaded and drawn through the same context:
        every later render*/render_async swaps it in, enqueues, and swaps it out again -- no upload, no host sync."""
        if self._slot is None:
            h = C.c_void_p()
            _chk(self.ctx.lib.b32_scene_create(self.ctx.h, C.byref(h)), "scene_create")
            self._slot = h
            _chk(self.ctx.lib.b32_scene_swap(self.ctx.h, self._slot), "scene_swap")
        return self

    def _swap(self):
        if self._slot is not None:
            _chk(self.ctx.lib.b32_scene_swap(self.ctx.h, self._slot), "scene_swap")

    def close(self):
        if self._slot is not None:
            self.ctx.lib.b32_scene_destroy(self.ctx.h, self._slot)
            self._slot = None

    def _handle(self):
        """The slot argument of the bone calls: this scene's slot, or None (the context's resident scene)."""
        return self._slot

    def set_rig(self, bone_of_vertex):
        """b32_scene_set_rig: the vertices as they are now become the rest pose; bone_of_vertex has one index per vertex (abi.BONE_NONE:
        no bone), resolved by the caller (v.bone_index.or(obj.default_bone_index))."""
        bo = np.ascontiguousarray(bone_of_vertex, np.uint16).reshape(-1)
        if len(bo) != self.n_body_vertices:
            raise ValueError("set_rig: one bone index per vertex")
        _chk(self.ctx.lib.b32_scene_set_rig(self.ctx.h, self._handle(), abi.ptr(bo) if len(bo) else None), "scene_set_rig")

    def pose(self, bones):
        """b32_scene_pose: enqueue one pose pass with this bone table (a sequence of Bone or an abi.BONE_DTYPE array; empty: the rest
        vertices come back)."""
        tab = pack_bones(bones)
        _chk(self.ctx.lib.b32_scene_pose(self.ctx.h, self._handle(), abi.ptr(tab) if len(tab) else None, len(tab)), "scene_pose")

    def build_skeleton(self, bones, style=None):
        """b32_scene_build_skeleton: enqueue one kernel that replaces the slot's tail with the octahedra of this skeleton (a sequence of
        SkelBone or an abi.SKEL_BONE_DTYPE array; empty and no preview: the tail goes).  n_vertices / n_faces are the slot's totals
        afterwards, n_body_vertices / n_body_faces what the upload left: rig, pose, hover, box selection, pick and the selection overlays
        see the body only."""
        tab = pack_skel_bones(bones)
        st = (style or SkeletonStyle()).pack()
        nv, nf = C.c_uint32(0), C.c_uint32(0)
        args = (abi.ptr(tab) if len(tab) else None, len(tab), abi.ptr(st))
        _chk(self.ctx.lib.b32_skeleton_counts(*args, C.byref(nv), C.byref(nf)), "skeleton_counts")
        _chk(self.ctx.lib.b32_scene_build_skeleton(self.ctx.h, self._handle(), *args), "scene_build_skeleton")
        self._tail_v, self._tail_f = nv.value, nf.value

    def read_vertices(self, first=0, count=None):
        """b32_scene_read_vertices (blocking): the slot's vertices as they are on the device now."""
        count = self.n_vertices - first if count is None else count
        out = np.zeros(max(count, 0), abi.VERTEX_DTYPE)
        _chk(self.ctx.lib.b32_scene_read_vertices(self.ctx.h, self._handle(), first, count, abi.ptr(out) if count > 0 else None), "scene_read_vertices")
        return out

    def bounds(self):
        """b32_scene_bounds (blocking): Asset::bounds of the body's vertices as they are on the device now -- (min, max, has_verts), the
        cached reduction OBJECT_BOX_MESH reads; reduced again only after the vertices changed."""
        mn, mx, has = (C.c_float * 3)(), (C.c_float * 3)(), C.c_uint32()
        _chk(self.ctx.lib.b32_scene_bounds(self.ctx.h, self._handle(), mn, mx, C.byref(has)), "scene_bounds")
        return np.array(mn[:], np.float32), np.array(mx[:], np.float32), bool(has.value)

    def bounds_async(self, out=None):
        """b32_scene_bounds_async: (ticket, (array, pointer) of 32 page-locked bytes -- abi.SCENE_BOUNDS_DTYPE once the ticket is done)."""
        buf = out if out is not None else self.ctx.host_alloc(32)
        t = C.c_uint64()
        _chk(self.ctx.lib.b32_scene_bounds_async(self.ctx.h, self._handle(), buf[1], C.byref(t)), "scene_bounds_async")
        return int(t.value), buf

    def read_faces(self, first=0, count=None):
        """b32_scene_read_faces (blocking): the slot's faces as they are on the device now."""
        count = self.n_faces - first if count is None else count
        out = np.zeros(max(count, 0), abi.FACE_DTYPE)
        _chk(self.ctx.lib.b32_scene_read_faces(self.ctx.h, self._handle(), first, count, abi.ptr(out) if count > 0 else None), "scene_read_faces")
        return out

    # ---- in-place edits (b32_scene_patch_*): nothing is uploaded again, the rig, the pose and the tail stay
    def patch_vertices(self, indices, vertices):
        """b32_scene_patch_vertices: whole vertex records at strictly ascending body indices; on a rigged scene they are in rest space."""
        recs = np.zeros(len(np.asarray(indices).reshape(-1)), abi.VERTEX_PATCH_DTYPE)
        recs["index"] = np.asarray(indices).reshape(-1)
        recs["v"] = np.asarray(vertices, abi.VERTEX_DTYPE).reshape(-1)
        _chk(self.ctx.lib.b32_scene_patch_vertices(self.ctx.h, self._handle(), abi.ptr(recs) if len(recs) else None, len(recs)), "scene_patch_vertices")

    def patch_faces(self, indices, faces):
        """b32_scene_patch_faces: whole face records at strictly ascending body indices (the first call after an upload synchronises once)."""
        recs = np.zeros(len(np.asarray(indices).reshape(-1)), abi.FACE_PATCH_DTYPE)
        recs["index"] = np.asarray(indices).reshape(-1)
        recs["f"] = np.asarray(faces, abi.FACE_DTYPE).reshape(-1)
        _chk(self.ctx.lib.b32_scene_patch_faces(self.ctx.h, self._handle(), abi.ptr(recs) if len(recs) else None, len(recs)), "scene_patch_faces")

    @staticmethod
    def _rows(block, dtype, tail):
        """A rectangle as the library takes it: (array to keep alive, h, w, stride in elements).  A view whose rows are contiguous is
        passed with its own stride; anything else is copied."""
        b = np.asarray(block, dtype)
        if b.ndim != 2 + len(tail) or b.shape[2:] != tail:
            raise ValueError("patch: the rectangle is (h, w%s)" % "".join(", %d" % k for k in tail))
        elem = b.dtype.itemsize * int(np.prod(tail, dtype=np.int64))
        h, w = b.shape[:2]
        inner = b.strides[1] == elem and (not tail or b.strides[2] == b.dtype.itemsize)
        if h and w and not (inner and b.strides[0] % elem == 0 and b.strides[0] >= w * elem):
            b = np.ascontiguousarray(b)
        return b, h, w, (b.strides[0] // elem if h and w else w)

    def patch_texels(self, tex, x, y, block):
        """b32_scene_patch_texels: `block` is (h, w) Color15 for an RGB555 scene, (h, w, 4) Color bytes for an 8-bit-colour one."""
        b, h, w, stride = self._rows(block, np.uint8 if self.fmt8 else np.uint16, (4,) if self.fmt8 else ())
        _chk(self.ctx.lib.b32_scene_patch_texels(self.ctx.h, self._handle(), tex, x, y, w, h, b.ctypes.data if b.size else None, stride), "scene_patch_texels")

    def patch_indexed(self, tex, x, y, index_block, clut):
        """b32_scene_patch_indexed: `index_block` is (h, w) index bytes, `clut` the palette they are looked up in."""
        b, h, w, stride = self._rows(index_block, np.uint8, ())
        cl = np.ascontiguousarray(clut, np.uint16).reshape(-1)
        _chk(self.ctx.lib.b32_scene_patch_indexed(self.ctx.h, self._handle(), tex, x, y, w, h, b.ctypes.data if b.size else None, stride,
                                                  abi.ptr(cl) if len(cl) else None, len(cl)), "scene_patch_indexed")

    def read_texels(self, tex, width, height):
        """b32_scene_read_texels (blocking): the expanded pool texels of texture `tex`, whose size the caller states: (height, width)
        Color15, or (height, width, 4) Color bytes on an 8-bit-colour scene."""
        out = np.zeros((height, width, 4), np.uint8) if self.fmt8 else np.zeros((height, width), np.uint16)
        _chk(self.ctx.lib.b32_scene_read_texels(self.ctx.h, self._handle(), tex, abi.ptr(out) if out.size else None), "scene_read_texels")
        return out

    def _pack(self, camera, settings, fog):
        cam = camera.pack()
        st, kl = settings.pack()
        fg = T.pack_fog(fog)
        self._packed = (cam, st, kl, fg)
        return self._packed

    def render_placed_async(self, placement):
        """b32_render_scene_15_placed_async with the last packed camera / settings / fog: RGB555 and 8-bit-colour scenes alike."""
        cam, st, _kl, fg = self._packed
        pl = _pack_placement(placement)
        self._swap()
        try:
            _chk(self.ctx.lib.b32_render_scene_15_placed_async(self.ctx.h, C.byref(cam), C.byref(st), C.byref(fg) if fg is not None else None,
                                                               C.byref(pl) if pl is not None else None), "render_scene_15_placed_async")
        finally:
            self._swap()

    def render(self, camera, settings, fog=None) -> T.RasterTimings:
        cam, st, _kl, fg = self._pack(camera, settings, fog)
        tm = abi.B32Timings()
        self._swap()
        try:
            if self.fmt8:
                _chk(self.ctx.lib.b32_render_scene(self.ctx.h, C.byref(cam), C.byref(st), C.byref(tm)), "render_scene")
            else:
                _chk(self.ctx.lib.b32_render_scene_15(self.ctx.h, C.byref(cam), C.byref(st),
                                                      C.byref(fg) if fg is not None else None, C.byref(tm)), "render_scene_15")
        finally:
            self._swap()
        return T.RasterTimings.from_c(tm)

    def render_async(self, camera=None, settings=None, fog=None, placement=None):
        """Enqueue only. With no arguments, re-enqueues the last packed camera/settings (no Python packing cost).
        placement: a Placement (or abi.B32Placement) -- the resident mesh is drawn rotated and moved, nothing is uploaded."""
        if camera is not None:
            self._pack(camera, settings, fog)
        if placement is not None:
            return self.render_placed_async(placement)
        cam, st, _kl, fg = self._packed
        self._swap()
        try:
            if self.fmt8:
                _chk(self.ctx.lib.b32_render_scene_async(self.ctx.h, C.byref(cam), C.byref(st)), "render_scene_async")
            else:
                _chk(self.ctx.lib.b32_render_scene_15_async(self.ctx.h, C.byref(cam), C.byref(st),
                                                            C.byref(fg) if fg is not None else None), "render_scene_15_async")
        finally:
            self._swap()

    def finish(self) -> T.RasterTimings:
        tm = abi.B32Timings()
        _chk(self.ctx.lib.b32_frame_finish(self.ctx.h, C.byref(tm)), "frame_finish")
        return T.RasterTimings.from_c(tm)
