"""Bones, poses, in-place edits and the skeleton's octahedra in numpy float32 (b32_scene_pose, b32_scene_patch_*, b32_scene_build_skeleton)."""
import numpy as np

from .. import abi
from ..records import Bone, pack_bones, pack_skel_bones


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


# ---- mirror editing (b32_scene_build_mirror): the mesh the modeler assembles while MirrorSettings is enabled (viewport.rs:1209-1311)
class MeshMirror:
    """What b32_scene_build_mirror leaves in its derived slot, in numpy: the source body's vertices with the selected range's twins
    behind the range, the range's faces each followed by its twin, later faces shifted.  The rules are methods so that a test can change
    one of them and watch a case move."""

    @staticmethod
    def flip(a):
        """Rust's -x on the bits of a float32 array: -0.0 <-> +0.0, a NaN keeps its payload."""
        return (np.ascontiguousarray(a, np.float32).view(np.uint32) ^ np.uint32(0x80000000)).view(np.float32)

    def dim_channel(self, ch, dim):
        """(ch as f32 * dim) as u8 with Rust's saturating cast (NaN -> 0)."""
        with np.errstate(all="ignore"):
            f = np.asarray(ch, np.uint8).astype(np.float32) * np.float32(dim)
            t = np.where(f > 0, np.minimum(np.trunc(f), np.float32(255.0)), np.float32(0.0))
        return t.astype(np.uint8)

    def mirror_local(self, pos, normal, axis):
        """mirror_position / mirror_normal (state.rs:832-848): (pos, normal) with the axis component's sign flipped."""
        pos, normal = np.array(pos, np.float32, copy=True), np.array(normal, np.float32, copy=True)
        pos[:, axis - 1] = self.flip(pos[:, axis - 1])
        normal[:, axis - 1] = self.flip(normal[:, axis - 1])
        return pos, normal

    def twin_posed(self, pos, normal, axis, pose):
        """First mirror in local space, then the vertex's bone (viewport.rs:1250-1266).  pose: (pos, normal) -> (pos, normal)."""
        return pose(*self.mirror_local(pos, normal, axis))

    def twin_blend(self, src_blend):
        """Color::new sets BlendMode::Opaque (types.rs:773-775)."""
        return np.full(len(src_blend), abi.OPAQUE, np.uint8)

    def twin_face(self, v, c):
        """(mirror_offset + v0, mirror_offset + v2, mirror_offset + v1), wrapping u32 adds."""
        return self.shifted(v[:, [0, 2, 1]], c)

    @staticmethod
    def shifted(v, c):
        return ((np.asarray(v, np.uint32).astype(np.uint64) + np.uint64(c)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)

    def range_faces(self, faces, c):
        """Each face of the range, its twin directly behind it."""
        out = np.zeros(2 * len(faces), abi.FACE_DTYPE)
        out[0::2] = faces
        tw = np.array(faces, copy=True)
        tw["v"] = self.twin_face(faces["v"], c)
        out[1::2] = tw
        return out

    def later_faces(self, faces, c):
        """A later object's faces: vertex_offset has grown by the twins."""
        out = np.array(faces, copy=True)
        out["v"] = self.shifted(faces["v"], c)
        return out

    def twins(self, src, local_pos, local_normal, mirror, bone_of, bones):
        """The twins of the records `src` whose local positions and normals are given; bone_of None: no rig."""
        t = np.array(src, dtype=abi.VERTEX_DTYPE, copy=True)

        def pose(p, n):
            if bone_of is None:
                return p, n
            r = np.zeros(len(p), abi.VERTEX_DTYPE)
            r["pos"], r["normal"] = p, n
            r = pose_vertices(r, bone_of, bones if bones is not None else ())
            return r["pos"], r["normal"]

        p, n = self.twin_posed(local_pos, local_normal, int(mirror["axis"]), pose)
        t["pos"].view(np.uint32)[...] = np.ascontiguousarray(p, np.float32).view(np.uint32)
        t["normal"].view(np.uint32)[...] = np.ascontiguousarray(n, np.float32).view(np.uint32)
        for ch in ("r", "g", "b"):
            t[ch] = self.dim_channel(src[ch], mirror["dim"])
        t["blend"] = self.twin_blend(src["blend"])
        return t

    def mesh(self, vertices, faces, mirror, rest=None, bone_of=None, bones=None):
        from ..records import pack_mirror
        m = pack_mirror(mirror)[0]
        v = np.asarray(vertices, abi.VERTEX_DTYPE).reshape(-1)
        f = np.asarray(faces, abi.FACE_DTYPE).reshape(-1)
        v0, c, f0, fc = int(m["v_first"]), int(m["v_count"]), int(m["f_first"]), int(m["f_count"])
        if m["axis"] not in (1, 2, 3) or v0 + c > len(v) or f0 + fc > len(f):
            raise ValueError("mirror_mesh: axis is 1..3 and the ranges lie inside the body")
        src = v[v0:v0 + c]
        if rest is not None:
            r = np.asarray(rest, np.float32).reshape(-1, 6)[v0:v0 + c]
            lp, ln = r[:, 0:3], r[:, 3:6]
            bo = np.asarray(bone_of).reshape(-1)[v0:v0 + c]
        else:
            lp, ln, bo = src["pos"], src["normal"], None
        tw = self.twins(src, lp, ln, m, bo, bones)
        vo = np.concatenate([v[:v0 + c], tw, v[v0 + c:]])
        fo = np.concatenate([f[:f0], self.range_faces(f[f0:f0 + fc], c), self.later_faces(f[f0 + fc:], c)])
        return vo, fo


def mirror_mesh(vertices, faces, mirror, rest=None, bone_of=None, bones=None):
    """MeshMirror().mesh: (vertices, faces) b32_scene_build_mirror writes for a source body `vertices` / `faces` (posed, if the source is
    posed) and a Mirror.  rest / bone_of / bones: the source's rig -- its (n, 6) rest stream, its bone index per vertex and the table of
    its last pose (None or empty: none yet); without `rest` the source has no rig and the twins mirror the vertices as they are."""
    return MeshMirror().mesh(vertices, faces, mirror, rest, bone_of, bones)


# ---- the bone octahedra (b32_scene_build_skeleton, b32_skeleton_items): skeleton_to_triangles / draw_skeleton / draw_bone_dots
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
