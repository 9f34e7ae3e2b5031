"""A room's sector records, render mesh, hover and box selection in numpy float32 (b32_room_build_mesh, b32_room_hover, b32_room_box_select)."""
import numpy as np

from .. import abi
from .. import rtypes as T
from .screen import _closest_in_order, _project_f32, _selection_words, _triangle_hit

# ---- room hover and box selection (b32_room_hover, b32_room_box_select): the world editor's find_hovered_elements / find_selections_in_rect
_ROOM_KEYS = (("floor", abi.ROOM_FLOOR), ("ceiling", abi.ROOM_CEILING), ("walls_north", abi.ROOM_WALL_NORTH), ("walls_east", abi.ROOM_WALL_EAST),
              ("walls_south", abi.ROOM_WALL_SOUTH), ("walls_west", abi.ROOM_WALL_WEST), ("walls_nwse", abi.ROOM_WALL_NWSE), ("walls_nesw", abi.ROOM_WALL_NESW))
# corner k's (x, z) selectors per kind, 0 = base, 1 = base + S (viewport_3d.rs:6603-6657, :7099-7170, :7183-7279)
_ROOM_XSEL = np.array([[0, 1, 1, 0], [0, 1, 1, 0], [0, 1, 1, 0], [1, 1, 1, 1], [1, 0, 0, 1], [0, 0, 0, 0], [0, 1, 1, 0], [1, 0, 0, 1]], bool)
_ROOM_ZSEL = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 0, 0], [0, 1, 1, 0], [1, 1, 1, 1], [1, 0, 0, 1], [0, 1, 1, 0], [0, 1, 1, 0]], bool)
# wall_center_in_rect's own (x0, z0, x1, z1) per direction, as selectors (viewport_3d.rs:7633-7640); rows 0 and 1 are unused
_ROOM_CENTRE_SEL = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0], [1, 0, 1, 1], [0, 1, 1, 1], [0, 0, 0, 1], [0, 0, 1, 1], [1, 0, 0, 1]], bool)


def _sector_faces(sectors):
    """(gx, gz, kind, i, face) of every face in the reference's one loop order (iter_sectors, world/geometry.rs:2828-2835): gx outer, gz
    inner; inside a sector floor, ceiling, the north, east, south and west walls by i, then the nwse and the nesw walls."""
    for gx, col in enumerate(sectors):
        for gz, sec in enumerate(col):
            if sec is None:
                continue
            for key, kind in _ROOM_KEYS:
                got = sec.get(key)
                if got is not None:
                    for i, face in enumerate([got] if kind < 2 else list(got)):
                        yield gx, gz, kind, i, face


def room_faces_from_sectors(sectors):
    """A room's sector grid as abi.SECTOR_FACE_DTYPE records in the reference's one loop order (_sector_faces).
    sectors[gx][gz] is None or a mapping with the optional keys floor, ceiling (one face) and walls_north, walls_east, walls_south,
    walls_west, walls_nwse, walls_nesw (lists of faces); a face is four heights or a mapping with "heights"."""
    rows = [(gx, gz, kind, i, 0, tuple(float(np.float32(v)) for v in (face["heights"] if hasattr(face, "keys") else face)))
            for gx, gz, kind, i, face in _sector_faces(sectors)]
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
    rows = [(kind, face if hasattr(face, "keys") else {}) for _gx, _gz, kind, _i, face in _sector_faces(sectors)]
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
            # faces, check_quad_hit_with_depth, viewport_3d.rs:7436-7481: the triangles (0, 1, 2) and (0, 2, 3)
            in_a, dep_a = _triangle_hit(px, py, *([a[:, k] for k in (0, 1, 2)] for a in (sx, sy, d)))
            in_b, dep_b = _triangle_hit(px, py, *([a[:, k] for k in (0, 2, 3)] for a in (sx, sy, d)))
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
        return _selection_words(sel)


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
