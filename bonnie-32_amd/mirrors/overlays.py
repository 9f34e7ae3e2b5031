"""The editors' overlays as abi.PRIM_DTYPE records in numpy float32, place for place what the device producers make
(b32_draw_room_overlay, b32_draw_object_overlays, b32_draw_mesh_overlay), and the line helpers they draw through."""
import numpy as np

from .. import abi
from ..records import noop_prims
from .room import _ROOM_XSEL, _ROOM_ZSEL, RoomMirror, _room_grid, room_hover_winner
from .screen import _positions, _project_f32

# ---- the world editor's room overlays (editor/viewport_3d.rs:4273-4658, :4862-5362) from a room's records: b32_draw_room_overlay and its mirror
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
    pos, bz = (np.array([f32(v) for v in getattr(camera, k)], f32) for k in ("position", "basis_z"))
    vdot = lambda r, b: (r[:, 0] * b[0] + r[:, 1] * b[1]) + r[:, 2] * b[2]
    NEAR = f32(0.1)
    with np.errstate(all="ignore"):
        z0, z1 = vdot(P0 - pos, bz), vdot(P1 - pos, bz)
        b0, b1 = z0 <= NEAR, z1 <= NEAR
        t = (NEAR - z0) / (z1 - z0)
        Q = (P0 + (P1 - P0) * t[:, None]).astype(f32)
        C0 = np.where((b0 & ~b1)[:, None], Q, P0); C1 = np.where((~b0 & b1)[:, None], Q, P1)
        x0, y0, _d0, some0 = _project_f32(C0[:, 0], C0[:, 1], C0[:, 2], camera, w, h, None)
        x1, y1, _d1, some1 = _project_f32(C1[:, 0], C1[:, 1], C1[:, 2], camera, w, h, None)
        ok = ~(b0 & b1) & some0 & some1
    return x0, y0, x1, y1, ok


def _cast_segments(x0, y0, x1, y1, ok):
    """Both ends cast (`as i32`) and the call's fate: (x0, y0, x1, y1 as int64, state 0 drawn / 1 dropped (not ok) / 2 rejected (an extent >= 2^30))"""
    ix0, iy0, ix1, iy1 = (_ov_i32(v).astype(np.int64) for v in (x0, y0, x1, y1))
    lim = 1 << 30
    return ix0, iy0, ix1, iy1, np.where(ok, np.where((np.abs(ix1 - ix0) >= lim) | (np.abs(iy1 - iy0) >= lim), 2, 0), 1)


def _np_draw_3d_lines_clipped(P0, P1, camera, w, h):
    """draw_3d_line_clipped (draw.rs:12-67) for m segments at once in f32: the near clip, world_to_screen, the cast -- no screen clip.
    Returns what _np_draw_3d_lines returns."""
    return _cast_segments(*_np_near_clip_project(P0, P1, camera, w, h))


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
    return _cast_segments(x0, y0, x1, y1, ok & accept)


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
        x0, y0, x1, y1, state = _cast_segments(ax, ay, bx_, by_, asome & bsome)
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


# ---- the modeler's selection overlays (modeler/viewport.rs:1782-2247) from vertex positions: b32_draw_mesh_overlay and its mirror
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
