"""Picking, hover and box selection of one mesh in numpy float32 (b32_pick_meshes, b32_hover_mesh, b32_box_select): a host's walk per mouse move."""
import numpy as np

from .. import abi
from ..records import _placement_triple
from .screen import _TriangleTable, _closest_in_order, _positions, _project_f32, _selection_words, _world_f32


class PickMirror(_TriangleTable):
    """check_mesh_hit (editor/viewport_3d.rs:7700-7756) and the face branch of find_hovered_element (modeler/viewport.rs:2544-2594) for one
    placed mesh in numpy float32: what b32_pick_meshes computes per item, and what a host without this library walks per mouse move.
    The constructor does what the reference does once per mesh and frame (place and project every vertex: screen_verts); pick() is the
    triangle loop for one cursor.  Every operation is one separately rounded f32 operation in the reference's order."""

    def __init__(self, vertices, faces, placement, camera, w, h, ortho=None):
        fv = np.ascontiguousarray(faces["v"] if getattr(faces, "dtype", None) is not None and faces.dtype.names else faces).reshape(-1, 3).astype(np.int64)
        with np.errstate(all="ignore"):
            placed = _world_f32(_positions(vertices), _placement_triple(placement))     # picking always places: None is an error, as ever
            super().__init__(*_project_f32(*placed, camera, w, h, ortho), fv)

    def pick(self, mx, my, cull_backfaces=False):
        """(hit, tri, depth): the closest hit by the reference's strict `<` in face order -- the first of equal depths, a NaN depth only when
        it is the first hit (reported as the quiet NaN 0x7FC00000); no hit: (False, 0xFFFFFFFF, 0.0)."""
        t, depth = self.candidates(mx, my, cull_backfaces)
        return _closest_in_order(t, depth)


def pick_mesh(vertices, faces, placement, camera, w, h, mx, my, ortho=None, cull_backfaces=False):
    """Host mirror of one item of b32_pick_meshes (see PickMirror): (hit, tri, depth)."""
    return PickMirror(vertices, faces, placement, camera, w, h, ortho).pick(mx, my, cull_backfaces)


def pick_best(hits):
    """The loop over the items (viewport_3d.rs:7370) on a PICK_HIT_DTYPE array: the index of the closest hit item, or -1."""
    hits = np.asarray(hits, abi.PICK_HIT_DTYPE)
    i = np.nonzero(hits["hit"])[0]
    hit, best, _ = _closest_in_order(i, hits["depth"][i])
    return best if hit else -1


# ---- hover and box selection (b32_hover_mesh, b32_box_select): the modeler's find_hovered_element / apply_box_selection for one mesh
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
        self.faces = _TriangleTable(sx, sy, self.cz, some, t.fan)              # the fan triangles, as PickMirror walks a mesh's

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
    return _selection_words(sel)
