"""What every mirror shares, each rule once: placement and projection of positions, the projected-triangle table, the triangle test and its
depth, the closest hit in order, the selection words.  Every operation is one separately rounded f32 operation in the reference's order."""
import numpy as np

from .. import abi
from ..records import _placement_triple, _positions  # noqa: F401  (_positions: the positions of a vertex array, for every mirror)


def _world_f32(pos, placement):
    """The positions the loops project: as they are (placement None) or placed as check_mesh_hit does (viewport_3d.rs:7716-7718)."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    if placement is None:
        return x, y, z
    c, s, wp = _placement_triple(placement)
    return (x * c - z * s) + wp[0], y + wp[1], (x * s + z * c) + wp[2]


def _project_f32(x, y, z, camera, w, h, ortho):
    """world_to_screen_with_ortho (math.rs:538-575; its two branches :595-599, never None, and :621-652) on f32 arrays: (sx, sy, cam_z, some)."""
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


class _TriangleTable:
    """The projected triangles `fv` ((n, 3) int64 indices): ok (screen_verts.get(..): an index out of range skips the triangle; every corner
    projects), the corners' x, y and depth d, the signed area and `front` (modeler/viewport.rs:2571-2574: a NaN area is not culled)."""

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

    def candidates(self, mx, my, cull_backfaces=False):
        """(triangle indices in face order, their depths) of every triangle the cursor hits."""
        px, py = np.float32(mx), np.float32(my)
        with np.errstate(all="ignore"):
            hit = self.ok & _point_in_triangle(px, py, *self.x, *self.y)
            if cull_backfaces:
                hit &= self.front
            t = np.nonzero(hit)[0]
            depth = _depth_in_triangle(px, py, *(v[t] for v in self.x), *(v[t] for v in self.y), *(v[t] for v in self.d))
        return t, depth


def _point_in_triangle(px, py, x0, x1, x2, y0, y1, y2):
    """point_in_triangle_2d, math.rs:687-706"""
    d1 = (px - x1) * (y0 - y1) - (x0 - x1) * (py - y1)
    d2 = (px - x2) * (y1 - y2) - (x1 - x2) * (py - y2)
    d3 = (px - x0) * (y2 - y0) - (x2 - x0) * (py - y0)
    has_neg = (d1 < 0) | (d2 < 0) | (d3 < 0)
    has_pos = (d1 > 0) | (d2 > 0) | (d3 > 0)
    return ~(has_neg & has_pos)


def _depth_in_triangle(px, py, x0, x1, x2, y0, y1, y2, e0, e1, e2):
    """interpolate_depth_in_triangle, viewport_3d.rs:7485-7508"""
    f32 = np.float32
    area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    w0 = ((x1 - px) * (y2 - py) - (x2 - px) * (y1 - py)) / area
    w1 = ((x2 - px) * (y0 - py) - (x0 - px) * (y2 - py)) / area
    w2 = f32(1.0) - w0 - w1
    return np.where(np.abs(area) < f32(0.0001), (e0 + e1 + e2) / f32(3.0), w0 * e0 + w1 * e1 + w2 * e2).astype(f32)


def _triangle_hit(px, py, x, y, d):
    """(inside, depth) of the cursor in triangles given as three x, three y and three depths."""
    return _point_in_triangle(px, py, *x, *y), _depth_in_triangle(px, py, *x, *y, *d)


def _closest_in_order(ids, depth):
    """`closest = None; for (id, depth): if closest is None or depth < closest.depth: closest = (depth, id)` without the loop: the first
    of equal depths, a NaN depth only when it is the first hit (reported as the quiet NaN 0x7FC00000); no hit: (False, 0xFFFFFFFF, 0.0)."""
    f32 = np.float32
    if not len(ids):
        return False, abi.PICK_NO_TRI, f32(0.0)
    if np.isnan(depth[0]):
        return True, int(ids[0]), np.array([0x7FC00000], np.uint32).view(f32)[0]
    num = ~np.isnan(depth)
    j = int(np.nonzero(num & (depth == depth[num].min()))[0][0])
    return True, int(ids[j]), depth[j]


def _selection_words(sel):
    """(words, n_selected) of a box selection: bit i of word i // 32 set iff element i is selected."""
    n = len(sel)
    bits = np.zeros(((n + 31) // 32) * 32, np.uint8)
    bits[:n] = sel
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    return words, int(sel.sum())
