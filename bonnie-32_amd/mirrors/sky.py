"""The resident sky and the star records in numpy float32 / int32: what k_sky_place_project and k_star_records compute, operation for
operation.  Imports neither the binding nor the library."""
import numpy as np

from .. import abi

_QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def sky_place(offsets, cam_pos):
    """Skybox::generate_mesh's positions (world/geometry.rs:555-559, :686-710) from the camera-independent products: camera_pos + offset,
    one f32 addition per component.  `offsets`: an abi.SKY_VERTEX_DTYPE array (returned as a placed copy) or (n, 3) positions."""
    c = np.asarray(cam_pos, np.float32).reshape(3)
    if getattr(offsets, "dtype", None) is not None and offsets.dtype.names:
        out = np.array(offsets, abi.SKY_VERTEX_DTYPE)
        with np.errstate(all="ignore"):
            out["pos"] = (c[None, :] + out["pos"]).astype(np.float32)
        return out
    with np.errstate(all="ignore"):
        return (c[None, :] + np.asarray(offsets, np.float32).reshape(-1, 3)).astype(np.float32)


def sky_project(offsets, camera, width, height):
    """b32_sky_project_batch: (n, 2) f32 screen points of the placed vertices (render.rs:97-103 -> math.rs:103-136), the quiet NaN
    0x7FC00000 twice for a vertex behind the camera.  rel = (camera + offset) - camera: two roundings, not the offset."""
    f32 = np.float32
    off = offsets["pos"] if getattr(offsets, "dtype", None) is not None and offsets.dtype.names else offsets
    cp, bx, by, bz = (np.asarray(getattr(camera, n), f32) for n in ("position", "basis_x", "basis_y", "basis_z"))
    with np.errstate(all="ignore"):
        rel = (sky_place(np.asarray(off, f32).reshape(-1, 3), cp) - cp[None, :]).astype(f32)
        cx, cy, cz = (((rel[:, 0] * b[0] + rel[:, 1] * b[1]).astype(f32) + rel[:, 2] * b[2]).astype(f32) for b in (bx, by, bz))
        vs = f32(f32(min(width, height)) / f32(2.0)) * f32(0.75)
        hw, hh = f32(width) / f32(2.0), f32(height) / f32(2.0)
        denom = (cz + f32(5.0)).astype(f32)
        sx = ((cx * f32(4.0)) / denom * vs + hw).astype(f32)
        sy = ((cy * f32(4.0)) / denom * vs + hh).astype(f32)
        flat = np.abs(denom) < f32(0.001)
        behind = cz <= f32(0.1)
    sx = np.where(behind, _QNAN, np.where(flat, hw, sx)).astype(f32)
    sy = np.where(behind, _QNAN, np.where(flat, hh, sy)).astype(f32)
    return np.stack([sx, sy], axis=1)


def star_per(size):
    """The set_pixel_safe calls of one star: s = size.max(1.0) as i32 (render.rs:207; NaN -> 1, the cast saturates) -> 1, 5 or 9."""
    s = np.float32(size)
    return 9 if s >= np.float32(3.0) else (5 if s >= np.float32(2.0) else 1)


_STAR_DX = np.array([0, -1, 1, 0, 0, -2, 2, 0, 0], np.int64)
_STAR_DY = np.array([0, 0, 0, -1, 1, 0, 0, -2, 2], np.int64)
_STAR_SCALE = np.array([1.0, 0.7, 0.7, 0.7, 0.7, 0.4, 0.4, 0.4, 0.4], np.float32)


def star_records(stars, size):
    """b32_star_records_batch: draw_star_diamond (render.rs:206-237) for every star of `stars` (abi.STAR_DTYPE) as abi.PRIM_DTYPE records,
    star i's at [i * per, (i + 1) * per): each set_pixel_safe call a 1x1 FILLED_RECT.  cx + dx wraps like a release build's i32."""
    st = np.ascontiguousarray(stars, abi.STAR_DTYPE).reshape(-1)
    per = star_per(size)
    n = len(st)
    out = np.zeros(n * per, abi.PRIM_DTYPE)
    if not n:
        return out

    def wrap(v):
        return (((v + 2**31) % 2**32) - 2**31).astype(np.int32)
    x = wrap(st["cx"].astype(np.int64)[:, None] + _STAR_DX[None, :per]).reshape(-1)
    y = wrap(st["cy"].astype(np.int64)[:, None] + _STAR_DY[None, :per]).reshape(-1)
    out["x0"], out["x1"], out["y0"], out["y1"] = x, x, y, y
    for ch in "rgb":
        c = st[ch].astype(np.float32)[:, None] * _STAR_SCALE[None, :per]           # (c as f32 * 0.7) as u8; the centre keeps c
        out[ch] = np.where(np.arange(per)[None, :] == 0, st[ch][:, None], c.astype(np.uint8)).reshape(-1)
    out["blend"], out["kind"], out["alpha"] = abi.OPAQUE, abi.PRIM_FILLED_RECT, 255
    return out
