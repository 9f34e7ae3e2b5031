"""The sky of the game tab's frame without a host wait: a resident sky (b32_sky) drawn from the camera alone, and the star sprites as
records of the ordered tile pass (b32_draw_stars).

    from bonnie32_amd import sky
    s = sky.ResidentSky(fb.ctx, offsets, faces)       # offsets: generate_mesh((0, 0, 0), time) -- its positions are the offsets
    s.render(fb, camera)                              # per frame: enqueued, never waits
    s.update(first, vertices)                         # while a cloud layer scrolls: the rows inside it
    sky.draw_stars(fb, stars, 3.0)                    # stars: abi.STAR_DTYPE (records.pack_stars)

pack_stars / pack_sky_vertices (records.py) and the numpy mirror sky_place / sky_project / star_records (mirrors/sky.py) are re-exported
here; this module imports neither the binding nor the library: a context or a framebuffer brings it."""
import ctypes as C

import numpy as np

from . import abi
from .mirrors.sky import sky_place, sky_project, star_per, star_records  # noqa: F401
from .records import _chk, pack_sky_vertices, pack_stars  # noqa: F401


def _ctx(ctx):
    """A Context, or what holds one (a Framebuffer)."""
    return getattr(ctx, "ctx", ctx)


class ResidentSky:
    """A resident sky (b32_sky) of one context: the camera-independent offsets with their colours, and the faces."""

    def __init__(self, ctx, offsets, faces):
        self.ctx = _ctx(ctx)
        v = pack_sky_vertices(offsets)
        f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
        self.n_vertices, self.n_faces = len(v), len(f)
        h = C.c_void_p()
        _chk(self.ctx.lib.b32_sky_create(self.ctx.h, abi.ptr(v) if len(v) else None, len(v), abi.ptr(f) if len(f) else None, len(f), C.byref(h)),
             "sky_create")
        self._h = h

    def update(self, first, vertices):
        """b32_sky_update: vertices [first, first + len(vertices)) replaced, ordered on the context's stream; no host synchronisation."""
        v = pack_sky_vertices(vertices)
        _chk(self.ctx.lib.b32_sky_update(self.ctx.h, self._h, int(first), len(v), abi.ptr(v) if len(v) else None), "sky_update")

    def render(self, fb, camera):
        """b32_render_sky: step 1 of Framebuffer::render_skybox for generate_mesh(camera.position, ..) on `fb` (a Framebuffer of this
        sky's context, or of another one: B32_E_ARG); enqueued, never waits."""
        cam = camera.pack() if hasattr(camera, "pack") else camera
        c = _ctx(fb)
        _chk(c.lib.b32_render_sky(c.h, self._h, C.byref(cam)), "render_sky")

    def project_batch(self, camera, width, height):
        """b32_sky_project_batch (stage tap, blocking): (n_vertices, 2) f32 screen points, a NaN pair behind the camera."""
        cam = camera.pack() if hasattr(camera, "pack") else camera
        xy = np.zeros((self.n_vertices, 2), np.float32)
        _chk(self.ctx.lib.b32_sky_project_batch(self.ctx.h, self._h, C.byref(cam), int(width), int(height), abi.ptr(xy) if len(xy) else None),
             "sky_project_batch")
        return xy

    def destroy(self):
        if self._h and getattr(self.ctx, "h", None):
            self.ctx.lib.b32_sky_destroy(self.ctx.h, self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()


def draw_stars(fb, stars, size):
    """b32_draw_stars: draw_star_diamond (render.rs:206-237) for every star of `stars` (abi.STAR_DTYPE) in order, through the ordered tile
    pass; enqueued, no host synchronisation."""
    s = pack_stars(stars)
    c = _ctx(fb)
    _chk(c.lib.b32_draw_stars(c.h, abi.ptr(s) if len(s) else None, len(s), float(size)), "draw_stars")


def star_record_count(n, size, lib=None):
    """b32_star_record_count (host only): the records b32_draw_stars makes of n stars."""
    lib = lib or abi.load_library()
    r = C.c_uint64(0)
    _chk(lib.b32_star_record_count(int(n), float(size), C.byref(r)), "star_record_count")
    return int(r.value)


def star_records_batch(ctx, stars, size):
    """b32_star_records_batch (stage tap, blocking): the abi.PRIM_DTYPE records k_star_records writes for `stars`."""
    s = pack_stars(stars)
    c = _ctx(ctx)
    n = star_record_count(len(s), size, c.lib)
    out = np.zeros(n, abi.PRIM_DTYPE)
    got = C.c_uint32()
    _chk(c.lib.b32_star_records_batch(c.h, abi.ptr(s) if len(s) else None, len(s), float(size), abi.ptr(out) if n else None, n, C.byref(got)),
         "star_records_batch")
    return out[:int(got.value)]
