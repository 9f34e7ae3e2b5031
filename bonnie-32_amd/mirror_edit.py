"""Mirror editing (b32_scene_build_mirror): the Python side of the modeler's mirrored half built on the device into a derived slot.

    from bonnie32_amd import mirror_edit
    mirror_edit.build_mirror(dst, src, mirror_edit.Mirror("x", v_first, v_count, f_first, f_count))

`src` and `dst` are two rasterizer.ResidentScene of one context: src keeps the combined mesh (pose, patch, hover, box selection and the
overlays keep addressing it), dst is what the frame draws.  Mirror / pack_mirror (records.py) and the numpy mirror mirror_mesh / MeshMirror
(mirrors/rig.py) are re-exported here; this module imports neither the binding nor the library: a scene brings its context."""
import ctypes as C

from . import abi
from .mirrors.rig import MeshMirror, mirror_mesh  # noqa: F401
from .records import Mirror, _chk, pack_mirror  # noqa: F401


def mirror_counts(n_vertices, n_faces, mirror, lib=None):
    """b32_mirror_counts (host only): (vertices, faces) of the mesh build_mirror writes for a body of n_vertices / n_faces."""
    lib = lib or abi.load_library()
    m = pack_mirror(mirror)
    nv, nf = C.c_uint32(0), C.c_uint32(0)
    _chk(lib.b32_mirror_counts(int(n_vertices), int(n_faces), abi.ptr(m), C.byref(nv), C.byref(nf)), "mirror_counts")
    return int(nv.value), int(nf.value)


def build_mirror(dst, src, mirror):
    """b32_scene_build_mirror: enqueue one kernel that replaces dst's geometry with the mirror-editing mesh of src's body (two
    ResidentScene of one context, detached or not; a Mirror or an abi.MIRROR_DTYPE record).  dst's textures stay, its rig and tail go
    (dst.build_skeleton afterwards); src is read only.  No upload; the first build after src's upload synchronises once."""
    m = pack_mirror(mirror)
    ctx = dst.ctx
    _chk(ctx.lib.b32_scene_build_mirror(ctx.h, src._handle(), dst._handle(), abi.ptr(m)), "scene_build_mirror")
    dst.n_vertices, dst.n_faces = mirror_counts(src.n_body_vertices, src.n_body_faces, m, ctx.lib)
