"""Host-side mirror of the reference rasterizer interface, running on the MI355X through the C ABI: the ctypes binding.

Same names and argument meaning as the reference:
    Framebuffer::{new, resize, clear}       src/rasterizer/render.rs:18-45
    render_mesh_15(fb, vertices, faces, textures, camera, settings, fog) -> RasterTimings   render.rs:2302-2310
Errors the reference turns into panics come back as B32Error (index out of range, NaN sort key).

There is no CPU path here: if libb32raster.so or a HIP device is missing, construction raises.  What needs neither (records.py,
mirrors/) is re-exported here under its name.
"""
import ctypes as C

import numpy as np

from . import abi
from . import rtypes as T
from .records import (B32Error, Bone, MeshOverlay, ObjectItem, ObjectPart, Placement, RoomOverlay, SkelBone, SkeletonStyle, Topology,  # noqa: F401
                      _chk, _pack_ortho, _pack_placement, _pack_triple, floor_grid_items, gizmo_item, gizmo_record_count, noop_prims,
                      octahedron_items, pack_bones, pack_object_items, pack_skel_bones, place_vertices, prim, world_item)
from .mirrors.overlays import (OVERLAY_COLORS, ROOM_OVERLAY_COLORS, mesh_bounds, mesh_overlay_layout, mesh_overlay_record_count,  # noqa: F401
                               mesh_overlay_records, object_overlay_layout, object_overlay_record_count, object_overlay_records,
                               room_overlay_layout, room_overlay_record_count, room_overlay_records)
from .mirrors.query import HoverMirror, PickMirror, box_select_mesh, hover_mesh, hovered_element, pick_best, pick_mesh  # noqa: F401
from .mirrors.rig import (SkeletonMirror, bone_world_transforms, clut_lookup, kept_clut, patch_faces, patch_indexed, patch_indices,  # noqa: F401
                          patch_texels, patch_vertices, pose_vertices, rest_stream, rotate_by_euler, skeleton_items, skeleton_mesh)
from .mirrors.room import (RoomMirror, _room_grid, room_box_select, room_faces_from_sectors, room_hover, room_hover_winner,  # noqa: F401
                           room_materials_from_sectors, room_mesh, room_mesh_counts)
# Three private names that code written against the one-file layout reads from this module (`R._project_f32`, ...).  They live in mirrors/
# now: import them from there.  A name set here is not the one the mirrors read -- change a mirror's rule in its own module.
from .mirrors.overlays import _object_place  # noqa: F401
from .mirrors.room import _room_mesh_layout  # noqa: F401
from .mirrors.screen import _project_f32  # noqa: F401


def _cam(camera):
    """A camera as the library takes it: an rtypes.Camera packed, an abi.B32Camera as it is."""
    return camera.pack() if hasattr(camera, "pack") else camera


def _ref(struct):
    """An optional struct argument: its reference, or NULL."""
    return C.byref(struct) if struct is not None else None


def _item_args(h, items, dtype, camera, ortho):
    """What b32_draw_world, b32_draw_gizmos and their stage taps begin with.  Returns (the argument tuple: context, camera, ortho, items,
    count; the packed items array, which must stay alive while the tuple is in use)."""
    arr = np.ascontiguousarray(items, dtype=dtype).reshape(-1)
    cam = camera.pack()
    o = _pack_ortho(ortho)
    return (h, C.byref(cam), _ref(o), arr.ctypes.data if len(arr) else None, len(arr)), arr


def _tap(name, entry, args, width, height, n):
    """A stage tap's own tail behind the arguments of its draw_* twin: the frame size, room for n abi.PRIM_DTYPE records, how many came back."""
    out = np.zeros(n, abi.PRIM_DTYPE)
    got = C.c_uint32()
    _chk(entry(*args, width, height, abi.ptr(out) if n else None, n, C.byref(got)), name)
    return out[:int(got.value)]


class _OwnedResult:
    """What an async query delivers into `buf` once its ticket is done; close() frees page-locked memory of the result's own."""

    def __init__(self, buf, owner=None):
        self.buf, self._owner = buf, owner

    def close(self):
        if self._owner is not None:
            ctx, p = self._owner
            ctx.host_free(p)
            self._owner = None


class PickResult(_OwnedResult):
    """What b32_pick_meshes_async delivers into `buf` (16 + 16 * n bytes) once its ticket is done."""

    def __init__(self, buf, n, owner=None):
        self.buf, self.n, self._owner = buf, n, owner

    @property
    def best(self):
        return int(self.buf[:4].view(np.int32)[0])

    @property
    def hits(self):
        return self.buf[abi.PICK_HEADER_BYTES:abi.PICK_HEADER_BYTES + 16 * self.n].view(abi.PICK_HIT_DTYPE).copy()


class HoverResult(_OwnedResult):
    """What b32_hover_mesh_async delivers into `buf` (32 bytes) once its ticket is done."""

    @property
    def record(self):
        return self.buf[:32].view(abi.HOVER_RESULT_DTYPE)[0].copy()


class BoxResult(_OwnedResult):
    """What b32_box_select_async delivers into `buf` once its ticket is done: n_elements, n_selected and the words."""

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


class RoomHoverResult(_OwnedResult):
    """What b32_room_hover_async delivers into `buf` (48 bytes) once its ticket is done."""

    @property
    def record(self):
        return self.buf[:48].view(abi.ROOM_HOVER_DTYPE)[0].copy()


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


def _object_args(ctx, parts, items, camera):
    """The arguments b32_draw_object_overlays and its stage tap share, and the arrays they point into."""
    cam = camera.pack()
    pa, ia = pack_object_parts(parts, ctx), pack_object_items(items)
    return (ctx.h, C.byref(cam), abi.ptr(pa) if len(pa) else None, len(pa), abi.ptr(ia) if len(ia) else None, len(ia)), (pa, ia)


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
            _chk(self.lib.b32_frame_add_scene_placed(self.h, scene._slot, C.byref(p), _ref(pl)), "b32_frame_add_scene_placed")
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

    def _deliver(self, name, call, need, out, make_result):
        """The end every async query shares: call(pointer, ticket reference) delivers into `out` (an (array, pointer) pair from host_alloc
        of at least `need` bytes) or into page-locked memory of the result's own, freed at once when the call is refused: (ticket, result)."""
        own = out is None
        arr, ptr = self.host_alloc(need) if own else out
        if len(arr) < need:
            raise ValueError(name + ": the result buffer is too small")
        t = C.c_uint64()
        rc = call(ptr, C.byref(t))
        if rc != abi.B32_OK and own:
            self.host_free(ptr)
        _chk(rc, "b32_" + name)
        return int(t.value), make_result(arr, (self, ptr) if own else None)

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
            table[1][i] = _pack_triple(pl)

    def _pick_args(self, items, camera, mouse, ortho, cull_backfaces):
        slots, places, n = items if isinstance(items, tuple) else self.make_pick_table(items)
        cam = _cam(camera)
        o = _pack_ortho(ortho)
        return (self.h, C.byref(cam), _ref(o), float(mouse[0]), float(mouse[1]),
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
        return self._deliver("pick_meshes_async", lambda ptr, t: self.lib.b32_pick_meshes_async(*args, ptr, t), abi.PICK_HEADER_BYTES + 16 * n, out,
                             lambda arr, owner: PickResult(arr, n, owner))

    # ---- hover and box selection (b32_hover_mesh, b32_box_select): one detached ResidentScene and a Topology
    def _hover_args(self, scene, topology, camera, mouse, ortho, placement, see_through, mirror_axis, mirror_threshold, vertex_threshold, edge_threshold):
        prm = np.zeros(1, abi.HOVER_PARAMS_DTYPE)
        prm["mx"], prm["my"] = mouse
        prm["vertex_threshold"], prm["edge_threshold"] = vertex_threshold, edge_threshold
        prm["flags"] = abi.HOVER_SEE_THROUGH if see_through else 0
        prm["mirror_axis"], prm["mirror_threshold"] = mirror_axis, mirror_threshold
        return self._mesh_args(scene, topology, camera, ortho, placement) + (prm,)

    def _mesh_args(self, scene, topology, camera, ortho, placement):
        cam = _cam(camera)
        o = _pack_ortho(ortho)
        pl = _pack_triple(placement) if placement is not None else None         # a query always applies a placement it is given
        top = topology.handle(self) if topology is not None else None
        return (self.h, C.byref(cam), _ref(o), scene._slot, top, _ref(pl)), (cam, o, pl)

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
        p = {**dict(see_through=False, mirror_axis=0, mirror_threshold=1.0, vertex_threshold=abi.HOVER_VERTEX_THRESHOLD, edge_threshold=abi.HOVER_EDGE_THRESHOLD), **params}
        args, _keep, prm = self._hover_args(scene, topology, camera, mouse, ortho, placement, **p)
        return self._deliver("hover_mesh_async", lambda ptr, t: self.lib.b32_hover_mesh_async(*args, prm.ctypes.data, ptr, t), 32, out, HoverResult)

    def _box_args(self, scene, topology, camera, rect, mode, ortho, placement, n_elements):
        """(the arguments b32_box_select and its async twin share, what must stay alive, the element count)"""
        args, keep = self._mesh_args(scene, topology, camera, ortho, placement)
        prm = np.zeros(1, abi.BOX_PARAMS_DTYPE)
        prm["x0"], prm["y0"], prm["x1"], prm["y1"] = rect
        prm["mode"] = mode
        n = (topology.np if mode == abi.BOX_POLYGONS else scene.n_body_vertices) if n_elements is None else n_elements
        return args + (prm.ctypes.data,), (keep, prm), n

    def box_select(self, scene, topology, camera, rect, mode=abi.BOX_VERTICES, ortho=None, placement=None, n_elements=None):
        """b32_box_select: (words, n_selected) for the rectangle (x0, y0, x1, y1).  n_elements: the slot's vertex count in mode BOX_VERTICES
        (default: the uploaded scene's), the topology's polygon count in mode BOX_POLYGONS."""
        args, _keep, n = self._box_args(scene, topology, camera, rect, mode, ortho, placement, n_elements)
        words = np.zeros((n + 31) // 32, np.uint32)
        cnt = C.c_uint32()
        _chk(self.lib.b32_box_select(*args, words.ctypes.data if len(words) else None, C.byref(cnt)), "b32_box_select")
        return words, int(cnt.value)

    def box_select_async(self, scene, topology, camera, rect, mode=abi.BOX_VERTICES, ortho=None, placement=None, out=None, n_elements=None):
        """b32_box_select_async -> (ticket, BoxResult); out as for hover_mesh_async, of at least 16 + 4 * ceil(n_elements / 32) bytes."""
        args, _keep, n = self._box_args(scene, topology, camera, rect, mode, ortho, placement, n_elements)
        return self._deliver("box_select_async", lambda ptr, t: self.lib.b32_box_select_async(*args, ptr, t), abi.BOX_HEADER_BYTES + 4 * ((n + 31) // 32), out,
                             BoxResult)

    # ---- room hover and box selection (b32_room_hover, b32_room_box_select): one Room
    def _room_hover_args(self, room, camera, mouse, vertex_threshold, edge_threshold):
        cam = _cam(camera)
        prm = np.zeros(1, abi.ROOM_HOVER_PARAMS_DTYPE)
        prm["mx"], prm["my"] = mouse
        prm["vertex_threshold"], prm["edge_threshold"] = vertex_threshold, edge_threshold
        return (self.h, C.byref(cam), room._h, prm.ctypes.data), prm

    def room_hover(self, room, camera, mouse, vertex_threshold=abi.ROOM_VERTEX_THRESHOLD, edge_threshold=abi.ROOM_EDGE_THRESHOLD):
        """b32_room_hover: one abi.ROOM_HOVER_DTYPE record (all three loops, raw; room_hover_winner() is the reference's answer)."""
        args, _keep = self._room_hover_args(room, camera, mouse, vertex_threshold, edge_threshold)
        out = np.zeros(1, abi.ROOM_HOVER_DTYPE)
        _chk(self.lib.b32_room_hover(*args, out.ctypes.data), "b32_room_hover")
        return out[0]

    def room_hover_async(self, room, camera, mouse, vertex_threshold=abi.ROOM_VERTEX_THRESHOLD, edge_threshold=abi.ROOM_EDGE_THRESHOLD, out=None):
        """b32_room_hover_async -> (ticket, RoomHoverResult).  out: an (array, pointer) pair from host_alloc of at least 48 bytes; None:
        page-locked memory of the result's own, released by RoomHoverResult.close()."""
        args, _keep = self._room_hover_args(room, camera, mouse, vertex_threshold, edge_threshold)
        return self._deliver("room_hover_async", lambda ptr, t: self.lib.b32_room_hover_async(*args, ptr, t), 48, out, RoomHoverResult)

    def room_hover_winner(self, record):
        """b32_room_hover_winner of one abi.ROOM_HOVER_DTYPE record."""
        rec = np.ascontiguousarray(record, abi.ROOM_HOVER_DTYPE).reshape(1)
        return int(self.lib.b32_room_hover_winner(rec.ctypes.data))

    def _room_box_args(self, room, camera, rect, points):
        """(the arguments b32_room_box_select and its async twin share, the points array, the element count)"""
        cam = _cam(camera)
        pts = np.zeros((0, 3), np.float32) if points is None else np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        return (self.h, C.byref(cam), room._h, *[float(v) for v in rect], pts.ctypes.data if len(pts) else None, len(pts)), pts, room.n + len(pts)

    def room_box_select(self, room, camera, rect, points=None):
        """b32_room_box_select: (words, n_selected) for the rectangle (x0, y0, x1, y1); element i is record i, then point i - n."""
        args, _keep, n = self._room_box_args(room, camera, rect, points)
        words = np.zeros((n + 31) // 32, np.uint32)
        cnt = C.c_uint32()
        _chk(self.lib.b32_room_box_select(*args, words.ctypes.data if len(words) else None, C.byref(cnt)), "b32_room_box_select")
        return words, int(cnt.value)

    def room_box_select_async(self, room, camera, rect, points=None, out=None):
        """b32_room_box_select_async -> (ticket, BoxResult); out as for room_hover_async, of at least 16 + 4 * ceil(n_elements / 32) bytes."""
        args, _keep, n = self._room_box_args(room, camera, rect, points)
        return self._deliver("room_box_select_async", lambda ptr, t: self.lib.b32_room_box_select_async(*args, ptr, t),
                             abi.BOX_HEADER_BYTES + 4 * ((n + 31) // 32), out, BoxResult)

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
        args, arr = _item_args(self.h, items, abi.GIZMO_ITEM_DTYPE, camera, ortho)
        # (a thickness beyond the cap is refused before anything is written)
        cap = int(sum(gizmo_record_count(int(k), min(int(s), abi.GIZMO_MAX_THICKNESS)) for k, s in zip(arr["kind"], arr["size"])))
        return _tap("gizmo_project_batch", self.lib.b32_gizmo_project_batch, args, int(width), int(height), cap)

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
        args, _keep = _item_args(self.ctx.h, items, abi.WORLD_ITEM_DTYPE, camera, ortho)
        _chk(self.ctx.lib.b32_draw_world(*args), "draw_world")

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

    def _counts(self, name):
        """(drawn, dropped, rejected) of b32_<name>"""
        v = [C.c_uint64() for _ in range(3)]
        _chk(getattr(self.ctx.lib, "b32_" + name)(self.ctx.h, *[C.byref(x) for x in v]), name)
        return tuple(int(x.value) for x in v)

    def world_counts(self):
        """b32_world_counts: (drawn, dropped, rejected) items this context has projected so far; synchronises."""
        return self._counts("world_counts")

    def world_project_batch(self, items, camera: T.Camera, ortho=None, width=None, height=None):
        """b32_world_project_batch (stage tap): the abi.PRIM_DTYPE records b32_draw_world hands to the tile pass."""
        args, arr = _item_args(self.ctx.h, items, abi.WORLD_ITEM_DTYPE, camera, ortho)
        out = np.zeros(len(arr), abi.PRIM_DTYPE)                 # one record per item: this tap takes no room and reports no count
        _chk(self.ctx.lib.b32_world_project_batch(*args, width or self.width, height or self.height, out.ctypes.data if len(arr) else None),
             "world_project_batch")
        return out

    # ---- the world editor's clipped lines and filled gizmos (editor/viewport_3d.rs:5687-6357): projected on the device, b32_draw_gizmos
    def draw_gizmos(self, items, camera: T.Camera, ortho=None):
        """b32_draw_gizmos: every item of `items` (abi.GIZMO_ITEM_DTYPE) drawn as the editor's helper calls in array order; enqueued, no
        host synchronisation.  ortho: None or (zoom, center_x, center_y), read by GIZMO_TRIANGLE_VIEW only."""
        args, _keep = _item_args(self.ctx.h, items, abi.GIZMO_ITEM_DTYPE, camera, ortho)
        _chk(self.ctx.lib.b32_draw_gizmos(*args), "draw_gizmos")

    def gizmo_batch(self):
        """A GizmoBatch on this framebuffer: the editor's helper calls recorded; flush(camera, ortho) draws them with one b32_draw_gizmos call."""
        return GizmoBatch(self)

    def gizmo_counts(self):
        """b32_gizmo_counts: (drawn, dropped, rejected) gizmo items this context has projected so far; synchronises."""
        return self._counts("gizmo_counts")

    # ---- the modeler's selection overlays from a slot's resident vertices (modeler/viewport.rs:1782-2247): b32_draw_mesh_overlay
    def _overlay_args(self, scene, topology, overlay, camera, ortho, selected):
        cam = camera.pack()
        o = _pack_ortho(ortho)
        ov, sel = overlay.pack(selected)
        top = topology.handle(self.ctx) if topology is not None else None
        return (self.ctx.h, C.byref(cam), _ref(o), scene._slot, top, C.byref(ov), abi.ptr(sel) if len(sel) else None), (cam, o, ov, sel)

    def draw_mesh_overlay(self, scene, topology, overlay, camera: T.Camera, ortho=None, selected=None):
        """b32_draw_mesh_overlay: the sections of `overlay` (a MeshOverlay) made into records on the device from the vertices of `scene` (a
        detached ResidentScene, posed or not) and drawn in the reference's order; enqueued, no host synchronisation, nothing read back."""
        args, _keep = self._overlay_args(scene, topology, overlay, camera, ortho, selected)
        _chk(self.ctx.lib.b32_draw_mesh_overlay(*args), "draw_mesh_overlay")

    def mesh_overlay_project_batch(self, scene, topology, overlay, camera: T.Camera, ortho=None, selected=None, width=None, height=None):
        """b32_mesh_overlay_project_batch (stage tap): the abi.PRIM_DTYPE records b32_draw_mesh_overlay hands to the tile pass."""
        n = mesh_overlay_record_count(topology, scene.n_body_vertices, overlay, selected)
        args, _keep = self._overlay_args(scene, topology, overlay, camera, ortho, selected)
        return _tap("mesh_overlay_project_batch", self.ctx.lib.b32_mesh_overlay_project_batch, args, width or self.width, height or self.height, n)

    # ---- the world editor's room overlays from a resident room (editor/viewport_3d.rs:4273-4658, :4862-5362): b32_draw_room_overlay
    def _room_overlay_args(self, room, overlay, camera):
        cam = camera.pack()
        o, lists = overlay.pack()
        return (self.ctx.h, C.byref(cam), room._h, C.byref(o), *lists), (cam, o)

    def draw_room_overlay(self, room, overlay, camera: T.Camera):
        """b32_draw_room_overlay: the sections of `overlay` (a RoomOverlay) made into records on the device from the records of `room` (a
        Room) as they are there -- and, with hover_source = abi.ROOM_OVERLAY_HOVER_RESIDENT, from its last hover without waiting for it --
        and drawn in the reference's order; enqueued, no host synchronisation, nothing read back."""
        args, _keep = self._room_overlay_args(room, overlay, camera)
        _chk(self.ctx.lib.b32_draw_room_overlay(*args), "draw_room_overlay")

    def room_overlay_project_batch(self, room, overlay, camera: T.Camera, width=None, height=None):
        """b32_room_overlay_project_batch (stage tap): the abi.PRIM_DTYPE records b32_draw_room_overlay hands to the tile pass."""
        n = room_overlay_record_count(room.n, overlay)
        args, _keep = self._room_overlay_args(room, overlay, camera)
        return _tap("room_overlay_project_batch", self.ctx.lib.b32_room_overlay_project_batch, args, width or self.width, height or self.height, n)

    # ---- the world editor's object overlays from resident asset parts (viewport_3d.rs:255-291, :7658-7697; asset.rs:288-312)
    def draw_object_overlays(self, parts, items, camera: T.Camera):
        """b32_draw_object_overlays: the wireframes and bounding boxes of `items` (ObjectItem) over the asset parts `parts` (ObjectPart with
        detached scenes) made into records on the device and drawn in array order; enqueued, no host synchronisation, nothing read back."""
        args, _keep = _object_args(self.ctx, parts, items, camera)
        _chk(self.ctx.lib.b32_draw_object_overlays(*args), "draw_object_overlays")

    def object_overlay_project_batch(self, parts, items, camera: T.Camera, width=None, height=None):
        """b32_object_overlay_project_batch (stage tap): the abi.PRIM_DTYPE records b32_draw_object_overlays hands to the tile pass."""
        n = self.ctx.object_overlay_record_count(parts, items)
        args, _keep = _object_args(self.ctx, parts, items, camera)
        return _tap("object_overlay_project_batch", self.ctx.lib.b32_object_overlay_project_batch, args, width or self.width, height or self.height, n)

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
    """(vertices, faces as contiguous ABI arrays, the four arguments they are passed as: pointer or NULL and count of each)"""
    v = np.ascontiguousarray(vertices, dtype=abi.VERTEX_DTYPE)
    f = np.ascontiguousarray(faces, dtype=abi.FACE_DTYPE)
    return v, f, (v.ctypes.data if len(v) else None, len(v), f.ctypes.data if len(f) else None, len(f))


def render_mesh_15(fb: Framebuffer, vertices, faces, textures, camera: T.Camera, settings: T.RasterSettings,
                   fog=None) -> T.RasterTimings:
    """render_mesh_15 (render.rs:2302-2310): host slices in, draws into the device framebuffer."""
    v, f, geom = _geom(vertices, faces)
    tex_arr, _keep = T.pack_textures(textures)
    cam = camera.pack()
    st, _kl = settings.pack()
    fg = T.pack_fog(fog)
    tm = abi.B32Timings()
    rc = fb.ctx.lib.b32_render_mesh_15(fb.ctx.h, *geom, C.cast(tex_arr, C.c_void_p), len(textures), C.byref(cam), C.byref(st), _ref(fg), C.byref(tm))
    _chk(rc, "render_mesh_15")
    return T.RasterTimings.from_c(tm)


def render_mesh(fb: Framebuffer, vertices, faces, textures, camera: T.Camera, settings: T.RasterSettings) -> T.RasterTimings:
    """render_mesh (render.rs:1971-1978), the 8-bit-colour path every caller takes when `settings.use_rgb555` is false
    (scene.rs:163-169).  `textures` are rtypes.Texture (Color texels with per-texel blend modes)."""
    v, f, geom = _geom(vertices, faces)
    tex_arr, _keep = T.pack_textures8(textures)
    cam = camera.pack()
    st, _kl = settings.pack()
    tm = abi.B32Timings()
    rc = fb.ctx.lib.b32_render_mesh(fb.ctx.h, *geom, C.cast(tex_arr, C.c_void_p), len(textures), C.byref(cam), C.byref(st), C.byref(tm))
    _chk(rc, "render_mesh")
    return T.RasterTimings.from_c(tm)


# aliases named in BASELINE.json's north_star (the reference's real entry point is render_mesh_15)
draw_mesh = render_mesh_15


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
        v, f, geom = _geom(vertices, faces)
        self.fmt8 = textures8 is not None
        if textures8 is not None:                       # the 8-bit-colour path (render_mesh)
            arr, keep = T.pack_textures8(textures8)
            rc = self.ctx.lib.b32_scene_upload_rgba(self.ctx.h, *geom, C.cast(arr, C.c_void_p), len(textures8))
        elif indexed_textures is not None:
            arr, keep = T.pack_indexed_textures(indexed_textures)
            rc = self.ctx.lib.b32_scene_upload_indexed(self.ctx.h, *geom, C.cast(arr, C.c_void_p), len(indexed_textures))
        else:
            textures = textures or []
            arr, keep = T.pack_textures(textures)
            rc = self.ctx.lib.b32_scene_upload(self.ctx.h, *geom, C.cast(arr, C.c_void_p), len(textures))
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
                _chk(self.ctx.lib.b32_render_scene_15(self.ctx.h, C.byref(cam), C.byref(st), _ref(fg), C.byref(tm)), "render_scene_15")
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
