"""One slot walked through every kind of writer in a row (csrc/b32_scene_state.h): pose, vertex patch, face patch, texel patch,
b32_scene_build_skeleton, b32_room_build_mesh and uploads of the same and of another face count.

What a writer forgets to invalidate shows one frame later and only on some routes: packed vertex streams that were not dropped draw the
old vertices on meshes above 8192 faces, a content number that was not renewed draws the old merged mesh in a batched frame.  So after
every step the slot is drawn on its own and as a member of a batched frame, and both frames are compared bit for bit -- pixels and depth
-- with the oracle's frames of the same content, which is what a fresh context given that content draws.  9000 triangles is the smallest
mesh of the suite above the 8192-face threshold of frame_positions; 300 triangles take the inline route."""
import copy
import functools

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi, scenegen
from bonnie32_amd import rasterizer as RM
from tests.test_room_mesh import real_mesh, real_room, real_scene
from tests.test_scene_patch import _bones, _nudged

W, H = 320, 240
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _scene(n_tris, seed=5):
    return scenegen.make_scene("C3", n_tris=n_tris, width=W, height=H, bbox_px=60.0, seed=seed, variant="gouraud")


def _tex_arrays(textures):
    return [np.asarray(t.pixels, np.uint16).reshape(t.height, t.width).copy() for t in textures]


def _textures(arrays, like):
    return [b32.Texture15(a.shape[1], a.shape[0], a.reshape(-1), t.blend_mode) for a, t in zip(arrays, like)]


def _skeleton():
    """Three bones in the middle of the C3 cloud; the selected one keeps editor_alpha, the others are dimmed to alpha 30: a blending tail."""
    bones = RM.pack_skel_bones([RM.SkelBone.from_rig((0.0, 0.0, 2500.0), (10.0, 0.0, -5.0), 900.0, 90.0, None),
                                RM.SkelBone.from_rig((600.0, -100.0, 2600.0), (0.0, 30.0, 40.0), 600.0, 0.0, 0),
                                RM.SkelBone.from_rig((-600.0, 200.0, 2700.0), (75.0, 0.0, 100.0), 700.0, 60.0, 0)])
    return bones, RM.SkeletonStyle(editor_alpha=220, selected_bone=1)


def _steps(n_tris):
    """The walk as (name, what to do to the slot, the slot's content afterwards as (vertices, faces, textures, camera))."""
    sc = _scene(n_tris)
    cam = sc.camera
    nv = len(sc.vertices)
    bo = (np.arange(nv) // 3 % 7).astype(np.uint16)
    A = _bones(2.0, 3000.0)
    rest, faces, tex = sc.vertices.copy(), sc.faces.copy(), _tex_arrays(sc.textures)
    T = lambda: _textures(tex, sc.textures)
    out = []

    def pose(rs):
        rs.set_rig(bo); rs.pose(A)
    out.append(("pose", pose, (RM.pose_vertices(rest, bo, A), faces, T(), cam)))

    idx = np.arange(1, nv, 7, dtype=np.uint32)
    new = _nudged(rest[idx], 1, 3000.0)
    rest = RM.patch_vertices(rest, idx, new)
    body = RM.pose_vertices(rest, bo, A)
    out.append(("vertex patch", lambda rs: rs.patch_vertices(idx, new), (body, faces, T(), cam)))

    opaque = np.nonzero((faces["blend_mode"] == abi.OPAQUE) & (faces["editor_alpha"] == 255))[0]
    one = opaque[len(opaque) // 2: len(opaque) // 2 + 40].astype(np.uint32)       # (forty faces in a row: some of them are in view)
    was = faces[one].copy()
    avg = was.copy(); avg["blend_mode"] = abi.AVERAGE
    blending = RM.patch_faces(faces, one, avg)
    out.append(("face patch: blending", lambda rs: rs.patch_faces(one, avg), (body, blending, T(), cam)))
    out.append(("face patch: opaque again", lambda rs: rs.patch_faces(one, was), (body, faces, T(), cam)))

    block = np.full((90, 120), 0x7C1F, np.uint16); block[::3] = 0x0000              # (magenta, with rows the black_transparent rule skips)
    tex[0] = RM.patch_texels(tex[0], 5, 9, block)
    out.append(("texel patch", lambda rs: rs.patch_texels(0, 5, 9, block), (body, faces, T(), cam)))

    skel = _skeleton()
    tv, tf = RM.skeleton_mesh(*skel, nv)
    assert len(tv) == 18 and int((tf["editor_alpha"] < 255).sum()) >= 8
    out.append(("skeleton", lambda rs: rs.build_skeleton(*skel), (np.concatenate([body, tv]), np.concatenate([faces, tf]), T(), cam)))

    room = real_room("dungeon")
    rv, rf = real_mesh("dungeon")
    room_cam = real_scene("dungeon-room0-game").camera
    out.append(("room mesh", room, (rv, rf, T(), room_cam)))

    k = len(rf)                                                                     # an upload of a mesh with the SAME face count ...
    big = _scene(9000)
    assert int(big.faces["v"][:k].max()) < 3 * k
    v2, f2 = _nudged(big.vertices[:3 * k], 2, 3000.0), big.faces[:k].copy()
    out.append(("upload, same face count", (v2, f2), (v2, f2, T(), cam)))
    v3 = _nudged(sc.vertices, 3, 3000.0)                                            # ... and of another one
    out.append(("upload, another face count", (v3, sc.faces), (v3, sc.faces, T(), cam)))
    return out


def _oracle(oracle, draws, cam, st):
    ofb = oracle.Framebuffer(W, H); ofb.clear(_scene(300).clear_color)
    for v, f, tex in draws:
        rc, _tm = oracle.render_mesh_15(ofb, v, f, tex, cam, st)
        assert rc == 0
    return ofb.pixels.copy(), ofb.zbuffer.view(np.uint32).copy()


def _assert_frame(fb, want, what):
    got, gz = fb.pixels, fb.zbuffer.view(np.uint32)
    assert np.array_equal(got, want[0]), f"{what}: {int((got != want[0]).sum())} bytes differ"
    assert np.array_equal(gz, want[1]), f"{what}: {int((gz != want[1]).sum())} depths differ"


@pytest.mark.gpu
@pytest.mark.parametrize("n_tris", [9000, 300], ids=["packed_streams", "inline"])
def test_one_slot_through_every_writer(oracle, n_tris):
    from bonnie32_amd import rasterizer as R
    sc, other = _scene(n_tris), _scene(300, seed=6)
    st = sc.settings                                                                # painter's mode, Gouraud, two lights: the lit stream is packed too
    st_z = copy.copy(st); st_z.use_zbuffer = True                                   # (a batched frame merges in z-buffer mode only)
    assert not st.use_zbuffer and st.use_rgb555 and len(st.lights) >= 1
    ctx = R.Context(0)
    room = None
    try:
        fb = R.Framebuffer(W, H, ctx)
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
        b = R.ResidentScene(fb, other.vertices, other.faces, other.textures).detach()
        seen = []

        def check(name, content):
            v, f, tex, cam = content
            fb.clear(sc.clear_color); rs.render_async(cam, st); rs.finish()
            want = _oracle(oracle, [(v, f, tex)], cam, st)
            _assert_frame(fb, want, name)
            merged = ctx.batch_counts()["merged_draws"]
            fb.clear(sc.clear_color); ctx.frame_submit(ctx.make_frame_table(cam, st_z, [b, rs])); ctx.finish()
            assert ctx.batch_counts()["merged_draws"] == merged + 1, name
            _assert_frame(fb, _oracle(oracle, [(other.vertices, other.faces, other.textures), (v, f, tex)], cam, st_z), name + ", batched")
            seen.append(want[0])

        first = (sc.vertices, sc.faces, sc.textures, sc.camera)
        check("first frame", first)
        check("second frame", first)                                               # (the streams are packed now)
        for name, action, content in _steps(n_tris):
            if callable(action):
                action(rs)
            elif name == "room mesh":
                room = R.Room(ctx, action[0], action[2])
                room.set_materials(action[1])
                room.build_mesh(rs)
                rs.n_vertices, rs.n_faces = len(content[0]), len(content[1])
            else:                                                                   # an upload into the slot: swapped in, replaced, swapped out
                rs._swap()
                R.ResidentScene(fb, action[0], action[1], content[2])
                rs._swap()
                rs.n_vertices, rs.n_faces = len(action[0]), len(action[1])
            check(name, content)
            assert not np.array_equal(seen[-1], seen[-2]), name + ": the step did not show"
        rs.close(); b.close()
    finally:
        if room is not None:
            room.close()
        ctx.close()
