"""Mirror editing: the modeler's mirrored half built on the device into a derived slot (b32_scene_build_mirror).

Without a GPU: a literal restatement of modeler/viewport.rs:1156-1311 over a list of objects with one selected, the numpy mirror
(mirror_edit.mirror_mesh) and csrc/b32_mirror_body.h built for the host (tests/cpp/mirror_host.cpp) agree vertex for vertex and face for
face on named cases; the order case on the oracle; one-point mutations of the mirror, each of which must move a named case; the host
program under the sanitizers.
On the GPU: the derived slot's bits, frames against the oracle's render of the mirror-built arrays, and the contract: the chain of
edits, the transparent-pass bookkeeping, the skeleton behind a build, the source unchanged, a two-slot frame, drag frames without a host
wait, the error table.  Every comparison is bit for bit."""
import atexit
import copy
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi
from bonnie32_amd import mirror_edit as ME       # (imports neither the binding nor the library)
from bonnie32_amd import rasterizer as RM          # (imports no device code: the host mirrors live there)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden", "scenes", "real")
f32 = np.float32
NONE = abi.BONE_NONE
M = ME.Mirror


def _same_mesh(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ================================================================== the literal restatement (scalar f32, the Rust text line by line)
def _rust_as_u8(x):
    """`x as u8` for an f32: saturating, NaN -> 0"""
    if np.isnan(x) or x <= 0:
        return 0
    return 255 if x >= 255 else int(x)


def _lit_rotate(v, bone):
    """rotate_by_euler (state.rs:30-54) with the bone's cos / sin taken on the host (B32Bone)"""
    x, y, z = v
    if not bone["rotate"]:
        return (x, y, z)
    cx, sx, cz, sz = bone["cos_x"], bone["sin_x"], bone["cos_z"], bone["sin_z"]
    y1 = y * cx + z * sx
    z1 = (-y) * sx + z * cx
    x2 = x * cz + y1 * sz
    y2 = (-x) * sz + y1 * cz
    return (x2, y2, z1)


def _lit_mirror(v, axis):
    """mirror_position / mirror_normal (state.rs:832-848): Vec3::new(-pos.x, pos.y, pos.z) for Axis::X, ..."""
    x, y, z = v
    return (-x, y, z) if axis == 1 else ((x, -y, z) if axis == 2 else (x, y, -z))


class Obj:
    """One modeler object: its local vertices (abi.VERTEX_DTYPE: pos, normal, uv; the colour column is the object's base_color per
    vertex), a bone index per vertex (None: none) with the object's default, and its triangles (abi.FACE_DTYPE with LOCAL indices)."""

    def __init__(self, vertices, faces, bone=None, default_bone=None):
        self.v = np.asarray(vertices, abi.VERTEX_DTYPE).reshape(-1)
        self.f = np.asarray(faces, abi.FACE_DTYPE).reshape(-1)
        self.bone = list(bone) if bone is not None else [None] * len(self.v)
        self.default_bone = default_bone


def literal_mesh(objects, selected, axis, bones, dim=0.85):
    """viewport.rs:1156-1311: the combined mesh; axis None: mirror mode off.  bones: abi.BONE_DTYPE records (bone_transforms)."""
    all_vertices, all_faces = [], []
    u32 = lambda x: int(x) & 0xFFFFFFFF

    def skinned(pos, normal, bone_idx):
        bt = bones[bone_idx] if bone_idx is not None and bone_idx < len(bones) else None
        if bt is not None:
            rotated = _lit_rotate(pos, bt)
            world_pos = tuple(rotated[k] + bt["pos"][k] for k in range(3))
            return world_pos, _lit_rotate(normal, bt)
        return pos, normal

    with np.errstate(all="ignore"):
        for obj_idx, obj in enumerate(objects):
            vertex_offset = len(all_vertices)
            for k, v in enumerate(obj.v):
                bone_idx = obj.bone[k] if obj.bone[k] is not None else obj.default_bone
                pos, normal = skinned(tuple(v["pos"]), tuple(v["normal"]), bone_idx)
                all_vertices.append((pos, normal, v["uv"].copy(), (v["r"], v["g"], v["b"], v["blend"])))
            mirror_vertex_offset = None
            if axis is not None and selected == obj_idx:
                mirror_vertex_offset = len(all_vertices)
                for k, v in enumerate(obj.v):
                    mirrored_pos = _lit_mirror(tuple(v["pos"]), axis)
                    mirrored_normal = _lit_mirror(tuple(v["normal"]), axis)
                    bone_idx = obj.bone[k] if obj.bone[k] is not None else obj.default_bone
                    pos, normal = skinned(mirrored_pos, mirrored_normal, bone_idx)
                    colour = tuple(_rust_as_u8(f32(ch) * f32(dim)) for ch in (v["r"], v["g"], v["b"])) + (abi.OPAQUE,)       # RasterColor::new
                    all_vertices.append((pos, normal, v["uv"].copy(), colour))
            for face in obj.f:
                v0, v1, v2 = (int(i) for i in face["v"])
                rest = (face["texture_id"], face["black_transparent"], face["blend_mode"], face["editor_alpha"], face["_pad"])
                all_faces.append(((u32(vertex_offset + v0), u32(vertex_offset + v1), u32(vertex_offset + v2)),) + rest)
                if mirror_vertex_offset is not None:
                    all_faces.append(((u32(mirror_vertex_offset + v0), u32(mirror_vertex_offset + v2), u32(mirror_vertex_offset + v1)),) + rest)
    v = np.zeros(len(all_vertices), abi.VERTEX_DTYPE); f = np.zeros(len(all_faces), abi.FACE_DTYPE)
    for k, (p, n, uv, c) in enumerate(all_vertices):
        v[k]["pos"], v[k]["normal"], v[k]["uv"] = p, n, uv
        v[k]["r"], v[k]["g"], v[k]["b"], v[k]["blend"] = c
    for k, (idx, tex, bt, bm, ea, pad) in enumerate(all_faces):
        f[k]["v"], f[k]["texture_id"], f[k]["black_transparent"], f[k]["blend_mode"], f[k]["editor_alpha"], f[k]["_pad"] = idx, tex, bt, bm, ea, pad
    return v, f


def source_of(objects, selected, bones, rigged=True):
    """What the host keeps resident for these objects: the combined body (posed), its rest stream, the resolved bone index per vertex,
    and the selected object's ranges as a Mirror's four numbers."""
    body_v, body_f = literal_mesh(objects, selected, None, bones if rigged else [])
    local = np.concatenate([o.v for o in objects]) if objects else np.zeros(0, abi.VERTEX_DTYPE)
    bone_of = np.array([NONE if (b if b is not None else o.default_bone) is None else (b if b is not None else o.default_bone) for o in objects for b in o.bone], np.uint16)
    v_first = sum(len(o.v) for o in objects[:selected]); f_first = sum(len(o.f) for o in objects[:selected])
    rng = (v_first, len(objects[selected].v), f_first, len(objects[selected].f)) if objects else (0, 0, 0, 0)
    return body_v, body_f, (RM.rest_stream(local) if rigged else None), (bone_of if rigged else None), rng


# ================================================================== the host build of the device header
HOST_FLAGS = {"off": ["-O1", "-ffp-contract=off"], "san": ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@functools.lru_cache(maxsize=None)
def _host_dir():
    d = tempfile.mkdtemp(prefix="b32_mirror_host_")
    atexit.register(shutil.rmtree, d, True)
    return d


@functools.lru_cache(maxsize=None)
def _host_exe(mode):
    exe = os.path.join(_host_dir(), "mirror_host_" + mode)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + HOST_FLAGS[mode] + ["-I", os.path.join(ROOT, "bonnie-32_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "mirror_host.cpp"), "-o", exe], check=True)
    return exe


def host_mesh(vertices, faces, mirror, rest=None, bone_of=None, bones=None, mode="off"):
    """(rc, vertices, faces) from csrc/b32_mirror_body.h compiled for the host"""
    d = _host_dir()
    src, dst = os.path.join(d, "in_" + mode), os.path.join(d, "out_" + mode)
    v = np.ascontiguousarray(vertices, abi.VERTEX_DTYPE).reshape(-1); f = np.ascontiguousarray(faces, abi.FACE_DTYPE).reshape(-1)
    tab = RM.pack_bones(bones if bones is not None else [])
    blob = np.array([len(v), len(f), 0 if rest is None else 1, len(tab) if rest is not None else 0], np.uint32).tobytes() + ME.pack_mirror(mirror).tobytes()
    blob += v.tobytes() + f.tobytes()
    if rest is not None:
        bo = np.ascontiguousarray(bone_of, np.uint16).tobytes()
        blob += np.ascontiguousarray(rest, f32).tobytes() + bo + b"\0" * (-len(bo) % 4) + tab.tobytes()
    with open(src, "wb") as fh:
        fh.write(blob)
    subprocess.run([_host_exe(mode), src, dst], check=True)
    out = open(dst, "rb").read()
    rc = int(np.frombuffer(out[:4], np.int32)[0])
    if rc:
        return rc, None, None
    nv, nf = (int(x) for x in np.frombuffer(out[4:12], np.uint32))
    return 0, np.frombuffer(out, abi.VERTEX_DTYPE, nv, 12), np.frombuffer(out, abi.FACE_DTYPE, nf, 12 + 36 * nv)


# ================================================================== the cases
def _obj(seed, nv, nf, n_bones=5, colour=180, tex=0, specials=False):
    rng = np.random.default_rng(seed)
    v = np.zeros(nv, abi.VERTEX_DTYPE)
    v["pos"] = rng.standard_normal((nv, 3)).astype(f32) * f32(50.0)
    n = rng.standard_normal((nv, 3)).astype(f32)
    v["normal"] = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-6)
    v["uv"] = rng.random((nv, 2)).astype(f32)
    v["r"] = v["g"] = v["b"] = colour
    if specials and nv >= 8:
        sp = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFA00001, 0x00000001, 0x80000001], np.uint32).view(f32)
        for k in range(8):
            v["pos"][k, k % 3] = sp[k]; v["normal"][k, (k + 1) % 3] = sp[(k + 3) % 8]
    f = b32.make_faces(nf, tex)
    if nv:
        f["v"] = rng.integers(0, nv, (nf, 3))
    f["black_transparent"] = rng.integers(0, 2, nf); f["blend_mode"] = rng.integers(0, 6, nf); f["editor_alpha"] = rng.choice([255, 100, 0], nf)
    bone = [None if r < 0.15 else int(rng.integers(0, n_bones + 2)) for r in rng.random(nv)]      # (some indices lie past the table)
    if specials and nv >= 8:                    # a NaN that meets another NaN in a rotation has the machine's bits: the specials keep to
        bone[:8] = [None, 1, 4, 6, None, 1, 4, 63]      # no bone, a bone past the table and the two bones that only translate
    return Obj(v, f, bone, default_bone=int(seed) % n_bones if seed % 2 else None)


def _bones(t=1.0):
    """rotating bones, two that take rotate_by_euler's early return, one that only translates by zero"""
    return RM.pack_bones([RM.Bone.from_euler((3.0 * t, 1.0, -2.0), (6.0 + 3.0 * t, 0.0, -5.0 + 2.0 * t)), RM.Bone.from_euler((0.35, -0.05, 0.02 * t), (0.0004, 30.0, 0.0)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (-4.0 - 1.5 * t, 0.0, 3.0 + t)), RM.Bone.from_euler((-7.0, 2.0 * t, 5.0), (75.0, 0.0, 100.0)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))])


@functools.lru_cache(maxsize=None)
def object_cases():
    """name -> (objects, selected, bones, rigged)"""
    three = [_obj(1, 9, 7), _obj(2, 14, 11, specials=True), _obj(3, 5, 6)]
    c = {}
    for k, name in enumerate(("first", "middle", "last")):
        c["three_" + name] = (three, k, _bones(), True)
    c["one_object"] = ([_obj(4, 12, 9, specials=True)], 0, _bones(2.0), True)
    c["unrigged_specials"] = ([_obj(5, 6, 4), _obj(6, 16, 9, specials=True)], 1, [], False)
    c["no_pose_yet"] = (three, 1, [], True)                                     # (also: pose with n_bones = 0)
    c["no_vertices_no_faces"] = ([_obj(7, 4, 3), Obj(np.zeros(0, abi.VERTEX_DTYPE), b32.make_faces(0)), _obj(8, 3, 2)], 1, _bones(), True)
    c["no_faces"] = ([_obj(9, 4, 3), Obj(_obj(10, 5, 0).v, b32.make_faces(0)), _obj(11, 3, 2)], 1, _bones(), True)
    c["empty_mesh"] = ([Obj(np.zeros(0, abi.VERTEX_DTYPE), b32.make_faces(0))], 0, _bones(), True)
    c["early_return_bones"] = ([Obj(_obj(12, 10, 6, specials=True).v, _obj(12, 10, 6).f, [1, 4] * 5)], 0, _bones(), True)
    c["bone_none_and_past"] = ([Obj(_obj(13, 10, 6, specials=True).v, _obj(13, 10, 6).f, [None, 5, 63, 0xFFFE, None, 5, 63, 0xFFFE, 0, 0])], 0, _bones(), True)
    return c


def _three_way(objects, selected, bones, rigged, axis, dim=0.85):
    bv, bf, rest, bo, (v0, vc, f0, fc) = source_of(objects, selected, bones, rigged)
    m = M(axis, v0, vc, f0, fc, dim)
    lit = literal_mesh(objects, selected, axis, bones if rigged else [], dim)
    mir = ME.mirror_mesh(bv, bf, m, rest, bo, bones if rigged else None)
    rc, hv, hf = host_mesh(bv, bf, m, rest, bo, bones if rigged else None)
    assert rc == 0
    return lit, mir, (hv, hf), (bv, bf, rest, bo, m)


def test_restatement_mirror_and_header_agree_on_the_object_cases():
    """Three texts, every named case, axes X, Y and Z: vertex for vertex, face for face, bit for bit."""
    for name, (objects, selected, bones, rigged) in object_cases().items():
        for axis in (1, 2, 3):
            lit, mir, hdr, (bv, bf, _, _, m) = _three_way(objects, selected, bones, rigged, axis)
            assert _same_mesh(lit, mir), (name, axis)
            assert _same_mesh(hdr, mir), (name, axis)
            assert len(mir[0]) == len(bv) + m.v_count and len(mir[1]) == len(bf) + m.f_count
    # the cases are what their names say
    lit, mir, _, (bv, bf, rest, bo, m) = _three_way(*object_cases()["three_middle"], 1)
    assert (m.v_first, m.v_count, m.f_first, m.f_count) == (9, 14, 7, 11)
    tw, src = mir[0][23:37], bv[9:23]
    assert mir[0][:23].tobytes() == bv[:23].tobytes() and mir[0][37:].tobytes() == bv[23:].tobytes()
    assert (tw["r"] == 153).all() and (src["r"] == 180).all() and tw["uv"].tobytes() == src["uv"].tobytes()
    assert np.array_equal(mir[1]["v"][7:29:2], bf["v"][7:18]) and np.array_equal(mir[1]["v"][8:29:2], bf["v"][7:18][:, [0, 2, 1]] + 14)
    assert np.array_equal(mir[1]["v"][29:], bf["v"][18:] + 14) and np.array_equal(mir[1]["v"][:7], bf["v"][:7])
    # the specials: a zero's sign flips, a NaN keeps its payload (unrigged: the twin's bits are the source's with one sign bit flipped)
    _, mir, _, (bv, _, _, _, m) = _three_way(*object_cases()["unrigged_specials"], 1)
    sb, tb = bv["pos"][m.v_first:m.v_first + 8].view(np.uint32), mir[0]["pos"][m.v_first + m.v_count:][:8].view(np.uint32)
    assert np.array_equal(tb[:, 0], sb[:, 0] ^ 0x80000000) and np.array_equal(tb[:, 1:], sb[:, 1:])
    assert {0x00000000, 0x80000000, 0x7FC12345, 0x7F800000} <= set(int(x) for x in sb[:, 0]) | set(int(x) for x in sb.reshape(-1))
    # before the first pose the twins are the mirrored rest bits
    _, mir, _, (bv, _, rest, _, m) = _three_way(*object_cases()["no_pose_yet"], 3)
    tw = mir[0][m.v_first + m.v_count:][:m.v_count]
    r = rest[m.v_first:m.v_first + m.v_count].view(np.uint32).copy(); r[:, 2] ^= 0x80000000; r[:, 5] ^= 0x80000000
    assert np.array_equal(tw["pos"].view(np.uint32), r[:, :3]) and np.array_equal(tw["normal"].view(np.uint32), r[:, 3:])
    # an early-return bone with position zero turns a twin's -0.0 into +0.0 (x + 0.0), a missing bone does not
    objs, sel, bones, _ = object_cases()["early_return_bones"]
    assert not bones[4]["rotate"] and not bones[1]["rotate"] and bones[0]["rotate"]


def _generic(nv=40, nf=30, seed=20):
    o = _obj(seed, nv, nf, specials=True)
    return o.v.copy(), o.f.copy()


def test_mirror_and_header_agree_on_records_the_modeler_never_builds():
    """Mirror == header on arrays the rule must not look into, and the named values against their scalar restatement: all 256 channel
    values under dim 0.85 and under dim in {0, 1, 2, -1, inf, NaN}; indices >= nv and near 2^32 (the wrap); B32_NO_TEXTURE; every flag
    byte; a source vertex whose blend byte is set."""
    v, f = _generic(256, 256)
    v["r"], v["g"], v["b"] = np.arange(256), np.arange(256)[::-1], (np.arange(256) * 7) % 256
    v["blend"] = np.arange(256) % 6
    f["v"][:8] = [(0xFFFFFFFF, 0, 1), (0xFFFFFF00, 0xFFFFFFFE, 256), (300, 400, 500), (255, 256, 257), (0x80000000, 0x7FFFFFFF, 5), (1, 2, 3), (0, 0, 0), (9, 9, 0xFFFFFFF0)]
    f["texture_id"][::3] = abi.NO_TEXTURE; f["texture_id"][1::3] = 0xFFFFFFFE
    f["black_transparent"], f["blend_mode"], f["editor_alpha"], f["_pad"] = np.arange(256), np.arange(256)[::-1], (np.arange(256) * 3) % 256, (np.arange(256) * 5) % 256
    with np.errstate(all="ignore"):
        for dim in (0.85, 0.0, 1.0, 2.0, -1.0, np.inf, np.nan):
            m = M(2, 0, 256, 0, 256, dim)
            mv, mf = ME.mirror_mesh(v, f, m)
            rc, hv, hf = host_mesh(v, f, m)
            assert rc == 0 and _same_mesh((hv, hf), (mv, mf)), dim
            tw = mv[256:]
            for ch in ("r", "g", "b"):
                assert tw[ch].tolist() == [_rust_as_u8(f32(int(x)) * f32(dim)) for x in v[ch]], (dim, ch)
            assert (tw["blend"] == abi.OPAQUE).all() and mv[:256].tobytes() == v.tobytes()
            if dim == 0.85:
                assert (tw["r"][180], tw["r"][255], tw["r"][1]) == (153, 216, 0)
            if dim == 2.0:
                assert tw["r"][127] == 254 and tw["r"][128] == 255 and tw["r"][255] == 255
            if dim in (0.0, -1.0) or dim != dim:
                assert not tw["r"].any()
            if dim == np.inf:
                assert tw["r"][0] == 0 and (tw["r"][1:] == 255).all()          # 0 * inf is a NaN
    # the wrap, the copied bytes
    tv = mf["v"][1::2]
    assert tv[0].tolist() == [0xFF, 257, 256] and tv[1].tolist() == [0, 512, 0xFE] and tv[4].tolist() == [0x80000100, 261, 0x800000FF]
    for col in ("texture_id", "black_transparent", "blend_mode", "editor_alpha", "_pad"):
        assert np.array_equal(mf[col][0::2], f[col]) and np.array_equal(mf[col][1::2], f[col])
    # a partial range in the middle: later faces shift by the wrapping add, earlier ones do not
    m = M(1, 100, 50, 3, 4)
    mv, mf = ME.mirror_mesh(v, f, m)
    rc, hv, hf = host_mesh(v, f, m)
    assert rc == 0 and _same_mesh((hv, hf), (mv, mf))
    assert mf["v"][0].tolist() == [0xFFFFFFFF, 0, 1] and mf["v"][11].tolist() == [9 + 50, 9 + 50, (0xFFFFFFF0 + 50) & 0xFFFFFFFF]
    # the argument rules, as the library's host-only entry and the header have them
    lib = abi.load_library()
    nvo, nfo = C.c_uint32(), C.c_uint32()
    E, U = abi.B32_E_ARG, abi.B32_E_UNSUPPORTED
    for nv, nf, mm, want in ((5, 5, M(1, 2, 3, 1, 4), 0), (5, 5, M(0, 0, 0, 0, 0), E), (5, 5, M(4, 0, 0, 0, 0), E), (5, 5, M(1, 2, 4, 0, 0), E), (5, 5, M(1, 0, 0, 5, 1), E),
                             (0xFFFFFFFF, 0, M(1, 0, 1, 0, 0), U), (0, 0xFFFFFFFF, M(1, 0, 0, 7, 1), U), (0x80000000, 0x80000000, M(3, 1, 0x7FFFFFFF, 0, 0x7FFFFFFF), 0),
                             (0, 0, M(3, 0, 0, 0, 0), 0)):
        p = mm.pack()
        assert lib.b32_mirror_counts(nv, nf, abi.ptr(p), C.byref(nvo), C.byref(nfo)) == want, (nv, nf, vars(mm))
        if want == 0:
            assert (nvo.value, nfo.value) == (nv + mm.v_count, nf + mm.f_count)
    assert lib.b32_mirror_counts(5, 5, None, C.byref(nvo), C.byref(nfo)) == E
    assert host_mesh(v[:5], f[:5], M(1, 2, 4, 0, 0))[0] == E and host_mesh(v[:5], f[:5], M(7, 0, 0, 0, 0))[0] == E
    with pytest.raises(ValueError):
        ME.mirror_mesh(v[:5], f[:5], M(1, 2, 4, 0, 0))


def test_host_program_under_the_sanitizers():
    """tests/cpp/mirror_host.cpp built with -fsanitize=address,undefined: its own walk of the argument rules and of the source mapping
    at counts up to 2^32 - 1 runs clean, and so do the fullest, the emptiest and the rigged case, with the same bytes."""
    r = subprocess.run([_host_exe("san")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    for name in ("three_middle", "empty_mesh", "no_vertices_no_faces", "bone_none_and_past", "unrigged_specials"):
        objects, selected, bones, rigged = object_cases()[name]
        bv, bf, rest, bo, (v0, vc, f0, fc) = source_of(objects, selected, bones, rigged)
        m = M(3, v0, vc, f0, fc)
        rc, hv, hf = host_mesh(bv, bf, m, rest, bo, bones if rigged else None, mode="san")
        assert rc == 0 and _same_mesh((hv, hf), ME.mirror_mesh(bv, bf, m, rest, bo, bones if rigged else None)), name


# ================================================================== the order case
OW, OH = 160, 120


@functools.lru_cache(maxsize=None)
def order_case():
    """Two overlapping body triangles at ONE camera depth, the camera at x = 0 with the identity basis and the mirror axis X: a twin has
    its source's depth.  A spans x in [-20, 60], B x in [-70, 30]: A's twin lies over B where A itself does not.  Flat colour per face."""
    v = b32.make_vertices(6)
    v["pos"] = [(-20, -40, 200), (60, -40, 200), (20, 45, 200), (-70, -25, 200), (30, -30, 200), (-25, 50, 200)]
    v["normal"] = (0.0, 0.0, -1.0)
    v["r"][:3], v["g"][:3], v["b"][:3] = 250, 40, 40
    v["r"][3:], v["g"][3:], v["b"][3:] = 40, 60, 250
    f = b32.make_faces(2)
    f["v"] = [(0, 1, 2), (3, 4, 5)]
    cam = b32.Camera(position=(0.0, 0.0, 0.0))
    return v, f, cam, M(1, 0, 6, 0, 2)


def _order_settings(mode):
    st = b32.RasterSettings.game()
    st.shading = abi.SHADE_NONE; st.lights = []; st.backface_cull = False; st.dithering = False
    st.use_zbuffer = mode != "painter"
    if mode == "rgba8":
        st.use_rgb555 = False
    return st


def _oracle_frame(oracle, v, f, textures, cam, st, w, h, clear=None):
    ofb = oracle.Framebuffer(w, h); ofb.clear(clear if clear is not None else b32.Color(10, 10, 10))
    if st.use_rgb555:
        rc, tm, d = oracle.render_mesh_15(ofb, v, f, textures, cam, st, dump=True)
    else:
        rc, tm, d = oracle.render_mesh(ofb, v, f, textures, cam, st, dump=True)
    assert rc == 0
    return ofb.pixels.copy(), ofb.zbuffer.copy(), tm.triangles_drawn, d["draw_order"].copy()


def test_the_order_case_is_live(oracle):
    """A twin drawn directly behind its source face is another frame than all body faces followed by all twins: in painter's mode by equal
    keys, in z-buffer mode by equal depths under strict `<`.  Both pixel counts are non-zero."""
    v, f, cam, m = order_case()
    mv, mf = ME.mirror_mesh(v, f, m)
    assert np.array_equal(mv["pos"][6:, 2], v["pos"][:, 2]) and np.array_equal(mv["pos"][6:, 0], -v["pos"][:, 0])
    tail = (mv, np.concatenate([mf[0::2], mf[1::2]]))                           # all body faces, then all twins
    for mode in ("painter", "zbuffer"):
        st = _order_settings(mode)
        built = _oracle_frame(oracle, mv, mf, [], cam, st, OW, OH)
        other = _oracle_frame(oracle, tail[0], tail[1], [], cam, st, OW, OH)
        assert built[2] == other[2] == 4
        n = int((built[0].reshape(-1, 4) != other[0].reshape(-1, 4)).any(axis=1).sum())
        print(mode, "pixels that differ between interleaved twins and twins as a tail:", n)
        assert n > 0, mode


# ================================================================== mutations
def _moved(mirror, names, axis=1):
    out = []
    for name in names:
        objects, selected, bones, rigged = object_cases()[name]
        bv, bf, rest, bo, (v0, vc, f0, fc) = source_of(objects, selected, bones, rigged)
        m = M(axis, v0, vc, f0, fc)
        args = (bv, bf, m, rest, bo, bones if rigged else None)
        out.append(not _same_mesh(mirror.mesh(*args), ME.mirror_mesh(*args)))
    return out


def test_mutations_of_the_mirror_move_named_cases():
    """Each one-point change to the mirror changes the case named for it (and leaves alone a case that cannot see it)."""
    MM = ME.MeshMirror

    class NoWindingSwap(MM):
        def twin_face(self, v, c):
            return self.shifted(v, c)

    class TwinFirst(MM):
        def range_faces(self, faces, c):
            out = MM.range_faces(self, faces, c)
            out[0::2], out[1::2] = out[1::2].copy(), out[0::2].copy()
            return out

    class MirrorAfterBone(MM):
        def twin_posed(self, pos, normal, axis, pose):
            return self.mirror_local(*pose(pos, normal), axis)

    class NormalNotMirrored(MM):
        def mirror_local(self, pos, normal, axis):
            return MM.mirror_local(self, pos, normal, axis)[0], np.array(normal, f32, copy=True)

    class ZeroMinus(MM):
        @staticmethod
        def flip(a):
            with np.errstate(all="ignore"):
                return f32(0.0) - np.asarray(a, f32)

    class Rounded(MM):
        def dim_channel(self, ch, dim):
            return np.minimum(np.rint(np.asarray(ch, np.uint8).astype(f32) * f32(dim)), 255).astype(np.uint8)

    class BlendCopied(MM):
        def twin_blend(self, src_blend):
            return np.array(src_blend, np.uint8, copy=True)

    class LaterNotShifted(MM):
        def later_faces(self, faces, c):
            return np.array(faces, copy=True)

    assert _moved(NoWindingSwap(), ["three_middle", "no_faces"]) == [True, False]
    assert _moved(TwinFirst(), ["three_first", "no_faces"]) == [True, False]
    assert _moved(MirrorAfterBone(), ["one_object", "unrigged_specials", "no_pose_yet"]) == [True, False, False]
    assert _moved(NormalNotMirrored(), ["three_last", "unrigged_specials"]) == [True, True]
    assert _moved(ZeroMinus(), ["unrigged_specials"]) == [True]                # (+0.0 -> 0 - 0 = +0.0, and the NaN's sign stays)
    assert _moved(LaterNotShifted(), ["three_first", "three_middle", "three_last"]) == [True, True, False]
    # the colour rules on records of their own: 180 * 0.85 = 153.0 exactly, 255 * 0.85 = 216.75 -> 216 truncated, 217 rounded
    v, f = _generic()
    v["r"] = 255; v["blend"] = abi.ADD
    m = M(1, 0, len(v), 0, len(f))
    assert not _same_mesh(Rounded().mesh(v, f, m), ME.mirror_mesh(v, f, m)) and Rounded().mesh(v, f, m)[0]["r"][-1] == 217 and ME.mirror_mesh(v, f, m)[0]["r"][-1] == 216
    assert not _same_mesh(BlendCopied().mesh(v, f, m), ME.mirror_mesh(v, f, m))
    v["r"] = 180; v["blend"] = abi.OPAQUE
    assert _same_mesh(Rounded().mesh(v, f, m), ME.mirror_mesh(v, f, m)) and _same_mesh(BlendCopied().mesh(v, f, m), ME.mirror_mesh(v, f, m))


# ================================================================== on the GPU
def _real(name):
    from bonnie32_amd import scenefile
    return scenefile.read_scene(os.path.join(REAL, name + ".b32scene"))


def _assert_frame(fb, pixels, zbuffer, what=""):
    got = fb.pixels
    assert np.array_equal(got, pixels), f"{what}: {int((got != pixels).sum())} bytes differ"
    gz = fb.zbuffer.view(np.uint32)
    assert np.array_equal(gz, zbuffer.view(np.uint32)), f"{what}: {int((gz != zbuffer.view(np.uint32)).sum())} depths differ"


def _pose_table(t, scale):
    """test_pose.py's bone table of frame t"""
    s = scale
    return RM.pack_bones([RM.Bone.from_euler((0.06 * s * np.sin(0.7 * t), 0.03 * s, -0.04 * s * np.cos(0.4 * t)), (6.0 + 3.0 * t, 0.0, -5.0 + 2.0 * t)),
                          RM.Bone.from_euler((0.35 * s - 0.02 * s * t, -0.05 * s, 0.02 * s * t), (0.0004, 30.0, 0.0)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (-4.0 - 1.5 * t, 0.0, 3.0 + t)),
                          RM.Bone.from_euler((-0.3 * s + 0.01 * s * t, 0.02 * s * t, 0.05 * s), (2.0 * t, 0.0, 9.0)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))])


@functools.lru_cache(maxsize=None)
def _warrior():
    sc = _real("obj-warrior")
    assert len(sc.vertices) == 227
    sc.textures8 = [b32.Texture.from_texture15(t) for t in sc.textures]
    rng = np.random.default_rng(5)
    bo = np.repeat(rng.integers(0, 8, 227 // 8 + 2).astype(np.uint16), 8)[:227].copy()
    bo[bo == 7] = NONE
    return sc, bo, 1000.0


def _warrior_mirror():
    sc, _, _ = _warrior()
    return M(1, 0, len(sc.vertices), 0, len(sc.faces))


def _warrior_built(t, faces=None, vertices=None):
    """(vertices, faces) the reference would assemble from the warrior posed by table t (None: no pose yet)"""
    sc, bo, scale = _warrior()
    v = sc.vertices if vertices is None else vertices
    f = sc.faces if faces is None else faces
    tab = _pose_table(t, scale) if t is not None else None
    posed = RM.pose_vertices(v, bo, tab) if tab is not None else v
    return ME.mirror_mesh(posed, f, _warrior_mirror(), RM.rest_stream(v), bo, tab)


def _bits_source(bv, rigged):
    """a body of bv vertices and bv + 3 faces; a rigged one keeps its specials on vertices without a bone (the bits of a NaN that goes
    through arithmetic are the machine's)"""
    o = _obj(100 + bv, bv, bv + 3, specials=True)
    bo = np.array([NONE if b is None else b for b in o.bone], np.uint16)
    if bv >= 8:
        bo[:8] = [NONE, 5, 63, 0xFFFE, NONE, 7, NONE, 6]
    return o.v, o.f, bo


def _ranges(bv, bf):
    out = [(0, bv, 0, bf), (0, 0, 0, 0), (bv // 3, bv // 3, bf // 3, bf // 3), (0, 0, bf // 2, bf - bf // 2), (bv // 2, bv - bv // 2, 0, 0)]
    if bv >= 257:
        out += [(100, 20, 100, 20), (200, 50, 200, 50)] + [(e - 3, 3, e - 3, 3) for e in (255, 256, 257)] + [(0, e, 0, e) for e in (255, 256, 257)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dst_size", ["grows", "larger"])
@pytest.mark.parametrize("rigged", [False, True], ids=["unrigged", "rigged"])
def test_built_bits(gpu_ctx, rigged, dst_size):
    """b32_scene_read_vertices / _read_faces of dst equal mirror_mesh: bv in {0, 1, 63, 64, 65, 257, 1025}, ranges whose ends fall on 255,
    256 and 257, rigged and unrigged, into a dst that has to grow and into one that is larger."""
    from bonnie32_amd import rasterizer as R
    fb = R.Framebuffer(64, 48, gpu_ctx)
    n0 = 1 if dst_size == "grows" else 3000
    dst = R.ResidentScene(fb, b32.make_vertices(n0), b32.make_faces(n0)).detach()
    tab = _bones(1.5)
    try:
        for bv in (0, 1, 63, 64, 65, 257, 1025):
            v, f, bo = _bits_source(bv, rigged)
            src = R.ResidentScene(fb, v, f).detach()
            try:
                posed, rest = v, None
                if rigged:
                    src.set_rig(bo)
                    if bv != 63:                                                # (63: built before the first pose)
                        src.pose(tab)
                        posed = RM.pose_vertices(v, bo, tab)
                    rest = RM.rest_stream(v)
                for axis, (v0, vc, f0, fc) in enumerate(_ranges(bv, len(f))):
                    m = M(1 + axis % 3, v0, vc, f0, fc)
                    ME.build_mirror(dst, src, m)
                    want = ME.mirror_mesh(posed, f, m, rest, bo if rigged else None, tab if rigged and bv != 63 else None)
                    assert (dst.n_vertices, dst.n_faces) == (len(want[0]), len(want[1]))
                    assert _same_mesh((dst.read_vertices(), dst.read_faces()), want), (bv, vars(m))
                assert _same_mesh((src.read_vertices(), src.read_faces()), (posed, f)), bv
            finally:
                src.close()
    finally:
        dst.close()


def _settings(mode):
    sc, _, _ = _warrior()
    st = copy.copy(sc.settings)
    if mode == "painter":
        st.use_zbuffer = False; st.shading = abi.SHADE_NONE; st.backface_wireframe = False; st.lights = []
    elif mode == "zbuffer_wire":
        assert st.use_zbuffer and st.backface_wireframe and st.backface_cull
    elif mode == "nocull":
        st.use_zbuffer = False; st.backface_cull = False; st.backface_wireframe = False
    elif mode == "rgba8":
        st.use_rgb555 = False
    return st


MODES = ["painter", "zbuffer_wire", "nocull", "rgba8"]
_EXPECT = {}


def _expect_warrior(oracle, mode, t):
    if (mode, t) not in _EXPECT:
        sc, _, _ = _warrior()
        v, f = _warrior_built(t)
        _EXPECT[(mode, t)] = _oracle_frame(oracle, v, f, sc.textures8 if mode == "rgba8" else sc.textures, sc.camera, _settings(mode), 640, 480, sc.clear_color)
        assert _EXPECT[(mode, t)][2] > 100
    return _EXPECT[(mode, t)]


def _pair(R, fb, mode, rig=True):
    """(src in a slot, dst as the context's scene) of the warrior; dst starts as the warrior itself with its textures"""
    sc, bo, _ = _warrior()
    src = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    if rig:
        src.set_rig(bo)
    dst = R.ResidentScene(fb, sc.vertices, sc.faces, textures8=sc.textures8) if mode == "rgba8" else R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    return src, dst


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_warrior_frame_equals_the_oracle(oracle, mode):
    """Drawing dst equals the oracle's render of the mirror-built arrays: pixels, z-buffer, triangles_drawn and b32_last_draw_order;
    obj-warrior at 640x480, rigged and posed, the whole mesh mirrored."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(640, 480, ctx)
        src, dst = _pair(R, fb, mode)
        for t in (1.0, 4.0):
            px, zb, drawn, order = _expect_warrior(oracle, mode, t)
            src.pose(_pose_table(t, scale))
            ME.build_mirror(dst, src, _warrior_mirror())
            fb.clear(sc.clear_color)
            dst.render_async(sc.camera, _settings(mode))
            tm = dst.finish()
            _assert_frame(fb, px, zb, f"{mode}, t = {t}")
            assert tm.triangles_drawn == drawn
            assert np.array_equal(ctx.last_draw_order(dst.n_faces), order)
        src.close()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["painter", "zbuffer", "rgba8"])
def test_order_case_frame_equals_the_oracle(oracle, mode):
    """The order case on the device: the frame of the built slot is the oracle's frame of the interleaved arrays, not that of the twins
    as a tail."""
    from bonnie32_amd import rasterizer as R
    v, f, cam, m = order_case()
    st = _order_settings(mode)
    mv, mf = ME.mirror_mesh(v, f, m)
    px, zb, drawn, order = _oracle_frame(oracle, mv, mf, [], cam, st, OW, OH)
    other = _oracle_frame(oracle, mv, np.concatenate([mf[0::2], mf[1::2]]), [], cam, st, OW, OH)
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(OW, OH, ctx)
        src = R.ResidentScene(fb, v, f).detach()
        dst = R.ResidentScene(fb, v[:1], f[:0], textures8=[]) if mode == "rgba8" else R.ResidentScene(fb, v[:1], f[:0])
        ME.build_mirror(dst, src, m)
        fb.clear(b32.Color(10, 10, 10))
        dst.render_async(cam, st)
        tm = dst.finish()
        _assert_frame(fb, px, zb, mode)
        assert tm.triangles_drawn == drawn == 4 and np.array_equal(ctx.last_draw_order(4), order)
        assert not np.array_equal(fb.pixels, other[0])
        src.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_the_chain_of_edits(oracle):
    """set_rig on src, pose A, build, draw; then pose B, pose none, a rest-space patch_vertices and a patch_faces to alpha 100, each
    followed by a build: dst's bits are mirror_mesh of the host-side composition, b32_transparent_counts a fresh upload's, and the last
    frame the oracle's."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    st = _settings("painter")
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(640, 480, ctx)
        src, dst = _pair(R, fb, "painter")
        verts, faces = sc.vertices.copy(), sc.faces.copy()

        def check(t, what):
            ME.build_mirror(dst, src, _warrior_mirror())
            want = _warrior_built(t, faces, verts)
            assert _same_mesh((dst.read_vertices(), dst.read_faces()), want), what
            return want

        src.pose(_pose_table(1.0, scale))
        px, zb, drawn, _ = _expect_warrior(oracle, "painter", 1.0)
        check(1.0, "pose A")
        fb.clear(sc.clear_color); dst.render_async(sc.camera, st); tm = dst.finish()
        _assert_frame(fb, px, zb, "pose A"); assert tm.triangles_drawn == drawn
        src.pose(_pose_table(4.0, scale)); check(4.0, "pose B")
        src.pose([]); check(None, "pose none")
        src.pose(_pose_table(4.0, scale))
        idx = np.arange(3, 227, 17)
        recs = verts[idx].copy(); recs["pos"] += f32(12.5); recs["normal"][:, 1] = f32(-0.0); recs["r"] = 90
        src.patch_vertices(idx, recs); verts[idx] = recs
        check(4.0, "patch_vertices")
        assert ctx.transparent_counts()[0] == 0
        fidx = np.arange(0, len(faces), 3)
        frecs = faces[fidx].copy(); frecs["editor_alpha"] = 100
        src.patch_faces(fidx, frecs); faces[fidx] = frecs
        want = check(4.0, "patch_faces")
        assert ctx.transparent_counts()[0] == 2 * len(fidx)
        px, zb, drawn, _ = _oracle_frame(oracle, want[0], want[1], sc.textures, sc.camera, st, 640, 480, sc.clear_color)
        fb.clear(sc.clear_color); dst.render_async(sc.camera, st); tm = dst.finish()
        _assert_frame(fb, px, zb, "alpha 100"); assert tm.triangles_drawn == drawn
        # ... and what a fresh upload of the built arrays leaves
        R.ResidentScene(fb, want[0], want[1], sc.textures)
        assert ctx.transparent_counts()[0] == 2 * len(fidx)
        src.close()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["rgb555", "rgba8"])
def test_transparent_counts_equal_a_fresh_uploads(fmt):
    """dst's blend bookkeeping after a build equals a fresh upload of the built arrays with dst's textures: a dst whose texture blends
    (Average) under a src whose textures do not, faces with a blend mode and with editor_alpha < 255 inside and outside the range, then
    none of either."""
    from bonnie32_amd import rasterizer as R
    sc, _, _ = _warrior()
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(64, 48, ctx)
        faces = sc.faces.copy()
        faces["texture_id"][::5] = abi.NO_TEXTURE; faces["texture_id"][1::5] = 7
        faces["blend_mode"][10:40:4] = abi.ADD; faces["editor_alpha"][100:160:7] = 100
        blending = [copy.copy(t) for t in sc.textures]
        for t in blending:
            t.blend_mode = abi.AVERAGE
        tex = {"plain": sc.textures, "blending": blending}
        tex8 = {k: [b32.Texture.from_texture15(t) for t in v] for k, v in tex.items()}
        mk = lambda v, f, which: R.ResidentScene(fb, v, f, textures8=tex8[which]) if fmt == "rgba8" else R.ResidentScene(fb, v, f, tex[which])
        for which in ("blending", "plain"):
            for f in (faces, sc.faces):
                src = R.ResidentScene(fb, sc.vertices, f, sc.textures).detach()
                for m in (M(2, 0, 227, 0, len(f)), M(2, 50, 100, 20, 100), M(3, 0, 0, 0, 0)):
                    want_v, want_f = ME.mirror_mesh(sc.vertices, f, m)
                    mk(want_v, want_f, which)
                    want = ctx.transparent_counts()[0]
                    dst = mk(sc.vertices[:3], sc.faces[:1], which)
                    ME.build_mirror(dst, src, m)
                    assert ctx.transparent_counts()[0] == want, (which, vars(m))
                    if fmt == "rgb555" and which == "plain" and f is faces:
                        own = (f["blend_mode"] != 0) | (f["editor_alpha"] < 255)
                        assert want == int(own.sum() + own[m.f_first:m.f_first + m.f_count].sum()) and want > 0
                src.close()
    finally:
        ctx.close()


def _rig_bones(scale, t):
    s = scale
    rots = [(6.0 + 3.0 * t, 0.0, -5.0 + 2.0 * t), (0.0004, 30.0, 0.0), (-4.0 - 1.5 * t, 0.0, 3.0 + t), (2.0 * t, 0.0, 9.0), (75.0, 0.0, 100.0 + 10.0 * t)]
    pos = [(0.06 * s * np.sin(0.7 * t), 0.03 * s, -0.04 * s * np.cos(0.4 * t)), (0.35 * s - 0.02 * s * t, -0.05 * s, 0.02 * s * t), (0.0, 0.0, 0.0),
           (-0.3 * s + 0.01 * s * t, 0.02 * s * t, 0.05 * s), (0.1 * s, 0.4 * s, -0.1 * s)]
    lengths, widths, parents = [0.3 * s, 0.2 * s, 0.25 * s, 0.15 * s, 0.35 * s], [0.0, 0.03 * s, 0.0, 0.02 * s, 0.04 * s], [None, 0, 1, 0, 3]
    return RM.pack_skel_bones([RM.SkelBone.from_rig(pos[k], rots[k], lengths[k], widths[k], parents[k]) for k in range(5)])


def _with_tail(built, scale, t, style):
    tv, tf = RM.skeleton_mesh(_rig_bones(scale, t), style, len(built[0]))
    return np.concatenate([built[0], tv]), np.concatenate([built[1], tf])


@pytest.mark.gpu
def test_skeleton_behind_a_build(oracle):
    """b32_scene_build_skeleton(dst) after a build equals the oracle on (built mesh + mirror tail) as one mesh; the next build drops the
    tail again."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    st = _settings("zbuffer_wire")
    style = RM.SkeletonStyle(editor_alpha=100, hovered_tip=2)
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(640, 480, ctx)
        src, dst = _pair(R, fb, "zbuffer_wire")
        src.pose(_pose_table(1.0, scale))
        ME.build_mirror(dst, src, _warrior_mirror())
        dst.build_skeleton(_rig_bones(scale, 1.0), style)
        v, f = _with_tail(_warrior_built(1.0), scale, 1.0, style)
        assert (dst.n_vertices, dst.n_faces, dst.n_body_vertices) == (len(v), len(f), 454)
        assert _same_mesh((dst.read_vertices(), dst.read_faces()), (v, f))
        px, zb, drawn, order = _oracle_frame(oracle, v, f, sc.textures, sc.camera, st, 640, 480, sc.clear_color)
        fb.clear(sc.clear_color); dst.render_async(sc.camera, st); tm = dst.finish()
        _assert_frame(fb, px, zb, "built + tail")
        assert tm.triangles_drawn == drawn and np.array_equal(ctx.last_draw_order(dst.n_faces), order)
        ME.build_mirror(dst, src, _warrior_mirror())
        assert (dst.n_vertices, dst.n_faces) == (454, 2 * len(sc.faces)) and _same_mesh((dst.read_vertices(), dst.read_faces()), _warrior_built(1.0))
        src.close()
    finally:
        ctx.close()


def _merge_quads(faces):
    fv = [tuple(int(i) for i in f) for f in faces["v"]]
    out, i = [], 0
    while i < len(fv):
        if i + 1 < len(fv) and fv[i][0] == fv[i + 1][0] and fv[i][2] == fv[i + 1][1]:
            out.append([fv[i][0], fv[i][1], fv[i][2], fv[i + 1][2]]); i += 2
        else:
            out.append(list(fv[i])); i += 1
    return out


@pytest.mark.gpu
def test_src_comes_through_a_build_unchanged(gpu_ctx):
    """src's bits, tail, hover, box-select and pick answers and bounds are the same before and after a build, and a merged run that holds
    src is not rebuilt (b32_batch_count)."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    other = _real("obj-ghost-game")
    cam, w, h = sc.camera, sc.width, sc.height
    top = R.Topology.from_polygons(_merge_quads(sc.faces))
    fb = R.Framebuffer(w, h, gpu_ctx)
    src = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    dst = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
    b = R.ResidentScene(fb, other.vertices, other.faces, other.textures).detach()
    st = b32.RasterSettings.game()
    pl = b32.Placement(facing=0.0)
    try:
        src.set_rig(bo); src.pose(_pose_table(1.0, scale))
        src.build_skeleton(_rig_bones(scale, 1.0), RM.SkeletonStyle())
        bm = R.HoverMirror(RM.pose_vertices(sc.vertices, bo, _pose_table(1.0, scale)), top, None, cam, w, h)
        curs = [(float(bm.sx[i]) + 1.0, float(bm.sy[i]) - 1.0) for i in np.nonzero(bm.some)[0][::37]]
        table = gpu_ctx.make_frame_table(cam, st, [src, b])

        def answers():
            gpu_ctx.frame_submit(table); gpu_ctx.finish()
            out = [src.read_vertices().tobytes(), src.read_faces().tobytes(), (src.n_vertices, src.n_body_vertices)]
            for c in curs:
                out.append(np.asarray(gpu_ctx.hover_mesh(src, top, cam, c)).tobytes())
                best, hits = gpu_ctx.pick_meshes([(src, pl)], cam, c)
                out.append((best, hits.tobytes()))
            for mode in (abi.BOX_VERTICES, abi.BOX_POLYGONS):
                words, n = gpu_ctx.box_select(src, top, cam, (w * 0.2, h * 0.1, w * 0.8, h * 0.9), mode)
                out.append((words.tobytes(), n))
            mn, mx, has = src.bounds()
            out.append((mn.tobytes(), mx.tobytes(), has))
            return out, gpu_ctx.batch_counts()["merged_built"]

        before, built0 = answers()
        ME.build_mirror(dst, src, _warrior_mirror())
        ME.build_mirror(dst, src, M(3, 10, 50, 5, 60))
        after, built1 = answers()
        assert before == after and built1 == built0
        assert dst.n_vertices == 227 + 50
    finally:
        src.close(); dst.close(); b.close(); top.close()


@pytest.mark.gpu
def test_dst_in_a_two_slot_frame(oracle):
    """dst and a second slot in b32_frame_submit equal the sequential oracle calls, for two builds."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    other = _real("obj-ghost-game")
    st = b32.RasterSettings.game()
    st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7)]
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(320, 240, ctx)
        src = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach(); src.set_rig(bo)
        dst = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
        b = R.ResidentScene(fb, other.vertices, other.faces, other.textures).detach()
        table = ctx.make_frame_table(sc.camera, st, [dst, b])
        for t in (1.0, 4.0):
            src.pose(_pose_table(t, scale))
            ME.build_mirror(dst, src, _warrior_mirror())
            fb.clear(sc.clear_color)
            ctx.frame_submit(table); ctx.finish()
            ofb = oracle.Framebuffer(320, 240); ofb.clear(sc.clear_color)
            for v, f, tex in (_warrior_built(t) + (sc.textures,), (other.vertices, other.faces, other.textures)):
                assert oracle.render_mesh_15(ofb, v, f, tex, sc.camera, st)[0] == 0
            _assert_frame(fb, ofb.pixels, ofb.zbuffer, f"t = {t}")
        src.close(); dst.close(); b.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_drag_frames_without_a_host_wait(oracle):
    """Four delivered drag frames -- patch_vertices(src), pose(src), build_mirror, build_skeleton(dst), draw, download_async -- with only
    the last ticket waited for equal the host-side composition."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    st = _settings("painter")
    style = RM.SkeletonStyle(hovered_bone=1)
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(320, 240, ctx)
        src, dst = _pair(R, fb, "painter")
        ME.build_mirror(dst, src, _warrior_mirror()); dst.build_skeleton(_rig_bones(scale, 1.0), style)     # (the buffers have grown, src's faces are on the host)
        verts = sc.vertices.copy()
        idx = np.arange(5, 227, 11)
        frames = [1.0, 4.0, 2.0, 4.0]
        bufs = [ctx.host_alloc(320 * 240 * 4) for _ in frames]
        tickets, wants = [], []
        for k, t in enumerate(frames):
            recs = verts[idx].copy(); recs["pos"][:, 0] += f32(3.0 * (k + 1))
            src.patch_vertices(idx, recs); verts[idx] = recs
            src.pose(_pose_table(t, scale))
            ME.build_mirror(dst, src, _warrior_mirror())
            dst.build_skeleton(_rig_bones(scale, t), style)
            fb.clear(sc.clear_color)
            dst.render_async(sc.camera, st)
            tickets.append(ctx.download_async(bufs[k][1]))
            wants.append(_with_tail(_warrior_built(t, None, verts.copy()), scale, t, style))
        ctx.ticket_wait(tickets[-1])
        dst.finish()
        for k, (v, f) in enumerate(wants):
            px = _oracle_frame(oracle, v, f, sc.textures, sc.camera, st, 320, 240, sc.clear_color)[0]
            assert bufs[k][0].tobytes() == px.tobytes(), f"frame {k}"
        for _, p in bufs:
            ctx.host_free(p)
        src.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_error_table():
    """Every refused call returns its code and leaves dst untouched."""
    from bonnie32_amd import rasterizer as R
    sc, bo, _ = _warrior()
    ctx = R.Context(0)
    lib, E, U = ctx.lib, abi.B32_E_ARG, abi.B32_E_UNSUPPORTED
    try:
        fb = R.Framebuffer(64, 48, ctx)
        empty = C.c_void_p()
        assert lib.b32_scene_create(ctx.h, C.byref(empty)) == 0
        ok = M(1, 0, 227, 0, len(sc.faces)).pack()
        assert lib.b32_scene_build_mirror(ctx.h, empty, None, abi.ptr(ok)) == E                   # no scene anywhere yet
        src = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
        assert lib.b32_scene_build_mirror(ctx.h, src._slot, None, abi.ptr(ok)) == E               # dst (the context) without a scene
        dst = R.ResidentScene(fb, sc.vertices[:9], sc.faces[:2], sc.textures)
        gen = lambda: (dst.read_vertices().tobytes(), dst.read_faces().tobytes(), ctx.transparent_counts()[0])
        before = gen()
        bad = lambda *a: abi.ptr(M(*a).pack())
        nf = len(sc.faces)
        keep = []
        for args, want in (((None, src._slot, None, abi.ptr(ok)), E), ((ctx.h, src._slot, None, None), E), ((ctx.h, None, None, abi.ptr(ok)), E),
                           ((ctx.h, src._slot, src._slot, abi.ptr(ok)), E), ((ctx.h, empty, None, abi.ptr(ok)), E), ((ctx.h, src._slot, empty, abi.ptr(ok)), E)):
            assert lib.b32_scene_build_mirror(*args) == want, args
        for a in ((0, 0, 0, 0, 0), (4, 0, 0, 0, 0), (1, 1, 227, 0, 0), (1, 228, 0, 0, 0), (1, 0, 0, 1, nf), (1, 0, 0, nf + 1, 0), (2, 0xFFFFFFFF, 2, 0, 0)):
            p = M(*a).pack(); keep.append(p)
            assert lib.b32_scene_build_mirror(ctx.h, src._slot, None, abi.ptr(p)) == E, a
        assert gen() == before and (dst.n_vertices, dst.n_faces) == (9, 2)
        assert lib.b32_scene_build_mirror(ctx.h, src._slot, None, abi.ptr(ok)) == 0
        assert lib.b32_scene_read_vertices(ctx.h, None, 453, 1, abi.ptr(np.zeros(1, abi.VERTEX_DTYPE))) == 0
        nvo, nfo = C.c_uint32(), C.c_uint32()
        big = M(1, 0, 1, 0, 0).pack()
        assert lib.b32_mirror_counts(0xFFFFFFFF, 0, abi.ptr(big), C.byref(nvo), C.byref(nfo)) == U
        src.close()
        lib.b32_scene_destroy(ctx.h, empty)
    finally:
        ctx.close()
