"""The modeler's bone octahedra as a mesh tail (b32_scene_build_skeleton) and the skeleton's overlay (b32_skeleton_items).

Without a GPU: csrc/b32_skeleton_body.h built for the host (tests/cpp/skeleton_host.cpp) against a literal restatement of the Rust
text and against the numpy mirror (rasterizer.SkeletonMirror), bit for bit on named cases; the library's host-only entries; the
constants; one-point mutations of the mirror, each of which must move a named case.
On the GPU: the tail's bits, frames against the oracle's render of (posed body + mirror tail) as ONE mesh, order independence with
b32_scene_pose, the queries that must not see the tail, lifetime and errors, the overlay, and a frame sequence without a host wait."""
import atexit
import copy
import ctypes as C
import functools
import json
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi
from bonnie32_amd import rasterizer as RM          # (imports no device code: the host mirrors live there)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden", "scenes", "real")
GOLD = os.path.join(ROOT, "tests", "golden")
f32 = np.float32
NONE = abi.BONE_NONE
W, H = 320, 240
QNAN = 0x7FC00000


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same_bits(a, b):
    """bit for bit, except that any NaN equals any NaN (the literal restatement keeps the machine's NaN, the library writes 0x7FC00000)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _same_mesh(a, b, nan_any=False):
    (av, af), (bv, bf) = a, b
    if nan_any:
        return (len(av) == len(bv) and _same_bits(av["pos"], bv["pos"]) and _same_bits(av["normal"], bv["normal"]) and _same_bits(av["uv"], bv["uv"])
                and all(np.array_equal(av[k], bv[k]) for k in ("r", "g", "b", "blend")) and af.tobytes() == bf.tobytes())
    return av.tobytes() == bv.tobytes() and af.tobytes() == bf.tobytes()


# ================================================================== the literal restatement (scalar f32, the Rust text line by line)
class V3:
    """rasterizer/math.rs Vec3 over np.float32"""

    def __init__(self, x, y, z):
        self.x, self.y, self.z = f32(x), f32(y), f32(z)

    def dot(self, o):
        return self.x * o.x + self.y * o.y + self.z * o.z

    def len(self):
        return np.sqrt(self.dot(self))

    def normalize(self):
        l = self.len()
        if l == 0.0:
            return V3(0, 0, 0)
        return V3(self.x / l, self.y / l, self.z / l)

    def __add__(self, o):
        return V3(self.x + o.x, self.y + o.y, self.z + o.z)

    def __sub__(self, o):
        return V3(self.x - o.x, self.y - o.y, self.z - o.z)

    def __mul__(self, s):
        return V3(self.x * f32(s), self.y * f32(s), self.z * f32(s))

    def t(self):
        return (self.x, self.y, self.z)


def _cross(a, b):
    return V3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x)


def _perpendicular_axes(d):
    up = V3(0.0, 1.0, 0.0) if abs(d.y) < f32(0.9) else V3(1.0, 0.0, 0.0)
    perp1 = _cross(d, up).normalize()
    perp2 = _cross(d, perp1).normalize()
    return perp1, perp2


def _lit_tip(b):
    direction = V3(b["sin_z"] * b["cos_x"], b["cos_z"] * b["cos_x"], -b["sin_x"]).normalize()
    return V3(*b["pos"]) + direction * b["length"]


def _lit_octahedron(base, tip, bone_width, color, editor_alpha, vertices, faces, offset):
    direction = tip - base
    length = direction.len()
    if length < f32(0.001):
        return
    dir_norm = direction * (f32(1.0) / length)
    perp1, perp2 = _perpendicular_axes(dir_norm)
    width = f32(bone_width)
    ring_center = base + dir_norm * (length * f32(0.2))
    ring = [ring_center + perp1 * width, ring_center + perp2 * width, ring_center - perp1 * width, ring_center - perp2 * width]
    v_start = offset + len(vertices)
    vertices.append((base.t(), (dir_norm * -1.0).t(), color))
    vertices.append((tip.t(), dir_norm.t(), color))
    for i in range(4):
        vertices.append((ring[i].t(), (ring[i] - ring_center).normalize().t(), color))
    for i in range(4):
        nxt = (i + 1) % 4
        faces.append((v_start + 0, v_start + 2 + i, v_start + 2 + nxt, editor_alpha))
    for i in range(4):
        nxt = (i + 1) % 4
        faces.append((v_start + 1, v_start + 2 + nxt, v_start + 2 + i, editor_alpha))


COL = {"default": (200, 200, 200), "selected": (80, 255, 80), "hovered": (100, 180, 255), "tip_hovered": (255, 180, 80), "root": (255, 220, 100),
       "creating": (255, 150, 50), "line": (100, 100, 100)}


def literal_mesh(tab, st, offset=0):
    """skeleton_to_triangles (mode 0) / skeleton_to_triangles_from_bones (mode 1)"""
    vertices, faces = [], []
    with np.errstate(all="ignore"):
        has_selection = st.selected_bone is not None
        for idx, b in enumerate(tab):
            root = b["parent"] == NONE
            if st.mode == 1:
                color, alpha = COL["root"] if root else COL["default"], st.editor_alpha
            else:
                if st.selected_bone == idx:
                    color = COL["selected"]
                elif st.hovered_tip == idx:
                    color = COL["tip_hovered"]
                elif st.hovered_bone == idx:
                    color = COL["hovered"]
                elif root:
                    color = COL["root"]
                else:
                    color = COL["default"]
                alpha = min(st.editor_alpha, 30) if has_selection and st.selected_bone != idx else st.editor_alpha
            _lit_octahedron(V3(*b["pos"]), _lit_tip(b), b["width"], color, alpha, vertices, faces, offset)
        if st.mode == 0 and st.preview is not None:
            _lit_octahedron(V3(*st.preview[0]), V3(*st.preview[1]), 40.0, COL["creating"], 255, vertices, faces, offset)
    v = np.zeros(len(vertices), abi.VERTEX_DTYPE); f = np.zeros(len(faces), abi.FACE_DTYPE)
    for k, (p, n, c) in enumerate(vertices):
        v[k]["pos"], v[k]["normal"] = p, n
        v[k]["r"], v[k]["g"], v[k]["b"] = c
    for k, (a, b_, c, alpha) in enumerate(faces):
        f[k]["v"] = (a, b_, c)
        f[k]["texture_id"], f[k]["editor_alpha"] = abi.NO_TEXTURE, alpha
    return v, f


def literal_items(tab, st):
    """draw_skeleton's then draw_bone_dots' calls: (kind, p0, p1, size, rgb, flags)"""
    calls = []
    with np.errstate(all="ignore"):
        for idx, b in enumerate(tab):
            if b["parent"] != NONE:
                parent_pos = tuple(tab[b["parent"]]["pos"]) if b["parent"] < len(tab) else (f32(0), f32(0), f32(0))
                calls.append((abi.LINE_2D, parent_pos, tuple(b["pos"]), 0, COL["line"], abi.WORLD_CLIP_NEAR))
        for idx, b in enumerate(tab):
            radius, color = (11, (255, 180, 80)) if st.hovered_tip == idx else ((8, (80, 255, 80)) if st.selected_bone == idx else (5, (220, 220, 230)))
            calls.append((abi.PRIM_CIRCLE, _lit_tip(b).t(), (0, 0, 0), radius, color, 0))
            radius, color = (11, COL["hovered"]) if st.hovered_bone == idx else ((8, (80, 255, 80)) if st.selected_bone == idx else (5, (150, 150, 160)))
            calls.append((abi.PRIM_CIRCLE, tuple(b["pos"]), (0, 0, 0), radius, color, 0))
    it = np.zeros(len(calls), abi.WORLD_ITEM_DTYPE)
    for k, (kind, p0, p1, size, rgb, flags) in enumerate(calls):
        it[k]["kind"], it[k]["p0"], it[k]["p1"], it[k]["size"], it[k]["flags"] = kind, p0, p1, size, flags
        it[k]["r"], it[k]["g"], it[k]["b"] = rgb
    it["alpha"] = 255
    return it


# ================================================================== the cases
def _rig(scale, t):
    """The skeleton that goes with test_pose.py's bone table of frame t (t None: unposed): five bones, a chain and a branch."""
    s = scale
    if t is None:
        rots = [(0.0, 0.0, 0.0)] * 5
        t = 0.0
    else:
        rots = [(6.0 + 3.0 * t, 0.0, -5.0 + 2.0 * t), (0.0004, 30.0, 0.0), (-4.0 - 1.5 * t, 0.0, 3.0 + t), (2.0 * t, 0.0, 9.0), (75.0, 0.0, 100.0 + 10.0 * t)]
    pos = [(0.06 * s * np.sin(0.7 * t), 0.03 * s, -0.04 * s * np.cos(0.4 * t)), (0.35 * s - 0.02 * s * t, -0.05 * s, 0.02 * s * t), (0.0, 0.0, 0.0),
           (-0.3 * s + 0.01 * s * t, 0.02 * s * t, 0.05 * s), (0.1 * s, 0.4 * s, -0.1 * s)]
    lengths, widths, parents = [0.3 * s, 0.2 * s, 0.25 * s, 0.15 * s, 0.35 * s], [0.0, 0.03 * s, 0.0, 0.02 * s, 0.04 * s], [None, 0, 1, 0, 3]
    return RM.pack_skel_bones([RM.SkelBone.from_rig(pos[k], rots[k], lengths[k], widths[k], parents[k]) for k in range(5)])


def _random_rig(seed, n, scale=300.0):
    rng = np.random.default_rng(seed)
    return RM.pack_skel_bones([RM.SkelBone.from_rig(rng.standard_normal(3) * scale, rng.uniform(-180, 180, 3), rng.uniform(1.0, scale),
                                                    rng.choice([0.0, 5.0, 40.0]), None if k == 0 or rng.random() < 0.1 else int(rng.integers(0, k))) for k in range(n)])


def _straight(length, width=4.0, pos=(0.0, 0.0, 0.0), parent=None):
    """a bone along +Y exactly: direction (0, 1, 0), tip = pos + (0, length, 0)"""
    return RM.SkelBone(pos, 1.0, 0.0, 1.0, 0.0, length, width, parent)


DEAD = RM.SkelBone((1.0, 2.0, 3.0), 0.0, 0.0, 0.0, 0.0, 50.0, 4.0, 0)               # direction ZERO: tip == base
LIVE = [_straight(30.0, 4.0, (10.0 * k, 0.0, 5.0), None if k == 0 else k - 1) for k in range(4)]


def _next(x, up):
    return np.nextafter(f32(x), f32(np.inf if up else -np.inf))


@functools.lru_cache(maxsize=None)
def _up_bones():
    """Two bones whose dir_norm.y is exactly f32(0.9) and the float just below: found among directions (sqrt(1 - c*c), c, 0) near c = 0.9."""
    m = RM.SkeletonMirror()
    found = {}
    with np.errstate(all="ignore"):
        c = f32(0.9)
        for _ in range(400):
            c = _next(c, False)
        for _ in range(800):
            c = _next(c, True)
            for pos, length in (((3.0, -2.0, 7.0), 100.0), ((0.0, 0.0, 0.0), 64.0), ((0.0, 0.0, 0.0), 37.0), ((1.0, 1.0, 1.0), 3.25)):
                b = RM.SkelBone(pos, 1.0, 0.0, c, np.sqrt(f32(1.0) - c * c), length, 6.0)
                r = b.record()
                tip = m.tip(r)
                d = [tip[k] - r["pos"][k] for k in range(3)]
                y = d[1] * (f32(1.0) / m.length(d))
                for name, want in (("at", f32(0.9)), ("below", _next(0.9, False))):
                    if y == want and name not in found:
                        found[name] = b
    assert set(found) == {"at", "below"}, found.keys()
    return found


def _len_bone(target):
    b = _straight(target)
    m = RM.SkeletonMirror()
    with np.errstate(all="ignore"):
        r = b.record(); tip = m.tip(r)
        got = m.length([tip[k] - r["pos"][k] for k in range(3)])
    assert _bits(got) == _bits(f32(target)) or (np.isnan(got) and np.isnan(target))
    return b


S = RM.SkeletonStyle


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (bone table, style)"""
    c = {}
    c["warrior_posed"] = (_rig(1000.0, 1.0), S())
    c["warrior_unposed"] = (_rig(1000.0, None), S())
    for n in (1, 7, 33, 64):
        c[f"random_{n}"] = (_random_rig(n, n), S(editor_alpha=180))
    c["up_at"] = ([_up_bones()["at"]], S())
    c["up_below"] = ([_up_bones()["below"]], S())
    for name, L in (("len_at", f32(0.001)), ("len_below", _next(0.001, False)), ("len_above", _next(0.001, True)), ("len_zero", f32(0.0)), ("len_nan", f32(np.nan))):
        c[name] = ([LIVE[0], _len_bone(L), LIVE[1]], S())
    c["zero_direction"] = ([DEAD], S())
    c["dead_first"] = ([DEAD] + LIVE[:3], S())
    c["dead_middle"] = ([LIVE[0], DEAD, DEAD, LIVE[1]], S())
    c["dead_last"] = (LIVE[:3] + [DEAD], S())
    c["dead_all"] = ([DEAD, DEAD, DEAD], S())
    c["full_64_preview"] = (_random_rig(64, 64), S(preview=((5.0, 6.0, 7.0), (40.0, -30.0, 20.0)), hovered_bone=63))
    c["preview_only"] = ([], S(preview=((0.0, 0.0, 0.0), (0.0, 0.0, 25.0))))
    c["preview_dead"] = (LIVE[:1], S(preview=((1.0, 1.0, 1.0), (1.0, 1.0, 1.0))))
    c["parent_out_of_range"] = ([LIVE[0], _straight(20.0, 4.0, (7.0, 7.0, 7.0), 9)], S())
    c["inf_nan_positions"] = ([_straight(20.0, 4.0, (np.inf, 0.0, 0.0)), _straight(20.0, 4.0, (0.0, np.nan, 0.0), 0), LIVE[0]], S())
    rig = _rig(200.0, 2.0)                                                     # bone 0 a root, the others children
    for who, i in (("root", 0), ("child", 3)):
        c[f"selected_{who}"] = (rig, S(selected_bone=i))
        c[f"hovered_{who}"] = (rig, S(hovered_bone=i))
        c[f"tip_hovered_{who}"] = (rig, S(hovered_tip=i))
    c["priority"] = (rig, S(selected_bone=1, hovered_tip=1, hovered_bone=1))
    c["priority_tip_over_hover"] = (rig, S(hovered_tip=2, hovered_bone=2))
    c["dim_below_30"] = (rig, S(selected_bone=1, editor_alpha=20))
    c["dim_above_30"] = (rig, S(selected_bone=1, editor_alpha=100))
    c["selected_past_the_table"] = (rig, S(selected_bone=40, editor_alpha=100))
    c["mode_1"] = (rig, S(selected_bone=1, hovered_bone=2, hovered_tip=3, editor_alpha=140, mode=1, preview=((0.0, 0.0, 0.0), (0.0, 9.0, 0.0))))
    return {k: (RM.pack_skel_bones(v[0]), v[1]) for k, v in c.items()}


# ================================================================== the host build of the device header
HOST_FLAGS = {"off": ["-O1", "-ffp-contract=off"], "fused": ["-O2", "-ffp-contract=fast", "-mfma"],
              "san": ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@functools.lru_cache(maxsize=None)
def _host_dir():
    d = tempfile.mkdtemp(prefix="b32_skeleton_host_")
    atexit.register(shutil.rmtree, d, True)
    return d


@functools.lru_cache(maxsize=None)
def _host_exe(mode):
    exe = os.path.join(_host_dir(), "skeleton_host_" + mode)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + HOST_FLAGS[mode] + ["-I", os.path.join(ROOT, "bonnie-32_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "skeleton_host.cpp"), "-o", exe], check=True)
    return exe


def host_mesh(tab, st, offset=0, mode="off"):
    """(vertices, faces, tips) from csrc/b32_skeleton_body.h compiled for the host"""
    d = _host_dir()
    src, dst = os.path.join(d, "in_" + mode), os.path.join(d, "out_" + mode)
    with open(src, "wb") as f:
        f.write(np.array([len(tab), offset], np.uint32).tobytes() + st.pack().tobytes() + np.ascontiguousarray(tab).tobytes())
    subprocess.run([_host_exe(mode), src, dst], check=True)
    blob = open(dst, "rb").read()
    nv, nf = np.frombuffer(blob[:8], np.uint32)
    v = np.frombuffer(blob, abi.VERTEX_DTYPE, nv, 8)
    f = np.frombuffer(blob, abi.FACE_DTYPE, nf, 8 + 36 * int(nv))
    tips = np.frombuffer(blob, f32, 3 * len(tab), 8 + 36 * int(nv) + 20 * int(nf)).reshape(-1, 3)
    return v, f, tips


def test_header_on_the_host_equals_the_literal_restatement_and_the_mirror():
    """Check 1: every named case, vertex for vertex and face for face: header == mirror bit for bit, == the literal restatement with any
    NaN equal to any NaN (the restatement does not canonicalise), a NaN always 0x7FC00000 in the library's output; the tips are the
    mirror's; an offset moves nothing but the indices."""
    n_live = {}
    for name, (tab, st) in cases().items():
        for offset in (0, 227):
            hv, hf, tips = host_mesh(tab, st, offset)
            mirror = RM.skeleton_mesh(tab, st, offset)
            assert _same_mesh((hv, hf), mirror), name
            assert _same_mesh((hv, hf), literal_mesh(tab, st, offset), nan_any=True), name
            for k in ("pos", "normal"):
                assert (_bits(hv[k])[np.isnan(hv[k])] == QNAN).all(), name
            m = RM.SkeletonMirror()
            with np.errstate(all="ignore"):
                assert _same_bits(tips, np.array([m.tip(b) for b in tab], f32).reshape(-1, 3)), name
            if len(hf):
                assert hf["v"].min() == offset and hf["v"].max() == offset + len(hv) - 1
        n_live[name] = len(hv) // 6
    # the cases are what their names say
    assert n_live["len_at"] == 3 and n_live["len_above"] == 3 and n_live["len_nan"] == 3 and n_live["len_below"] == 2 and n_live["len_zero"] == 2
    assert n_live["zero_direction"] == 0 and n_live["dead_all"] == 0 and n_live["dead_first"] == 3 and n_live["dead_middle"] == 2 and n_live["dead_last"] == 3
    assert n_live["full_64_preview"] == 65 and n_live["preview_only"] == 1 and n_live["preview_dead"] == 1 and n_live["mode_1"] == 5
    assert n_live["inf_nan_positions"] == 3 and n_live["parent_out_of_range"] == 2
    a, b = (RM.skeleton_mesh(*cases()[k])[0] for k in ("up_at", "up_below"))
    assert abs(a["normal"][2][0]) == 0.0 and abs(b["normal"][2][1]) == 0.0      # perp1 = cross(dir, +X) has no x; cross(dir, +Y) has no y


FUSED = os.path.join(GOLD, "skeleton", "fused_input.npz")


def test_a_contracted_build_is_told_apart():
    """Check 1, the FMA build: on the committed input the header built with -ffp-contract=fast -mfma differs from the restatement, and the
    build without contraction does not."""
    z = np.load(FUSED)
    tab = np.ascontiguousarray(z["bones"].view(abi.SKEL_BONE_DTYPE).reshape(-1))
    st = S(editor_alpha=int(z["editor_alpha"]))
    want = literal_mesh(tab, st)
    hv, hf, _ = host_mesh(tab, st)
    assert _same_mesh((hv, hf), want, nan_any=True)
    fv, ff, _ = host_mesh(tab, st, mode="fused")
    assert len(fv) == len(want[0]) and ff.tobytes() == want[1].tobytes()
    n = int(((_bits(fv["pos"]) != _bits(want[0]["pos"])) | (_bits(fv["normal"]) != _bits(want[0]["normal"]))).any(axis=1).sum())
    print("vertices a contracted build places differently:", n, "of", len(fv))
    assert n >= 1


def test_host_program_under_the_sanitizers():
    """Check 1, last point: the stand-alone program built with -fsanitize=address,undefined runs clean on the fullest and the emptiest
    case and gives the same bytes."""
    for name in ("full_64_preview", "dead_all", "inf_nan_positions", "preview_only"):
        tab, st = cases()[name]
        hv, hf, _ = host_mesh(tab, st, 7, mode="san")
        assert _same_mesh((hv, hf), RM.skeleton_mesh(tab, st, 7)), name


def test_counts_items_and_constants():
    """Check 2: b32_skeleton_counts and b32_skeleton_items from the built library equal the mirror and the literal restatement call for
    call; the error returns of the host-only entries; the literals of header and mirror equal tests/golden/skeleton_constants.json."""
    lib = abi.load_library()
    for name, (tab, st) in cases().items():
        s = st.pack()
        nv, nf, n = C.c_uint32(9), C.c_uint32(9), C.c_uint32(9)
        p = abi.ptr(tab) if len(tab) else None
        assert lib.b32_skeleton_counts(p, len(tab), abi.ptr(s), C.byref(nv), C.byref(nf)) == 0
        v, f = RM.skeleton_mesh(tab, st)
        assert (nv.value, nf.value) == (len(v), len(f)), name
        want = literal_items(tab, st)
        assert RM.skeleton_items(tab, st).tobytes() == want.tobytes(), name
        out = np.zeros(len(want) + 2, abi.WORLD_ITEM_DTYPE)
        assert lib.b32_skeleton_items(p, len(tab), abi.ptr(s), abi.ptr(out), len(out), C.byref(n)) == 0 and n.value == len(want), name
        assert out[:n.value].tobytes() == want.tobytes() and not out[n.value:].tobytes().strip(b"\0"), name
        assert lib.b32_skeleton_items(p, len(tab), abi.ptr(s), None, 0, C.byref(n)) == 0 and n.value == len(want)
        if len(want) > 1:                                                       # a short buffer is filled and not overrun
            short = np.zeros(2, abi.WORLD_ITEM_DTYPE)
            assert lib.b32_skeleton_items(p, len(tab), abi.ptr(s), abi.ptr(short), 1, C.byref(n)) == 0 and n.value == len(want)
            assert short[0].tobytes() == want[0].tobytes() and not short[1].tobytes().strip(b"\0")
    tab, st = cases()["selected_child"]
    assert (literal_items(tab, st)["kind"] == abi.LINE_2D).sum() == 4 and len(literal_items(tab, st)) == 14
    assert len(literal_items(*cases()["parent_out_of_range"])) == 5 and not literal_items(*cases()["parent_out_of_range"])[0]["p0"].any()
    s, n = st.pack(), C.c_uint32()
    E, U = abi.B32_E_ARG, abi.B32_E_UNSUPPORTED
    big = np.zeros(65, abi.SKEL_BONE_DTYPE)
    bad = S(mode=2).pack()
    assert lib.b32_skeleton_counts(None, 3, abi.ptr(s), None, None) == E and lib.b32_skeleton_counts(abi.ptr(tab), 5, None, None, None) == E
    assert lib.b32_skeleton_counts(abi.ptr(tab), 5, abi.ptr(bad), None, None) == E and lib.b32_skeleton_counts(abi.ptr(big), 65, abi.ptr(s), None, None) == U
    assert lib.b32_skeleton_counts(abi.ptr(big), 64, abi.ptr(s), None, None) == 0 and lib.b32_skeleton_counts(None, 0, abi.ptr(s), None, None) == 0
    assert lib.b32_skeleton_items(abi.ptr(tab), 5, abi.ptr(s), None, 0, None) == E and lib.b32_skeleton_items(None, 5, abi.ptr(s), None, 0, C.byref(n)) == E
    assert lib.b32_skeleton_items(abi.ptr(big), 65, abi.ptr(s), None, 0, C.byref(n)) == U and lib.b32_skeleton_items(abi.ptr(tab), 5, None, None, 0, C.byref(n)) == E
    assert lib.b32_scene_build_skeleton(None, None, abi.ptr(tab), 5, abi.ptr(s)) == E
    # constants
    k = json.load(open(os.path.join(GOLD, "skeleton_constants.json")))
    M = RM.SkeletonMirror
    assert {n_: list(v) for n_, v in M.COLOURS.items()} == k["bone_colours"]
    assert {n_: {"radius": r, "colour": list(c)} for n_, (r, c) in M.DOTS.items()} == k["dots"] and list(M.DOT_ORDER) == k["dot_order"]
    assert M.DIM_ALPHA == k["dim_alpha"] and _bits(M.DEFAULT_WIDTH) == _bits(f32(k["default_width"])) and _bits(M.DEGENERATE) == _bits(f32(k["degenerate_length"]))
    assert _bits(M.UP_LIMIT) == _bits(f32(k["up_limit"])) and _bits(M.RING_AT) == _bits(f32(k["ring_at"]))
    dw = k["display_width"]
    assert (dw["scale"], dw["min"], dw["max"]) == (0.15, 20.0, 200.0) and k["opacity_to_alpha"] == [255, 220, 180, 140, 100, 60, 30, 0]
    for length, width, want in ((100.0, 7.0, 7.0), (100.0, 0.0, 20.0), (400.0, 0.0, 60.0), (4000.0, -1.0, 200.0)):
        assert _bits(RM.SkelBone.display_width(length, width)) == _bits(f32(length) * f32(dw["scale"]) if want == 60.0 else f32(want))
    src = open(os.path.join(ROOT, "bonnie-32_amd", "csrc", "b32_skeleton_body.h")).read()
    lit = {m.group(1): m.group(2) for m in re.finditer(r"constexpr (?:float|uint32_t) (SKEL_[A-Z_]+) = ([0-9.]+)[fu];", src)}
    assert (float(lit["SKEL_DEGENERATE"]), float(lit["SKEL_UP_LIMIT"]), float(lit["SKEL_RING_AT"]), float(lit["SKEL_DEFAULT_WIDTH"]), int(lit["SKEL_DIM_ALPHA"])) == \
        (k["degenerate_length"], k["up_limit"], k["ring_at"], k["default_width"], k["dim_alpha"])
    cols = {m.group(1).lower(): [int(m.group(2)), int(m.group(3)), int(m.group(4))] for m in re.finditer(r"(?:case SKEL_COL_([A-Z_]+)|(?=default)): return (\d+)u \| (\d+)u << 8 \| (\d+)u << 16;", src) if m.group(1)}
    assert cols == {n_: v for n_, v in k["bone_colours"].items() if n_ != "default"}
    assert re.search(r"default: return 200u \| 200u << 8 \| 200u << 16;", src) and k["bone_colours"]["default"] == [200, 200, 200]


def _moved(mirror, names, what="mesh"):
    """the named cases on which a changed mirror answers differently"""
    out = []
    for name in names:
        tab, st = cases()[name]
        if what == "mesh":
            out.append(not _same_mesh(mirror.mesh(tab, st), RM.skeleton_mesh(tab, st)))
        else:
            out.append(mirror.items(tab, st).tobytes() != RM.skeleton_items(tab, st).tobytes())
    return out


def test_mutations_of_the_mirror_move_named_cases():
    """Check 3: each one-point change to the mirror changes the case named for it (and leaves its neighbour alone where there is one)."""
    M = RM.SkeletonMirror

    class LessEqual(M):
        def degenerate(self, length):
            return length <= self.DEGENERATE

    class UpPlus(M):
        UP_LIMIT = _next(0.9, True)

    class UpMinus(M):
        UP_LIMIT = _next(0.9, False)

    class Reciprocal(M):
        def normalize(self, v):
            l = self.length(v)
            if l == 0.0:
                return [f32(0.0)] * 3
            r = f32(1.0) / l
            return [v[0] * r, v[1] * r, v[2] * r]

    class Winding(M):
        RING = ((0, 1), (1, -1), (0, -1), (1, 1))

    class DimAll(M):
        def dimmed(self, style, i):
            return style.selected_bone is not None and style.selected_bone >= 0

    class BaseFirst(M):
        DOT_ORDER = ("base", "tip")

    assert _moved(LessEqual(), ["len_at", "len_above", "len_below"]) == [True, False, False]
    assert _moved(UpPlus(), ["up_at", "up_below"]) == [True, False]
    assert _moved(UpMinus(), ["up_at", "up_below"]) == [False, True]
    assert any(_moved(Reciprocal(), ["warrior_posed", "random_64"]))
    assert all(_moved(Winding(), ["warrior_posed", "up_at", "preview_only"]))
    assert _moved(DimAll(), ["dim_above_30", "dim_below_30", "hovered_root"]) == [True, False, False]
    assert all(_moved(BaseFirst(), ["warrior_posed", "selected_child"], "items")) and not any(_moved(BaseFirst(), ["warrior_posed"]))


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


STYLES = {"opaque": S(editor_alpha=255, hovered_bone=1), "alpha100": S(editor_alpha=100, hovered_tip=2), "dimmed": S(editor_alpha=220, selected_bone=3)}
_EXPECT = {}


def _combined(t, style):
    """(posed body + mirror tail) as ONE mesh"""
    sc, bo, scale = _warrior()
    body = RM.pose_vertices(sc.vertices, bo, _pose_table(t, scale)) if t is not None else sc.vertices
    tv, tf = RM.skeleton_mesh(_rig(scale, t), style, len(body))
    return np.concatenate([body, tv]), np.concatenate([sc.faces, tf])


def _expect(oracle, mode, t, style_name):
    key = (mode, t, style_name)
    if key not in _EXPECT:
        sc, _, _ = _warrior()
        v, f = _combined(t, STYLES[style_name])
        ofb = oracle.Framebuffer(W, H); ofb.clear(sc.clear_color)
        if mode == "rgba8":
            rc, tm, d = oracle.render_mesh(ofb, v, f, sc.textures8, sc.camera, _settings(mode), dump=True)
        else:
            rc, tm, d = oracle.render_mesh_15(ofb, v, f, sc.textures, sc.camera, _settings(mode), dump=True)
        assert rc == 0 and tm.triangles_drawn > 50 and (d["draw_order"] >= len(sc.faces)).sum() >= 8
        _EXPECT[key] = (ofb.pixels.copy(), ofb.zbuffer.copy(), tm.triangles_drawn, d["draw_order"].copy())
    return _EXPECT[key]


def _scene(R, fb, mode, detached=True):
    sc, bo, _ = _warrior()
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, textures8=sc.textures8) if mode == "rgba8" else R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    if detached:
        rs.detach()
    rs.set_rig(bo)
    return rs


TAILS = ["dead_all", "preview_only", "len_below", "dead_first", "dead_middle", "dead_last", "full_64_preview"]


@pytest.mark.gpu
@pytest.mark.parametrize("body", ["warrior", "empty", "tight"])
def test_tail_bits(gpu_ctx, body):
    """Check 4: after build_skeleton the tail read back equals skeleton_mesh and the body's bits are untouched: 0, 1, 3 and 64 bones plus
    the preview, dead bones first / middle / last, on obj-warrior, on an empty body and on a fresh upload whose capacity every growing
    tail has to outgrow while the body is kept."""
    from bonnie32_amd import rasterizer as R
    sc, _, _ = _warrior()
    fb = R.Framebuffer(W, H, gpu_ctx)
    bv, bf = (sc.vertices, sc.faces) if body != "empty" else (np.zeros(0, abi.VERTEX_DTYPE), b32.make_faces(0))
    rs = R.ResidentScene(fb, bv, bf, sc.textures).detach()
    try:
        for name in (["full_64_preview", "dead_all", "preview_only"] if body == "tight" else TAILS):
            if body == "tight":                                                 # a fresh upload: capacity for the body alone
                rs._swap()
                assert gpu_ctx.lib.b32_scene_upload(gpu_ctx.h, abi.ptr(np.ascontiguousarray(bv)), len(bv), abi.ptr(np.ascontiguousarray(bf)), len(bf), None, 0) == 0
                rs._swap(); rs.n_vertices, rs.n_faces = len(bv), len(bf)
            tab, st = cases()[name]
            rs.build_skeleton(tab, st)
            tv, tf = RM.skeleton_mesh(tab, st, len(bv))
            assert (rs.n_vertices, rs.n_faces, rs.n_body_vertices, rs.n_body_faces) == (len(bv) + len(tv), len(bf) + len(tf), len(bv), len(bf)), name
            gv, gf = rs.read_vertices(), rs.read_faces()
            assert gv[:len(bv)].tobytes() == np.ascontiguousarray(bv).tobytes() and gf[:len(bf)].tobytes() == np.ascontiguousarray(bf).tobytes(), name
            assert gv[len(bv):].tobytes() == tv.tobytes() and gf[len(bf):].tobytes() == tf.tobytes(), name
            assert gpu_ctx.lib.b32_scene_read_vertices(gpu_ctx.h, rs._slot, len(gv), 1, abi.ptr(np.zeros(1, abi.VERTEX_DTYPE))) == abi.B32_E_ARG
        rs.build_skeleton([], S())
        assert (rs.n_vertices, rs.n_faces) == (len(bv), len(bf)) and rs.read_vertices().tobytes() == np.ascontiguousarray(bv).tobytes()
    finally:
        rs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["context", "slot"])
@pytest.mark.parametrize("style", ["opaque", "alpha100", "dimmed"])
@pytest.mark.parametrize("mode", ["painter", "zbuffer_wire", "nocull", "rgba8"])
def test_frame_equals_the_oracle_on_one_combined_mesh(oracle, mode, style, where):
    """Check 5: pose + build_skeleton + draw equals the oracle's render of (posed body + mirror tail) as one mesh: pixels, z-buffer,
    triangles_drawn and the draw order, for two bone tables, every mode with an opaque, an alpha-100 and a dimmed-to-30 tail, through the
    context's own scene and through a slot of b32_scene_swap.  b32_last_draw_order reads the context's scene, so the order is compared
    there; an 8-bit frame that blends is finished by the slot's swap, which keeps no timings, so its triangles_drawn is compared in the
    context only.  In painter's mode with an opaque tail the frame differs from body-then-skeleton as two draws (asserted on the
    oracle): the tail's faces sort among the body's."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    st = _settings(mode)
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        rs = _scene(R, fb, mode, detached=(where == "slot"))
        for t in (1.0, 4.0):
            px, zb, drawn, order = _expect(oracle, mode, t, style)
            rs.pose(_pose_table(t, scale))
            rs.build_skeleton(_rig(scale, t), STYLES[style])
            fb.clear(sc.clear_color)
            rs.render_async(sc.camera, st)
            tm = rs.finish()
            _assert_frame(fb, px, zb, f"{mode}, {style}, {where}, t = {t}")
            if where == "context" or not (mode == "rgba8" and style != "opaque"):
                assert tm.triangles_drawn == drawn
            if where == "context":
                got = ctx.last_draw_order(rs.n_faces)
                print(mode, style, "draw order:", len(got), "faces,", int((order >= len(sc.faces)).sum()), "of the tail")
                assert np.array_equal(got, order)
        if mode == "painter" and style == "opaque":                             # (a transparent tail is drawn behind the opaque pass either way)
            v, f = _combined(4.0, STYLES[style])
            ofb = oracle.Framebuffer(W, H); ofb.clear(sc.clear_color)
            nb = len(sc.vertices)
            tail_f = f[len(sc.faces):].copy(); tail_f["v"] -= nb
            for vv, ff in ((v[:nb], sc.faces), (v[nb:], tail_f)):
                assert oracle.render_mesh_15(ofb, vv, ff, sc.textures, sc.camera, st)[0] == 0
            assert not np.array_equal(ofb.pixels, _expect(oracle, mode, 4.0, style)[0])
        rs.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_tail_in_a_merged_run(oracle):
    """Check 5, the merged run: a slot with a tail and a second slot in b32_frame_submit equal the sequential oracle calls."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    other = _real("obj-ghost-game")
    st = b32.RasterSettings.game()
    st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7)]
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        a = _scene(R, fb, "game")
        b = R.ResidentScene(fb, other.vertices, other.faces, other.textures).detach()
        table = ctx.make_frame_table(sc.camera, st, [a, b])
        for t, style in ((1.0, "opaque"), (4.0, "alpha100")):
            a.pose(_pose_table(t, scale))
            a.build_skeleton(_rig(scale, t), STYLES[style])
            fb.clear(sc.clear_color)
            ctx.frame_submit(table)
            ctx.finish()
            ofb = oracle.Framebuffer(W, H); ofb.clear(sc.clear_color)
            for v, f, tex in (_combined(t, STYLES[style]) + (sc.textures,), (other.vertices, other.faces, other.textures)):
                assert oracle.render_mesh_15(ofb, v, f, tex, sc.camera, st)[0] == 0
            _assert_frame(fb, ofb.pixels, ofb.zbuffer, f"t = {t}")
        assert ctx.batch_counts()["merged_draws"] >= 1, ctx.batch_counts()     # (the opaque tail is merged; a run with transparent faces is drawn in sequence)
        a.close(); b.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_order_independence_and_replacement(oracle, gpu_ctx):
    """Check 6: pose -> build and build -> pose leave the same slot; a second build replaces the tail only; n_bones == 0 restores the
    body-only slot and its frame."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    st = _settings("zbuffer_wire")
    fb = R.Framebuffer(W, H, gpu_ctx)
    a, b = _scene(R, fb, "zbuffer_wire"), _scene(R, fb, "zbuffer_wire")
    try:
        a.pose(_pose_table(1.0, scale)); a.build_skeleton(_rig(scale, 1.0), STYLES["alpha100"])
        b.build_skeleton(_rig(scale, 1.0), STYLES["alpha100"]); b.pose(_pose_table(1.0, scale))
        wv, wf = _combined(1.0, STYLES["alpha100"])
        for rs in (a, b):
            assert rs.read_vertices().tobytes() == wv.tobytes() and rs.read_faces().tobytes() == wf.tobytes()
        tab, style = cases()["full_64_preview"]
        a.build_skeleton(tab, style)                                            # another table: the tail only (and it grows)
        tv, tf = RM.skeleton_mesh(tab, style, 227)
        assert a.read_vertices().tobytes() == np.concatenate([wv[:227], tv]).tobytes() and a.read_faces().tobytes() == np.concatenate([sc.faces, tf]).tobytes()
        a.pose(_pose_table(4.0, scale))                                         # a pose leaves the tail's bits alone
        assert a.read_vertices(227).tobytes() == tv.tobytes()
        assert a.read_vertices(0, 227).tobytes() == RM.pose_vertices(sc.vertices, bo, _pose_table(4.0, scale)).tobytes()
        a.build_skeleton([], S())
        assert (a.n_vertices, a.n_faces) == (227, len(sc.faces))
        posed = RM.pose_vertices(sc.vertices, bo, _pose_table(4.0, scale))
        ofb = oracle.Framebuffer(W, H); ofb.clear(sc.clear_color)
        rc, otm = oracle.render_mesh_15(ofb, posed, sc.faces, sc.textures, sc.camera, st)
        fb.clear(sc.clear_color); a.render_async(sc.camera, st); tm = a.finish()
        _assert_frame(fb, ofb.pixels, ofb.zbuffer, "tail removed")
        assert rc == 0 and tm.triangles_drawn == otm.triangles_drawn
    finally:
        a.close(); b.close()


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
def test_the_tail_is_never_queried(gpu_ctx):
    """Check 7: b32_hover_mesh, b32_box_select (result size and bits), b32_pick_meshes and b32_draw_mesh_overlay / _record_count on a slot
    with a tail answer exactly as on the same slot without one: cursors on a bone's tip vertex, inside a tail face and on body vertices,
    the rectangle over the whole frame."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    cam, w, h = sc.camera, sc.width, sc.height
    top = R.Topology.from_polygons(_merge_quads(sc.faces))
    style = STYLES["opaque"]
    tv, tf = RM.skeleton_mesh(_rig(scale, 1.0), style, 227)
    tm = R.HoverMirror(tv, R.Topology.triangles(tf["v"] - 227), None, cam, w, h)           # where the tail lands on the screen
    assert tm.some.all()
    bm = R.HoverMirror(RM.pose_vertices(sc.vertices, bo, _pose_table(1.0, scale)), top, None, cam, w, h)
    tri = tf["v"][4] - 227
    curs = [(float(tm.sx[1]), float(tm.sy[1])), (float(tm.sx[7]), float(tm.sy[7])), (float(tm.sx[tri].mean()), float(tm.sy[tri].mean()))]
    curs += [(float(bm.sx[i]) + 1.0, float(bm.sy[i]) - 1.0) for i in np.nonzero(bm.some)[0][::23]]
    assert all(0 <= x < w and 0 <= y < h for x, y in curs[:3])
    fb = R.Framebuffer(w, h, gpu_ctx)
    rs, plain = _scene(R, fb, "painter"), _scene(R, fb, "painter")
    ov = R.MeshOverlay(sections=abi.OVERLAY_BRACKETS | abi.OVERLAY_DOTS | abi.OVERLAY_EDGES)
    pl = b32.Placement(facing=0.0)
    try:
        for rs_ in (rs, plain):
            rs_.pose(_pose_table(1.0, scale))
        rs.build_skeleton(_rig(scale, 1.0), style)
        assert rs.n_vertices == 227 + len(tv) and plain.n_vertices == 227
        canon = lambda r: tuple(int(np.asarray(r[k]).view(np.uint32)) if "d" in k[-5:] and k != "edge_v0" else int(r[k])
                                for k in ("vertex", "vertex_dist", "edge_v0", "edge_v1", "edge_dist", "face", "face_depth"))
        n_hit = 0
        for c in curs:
            for see in (False, True):
                got, want = gpu_ctx.hover_mesh(rs, top, cam, c, see_through=see), gpu_ctx.hover_mesh(plain, top, cam, c, see_through=see)
                assert canon(got) == canon(want), (c, see)
                n_hit += R.hovered_element(want) != (None, None, None)
            (bg, hg), (bw, hw) = gpu_ctx.pick_meshes([(rs, pl)], cam, c), gpu_ctx.pick_meshes([(plain, pl)], cam, c)
            assert bg == bw and hg.tobytes() == hw.tobytes(), c
        assert n_hit >= 4
        for rect in ((0.0, 0.0, float(w), float(h)), (w * 0.3, h * 0.2, w * 0.8, h * 0.9)):
            for mode in (abi.BOX_VERTICES, abi.BOX_POLYGONS):
                (gw, gn), (ww, wn) = gpu_ctx.box_select(rs, top, cam, rect, mode), gpu_ctx.box_select(plain, top, cam, rect, mode)
                assert gn == wn and len(gw) == len(ww) and np.array_equal(gw, ww), (rect, mode)
        words, cnt = gpu_ctx.box_select(rs, top, cam, (0.0, 0.0, float(w), float(h)), abi.BOX_VERTICES)
        assert len(words) == (227 + 31) // 32 and cnt <= 227
        assert gpu_ctx.mesh_overlay_record_count(top, rs.n_body_vertices, ov) == gpu_ctx.mesh_overlay_record_count(top, 227, ov)
        got = fb.mesh_overlay_project_batch(rs, top, ov, cam)
        want = fb.mesh_overlay_project_batch(plain, top, ov, cam)
        assert len(got) == len(want) and got.tobytes() == want.tobytes()
        frames = []
        for rs_ in (rs, plain):
            fb.clear(sc.clear_color); fb.draw_mesh_overlay(rs_, top, ov, cam); frames.append(fb.pixels.copy())
        assert np.array_equal(frames[0], frames[1]) and (frames[0].reshape(-1, 4) != frames[0][:4]).any()
    finally:
        rs.close(); plain.close(); top.close()


@pytest.mark.gpu
def test_lifetime_and_errors():
    """Check 8: b32_scene_upload and b32_room_build_mesh drop the tail, b32_scene_swap carries it, and the error codes."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    tab, style = _rig(scale, 1.0), STYLES["alpha100"]
    s = style.pack()
    ctx = R.Context(0)
    lib, E, U = ctx.lib, abi.B32_E_ARG, abi.B32_E_UNSUPPORTED
    try:
        fb = R.Framebuffer(W, H, ctx)
        empty = C.c_void_p()
        assert lib.b32_scene_create(ctx.h, C.byref(empty)) == 0
        big = np.zeros(65, abi.SKEL_BONE_DTYPE)
        assert lib.b32_scene_build_skeleton(ctx.h, None, abi.ptr(tab), 5, abi.ptr(s)) == E          # no scene: in the context, in a slot
        assert lib.b32_scene_build_skeleton(ctx.h, empty, abi.ptr(tab), 5, abi.ptr(s)) == E
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        assert lib.b32_scene_build_skeleton(ctx.h, None, None, 5, abi.ptr(s)) == E and lib.b32_scene_build_skeleton(ctx.h, None, abi.ptr(tab), 5, None) == E
        assert lib.b32_scene_build_skeleton(ctx.h, None, abi.ptr(tab), 5, abi.ptr(S(mode=2).pack())) == E
        assert lib.b32_scene_build_skeleton(ctx.h, None, abi.ptr(big), 65, abi.ptr(s)) == U
        assert rs.read_vertices().tobytes() == sc.vertices.tobytes()            # (a refused call leaves the slot alone)
        assert lib.b32_scene_build_skeleton(ctx.h, None, abi.ptr(big), 64, abi.ptr(s)) == 0         # 64 bones of length 0: no tail
        assert lib.b32_scene_read_vertices(ctx.h, None, 227, 1, abi.ptr(np.zeros(1, abi.VERTEX_DTYPE))) == E
        rs.build_skeleton(tab, style)
        tv, tf = RM.skeleton_mesh(tab, style, 227)
        rs.detach()                                                             # b32_scene_swap carries the tail
        assert lib.b32_scene_read_vertices(ctx.h, None, 0, 0, None) == E
        assert rs.read_vertices(227).tobytes() == tv.tobytes() and rs.read_faces(len(sc.faces)).tobytes() == tf.tobytes()
        rs.set_rig(bo)                                                          # the rig is the body's: 227 indices
        rs.pose(_pose_table(2.0, scale))
        assert rs.read_vertices(227).tobytes() == tv.tobytes()
        rs._swap()                                                              # an upload drops the tail
        assert lib.b32_scene_upload(ctx.h, abi.ptr(np.ascontiguousarray(sc.vertices)), 227, abi.ptr(np.ascontiguousarray(sc.faces)), len(sc.faces), None, 0) == 0
        out = np.zeros(1, abi.VERTEX_DTYPE)
        assert lib.b32_scene_read_vertices(ctx.h, None, 227, 1, abi.ptr(out)) == E and lib.b32_scene_read_vertices(ctx.h, None, 226, 1, abi.ptr(out)) == 0
        rs._swap(); rs.n_vertices, rs.n_faces = 227, len(sc.faces)
        rs.build_skeleton(tab, style)
        assert rs.n_vertices == 227 + len(tv)
        # b32_room_build_mesh drops it too
        faces = np.zeros(1, abi.SECTOR_FACE_DTYPE); faces["heights"] = 0.0
        room = R.Room(ctx, faces)
        mats = np.zeros(1, abi.FACE_MATERIAL_DTYPE); mats["texture_id"] = abi.NO_TEXTURE; mats["texture_id_2"] = abi.NO_TEXTURE; mats["colors"] = 128; mats["colors_2"] = 128
        room.set_materials(mats)
        room.build_mesh(rs)
        nv, nf = room.mesh_counts()
        assert (rs.n_vertices, rs.n_faces, rs.n_body_vertices) == (nv, nf, nv)
        assert lib.b32_scene_read_vertices(ctx.h, rs._slot, nv, 1, abi.ptr(out)) == E and len(rs.read_vertices()) == nv
        rs.build_skeleton(tab, style)                                           # ... and a tail goes behind a room mesh like behind any body
        assert rs.read_vertices(nv).tobytes() == RM.skeleton_mesh(tab, style, nv)[0].tobytes()
        room.close(); rs.close()
        lib.b32_scene_destroy(ctx.h, empty)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ortho", [None, (0.25, 10.0, -20.0)], ids=["perspective", "ortho"])
def test_overlay_items_over_the_frame(oracle, gpu_ctx, ortho):
    """Check 9: b32_draw_world of skeleton_items over the frame of check 5 equals the oracle frame plus the restated calls through the
    world model; one bone sits across the near plane."""
    from bonnie32_amd import rasterizer as R
    from tests.test_world import cpu_world
    sc, bo, scale = _warrior()
    cam = sc.camera
    style = STYLES["dimmed"]
    px, zb, _, _ = _expect(oracle, "zbuffer_wire", 1.0, "dimmed")
    tab = _rig(scale, 1.0).copy()
    extra = np.zeros(2, abi.SKEL_BONE_DTYPE)
    p = np.asarray(cam.position, f32); z = np.asarray(cam.basis_z, f32)
    extra[0] = RM.SkelBone(tuple(p + z * f32(300.0)), 1.0, 0.0, 1.0, 0.0, 50.0, 10.0, 4).record()
    extra[1] = RM.SkelBone(tuple(p - z * f32(200.0)), 1.0, 0.0, 1.0, 0.0, 50.0, 10.0, 5).record()          # behind the camera: its line crosses the near plane
    tab = np.concatenate([tab, extra])
    items = literal_items(tab, style)
    assert RM.skeleton_items(tab, style).tobytes() == items.tobytes()
    want = px.copy()
    counts = cpu_world(want, zb, W, H, items, cam, ortho)
    assert counts[0] >= 10 and not np.array_equal(want, px)
    fb = R.Framebuffer(W, H, gpu_ctx)
    rs = _scene(R, fb, "zbuffer_wire")
    try:
        rs.pose(_pose_table(1.0, scale)); rs.build_skeleton(_rig(scale, 1.0), style)
        fb.clear(sc.clear_color); rs.render_async(cam, _settings("zbuffer_wire")); rs.finish()
        fb.draw_world(RM.skeleton_items(tab, style), cam, ortho)
        _assert_frame(fb, want, zb, "overlay")
    finally:
        rs.close()


@pytest.mark.gpu
def test_frame_sequence_without_a_host_wait(oracle):
    """Check 10: pose -> build_skeleton -> draw -> b32_draw_world -> b32_fb_download_async with another bone table every frame and only the
    last ticket waited for: every delivered frame equals the host-side composition."""
    from bonnie32_amd import rasterizer as R
    from tests.test_world import cpu_world
    sc, bo, scale = _warrior()
    st = _settings("painter")
    frames = [(1.0, "opaque"), (4.0, "alpha100"), (1.0, "dimmed"), (4.0, "opaque")]
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        rs = _scene(R, fb, "painter")
        rs.build_skeleton(cases()["full_64_preview"][0], S())                   # (the buffers have grown before the sequence starts)
        bufs = [ctx.host_alloc(W * H * 4) for _ in frames]
        tickets = []
        for k, (t, style) in enumerate(frames):
            rs.pose(_pose_table(t, scale))
            rs.build_skeleton(_rig(scale, t), STYLES[style])
            fb.clear(sc.clear_color)
            rs.render_async(sc.camera, st)
            fb.draw_world(RM.skeleton_items(_rig(scale, t), STYLES[style]), sc.camera)
            tickets.append(ctx.download_async(bufs[k][1]))
        ctx.ticket_wait(tickets[-1])
        rs.finish()
        for k, (t, style) in enumerate(frames):
            px, zb, _, _ = _expect(oracle, "painter", t, style)
            want = px.copy()
            cpu_world(want, None, W, H, literal_items(_rig(scale, t), STYLES[style]), sc.camera)
            assert bufs[k][0].tobytes() == want.tobytes(), f"frame {k}"
        for _, p in bufs:
            ctx.host_free(p)
        rs.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_cpp_skeleton_harness(tmp_path):
    """tests/cpp/skeleton_harness.cpp: a golden scene file through the C++ mirror's SkelBone::from_rig / display_width,
    ResidentMesh::build_skeleton and skeleton_items.  from_rig's position, length, resolved width and parent equal the Python mirror's bit
    for bit; cos / sin are each side's libm (glibc's cosf / sinf and numpy's float32 routines both document an error below 1 ulp, so two
    results lie at most 2 ulps apart: that is the bound, and the figure is printed).  The device's tail and the items then equal the
    Python mirror run on the records the C++ side packed, bit for bit."""
    import __graft_entry__ as g
    g.build()
    sc, _, scale = _warrior()
    exe = tmp_path / "skeleton_harness"
    lib_dir = os.path.join(ROOT, "bonnie-32_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bonnie-32_amd", "host"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "skeleton_harness.cpp"), "-o", str(exe), "-L", lib_dir, "-lb32raster", f"-Wl,-rpath,{lib_dir}"], check=True)
    s = scale                                   # widths 0: display_width's three branches (clamped below, scaled, clamped above); one dead bone
    rig = [((0.0, 0.03 * s, 0.0), (6.0, -5.0), 0.3 * s, 0.0, -1), ((0.3 * s, 0.0, 0.02 * s), (95.0, 30.0), 40.0, 0.0, 0), ((0.0, 0.2 * s, 0.0), (-41.5, 170.25), 2000.0, 0.0, 1),
           ((-0.3 * s, 0.0, 0.05 * s), (0.0, 0.0), 0.0, 25.0, 0), ((0.1 * s, 0.4 * s, -0.1 * s), (75.0, 100.0), 0.35 * s, 0.04 * s, 9)]
    args = []
    for pos, (rx, rz), length, width, parent in rig:
        args += [float(f32(x)).hex() for x in pos + (rx, rz, length, width)] + [str(parent)]
    r = subprocess.run([str(exe), os.path.join(REAL, "obj-warrior.b32scene"), "100", "2", str(len(rig))] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = {}
    for line in r.stdout.split("\n"):
        if line:
            rows.setdefault(line[0], []).append(np.array([int(x, 16) for x in line.split()[1:]], np.uint32))
    tab = np.ascontiguousarray(np.stack(rows["B"])).view(abi.SKEL_BONE_DTYPE).reshape(-1)
    want = RM.pack_skel_bones([RM.SkelBone.from_rig(pos, (rx, 0.0, rz), length, width, None if parent < 0 else parent) for pos, (rx, rz), length, width, parent in rig])
    for k in ("pos", "length", "width"):
        assert np.array_equal(_bits(tab[k]), _bits(want[k])), k
    assert np.array_equal(tab["parent"], want["parent"]) and 44.0 < tab["width"][0] < 46.0 and tab["width"][1] == 20.0 and tab["width"][2] == 200.0
    ulps = max(int(np.abs(_bits(tab[k]).astype(np.int64) - _bits(want[k]).astype(np.int64)).max()) for k in ("cos_x", "sin_x", "cos_z", "sin_z"))
    print("cos / sin of the C++ mirror and of the Python mirror differ by at most", ulps, "ulp")
    assert ulps <= 2
    style = S(selected_bone=2, editor_alpha=100)
    tv, tf = RM.skeleton_mesh(tab, style, 227)
    assert rows["C"][0].tolist() == [227, len(tv), len(tf)] and len(tv) == 24
    assert np.stack(rows["V"]).tobytes() == tv.tobytes() and np.stack(rows["F"]).tobytes() == tf.tobytes()
    assert np.stack(rows["I"]).tobytes() == RM.skeleton_items(tab, style).tobytes()
