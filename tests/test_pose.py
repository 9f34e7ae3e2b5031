"""Bones: a rigged resident mesh posed on the device from a per-frame bone table (b32_scene_set_rig, b32_scene_pose).

The modeler skins per vertex on the host -- rotate_by_euler(v.pos, bone_rot) + bone_pos (modeler/state.rs:30-54), in the draw, the box
selection, the selection brackets and the hover -- and only then draws or projects.  `pose_vertices` restates that on the host; the
expected result of every GPU test here is the oracle's render_mesh_15 / render_mesh, or the host mirrors of hover / box selection / pick,
on `pose_vertices` output -- literally what the reference does -- and every comparison is bit for bit: pixels, the depth buffer viewed as
u32, triangles_drawn, positions and normals as u32 (any NaN equals any NaN)."""
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
from bonnie32_amd import abi, scenegen
from bonnie32_amd import rasterizer as RM          # (imports no device code: the host mirrors live there)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "tests", "golden", "scenes", "real")
f32 = np.float32
NONE = abi.BONE_NONE
W, H = 320, 240


# ================================================================== without a GPU
def _same_bits(a, b):
    """bit for bit, except that any NaN equals any NaN (the payload of an invalid operation is not the reference's business)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _same_vertices(a, b):
    return (_same_bits(a["pos"], b["pos"]) and _same_bits(a["normal"], b["normal"]) and np.array_equal(a["uv"].view(np.uint32), b["uv"].view(np.uint32))
            and all(np.array_equal(a[k], b[k]) for k in ("r", "g", "b", "blend")))


def _random_vertices(rng, n, scale):
    v = np.zeros(n, abi.VERTEX_DTYPE)
    v["pos"] = (rng.standard_normal((n, 3)) * scale).astype(f32)
    v["uv"] = rng.random((n, 2)).astype(f32)
    nrm = rng.standard_normal((n, 3)).astype(f32)
    v["normal"] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True).astype(f32)
    for k in ("r", "g", "b", "blend"):
        v[k] = rng.integers(0, 256, n).astype(np.uint8)
    return v


def _scalar_turn(v, bn):
    """state.rs:43-53 one separately rounded f32 operation at a time"""
    x, y, z = (f32(t) for t in v)
    cx, sx, cz, sz = (f32(bn[k]) for k in ("cos_x", "sin_x", "cos_z", "sin_z"))
    a = f32(y * cx); b = f32(z * sx); y1 = f32(a + b)
    ny = f32(-y); c = f32(ny * sx); d = f32(z * cx); z1 = f32(c + d)
    e = f32(x * cz); g = f32(y1 * sz); x2 = f32(e + g)
    nx = f32(-x); h = f32(nx * sz); i = f32(y1 * cz); y2 = f32(h + i)
    return x2, y2, z1


def _scalar_pose(v, bone_of, table):
    """What the four skinning loops of modeler/viewport.rs compute, vertex by vertex."""
    out = v.copy()
    with np.errstate(all="ignore"):
        for i in range(len(v)):
            b = int(bone_of[i])
            if b >= len(table):
                continue                                                        # bone_transforms.get(idx) == None
            bn = table[b]
            bp = [f32(t) for t in bn["pos"]]
            if not bn["rotate"]:                                                # rotate_by_euler returns v
                out["pos"][i] = [f32(f32(v["pos"][i][k]) + bp[k]) for k in range(3)]
                continue
            r = _scalar_turn(v["pos"][i], bn)
            out["pos"][i] = [f32(r[k] + bp[k]) for k in range(3)]
            out["normal"][i] = _scalar_turn(v["normal"][i], bn)
    return out


def _table5(scale=1.0):
    """Five bones: a rotating one, one that takes rotate_by_euler's early return, a rotating one without translation, a second rotating
    one, and an early return without translation."""
    s = scale
    return RM.pack_bones([RM.Bone.from_euler((12.5 * s, -3.25 * s, 40.0 * s), (33.0, 10.0, -71.5)),
                          RM.Bone.from_euler((-7.0 * s, 2.5 * s, 0.125 * s), (0.0005, 45.0, -0.0005)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (-12.0, 0.0, 0.25)),
                          RM.Bone.from_euler((1.0 * s, 100.0 * s, -50.0 * s), (0.0, 0.0, 179.0)),
                          RM.Bone.from_euler((0.0, -0.0, 0.0), (0.0, 90.0, 0.0))])


@functools.lru_cache(maxsize=None)
def _the_set():
    """The vertices, indices and table of tests 1 and 6: random values, zeros of both signs, magnitudes that overflow to infinity (and
    inf - inf), indices at B32_BONE_NONE, n_bones - 1 and n_bones."""
    rng = np.random.default_rng(31)
    v = _random_vertices(rng, 1500, 2000.0)
    special = [0.0, -0.0, 1.0, -1.0, 1e-40, -1e-45, 16777216.0, 1e30, -1e30, 3e38, -3e38]
    grid = np.array([(a, b) for a in special for b in special], f32)
    sv = np.zeros(len(grid) * 5, abi.VERTEX_DTYPE)                             # every special pair under every bone
    g5 = np.tile(grid, (5, 1))
    sv["pos"][:, 1] = g5[:, 0]; sv["pos"][:, 2] = g5[:, 1]; sv["pos"][:, 0] = g5[::-1, 0]
    sv["normal"][:, 0] = g5[:, 1]; sv["normal"][:, 1] = g5[::-1, 1]; sv["normal"][:, 2] = g5[:, 0]
    sv["uv"] = rng.random((len(sv), 2)).astype(f32); sv["r"] = 7; sv["blend"] = 3
    bo = np.concatenate([rng.integers(0, 8, len(v)), np.repeat(np.arange(5), len(grid))]).astype(np.uint16)
    bo[bo == 7] = NONE                                                          # 5, 6: past the table; 7: B32_BONE_NONE
    v = np.concatenate([v, sv])
    bo[:3] = (NONE, 4, 5)
    tab = _table5()
    tab = np.concatenate([tab[:3], RM.pack_bones([RM.Bone((1e30, -3e38, np.inf), cos_x=0.6, sin_x=-0.8, cos_z=-0.0, sin_z=1.0)]), tab[4:]])
    return v, bo, tab


def test_pose_vertices_is_the_scalar_f32_restatement():
    """Test 1: pose_vertices against the reference's expression evaluated step by step in f32 scalars."""
    v, bo, tab = _the_set()
    assert (bo == NONE).sum() > 50 and (bo == 4).sum() > 50 and (bo == 5).sum() > 50 and len(tab) == 5
    got = RM.pose_vertices(v, bo, tab)
    want = _scalar_pose(v, bo, tab)
    assert _same_vertices(got, want)
    assert np.isnan(got["pos"]).any() and np.isinf(got["pos"]).any()          # inf - inf and overflow are in the set
    out = bo >= len(tab)
    assert np.array_equal(got["pos"][out].view(np.uint32), v["pos"][out].view(np.uint32)) and np.array_equal(got["normal"][out].view(np.uint32), v["normal"][out].view(np.uint32))
    # an early-return bone with zero translation: x + 0.0 turns -0.0 into +0.0 and nothing else; the normal keeps its bits
    m = bo == 4
    p, q = v["pos"][m].view(np.uint32), got["pos"][m].view(np.uint32)
    assert np.all((p == q) | ((p == 0x80000000) & (q == 0))) and int((p != q).sum()) > 0
    assert np.array_equal(v["normal"][m].view(np.uint32), got["normal"][m].view(np.uint32))
    # no table, no vertices
    assert _same_vertices(RM.pose_vertices(v, bo, []), v) and RM.pose_vertices(v[:0], bo[:0], tab).shape == (0,)
    assert v is not got and not np.shares_memory(v, got)


def test_from_euler_and_the_rotate_boundary():
    """Test 2: rotate is the reference's strict `<` on |rot.x| and |rot.z| in f32 (y does not count); an early-return bone is "copy +
    translate", which is NOT a multiplication by the tiny angle's cos / sin."""
    assert not RM.Bone.from_euler((1, 2, 3), (0.00099, 77.0, -0.00099)).rotate
    assert RM.Bone.from_euler((1, 2, 3), (0.001, 0.0, 0.0)).rotate             # f32(0.001) < f32(0.001) is false
    assert RM.Bone.from_euler((1, 2, 3), (0.0, 0.0, -0.001)).rotate
    assert RM.Bone.from_euler((0, 0, 0), (np.nan, 0.0, 0.0)).rotate            # NaN < 0.001 is false: the reference rotates (by NaN)
    b = RM.Bone.from_euler((0, 0, 0), (33.0, 0.0, -71.5))
    k = f32(np.pi / 180.0)
    assert b.cos_x == np.cos(f32(33.0) * k) and b.sin_z == np.sin(f32(-71.5) * k) and b.cos_x.dtype == f32
    rec = b.record()
    assert rec["rotate"] == 1 and rec["cos_z"] == b.cos_z and RM.Bone((1, 2, 3), rotate=False).record()["rotate"] == 0
    rng = np.random.default_rng(32)
    v = _random_vertices(rng, 4000, 500.0)
    bo = np.zeros(len(v), np.uint16)
    rot = (0.00099, 0.0, -0.00099)
    early = RM.pose_vertices(v, bo, [RM.Bone.from_euler((5.0, -6.0, 7.0), rot)])
    want = v.copy(); want["pos"] = v["pos"] + np.array([5.0, -6.0, 7.0], f32)
    assert _same_vertices(early, want)
    ax, az = f32(rot[0]) * k, f32(rot[2]) * k
    tiny = RM.pose_vertices(v, bo, [RM.Bone((5.0, -6.0, 7.0), cos_x=np.cos(ax), sin_x=np.sin(ax), cos_z=np.cos(az), sin_z=np.sin(az))])
    differs = (tiny["pos"].view(np.uint32) != early["pos"].view(np.uint32)).any(axis=1)
    assert differs.all(), int((~differs).sum())


def test_random_set_tells_a_fused_evaluation_apart():
    """Test 3: y*cos_x + z*sin_x contracted into a fused multiply-add rounds differently for some inputs.  The fused forms are evaluated
    in float64 (the product of two f32 is exact there) and rounded once; the set must contain values where they differ, and pose_vertices
    must be the separately rounded one."""
    rng = np.random.default_rng(33)
    v = _random_vertices(rng, 4000, 500.0)
    k = f32(np.pi / 180.0)
    cx, sx = np.cos(f32(33.0) * k), np.sin(f32(33.0) * k)
    y, z = v["pos"][:, 1], v["pos"][:, 2]
    y64, z64, cx64, sx64 = y.astype(np.float64), z.astype(np.float64), np.float64(cx), np.float64(sx)
    r32 = lambda t: t.astype(f32).astype(np.float64)
    # z1 = (-y)*sin_x + z*cos_x is the z of the posed position (bone_pos.z = 0) under the bone (33, 0, -71.5)
    got = RM.pose_vertices(v, np.zeros(len(v), np.uint16), [RM.Bone.from_euler((0.0, 0.0, 0.0), (33.0, 0.0, -71.5))])
    z1 = ((-y) * sx).astype(f32) + (z * cx).astype(f32)
    z1_fa = ((-y64) * sx64 + r32(z * cx)).astype(f32); z1_fb = (r32((-y) * sx) + z64 * cx64).astype(f32)
    assert np.array_equal(got["normal"][:, 2], ((-v["normal"][:, 1]) * sx).astype(f32) + (v["normal"][:, 2] * cx).astype(f32))
    assert np.array_equal(got["pos"][:, 2], z1 + f32(0.0))
    # y1 = y*cos_x + z*sin_x shows as y2 when the second rotation is the identity's numbers (cos_z = 1, sin_z = 0: (-x)*0 + y1*1)
    got_y = RM.pose_vertices(v, np.zeros(len(v), np.uint16), [RM.Bone((0.0, 0.0, 0.0), cos_x=cx, sin_x=sx, cos_z=1.0, sin_z=0.0)])
    y1 = (y * cx).astype(f32) + (z * sx).astype(f32)
    y1_fa = (y64 * cx64 + r32(z * sx)).astype(f32); y1_fb = (r32(y * cx) + z64 * sx64).astype(f32)
    assert np.array_equal(got_y["pos"][:, 1], y1)
    counts = [int((a != b).sum()) for a, b in ((y1_fa, y1), (y1_fb, y1), (z1_fa, z1), (z1_fb, z1))]
    print("fused evaluations that differ (y1 a, y1 b, z1 a, z1 b):", counts)
    assert all(c >= 1 for c in counts), counts
    assert int((got_y["pos"][:, 1] != y1_fa).sum()) == counts[0] and int((got["pos"][:, 2] != z1_fb).sum()) == counts[3]


def _literal_bone_world(lp, lr, parents, idx):
    """get_bone_world_transform, state.rs:2585-2614, as written there"""
    n = len(lp)
    if idx >= n:
        return (f32(0), f32(0), f32(0)), (f32(0), f32(0), f32(0))
    position = [f32(0)] * 3; rotation = [f32(0)] * 3
    chain, cur = [], idx
    while cur is not None:
        chain.append(cur); cur = parents[cur]
    for i in reversed(chain):
        v = [f32(t) for t in lp[i]]
        if abs(rotation[0]) < f32(0.001) and abs(rotation[2]) < f32(0.001):
            rp = v
        else:
            k = f32(np.pi / 180.0)
            rx, rz = rotation[0] * k, rotation[2] * k
            rp = _scalar_turn(v, dict(cos_x=np.cos(rx), sin_x=np.sin(rx), cos_z=np.cos(rz), sin_z=np.sin(rz)))
        position = [f32(position[j] + rp[j]) for j in range(3)]
        rotation = [f32(rotation[j] + f32(lr[i][j])) for j in range(3)]
    return tuple(position), tuple(rotation)


def test_bone_world_transforms_against_a_literal_loop():
    """Test 4: a root, a child and a grandchild; a second tree whose summed rotation crosses the 0.001 threshold between child and
    grandchild; an index out of range gives (0, 0)."""
    lp = [(0.0, 100.0, 0.0), (10.0, 50.0, -5.0), (0.0, 30.0, 2.5), (1.0, 2.0, 3.0), (4.0, 5.0, 6.0), (7.0, 8.0, 9.0)]
    lr = [(20.0, 5.0, -30.0), (-45.5, 0.0, 12.25), (3.0, 3.0, 3.0), (0.0006, 0.0, 0.0), (0.0006, 9.0, 0.0), (10.0, 0.0, 0.0)]
    parents = [None, 0, 1, None, 3, 4]
    idx = [0, 1, 2, 3, 4, 5, 6, 99]
    pos, rot = RM.bone_world_transforms(lp, lr, parents, indices=idx)
    for row, i in enumerate(idx):
        wp, wr = _literal_bone_world(lp, lr, parents, i)
        assert _same_bits(pos[row], np.array(wp, f32)) and _same_bits(rot[row], np.array(wr, f32)), i
    assert not pos[6:].any() and not rot[6:].any()
    # bone 4 is placed with the root's 0.0006 (early return: its local position as it is), bone 5 with 0.0012 (rotated)
    assert np.array_equal(pos[4], np.array(lp[3], f32) + np.array(lp[4], f32))
    assert not np.array_equal(pos[5], pos[4] + np.array(lp[5], f32)) and rot[5][0] == f32(f32(f32(0.0006) + f32(0.0006)) + f32(10.0))
    allp, allr = RM.bone_world_transforms(lp, lr, [-1 if p is None else p for p in parents])
    assert np.array_equal(allp, pos[:6]) and np.array_equal(allr, rot[:6])
    assert [RM.Bone.from_euler(allp[i], allr[i]).rotate for i in range(6)] == [True, True, True, False, True, True]


def test_bone_layout_symbols_and_cpp_mirror():
    """Test 5: B32Bone is 32 bytes with the same offsets on both sides of the boundary, the entries resolve in the built library and
    answer B32_E_ARG without a context, and the C++ mirror's bone calls compile without a warning."""
    import __graft_entry__ as g
    g.build()
    lib = abi.load_library()
    assert abi.BONE_DTYPE.itemsize == 32 and [abi.BONE_DTYPE.fields[k][1] for k in ("pos", "cos_x", "sin_x", "cos_z", "sin_z", "rotate")] == [0, 12, 16, 20, 24, 28]
    for name in ("b32_scene_set_rig", "b32_scene_pose", "b32_scene_read_vertices"):
        assert name in {n for n, _, _ in abi.SYMBOLS} and getattr(lib, name).argtypes is not None
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %u %u\\n", sizeof(B32Bone), '
            'offsetof(B32Bone, pos), offsetof(B32Bone, cos_x), offsetof(B32Bone, sin_x), offsetof(B32Bone, cos_z), offsetof(B32Bone, sin_z), '
            'offsetof(B32Bone, rotate), B32_BONE_NONE, B32_MAX_BONES); return 0; }\n')
    cpp = ('#include "rasterizer.hpp"\n'
           'std::vector<B32Vertex> f(b32::ResidentMesh& m, const std::vector<B32Vertex>& v, const std::vector<uint16_t>& bo) {\n'
           '    std::vector<b32::Bone> bones{ b32::Bone::from_euler({ 1, 2, 3 }, { 10, 0, -20 }), b32::Bone{} };\n'
           '    m.set_rig(bo); m.pose(bones); m.pose({});\n'
           '    std::vector<B32Vertex> d = m.read_vertices(0, (uint32_t)v.size());\n'
           '    std::vector<B32Vertex> h = b32::pose_vertices(v, bo, bones);\n'
           '    d.push_back(b32::pose_vertex(h[0], nullptr));\n'
           '    return d;\n}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
        assert [int(x) for x in out] == [32, 0, 12, 16, 20, 24, 28, NONE, abi.MAX_BONES]
        open(os.path.join(d, "t.cpp"), "w").write(cpp)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "bonnie-32_amd", "host"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(d, "t.cpp")], check=True)
    E = abi.B32_E_ARG
    assert lib.b32_scene_set_rig(None, None, None) == E and lib.b32_scene_pose(None, None, None, 0) == E
    assert lib.b32_scene_read_vertices(None, None, 0, 0, None) == E


# ---------------------------------------------------------------- the host build of the device header
# (g++ forms fused multiply-adds from -O2 on, and only where the target has them)
HOST_FLAGS = {"off": ["-O1", "-ffp-contract=off"], "fused": ["-O2", "-ffp-contract=fast", "-mfma"]}
HOST_PROG = r'''
// reads: u32 nv, u32 n_bones, n_bones B32Bone, nv u16 bone indices (padded to 4 bytes), nv x 6 floats (position, normal); writes nv x 6 floats
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "b32_pose_body.h"
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t nv = 0, nb = 0;
    if (std::fread(&nv, 4, 1, f) != 1 || std::fread(&nb, 4, 1, f) != 1) return 3;
    std::vector<B32Bone> bones(nb); std::vector<uint16_t> bo((nv + 1) & ~1u); std::vector<float> rest((size_t)nv * 6), out((size_t)nv * 6);
    if (nb && std::fread(bones.data(), sizeof(B32Bone), nb, f) != nb) return 3;
    if (nv && (std::fread(bo.data(), 2, bo.size(), f) != bo.size() || std::fread(rest.data(), 24, nv, f) != nv)) return 3;
    std::fclose(f);
    for (uint32_t i = 0; i < nv; ++i) b32::pose_vertex(bo[i] < nb ? &bones[bo[i]] : nullptr, &rest[(size_t)i * 6], &out[(size_t)i * 6]);
    f = std::fopen(argv[2], "wb");
    if (!f || (nv && std::fwrite(out.data(), 24, nv, f) != nv)) return 4;
    std::fclose(f);
    return 0;
}
'''


@functools.lru_cache(maxsize=None)
def _host_dir():
    d = tempfile.mkdtemp(prefix="b32_pose_host_")
    atexit.register(shutil.rmtree, d, True)
    open(os.path.join(d, "pose_host.cpp"), "w").write(HOST_PROG)
    return d


@functools.lru_cache(maxsize=None)
def _host_exe(mode):
    d = _host_dir()
    exe = os.path.join(d, "pose_host_" + mode)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + HOST_FLAGS[mode] + ["-I", os.path.join(ROOT, "bonnie-32_amd", "csrc"), os.path.join(d, "pose_host.cpp"), "-o", exe],
                   check=True)
    return exe


def _host_pose(v, bo, tab, mode="off"):
    d = _host_dir()
    bo2 = np.zeros((len(v) + 1) & ~1, np.uint16); bo2[:len(v)] = bo
    rest = np.concatenate([v["pos"], v["normal"]], axis=1).astype(f32)
    src, dst = os.path.join(d, "in_" + mode), os.path.join(d, "out_" + mode)
    with open(src, "wb") as f:
        f.write(np.array([len(v), len(tab)], np.uint32).tobytes() + np.ascontiguousarray(tab).tobytes() + bo2.tobytes() + np.ascontiguousarray(rest).tobytes())
    subprocess.run([_host_exe(mode), src, dst], check=True)
    out = np.fromfile(dst, f32).reshape(len(v), 6)
    got = v.copy(); got["pos"] = out[:, :3]; got["normal"] = out[:, 3:]
    return got


def test_kernel_arithmetic_compiled_for_the_host():
    """Test 6: csrc/b32_pose_body.h -- the text k_pose runs -- built for the host without contraction equals pose_vertices on the set of
    test 1; built with FMA contraction it does not (on the set of test 3, whose values are finite)."""
    v, bo, tab = _the_set()
    assert _same_vertices(_host_pose(v, bo, tab), RM.pose_vertices(v, bo, tab))
    rng = np.random.default_rng(33)
    w = _random_vertices(rng, 4000, 500.0)
    bw = (np.arange(len(w)) % 7).astype(np.uint16)
    t5 = _table5()
    want = RM.pose_vertices(w, bw, t5)
    assert _same_vertices(_host_pose(w, bw, t5), want)
    fused = _host_pose(w, bw, t5, "fused")
    n = int((fused["pos"].view(np.uint32) != want["pos"].view(np.uint32)).any(axis=1).sum())
    print("vertices a contracted build poses differently:", n, "of", len(w))
    assert n >= 1
    early = ~np.isin(bw, [0, 2, 3])                                            # early-return bones and no bone: nothing to contract
    assert _same_bits(fused["pos"][early], want["pos"][early])


# ================================================================== on the GPU
def _real(name):
    from bonnie32_amd import scenefile
    return scenefile.read_scene(os.path.join(REAL, name + ".b32scene"))


def _assert_frame(fb, pixels, zbuffer, what=""):
    got = fb.pixels
    assert np.array_equal(got, pixels), f"{what}: {int((got != pixels).sum())} bytes differ"
    gz = fb.zbuffer.view(np.uint32)
    assert np.array_equal(gz, zbuffer.view(np.uint32)), f"{what}: {int((gz != zbuffer.view(np.uint32)).sum())} depths differ"


def _bones(t, scale):
    """The bone table of frame t for a mesh of extent `scale`: a rotating bone, an early return with a translation, a rotating bone
    without translation, a second rotating bone, and an early return without translation."""
    s = scale
    return RM.pack_bones([RM.Bone.from_euler((0.06 * s * np.sin(0.7 * t), 0.03 * s, -0.04 * s * np.cos(0.4 * t)), (6.0 + 3.0 * t, 0.0, -5.0 + 2.0 * t)),
                          RM.Bone.from_euler((0.35 * s - 0.02 * s * t, -0.05 * s, 0.02 * s * t), (0.0004, 30.0, 0.0)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (-4.0 - 1.5 * t, 0.0, 3.0 + t)),
                          RM.Bone.from_euler((-0.3 * s + 0.01 * s * t, 0.02 * s * t, 0.05 * s), (2.0 * t, 0.0, 9.0)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))])


def _bone_of(n, seed=5):
    """Indices 0..4 (the five bones), 5 and 6 (past the table) and B32_BONE_NONE, in runs so that neighbouring vertices share a bone."""
    rng = np.random.default_rng(seed)
    runs = rng.integers(0, 8, (n + 7) // 8 + 1).astype(np.uint16)
    bo = np.repeat(runs, 8)[:n].copy()
    bo[bo == 7] = NONE
    for k, b in enumerate((0, 1, 2, 3, 4, 5, NONE)[:n]):
        bo[(k * 31) % n] = b
    return bo


@functools.lru_cache(maxsize=None)
def _warrior():
    sc = _real("obj-warrior")
    assert len(sc.vertices) == 227
    sc.textures8 = [b32.Texture.from_texture15(t) for t in sc.textures]
    return sc, _bone_of(len(sc.vertices)), 1000.0


def _warrior_settings(mode):
    sc, _, _ = _warrior()
    st = copy.copy(sc.settings)
    if mode == "painter":                                                       # painter's mode without shading
        st.use_zbuffer = False; st.shading = abi.SHADE_NONE; st.backface_wireframe = False; st.lights = []
    elif mode == "lit_wire":                                                    # z-buffer + Gouraud + one light + back-face wireframe
        assert st.use_zbuffer and st.shading == abi.SHADE_GOURAUD and len(st.lights) == 1 and st.backface_wireframe and st.backface_cull
    elif mode == "rgba8":                                                       # the 8-bit-colour path (render_mesh)
        st.use_rgb555 = False
    return st


_EXPECT = {}


def _warrior_expect(oracle, mode, t):
    """The oracle's frame of the warrior posed with _bones(t): (pixels, zbuffer, triangles_drawn, posed vertices)."""
    key = (mode, t)
    if key not in _EXPECT:
        sc, bo, scale = _warrior()
        st = _warrior_settings(mode)
        posed = RM.pose_vertices(sc.vertices, bo, _bones(t, scale)) if t is not None else sc.vertices
        ofb = oracle.Framebuffer(W, H); ofb.clear(sc.clear_color)
        if mode == "rgba8":
            rc, tm = oracle.render_mesh(ofb, posed, sc.faces, sc.textures8, sc.camera, st)
        else:
            rc, tm = oracle.render_mesh_15(ofb, posed, sc.faces, sc.textures, sc.camera, st)
        assert rc == 0 and tm.triangles_drawn > 50
        _EXPECT[key] = (ofb.pixels.copy(), ofb.zbuffer.copy(), tm.triangles_drawn, posed)
    return _EXPECT[key]


def _warrior_scene(R, fb, mode, detached):
    sc, bo, _ = _warrior()
    rs = R.ResidentScene(fb, sc.vertices, sc.faces, textures8=sc.textures8) if mode == "rgba8" else R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
    if detached:
        rs.detach()
    rs.set_rig(bo)
    return rs


@pytest.mark.gpu
@pytest.mark.parametrize("nv", [1, 255, 256, 257, 227])
def test_read_vertices_after_a_pose(gpu_ctx, nv):
    """Test 7: the slot's vertices after a pose equal pose_vertices at one vertex, around the workgroup size and on the warrior: positions
    and normals bit for bit, uv and colour untouched, a window in the middle, and the empty table gives the uploaded vertices back."""
    from bonnie32_amd import rasterizer as R
    if nv == 227:
        sc, bo, scale = _warrior()
        v = sc.vertices
    else:
        v = scenegen.make_scene("C1", variant="gouraud").vertices[:nv].copy()
        v["pos"][::5, 1] = -0.0; v["normal"][::3, 0] = -0.0
        bo, scale = _bone_of(nv), 4000.0
    tab = _bones(1.0, scale)
    assert tab["rotate"].tolist() == [1, 0, 1, 1, 0] and not tab["pos"][2].any()
    if nv >= 227:
        assert (bo == NONE).any() and (bo == 5).any() and all((bo == k).any() for k in range(5))
    fb = R.Framebuffer(W, H, gpu_ctx)
    rs = R.ResidentScene(fb, v, b32.make_faces(0), []).detach()
    try:
        assert _same_vertices(rs.read_vertices(), v)
        rs.set_rig(bo)
        rs.pose(tab)
        want = RM.pose_vertices(v, bo, tab)
        got = rs.read_vertices()
        assert _same_vertices(got, want)
        if nv > 1:
            assert not _same_bits(got["pos"], v["pos"])
        a, n = nv // 3, max(1, nv // 2)
        assert _same_vertices(rs.read_vertices(a, n), want[a:a + n]) and len(rs.read_vertices(nv, 0)) == 0
        rs.pose(_bones(2.0, scale))                                             # from the rest stream: poses do not accumulate
        assert _same_vertices(rs.read_vertices(), RM.pose_vertices(v, bo, _bones(2.0, scale)))
        rs.pose(tab[:2])                                                        # a shorter table: indices 2, 3, 4 are now past it
        assert _same_vertices(rs.read_vertices(), RM.pose_vertices(v, bo, tab[:2]))
        rs.pose([])
        back = rs.read_vertices()
        assert back.tobytes() == np.ascontiguousarray(v).tobytes()
    finally:
        rs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("detached", [False, True], ids=["context", "slot"])
@pytest.mark.parametrize("mode", ["painter", "lit_wire", "rgba8"])
def test_posed_warrior_equals_the_oracle(oracle, mode, detached):
    """Test 8: obj-warrior posed on the device, then drawn, equals the oracle's render_mesh_15 / render_mesh on pose_vertices output:
    through the context's own scene (slot NULL) and through a detached slot."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    st = _warrior_settings(mode)
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        rs = _warrior_scene(R, fb, mode, detached)
        assert (rs._slot is None) == (not detached)
        for t in (1.0, 4.0):
            px, zb, drawn, _ = _warrior_expect(oracle, mode, t)
            rs.pose(_bones(t, scale))
            fb.clear(sc.clear_color)
            rs.render_async(sc.camera, st)
            tm = rs.finish()
            _assert_frame(fb, px, zb, f"{mode}, t = {t}")
            assert tm.triangles_drawn == drawn
        assert not np.array_equal(_warrior_expect(oracle, mode, 1.0)[0], _warrior_expect(oracle, mode, 4.0)[0])
        assert not np.array_equal(_warrior_expect(oracle, mode, 1.0)[0], _warrior_expect(oracle, mode, None)[0])
        rs.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_pose_a_b_a(oracle):
    """Test 9: pose A, draw; pose B, draw; pose A, draw -- the first and the third frame are byte-equal and each equals the oracle."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    st = _warrior_settings("lit_wire")
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        rs = _warrior_scene(R, fb, "lit_wire", True)
        frames = []
        for t in (2.0, 5.0, 2.0):
            px, zb, drawn, _ = _warrior_expect(oracle, "lit_wire", t)
            rs.pose(_bones(t, scale))
            fb.clear(sc.clear_color)
            rs.render_async(sc.camera, st)
            assert rs.finish().triangles_drawn == drawn
            _assert_frame(fb, px, zb, f"t = {t}")
            frames.append((fb.pixels.tobytes(), fb.zbuffer.tobytes()))
        assert frames[0] == frames[2] and frames[0] != frames[1]
        rs.close()
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _c2():
    sc = scenegen.make_scene("C2")
    assert len(sc.faces) == 100_000
    bo = (np.arange(len(sc.vertices)) // 3 % 7).astype(np.uint16)              # a bone per triangle; 5 and 6 are past the table
    lit = copy.copy(sc.settings)
    lit.shading = abi.SHADE_GOURAUD; lit.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7)]
    return sc, bo, lit


_C2_EXPECT = {}


def _c2_expect(oracle, t, lit):
    if (t, lit) not in _C2_EXPECT:
        sc, bo, lit_st = _c2()
        ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
        rc, tm = oracle.render_mesh_15(ofb, RM.pose_vertices(sc.vertices, bo, _bones(t, 3000.0)), sc.faces, sc.textures, sc.camera, lit_st if lit else sc.settings)
        assert rc == 0
        _C2_EXPECT[(t, lit)] = (ofb.pixels.copy(), ofb.zbuffer.copy(), tm.triangles_drawn)
    return _C2_EXPECT[(t, lit)]


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "nopacked"])
def test_pose_of_a_large_mesh_repacks_its_streams(oracle, packed):
    """Test 10: C2 (100 000 faces: from the second frame on the setup kernel reads packed position / attribute streams).  Three frames,
    then pose, draw, compare; then a lit frame (the lit stream is packed), pose again, draw, compare.  Once with the packed streams off."""
    from bonnie32_amd import rasterizer as R
    sc, bo, lit_st = _c2()
    ctx = R.Context(0)
    try:
        if not packed:
            ctx.set_routes(R.Context.ROUTE_PACKED_STREAMS)
        fb = R.Framebuffer(sc.width, sc.height, ctx)
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        rs.set_rig(bo)
        for _ in range(3):
            fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings); rs.finish()
        rs.pose(_bones(1.0, 3000.0))
        fb.clear(sc.clear_color); rs.render_async(sc.camera, sc.settings); tm = rs.finish()
        px, zb, drawn = _c2_expect(oracle, 1.0, False)
        _assert_frame(fb, px, zb, "unlit, t = 1"); assert tm.triangles_drawn == drawn
        fb.clear(sc.clear_color); rs.render_async(sc.camera, lit_st); tm = rs.finish()
        px, zb, drawn = _c2_expect(oracle, 1.0, True)
        _assert_frame(fb, px, zb, "lit, t = 1"); assert tm.triangles_drawn == drawn
        rs.pose(_bones(3.0, 3000.0))
        fb.clear(sc.clear_color); rs.render_async(sc.camera, lit_st); tm = rs.finish()
        px, zb, drawn = _c2_expect(oracle, 3.0, True)
        _assert_frame(fb, px, zb, "lit, t = 3"); assert tm.triangles_drawn == drawn
        assert not np.array_equal(px, _c2_expect(oracle, 1.0, True)[0])
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _c3():
    """More than 8192 faces (the setup kernel bins them itself, the route whose frames run two in flight), few enough for 24 oracle frames."""
    sc = scenegen.make_scene("C3", n_tris=9000, width=W, height=H, bbox_px=60.0, seed=5, variant="gouraud")
    return sc, (np.arange(len(sc.vertices)) // 3 % 7).astype(np.uint16)


_C3_EXPECT = {}


def _c3_expect(oracle, wire):
    if wire not in _C3_EXPECT:
        sc, bo = _c3()
        st = copy.copy(sc.settings); st.backface_wireframe = wire
        frames = []
        for t in range(24):
            ofb = oracle.Framebuffer(W, H); ofb.clear(sc.clear_color)
            rc, _tm = oracle.render_mesh_15(ofb, RM.pose_vertices(sc.vertices, bo, _bones(0.25 * t, 3000.0)), sc.faces, sc.textures, sc.camera, st)
            assert rc == 0
            frames.append(ofb.pixels.copy())
        assert all(not np.array_equal(frames[t], frames[t + 1]) for t in range(23))
        _C3_EXPECT[wire] = (st, frames)
    return _C3_EXPECT[wire]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["pipelined", "nopipeline", "wire"])
def test_a_pose_per_frame_in_deep_mode(oracle, how):
    """Test 11: 24 frames in deep mode, another bone table every frame, every frame delivered by ticket and compared with the oracle.
    The poses are enqueued between frames whose setup kernels run on the second stream: the pipelined run must have pipelined."""
    from bonnie32_amd import rasterizer as R
    sc, bo = _c3()
    st, want = _c3_expect(oracle, how == "wire")
    ctx = R.Context(0)
    bufs = []
    try:
        ctx.set_async_depth(1)
        if how == "nopipeline":
            ctx.set_routes(R.Context.ROUTE_PIPELINE)
        fb = R.Framebuffer(W, H, ctx)
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        rs.set_rig(bo)
        fb.clear(sc.clear_color); rs.render_async(sc.camera, st); rs.finish()   # (capacities settled by a warm-up frame, as deep mode asks)
        bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
        tickets = [0, 0]
        for t in range(24):
            rs.pose(_bones(0.25 * t, 3000.0))
            fb.clear(sc.clear_color)
            rs.render_async()
            tickets[t & 1] = ctx.download_async(bufs[t & 1][1])
            if t > 0:
                ctx.ticket_wait(tickets[(t - 1) & 1])
                got = bufs[(t - 1) & 1][0]
                assert np.array_equal(got, want[t - 1]), f"frame {t - 1}: {int((got != want[t - 1]).sum())} bytes differ"
        ctx.ticket_wait(tickets[1])
        assert np.array_equal(bufs[1][0], want[23])
        rs.finish()
        rc = ctx.route_counts()
        print(how, rc)
        if how == "nopipeline":
            assert rc["pipelined"] == 0
        else:
            assert int(ctx.lib.b32_route_count(ctx.h, 7)) > 0, rc
    finally:
        for _, p in bufs:
            ctx.host_free(p)
        ctx.close()


def _merge_quads(faces):
    """Each consecutive fan pair (a, b, c), (a, c, d) of a triangle list becomes the quad (a, b, c, d): the modeler's polygons."""
    fv = [tuple(int(i) for i in f) for f in faces["v"]]
    out, i = [], 0
    while i < len(fv):
        if i + 1 < len(fv) and fv[i][0] == fv[i + 1][0] and fv[i][2] == fv[i + 1][1]:
            out.append([fv[i][0], fv[i][1], fv[i][2], fv[i + 1][2]]); i += 2
        else:
            out.append(list(fv[i])); i += 1
    return out


def _canon(r):
    return tuple(int(np.asarray(r[k]).view(np.uint32)) if k in ("vertex_dist", "edge_dist", "face_depth") else int(r[k])
                 for k in ("vertex", "vertex_dist", "edge_v0", "edge_v1", "edge_dist", "face", "face_depth"))


@pytest.mark.gpu
def test_hover_box_select_and_pick_on_a_posed_slot(gpu_ctx):
    """Test 12: hover (mirror axis X: tested on the REST position while the posed one is projected), box selection and pick of a rigged,
    posed obj-warrior equal the host mirrors on pose_vertices output; an un-rigged slot in the same context is unchanged."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    cam, w, h = sc.camera, sc.width, sc.height
    tab = _bones(3.0, scale)
    rest = sc.vertices
    posed = RM.pose_vertices(rest, bo, tab)
    top = R.Topology.from_polygons(_merge_quads(sc.faces))
    right = R.HoverMirror(posed, top, None, cam, w, h, local_vertices=rest)
    wrong = R.HoverMirror(posed, top, None, cam, w, h)                          # the mirror plane tested on the posed position
    plain = R.HoverMirror(rest, top, None, cam, w, h)
    ok = np.nonzero(right.some)[0]
    assert len(ok) > 100
    offs = [(0.0, 0.0), (1.5, -1.0), (-2.5, 2.0), (4.0, 3.0)]
    curs = [(float(right.sx[i]) + offs[k % 4][0], float(right.sy[i]) + offs[k % 4][1]) for k, i in enumerate(ok[(np.arange(48) * 5) % len(ok)])]
    prm = dict(mirror_axis=1, mirror_threshold=0.0)
    fb = R.Framebuffer(w, h, gpu_ctx)
    rs = R.ResidentScene(fb, rest, sc.faces, sc.textures).detach()
    un = R.ResidentScene(fb, rest, sc.faces, sc.textures).detach()
    try:
        before = [_canon(gpu_ctx.hover_mesh(un, top, cam, c, see_through=see, **prm)) for c in curs[:12] for see in (False, True)]
        assert before == [_canon(plain.hover(*c, see_through=see, **prm)) for c in curs[:12] for see in (False, True)]
        rs.set_rig(bo)
        rs.pose(tab)
        n_differ = n_hit = 0
        for see in (False, True):
            for c in curs:
                want = right.hover(*c, see_through=see, **prm)
                got = gpu_ctx.hover_mesh(rs, top, cam, c, see_through=see, **prm)
                assert _canon(got) == _canon(want), (see, c, got, want)
                n_differ += _canon(wrong.hover(*c, see_through=see, **prm)) != _canon(want)
                n_hit += R.hovered_element(want) != (None, None, None)
                nomirror = right.hover(*c, see_through=see)                     # mirror off: the rest stream is not consulted
                assert _canon(gpu_ctx.hover_mesh(rs, top, cam, c, see_through=see)) == _canon(nomirror)
        print("cursors answered:", n_hit, "answers a mirror test on the posed position would change:", n_differ)
        assert n_hit >= 20 and n_differ >= 1
        # box selection reads the posed vertices
        for rect in ((0.0, 0.0, w * 0.55, h * 0.6), (w * 0.4, h * 0.3, w * 0.7, h * 0.9), (0.0, 0.0, float(w), float(h))):
            for mode in (abi.BOX_VERTICES, abi.BOX_POLYGONS):
                want_w, want_n = R.box_select_mesh(posed, top, None, cam, w, h, rect, mode)
                words, cnt = gpu_ctx.box_select(rs, top, cam, rect, mode)
                assert cnt == want_n and np.array_equal(words, want_w), (rect, mode)
                rest_w, _ = R.box_select_mesh(rest, top, None, cam, w, h, rect, mode)
                if rect[2] < w and mode == abi.BOX_VERTICES:
                    assert not np.array_equal(want_w, rest_w)                   # (the pose moved vertices across the rectangle's border)
        # pick with a placement on top: pose first, placement second
        pl = b32.Placement(facing=0.3, world_pos=(40.0, -25.0, 60.0))
        pm = R.PickMirror(posed, sc.faces, pl, cam, w, h)
        hm = R.HoverMirror(posed, top, pl, cam, w, h)
        n_pick = 0
        for k in range(0, 48, 3):
            c = (float(hm.sx[ok[k]]) + 2.0, float(hm.sy[ok[k]]) + 1.0)
            best, hits = gpu_ctx.pick_meshes([(rs, pl), (un, pl)], cam, c)
            want = pm.pick(*c)
            got = (bool(hits[0]["hit"]), int(hits[0]["tri"]), hits[0]["depth"])
            assert got[0] == want[0] and got[1] == want[1] and _same_bits(np.array([got[2]], f32), np.array([want[2]], f32)), (c, got, want)
            n_pick += want[0]
        assert n_pick >= 4
        # the un-rigged slot answers as before
        assert before == [_canon(gpu_ctx.hover_mesh(un, top, cam, c, see_through=see, **prm)) for c in curs[:12] for see in (False, True)]
        rs.pose([])
        assert _same_vertices(rs.read_vertices(), rest)
    finally:
        rs.close(); un.close(); top.close()


@pytest.mark.gpu
def test_posed_slot_beside_another_in_a_batched_frame(oracle):
    """Test 13: a posed slot and a second slot in b32_frame_submit: the frame equals the sequential oracle calls, also after a second
    pose, and each pose costs exactly one rebuild of the merged mesh."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    other = _real("obj-ghost-game")
    st = b32.RasterSettings.game()
    st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7)]
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        a = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).detach()
        b = R.ResidentScene(fb, other.vertices, other.faces, other.textures).detach()
        a.set_rig(bo)
        table = ctx.make_frame_table(sc.camera, st, [a, b])
        built = []
        for t in (1.0, 1.0, 4.0):
            if not built or t != 1.0:
                a.pose(_bones(t, scale))
            fb.clear(sc.clear_color)
            ctx.frame_submit(table)
            ctx.finish()
            built.append(ctx.batch_counts()["merged_built"])
            ofb = oracle.Framebuffer(W, H); ofb.clear(sc.clear_color)
            for m, v in ((sc, RM.pose_vertices(sc.vertices, bo, _bones(t, scale))), (other, other.vertices)):
                rc, _tm = oracle.render_mesh_15(ofb, v, m.faces, m.textures, sc.camera, st)
                assert rc == 0
            _assert_frame(fb, ofb.pixels, ofb.zbuffer, f"t = {t}")
        assert ctx.batch_counts()["merged_draws"] == 3, ctx.batch_counts()
        assert built[1] == built[0] and built[2] == built[1] + 1, built       # no pose, no rebuild; one pose, one rebuild
        a.close(); b.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_pose_errors_and_lifetime():
    """Test 14: the error returns, the rig travelling with b32_scene_swap and dropped by an upload, and a pose that touches neither the
    framebuffer nor a deferred clear."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    tab = _bones(1.0, scale)
    ctx = R.Context(0)
    lib, E, U = ctx.lib, abi.B32_E_ARG, abi.B32_E_UNSUPPORTED
    try:
        fb = R.Framebuffer(W, H, ctx)
        empty = C.c_void_p()
        assert lib.b32_scene_create(ctx.h, C.byref(empty)) == 0
        big = np.zeros(65, abi.BONE_DTYPE)
        # no scene: in the context, in a slot
        assert lib.b32_scene_set_rig(ctx.h, None, abi.ptr(bo)) == E and lib.b32_scene_set_rig(ctx.h, empty, abi.ptr(bo)) == E
        assert lib.b32_scene_pose(ctx.h, None, abi.ptr(tab), 5) == E and lib.b32_scene_pose(ctx.h, empty, abi.ptr(tab), 5) == E
        assert lib.b32_scene_read_vertices(ctx.h, empty, 0, 0, None) == E
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        out = np.zeros(4, abi.VERTEX_DTYPE)
        assert lib.b32_scene_pose(ctx.h, None, abi.ptr(tab), 5) == E            # no rig yet
        assert lib.b32_scene_set_rig(ctx.h, None, None) == E
        assert lib.b32_scene_read_vertices(ctx.h, None, 225, 3, abi.ptr(out)) == E and lib.b32_scene_read_vertices(ctx.h, None, 0, 2, None) == E
        assert lib.b32_scene_read_vertices(ctx.h, None, 0xFFFFFFFF, 2, abi.ptr(out)) == E
        assert lib.b32_scene_read_vertices(ctx.h, None, 225, 2, abi.ptr(out)) == 0 and out[:2].tobytes() == sc.vertices[225:].tobytes()
        rs.set_rig(bo)
        assert lib.b32_scene_pose(ctx.h, None, None, 3) == E
        assert lib.b32_scene_pose(ctx.h, None, abi.ptr(big), 65) == U
        assert lib.b32_scene_pose(ctx.h, None, abi.ptr(big), 64) == 0 and lib.b32_scene_pose(ctx.h, None, None, 0) == 0
        assert _same_vertices(rs.read_vertices(), sc.vertices)
        # the rig travels with b32_scene_swap
        rs.detach()
        assert lib.b32_scene_pose(ctx.h, None, abi.ptr(tab), 5) == E            # the context holds no scene now
        rs.pose(tab)
        want = RM.pose_vertices(sc.vertices, bo, tab)
        assert _same_vertices(rs.read_vertices(), want)
        # a pose changes no pixel and flushes no deferred clear
        st = _warrior_settings("lit_wire")
        fb.clear(sc.clear_color); rs.render_async(sc.camera, st); rs.finish()
        before = (fb.pixels.tobytes(), fb.zbuffer.tobytes())
        rs.pose(_bones(2.0, scale))
        assert (fb.pixels.tobytes(), fb.zbuffer.tobytes()) == before
        fb.clear(b32.Color(200, 10, 10))                                        # deferred: applied by whatever touches the framebuffer next
        rs.pose(_bones(3.0, scale))
        assert ctx.lib.b32_scene_read_vertices(ctx.h, rs._slot, 0, 4, abi.ptr(out)) == 0
        rs.render_async(sc.camera, st); rs.finish()
        ref = (fb.pixels.tobytes(), fb.zbuffer.tobytes())
        fb.clear(b32.Color(200, 10, 10)); rs.render_async(sc.camera, st); rs.finish()
        assert (fb.pixels.tobytes(), fb.zbuffer.tobytes()) == ref and ref != before
        # a second set_rig takes the vertices as they are now for the rest pose
        rs.pose(tab)
        rs.set_rig(bo)
        rs.pose([])
        assert _same_vertices(rs.read_vertices(), want)
        # an upload into the scene drops the rig
        rs._swap()
        v2 = sc.vertices.copy()
        assert lib.b32_scene_upload(ctx.h, abi.ptr(v2), len(v2), abi.ptr(np.ascontiguousarray(sc.faces)), len(sc.faces), None, 0) == 0
        assert lib.b32_scene_pose(ctx.h, None, abi.ptr(tab), 5) == E
        rs._swap()
        assert lib.b32_scene_pose(ctx.h, rs._slot, abi.ptr(tab), 5) == E
        rs.close()
        lib.b32_scene_destroy(ctx.h, empty)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_cpp_pose_harness(tmp_path):
    """Test 15: tests/cpp/pose_harness.cpp -- a golden scene file through the C++ mirror's set_rig / pose / read_vertices on the device and
    through its host pose_vertices (compiled without contraction), both against the Python mirror."""
    import __graft_entry__ as g
    g.build()
    sc, _, scale = _warrior()
    exe = tmp_path / "pose_harness"
    lib_dir = os.path.join(ROOT, "bonnie-32_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bonnie-32_amd", "host"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "pose_harness.cpp"), "-o", str(exe), "-L", lib_dir, "-lb32raster", f"-Wl,-rpath,{lib_dir}"], check=True)
    tab = _bones(2.0, scale)
    nb = len(tab)
    args = []
    for b in tab:
        args += [float(x).hex() for x in b["pos"]] + [float(b[k]).hex() for k in ("cos_x", "sin_x", "cos_z", "sin_z")] + [str(int(b["rotate"]))]
    r = subprocess.run([str(exe), os.path.join(REAL, "obj-warrior.b32scene"), str(nb)] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    i = np.arange(len(sc.vertices)) % (nb + 2)
    bo = np.where(i == nb + 1, NONE, i).astype(np.uint16)
    want = RM.pose_vertices(sc.vertices, bo, tab)
    wbits = np.concatenate([want["pos"], want["normal"]], axis=1).view(np.uint32)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(sc.vertices)
    for k, line in enumerate(lines):
        dev, host = (np.array([int(x, 16) for x in part.split()], np.uint32) for part in line.split("|"))
        for got in (dev, host):
            assert np.all((got == wbits[k]) | (np.isnan(got.view(f32)) & np.isnan(wbits[k].view(f32)))), (k, line)
