"""Editing a resident scene in place: b32_scene_patch_vertices / _faces / _texels / _indexed and b32_scene_read_texels.

The modeler changes its mesh on the host and hands all of it to the rasterizer again; the library changes the resident copy.  The
contract is that a patched slot is indistinguishable from a slot into which the patched arrays were uploaded afresh (followed by the same
rig, pose and skeleton), so every expected value here is the host composition: the numpy mirrors (rasterizer.patch_*) patch host arrays,
and the frame is the oracle's render of those arrays, and what a fresh upload of them gives.  Comparisons are bit for bit: pixels, the
depth buffer as u32, triangles_drawn, the draw order and the transparent counts."""
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
CSRC = os.path.join(ROOT, "bonnie-32_amd", "csrc")
f32 = np.float32
NONE = abi.BONE_NONE
W, H = 320, 240
U32 = C.c_uint32


# ================================================================== without a GPU
# ---------------------------------------------------------------- the host build of the device header, lane by lane
HOST_SRC = r'''
#include <vector>
#include "b32_patch_body.h"
#include "b32_patch_tally.h"
using namespace b32;
extern "C" {
void h_vertices(const uint32_t* recs, uint32_t n, uint32_t* verts, uint32_t* rest, const uint16_t* bone_of, const B32Bone* bones, uint32_t n_bones) {
    for (uint32_t t = 0; t < n; ++t) {
        const uint32_t* rec = recs + (size_t)t * PATCH_VERTEX_WORDS;
        const B32Bone* bone = nullptr;
        if (rest) { const uint32_t b = bone_of[rec[0]]; if (patch_has_bone(b, n_bones)) bone = &bones[b]; }
        patch_vertex(rec, verts, rest, bone);
    }
}
void h_faces(const uint32_t* recs, uint32_t n, uint32_t* faces) { for (uint32_t t = 0; t < n; ++t) patch_face(recs + (size_t)t * PATCH_FACE_WORDS, faces); }
void h_texels(uint32_t elem, uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t tex_w, uint32_t offset, const void* src, uint32_t stride, void* pool) {
    std::vector<unsigned char> packed((size_t)w * h * elem + 4);
    patch_pack_rect(src, stride, w, h, elem, packed.data());
    const PatchRect r{ x, y, w, h, tex_w, offset };
    for (uint32_t t = 0; t < w * h; ++t) {
        if (elem == 2) patch_texel(r, t, reinterpret_cast<const uint16_t*>(packed.data()), static_cast<uint16_t*>(pool));
        else patch_texel(r, t, reinterpret_cast<const uint32_t*>(packed.data()), static_cast<uint32_t*>(pool));
    }
}
void h_indexed(uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t tex_w, uint32_t offset, const uint8_t* idx, uint32_t stride, const uint16_t* clut, uint32_t clut_len,
               uint16_t* pool, uint8_t* kept_idx, uint16_t* kept_clut) {
    std::vector<uint8_t> packed((size_t)w * h + 4);
    patch_pack_rect(idx, stride, w, h, 1, packed.data());
    uint16_t padded[PATCH_CLUT_ENTRIES] = {};
    const uint32_t len = clut_len < PATCH_CLUT_ENTRIES ? clut_len : PATCH_CLUT_ENTRIES;
    for (uint32_t k = 0; k < len; ++k) padded[k] = clut[k];
    const PatchRect r{ x, y, w, h, tex_w, offset };
    for (uint32_t t = 0; t < w * h; ++t) patch_indexed_texel(r, t, packed.data(), padded, len, pool, kept_idx);
    if (kept_clut) for (uint32_t t = 0; t < PATCH_CLUT_ENTRIES; ++t) patch_kept_clut(t, padded, len, kept_clut);
}
int h_records_ok(const void* recs, uint32_t rec_bytes, uint32_t n, uint32_t limit) { return patch_records_ok(recs, rec_bytes, n, limit) ? 1 : 0; }
int h_rect_ok(uint32_t x, uint32_t y, uint32_t w, uint32_t h, uint32_t tw, uint32_t th) { return patch_rect_ok(x, y, w, h, tw, th) ? 1 : 0; }
// the tally: faces and tally3 = {own, any, alpha} are updated in place by a patch, as b32_scene_patch_faces does
void h_tally(const B32Face* f, uint32_t nf, const uint32_t* tex_blend, uint32_t nt, uint32_t* tally3) {
    const FaceTally t = tally_faces(f, nf, [&](uint32_t k) { return k < nt && tex_blend[k] != B32_BLEND_OPAQUE; });
    tally3[0] = t.own; tally3[1] = t.any; tally3[2] = t.alpha;
}
void h_tally_patch(B32Face* faces, uint32_t* tally3, const B32FacePatch* recs, uint32_t n, const uint32_t* tex_blend, uint32_t nt) {
    FaceTally t; t.own = tally3[0]; t.any = tally3[1]; t.alpha = tally3[2];
    const auto blends = [&](uint32_t k) { return k < nt && tex_blend[k] != B32_BLEND_OPAQUE; };
    for (uint32_t k = 0; k < n; ++k) { B32Face& f = faces[recs[k].index]; tally_face(t, f, false, blends); f = recs[k].f; tally_face(t, f, true, blends); }
    tally3[0] = t.own; tally3[1] = t.any; tally3[2] = t.alpha;
}
// state6 = {may_blend, blend8, blend_faces, body_may_blend, body_blend8, body_blend_faces}, in and out
void h_tally_slot(const uint32_t* tally3, uint32_t* state6, int fmt8, int any_texture_blends, int blend_texels8, int has_tail) {
    FaceTally t; t.own = tally3[0]; t.any = tally3[1]; t.alpha = tally3[2];
    const SlotBlend cur{ state6[0] != 0, state6[1] != 0, state6[2], state6[3] != 0, state6[4] != 0, state6[5] };
    const SlotBlend s = tally_slot(t, cur, fmt8 != 0, any_texture_blends != 0, blend_texels8 != 0, has_tail != 0);
    state6[0] = s.may_blend; state6[1] = s.blend8; state6[2] = s.blend_faces; state6[3] = s.body_may_blend; state6[4] = s.body_blend8; state6[5] = s.body_blend_faces;
}
// what upload_geometry does with the faces of an upload: one tally_faces pass, then blend_fresh on what the slot held (state6, in and out)
void h_fresh_upload(const B32Face* f, uint32_t nf, const uint32_t* tex_blend, uint32_t nt, uint32_t* state6, int fmt8, int blend_texels8) {
    bool any_texture_blends = false;
    for (uint32_t k = 0; k < nt; ++k) any_texture_blends |= tex_blend[k] != B32_BLEND_OPAQUE;
    const FaceTally t = tally_faces(f, nf, [&](uint32_t k) { return k < nt && tex_blend[k] != B32_BLEND_OPAQUE; });
    const SlotBlend cur{ state6[0] != 0, state6[1] != 0, state6[2], state6[3] != 0, state6[4] != 0, state6[5] };
    const SlotBlend s = blend_fresh(t, cur, fmt8 != 0, any_texture_blends, blend_texels8 != 0);
    state6[0] = s.may_blend; state6[1] = s.blend8; state6[2] = s.blend_faces; state6[3] = s.body_may_blend; state6[4] = s.body_blend8; state6[5] = s.body_blend_faces;
}
}
'''
# (g++ forms fused multiply-adds from -O2 on, and only where the target has them)
HOST_FLAGS = {"off": ["-O1", "-ffp-contract=off"], "fused": ["-O2", "-ffp-contract=fast", "-mfma"]}


@functools.lru_cache(maxsize=None)
def _host(mode="off"):
    d = tempfile.mkdtemp(prefix="b32_patch_host_")
    atexit.register(shutil.rmtree, d, True)
    src, so = os.path.join(d, "patch_host.cpp"), os.path.join(d, "patch_host_%s.so" % mode)
    open(src, "w").write(HOST_SRC)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC"] + HOST_FLAGS[mode] + ["-I", CSRC, src, "-o", so], check=True)
    return C.CDLL(so)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _same_bits(a, b):
    """bit for bit, except that any NaN equals any NaN (the payload of an invalid operation is not the reference's business)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _same_vertices(a, b):
    return (len(a) == len(b) and _same_bits(a["pos"], b["pos"]) and _same_bits(a["normal"], b["normal"])
            and np.array_equal(a["uv"].view(np.uint32), b["uv"].view(np.uint32)) and all(np.array_equal(a[k], b[k]) for k in ("r", "g", "b", "blend")))


def _random_vertices(rng, n, scale):
    v = np.zeros(n, abi.VERTEX_DTYPE)
    v["pos"] = (rng.standard_normal((n, 3)) * scale).astype(f32)
    v["uv"] = rng.random((n, 2)).astype(f32)
    nrm = rng.standard_normal((n, 3)).astype(f32)
    v["normal"] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True).astype(f32)
    for k in ("r", "g", "b", "blend"):
        v[k] = rng.integers(0, 256, n).astype(np.uint8)
    return v


def _table5(scale=1.0):
    """Five bones: rotating, rotate_by_euler's early return, rotating without translation, a second rotating one, early return without
    translation."""
    s = scale
    return RM.pack_bones([RM.Bone.from_euler((12.5 * s, -3.25 * s, 40.0 * s), (33.0, 10.0, -71.5)),
                          RM.Bone.from_euler((-7.0 * s, 2.5 * s, 0.125 * s), (0.0005, 45.0, -0.0005)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (-12.0, 0.0, 0.25)),
                          RM.Bone.from_euler((1.0 * s, 100.0 * s, -50.0 * s), (0.0, 0.0, 179.0)),
                          RM.Bone.from_euler((0.0, -0.0, 0.0), (0.0, 90.0, 0.0))])


def _vertex_records(indices, vertices):
    recs = np.zeros(len(indices), abi.VERTEX_PATCH_DTYPE)
    recs["index"] = indices; recs["v"] = vertices
    return recs


def _host_vertices(lib, verts, idx, recs, rest=None, bo=None, tab=None):
    v = np.ascontiguousarray(verts).copy()
    r = None if rest is None else np.ascontiguousarray(rest, f32).copy()
    rr = _vertex_records(idx, recs)
    tab = np.zeros(0, abi.BONE_DTYPE) if tab is None else np.ascontiguousarray(tab)
    bo = None if bo is None else np.ascontiguousarray(bo, np.uint16)
    lib.h_vertices(_p(rr), U32(len(rr)), _p(v), _p(r), _p(bo), _p(tab) if len(tab) else None, U32(len(tab)))
    return v, r


COUNTS = (0, 1, 63, 64, 65, 257)


def _ascending(rng, n, limit):
    return np.sort(rng.choice(limit, n, replace=False)).astype(np.uint32)


def _special_records(rng, n):
    """Records whose positions and normals include NaN, infinities and zeros of both signs."""
    recs = _random_vertices(rng, n, 300.0)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -3e38], f32)
    if n:
        recs["pos"][::3, 0] = special[np.arange(len(recs[::3])) % len(special)]
        recs["normal"][::4, 2] = special[(np.arange(len(recs[::4])) + 3) % len(special)]
    return recs


@pytest.mark.parametrize("n", COUNTS)
def test_vertex_lane_equals_the_mirror(n):
    """CPU test 1, vertices: b32_patch_body.h built for the host, driven record by record, equals rasterizer.patch_vertices bit for bit on
    an unrigged slot (NaN, infinities, -0.0 copied as they are) and on a rigged one (every bone of the table, B32_BONE_NONE, an index past
    the table; a table of none: "copy")."""
    lib = _host()
    rng = np.random.default_rng(100 + n)
    nv = 300
    verts = _random_vertices(rng, nv, 500.0)
    idx = _ascending(rng, n, nv)
    recs = _special_records(rng, n)
    got, _ = _host_vertices(lib, verts, idx, recs)
    want = RM.patch_vertices(verts, idx, recs)
    assert got.tobytes() == want.tobytes()                                      # whole records, NaN payloads included
    if n:
        assert got.tobytes() != verts.tobytes() and np.isnan(got["pos"]).any() == (n > 0)
    # rigged: finite records (an invalid operation's NaN payload is the machine's), bones 0..4, 5 and 6 past the table, NONE
    bo = (np.arange(nv) % 8).astype(np.uint16); bo[bo == 7] = NONE
    rest = RM.rest_stream(verts)
    tab = _table5()
    posed = RM.pose_vertices(verts, bo, tab)
    recs = _random_vertices(rng, n, 500.0)
    if n:
        recs["pos"][0] = (-0.0, 0.0, -0.0)                                      # (an early-return bone without translation: -0.0 + 0.0)
    got_v, got_r = _host_vertices(lib, posed, idx, recs, rest, bo, tab)
    want_v, want_r = RM.patch_vertices(posed, idx, recs, rest=rest, bone_of_vertex=bo, bones=tab)
    assert _same_vertices(got_v, want_v) and got_r.tobytes() == want_r.tobytes()
    # the composition the contract names: patch the rest arrays, pose them afresh
    fresh_rest = RM.patch_vertices(verts, idx, recs)
    assert _same_vertices(want_v, RM.pose_vertices(fresh_rest, bo, tab)) and want_r.tobytes() == RM.rest_stream(fresh_rest).tobytes()
    if n >= 63:
        moved = (bo[idx] < 5) & (bo[idx] != 4)
        assert moved.any() and not _same_bits(want_v["pos"][idx[moved]], recs["pos"][moved])
        out = bo[idx] >= 5
        assert out.any() and _same_bits(want_v["pos"][idx[out]], recs["pos"][out])
    # before the first pose / after a pose with no bones: the rule is "copy"
    got_v, got_r = _host_vertices(lib, verts, idx, recs, rest, bo, None)
    want_v, want_r = RM.patch_vertices(verts, idx, recs, rest=rest, bone_of_vertex=bo, bones=[])
    assert got_v.tobytes() == want_v.tobytes() == RM.patch_vertices(verts, idx, recs).tobytes() and got_r.tobytes() == want_r.tobytes()


def test_rigged_lane_built_with_contraction_differs():
    """CPU test 1, the rigged case under FMA contraction: on a fixed set of finite records the separately rounded build equals the mirror
    and the contracted build does not (only under the rotating bones)."""
    rng = np.random.default_rng(33)
    nv = 4000
    verts = _random_vertices(rng, nv, 500.0)
    recs = _random_vertices(rng, nv, 500.0)
    idx = np.arange(nv, dtype=np.uint32)
    bo = (idx % 7).astype(np.uint16)
    tab = _table5()
    rest = RM.rest_stream(verts)
    want_v, want_r = RM.patch_vertices(verts, idx, recs, rest=rest, bone_of_vertex=bo, bones=tab)
    got_v, got_r = _host_vertices(_host("off"), verts, idx, recs, rest, bo, tab)
    assert _same_vertices(got_v, want_v) and got_r.tobytes() == want_r.tobytes()
    fused_v, fused_r = _host_vertices(_host("fused"), verts, idx, recs, rest, bo, tab)
    differ = (fused_v["pos"].view(np.uint32) != want_v["pos"].view(np.uint32)).any(axis=1)
    print("vertices a contracted build patches differently:", int(differ.sum()), "of", nv)
    assert differ.sum() >= 1 and not differ[~np.isin(bo, [0, 2, 3])].any() and fused_r.tobytes() == want_r.tobytes()


def _random_faces(rng, n, nv=1000, nt=3):
    f = np.zeros(n, abi.FACE_DTYPE)
    f["v"] = rng.integers(0, nv, (n, 3))
    f["texture_id"] = rng.choice(np.array(list(range(nt)) + [nt + 5, abi.NO_TEXTURE], np.uint32), n)     # resolves / out of range / none
    f["black_transparent"] = rng.integers(0, 2, n)
    f["blend_mode"] = np.where(rng.random(n) < 0.5, abi.OPAQUE, rng.integers(0, 6, n))
    f["editor_alpha"] = rng.choice(np.array([0, 100, 254, 255, 255, 255], np.uint8), n)
    f["_pad"] = rng.integers(0, 256, n)
    return f


def _face_records(indices, faces):
    recs = np.zeros(len(indices), abi.FACE_PATCH_DTYPE)
    recs["index"] = indices; recs["f"] = faces
    return recs


@pytest.mark.parametrize("n", COUNTS)
def test_face_lane_equals_the_mirror(n):
    """CPU test 1, faces: the whole record, padding byte included."""
    rng = np.random.default_rng(200 + n)
    faces = _random_faces(rng, 300)
    idx = _ascending(rng, n, len(faces))
    recs = _random_faces(rng, n)
    got = faces.copy()
    rr = _face_records(idx, recs)
    _host().h_faces(_p(rr), U32(n), _p(got))
    want = RM.patch_faces(faces, idx, recs)
    assert got.tobytes() == want.tobytes() and (n == 0) == (got.tobytes() == faces.tobytes())


# (texture width, height, x, y, w, h): 1x1, 1xh, wx1, odd widths at odd x, rectangles ending at the last texel, whole textures
RECTS = [(4, 4, 3, 3, 1, 1), (3, 5, 1, 0, 1, 5), (3, 5, 0, 4, 3, 1), (64, 64, 7, 3, 5, 9), (64, 64, 61, 1, 3, 63), (64, 64, 1, 63, 63, 1),
         (1, 1, 0, 0, 1, 1), (4, 4, 0, 0, 4, 4), (3, 5, 0, 0, 3, 5), (64, 64, 0, 0, 64, 64)]


def _pool_of(rng, tw, th, dtype):
    """A pool of three textures -- 5x3 in front, the one under test, 4x4 behind -- each padded to 8 texels, and the middle one's offset."""
    sizes = [15, tw * th, 16]
    offs = np.cumsum([0] + [(s + 7) & ~7 for s in sizes])
    hi = 1 << (8 * np.dtype(dtype).itemsize)
    return rng.integers(1, hi, int(offs[-1]) + 8).astype(dtype), int(offs[1])


@pytest.mark.parametrize("rect", RECTS, ids=lambda r: "%dx%d_at_%d_%d_%dx%d" % r)
def test_texel_lanes_equal_the_mirror(rect):
    """CPU test 1, texels: Color15 and Color rectangles from a caller's array with a stride of its own, into the middle texture of a
    pool; nothing outside the rectangle changes (not the padding behind the texture, not the next texture's first texel)."""
    tw, th, x, y, w, h = rect
    lib = _host()
    for dtype in (np.uint16, np.uint32):
        rng = np.random.default_rng(300 + tw + 7 * x + w)
        pool, off = _pool_of(rng, tw, th, dtype)
        stride = w + 3
        big = rng.integers(0, 1 << 16, (h, stride)).astype(dtype)
        block = big[:, :w]
        got = pool.copy()
        lib.h_texels(U32(pool.itemsize), U32(x), U32(y), U32(w), U32(h), U32(tw), U32(off), _p(big), U32(stride), _p(got))
        tex = pool[off:off + tw * th].reshape(th, tw)
        want = pool.copy(); want[off:off + tw * th] = RM.patch_texels(tex, x, y, block).reshape(-1)
        assert np.array_equal(got, want) and not np.array_equal(got, pool)
        assert np.array_equal(got[:off], pool[:off]) and np.array_equal(got[off + tw * th:], pool[off + tw * th:])


@pytest.mark.parametrize("rect", RECTS, ids=lambda r: "%dx%d_at_%d_%d_%dx%d" % r)
def test_indexed_lanes_equal_the_mirror(rect):
    """CPU test 1, indices: Clut::lookup into the pool (indices past a 16-entry palette give 0x0000), the kept index bytes, and the kept
    CLUT zero-filled behind a shorter palette."""
    tw, th, x, y, w, h = rect
    lib = _host()
    rng = np.random.default_rng(400 + tw + 7 * x + w)
    pool, off = _pool_of(rng, tw, th, np.uint16)
    atlas = rng.integers(0, 256, tw * th).astype(np.uint8)
    stride = w + 5
    big = rng.integers(0, 20, (h, stride)).astype(np.uint8); big[0, 0] = 255; big[-1, w - 1] = 16
    clut = rng.integers(1, 1 << 16, 16).astype(np.uint16)
    old_clut = rng.integers(1, 1 << 16, 256).astype(np.uint16)
    got, got_atlas, got_clut = pool.copy(), atlas.copy(), old_clut.copy()
    lib.h_indexed(U32(x), U32(y), U32(w), U32(h), U32(tw), U32(off), _p(big), U32(stride), _p(clut), U32(16), _p(got), _p(got_atlas), _p(got_clut))
    t2, a2 = RM.patch_indexed(pool[off:off + tw * th].reshape(th, tw), atlas.reshape(th, tw), x, y, big[:, :w], clut)
    want = pool.copy(); want[off:off + tw * th] = t2.reshape(-1)
    assert np.array_equal(got, want) and np.array_equal(got_atlas, a2.reshape(-1)) and np.array_equal(got_clut, RM.kept_clut(clut))
    assert got[off + y * tw + x] == 0 and not got_clut[16:].any()               # index 255 under 16 entries; the kept CLUT's tail
    assert np.array_equal(RM.clut_lookup(clut, [0, 15, 16, 255]), [clut[0], clut[15], 0, 0])
    # without a kept atlas only the pool is written
    got2 = pool.copy()
    lib.h_indexed(U32(x), U32(y), U32(w), U32(h), U32(tw), U32(off), _p(big), U32(stride), _p(clut), U32(16), _p(got2), None, None)
    assert np.array_equal(got2, want)


def test_record_rules():
    """Strictly ascending indices below the limit; rectangles inside the texture; the mirrors refuse what the library refuses."""
    lib = _host()
    def ok(idx, limit):
        r = _face_records(np.array(idx, np.uint32), _random_faces(np.random.default_rng(1), len(idx)))
        return bool(lib.h_records_ok(_p(r), U32(24), U32(len(idx)), U32(limit)))
    assert ok([], 0) and ok([0], 1) and ok([0, 1, 5], 6) and ok([4294967294], 4294967295)
    assert not ok([0], 0) and not ok([0, 0], 5) and not ok([2, 1], 5) and not ok([0, 5], 5) and not ok([1, 3, 3], 9)
    for idx, limit in (([0, 0], 5), ([2, 1], 5), ([0, 5], 5)):
        with pytest.raises(ValueError):
            RM.patch_indices(idx, limit)
    R = lambda *a: bool(lib.h_rect_ok(*[U32(k) for k in a]))
    assert R(0, 0, 4, 4, 4, 4) and R(3, 4, 1, 1, 4, 5) and not R(0, 0, 5, 1, 4, 4) and not R(4, 0, 1, 1, 4, 4) and not R(0, 3, 1, 2, 4, 4)
    assert not R(0, 0, 0, 1, 4, 4) and not R(0xFFFFFFFF, 0, 2, 1, 4, 4) and not R(1, 1, 0xFFFFFFFF, 1, 4, 4)
    with pytest.raises(ValueError):
        RM.patch_texels(np.zeros((4, 4), np.uint16), 3, 0, np.zeros((1, 2), np.uint16))


# ---------------------------------------------------------------- the tally
def _scratch_state(faces, tex_blend, fmt8, blend_texels8, tail_alpha=None):
    """upload_geometry / b32_scene_upload[_rgba] / b32_scene_build_skeleton restated: the slot's bookkeeping for these body faces and a
    tail of octahedra with these alphas (None: no tail).  Returns (may_blend, blend8, blend_faces) -- blend8 only means something on an
    8-bit-colour scene and may_blend only on an RGB555 one."""
    nt = len(tex_blend)
    own = (faces["blend_mode"] != abi.OPAQUE) | (faces["editor_alpha"] < 255)
    t = faces["texture_id"].astype(np.int64)
    texb = np.array([ti != abi.NO_TEXTURE and ti < nt and tex_blend[ti] != abi.OPAQUE for ti in t], bool) if len(t) else np.zeros(0, bool)
    blend_faces = int((own | texb).sum())
    may_blend = (not fmt8) and (bool(own.any()) or any(b != abi.OPAQUE for b in tex_blend))
    blend8 = bool(fmt8 and (blend_texels8 or (faces["editor_alpha"] < 255).any()))
    if tail_alpha is not None:
        nb = 8 * sum(1 for a in tail_alpha if a < 255)
        blend_faces += nb
        if fmt8:
            blend8 = blend8 or nb != 0
        else:
            may_blend = may_blend or nb != 0
    return may_blend, blend8, blend_faces


def _tally3(lib, faces, tex_blend):
    out = np.zeros(3, np.uint32)
    tb = np.ascontiguousarray(tex_blend, np.uint32)
    lib.h_tally(_p(faces), U32(len(faces)), _p(tb), U32(len(tb)), _p(out))
    return out


def _walk(lib, faces, tex_blend, fmt8, blend_texels8, tail_alpha, patches):
    """Upload `faces`, build the tail, then apply `patches` (index arrays with their records) incrementally; after every step the slot's
    state must be what a fresh upload of the faces patched so far (and the same tail) gives."""
    tb = np.ascontiguousarray(tex_blend, np.uint32)
    host = faces.copy()
    tally = _tally3(lib, host, tb)
    body = _scratch_state(host, tex_blend, fmt8, blend_texels8)
    slot = _scratch_state(host, tex_blend, fmt8, blend_texels8, tail_alpha)
    has_tail = tail_alpha is not None
    state = np.array([slot[0], slot[1], slot[2], body[0], body[1], body[2]] if has_tail else [slot[0], slot[1], slot[2], 0, 0, 0], np.uint32)
    seen = []
    for idx, recs in patches:
        rr = _face_records(idx, recs)
        lib.h_tally_patch(_p(host), _p(tally), _p(rr), U32(len(rr)), _p(tb), U32(len(tb)))
        lib.h_tally_slot(_p(tally), _p(state), int(fmt8), int(any(b != abi.OPAQUE for b in tex_blend)), int(blend_texels8), int(has_tail))
        want_faces = RM.patch_faces(faces, idx, recs); faces = want_faces
        assert host.tobytes() == want_faces.tobytes()
        assert tally.tolist() == _tally3(lib, want_faces, tb).tolist()
        own = (want_faces["blend_mode"] != abi.OPAQUE) | (want_faces["editor_alpha"] < 255)
        assert int(tally[0]) == int(own.sum()) and int(tally[2]) == int((want_faces["editor_alpha"] < 255).sum())
        want = _scratch_state(want_faces, tex_blend, fmt8, blend_texels8, tail_alpha)
        got = (bool(state[0]), bool(state[1]), int(state[2]))
        if fmt8:
            assert (got[1], got[2]) == (want[1], want[2]) and not got[0], (got, want)
        else:
            assert (got[0], got[2]) == (want[0], want[2]), (got, want)
        if has_tail:
            wb = _scratch_state(want_faces, tex_blend, fmt8, blend_texels8)
            assert int(state[5]) == wb[2] and (bool(state[4]) == wb[1] if fmt8 else bool(state[3]) == wb[0])
        seen.append(got)
    return seen


@pytest.mark.parametrize("fmt8", [False, True], ids=["rgb555", "rgba8"])
def test_incremental_tally_equals_a_fresh_upload(fmt8):
    """CPU test 2: random sequences of face patches -- opaque, every blend mode, alpha 0 / 100 / 254 / 255, texture ids that resolve (one
    of them to a blending texture), one out of range and B32_NO_TEXTURE -- with and without a tail that has blending faces."""
    lib = _host()
    rng = np.random.default_rng(7 + fmt8)
    tex_blend = [abi.OPAQUE, abi.ADD, abi.OPAQUE]
    for tail_alpha in (None, [255, 30, 255], [255, 255]):
        for tex in (tex_blend, [abi.OPAQUE] * 3):
            faces = _random_faces(rng, 200)
            patches = []
            for _ in range(12):
                n = int(rng.choice([1, 2, 17, 64, 200]))
                patches.append((_ascending(rng, n, len(faces)), _random_faces(rng, n)))
            seen = _walk(lib, faces, tex, fmt8, False, tail_alpha, patches)
            assert len({s[2] for s in seen}) > 3


@pytest.mark.parametrize("fmt8", [False, True], ids=["rgb555", "rgba8"])
@pytest.mark.parametrize("tail_alpha", [None, [255, 255], [255, 30]], ids=["no_tail", "opaque_tail", "blending_tail"])
def test_tally_transitions_to_and_from_no_face_blends(fmt8, tail_alpha):
    """CPU test 2: all-opaque -> one blending face -> all-opaque, by blend mode (RGB555: may_blend) and by editor alpha (both; the 8-bit
    path's blend8), also under a tail."""
    lib = _host()
    faces = b32.make_faces(50, 0); faces["v"] = np.arange(150).reshape(50, 3)
    one = faces[7:8].copy(); back = faces[7:8].copy()
    steps = []
    one["blend_mode"] = abi.AVERAGE
    steps += [(np.array([7], np.uint32), one.copy()), (np.array([7], np.uint32), back)]
    one["blend_mode"] = abi.OPAQUE; one["editor_alpha"] = 254
    steps += [(np.array([7], np.uint32), one.copy()), (np.array([7], np.uint32), back)]
    rng_idx = np.arange(10, 30, dtype=np.uint32)
    dim = faces[10:30].copy(); dim["editor_alpha"] = 100
    steps += [(rng_idx, dim), (rng_idx, faces[10:30].copy())]
    seen = _walk(lib, faces, [abi.OPAQUE], fmt8, False, tail_alpha, steps)
    tail_blends = tail_alpha is not None and min(tail_alpha) < 255
    tail_faces = 8 if tail_blends else 0
    flags = [s[1] if fmt8 else s[0] for s in seen]
    if fmt8:                                                                    # (a face's blend mode alone is not the 8-bit path's business)
        assert flags == [tail_blends, tail_blends, True, tail_blends, True, tail_blends]
    else:
        assert flags == [True, tail_blends, True, tail_blends, True, tail_blends]
    assert [s[2] for s in seen] == [1 + tail_faces, tail_faces, 1 + tail_faces, tail_faces, 20 + tail_faces, tail_faces]
    # blending texels keep an 8-bit scene's ordered walk whatever the faces do
    if fmt8:
        assert all(s[1] for s in _walk(lib, faces, [abi.OPAQUE], True, True, tail_alpha, steps))


def test_tally_program_runs_clean_under_the_sanitizers(tmp_path):
    """CPU test 2: tests/cpp/patch_tally_host.cpp -- a program of its own around the tally header and the record rules -- built with the
    address and undefined-behaviour sanitizers, runs its random sequences clean."""
    exe = tmp_path / "patch_tally_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "patch_tally_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ok" in r.stdout


@pytest.mark.parametrize("fmt8", [False, True], ids=["rgb555", "rgba8"])
@pytest.mark.parametrize("tex_blend", [[abi.OPAQUE] * 3, [abi.OPAQUE, abi.ADD, abi.OPAQUE]], ids=["opaque_textures", "blending_texture"])
def test_fresh_upload_state_equals_the_scratch_state(fmt8, tex_blend):
    """The uploads take their blend bookkeeping from the rule the patches use (tally_faces, then blend_fresh): for random faces, all-opaque
    ones, and opaque ones with one alpha face it equals _scratch_state, whatever the slot held before; what an upload leaves alone (blend8
    on an RGB555 scene, the body's copies) stays."""
    lib = _host()
    rng = np.random.default_rng(31 + fmt8)
    tb = np.ascontiguousarray(tex_blend, np.uint32)
    plain = b32.make_faces(60, 0); plain["v"] = np.arange(180).reshape(60, 3)
    dim = plain.copy(); dim["editor_alpha"][17] = 254
    textured = plain.copy(); textured["texture_id"][5:9] = 1
    for faces in (_random_faces(rng, 200), _random_faces(rng, 1), plain, dim, textured, plain[:0]):
        for blend_texels8 in (False, True):
            for held in ([1, 1, 77, 1, 1, 55], [0, 0, 0, 0, 0, 0]):
                state = np.array(held, np.uint32)
                lib.h_fresh_upload(_p(faces) if len(faces) else None, U32(len(faces)), _p(tb), U32(len(tb)), _p(state), int(fmt8), int(blend_texels8))
                want = _scratch_state(faces, tex_blend, fmt8, blend_texels8)
                assert (bool(state[0]), int(state[2])) == (want[0], want[2]), (state, want)
                assert bool(state[1]) == (want[1] if fmt8 else bool(held[1])), (state, want)
                assert state[3:].tolist() == held[3:]


def test_scene_state_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/cpp/scene_state_host.cpp -- every sequence of four writers of a slot, the rules of b32_scene_state.h against the assignments
    the writers made by hand before -- built with the address and undefined-behaviour sanitizers, ends with every field equal."""
    exe = tmp_path / "scene_state_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "scene_state_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ok" in r.stdout


# ---------------------------------------------------------------- one-point mutations of the mirrors
def test_mutations_of_the_mirrors_are_told_apart():
    """CPU test 3: each mutant is the mirror with one rule changed; each changes the named case and the host build of the device text
    sides with the mirror."""
    lib = _host()
    rng = np.random.default_rng(5)
    nv = 64
    verts = _random_vertices(rng, nv, 500.0)
    bo = (np.arange(nv) % 5).astype(np.uint16)
    tab = _table5()
    rest = RM.rest_stream(verts)
    posed = RM.pose_vertices(verts, bo, tab)
    idx = np.arange(0, nv, 3, dtype=np.uint32)
    recs = _random_vertices(rng, len(idx), 500.0)
    want_v, want_r = RM.patch_vertices(posed, idx, recs, rest=rest, bone_of_vertex=bo, bones=tab)
    got_v, got_r = _host_vertices(lib, posed, idx, recs, rest, bo, tab)
    assert _same_vertices(got_v, want_v) and got_r.tobytes() == want_r.tobytes()
    # (a) the rest stream not written: the next pose brings the old vertex back
    assert rest.tobytes() != want_r.tobytes()
    later = _table5(2.0)
    right = RM.pose_vertices(RM.patch_vertices(verts, idx, recs), bo, later)
    stale = RM.pose_vertices(verts, bo, later)
    assert not _same_bits(right["pos"][idx], stale["pos"][idx])
    from_rest = want_v.copy(); from_rest["pos"] = want_r[:, :3]; from_rest["normal"] = want_r[:, 3:]        # (what k_pose starts from)
    assert _same_vertices(RM.pose_vertices(from_rest, bo, later), right)
    # (b) the normal not posed
    mut = want_v.copy(); mut["normal"][idx] = recs["normal"]
    rot = np.isin(bo[idx], [0, 2, 3])
    assert rot.any() and not _same_bits(mut["normal"][idx[rot]], want_v["normal"][idx[rot]]) and _same_bits(got_v["normal"], want_v["normal"])
    # (c) the rectangle's stride taken as w
    tw, th, x, y, w, h = 16, 8, 3, 2, 5, 4
    pool = rng.integers(1, 1 << 16, tw * th + 8).astype(np.uint16)
    big = rng.integers(1, 1 << 16, (h, w + 3)).astype(np.uint16)
    want = RM.patch_texels(pool[:tw * th].reshape(th, tw), x, y, big[:, :w])
    mut = RM.patch_texels(pool[:tw * th].reshape(th, tw), x, y, big.reshape(-1)[:w * h].reshape(h, w))
    got = pool.copy()
    lib.h_texels(U32(2), U32(x), U32(y), U32(w), U32(h), U32(tw), U32(0), _p(big), U32(w + 3), _p(got))
    assert np.array_equal(got[:tw * th].reshape(th, tw), want) and not np.array_equal(mut, want) and np.array_equal(mut[y], want[y])
    # (d) the kept CLUT not zero-filled
    old = rng.integers(1, 1 << 16, 256).astype(np.uint16)
    clut = rng.integers(1, 1 << 16, 16).astype(np.uint16)
    mut = old.copy(); mut[:16] = clut
    kept = old.copy(); p2 = pool.copy(); at = np.zeros(tw * th, np.uint8)
    whole = rng.integers(0, 32, (th, tw)).astype(np.uint8)
    lib.h_indexed(U32(0), U32(0), U32(tw), U32(th), U32(tw), U32(0), _p(whole), U32(tw), _p(clut), U32(16), _p(p2), _p(at), _p(kept))
    assert np.array_equal(kept, RM.kept_clut(clut)) and not np.array_equal(mut, kept)
    assert not np.array_equal(RM.clut_lookup(mut, whole), RM.clut_lookup(kept, whole))      # (a lookup through the unfilled one sees stale colours)
    assert np.array_equal(RM.clut_lookup(kept, whole), RM.clut_lookup(clut, whole))
    # (e) black_transparent dropped from the face copy
    faces = b32.make_faces(20, 0); faces["black_transparent"] = 0
    fi = np.array([3, 4, 11], np.uint32)
    fr = faces[fi].copy(); fr["black_transparent"] = 1; fr["editor_alpha"] = 77
    want = RM.patch_faces(faces, fi, fr)
    mut = want.copy(); mut["black_transparent"][fi] = faces["black_transparent"][fi]
    got = faces.copy(); rr = _face_records(fi, fr)
    lib.h_faces(_p(rr), U32(3), _p(got))
    assert got.tobytes() == want.tobytes() and mut.tobytes() != want.tobytes() and want["black_transparent"][fi].all()


def test_layouts_symbols_and_null_arguments():
    """The records' layout on both sides of the boundary, and the entries answer B32_E_ARG without a context."""
    import __graft_entry__ as g
    g.build()
    lib = abi.load_library()
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "b32raster.h"\nint main(void){ printf("%zu %zu %zu %zu\\n", sizeof(B32VertexPatch), '
            'offsetof(B32VertexPatch, v), sizeof(B32FacePatch), offsetof(B32FacePatch, f)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [abi.VERTEX_PATCH_DTYPE.itemsize, abi.VERTEX_PATCH_DTYPE.fields["v"][1], abi.FACE_PATCH_DTYPE.itemsize, abi.FACE_PATCH_DTYPE.fields["f"][1]]
    E = abi.B32_E_ARG
    assert lib.b32_scene_patch_vertices(None, None, None, 0) == E and lib.b32_scene_patch_faces(None, None, None, 0) == E
    assert lib.b32_scene_patch_texels(None, None, 0, 0, 0, 0, 0, None, 0) == E and lib.b32_scene_patch_indexed(None, None, 0, 0, 0, 0, 0, None, 0, None, 0) == E
    assert lib.b32_scene_read_texels(None, None, 0, None) == E


# ================================================================== on the GPU
def _real(name):
    from bonnie32_amd import scenefile
    return scenefile.read_scene(os.path.join(REAL, name + ".b32scene"))


def _bones(t, scale):
    """The bone table of frame t: rotating, early return with a translation, rotating without translation, rotating, early return."""
    s = scale
    return RM.pack_bones([RM.Bone.from_euler((0.06 * s * np.sin(0.7 * t), 0.03 * s, -0.04 * s * np.cos(0.4 * t)), (6.0 + 3.0 * t, 0.0, -5.0 + 2.0 * t)),
                          RM.Bone.from_euler((0.35 * s - 0.02 * s * t, -0.05 * s, 0.02 * s * t), (0.0004, 30.0, 0.0)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (-4.0 - 1.5 * t, 0.0, 3.0 + t)),
                          RM.Bone.from_euler((-0.3 * s + 0.01 * s * t, 0.02 * s * t, 0.05 * s), (2.0 * t, 0.0, 9.0)),
                          RM.Bone.from_euler((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))])


@functools.lru_cache(maxsize=None)
def _warrior():
    """obj-warrior (227 vertices) with every face and texture Opaque, its textures widened for the 8-bit-colour path, and bone indices
    0..4, 5 and 6 (past the table) and B32_BONE_NONE in runs."""
    sc = _real("obj-warrior")
    assert len(sc.vertices) == 227
    sc.faces = sc.faces.copy(); sc.faces["blend_mode"] = abi.OPAQUE; sc.faces["editor_alpha"] = 255
    sc.textures = [b32.Texture15(t.width, t.height, t.pixels, abi.OPAQUE) for t in sc.textures]
    sc.textures8 = [b32.Texture.from_texture15(t) for t in sc.textures]
    rng = np.random.default_rng(5)
    bo = np.repeat(rng.integers(0, 8, 227 // 8 + 2).astype(np.uint16), 8)[:227].copy()
    bo[bo == 7] = NONE
    return sc, bo, 1000.0


@functools.lru_cache(maxsize=None)
def _triangle():
    """One triangle between three far-apart vertices of the warrior, drawn from both sides."""
    sc, _, _ = _warrior()
    p = sc.vertices["pos"]
    v = sc.vertices[[int(np.argmin(p[:, 0])), int(np.argmax(p[:, 0])), int(np.argmax(p[:, 1]))]].copy()
    f = b32.make_faces(1, 0); f["v"][0] = (0, 1, 2)
    return v, f


def _settings(mode, cull=True):
    sc, _, _ = _warrior()
    st = copy.copy(sc.settings)
    if mode == "painter":                                                       # painter's mode without shading
        st.use_zbuffer = False; st.shading = abi.SHADE_NONE; st.backface_wireframe = False; st.lights = []
    elif mode == "lit_wire":                                                    # z-buffer + Gouraud + one light + back-face wireframe
        assert st.use_zbuffer and st.backface_wireframe
    elif mode == "rgba8":                                                       # the 8-bit-colour path (render_mesh)
        st.use_rgb555 = False
    if not cull:
        st.backface_cull = False
    return st


def _oracle_frame(oracle, v, f, textures, camera, st, clear, fmt8=False, fog=None, size=(W, H)):
    ofb = oracle.Framebuffer(*size); ofb.clear(clear)
    if fmt8:
        rc, tm = oracle.render_mesh(ofb, v, f, textures, camera, st)
    else:
        rc, tm = oracle.render_mesh_15(ofb, v, f, textures, camera, st, fog)
    assert rc == 0
    return ofb.pixels.copy(), ofb.zbuffer.view(np.uint32).copy(), tm.triangles_drawn


def _draw(fb, rs, camera, st, clear, fog=None):
    fb.clear(clear)
    rs.render_async(camera, st, fog)
    return rs.finish()


def _assert_frame(fb, tm, want, what=""):
    px, zb, drawn = want
    got = fb.pixels
    assert np.array_equal(got, px), f"{what}: {int((got != px).sum())} bytes differ"
    gz = fb.zbuffer.view(np.uint32)
    assert np.array_equal(gz, zb), f"{what}: {int((gz != zb).sum())} depths differ"
    assert tm.triangles_drawn == drawn, what


def _observe(ctx, fb, rs, tm):
    """Everything a finished frame shows: pixels, depth bits, triangles_drawn, the draw order and the transparent counts."""
    rs._swap()
    try:
        order = ctx.last_draw_order(rs.n_faces).tolist()
        counts = ctx.transparent_counts()
    finally:
        rs._swap()
    return fb.pixels.tobytes(), fb.zbuffer.tobytes(), tm.triangles_drawn, order, counts


def _upload(R, fb, v, f, textures, fmt8=False, detached=False):
    """(A frame of a slot that may have to be redrawn is settled by the swap that takes the slot out again, and b32_frame_finish then has no
    frame to report on: the tests that read triangles_drawn of such frames draw the context's own scene.)"""
    rs = R.ResidentScene(fb, v, f, textures8=textures) if fmt8 else R.ResidentScene(fb, v, f, textures)
    return rs.detach() if detached else rs


def _fresh(R, fb, v, f, textures, camera, st, clear, fmt8=False, rig=None, bones=None, skeleton=None):
    """The other side of the contract: the arrays uploaded afresh into another context, the same rig, pose and skeleton, one
    frame, everything observed."""
    rs = _upload(R, fb, v, f, textures, fmt8)
    try:
        if rig is not None:
            rs.set_rig(rig)
            if bones is not None:
                rs.pose(bones)
        if skeleton is not None:
            rs.build_skeleton(*skeleton)
        tm = _draw(fb, rs, camera, st, clear)
        return _observe(fb.ctx, fb, rs, tm)
    finally:
        rs.close()


def _nudged(v, step, extent):
    """Edited vertices: moved, other uv, other colour."""
    rng = np.random.default_rng(1000 + step)
    out = v.copy()
    out["pos"] = v["pos"] + (rng.standard_normal((len(v), 3)) * 0.04 * extent).astype(f32)
    out["uv"] = v["uv"] + (rng.random((len(v), 2)) * 0.2).astype(f32)
    out["r"] = (v["r"].astype(np.int64) + 40 * (step + 1)) % 256
    out["g"] = 255 - v["g"]
    return out


VERTEX_CASES = [("warrior", "painter", False), ("warrior", "lit_wire", True), ("warrior", "rgba8", False), ("warrior", "rgba8", True),
                ("triangle", "painter", True), ("triangle", "lit_wire", False), ("triangle", "rgba8", True)]


@pytest.mark.gpu
@pytest.mark.parametrize("mesh,mode,detached", VERTEX_CASES, ids=["%s-%s-%s" % (a, b, "slot" if c else "context") for a, b, c in VERTEX_CASES])
def test_vertex_patches_equal_the_oracle_and_a_fresh_upload(oracle, mesh, mode, detached):
    """GPU test 4 (and 10c): the first, the last, a scattered ascending set and all vertices patched in turn; read_vertices equals the
    mirror's bits, the frame the oracle's render of the mirror-patched arrays, and everything observable a fresh upload's -- drawn as the
    context's own scene and through b32_scene_swap."""
    from bonnie32_amd import rasterizer as R
    sc, _, _ = _warrior()
    fmt8 = mode == "rgba8"
    textures = sc.textures8 if fmt8 else sc.textures
    if mesh == "warrior":
        v, f, st = sc.vertices, sc.faces, _settings(mode)
        sets = [[0], [226], sorted({3, 4, 64, 65, 100, 190, 225} | set(range(7, 227, 13))), list(range(227))]
    else:
        (v, f), st = _triangle(), _settings(mode, cull=False)
        sets = [[0], [2], [0, 2], [0, 1, 2]]
    extent = float(np.ptp(sc.vertices["pos"], axis=0).max())
    ctx, ctx2 = R.Context(0), R.Context(0)
    try:
        fb, fb2 = R.Framebuffer(W, H, ctx), R.Framebuffer(W, H, ctx2)
        rs = _upload(R, fb, v, f, textures, fmt8, detached)
        assert (rs._slot is None) == (not detached)
        before = _oracle_frame(oracle, v, f, textures, sc.camera, st, sc.clear_color, fmt8)
        _assert_frame(fb, _draw(fb, rs, sc.camera, st, sc.clear_color), before, "unpatched")
        assert before[2] >= 1
        cur = v.copy()
        for step, idx in enumerate(sets):
            idx = np.array(idx, np.uint32)
            new = _nudged(cur[idx], step, extent)
            rs.patch_vertices(idx, new)
            cur = RM.patch_vertices(cur, idx, new)
            assert rs.read_vertices().tobytes() == cur.tobytes(), step
            tm = _draw(fb, rs, sc.camera, st, sc.clear_color)
            want = _oracle_frame(oracle, cur, f, textures, sc.camera, st, sc.clear_color, fmt8)
            _assert_frame(fb, tm, want, f"step {step}")
            assert _observe(ctx, fb, rs, tm) == _fresh(R, fb2, cur, f, textures, sc.camera, st, sc.clear_color, fmt8), step
        assert not np.array_equal(want[0], before[0])
        rs.close()
    finally:
        ctx.close(); ctx2.close()


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
def test_rigged_slot_is_patched_in_rest_space(gpu_ctx, oracle):
    """GPU test 5: set_rig, pose(A), a patch in rest space: the vertices are pose(patched rest, A); after pose(B) they are pose(patched
    rest, B), which a patch that wrote only the posed vertices would miss; pose([]) gives the patched rest back; before the first pose
    and after pose([]) a patch copies.  The frame equals the oracle; hover, box selection and pick answer as on a fresh upload of the
    patched mesh (and as the host mirrors)."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    A, B = _bones(1.0, scale), _bones(4.0, scale)
    st = _settings("lit_wire")
    idx = np.array(sorted({0, 226} | set(range(5, 227, 9))), np.uint32)
    assert all((bo[idx] == k).any() for k in (0, 1, 2, 3, 4, 5, NONE))
    fb = R.Framebuffer(W, H, gpu_ctx)
    rs = _upload(R, fb, sc.vertices, sc.faces, sc.textures, detached=True)
    fr = None
    top = R.Topology.from_polygons(_merge_quads(sc.faces))
    try:
        rs.set_rig(bo)
        first = _nudged(sc.vertices[idx[:3]], 9, scale)
        rs.patch_vertices(idx[:3], first)                                       # before the first pose: copied
        rest = RM.patch_vertices(sc.vertices, idx[:3], first)
        assert rs.read_vertices().tobytes() == rest.tobytes()
        rs.pose(A)
        recs = _nudged(rest[idx], 0, scale)
        rs.patch_vertices(idx, recs)
        rest = RM.patch_vertices(rest, idx, recs)
        posed = RM.pose_vertices(rest, bo, A)
        assert _same_vertices(rs.read_vertices(), posed)
        tm = _draw(fb, rs, sc.camera, st, sc.clear_color)
        _assert_frame(fb, tm, _oracle_frame(oracle, posed, sc.faces, sc.textures, sc.camera, st, sc.clear_color), "posed A")
        # the queries: the patched slot, a fresh upload of the patched rest mesh with the same rig and pose, the host mirrors
        fr = _upload(R, fb, rest, sc.faces, sc.textures, detached=True)
        fr.set_rig(bo); fr.pose(A)
        cam, w, h = sc.camera, W, H                                            # (queries see the context's framebuffer size)
        mirror = R.HoverMirror(posed, top, None, cam, w, h, local_vertices=rest)
        ok = np.nonzero(mirror.some)[0]
        curs = [(float(mirror.sx[i]) + 1.5, float(mirror.sy[i]) - 1.0) for i in ok[(np.arange(24) * 7) % len(ok)]]
        prm = dict(mirror_axis=1, mirror_threshold=0.0)
        hits = 0
        for c in curs:
            got = _canon(gpu_ctx.hover_mesh(rs, top, cam, c, **prm))
            assert got == _canon(gpu_ctx.hover_mesh(fr, top, cam, c, **prm)) == _canon(mirror.hover(*c, **prm)), c
            hits += R.hovered_element(mirror.hover(*c, **prm)) != (None, None, None)
        assert hits >= 8
        for rect in ((0.0, 0.0, w * 0.55, h * 0.6), (w * 0.4, h * 0.3, w * 0.7, h * 0.9)):
            for bmode in (abi.BOX_VERTICES, abi.BOX_POLYGONS):
                words, cnt = gpu_ctx.box_select(rs, top, cam, rect, bmode)
                words2, cnt2 = gpu_ctx.box_select(fr, top, cam, rect, bmode)
                want_w, want_n = R.box_select_mesh(posed, top, None, cam, w, h, rect, bmode)
                assert cnt == cnt2 == want_n and np.array_equal(words, words2) and np.array_equal(words, want_w), (rect, bmode)
        here = b32.Placement(facing=0.0, world_pos=(0.0, 0.0, 0.0))
        picked = 0
        for c in curs[::3]:
            best, ph = gpu_ctx.pick_meshes([(rs, here), (fr, here)], cam, c)
            assert (int(ph[0]["hit"]), int(ph[0]["tri"])) == (int(ph[1]["hit"]), int(ph[1]["tri"])) and _same_bits(ph[0]["depth"], ph[1]["depth"]), c
            picked += int(ph[0]["hit"])
        assert picked >= 2
        # another pose starts from the patched rest stream
        rs.pose(B)
        got = rs.read_vertices()
        assert _same_vertices(got, RM.pose_vertices(rest, bo, B))
        only_posed = RM.pose_vertices(sc.vertices, bo, B)
        assert not _same_bits(got["pos"][idx], only_posed["pos"][idx])
        rs.pose([])
        assert rs.read_vertices().tobytes() == rest.tobytes()
        last = _nudged(rest[idx[-2:]], 3, scale)
        rs.patch_vertices(idx[-2:], last)                                       # after n_bones = 0: copied
        rest = RM.patch_vertices(rest, idx[-2:], last)
        assert rs.read_vertices().tobytes() == rest.tobytes()
        rs.pose(A)
        assert _same_vertices(rs.read_vertices(), RM.pose_vertices(rest, bo, A))
    finally:
        rs.close(); top.close()
        if fr is not None:
            fr.close()


def _skeleton(scale):
    bones = RM.pack_skel_bones([RM.SkelBone.from_rig((0.0, 0.03 * scale, 0.0), (10.0, 0.0, -5.0), 0.3 * scale, 0.03 * scale, None),
                                RM.SkelBone.from_rig((0.3 * scale, -0.05 * scale, 0.02 * scale), (0.0, 30.0, 40.0), 0.2 * scale, 0.0, 0),
                                RM.SkelBone.from_rig((-0.3 * scale, 0.1 * scale, 0.05 * scale), (75.0, 0.0, 100.0), 0.25 * scale, 0.02 * scale, 0)])
    return bones, RM.SkeletonStyle(editor_alpha=220, selected_bone=1)          # (the other bones are dimmed to alpha 30: a blending tail)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["painter", "rgba8"])
def test_body_patches_leave_the_tail_alone(oracle, mode):
    """GPU test 6: under a skeleton tail a vertex patch and a face patch of the body leave the tail's bits as they were, the frame is the
    oracle's render of (patched posed body + mirror tail) and equals a fresh upload with the same rig, pose and skeleton; an index inside
    the tail is B32_E_ARG and changes nothing."""
    from bonnie32_amd import rasterizer as R
    sc, bo, scale = _warrior()
    fmt8 = mode == "rgba8"
    textures = sc.textures8 if fmt8 else sc.textures
    st = _settings(mode)
    A = _bones(2.0, scale)
    skel = _skeleton(scale)
    tv, tf = RM.skeleton_mesh(*skel, 227)
    tail_blend = int((tf["editor_alpha"] < 255).sum())
    assert len(tv) == 18 and tail_blend >= 16
    ctx, ctx2 = R.Context(0), R.Context(0)
    try:
        fb, fb2 = R.Framebuffer(W, H, ctx), R.Framebuffer(W, H, ctx2)
        rs = _upload(R, fb, sc.vertices, sc.faces, textures, fmt8)
        rs.set_rig(bo); rs.pose(A); rs.build_skeleton(*skel)
        nv, nf = len(sc.vertices), len(sc.faces)
        assert rs.n_vertices == nv + 18 and rs.read_vertices(nv).tobytes() == tv.tobytes()
        _draw(fb, rs, sc.camera, st, sc.clear_color)
        idx = np.arange(2, nv, 5, dtype=np.uint32); idx[-1] = nv - 1
        recs = _nudged(sc.vertices[idx], 1, scale)
        rs.patch_vertices(idx, recs)
        rest = RM.patch_vertices(sc.vertices, idx, recs)
        fi = np.arange(0, nf, 3, dtype=np.uint32); fi[-1] = nf - 1
        fr = sc.faces[fi].copy(); fr["editor_alpha"] = 140; fr["black_transparent"] ^= 1
        rs.patch_faces(fi, fr)
        faces = RM.patch_faces(sc.faces, fi, fr)
        assert rs.read_vertices(nv).tobytes() == tv.tobytes() and rs.read_faces(nf).tobytes() == tf.tobytes()
        body = RM.pose_vertices(rest, bo, A)
        assert _same_vertices(rs.read_vertices(0, nv), body) and rs.read_faces(0, nf).tobytes() == faces.tobytes()
        tm = _draw(fb, rs, sc.camera, st, sc.clear_color)
        want = _oracle_frame(oracle, np.concatenate([body, tv]), np.concatenate([faces, tf]), textures, sc.camera, st, sc.clear_color, fmt8)
        _assert_frame(fb, tm, want, "body + tail")
        obs = _observe(ctx, fb, rs, tm)
        assert obs == _fresh(R, fb2, rest, faces, textures, sc.camera, st, sc.clear_color, fmt8, rig=bo, bones=A, skeleton=skel)
        assert obs[4][0] == len(fi) + tail_blend                                        # (the host's bound: the patched body faces and the dimmed bones')
        # back to an all-opaque body: only the tail blends
        rs.patch_faces(fi, sc.faces[fi])
        tm = _draw(fb, rs, sc.camera, st, sc.clear_color)
        assert _observe(ctx, fb, rs, tm) == _fresh(R, fb2, rest, sc.faces, textures, sc.camera, st, sc.clear_color, fmt8, rig=bo, bones=A, skeleton=skel)
        # the tail is never patched
        lib, E = ctx.lib, abi.B32_E_ARG
        vr = _vertex_records(np.array([nv - 1, nv], np.uint32), sc.vertices[:2])
        frr = _face_records(np.array([nf], np.uint32), sc.faces[:1])
        state = (rs.read_vertices().tobytes(), rs.read_faces().tobytes())
        assert lib.b32_scene_patch_vertices(ctx.h, rs._slot, abi.ptr(vr), 2) == E and lib.b32_scene_patch_faces(ctx.h, rs._slot, abi.ptr(frr), 1) == E
        assert (rs.read_vertices().tobytes(), rs.read_faces().tobytes()) == state
        rs.close()
    finally:
        ctx.close(); ctx2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["painter", "lit_wire", "rgba8"])
def test_face_patches_equal_the_oracle_and_a_fresh_upload(oracle, mode):
    """GPU test 7: an all-opaque scene; one face patched to Average, then alpha 255 -> 100 on a range, then everything back.  Frames,
    draw order and transparent counts at each step equal a fresh upload's and the oracle; also on the 8-bit path."""
    from bonnie32_amd import rasterizer as R
    sc, _, _ = _warrior()
    fmt8 = mode == "rgba8"
    textures = sc.textures8 if fmt8 else sc.textures
    st = _settings(mode)
    nf = len(sc.faces)
    one = np.array([nf // 2], np.uint32)
    avg = sc.faces[one].copy(); avg["blend_mode"] = abi.AVERAGE
    rng_i = np.arange(20, 90, dtype=np.uint32)
    dim = sc.faces[rng_i].copy(); dim["editor_alpha"] = 100
    both = np.array(sorted(set(one.tolist()) | set(rng_i.tolist())), np.uint32)
    steps = [(one, avg), (rng_i, dim), (both, sc.faces[both].copy())]
    ctx, ctx2 = R.Context(0), R.Context(0)
    try:
        fb, fb2 = R.Framebuffer(W, H, ctx), R.Framebuffer(W, H, ctx2)
        rs = _upload(R, fb, sc.vertices, sc.faces, textures, fmt8)
        tm = _draw(fb, rs, sc.camera, st, sc.clear_color)
        opaque = _observe(ctx, fb, rs, tm)
        assert opaque[4] == (0, 0)
        faces = sc.faces.copy()
        bounds = []
        for step, (idx, recs) in enumerate(steps):
            rs.patch_faces(idx, recs)
            faces = RM.patch_faces(faces, idx, recs)
            assert rs.read_faces().tobytes() == faces.tobytes()
            tm = _draw(fb, rs, sc.camera, st, sc.clear_color)
            _assert_frame(fb, tm, _oracle_frame(oracle, sc.vertices, faces, textures, sc.camera, st, sc.clear_color, fmt8), f"step {step}")
            obs = _observe(ctx, fb, rs, tm)
            assert obs == _fresh(R, fb2, sc.vertices, faces, textures, sc.camera, st, sc.clear_color, fmt8), step
            bounds.append(obs[4][0])
        assert bounds == [1, 71, 0] and obs == opaque
        rs.close()
    finally:
        ctx.close(); ctx2.close()


@pytest.mark.gpu
def test_face_patch_with_a_vertex_index_out_of_range(gpu_ctx):
    """GPU test 7: vertex indices are not validated by the patch; the frame reports B32_E_INDEX at b32_frame_finish, as after an upload."""
    from bonnie32_amd import rasterizer as R
    sc, _, _ = _warrior()
    st = _settings("lit_wire")
    fb = R.Framebuffer(W, H, gpu_ctx)
    rs = _upload(R, fb, sc.vertices, sc.faces, sc.textures, detached=True)
    try:
        _draw(fb, rs, sc.camera, st, sc.clear_color)
        good = (fb.pixels.tobytes(), fb.zbuffer.tobytes())
        bad = sc.faces[5:6].copy(); bad["v"][0, 2] = len(sc.vertices) + 3
        rs.patch_faces([5], bad)
        fb.clear(sc.clear_color); rs.render_async(sc.camera, st)
        with pytest.raises(R.B32Error) as e:
            rs.finish()
        assert e.value.code == abi.B32_E_INDEX
        rs.patch_faces([5], sc.faces[5:6])
        _draw(fb, rs, sc.camera, st, sc.clear_color)
        assert (fb.pixels.tobytes(), fb.zbuffer.tobytes()) == good
    finally:
        rs.close()


@pytest.mark.gpu
def test_later_face_patches_need_no_synchronisation(oracle):
    """GPU test 7: after the first face patch (which fetches the faces), four patched frames are enqueued back to back -- patch, clear,
    draw, download by ticket -- and only the last ticket is waited for; every delivered frame equals the oracle."""
    from bonnie32_amd import rasterizer as R
    sc, _, _ = _warrior()
    st = _settings("painter")
    ctx = R.Context(0)
    bufs = []
    try:
        ctx.set_async_depth(1)
        fb = R.Framebuffer(W, H, ctx)
        rs = _upload(R, fb, sc.vertices, sc.faces, sc.textures, detached=False)
        rs.patch_faces([0], sc.faces[:1])
        _draw(fb, rs, sc.camera, st, sc.clear_color)
        bufs = [ctx.host_alloc(W * H * 4) for _ in range(4)]
        idx = np.arange(10, 150, dtype=np.uint32)
        want, tickets = [], []
        for k, alpha in enumerate((200, 120, 40, 255)):
            recs = sc.faces[idx].copy(); recs["editor_alpha"] = alpha
            rs.patch_faces(idx, recs)
            fb.clear(sc.clear_color)
            rs.render_async()
            tickets.append(ctx.download_async(bufs[k][1]))
            want.append(_oracle_frame(oracle, sc.vertices, RM.patch_faces(sc.faces, idx, recs), sc.textures, sc.camera, st, sc.clear_color)[0])
        ctx.ticket_wait(tickets[-1])
        for k in range(4):
            assert np.array_equal(bufs[k][0], want[k].reshape(-1).view(np.uint8)), f"frame {k}: {int((bufs[k][0] != want[k].reshape(-1).view(np.uint8)).sum())} bytes differ"
        assert not np.array_equal(want[0], want[3])
        rs.finish()
    finally:
        for _, p in bufs:
            ctx.host_free(p)
        ctx.close()


def _two_texture_scene():
    """A textured mesh (600 triangles with uv all over the unit square) over two small textures in one pool, 4x4 and 3x5 (15 texels,
    padded to 16), none of whose texels can be skipped; every face honours black_transparent."""
    sc = scenegen.make_scene("C1", n_tris=600, width=W, height=H, seed=808)
    rng = np.random.default_rng(77)
    t0 = rng.integers(1, 0x8000, (4, 4)).astype(np.uint16) | np.uint16(0x0421)
    t1 = rng.integers(1, 0x8000, (5, 3)).astype(np.uint16) | np.uint16(0x0421)
    f = sc.faces.copy()
    f["texture_id"] = np.arange(len(f)) % 2
    f["black_transparent"] = 1
    return sc, f, t0, t1


def _tex15(*arrays):
    return [b32.Texture15(a.shape[1], a.shape[0], a, abi.OPAQUE) for a in arrays]


@pytest.mark.gpu
def test_texel_patches_of_a_pool_of_two_textures(oracle):
    """GPU test 8: the last texel of the first texture is patched and the second texture's first texel stays; then a rectangle brings
    0x0000 and 0x8000 texels into a texture that had none, under black_transparent faces (the skip mask must be rebuilt); read_texels of
    both textures equals the mirror and the frames the oracle.  Out-of-range rectangles are B32_E_ARG and change nothing."""
    from bonnie32_amd import rasterizer as R
    sc, f, t0, t1 = _two_texture_scene()
    st = sc.settings
    gpu_ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, gpu_ctx)
        rs = _upload(R, fb, sc.vertices, f, _tex15(t0, t1))
        first = _oracle_frame(oracle, sc.vertices, f, _tex15(t0, t1), sc.camera, st, sc.clear_color)
        _assert_frame(fb, _draw(fb, rs, sc.camera, st, sc.clear_color), first, "unpatched")
        rs.patch_texels(0, 3, 3, np.array([[0x7C1F]], np.uint16))
        t0 = RM.patch_texels(t0, 3, 3, np.array([[0x7C1F]], np.uint16))
        assert np.array_equal(rs.read_texels(0, 4, 4), t0) and np.array_equal(rs.read_texels(1, 3, 5), t1)
        want = _oracle_frame(oracle, sc.vertices, f, _tex15(t0, t1), sc.camera, st, sc.clear_color)
        _assert_frame(fb, _draw(fb, rs, sc.camera, st, sc.clear_color), want, "last texel of the first texture")
        assert not np.array_equal(want[0], first[0])
        # a strided view with transparent texels, into the second texture: x = 1, an odd width of one, five rows -- and its last texel
        big = np.full((5, 4), 0x1234, np.uint16); big[:, 2] = (0x0000, 0x8000, 0x0000, 0x7FFF, 0x8000)
        rs.patch_texels(1, 1, 0, big[:, 2:3])
        t1 = RM.patch_texels(t1, 1, 0, big[:, 2:3])
        rs.patch_texels(1, 0, 4, np.array([[0x0000, 0x0001, 0x0000]], np.uint16))
        t1 = RM.patch_texels(t1, 0, 4, np.array([[0x0000, 0x0001, 0x0000]], np.uint16))
        assert np.array_equal(rs.read_texels(0, 4, 4), t0) and np.array_equal(rs.read_texels(1, 3, 5), t1)
        holes = _oracle_frame(oracle, sc.vertices, f, _tex15(t0, t1), sc.camera, st, sc.clear_color)
        _assert_frame(fb, _draw(fb, rs, sc.camera, st, sc.clear_color), holes, "transparent texels")
        solid = f.copy(); solid["black_transparent"] = 0
        assert not np.array_equal(holes[0], _oracle_frame(oracle, sc.vertices, solid, _tex15(t0, t1), sc.camera, st, sc.clear_color)[0])
        # errors: nothing changes
        lib, E, h = gpu_ctx.lib, abi.B32_E_ARG, rs._slot
        px = np.zeros(64, np.uint16)
        for args in ((2, 0, 0, 1, 1), (0, 4, 0, 1, 1), (0, 0, 4, 1, 1), (0, 3, 0, 2, 1), (0, 0, 3, 1, 2), (1, 0, 0, 4, 1), (1, 0, 0, 3, 6), (0, 0xFFFFFFFF, 0, 2, 1)):
            assert lib.b32_scene_patch_texels(gpu_ctx.h, h, *args, abi.ptr(px), 8) == E, args
            assert lib.b32_scene_patch_indexed(gpu_ctx.h, h, *args, abi.ptr(px.view(np.uint8)), 8, abi.ptr(px), 16) == E, args
        assert lib.b32_scene_patch_texels(gpu_ctx.h, h, 0, 0, 0, 2, 2, None, 2) == E and lib.b32_scene_patch_texels(gpu_ctx.h, h, 0, 0, 0, 2, 2, abi.ptr(px), 1) == E
        assert lib.b32_scene_patch_texels(gpu_ctx.h, h, 0, 1, 1, 0, 3, None, 0) == 0 and lib.b32_scene_patch_texels(gpu_ctx.h, h, 1, 0, 0, 3, 0, abi.ptr(px), 3) == 0
        assert lib.b32_scene_read_texels(gpu_ctx.h, h, 2, abi.ptr(px)) == E and lib.b32_scene_read_texels(gpu_ctx.h, h, 0, None) == E
        assert np.array_equal(rs.read_texels(0, 4, 4), t0) and np.array_equal(rs.read_texels(1, 3, 5), t1)
        _assert_frame(fb, _draw(fb, rs, sc.camera, st, sc.clear_color), holes, "after the refused calls")
    finally:
        gpu_ctx.close()


@pytest.mark.gpu
def test_texel_patches_of_an_rgba_scene(oracle):
    """GPU test 8: Color texels: a rectangle of Erase texels, then texels that blend (the scene's walk becomes the ordered one, as a
    fresh upload's), then opaque ones again; patch_indexed on such a scene is B32_E_ARG."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C1", n_tris=600, width=W, height=H, seed=809)
    st = copy.copy(sc.settings); st.use_rgb555 = False
    t = b32.Texture.from_texture15(sc.textures[0])
    tex = t.pixels.reshape(t.height, t.width, 4).copy()
    tex[tex[:, :, 3] != abi.ERASE, 3] = abi.OPAQUE
    others = [b32.Texture.from_texture15(o) for o in sc.textures[1:]]
    mk = lambda a: [b32.Texture(t.width, t.height, a.reshape(-1, 4), abi.OPAQUE)] + others
    x, y, w, h = 1, 2, min(21, t.width - 1), min(13, t.height - 2)
    ctx, ctx2 = R.Context(0), R.Context(0)
    try:
        fb, fb2 = R.Framebuffer(W, H, ctx), R.Framebuffer(W, H, ctx2)
        rs = _upload(R, fb, sc.vertices, sc.faces, mk(tex), True)
        _draw(fb, rs, sc.camera, st, sc.clear_color)
        frames = []
        for step, blend in enumerate((abi.ERASE, abi.AVERAGE, abi.OPAQUE)):
            block = np.zeros((h, w, 4), np.uint8); block[:, :, 0] = 200; block[:, :, 1] = 40 * step; block[:, :, 2] = 90; block[:, :, 3] = blend
            rs.patch_texels(0, x, y, block)
            tex = RM.patch_texels(tex, x, y, block)
            assert np.array_equal(rs.read_texels(0, t.width, t.height), tex)
            tm = _draw(fb, rs, sc.camera, st, sc.clear_color)
            want = _oracle_frame(oracle, sc.vertices, sc.faces, mk(tex), sc.camera, st, sc.clear_color, True)
            _assert_frame(fb, tm, want, f"step {step}")
            assert _observe(ctx, fb, rs, tm) == _fresh(R, fb2, sc.vertices, sc.faces, mk(tex), sc.camera, st, sc.clear_color, True), step
            frames.append(want[0])
        assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
        idx = np.zeros(4, np.uint8); clut = np.zeros(16, np.uint16)
        assert ctx.lib.b32_scene_patch_indexed(ctx.h, rs._slot, 0, 0, 0, 2, 2, abi.ptr(idx), 2, abi.ptr(clut), 16) == abi.B32_E_ARG
        rs.close()
    finally:
        ctx.close(); ctx2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [True, False], ids=["lds_atlas", "no_lds_atlas"])
def test_indexed_patches_and_the_kept_atlas(oracle, lds):
    """GPU test 9: a one-texture indexed scene whose frames stage CLUT and indices in LDS (route 8 counts them).  A partial patch_indexed
    with the same CLUT and a whole-texture palette change keep the route and equal the oracle; a partial patch with another CLUT, or
    patch_texels, equal the oracle from the expanded texels, the route no longer taken.  The same frames with the route switched off."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C1", n_tris=2000, width=W, height=H, seed=6242)
    at = sc.indexed_textures[0]
    tw, th = at.width, at.height
    assert len(sc.indexed_textures) == 1 and at.clut.size == 16
    rng = np.random.default_rng(91)
    ctx = R.Context(0)
    try:
        if not lds:
            ctx.set_routes(R.Context.ROUTE_LDS_ATLAS)
        fb = R.Framebuffer(W, H, ctx)
        taken = lambda: ctx.route_counts()["lds_atlas"]

        def frame(rs, texels, expect_lds, what):
            before = taken()
            tm = _draw(fb, rs, sc.camera, sc.settings, sc.clear_color, sc.fog)
            want = _oracle_frame(oracle, sc.vertices, sc.faces, [b32.Texture15(tw, th, texels, at.blend_mode)], sc.camera, sc.settings, sc.clear_color, fog=sc.fog)
            _assert_frame(fb, tm, want, what)
            assert np.array_equal(rs.read_texels(0, tw, th), texels), what
            assert (taken() > before) == (expect_lds and lds), what
            return want[0]

        for drop in ("other_clut", "patch_texels"):
            rs = R.ResidentScene(fb, sc.vertices, sc.faces, indexed_textures=[at])
            atlas = at.indices.reshape(th, tw).copy()
            clut = at.clut.copy()
            texels = RM.clut_lookup(clut, atlas)
            f0 = frame(rs, texels, True, "uploaded")
            block = rng.integers(0, 20, (8, 8)).astype(np.uint8)                # (some indices past the 16-entry palette: 0x0000)
            rs.patch_indexed(0, 5, 9, block, clut)
            texels, atlas = RM.patch_indexed(texels, atlas, 5, 9, block, clut)
            f1 = frame(rs, texels, True, "a partial patch with the kept CLUT")
            clut2 = clut.copy(); clut2[1:9] = rng.integers(1, 0x8000, 8)
            rs.patch_indexed(0, 0, 0, atlas, clut2[:12])                        # a palette edit, with a shorter palette: 12..15 -> 0x0000
            texels, atlas = RM.patch_indexed(texels, atlas, 0, 0, atlas, clut2[:12])
            f2 = frame(rs, texels, True, "a whole-texture palette change")
            assert not np.array_equal(f0, f1) and not np.array_equal(f1, f2)
            rs.patch_indexed(0, 60, 0, atlas[0:3, 60:64], clut2[:12])           # the kept CLUT is now the 12-entry one
            f3 = frame(rs, texels, True, "a partial patch after the palette change")
            assert np.array_equal(f3, f2)
            if drop == "other_clut":
                block = rng.integers(0, 16, (7, 9)).astype(np.uint8)
                rs.patch_indexed(0, 30, 31, block, clut)
                texels, atlas = RM.patch_indexed(texels, atlas, 30, 31, block, clut)
            else:
                block = rng.integers(0, 0x10000, (7, 9)).astype(np.uint16)
                rs.patch_texels(0, 30, 31, block)
                texels = RM.patch_texels(texels, 30, 31, block)
            f4 = frame(rs, texels, False, drop)
            assert not np.array_equal(f4, f3)
            rs.patch_indexed(0, 0, 0, atlas[:4, :4], clut2[:12])                # the atlas stays dropped
            texels, _ = RM.patch_indexed(texels, None, 0, 0, atlas[:4, :4], clut2[:12])
            frame(rs, texels, False, "after the drop")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_patches_between_frames_in_flight(oracle):
    """GPU test 10: two frames in flight (their setup kernels on the second stream): patch -> draw -> patch -> draw -> download, every
    delivered frame equals its host-side composition, and the run did pipeline."""
    from bonnie32_amd import rasterizer as R
    sc = scenegen.make_scene("C3", n_tris=9000, width=W, height=H, bbox_px=60.0, seed=5, variant="gouraud")
    st = sc.settings
    nv = len(sc.vertices)
    ctx = R.Context(0)
    bufs = []
    try:
        ctx.set_async_depth(1)
        fb = R.Framebuffer(W, H, ctx)
        rs = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures)
        fb.clear(sc.clear_color); rs.render_async(sc.camera, st); rs.finish()   # (capacities settled by a warm-up frame, as deep mode asks)
        before = ctx.route_counts()["pipelined"]
        bufs = [ctx.host_alloc(W * H * 4) for _ in range(2)]
        tickets = [0, 0]
        cur = sc.vertices.copy()
        want = []
        extent = float(np.ptp(cur["pos"], axis=0).max())
        for t in range(8):
            idx = np.arange(t % 7, nv, 7, dtype=np.uint32)
            new = cur[idx].copy(); new["pos"] += (np.random.default_rng(t).standard_normal((len(idx), 3)) * 0.01 * extent).astype(f32)
            rs.patch_vertices(idx, new)
            cur = RM.patch_vertices(cur, idx, new)
            want.append(_oracle_frame(oracle, cur, sc.faces, sc.textures, sc.camera, st, sc.clear_color)[0].reshape(-1).view(np.uint8))
            fb.clear(sc.clear_color)
            rs.render_async()
            tickets[t & 1] = ctx.download_async(bufs[t & 1][1])
            if t > 0:
                ctx.ticket_wait(tickets[(t - 1) & 1])
                got = bufs[(t - 1) & 1][0]
                assert np.array_equal(got, want[t - 1]), f"frame {t - 1}: {int((got != want[t - 1]).sum())} bytes differ"
        ctx.ticket_wait(tickets[1])
        assert np.array_equal(bufs[1][0], want[7]) and not np.array_equal(want[0], want[7])
        rs.finish()
        assert ctx.route_counts()["pipelined"] > before
    finally:
        for _, p in bufs:
            ctx.host_free(p)
        ctx.close()


@pytest.mark.gpu
def test_patched_slot_in_a_batched_frame(oracle):
    """GPU test 10: a patched slot inside a b32_frame_submit run is redrawn from the patched data: a vertex patch costs one rebuild of
    the merged mesh, a frame without a patch none, and a face patch that makes the slot blend takes it out of the merged run (a slot that
    may blend is drawn on its own)."""
    from bonnie32_amd import rasterizer as R
    sc, _, scale = _warrior()
    other = _real("obj-ghost-game")
    st = b32.RasterSettings.game()
    st.lights = [b32.Light.directional((-1.0, -1.0, -1.0), 0.7)]
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        a = _upload(R, fb, sc.vertices, sc.faces, sc.textures, detached=True)
        b = _upload(R, fb, other.vertices, other.faces, other.textures, detached=True)
        table = ctx.make_frame_table(sc.camera, st, [a, b])
        cur_v, cur_f = sc.vertices.copy(), sc.faces.copy()
        built, single = [], []
        for step in range(4):
            if step == 1:
                idx = np.arange(0, 227, 4, dtype=np.uint32)
                new = _nudged(cur_v[idx], step, scale)
                a.patch_vertices(idx, new); cur_v = RM.patch_vertices(cur_v, idx, new)
            if step == 3:
                idx = np.arange(30, 120, dtype=np.uint32)
                new = cur_f[idx].copy(); new["editor_alpha"] = 90
                a.patch_faces(idx, new); cur_f = RM.patch_faces(cur_f, idx, new)
            fb.clear(sc.clear_color)
            ctx.frame_submit(table)
            ctx.finish()
            built.append(ctx.batch_counts()["merged_built"]); single.append(ctx.batch_counts()["single_draws"])
            ofb = oracle.Framebuffer(W, H); ofb.clear(sc.clear_color)
            for v, f, tex in ((cur_v, cur_f, sc.textures), (other.vertices, other.faces, other.textures)):
                rc, _tm = oracle.render_mesh_15(ofb, v, f, tex, sc.camera, st)
                assert rc == 0
            assert np.array_equal(fb.pixels, ofb.pixels), f"step {step}: {int((fb.pixels != ofb.pixels).sum())} bytes differ"
            assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32)), step
        assert [built[k + 1] - built[k] for k in range(3)] == [1, 0, 0], built
        assert single[2] == single[0] and single[3] > single[2], single
        a.close(); b.close()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_patch_errors_change_nothing(gpu_ctx):
    """The record rules at the interface: indices that repeat, descend or reach the body's count, missing arrays and a slot without a scene
    are B32_E_ARG; n == 0 is B32_OK; none of them changes the slot."""
    from bonnie32_amd import rasterizer as R
    sc, _, _ = _warrior()
    fb = R.Framebuffer(W, H, gpu_ctx)
    rs = _upload(R, fb, sc.vertices, sc.faces, sc.textures, detached=True)
    lib, E, h = gpu_ctx.lib, abi.B32_E_ARG, gpu_ctx.h
    empty = C.c_void_p()
    assert lib.b32_scene_create(h, C.byref(empty)) == 0
    try:
        nv, nf = len(sc.vertices), len(sc.faces)
        other = _nudged(sc.vertices[:3], 2, 1000.0)
        for idx in ([4, 4, 9], [9, 4, 12], [0, 1, nv], [0xFFFFFFFE, 0xFFFFFFFF, 3]):
            vr = _vertex_records(np.array(idx, np.uint32), other)
            fr = _face_records(np.array(idx, np.uint32), sc.faces[:3])
            assert lib.b32_scene_patch_vertices(h, rs._slot, abi.ptr(vr), 3) == E, idx
            if idx[2] == nv:
                fr["index"][2] = nf
            assert lib.b32_scene_patch_faces(h, rs._slot, abi.ptr(fr), 3) == E, idx
        vr = _vertex_records(np.array([1, 2, 3], np.uint32), other)
        fr = _face_records(np.array([1, 2, 3], np.uint32), sc.faces[:3])
        assert lib.b32_scene_patch_vertices(h, rs._slot, None, 3) == E and lib.b32_scene_patch_faces(h, rs._slot, None, 3) == E
        assert lib.b32_scene_patch_vertices(h, empty, abi.ptr(vr), 3) == E and lib.b32_scene_patch_faces(h, empty, abi.ptr(fr), 3) == E
        assert lib.b32_scene_patch_vertices(h, None, abi.ptr(vr), 3) == E       # (the context's own scene was moved into the slot)
        assert lib.b32_scene_patch_vertices(h, rs._slot, None, 0) == 0 and lib.b32_scene_patch_faces(h, rs._slot, abi.ptr(fr), 0) == 0
        assert rs.read_vertices().tobytes() == sc.vertices.tobytes() and rs.read_faces().tobytes() == sc.faces.tobytes()
        with pytest.raises(R.B32Error):
            rs.patch_vertices([3, 2], other[:2])
        rs.patch_vertices([1, 2, 3], other)
        assert rs.read_vertices().tobytes() == RM.patch_vertices(sc.vertices, [1, 2, 3], other).tobytes()
    finally:
        rs.close()
        lib.b32_scene_destroy(h, empty)


@pytest.mark.gpu
def test_cpp_patch_harness(tmp_path):
    """GPU test 11: tests/cpp/patch_harness.cpp -- a golden scene file through the C++ mirror's patch_vertices / patch_faces / patch_texels /
    patch_indexed / read_texels on the device and through its host restatements, both against the Python mirrors."""
    import __graft_entry__ as g
    g.build()
    sc = _real("obj-warrior")
    exe = tmp_path / "patch_harness"
    lib_dir = os.path.join(ROOT, "bonnie-32_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bonnie-32_amd", "host"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "patch_harness.cpp"), "-o", str(exe), "-L", lib_dir, "-lb32raster", f"-Wl,-rpath,{lib_dir}"], check=True)
    step, d = 3, np.array([12.5, -3.25, 0.1], f32)
    r = subprocess.run([str(exe), os.path.join(REAL, "obj-warrior.b32scene"), str(step)] + [float(x).hex() for x in d], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    vi = np.arange(0, len(sc.vertices), step, dtype=np.uint32)
    nv = sc.vertices[vi].copy(); nv["pos"] = nv["pos"] + d; nv["r"] ^= 255
    want_v = RM.patch_vertices(sc.vertices, vi, nv)
    fi = np.arange(1, len(sc.faces), step, dtype=np.uint32)
    nf = sc.faces[fi].copy(); nf["editor_alpha"] = 77; nf["black_transparent"] ^= 1
    want_f = RM.patch_faces(sc.faces, fi, nf)
    tex = (37 * np.arange(15) + 1).astype(np.uint16).reshape(3, 5)
    block = (0x4000 + 16 * np.arange(2)[:, None] + np.arange(4)[None, :]).astype(np.uint16)
    tex = RM.patch_texels(tex, 1, 1, block[:, :3])
    tex, _ = RM.patch_indexed(tex, None, 0, 0, np.array([[1, 0], [9, 2]], np.uint8), np.array([0x1111, 0x2222, 0x3333], np.uint16))
    want = {"v": np.ascontiguousarray(want_v).view(np.uint32).reshape(len(want_v), 9), "f": np.ascontiguousarray(want_f).view(np.uint32).reshape(len(want_f), 5),
            "t": tex.reshape(1, 15).astype(np.uint32)}
    seen = {"v": 0, "f": 0, "t": 0}
    for line in r.stdout.strip().splitlines():
        kind, rest = line[0], line[1:]
        dev, host = (np.array([int(x, 16) for x in part.split()], np.uint32) for part in rest.split("|"))
        row = want[kind][seen[kind]]
        assert np.array_equal(dev, row) and np.array_equal(host, row), (kind, seen[kind])
        seen[kind] += 1
    assert seen == {"v": len(want_v), "f": len(want_f), "t": 1}
    assert tex[0, 0] == 0x2222 and tex[1, 0] == 0 and tex[1, 1] == 0x3333 and tex[2, 3] == 0x4012
