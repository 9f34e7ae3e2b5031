"""k_setup's indexing by lane, wave and block: face counts around one wave (64), one block (256) and two blocks, through its three forms.

What is pinned: the face a lane owns (block * 256 + lane), the record slot a survivor takes (the wave's first face + its rank among the
wave's survivors: `face_of`, read back by b32_last_draw_order), the KEY_INVALID slots behind a wave's survivors, the per-block counters
(`partials[block * 8 + k]`, reduced into triangles_drawn and the error code) and the last, partly filled wave and block.

The mesh: nf small triangles scattered over a 64x48 frame from a fixed seed, every third one back-facing (culled: a wave's survivors do
not fill its slots), one of them beyond the fog's cull distance (culled only in the fog form).  Each count is drawn a second time with an
out-of-range vertex index in its LAST face -- the last lane of the last block; what that call returns and leaves in the frame is taken
from the oracle.  The forms: plain (benchmark(): fixed-point snap, painter's order, no lights), lit (game(): Gouraud, one point light) and
general (benchmark() with fog)."""
import functools

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi

f32 = np.float32
W, H = 64, 48
COUNTS = [1, 63, 64, 65, 255, 256, 257, 513]
FORMS = ["plain", "lit", "general"]
CAM = b32.Camera()
CLEAR = b32.Color(12, 24, 36)
FOG = (2200.0, 900.0, 3500.0, b32.Color(40, 60, 80))       # start, falloff, cull distance, colour
Z_FAR = 4000.0                                             # beyond the cull distance; every other vertex is nearer than 3000


def far_face(nf):
    """The face beyond the fog's cull distance: a front-facing one in the middle of the mesh (none below three faces)."""
    if nf < 3:
        return None
    k = nf // 2
    return k if k % 3 != 2 else k - 1


@functools.lru_cache(None)
def mesh(nf):
    rng = np.random.default_rng(20261019 + nf)
    v = b32.make_vertices(3 * nf)
    c = np.stack([rng.uniform(-600, 600, nf), rng.uniform(-450, 450, nf), rng.uniform(2000, 3000, nf)], axis=1).astype(f32)
    s = rng.uniform(60, 140, nf).astype(f32)
    if far_face(nf) is not None:
        c[far_face(nf), 2] = Z_FAR
    pos = np.repeat(c, 3, axis=0)
    pos[0::3, 0] -= s; pos[0::3, 1] -= s
    pos[1::3, 0] += s; pos[1::3, 1] -= s
    pos[2::3, 1] += s
    v["pos"] = pos
    n = rng.standard_normal((3 * nf, 3)).astype(f32)
    n[:, 2] = -np.abs(n[:, 2])
    v["normal"] = n / np.sqrt((n * n).sum(axis=1, dtype=f32))[:, None]
    v["uv"] = rng.random((3 * nf, 2), dtype=f32)
    rgb = rng.integers(0, 256, (3 * nf, 3))
    v["r"], v["g"], v["b"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    f = b32.make_faces(nf)
    idx = np.arange(nf)
    tri = np.stack([3 * idx, 3 * idx + 1, 3 * idx + 2], axis=1)
    back = idx % 3 == 2
    tri[back] = tri[back][:, [0, 2, 1]]                     # every third face: the other winding
    f["v"] = tri.astype(np.uint32)
    f["texture_id"] = np.where(idx % 2 == 0, 0, abi.NO_TEXTURE)
    f["blend_mode"] = abi.OPAQUE
    f["editor_alpha"] = 255
    px = rng.integers(1, 65536, 256).astype(np.uint16)
    tex = b32.Texture15(16, 16, px, abi.OPAQUE, "noise")
    for a in (v, f):
        a.setflags(write=False)
    return v, f, [tex]


@functools.lru_cache(None)
def bad_faces(nf):
    f = mesh(nf)[1].copy()
    f["v"][nf - 1, 1] = 3 * nf                              # the first index past the vertices, in the last lane that has a face
    f.setflags(write=False)
    return f


def settings_and_fog(form):
    if form == "lit":
        st = b32.RasterSettings.game()
        st.shading, st.lights = abi.SHADE_GOURAUD, [b32.Light.point((0.0, 0.0, 1200.0), 3000.0, 1.5)]
        return st, None
    return b32.RasterSettings.benchmark(), (FOG if form == "general" else None)


@functools.lru_cache(None)
def reference(nf, form, bad=False):
    """The oracle's verdict on one call, computed once and never written to afterwards: (rc, pixels, timings, dump)."""
    from oracle import oracle as O
    v, f, tex = mesh(nf)
    st, fog = settings_and_fog(form)
    fb = O.Framebuffer(W, H); fb.clear(CLEAR)
    rc, tm, d = O.render_mesh_15(fb, v, bad_faces(nf) if bad else f, tex, CAM, st, fog, dump=True)
    for a in (fb.pixels, d["shades"], d["colors"], d["draw_order"]):
        a.setflags(write=False)
    return rc, fb.pixels, tm, d


@pytest.mark.parametrize("nf", COUNTS)
def test_no_case_is_vacuous(oracle, nf):
    """By the oracle alone: every count and form draws a face, culls one from three faces up, the fog culls exactly the far face, and the
    call with the bad index is the reference's index panic with the frame as it was."""
    drawn = {}
    for form in FORMS:
        rc, px, tm, d = reference(nf, form)
        assert rc == 0
        drawn[form] = tm.triangles_drawn
        assert tm.triangles_drawn >= 1 and len(d["draw_order"]) == tm.triangles_drawn
        assert (px.reshape(-1, 4)[:, :3] != (CLEAR.r, CLEAR.g, CLEAR.b)).any()
        if nf >= 3:
            assert tm.triangles_drawn < nf                                   # (a back face was culled)
            assert set(np.arange(nf)[np.arange(nf) % 3 == 2]).isdisjoint(d["draw_order"].tolist())
        assert (d["shades"].shape == (tm.triangles_drawn, 9)) == (form == "lit")
        brc, bpx, _btm, _bd = reference(nf, form, bad=True)
        blank = oracle.Framebuffer(W, H); blank.clear(CLEAR)
        assert brc == abi.B32_E_INDEX and np.array_equal(bpx, blank.pixels)
    assert drawn["plain"] == drawn["lit"] == nf - nf // 3
    far = far_face(nf)
    assert drawn["general"] == drawn["plain"] - (far is not None)
    if far is not None:
        assert far in reference(nf, "plain")[3]["draw_order"] and far not in reference(nf, "general")[3]["draw_order"]
    if nf >= 65:                                                             # painter's order is not face order: face_of has work to do
        o = reference(nf, "plain")[3]["draw_order"]
        assert (np.diff(o.astype(np.int64)) < 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nf", COUNTS)
def test_counts_around_a_wave_and_a_block(gpu_ctx, nf, form):
    from bonnie32_amd import rasterizer as R
    v, f, tex = mesh(nf)
    st, fog = settings_and_fog(form)
    rc, px, etm, d = reference(nf, form)
    assert rc == 0
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(CLEAR)
    tm = R.render_mesh_15(fb, v, f, tex, CAM, st, fog)
    got = fb.pixels
    assert np.array_equal(got, px), f"{int((got != px).sum())} frame bytes differ"
    assert tm.triangles_drawn == etm.triangles_drawn
    assert np.array_equal(gpu_ctx.last_draw_order(nf), d["draw_order"])
    if form == "lit":
        faces, shades, _colors = gpu_ctx.last_surface_shading(nf)
        o = np.argsort(d["draw_order"], kind="stable")                       # (the tap answers in face order)
        assert np.array_equal(faces, d["draw_order"][o])
        assert np.array_equal(np.ascontiguousarray(shades, f32).view(np.uint32), np.ascontiguousarray(d["shades"][o], f32).view(np.uint32))
    # the same mesh with an index out of range in its last face: the oracle's verdict, and its frame
    brc, bpx, _btm, _bd = reference(nf, form, bad=True)
    fb.clear(CLEAR)
    with pytest.raises(R.B32Error) as e:
        R.render_mesh_15(fb, v, bad_faces(nf), tex, CAM, st, fog)
    assert e.value.code == brc and np.array_equal(fb.pixels, bpx)
