"""Per-vertex lighting and fog at float precision and at their parameter edges: shade_multi, fog_factor / fog_color, the normal
rotation of placed and posed meshes and the packed lit stream of b32_setup.hip, compared BEFORE the fill quantises them.

Why a stage tap (b32_last_surface_shading) and not the frame: a shade is an f32 in [-inf, 1]; the fill multiplies it into an 8-bit
channel and then drops three bits (`>> 3`, with dither).  Measured on the CPU with oracle/np_model.py on a C1 scene of 300 triangles at
128x96, RasterSettings.game(), one directional, one point and one spot light, 2908 drawn pixels: moving EVERY shade up by 1, 16 or 256 ulps
changes 0, 0 and 1 drawn pixels with flat shading and 3, 3 and 3 with Gouraud; moving every shade down by 1 ulp changes 59 and 26 pixels,
and only because shades saturated at exactly 1.0 fall off an integer product.  A contracted dot3, an acosf that is an ulp off or a
reciprocal in place of a division would pass every frame test.  The same holds for fogged vertex colours, 8-bit values seen through
`* tex8 / 128` and `>> 3`.  So the oracle's stage dump and the numpy model report the nine shades and the three fogged colours of every
drawn surface, the device tap returns what k_setup stored, and the three are compared bit for bit (float bits as uint32).

The mesh: two lattices of quads at 128x96, perspective camera at the origin.  The front one faces the camera at z = 2400 with vertices
at (150 i, 200 j, 2400), so that a light at (0, 0, 1200) is at distance sqrt(300^2 + 400^2 + 1200^2) = 1300 -- exactly, in f32 -- from the four
vertices (+-300, +-400, 2400) and n . l is positive there.  The rear one is tilted about the y axis, has alternating winding (backfaces: culled, or
drawn with negated normals when culling is off) and normals that point to and away from the lights.  Vertex normals follow a fixed
pattern: unit, x 1e20 and x 1e-30 (squares overflow / underflow), +0 and -0 vectors, a NaN component, an inf component, a denormal length.

One difference the reference leaves to the platform: f32::max(-0.0, 0.0) may return either zero (IEEE maxNum does not order them).
n . l == -0.0 happens here (a -0 normal), and the sign survives into the shade's bits only when every other term of the sum is -0.0 as
well, i.e. with ambient == -0.0: total = -0.0 + (+-0.0) * colour.  So ambient -0.0 is crossed only with lists whose every contribution
is the literal 0.0 of the `dist > radius` branch (and with the empty list), where both answers give the same shade.
"""
import functools

import numpy as np
import pytest

import bonnie32_amd as b32
from bonnie32_amd import abi

f32 = np.float32
W, H = 128, 96
Z0, LZ = 2400.0, 1200.0
NI, NJ = 5, 3                       # lattice indices i in -5..5, j in -3..3
CAM = b32.Camera()
CLEAR = b32.Color(12, 24, 36)
FOG_RGB = b32.Color(40, 60, 80)
INF, NAN = float("inf"), float("nan")
FLAT, GOURAUD = abi.SHADE_FLAT, abi.SHADE_GOURAUD


# ---------------------------------------------------------------- the mesh
def _vid(layer, i, j):
    return layer * (2 * NI + 1) * (2 * NJ + 1) + (j + NJ) * (2 * NI + 1) + (i + NI)


A, B, ANGLE_V = _vid(0, 0, 0), _vid(0, 0, 1), _vid(0, 2, 1)            # (0, 0, Z0), (0, 200, Z0), (300, 200, Z0)
RING = [_vid(0, i, j) for i in (-2, 2) for j in (-2, 2)]                # (+-300, +-400, Z0)


@functools.lru_cache(None)
def mesh():
    rng = np.random.default_rng(20261019)
    nv = 2 * (2 * NI + 1) * (2 * NJ + 1)
    v = b32.make_vertices(nv)
    base = np.zeros((nv, 3), f32)
    for j in range(-NJ, NJ + 1):
        for i in range(-NI, NI + 1):
            v["pos"][_vid(0, i, j)] = (150.0 * i, 200.0 * j, Z0)
            v["pos"][_vid(1, i, j)] = (150.0 * i + 40.0, 200.0 * j - 30.0, Z0 + 900.0 + 90.0 * i)
            base[_vid(0, i, j)] = (0.0, 0.0, -1.0)
    n2 = rng.standard_normal((nv // 2, 3)).astype(f32)
    n2[:, 2] = -np.abs(n2[:, 2]) * np.where(np.arange(nv // 2) % 3 == 0, f32(-1.0), f32(1.0))   # a third of them face away from the camera
    base[nv // 2:] = n2 / np.sqrt((n2 * n2).sum(axis=1, dtype=f32))[:, None]
    pattern = ["unit"] * 5 + ["big", "small", "zero", "negzero", "nan", "inf", "denormal"]
    nrm = base.copy()
    with np.errstate(all="ignore"):
        for k in range(nv):
            kind = pattern[k % len(pattern)]
            if kind == "big":
                nrm[k] = base[k] * f32(1e20)
            elif kind == "small":
                nrm[k] = base[k] * f32(1e-30)
            elif kind == "zero":
                nrm[k] = (0.0, 0.0, 0.0)
            elif kind == "negzero":
                nrm[k] = (-0.0, -0.0, -0.0)
            elif kind == "nan":
                nrm[k, k % 3] = np.nan
            elif kind == "inf":
                nrm[k, k % 3] = np.inf if k % 2 else -np.inf
            elif kind == "denormal":
                nrm[k] = base[k] * f32(1e-42)
    for k in RING + [ANGLE_V]:
        nrm[k] = (0.0, 0.0, -1.0)
    nrm[A] = nrm[B] = (0.6, 0.0, -0.8)                       # (the lights beside A and B sit along x: a normal with an x component sees them)
    v["normal"] = nrm
    v["uv"] = rng.random((nv, 2), dtype=f32)
    rgb = rng.integers(0, 256, (nv, 3))
    rgb[3] = (0, 255, 0); rgb[4] = (255, 0, 255)
    v["r"], v["g"], v["b"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    quads = []
    for layer in (0, 1):
        for j in range(-NJ, NJ):
            for i in range(-NI, NI):
                a, b, c, d = _vid(layer, i, j), _vid(layer, i + 1, j), _vid(layer, i + 1, j + 1), _vid(layer, i, j + 1)
                if layer == 1 and (i + j) % 2:
                    quads += [(a, c, b), (a, d, c)]
                else:
                    quads += [(a, b, c), (a, c, d)]
    f = b32.make_faces(len(quads))
    f["v"] = np.array(quads, np.uint32)
    idx = np.arange(len(f))
    f["texture_id"] = np.where(idx % 2 == 0, 0, abi.NO_TEXTURE)
    f["blend_mode"] = np.where(idx % 12 == 5, abi.ADD, abi.OPAQUE)
    f["editor_alpha"] = np.where(idx % 12 == 11, 90, 255)
    px = rng.integers(0, 65536, 256).astype(np.uint16)
    px[::17] = 0
    tex = b32.Texture15(16, 16, px, abi.OPAQUE, "noise")
    assert 200 <= len(f) <= 400 and (rgb == 0).any() and (rgb == 255).any()
    return v, f, [tex]


def big_mesh():
    """The same vertices under 36 copies of the face list: 8640 faces, past the 8192 from which a resident mesh is drawn from packed
    vertex streams (36-byte vertices on its first frame, the 12-byte position and 24-byte lit streams from its second)."""
    v, f, tex = mesh()
    return v, np.tile(f, 36), tex


# ---------------------------------------------------------------- light lists
def _dir(d, intensity, color=None, enabled=True):
    l = b32.Light.directional(d, intensity)
    if color is not None:
        l.color = color
    l.enabled = enabled
    return l


D = (0.3, -0.5, 1.0)
P0 = (0.0, 0.0, LZ)                  # on the axis through vertex A; 1300 from the ring
P1 = (40.0, 30.0, LZ)                # off every vertex's and every face centre's axis


def _spot_angle(vertex_pos, light_pos, direction):
    """spot_angle of render.rs:1043-1047 for one vertex, with the numpy model's own functions."""
    from oracle import np_model as M
    to_light = (np.asarray(light_pos, f32) - np.asarray(vertex_pos, f32)).astype(f32)
    neg = (M.normalize3(to_light) * f32(-1.0)).astype(f32)
    return M.acosf(M.dot3(neg, np.asarray(direction, f32)))


def _many(n):
    rng = np.random.default_rng(100 + n)
    out = []
    for k in range(n):
        p = (float(rng.integers(-900, 900)), float(rng.integers(-700, 700)), float(rng.integers(900, 3600)))
        l = b32.Light.point(p, float(rng.integers(1200, 3000)), 0.2)
        l.color = b32.Color(int(rng.integers(0, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 256)))
        out.append(l)
    return out


# Lists whose shades are EXPECTED to coincide with those of the empty list ("empty") or to be 1.0 throughout ("ones"), each with the
# reason; any other list that coincides fails test_oracle_and_numpy_model_agree.
COINCIDE = {
    "point_r0": "empty",          # dist > 0 everywhere: the literal 0.0
    "point_rneg": "empty",        # dist > -5
    "point_3e38": "empty",        # to_light^2 overflows: dist = inf > 3e38
    "dir_zero": "empty",          # n . 0 is 0 or NaN, max(NaN, 0) = 0
    "spot_a0": "empty",           # no vertex or centre on P1's axis: spot_angle > 0
    "spot_aneg": "empty",         # spot_angle > -1
    "spot_dir0": "empty",         # acos(0) = pi/2 > 0.5
    "point_rnan": "ones",         # dist > NaN is false, attenuation = 1 - dist / NaN
    "point_pinf": "ones",         # dist = inf is not > inf, attenuation = 1 - inf / inf
    "dir_iinf": "ones",           # n . l * inf is inf or (0 * inf) NaN
    "dir_inan": "ones",
    "spot_anan": "ones",          # spot_angle > NaN is false, edge_falloff = 1 - a / NaN; radius 1e6 reaches every vertex
    # per shading mode: flat shading normalises the mean normal, so an inf component becomes inf / inf = NaN and max(NaN, 0) * 0 = 0;
    # Gouraud takes the raw normal, and inf * 0 = NaN
    "dir_i0": {FLAT: "empty"},
}


@functools.lru_cache(None)
def light_lists():
    v, _f, _t = mesh()
    pa, pb = v["pos"][A], v["pos"][B]
    P, S = b32.Light.point, b32.Light.spot
    a_exact = float(_spot_angle(v["pos"][ANGLE_V], P0, (0.0, 0.0, 1.0)))
    L = {
        "empty": [],
        "basic": [_dir(D, 0.7), P(P0, 1300.0, 1.5), S((200.0, -100.0, LZ), (0.0, 0.0, 1.0), 0.5, 2500.0, 2.0)],
        "point": [P(P0, 1300.0, 1.5)],
        "point_at_vertex": [P(tuple(pa), 2000.0, 1.0)],
        "point_beside": [P((float(pa[0]) + 2.0 ** -10, float(pa[1]), float(pa[2])), 2000.0, 1.0),
                         P((float(pb[0]) + 2.0 ** -10 + 2.0 ** -13, float(pb[1]), float(pb[2])), 2000.0, 1.0)],
        "point_r0": [P(P0, 0.0, 1.5)],
        "point_rneg": [P(P0, -5.0, 1.5)],
        "point_rinf": [P(P0, INF, 1.5)],
        "point_rnan": [P(P0, NAN, 1.5)],
        "point_pinf": [P((INF, 0.0, LZ), INF, 1.5)],
        "point_3e38": [P((3e38, 3e38, 3e38), 3e38, 1.5)],
        "dir_iinf": [_dir(D, INF)],
        "dir_ineginf": [_dir(D, -INF)],
        "dir_ineg2": [_dir(D, -2.0)],
        "dir_inan": [_dir(D, NAN)],
        "dir_i0": [_dir(D, 0.0)],
        "dir_zero": [b32.Light(abi.LIGHT_DIRECTIONAL, direction=(0.0, 0.0, 0.0), intensity=0.7)],
        "dir_1e30": [b32.Light(abi.LIGHT_DIRECTIONAL, direction=(3e29, -5e29, 1e30), intensity=1e30)],
        "dir_colour": [_dir(D, 0.7, b32.Color(255, 0, 7))],
        "disabled": [_dir(D, NAN, enabled=False), b32.Light(9, intensity=1.0, enabled=False), _dir(D, 0.7)],
        "spot_a0": [S(P1, (0.0, 0.0, 1.0), 0.0, 1e6, 2.0)],
        "spot_aneg": [S(P1, (0.0, 0.0, 1.0), -1.0, 1e6, 2.0)],
        "spot_api": [S(P1, (0.0, 0.0, 1.0), float(f32(np.pi)), 1e6, 2.0)],
        "spot_ainf": [S(P1, (0.0, 0.0, 1.0), INF, 1e6, 2.0)],
        "spot_anan": [S(P1, (0.0, 0.0, 1.0), NAN, 1e6, 2.0)],
        # intensity inf makes the cone's edge visible in the shade: inside (and ON it, where edge_falloff is 0) inf or 0 * inf, outside 0
        "spot_exact": [S(P0, (0.0, 0.0, 1.0), a_exact, 1e6, 2.0), S(P0, (0.0, 0.0, 1.0), a_exact, 1e6, INF)],
        "spot_below": [S(P0, (0.0, 0.0, 1.0), float(np.nextafter(f32(a_exact), f32(0.0))), 1e6, 2.0),
                       S(P0, (0.0, 0.0, 1.0), float(np.nextafter(f32(a_exact), f32(0.0))), 1e6, INF)],
        "spot_dir0": [b32.Light(abi.LIGHT_SPOT, position=P1, direction=(0.0, 0.0, 0.0), angle=0.5, radius=1e6, intensity=2.0)],
        "spot_dirnan": [b32.Light(abi.LIGHT_SPOT, position=P1, direction=(NAN, 0.0, 1.0), angle=0.5, radius=2500.0, intensity=2.0)],
        "spot_dir3": [b32.Light(abi.LIGHT_SPOT, position=P1, direction=(0.0, 0.0, 3.0), angle=0.5, radius=2500.0, intensity=2.0)],
        "spot_at_vertex": [S(tuple(pa), (0.0, 0.0, 1.0), 1.2, 2000.0, 2.0)],
        "n8": _many(8), "n9": _many(9), "n17": _many(17),
    }
    return L


def test_inputs_hold_the_edges():
    """The conditions that keep the comparisons from being vacuous, on the INPUTS, in numpy f32 with the model's own operation order."""
    from oracle import np_model as M
    v, f, _t = mesh()
    L = light_lists()
    pos = v["pos"].astype(f32)

    def dist(light):
        t = (np.asarray(light.position, f32) - pos).astype(f32)
        return np.sqrt(M.dot3(t, t))
    d = dist(L["point"][0])
    assert (d == f32(L["point"][0].radius)).sum() >= 4 and (d[RING] == f32(1300.0)).all()
    assert (d > f32(1300.0)).any() and (d < f32(1300.0)).any()
    near, above = dist(L["point_beside"][0]), dist(L["point_beside"][1])
    lo = M.K("light.min_dist")
    assert near[A] == f32(2.0 ** -10) and near[A] < lo and (near < lo).sum() == 1
    assert above[B] == f32(2.0 ** -10 + 2.0 ** -13) and lo < above[B] < f32(0.0011) and (above < lo).sum() == 0
    assert dist(L["point_at_vertex"][0])[A] == 0
    axis = L["spot_exact"][0]
    t = (np.asarray(axis.position, f32) - pos[A]).astype(f32)
    assert M.dot3((M.normalize3(t) * f32(-1.0)).astype(f32), np.asarray(axis.direction, f32)) == f32(1.0)       # on the axis: acos(1) = 0
    a = _spot_angle(pos[ANGLE_V], axis.position, axis.direction)
    assert f32(axis.angle) == a and 0.0 < a < 1.0
    below = L["spot_below"][0]
    assert f32(below.angle) < a and np.nextafter(f32(below.angle), f32(1.0)) == a
    # no vertex and no face centre on P1's axis (spot_a0 must light nothing)
    third = f32(1.0) / f32(3.0)
    cen = (((pos[f["v"][:, 0]] + pos[f["v"][:, 1]]).astype(f32) + pos[f["v"][:, 2]]).astype(f32) * third).astype(f32)
    for p in (pos, cen):
        assert ((p[:, 0] != f32(P1[0])) | (p[:, 1] != f32(P1[1]))).all()
    # the normal pattern is all there
    n = v["normal"]
    with np.errstate(all="ignore"):
        sq = (n.astype(f32) ** 2).sum(axis=1, dtype=f32)
    assert np.isinf(sq[np.isfinite(n).all(axis=1)]).any()                                     # x 1e20: the square overflows
    assert ((sq == 0) & (n != 0).any(axis=1)).any()                                           # x 1e-30 / denormal: it underflows to 0
    assert ((n == 0).all(axis=1) & ~np.signbit(n).any(axis=1)).any() and ((n == 0).all(axis=1) & np.signbit(n).all(axis=1)).any()
    assert np.isnan(n).any() and np.isinf(n).any()
    assert ((np.abs(n) < f32(1.1754944e-38)) & (n != 0)).any()
    assert len(L["n8"]) == 8 and len(L["n9"]) == 9 and len(L["n17"]) == 17 and abi.SHADE_FLAT == 1


# ---------------------------------------------------------------- cases
def _cases():
    """name -> (light list, ambient, fog, backface_cull)."""
    out = {}
    for k, name in enumerate(light_lists()):
        out[name] = (name, 0.3, None, k % 2 == 0)
    k = 0
    for amb, tag in ((0.0, "0"), (-1.0, "neg1"), (5.0, "5"), (NAN, "nan")):
        for name in ("basic", "dir_ineg2", "point"):
            out[f"amb_{tag}-{name}"] = (name, amb, None, k % 2 == 0); k += 1
    for name in ("empty", "point_r0", "point_3e38"):            # (see the module docstring: the lists that do not depend on max(-0.0, 0.0))
        out[f"amb_negzero-{name}"] = (name, -0.0, None, k % 2 == 0); k += 1
    fogs = {
        "beyond": (5000.0, 1000.0, 1e9), "between": (2600.0, 800.0, 1e9), "falloff_0": (2600.0, 0.0, 1e9), "falloff_neg": (2600.0, -5.0, 1e9),
        "falloff_nan": (2600.0, NAN, 1e9), "falloff_denormal": (2600.0, 1e-40, 1e9), "falloff_inf": (2600.0, INF, 1e9),
        "start_nan": (NAN, 800.0, 1e9), "start_neginf": (-INF, 800.0, 1e9), "cull_nan": (2000.0, 1500.0, NAN), "cull_0": (2000.0, 1500.0, 0.0),
        "cull_between": (2000.0, 1500.0, 2600.0),
    }
    for k, (tag, (s, fo, c)) in enumerate(fogs.items()):
        out[f"fog_{tag}"] = ("basic", 0.3, (s, fo, c, FOG_RGB), k % 2 == 0)
    out["fog_blend3"] = ("basic", 0.3, (2000.0, 600.0, 1e9, b32.Color(90, 20, 200, 3)), True)
    return out


CASES = _cases()
# about eight lists that take each branch of shade_multi once (none, all three light types, a NaN source, a negative shade, the disabled
# skip, the inline and the device-buffer light table), for the paths that are not the drop-in call in z-buffer mode
REDUCED = ["empty", "basic", "point_beside", "dir_ineg2", "point_rnan", "disabled", "spot_exact", "spot_dir3", "n17"]


def settings_for(case, shading, **kw):
    name, amb, _fog, cull = CASES[case]
    st = b32.RasterSettings.game()
    st.shading, st.lights, st.ambient, st.backface_cull = shading, light_lists()[name], amb, cull
    for k, val in kw.items():
        setattr(st, k, val)
    return st


def tex8():
    return [b32.Texture.from_texture15(t, abi.AVERAGE) for t in mesh()[2]]


_REF = {}


def reference(oracle, case, shading, fmt8=False, geometry=None, key=None, **kw):
    """The oracle's frame, z-buffer and dump for a case, computed once per distinct request and never written to afterwards."""
    k = (case, shading, fmt8, key, tuple(sorted(kw.items())))
    if k not in _REF:
        v, f, tex = geometry if geometry is not None else mesh()
        st = settings_for(case, shading, **kw)
        fb = oracle.Framebuffer(W, H); fb.clear(CLEAR)
        if fmt8:
            rc, tm, d = oracle.render_mesh(fb, v, f, tex8(), CAM, st, dump=True)
        else:
            rc, tm, d = oracle.render_mesh_15(fb, v, f, tex, CAM, st, CASES[case][2], dump=True)
        assert rc == 0
        for a in (fb.pixels, fb.zbuffer, d["shades"], d["colors"], d["draw_order"]):
            a.setflags(write=False)
        _REF[k] = (fb.pixels, fb.zbuffer.view(np.uint32), tm, d)
    return _REF[k]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_floats(a, b):
    """Bit-equal, any NaN standing for any other NaN."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------- CPU: the two restatements agree, and the cases are not vacuous
@pytest.mark.parametrize("case", list(CASES))
def test_oracle_and_numpy_model_agree(oracle, case):
    from oracle import np_model as M
    v, f, tex = mesh()
    name, _amb, fog, _cull = CASES[case]
    for shading in (FLAT, GOURAUD):
        for fmt8 in ((False,) if fog is not None or shading == FLAT else (False, True)):
            px, zb, tm, d = reference(oracle, case, shading, fmt8)
            st = settings_for(case, shading)
            img = np.zeros(W * H * 4, np.uint8); img.reshape(-1, 4)[:] = (CLEAR.r, CLEAR.g, CLEAR.b, 255)
            z = np.full(W * H, np.finfo(f32).max, f32)
            with np.errstate(all="ignore"):
                m = M.render_mesh(img, W, H, v, f, tex8(), CAM, st, z) if fmt8 else M.render_mesh_15(img, W, H, v, f, tex, CAM, st, fog, z)
            assert np.array_equal(img, px), f"{int((img != px).sum())} frame bytes differ ({shading}, {fmt8})"
            assert np.array_equal(z.view(np.uint32), zb)
            assert m["triangles_drawn"] == tm.triangles_drawn and np.array_equal(m["draw_order"], d["draw_order"])
            assert same_floats(m["shades"], d["shades"]) and not np.isnan(d["shades"]).any()       # (total.min(1.0) drops every NaN)
            assert np.array_equal(m["colors"], d["colors"])
            assert d["shades"].shape == (tm.triangles_drawn, 9) and d["colors"].shape == (tm.triangles_drawn, 3)
            if case == "fog_cull_0":
                assert tm.triangles_drawn == 0
            else:
                assert tm.triangles_drawn >= 100 and int((px.reshape(-1, 4)[:, :3] != (CLEAR.r, CLEAR.g, CLEAR.b)).any(axis=1).sum()) > 1000
            if case in light_lists():                         # a list must leave its mark on the shades, unless it is named above
                empty = reference(oracle, "empty", shading, backface_cull=CASES[case][3])[3]["shades"]
                sh = d["shades"]
                is_empty = sh.shape == empty.shape and np.array_equal(bits(sh), bits(empty))
                is_ones = bool((sh == f32(1.0)).all())
                want = "empty" if case == "empty" else COINCIDE.get(case)
                want = want.get(shading) if isinstance(want, dict) else want
                assert (empty == f32(0.3)).all()
                assert is_empty == (want == "empty") and is_ones == (want == "ones"), (case, shading, is_empty, is_ones)


def test_fog_cases_move_the_colours(oracle):
    """Each fog tuple gives colours of its own, except the groups named here, each with its reason."""
    col = {c: reference(oracle, c, GOURAUD, backface_cull=True)[3] for c in CASES if c.startswith("fog_")}       # (one culling for all: the same surfaces)
    plain = reference(oracle, "basic", GOURAUD, backface_cull=True)[3]
    groups = {
        "fog_beyond": "none", "fog_falloff_inf": "none",                  # z <= start everywhere; (z - start) / inf = 0
        # behind the start the factor saturates: falloff <= 0 returns 1.0, (z - start) / 1e-40 = inf, min(NaN, 1.0) = 1.0
        "fog_falloff_0": "behind", "fog_falloff_neg": "behind", "fog_falloff_denormal": "behind", "fog_falloff_nan": "behind",
        # z <= NaN is false and min((z - NaN) / falloff, 1.0) = 1.0; (z + inf) / falloff = inf: the fog colour on every vertex
        "fog_start_nan": "all", "fog_start_neginf": "all",
    }
    assert len(col["fog_cull_0"]["colors"]) == 0 and 0 < len(col["fog_cull_between"]["colors"]) < len(plain["colors"])
    seen = {}
    for c, d in col.items():
        if c == "fog_cull_0":
            continue
        k = (d["colors"].tobytes(), d["draw_order"].tobytes())
        group = groups.get(c, c)
        assert seen.setdefault(k, group) == group, (c, seen[k])
        assert np.array_equal(d["colors"], plain["colors"]) == (group == "none"), c
    assert len(set(seen.values())) == len(seen)                           # (a group has ONE set of colours)
    assert (col["fog_start_nan"]["colors"] == (FOG_RGB.r | FOG_RGB.g << 8 | FOG_RGB.b << 16)).all()
    partial = col["fog_between"]["colors"]                                # some vertices untouched, some mixed, none NaN-saturated to black
    assert (partial == plain["colors"]).any() and (partial != plain["colors"]).any()


# ---------------------------------------------------------------- GPU
def by_face(d):
    """The oracle's per-surface dump keyed by face index (the tap's order)."""
    o = np.argsort(d["draw_order"], kind="stable")
    return d["draw_order"][o], d["shades"][o] if len(d["shades"]) else d["shades"], d["colors"][o]


def check_tap(ctx, d, nf, what=""):
    faces, shades, colors = ctx.last_surface_shading(nf)
    ef, es, ec = by_face(d)
    assert np.array_equal(faces, ef), what
    assert not np.isnan(shades).any(), what
    bad = ~((bits(shades) == bits(es)) | (np.isnan(shades) & np.isnan(es))) if shades.shape == es.shape else None
    assert bad is not None and not bad.any(), f"{what}: {int(bad.sum()) if bad is not None else '?'} shades differ, first at surface/slot {np.argwhere(bad)[:3].tolist() if bad is not None else ''}"
    assert np.array_equal(colors, ec), f"{what}: {int((colors != ec).any(axis=1).sum())} surfaces' colours differ"


def check_frame(fb, tm, ref, zmode=True, what=""):
    px, zb, etm, d = ref
    got = fb.pixels
    assert np.array_equal(got, px), f"{what}: {int((got != px).sum())} frame bytes differ"
    if zmode:
        assert np.array_equal(fb.zbuffer.view(np.uint32), zb), what
    assert tm.triangles_drawn == etm.triangles_drawn, what
    n = len(d["draw_order"])
    assert np.array_equal(fb.ctx.last_draw_order(max(n, 1)), d["draw_order"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_drop_in_zbuffer(gpu_ctx, oracle, case):
    """Every case, flat and Gouraud, through b32_render_mesh_15 in z-buffer mode: frame, z-buffer, count, order, shades, colours."""
    from bonnie32_amd import rasterizer as R
    v, f, tex = mesh()
    fb = R.Framebuffer(W, H, gpu_ctx)
    for shading in (FLAT, GOURAUD):
        ref = reference(oracle, case, shading)
        fb.clear(CLEAR)
        tm = R.render_mesh_15(fb, v, f, tex, CAM, settings_for(case, shading), CASES[case][2])
        check_frame(fb, tm, ref, what=f"{case}/{shading}")
        check_tap(gpu_ctx, ref[3], len(f), f"{case}/{shading}")


@pytest.mark.gpu
def test_tap_on_an_unlit_frame_and_its_refusals(gpu_ctx, oracle):
    from bonnie32_amd import rasterizer as R
    v, f, tex = mesh()
    fb = R.Framebuffer(W, H, gpu_ctx)
    fb.clear(CLEAR)
    ref = reference(oracle, "fog_between", abi.SHADE_NONE)
    tm = R.render_mesh_15(fb, v, f, tex, CAM, settings_for("fog_between", abi.SHADE_NONE), CASES["fog_between"][2])
    check_frame(fb, tm, ref)
    faces, shades, colors = gpu_ctx.last_surface_shading(len(f))
    assert shades.shape == (0, 9) and ref[3]["shades"].shape == (0, 9)
    ef, _es, ec = by_face(ref[3])
    assert np.array_equal(faces, ef) and np.array_equal(colors, ec)
    # pending frame: refused, like b32_last_draw_order
    rs = R.ResidentScene(fb, v, f, tex)
    fb.clear(CLEAR); rs.render_async(CAM, settings_for("basic", GOURAUD))
    with pytest.raises(R.B32Error):
        gpu_ctx.last_surface_shading(len(f))
    rs.finish()
    check_tap(gpu_ctx, reference(oracle, "basic", GOURAUD)[3], len(f))
    with pytest.raises(ValueError):
        gpu_ctx.last_surface_shading(3)                       # (more surfaces than room: nothing silently cut)


def _paths():
    return ["painter", "fmt8", "float", "ortho", "fog", "keyed", "placed", "posed", "resident"]


@pytest.mark.gpu
@pytest.mark.parametrize("path", _paths())
def test_reduced_lists_through_every_path(gpu_ctx, keyed_ctx, oracle, path):
    """The reduced set of lists, flat and Gouraud, through the paths that are not the drop-in call in z-buffer mode."""
    from bonnie32_amd import rasterizer as R
    v, f, tex = mesh()
    ctx = keyed_ctx if path == "keyed" else gpu_ctx
    fb = R.Framebuffer(W, H, ctx)
    for case in REDUCED:
        for shading in (FLAT, GOURAUD):
            what = f"{path}/{case}/{shading}"
            if path in ("painter", "float", "ortho", "keyed"):
                kw = {"painter": dict(use_zbuffer=False), "float": dict(use_fixed_point=False), "keyed": {},
                      "ortho": dict(ortho_projection=(0.06, 10.0, -20.0))}[path]
                ref = reference(oracle, case, shading, **kw)
                fb.clear(CLEAR)
                tm = R.render_mesh_15(fb, v, f, tex, CAM, settings_for(case, shading, **kw))
                check_frame(fb, tm, ref, zmode=path != "painter", what=what)
                check_tap(ctx, ref[3], len(f), what)
            elif path == "fmt8":                               # shade8 does not clamp: negative shades reach the channel product
                ref = reference(oracle, case, shading, fmt8=True)
                fb.clear(CLEAR)
                tm = R.render_mesh(fb, v, f, tex8(), CAM, settings_for(case, shading))
                check_frame(fb, tm, ref, what=what)
                check_tap(ctx, ref[3], len(f), what)
            elif path == "fog":
                fog = (2600.0, 800.0, 3400.0, b32.Color(90, 20, 200, 3))
                st = settings_for(case, shading)
                ofb = oracle.Framebuffer(W, H); ofb.clear(CLEAR)
                rc, etm, d = oracle.render_mesh_15(ofb, v, f, tex, CAM, st, fog, dump=True)
                assert rc == 0
                fb.clear(CLEAR)
                tm = R.render_mesh_15(fb, v, f, tex, CAM, st, fog)
                check_frame(fb, tm, (ofb.pixels, ofb.zbuffer.view(np.uint32), etm, d), what=what)
                check_tap(ctx, d, len(f), what)
            elif path == "placed":                             # rotated by 0.7 rad with an offset, against place_vertices on the host
                pl = b32.Placement(facing=0.7, world_pos=(-600.0, 50.0, 900.0))
                ref = reference(oracle, case, shading, geometry=(pl.apply(v), f, tex), key="placed")
                rs = R.ResidentScene(fb, v, f, tex)
                fb.clear(CLEAR); rs.render_async(CAM, settings_for(case, shading), placement=pl); tm = rs.finish()
                check_frame(fb, tm, ref, what=what)
                check_tap(ctx, ref[3], len(f), what)
            elif path == "posed":                              # two bones, one of them rotated, against pose_vertices
                bo = np.where(np.arange(len(v)) % 5 == 4, abi.BONE_NONE, np.arange(len(v)) % 2).astype(np.uint16)
                bones = [b32.Bone.from_euler((30.0, -20.0, 100.0), (0.0, 0.0, 0.0)), b32.Bone.from_euler((-50.0, 40.0, 300.0), (17.0, 0.0, -11.0))]
                ref = reference(oracle, case, shading, geometry=(b32.pose_vertices(v, bo, bones), f, tex), key="posed")
                rs = R.ResidentScene(fb, v, f, tex)
                rs.set_rig(bo); rs.pose(bones)
                fb.clear(CLEAR); rs.render_async(CAM, settings_for(case, shading)); tm = rs.finish()
                check_frame(fb, tm, ref, what=what)
                check_tap(ctx, ref[3], len(f), what)
            elif path == "resident":                           # 8640 faces: 36-byte vertices on frame 1, the packed lit stream on frame 3
                if shading == FLAT and case not in ("basic", "n17"):
                    continue
                bv, bf, _ = big_mesh()
                ref = reference(oracle, case, shading, geometry=(bv, bf, tex), key="big")
                rs = R.ResidentScene(fb, bv, bf, tex)
                assert len(bf) > 8192
                for frame in range(3):
                    fb.clear(CLEAR); rs.render_async(CAM, settings_for(case, shading)); tm = rs.finish()
                    if frame != 1:
                        check_frame(fb, tm, ref, what=f"{what}/frame {frame}")
                        check_tap(ctx, ref[3], len(bf), f"{what}/frame {frame}")


@pytest.mark.gpu
def test_light_count_changes_between_asynchronous_frames(oracle):
    """17, 9, 8 and 17 lights in consecutive asynchronous frames of one context: across the switch between the inline light table and the
    device buffer, and the buffer's "unchanged" shortcut on the second 17.  Every frame is delivered by ticket and compared."""
    from bonnie32_amd import rasterizer as R
    v, f, tex = mesh()
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        rs = R.ResidentScene(fb, v, f, tex)
        seq = ["n17", "n9", "n8", "n17"]
        bufs = [ctx.host_alloc(W * H * 4) for _ in seq]
        tickets = []
        for case, (_arr, p) in zip(seq, bufs):
            fb.clear(CLEAR); rs.render_async(CAM, settings_for(case, GOURAUD))
            tickets.append(ctx.download_async(p))
        for k, case in enumerate(seq):
            ctx.ticket_wait(tickets[k])
            px = reference(oracle, case, GOURAUD)[0]
            assert np.array_equal(bufs[k][0], px), f"frame {k} ({case}): {int((bufs[k][0] != px).sum())} bytes differ"
        tm = rs.finish()
        ref = reference(oracle, "n17", GOURAUD)
        check_frame(fb, tm, ref, what="last frame")
        check_tap(ctx, ref[3], len(f), "last frame")
        # ... and with the tap after every frame
        for case in seq:
            fb.clear(CLEAR); rs.render_async(CAM, settings_for(case, FLAT)); tm = rs.finish()
            ref = reference(oracle, case, FLAT)
            check_frame(fb, tm, ref, what=case)
            check_tap(ctx, ref[3], len(f), case)
        for _arr, p in bufs:
            ctx.host_free(p)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_merged_batch_with_hostile_ambients_and_fogs(oracle):
    """b32_frame_submit of three copies of the mesh, each with an ambient and a fog of its own, against sequential oracle calls (frame
    level: the tap refuses a batch)."""
    from bonnie32_amd import rasterizer as R
    v, f, tex = mesh()
    copies = []
    for dx, dz in ((0.0, 0.0), (-220.0, 350.0), (260.0, 700.0)):
        c = v.copy(); c["pos"][:, 0] += f32(dx); c["pos"][:, 2] += f32(dz)
        copies.append(c)
    # (meshes commute, and are merged into one draw, up to and including the first one with a transparent pass: only the last copy keeps
    # its blended faces)
    f_opaque = f.copy(); f_opaque["blend_mode"] = abi.OPAQUE; f_opaque["editor_alpha"] = 255
    face_lists = [f_opaque, f_opaque, f]
    ambients = [NAN, -1.0, 5.0]
    fogs = [(2600.0, NAN, 1e9, FOG_RGB), (NAN, 800.0, 3300.0, FOG_RGB), (2600.0, -5.0, 1e9, b32.Color(90, 20, 200, 3))]
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(W, H, ctx)
        slots = [R.ResidentScene(fb, c, fl, tex).detach() for c, fl in zip(copies, face_lists)]
        for shading in (FLAT, GOURAUD):
            st = settings_for("basic", shading)
            ofb = oracle.Framebuffer(W, H); ofb.clear(CLEAR)
            for c, fl, amb, fog in zip(copies, face_lists, ambients, fogs):
                st_i = settings_for("basic", shading, ambient=amb)
                assert oracle.render_mesh_15(ofb, c, fl, tex, CAM, st_i, fog)[0] == 0
            before = ctx.batch_counts()["merged_draws"]
            fb.clear(CLEAR)
            ctx.frame_submit(ctx.make_frame_table(CAM, st, slots, fogs=fogs, ambients=ambients))
            ctx.finish()
            assert ctx.batch_counts()["merged_draws"] == before + 1
            got = fb.pixels
            assert np.array_equal(got, ofb.pixels), f"{int((got != ofb.pixels).sum())} bytes differ"
            assert np.array_equal(fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32))
            with pytest.raises(R.B32Error):
                ctx.last_surface_shading(len(f))
    finally:
        ctx.close()
