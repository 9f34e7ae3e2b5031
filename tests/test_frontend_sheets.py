"""The front end face by face: near reject, area sign, fog cull, painter's key and class, draw order, per-pixel depth (tests/frontend_sheets.py
builds the sheets).

k_setup decides per face whether it is drawn (render.rs:2381-2453) and where it stands in the order (render.rs:2518-2545); the fill never
sees that order on the default route but takes, per pixel, the maximum of (painter's key << 32) | face id -- in z-buffer mode of
(~depth key << 32) | 0xFFFFFFFE - face id.  On a sheet every face has a cell of its own, or shares one screen triangle with the faces it
is ordered against, each in its own flat colour: a wrong verdict is a cell that is clear or coloured where it should not be, a wrong
priority is a cell of the wrong colour, and both show in b32_last_draw_order.

CPU tests (no mark): three restatements agree on every sheet and mode -- the C oracle, oracle/np_model.py, and `decide` below, a statement
of the decisions alone with exact rational arithmetic rounded once per f32 operation; a census from the projected bits shows that every
case the families aim at is realised; every one-point mutation of `decide` changes a named sheet.  GPU tests: every sheet drop-in and
resident, fragment counting on and off, on each binning route, through the 8-bit-colour path, as a batched frame, placed, in row bands,
family D drawn twice onto one z-buffer, and family V's NaN verdicts on the three routes that carry a copy of the rule.

Measured: cells changed by each one-point mutation of `decide`, summed over the sheets named in MUTATIONS (and asserted, MEASURED_MUTATIONS):
near `<=` -> `<` 289; near any -> all 1260; area `<= 0` -> `< 0` 388; area with one emulated FMA 61 (A-float 31, A-ortho 30); fog `>` -> `>=` 48;
fog all -> any 108; key summed before the back-face swap 12; key * (1/3) 12; key without the + 5.0 26; painter's ties to the earlier face 240;
-0.0 < +0.0 in the orthographic key 8; transparent faces sorted with the opaque ones 124; z-buffer mode sorting its opaque list 56; z-buffer
ties to the later face 130 all-tie cells of the D and K sheets; the NaN verdict at list length >= 1: 72 of 204 family-V draws.

Measured once on an MI355X: the 92 GPU tests take 2.2 s.  The library built with B32_EXTRA_FLAGS="-ffp-contract=fast" fails sheet A in float
projection: with culling on 27 faces (collinear, zero, fma_a, fma_b, tiny and tiny_back cells) enter or leave the draw order -- 95 surfaces
instead of 80 -- and 9 cells differ in pixels; with culling off or x-ray 17 cells differ.  It also fails 30 / 48 / 44 cells of D-fixed / -float /
-ortho (before the one-ulp pairs were picked by their reciprocals), 30 (painter's) and 42 (z-buffer) cells of K-float, 3 cells of K-fixed and 9 of K-ortho in z-buffer mode, and 3 to 5 cells of F-float.
Sheet A in orthographic projection does NOT change, although its fma_a / fma_b cells flip under either single-FMA form of the area by exact
arithmetic (test_census_a): the compiler does not contract that expression to another verdict.  The same expression serves every projection,
so the float-projection failures must come from the arithmetic in front of it: the contracted projection (x * us / denom * vs + W / 2) moves
the coordinates of near-degenerate triples by an ulp, and their area across zero."""
import copy
import math
from fractions import Fraction

import numpy as np
import pytest

from bonnie32_amd import abi
from bonnie32_amd.rtypes import Camera
from oracle import np_model as M
from tests import frontend_sheets as FS

gpu = pytest.mark.gpu
f32 = np.float32
BIN_ROUTES = ("direct_bin", "inline_bin", "counting_sort", "keyed")
MODES8 = [("8-bit", None, {"fmt8": True}), ("8-bit zbuffer", None, {"fmt8": True, "zbuffer": True})]


def all_modes(sh):
    return FS.modes(sh) + (MODES8 if sh.family in "NAK" else [])


# ------------------------------------------------------------------------------------------------ the decisions, restated
class NanKey(Exception):
    """the reference's `partial_cmp(..).unwrap()` panic (render.rs:2531)"""


def _add(a, b):
    """a + b in f32, rounded once (exact rational sum; the sign of a zero sum and non-finite operands by IEEE's rules)"""
    a, b = float(a), float(b)
    if math.isfinite(a) and math.isfinite(b):
        s = Fraction(a) + Fraction(b)
        if s == 0:
            return -0.0 if (math.copysign(1.0, a) < 0 and math.copysign(1.0, b) < 0) else 0.0
        return float(FS.rne32(s))
    with np.errstate(all="ignore"):
        return float(f32(a) + f32(b))


def _third(s, mul):
    s = float(s)
    if not math.isfinite(s):
        return s
    if s == 0:
        return s
    if mul:
        with np.errstate(all="ignore"):
            return float(FS.rne32(Fraction(s) * Fraction(float(f32(1.0) / f32(3.0)))))
    return float(FS.rne32(Fraction(s) / 3))


def _back_face(v1, v2, v3, mut):
    """signed_area <= 0 (render.rs:2393-2394) on f32 screen points"""
    pts = [float(t) for v in (v1, v2, v3) for t in v[:2]]
    if all(math.isfinite(t) for t in pts):
        fm = FS.area_forms(v1, v2, v3)
        area = fm["fma_a"] if mut == "area_fma" else fm["chain"]
    else:
        with np.errstate(all="ignore"):
            area = float((v2[0] - v1[0]) * (v3[1] - v1[1]) - (v3[0] - v1[0]) * (v2[1] - v1[1]))
    return area < 0 if mut == "area_lt" else area <= 0


def face_key(d, mut=None):
    """((d1 + d2) + d3) / 3.0f on the Surface's vertex order (render.rs:2529-2531)"""
    if mut == "assoc_other":
        d = (d[0], d[2], d[1])
    return _third(_add(_add(d[0], d[1]), d[2]), mut == "mul_third")


def decide(scr, camz, faces, proj, cull, xray=False, zbuffer=False, fmt8=False, fog_cd=None, mut=None):
    """The draw order render_mesh_15 arrives at (render.rs:2375-2545), from projected vertices alone: near reject on the camera depths,
    area sign, fog cull, back-face cull, key and class, two stable descending sorts.  `mut` names a one-point change (MUTATIONS)."""
    near = float(FS.NEAR)
    survivors = []                                           # (face, key, transparent)
    for fi in range(len(faces)):
        ids = [int(k) for k in faces["v"][fi]]
        cz = [float(camz[i]) for i in ids]
        if proj != "ortho":                                                          # :2381-2385
            rej = [(z < near) if mut == "near_lt" else (z <= near) for z in cz]
            if (all(rej) if mut == "near_all" else any(rej)):
                continue
        v = [scr[i] for i in ids]
        back = _back_face(v[0], v[1], v[2], mut)
        if fog_cd is not None:                                                       # :2419-2422
            cd = float(f32(fog_cd))
            beyond = [(z >= cd) if mut == "fog_ge" else (z > cd) for z in cz]
            if (any(beyond) if mut == "fog_any" else all(beyond)):
                continue
        if back and cull and not xray:                                               # :2451-2453
            continue
        order = (0, 2, 1) if (back and mut != "sum_before_swap") else (0, 1, 2)      # the Surface holds v1, v3, v2 of a back face
        if mut == "no_plus5" and proj != "ortho":                                    # (float projection's depth is cam.z + 5.0 as well, math.rs:118)
            d = [cz[k] for k in order]
        else:
            d = [float(v[k][2]) for k in order]
        key = face_key(d, mut)
        transparent = (int(faces["blend_mode"][fi]) != 0 or int(faces["editor_alpha"][fi]) < 255) and not fmt8      # :2175-2184: render_mesh never partitions
        if mut == "one_list":
            transparent = False
        survivors.append((fi, key, transparent))

    def rank(k):
        if mut == "abs_key":
            k = abs(k)
        if mut == "flush_denormals" and abs(k) < 2.0 ** -126:
            k = 0.0
        if mut == "drop_lsb" and k > 0 and math.isfinite(k):
            return float(FS.bits(k) >> 1)
        return k

    def painter(lst):
        if len(lst) >= (1 if mut == "nan_len1" else 2) and any(k != k for _, k, _ in lst):
            raise NanKey()
        if mut == "painter_tie_earlier":
            return sorted(lst, key=lambda s: (-rank(s[1]), -s[0]))
        if mut == "ascending":
            return sorted(lst, key=lambda s: rank(s[1]))
        if mut == "neg_zero_less":
            return sorted(lst, key=lambda s: (-rank(s[1]), s[1] == 0 and math.copysign(1.0, s[1]) < 0))
        return sorted(lst, key=lambda s: -rank(s[1]) if rank(s[1]) == rank(s[1]) else 0.0)      # (stable; -0.0 == +0.0)
    opaque = [s for s in survivors if not s[2]]
    transp = [s for s in survivors if s[2]]
    if not zbuffer or mut == "z_sorts_opaque":                                       # :2535: z-buffer mode leaves the opaque list in face order
        opaque = painter(opaque)
    transp = painter(transp)
    seq = (transp + opaque) if mut == "transparent_first" else (opaque + transp)
    return [s[0] for s in seq]


def decide_sheet(sh, fog_name=None, mut=None, **mode):
    scr, camz = sh.projected()
    return decide(scr, camz, sh.faces, sh.proj, sh.cull if mode.get("cull") is None else mode["cull"], xray=bool(mode.get("xray")),
                  zbuffer=bool(mode.get("zbuffer")), fmt8=bool(mode.get("fmt8")), fog_cd=FS.FOG_DISTANCES[fog_name] if fog_name else None, mut=mut)


def cell_sequences(sh, order):
    """per cell, its faces in draw order"""
    out = [[] for _ in sh.cell_tag]
    for fi in order:
        out[int(sh.cell_of[fi])].append(int(fi))
    return [tuple(s) for s in out]


def visible(sh, seq):
    """what of a cell's draw sequence shows when its faces share one triangle: the last face that overwrites (editor_alpha 255: an
    untextured face of blend mode Average has no semi-transparent texel and stores its colour as it is) and the alpha faces after it"""
    last = max([k for k, fi in enumerate(seq) if sh.meta[fi].alpha == 255], default=0)
    return tuple(seq[last:])


def changed_cells(sh, mut, fog_name=None, **mode):
    """cells whose draw sequence changes under the mutation (all of them when the verdict changes to a panic)"""
    a = cell_sequences(sh, decide_sheet(sh, fog_name, **mode))
    try:
        b = cell_sequences(sh, decide_sheet(sh, fog_name, mut=mut, **mode))
    except NanKey:
        return list(range(len(a)))
    return [c for c in range(len(a)) if a[c] != b[c]]


# ------------------------------------------------------------------------------------------------ CPU: three restatements agree
def _model(sh, fog_name, mode):
    px = np.zeros(sh.width * sh.height * 4, np.uint8)
    px.reshape(-1, 4)[:] = [FS.CLEAR.r, FS.CLEAR.g, FS.CLEAR.b, 255]
    zb = np.full(sh.width * sh.height, np.finfo(f32).max, f32)
    st = sh.settings(**mode)
    with np.errstate(all="ignore"):
        if mode.get("fmt8"):
            r = M.render_mesh(px, sh.width, sh.height, sh.vertices, sh.faces, sh.textures8(), sh.camera, st, zbuffer=zb)
        else:
            r = M.render_mesh_15(px, sh.width, sh.height, sh.vertices, sh.faces, sh.textures, sh.camera, st, FS.fog(fog_name) if fog_name else None, zbuffer=zb)
    return px, zb.view(np.uint32), r


@pytest.mark.parametrize("name", FS.NAMES)
def test_three_restatements_agree(oracle, name):
    """C oracle (stage dump), numpy model and `decide`: the same draw order in every mode; oracle and model also the same pixels and
    z-buffer bits.  The projection `decide` starts from is the dump's: depths bit for bit, fixed-point columns and rows exactly."""
    sh = FS.sheet(name)
    scr, camz = sh.projected()
    for label, fog_name, mode in all_modes(sh):
        o = sh.oracle(oracle, fog_name, **mode)
        assert o["rc"] == 0, (name, label)
        d = o["dump"]
        want = [int(x) for x in d["draw_order"]]
        assert o["tm"].triangles_drawn == len(want)
        got = decide_sheet(sh, fog_name, **mode)
        assert got == want, f"{name} {label}: decide and the oracle differ, first at position {next(i for i, (a, b) in enumerate(zip(got + [-1], want + [-1])) if a != b)}"
        px, zb, r = _model(sh, fog_name, mode)
        assert [int(x) for x in r["draw_order"]] == want, (name, label)
        msg = sh.first_difference(px, o["px"], f"model, {label}")
        assert not msg, msg
        if mode.get("zbuffer"):
            msg = sh.first_difference(zb, o["zb"], f"model depths, {label}")
            assert not msg, msg
        assert r["triangles_drawn"] == o["tm"].triangles_drawn and r["fragments"] == o["tm"].fragments, (name, label)
    assert np.array_equal(d["sz"].view(np.uint32), scr[:, 2].view(np.uint32)), name
    if sh.proj == "fixed":
        assert np.array_equal(d["sx"], scr[:, 0].astype(np.int64)) and np.array_equal(d["sy"], scr[:, 1].astype(np.int64)), name


def test_second_draw_of_sheet_d_agrees(oracle):
    """family D drawn twice onto one z-buffer, the second time with the two colours of every cell swapped: every fragment of the second
    draw ties with the stored depth or loses, so nothing changes (strict `<`); oracle and model say so alike"""
    for proj in FS.PROJS:
        first, second = FS.sheet(f"D-{proj}"), FS.sheet(f"D-{proj}-second")
        assert np.array_equal(first.vertices["pos"].view(np.uint32), second.vertices["pos"].view(np.uint32))
        assert not np.array_equal(first.vertices["r"], second.vertices["r"])
        px, zb = d_second_oracle(oracle, proj)
        o = first.oracle(oracle, None, zbuffer=True)
        assert np.array_equal(px, o["px"].reshape(-1)) and np.array_equal(zb, o["zb"])


def d_second_oracle(O, proj):
    """(pixels, z-buffer bits) after D-<proj> and then D-<proj>-second on one framebuffer, z-buffer mode"""
    first, second = FS.sheet(f"D-{proj}"), FS.sheet(f"D-{proj}-second")
    fb = O.Framebuffer(first.width, first.height)
    fb.clear(FS.CLEAR)
    for sh in (first, second):
        rc, _ = O.render_mesh_15(fb, sh.vertices, sh.faces, [], sh.camera, sh.settings(zbuffer=True))
        assert rc == 0
    return fb.pixels.copy(), fb.zbuffer.view(np.uint32).copy()


# ------------------------------------------------------------------------------------------------ CPU: census
@pytest.mark.parametrize("name", FS.NAMES)
def test_faces_stay_in_their_cells(oracle, name):
    """every vertex projects into its face's own cell (so no two faces of different cells can share a stored pixel: the fill stores
    inside the bounding box only), and the oracle's frames are clear outside the cells' triangles' boxes"""
    sh = FS.sheet(name)
    scr, _ = sh.projected()
    xy = scr[:, :2].reshape(sh.n, 3, 2)
    org = sh.cell_xy[sh.cell_of][:, None, :]
    assert ((xy >= org) & (xy < org + sh.cell)).all(), f"{name}: face {int(np.nonzero(~((xy >= org) & (xy < org + sh.cell)).all(axis=(1, 2)))[0][0])} leaves its cell"
    box = np.zeros((sh.height, sh.width), bool)
    for i in range(sh.n):
        x0, y0 = np.floor(xy[i].min(axis=0)).astype(int); x1, y1 = np.floor(xy[i].max(axis=0)).astype(int)
        box[y0:y1 + 1, x0:x1 + 1] = True
    for label, fog_name, mode in all_modes(sh):
        px = sh.oracle(oracle, fog_name, **mode)["px"]
        drawn = (px[..., :3] != (FS.CLEAR.r, FS.CLEAR.g, FS.CLEAR.b)).any(axis=2)
        assert not (drawn & ~box).any(), (name, label)
        if sh.family in "NFD" and not mode.get("fmt8"):           # flat opaque faces: a pixel's colour names a face of the pixel's own cell
            idx = sh.decode(px)
            ys, xs = np.nonzero(idx >= 0)
            per_row = sh.width // sh.cell
            assert np.array_equal(sh.cell_of[idx[ys, xs]], (ys // sh.cell) * per_row + xs // sh.cell), (name, label)


def _kept(sh, oracle, fog_name=None, **mode):
    return set(int(x) for x in sh.oracle(oracle, fog_name, **mode)["dump"]["draw_order"])


@pytest.mark.parametrize("proj", FS.PROJS)
@pytest.mark.parametrize("fam", ["N", "Nrot"])
def test_census_n(oracle, fam, proj):
    """For every subset of the vertex slots and every edge value there is a face whose camera depths have exactly those bits on the
    subset and lie comfortably behind the plane elsewhere (the rotated camera: 0.1f and its two neighbours, the bits dot3 gives);
    perspective keeps exactly the faces with every depth above 0.1f, orthographic projection keeps all."""
    sh = FS.sheet(f"{fam}-{proj}")
    _, camz = sh.projected()
    cz = camz.reshape(sh.n, 3)
    kept = _kept(sh, oracle)
    names = list(FS.N_VALUES) if fam == "N" else ["near", "near+", "near-"]
    if fam == "Nrot" and proj == "ortho":
        names = []                                               # (not snapped: the plane is ignored; the draw count below is the check)
    for slots in FS.SLOTS:
        rest = [s for s in range(3) if s not in slots]
        for vn in names:
            want = FS.bits(FS.N_VALUES[vn])
            hit = [i for i in range(sh.n) if all(FS.bits(cz[i, s]) == want for s in slots) and all(cz[i, s] > FS.up(FS.NEAR) for s in rest)]
            assert hit, f"{sh.name}: no face with camera depth {vn} exactly on slots {slots}"
            if proj != "ortho":
                assert all((i in kept) == (vn == "near+") for i in hit), (sh.name, slots, vn)
    if proj == "ortho":
        assert len(kept) == sh.n
    else:
        assert kept == {i for i in range(sh.n) if (cz[i] > FS.NEAR).all()} and 0 < len(kept) < sh.n


@pytest.mark.parametrize("proj", ["fixed", "float"])
def test_census_n_placed(oracle, proj):
    """The placed form of sheet N: the local vertices' depths are NOT the edge values, the placed ones (Placement.apply, the host
    restatement of place_vertex) are -- 0.1f and its two neighbours on every subset of the slots -- and the oracle keeps exactly the faces
    whose placed camera depths are all above 0.1f."""
    sh = FS.sheet(f"N-{proj}")
    local, pl = FS.placed_n(proj)
    assert pl.has_transform
    placed = pl.apply(local)
    cz = FS.project(placed["pos"], sh.camera, proj, sh.width, sh.height)[1].reshape(sh.n, 3)
    lz = local["pos"][:, 2].reshape(sh.n, 3)
    for slots in FS.SLOTS:
        rest = [s for s in range(3) if s not in slots]
        for vn in ("near", "near+", "near-"):
            want = FS.bits(FS.N_VALUES[vn])
            hit = [i for i in range(sh.n) if all(FS.bits(cz[i, s]) == want for s in slots) and all(cz[i, s] > FS.up(FS.NEAR) for s in rest)]
            assert hit, (proj, slots, vn)
            assert any(all(FS.bits(lz[i, s]) != want for s in slots) for i in hit), (proj, slots, vn)
    ofb = oracle.Framebuffer(sh.width, sh.height); ofb.clear(FS.CLEAR)
    rc, otm, d = oracle.render_mesh_15(ofb, placed, sh.faces, [], sh.camera, sh.settings(), dump=True)
    assert rc == 0 and set(int(x) for x in d["draw_order"]) == {i for i in range(sh.n) if (cz[i] > FS.NEAR).all()}
    assert 0 < otm.triangles_drawn < sh.n


@pytest.mark.parametrize("proj", FS.PROJS)
def test_census_a(oracle, proj):
    """Integer cases (fixed point and orthographic, where the screen coordinates are the integers aimed at): collinear and coincident
    triples have signed area exactly 0 and are back faces, area +1 is kept and -1 culled.  Searched cases (float and orthographic):
    every class is realised by the exact rational restatement of the projected points.  Empty surfaces are in the draw order and store
    nothing; with culling off or x-ray every face is a surface."""
    sh = FS.sheet(f"A-{proj}")
    scr, _ = sh.projected()
    tri = scr.reshape(sh.n, 3, 3)
    forms = [FS.area_forms(*tri[i]) for i in range(sh.n)]
    kept = _kept(sh, oracle)
    assert _kept(sh, oracle, cull=False) == _kept(sh, oracle, xray=True) == set(range(sh.n))
    tags = {}
    for i, m in enumerate(sh.meta):
        tags.setdefault(m.tag, []).append(i)
    if proj != "float":
        for t in ("collinear", "collinear-reversed", "collinear-flat", "coincident-12", "coincident-23", "coincident-13", "coincident-123"):
            assert tags[t] and all(forms[i]["chain"] == 0 and forms[i]["exact"] == 0 and i not in kept for i in tags[t]), t
        for t in ("area+1", "area+1-rotated"):
            assert all(forms[i]["chain"] == 1 and i in kept for i in tags[t]), t
        for t in ("area-1", "area-1-rotated"):
            assert all(forms[i]["chain"] == -1 and i not in kept for i in tags[t]), t
    assert all(i in kept for i in tags["front"]) and not any(i in kept for i in tags["back"])
    idx_count = np.bincount(sh.decode(sh.oracle(oracle)["px"]).reshape(-1) + 1, minlength=sh.n + 1)[1:]
    if proj != "fixed":
        for i in tags["zero"]:
            assert forms[i]["chain"] == 0 and forms[i]["exact"] != 0 and i not in kept
        assert any(forms[i]["exact"] > 0 for i in tags["zero"]), "no face whose exact area is positive and whose f32 area is 0"
        for k in ("fma_a", "fma_b"):
            assert tags[k] and all((forms[i][k] <= 0) != (forms[i]["chain"] <= 0) for i in tags[k]), k
        ar = FS._area_1500(tri[:, :, :2])
        for i in tags["tiny"]:
            assert forms[i]["chain"] > 0 and 0 < abs(ar[i]) < FS.AREA_EPS and i in kept and idx_count[i] == 0
        for i in tags["tiny_back"]:
            assert forms[i]["chain"] < 0 and i not in kept
        for i in tags["subpixel"]:
            assert forms[i]["chain"] > 0 and i in kept and idx_count[i] == 0
    assert 0 < len(kept) < sh.n
    # attribute swap: a back face drawn with culling off maps its colours / UVs as the Surface (v1, v3, v2) does -- another image than the
    # front face of the same three points gives, which is what a swap of the positions alone would draw
    off = sh.oracle(oracle, None, cull=False)["px"]
    for kind in ("gradient", "textured"):
        pairs = 0
        for b in tags[kind + "-back"]:
            tb = sh.meta[b].tri
            f = next(i for i in tags[kind + "-front"] if sh.meta[i].tri == (tb[0], tb[2], tb[1]))
            bx0, by0, bx1, by1 = sh.window(int(sh.cell_of[b])); fx0, fy0, fx1, fy1 = sh.window(int(sh.cell_of[f]))
            assert b not in kept and f in kept
            assert not np.array_equal(off[by0:by1, bx0:bx1], off[fy0:fy1, fx0:fx1]), (kind, b, f)
            pairs += 1
        assert pairs >= 4


@pytest.mark.parametrize("proj", FS.PROJS)
def test_census_f(oracle, proj):
    """camera depths exactly at each centre distance and its neighbours on every subset of the slots, the other vertices beyond or in front;
    every class has a culled and a kept member at its own distance; NaN never culls, -inf culls whatever passed the near plane"""
    sh = FS.sheet(f"F-{proj}")
    _, camz = sh.projected()
    cz = camz.reshape(sh.n, 3)
    passes = [i for i in range(sh.n) if proj == "ortho" or (cz[i] > FS.NEAR).all()]
    for fog_name, C in (("normal", 12.0), ("zero", 0.0), ("negative", -1.0)):
        kept = _kept(sh, oracle, fog_name)
        assert kept == {i for i in passes if not (cz[i] > f32(C)).all()}, fog_name
        if proj != "ortho" and C <= 0:
            continue                                             # (perspective: the near plane has taken these faces already)
        for slots in FS.SLOTS:
            rest = [s for s in range(3) if s not in slots]
            for vn, val in (("at", f32(C)), ("above", FS.up(C)), ("below", FS.down(C))):
                for far in (True, False):
                    hit = [i for i in passes if all(FS.bits(cz[i, s]) == FS.bits(val) for s in slots) and all((cz[i, s] > FS.up(C)) == far and cz[i, s] != val for s in rest)]
                    assert hit, (sh.name, fog_name, slots, vn, far)
                    culled = vn == "above" and (far or not rest)                 # every vertex strictly beyond the distance
                    assert all((i in kept) == (not culled) for i in hit), (sh.name, fog_name, slots, vn, far)
    assert _kept(sh, oracle, "nan") == _kept(sh, oracle, "+inf") == set(passes)
    assert _kept(sh, oracle, "-inf") == set() and passes


def _keys(sh, fi):
    scr, _ = sh.projected()
    d = [float(scr[int(k)][2]) for k in sh.faces["v"][fi]]
    return face_key(d), d


@pytest.mark.parametrize("proj", FS.PROJS)
def test_census_k(oracle, proj):
    """Every case has the bits it claims, and in its cells what is visible depends on the rule under test: recomputed with the rule's
    nearest alternative (the third field of the cell's tag) the visible part of the draw sequence changes -- in both face orders where
    the rule is a tie-break, in at least one of the two where a tie stands against a strict order."""
    sh = FS.sheet(f"K-{proj}")
    base = cell_sequences(sh, decide_sheet(sh))
    per_case, others = {}, {}
    for c, tag in enumerate(sh.cell_tag):
        case, alt, _ = tag[2:].split("|")
        if alt not in others:
            others[alt] = cell_sequences(sh, decide_sheet(sh, mut=alt))
        other = others[alt]
        per_case.setdefault((case, alt), []).append(visible(sh, base[c]) != visible(sh, other[c]))
        fcs = [i for i in sh.cell_faces(c) if sh.meta[i].tag != "rejected"]
        ks = [_keys(sh, i) for i in fcs]
        if case == "keys one ulp apart" or case == "negative keys one ulp apart":
            assert abs(FS.bits(ks[0][0]) - FS.bits(ks[1][0])) == 1, tag
        if case.startswith("equal keys") or case.startswith("three equal"):
            assert len({FS.bits(k) for k, _ in ks}) == 1, tag
        if case == "equal keys, different triples":
            assert ks[0][1] != ks[1][1]
        if case.startswith("non-associative"):
            x = next(d for (k, d), i in zip(ks, fcs) if len(set(d)) == 3)
            assert _add(_add(x[0], x[1]), x[2]) != _add(_add(x[0], x[2]), x[1]), tag
        if case.startswith("/ 3.0f"):
            assert ks[0][0] == ks[1][0] and face_key(ks[0][1], "mul_third") != face_key(ks[1][1], "mul_third"), tag
        if case == "camera depths equal after + 5.0":
            _, camz = sh.projected()
            a, b = (camz[int(sh.faces["v"][i][0])] for i in fcs)
            assert a != b and ks[0][0] == ks[1][0], tag
        if case.startswith("sums overflow"):
            assert all(k == math.inf for k, _ in ks) and ks[0][1] != ks[1][1], tag
        if case.startswith("-0.0 against"):
            assert sorted(math.copysign(1.0, k) for k, _ in ks) == [-1.0, 1.0] and all(k == 0 for k, _ in ks), tag
        if case.startswith("denormal against"):
            assert any(0 < k < 2.0 ** -126 for k, _ in ks), tag
        if case.startswith("-inf key"):
            assert any(k == -math.inf for k, _ in ks), tag
        if case.startswith("depth 3e38"):
            assert max(max(d) for _, d in ks) >= 2.9e38, tag
        if case.startswith("depth 1e37"):
            assert max(max(d) for _, d in ks) >= 9.9e36 and sh.proj == "float", tag
    for (case, alt), flags in per_case.items():
        need = len(flags) if alt in ("painter_tie_earlier", "one_list", "transparent_first", "ascending", "abs_key") and "four faces" not in case else len(flags) // 2
        assert sum(flags) >= need, f"{sh.name} '{case}': the alternative '{alt}' changes {sum(flags)} of {len(flags)} cells"
    trans = [i for i in range(sh.n) if sh.faces["blend_mode"][i] != 0 or sh.faces["editor_alpha"][i] < 255]
    order = decide_sheet(sh)
    assert trans and set(order[-len(trans):]) == set(trans), "the transparent faces are drawn after every opaque face"


@pytest.mark.parametrize("proj", FS.PROJS)
def test_census_d(oracle, proj):
    """every D cell but the deliberate tie cells shows both faces (pixels on both sides of the crossing line) -- which no per-face
    depth, the nearest alternative to the interpolated 1 / (bc . 1/z), can produce; an all-tie cell shows its first face only (strict `<`),
    an edge-tie cell with the nearer face first shows the other one on the shared edge at most"""
    sh = FS.sheet(f"D-{proj}")
    idx = sh.decode(sh.oracle(oracle, None, zbuffer=True)["px"])
    ties = edge_ties = ulp = 0
    for c, tag in enumerate(sh.cell_tag):
        x0, y0, x1, y1 = sh.window(c)
        seen = set(int(v) for v in np.unique(idx[y0:y1, x0:x1]) if v >= 0)
        a, b = sh.cell_faces(c)
        if tag.startswith("D all tie"):
            assert seen == {a}, sh.describe_cell(c); ties += 1
        elif tag == "D equal along an edge|reversed":
            # a deliberate edge-tie cell, (a, a, a + 1) in front of (a, a, b > a + 1): no crossing line.  The second face is behind everywhere
            # but on the shared edge v1 v2 (the cell's row 1), where both depths are a up to the rounding of 1 / (bc . 1/z): it shows there or nowhere
            assert a in seen and seen <= {a, b}, sh.describe_cell(c)
            # (float projection: the two faces' vertices are rounded from different depths and differ in the last bits, so the second face may
            #  also cover a pixel of the triangle's outline that the first one misses)
            ys, xs = np.nonzero(idx[y0:y1, x0:x1] == b)
            outline = (ys == 1) | (xs == 1) | (xs + ys == 15)
            assert (outline if proj == "float" else ys == 1).all(), sh.describe_cell(c); edge_ties += 1
        else:                                   # one ulp apart included: d_pairs picks neighbours whose reciprocals differ
            assert seen == {a, b}, sh.describe_cell(c)
            ulp += "one ulp apart" in tag
    assert ties >= 8 and edge_ties >= 8 and ulp >= 2 * (12 if proj == "ortho" else 17)


# ------------------------------------------------------------------------------------------------ CPU: family V by the three restatements
V_CASES = [(comp, nf, first, proj, z) for comp in FS.V_COMPOSITIONS for nf in (2, 65, 257) for first in (True, False) for proj in FS.PROJS for z in (False, True)
           if (comp != "backface_culled" or proj == "fixed") and (comp != "near_rejected" or proj != "ortho") and (nf > 2 or comp not in ("near_rejected", "backface_culled"))]
V_REFUSED = {("opaque_partner", False), ("nan_transparent_pair", False), ("nan_transparent_pair", True)}      # (composition, z-buffer mode)


def _v_decide(comp, nf, first, proj, zbuffer, mut=None):
    v, f = FS.v_mesh(comp, nf, first, proj)
    scr, camz = FS.project(v["pos"], Camera(), proj, 64, 64)
    return decide(scr, camz, f, proj, True, zbuffer=zbuffer, mut=mut)


def test_nan_verdicts_by_the_three_restatements(oracle):
    """A NaN key panics only if its list has at least two members: oracle, model and `decide` give the same verdict for every
    composition, face count, position of the NaN face, projection and mode -- and it is the verdict the composition was built for."""
    refused = 0
    for comp, nf, first, proj, z in V_CASES:
        rc, px, zb, tm, d = FS.v_oracle(oracle, comp, nf, first, proj, z)
        want_refusal = (comp, z) in V_REFUSED
        assert (rc == abi.B32_E_NAN_KEY) == want_refusal and rc in (0, abi.B32_E_NAN_KEY), (comp, nf, first, proj, z, rc)
        try:
            order = _v_decide(comp, nf, first, proj, z)
            assert not want_refusal and order == [int(x) for x in d["draw_order"]], (comp, nf, first, proj, z)
        except NanKey:
            assert want_refusal, (comp, nf, first, proj, z)
        if nf == 65 and first:
            v, f = FS.v_mesh(comp, nf, first, proj)
            mpx = np.zeros(64 * 64 * 4, np.uint8); mpx.reshape(-1, 4)[:] = [FS.CLEAR.r, FS.CLEAR.g, FS.CLEAR.b, 255]
            mzb = np.full(64 * 64, np.finfo(f32).max, f32)
            try:
                with np.errstate(all="ignore"):
                    M.render_mesh_15(mpx, 64, 64, v, f, [], Camera(), FS.v_settings(proj, z), zbuffer=mzb)
                assert not want_refusal and np.array_equal(mpx, px) and np.array_equal(mzb.view(np.uint32), zb), (comp, proj, z)
            except FloatingPointError:
                assert want_refusal, (comp, proj, z)
        refused += want_refusal
        if want_refusal:
            assert (px.reshape(-1, 4) == [FS.CLEAR.r, FS.CLEAR.g, FS.CLEAR.b, 255]).all()
    assert 0 < refused < len(V_CASES)


# ------------------------------------------------------------------------------------------------ CPU: mutations
P3 = ("fixed", "float", "ortho")
MUTATIONS = {      # name: (sheets, fog, mode)
    "near_lt": (["N-fixed", "N-float", "Nrot-fixed", "Nrot-float"], None, {}),
    "near_all": (["N-fixed", "N-float", "Nrot-fixed", "Nrot-float"], None, {}),
    "area_lt": ([f"A-{p}" for p in P3], None, {}),
    "area_fma": (["A-float", "A-ortho"], None, {}),
    "fog_ge": ([f"F-{p}" for p in P3], "normal", {}),
    "fog_any": ([f"F-{p}" for p in P3], "normal", {}),
    "sum_before_swap": ([f"K-{p}" for p in P3], None, {}),
    "mul_third": ([f"K-{p}" for p in P3], None, {}),
    "no_plus5": (["K-fixed", "K-float"], None, {}),
    "painter_tie_earlier": ([f"K-{p}" for p in P3], None, {}),
    "neg_zero_less": (["K-ortho"], None, {}),
    "one_list": ([f"K-{p}" for p in P3], None, {}),
    "z_sorts_opaque": ([f"K-{p}" for p in P3], None, {"zbuffer": True}),
}
# cells changed, summed over the named sheets (z_tie_later: all-tie cells of the D and K sheets; nan_len1: V compositions whose verdict changes)
MEASURED_MUTATIONS = {"near_lt": 289, "near_all": 1260, "area_lt": 388, "area_fma": 61, "fog_ge": 48, "fog_any": 108, "sum_before_swap": 12, "mul_third": 12,
                      "no_plus5": 26, "painter_tie_earlier": 240, "neg_zero_less": 8, "one_list": 124, "z_sorts_opaque": 56, "z_tie_later": 130, "nan_len1": 72}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_changes_a_named_sheet(mut):
    sheets, fog_name, mode = MUTATIONS[mut]
    counts = {n: len(changed_cells(FS.sheet(n), mut, fog_name, **mode)) for n in sheets}
    print(f"mutation {mut}: {counts}, total {sum(counts.values())}")
    assert all(counts.values()), (mut, counts)
    assert sum(counts.values()) == MEASURED_MUTATIONS[mut], (mut, counts)


def _tie_cells(sh):
    """cells of two opaque faces with bit-equal depth triples on one triangle: every fragment ties"""
    scr, _ = sh.projected()
    out = []
    for c in range(len(sh.cell_tag)):
        fcs = [i for i in sh.cell_faces(c) if sh.meta[i].tag != "rejected"]
        if len(fcs) == 2 and all(sh.meta[i].alpha == 255 and sh.meta[i].blend == 0 for i in fcs):
            a, b = (scr[sh.faces["v"][i]].view(np.uint32).tolist() for i in fcs)
            if a == b:
                out.append((c, fcs))
    return out


def test_mutation_z_tie_later(oracle):
    """z-buffer mode, equal fragment depths keep the FIRST face (strict `<`, render.rs:1681).  Unlike the other fourteen this is no
    mutation of `decide`, which states no per-pixel rule: it is a check of the oracle's frame.  In every all-tie cell -- two opaque faces
    with bit-equal vertices -- the rule names the first face and "ties to the later face" names the other one; the frame shows the first
    alone, so each such cell is a cell the changed rule would change.  The count is that of these cells."""
    total = 0
    for name in [f"D-{p}" for p in P3] + [f"K-{p}" for p in P3]:
        sh = FS.sheet(name)
        idx = sh.decode(sh.oracle(oracle, None, zbuffer=True)["px"])
        cells = _tie_cells(sh)
        assert cells, name
        for c, (first, later) in cells:
            x0, y0, x1, y1 = sh.window(c)
            seen = set(int(v) for v in np.unique(idx[y0:y1, x0:x1]) if v >= 0)
            assert seen == {first} and first < later, sh.describe_cell(c)
        total += len(cells)
    print(f"mutation z_tie_later: {total} all-tie cells")
    assert total == MEASURED_MUTATIONS["z_tie_later"]


def test_mutation_nan_len1():
    """the NaN verdict taken at `list length >= 1` refuses the compositions in which the NaN face is alone in its list"""
    changed = 0
    for comp, nf, first, proj, z in V_CASES:
        def verdict(mut):
            try:
                _v_decide(comp, nf, first, proj, z, mut)
                return True
            except NanKey:
                return False
        changed += verdict(None) != verdict("nan_len1")
    print(f"mutation nan_len1: {changed} of {len(V_CASES)} V draws change their verdict")
    assert changed == MEASURED_MUTATIONS["nan_len1"] and changed > 0


# ------------------------------------------------------------------------------------------------ GPU
def _same(sh, got, want, what):
    msg = sh.first_difference(got, want, what)
    assert not msg, msg


def _check(ctx, sh, oracle, what, label, fog_name, mode, counting, fb, tm):
    o = sh.oracle(oracle, fog_name, **mode)
    tag = f"{what}, {label}, counting={counting}"
    _same(sh, fb.pixels, o["px"], tag)
    if mode.get("zbuffer"):
        _same(sh, fb.zbuffer.view(np.uint32), o["zb"], tag + ", depths")
    assert tm.triangles_drawn == o["tm"].triangles_drawn, tag
    order = ctx.last_draw_order(sh.n)
    assert np.array_equal(order, o["dump"]["draw_order"]), f"[{sh.name} {tag}] draw order differs from the oracle's"
    if counting and not mode.get("zbuffer"):
        assert tm.fragments == o["tm"].fragments, tag


@gpu
@pytest.mark.parametrize("name", FS.NAMES)
def test_sheet_drop_in_and_resident(gpu_ctx, oracle, name):
    """every mode of the sheet, fragment counting on and off, immediate and resident: pixels, z-buffer bits, triangles_drawn, draw order
    and (counting on, painter's mode) the store count are the oracle's"""
    sh = FS.sheet(name)
    try:
        for label, fog_name, mode in FS.modes(sh):
            for counting in (1, 0):
                gpu_ctx.set_fragment_counting(counting)
                for resident in (False, True):
                    fb, tm = FS.gpu_draw(gpu_ctx, sh, resident=resident, fog_name=fog_name, **mode)
                    _check(gpu_ctx, sh, oracle, f"resident={resident}", label, fog_name, mode, counting, fb, tm)
    finally:
        gpu_ctx.set_fragment_counting(1)


def expected_route(sh, mode, off, C):
    """which way the tile lists are made (plan_route, b32_frame.hip): orthographic and x-ray frames take the keyed pipeline"""
    if sh.proj == "ortho" or mode.get("xray") or off & C.ROUTE_SORT_FREE:
        return "keyed"
    if off & C.ROUTE_INLINE_BIN and off & C.ROUTE_DIRECT_BIN:
        return "counting_sort"
    return "direct_bin" if off & C.ROUTE_INLINE_BIN else "inline_bin"


@gpu
@pytest.mark.parametrize("name", FS.NAMES)
def test_sheet_on_every_binning_route(gpu_ctx, oracle, name):
    """in-fill list collection, k_setup's direct binning, the counting-sort launches and the keyed pipelines (ROUTE_SORT_FREE off), in
    painter's and z-buffer mode, counting off and on: the fill's packed priority and the sorted lists give the same cells, and the route
    counter of the intended route -- and of no other -- moves"""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    sh = FS.sheet(name)
    picked = [m for m in FS.modes(sh) if m[0] in ("painter", "zbuffer", "cull off", "fog normal", "fog normal zbuffer", "fog nan")]
    try:
        # (an orthographic frame takes the keyed pipeline whatever is switched off: one setting says all there is to say)
        for off in (0, C.ROUTE_INLINE_BIN, C.ROUTE_INLINE_BIN | C.ROUTE_DIRECT_BIN, C.ROUTE_SORT_FREE)[:1 if sh.proj == "ortho" else 4]:
            for label, fog_name, mode in picked:
                for counting in (0, 1):
                    gpu_ctx.set_fragment_counting(counting)
                    gpu_ctx.set_routes(off)
                    before = gpu_ctx.route_counts()
                    fb, tm = FS.gpu_draw(gpu_ctx, sh, resident=True, fog_name=fog_name, **mode)
                    after = gpu_ctx.route_counts()
                    _check(gpu_ctx, sh, oracle, f"routes off: {off}", label, fog_name, mode, counting, fb, tm)
                    moved = sorted(k for k in BIN_ROUTES if after[k] != before[k])
                    assert moved == [expected_route(sh, mode, off, C)], (name, label, off, counting, moved)
    finally:
        gpu_ctx.set_routes(0)
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", FS.NAMES)
def test_sheet_through_the_keyed_context(keyed_ctx, oracle, name):
    """a context of its own with the sort-free path off from the start: global painter's sort with counting on, per-tile sort with it off"""
    sh = FS.sheet(name)
    try:
        for label, fog_name, mode in FS.modes(sh):
            for counting in (1, 0):
                keyed_ctx.set_fragment_counting(counting)
                fb, tm = FS.gpu_draw(keyed_ctx, sh, resident=True, fog_name=fog_name, **mode)
                _check(keyed_ctx, sh, oracle, "keyed context", label, fog_name, mode, counting, fb, tm)
    finally:
        keyed_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", [f"{fam}-{p}" for fam in ("N", "A", "K") for p in P3])
def test_sheet_on_the_8bit_colour_path(gpu_ctx, oracle, name):
    """render_mesh: the transparent flag is computed but never partitions -- one list, one sort; K's expectation is the oracle's for that"""
    sh = FS.sheet(name)
    if sh.family == "K":
        assert not np.array_equal(sh.oracle(oracle, None, fmt8=True)["dump"]["draw_order"], sh.oracle(oracle)["dump"]["draw_order"])
    try:
        for label, fog_name, mode in MODES8:
            for counting in (1, 0):
                gpu_ctx.set_fragment_counting(counting)
                for resident in (False, True):
                    fb, tm = FS.gpu_draw(gpu_ctx, sh, resident=resident, **mode)
                    _check(gpu_ctx, sh, oracle, f"resident={resident}", label, None, mode, counting, fb, tm)
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("zbuffer", [False, True], ids=["painter", "zbuffer"])
@pytest.mark.parametrize("name", [f"{fam}-{p}" for fam in ("N", "A", "F") for p in P3])
def test_sheet_as_a_batched_frame(gpu_ctx, oracle, name, zbuffer):
    """frame_begin / frame_add / frame_end with two member meshes of the same cells: culling on without fog, then culling off with the
    NaN cull distance (never culls); equal to the oracle's two sequential calls on one framebuffer"""
    from bonnie32_amd import rasterizer as R
    sh = FS.sheet(name)
    st = sh.settings(zbuffer=zbuffer)
    members = [dict(backface_cull=True, fog=None), dict(backface_cull=False, fog=FS.fog("nan"))]
    ofb = oracle.Framebuffer(sh.width, sh.height); ofb.clear(FS.CLEAR)
    for p in members:
        s2 = copy.copy(st); s2.backface_cull = p["backface_cull"]
        rc, tm = oracle.render_mesh_15(ofb, sh.vertices, sh.faces, sh.textures, sh.camera, s2, p["fog"])
        assert rc == 0
    try:
        for counting in (1, 0):
            gpu_ctx.set_fragment_counting(counting)
            fb = R.Framebuffer(sh.width, sh.height, gpu_ctx)
            slots = [R.ResidentScene(fb, sh.vertices, sh.faces, sh.textures).detach() for _ in members]
            try:
                fb.clear(FS.CLEAR)
                gpu_ctx.frame_begin(sh.camera, st)
                for rs, p in zip(slots, members):
                    gpu_ctx.frame_add(rs, **p)
                gpu_ctx.frame_end()
                gpu_ctx.finish()
                _same(sh, fb.pixels, ofb.pixels, f"batched frame counting={counting}")
                if zbuffer:
                    _same(sh, fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32), f"batched frame depths counting={counting}")
            finally:
                for rs in slots:
                    rs.close()
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", ["K-fixed", "Nrot-float", "D-ortho"])
def test_sheet_in_two_ragged_row_bands(gpu_ctx, oracle, name):
    """bands (0, 37) and (37, H): the cut runs through a row of cells; the two partial frames assemble to the oracle's"""
    sh = FS.sheet(name)
    mode = {"zbuffer": True} if sh.family == "D" else {}
    o = sh.oracle(oracle, None, **mode)
    row = sh.width * 4
    try:
        for counting in (0, 1):
            gpu_ctx.set_fragment_counting(counting)
            assembled = np.zeros(sh.width * sh.height * 4, np.uint8)
            for y0, y1 in ((0, 37), (37, sh.height)):
                fb, tm = FS.gpu_draw(gpu_ctx, sh, resident=True, band=(y0, y1), **mode)
                assembled[y0 * row:y1 * row] = fb.pixels[y0 * row:y1 * row]
                assert tm.triangles_drawn == o["tm"].triangles_drawn
            _same(sh, assembled, o["px"], f"bands counting={counting}")
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("proj", P3)
def test_sheet_d_second_draw_onto_the_kept_zbuffer(gpu_ctx, oracle, proj):
    """the same geometry again with the colours of every cell swapped, onto the z-buffer the first draw left: every fragment ties with or
    loses against the stored depth"""
    first, second = FS.sheet(f"D-{proj}"), FS.sheet(f"D-{proj}-second")
    want, wantz = d_second_oracle(oracle, proj)
    try:
        for counting in (1, 0):
            gpu_ctx.set_fragment_counting(counting)
            for resident in (False, True):
                fb, _ = FS.gpu_draw(gpu_ctx, first, resident=resident, zbuffer=True)
                fb, _ = FS.gpu_draw(gpu_ctx, second, resident=resident, fb=fb, zbuffer=True)
                _same(first, fb.pixels, want, f"second draw counting={counting} resident={resident}")
                _same(first, fb.zbuffer.view(np.uint32), wantz, f"second draw depths counting={counting} resident={resident}")
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("proj", ["fixed", "float"])
def test_sheet_n_as_a_placed_draw(gpu_ctx, oracle, proj):
    """render_async(placement=...): local vertices whose camera depth has the bits of 0.1f and its neighbours only AFTER place_vertex
    (test_census_n_placed verifies that with Placement.apply and the model's dot3); the frame is the oracle's of the placed vertices"""
    from bonnie32_amd import rasterizer as R
    sh = FS.sheet(f"N-{proj}")
    local, pl = FS.placed_n(proj)
    placed = pl.apply(local)
    cz = FS.project(placed["pos"], sh.camera, proj, sh.width, sh.height)[1].reshape(sh.n, 3)
    st = sh.settings()
    ofb = oracle.Framebuffer(sh.width, sh.height); ofb.clear(FS.CLEAR)
    rc, otm, d = oracle.render_mesh_15(ofb, placed, sh.faces, [], sh.camera, st, dump=True)
    assert rc == 0 and otm.triangles_drawn == int(((cz > FS.NEAR).all(axis=1)).sum())
    try:
        for counting in (1, 0):
            gpu_ctx.set_fragment_counting(counting)
            fb = R.Framebuffer(sh.width, sh.height, gpu_ctx); fb.clear(FS.CLEAR)
            rs = R.ResidentScene(fb, local, sh.faces, [])
            rs.render_async(sh.camera, st, placement=pl)
            tm = rs.finish()
            _same(sh, fb.pixels, ofb.pixels, f"placed counting={counting}")
            assert tm.triangles_drawn == otm.triangles_drawn
            assert np.array_equal(gpu_ctx.last_draw_order(sh.n), d["draw_order"])
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("proj", P3)
def test_nan_verdicts_on_every_route(gpu_ctx, oracle, proj):
    """Family V on the three routes that carry their own copy of "a NaN key panics only if its list has at least two members": list
    collection in the fill (b32_fill.hip), the counting-sort binning (b32_bin.hip), the keyed / general sort (b32_sort.hip).  A refused
    draw returns B32_E_NAN_KEY and leaves the framebuffer byte-equal; an accepted one leaves the oracle's frame.  The route counter
    shows which route ran (orthographic frames always take the keyed one)."""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    routes = ((0, "inline_bin"), (C.ROUTE_INLINE_BIN | C.ROUTE_DIRECT_BIN, "counting_sort"), (C.ROUTE_SORT_FREE, "keyed"))
    seen = {r: 0 for _, r in routes}
    try:
        for off, route in routes:
            gpu_ctx.set_routes(off)
            for comp, nf, first, p, z in V_CASES:
                if p != proj:
                    continue
                rc, px, zb, otm, d = FS.v_oracle(oracle, comp, nf, first, proj, z)
                v, f = FS.v_mesh(comp, nf, first, proj)
                fb = R.Framebuffer(64, 64, gpu_ctx); fb.clear(FS.CLEAR)
                before_px = fb.pixels
                before = gpu_ctx.route_counts()
                what = (comp, nf, first, proj, z, route)
                if rc:
                    with pytest.raises(R.B32Error) as e:
                        R.ResidentScene(fb, v, f, []).render(Camera(), FS.v_settings(proj, z))
                    assert e.value.code == abi.B32_E_NAN_KEY, what
                    assert np.array_equal(fb.pixels, before_px), what
                else:
                    tm = R.ResidentScene(fb, v, f, []).render(Camera(), FS.v_settings(proj, z))
                    assert np.array_equal(fb.pixels, px), what
                    if z:
                        assert np.array_equal(fb.zbuffer.view(np.uint32), zb), what
                    assert tm.triangles_drawn == otm.triangles_drawn, what
                    assert np.array_equal(gpu_ctx.last_draw_order(nf), d["draw_order"]), what
                after = gpu_ctx.route_counts()
                moved = sorted(k for k in BIN_ROUTES if after[k] != before[k])
                assert moved == ["keyed" if proj == "ortho" else route], (what, moved)
                seen[moved[0]] += 1
        assert seen["keyed"] and (proj == "ortho" or (seen["inline_bin"] and seen["counting_sort"]))
    finally:
        gpu_ctx.set_routes(0)
