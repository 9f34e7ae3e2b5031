"""The wireframe phases edge by edge: which occurrence supplies the depths, the strict depth test, Bresenham's ties, `as i32`, the faces
that count, the thresholds of the tile route (tests/wire_sheets.py builds the sheets).

CPU tests (no mark): three restatements agree on every sheet and mode -- the C oracle, oracle/np_model.py, and `wire_phases` below, a
literal restatement of render.rs:2574-2635 with draw_line_3d (render.rs:757-817) and draw_line (render.rs:716-750): the quadratic `any`
scan and the `err` loop, written from the reference text.  (Edges longer than 2^16 pixels, sheet T-walk only, are walked over their
visible steps alone: the literal loop would spin through 2^24 off-screen pixels in Python.)  A census per family finds every case by its
bits in the projection; every one-point mutation of `wire_phases` changes a named sheet by a stated number of pixels.
GPU tests: every sheet drop-in and resident, on the tile route and with B32_ROUTE_WIRE_TILES off, twice per context, through the
8-bit-colour path, placed, as a batched frame, in ragged bands.

The refusal rule has two limits, and sheet T-refuse sits on both.  Every extent of 2^30 and more is refused (flat: 2^30 - 1 drawn, 2^30
refused).  Below that a line is refused when the reference's `2 * err` leaves i32, which with minor steps happens from an extent of
2^31 / 3 on (one minor step: 715 827 883 drawn, 715 827 884 refused); oracle, model and kernel state that rule alike
(np_model.edge_overflows), and it is checked against the literal loop in short words.

Measured once: the 27 GPU tests take 2.5 s on an MI355X, the 44 CPU tests 17 s."""
import math

import numpy as np
import pytest

from bonnie32_amd import abi
from oracle import np_model as M
from tests import frontend_sheets as FS
from tests import wire_sheets as WS

gpu = pytest.mark.gpu
f32 = np.float32
NEAR = float(FS.NEAR)


# ------------------------------------------------------------------------------------------------ the phases, restated
def _as_i32(x, mut):
    x = float(x)
    if x != x:
        return 0
    t = math.floor(x) if mut == "floor_i32" else math.trunc(x)
    return max(-2147483648, min(2147483647, t))


def _unique(tris, mut, taken=()):
    """render.rs:2578-2598: the edges of the listed triangles as (x0, y0, z0, x1, y1, z1), direction-normalised, first occurrence kept"""
    unique = []
    for v1, v2, v3 in tris:
        for a, b in ((v1, v2), (v2, v3), (v3, v1)):
            x0, y0, z0, x1, y1, z1 = _as_i32(a[0], mut), _as_i32(a[1], mut), f32(a[2]), _as_i32(b[0], mut), _as_i32(b[1], mut), f32(b[2])
            if mut == "no_normalise" or (x0, y0) < (x1, y1):
                edge = (x0, y0, z0, x1, y1, z1)
            elif mut == "depths_not_swapped":
                edge = (x1, y1, z0, x0, y0, z1)
            else:
                edge = (x1, y1, z1, x0, y0, z0)
            hit = [i for i, e in enumerate(unique) if e[0] == edge[0] and e[1] == edge[1] and e[3] == edge[3] and e[4] == edge[4]]
            if any(e[0] == edge[0] and e[1] == edge[1] and e[3] == edge[3] and e[4] == edge[4] for e in taken):
                continue
            if not hit:
                unique.append(edge)
            elif mut == "last_occurrence":
                unique[hit[0]] = edge
    return unique


def _visible_steps(x0, y0, x1, y1, w, h):
    """a long line's steps inside the frame, by the closed form of np_model.line_points on the major axis (T-walk's edges only)"""
    adx, ady = abs(x1 - x0), abs(y1 - y0)
    xmajor = adx >= ady
    n, m0, sm, size = (adx, x0, 1 if x0 < x1 else -1, w) if xmajor else (ady, y0, 1 if y0 < y1 else -1, h)
    k_lo, k_hi = ((0 - m0), (size - 1 - m0)) if sm > 0 else ((m0 - size + 1), m0)
    k = np.arange(max(k_lo, 0), min(k_hi, n) + 1, dtype=np.int64)
    dmin, n0, sn = (ady, y0, 1 if y0 < y1 else -1) if xmajor else (adx, x0, 1 if x0 < x1 else -1)
    minor = n0 + sn * ((2 * dmin * k + n) // (2 * n))
    major = m0 + sm * k
    xs, ys = (major, minor) if xmajor else (minor, major)
    on = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    return [(int(a), int(b), int(c)) for a, b, c in zip(xs[on], ys[on], k[on])]


def _depth(z0, z1, step, total, mut):
    with np.errstate(all="ignore"):
        t = f32(step) / f32(total)
        if mut == "fused":                       # fl(z0 + t * dz): the product exact in f64 (two 24-bit factors)
            return f32(np.float64(z0) + np.float64(t) * np.float64(f32(z1 - z0)))
        return f32(z0 + f32(t * f32(z1 - z0)))


def _draw_line(img, zb, w, h, e, rgb, depth_test, mut):
    """draw_line_3d_impl (render.rs:768-817) / draw_line_blended (render.rs:720-752) with their `err` loop"""
    x0, y0, z0, x1, y1, z1 = e
    dx, dy = abs(x1 - x0), -abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    total = max(dx, max(-dy, 1)) if mut != "no_max1" else max(dx, -dy)

    def plot(x, y, step):
        if depth_test:
            z = _depth(z0, z1, step, total, mut)
            cur = zb[y, x]
            if not (z <= cur if mut == "le" else z < cur):
                return
        img[y, x] = (rgb[0], rgb[1], rgb[2], 255)
    if max(dx, -dy) > 1 << 16:
        for x, y, k in _visible_steps(x0, y0, x1, y1, w, h):
            plot(x, y, f32(k) if mut == "no_saturate" else f32(min(k, 1 << 24)))
        return
    err, x, y = dx + dy, x0, y0
    step, count = f32(0.0), 0
    xmajor = dx >= -dy
    while True:
        if 0 <= x < w and 0 <= y < h:
            plot(x, y, f32(count) if mut == "no_saturate" else step)
        if x == x1 and y == y1:
            break
        e2 = 2 * err
        stepped = False
        if (e2 > dy) if (mut == "half_down" and not xmajor) else (e2 >= dy):
            err += dy; x += sx; step = f32(step + f32(1.0)); stepped = True
        if (e2 < dx) if (mut == "half_down" and xmajor) else (e2 <= dx):
            err += dx; y += sy
            if not stepped:
                step = f32(step + f32(1.0))
        count += 1


def _refused(e, mut):
    """the rule oracle and device share: an extent of 2^30 or more, or a `2 * err` that leaves i32 (np_model.edge_overflows)"""
    x0, y0, _, x1, y1, _ = e
    if mut == "refuse_gt" and max(abs(x1 - x0), abs(y1 - y0)) == 1 << 30:
        return False
    return M.edge_overflows(x0, y0, x1, y1)


def wire_phases(sh, img, zb, mode, mut=None):
    """The wireframe phases of render_mesh_15 (render.rs:2574-2635) over a frame that holds the fill's result, from the projected
    vertices: which faces enter the two lists (render.rs:2381-2453, 2509-2511), the unique edges, the two line loops.  `mut` names a
    one-point change (MUTATIONS)."""
    scr, camz = sh.projected()
    cull, xray, overlay = mode.get("cull", True), mode.get("xray", False), mode.get("overlay", False)
    fg = sh.fog(mode)
    back_wires, front_wires = [], []
    for fi in range(sh.n):
        ids = [int(k) for k in sh.faces["v"][fi]]
        cz = [float(camz[i]) for i in ids]
        kept = sh.proj == "ortho" or not any(z <= NEAR for z in cz)
        v1, v2, v3 = (scr[i] for i in ids)
        with np.errstate(all="ignore"):
            area = (v2[0] - v1[0]) * (v3[1] - v1[1]) - (v3[0] - v1[0]) * (v2[1] - v1[1])
        back = bool(area < 0) if mut == "zero_area_front" else bool(area <= 0)
        if kept and fg is not None and all(z > float(f32(fg[2])) for z in cz):
            kept = False
        if mut == "rejected_claims":
            if back:
                back_wires.append((v1, v2, v3))
            elif kept and overlay:
                front_wires.append((v1, v2, v3))
            continue
        if not kept:
            continue
        if back and not xray:
            back_wires.append((v1, v2, v3))
        if not back and overlay:
            front_wires.append((v1, v2, v3))
    w, h = sh.width, sh.height
    back_edges = _unique(back_wires, mut) if cull and mode.get("wire", True) else []
    front_edges = _unique(front_wires, mut, taken=back_edges if mut == "joint_dedupe" else ()) if overlay and front_wires else []
    phases = [(back_edges, WS.COL_BACK, True), (front_edges, WS.COL_FRONT, False)]
    for edges, rgb, depth_test in (phases[::-1] if mut == "back_after_overlay" else phases):
        for e in edges:
            if _refused(e, mut):
                return abi.B32_E_UNSUPPORTED
            _draw_line(img, zb, w, h, e, rgb, depth_test, mut)
    return 0


def restated(sh, oracle, mode, mut=None, with_rc=False):
    """the frame `wire_phases` arrives at, over the oracle's frame of the same draw without the wireframe phases"""
    base = dict(mode); base["wire"] = False
    if mode.get("overlay"):                     # (render.rs:2550: the overlay replaces the fill; what is left of the frame is the clear)
        img = np.zeros((sh.height, sh.width, 4), np.uint8); img[:] = (FS.CLEAR.r, FS.CLEAR.g, FS.CLEAR.b, 255)
        zb = np.full((sh.height, sh.width), np.finfo(f32).max, f32)
    else:
        o = sh.oracle(oracle, **base)
        img, zb = o["px"].copy(), o["zb"].view(np.float32).copy()
    rc = wire_phases(sh, img, zb, mode, mut)
    return (rc, img) if with_rc else img


def changed(sh, oracle, mode, mut):
    return int((restated(sh, oracle, mode) != restated(sh, oracle, mode, mut)).any(axis=2).sum())


def all_modes(sh):
    return WS.modes(sh) + [("8-bit", {"fmt8": True})]


# ------------------------------------------------------------------------------------------------ CPU: three restatements agree
@pytest.mark.parametrize("name", WS.NAMES)
def test_three_restatements_agree(oracle, name):
    sh = WS.sheet(name)
    for label, mode in all_modes(sh):
        o = sh.oracle(oracle, **mode)
        assert o["rc"] == 0, (name, label)
        msg = sh.first_difference(restated(sh, oracle, mode), o["px"], f"wire_phases, {label}")
        assert not msg, msg
        px = np.zeros(sh.width * sh.height * 4, np.uint8); px.reshape(-1, 4)[:] = [FS.CLEAR.r, FS.CLEAR.g, FS.CLEAR.b, 255]
        zb = np.full(sh.width * sh.height, np.finfo(f32).max, f32)
        with np.errstate(all="ignore"):
            if mode.get("fmt8"):
                r = M.render_mesh(px, sh.width, sh.height, sh.vertices, sh.faces, [], sh.camera, sh.settings(**mode), zbuffer=zb)
            else:
                r = M.render_mesh_15(px, sh.width, sh.height, sh.vertices, sh.faces, [], sh.camera, sh.settings(**mode), sh.fog(mode), zbuffer=zb)
        msg = sh.first_difference(px, o["px"], f"model, {label}")
        assert not msg, msg
        assert np.array_equal(zb.view(np.uint32).reshape(sh.height, sh.width), o["zb"]), (name, label)
        assert r["triangles_drawn"] == o["tm"].triangles_drawn, (name, label)
        if not mode.get("overlay"):             # lines never write depth: the z-buffer is the one the draw without the wireframe phases leaves
            assert np.array_equal(o["zb"], sh.oracle(oracle, **dict(mode, wire=False))["zb"]), (name, label)


# ------------------------------------------------------------------------------------------------ CPU: census
def _drawn(o, rgb=WS.COL_BACK):
    return (o["px"][..., :3] == rgb).all(axis=2)


@pytest.mark.parametrize("proj", ["fixed", "float"])
def test_census_l(oracle, proj):
    """all 225 vectors in both directions, found in the projection; the A->B and B->A cells plot the same set (read from the oracle's
    frame, relative to the cell's centre); the half-step ties are counted; the centres stand on tile boundaries; float projection: the
    fractional and negative fractional coordinates are there by their bits and truncate toward zero"""
    sh = WS.sheet("L-" + proj)
    assert sh.width % 64 and sh.height % 16
    e = sh.edges_i32()
    img = _drawn(sh.oracle(oracle))
    seen, ties, on64, on16 = set(), 0, 0, 0
    sets = {}
    for c in sh.cells:
        if "vec" not in c:
            continue
        fi = c["faces"][0]
        pts = {tuple(int(t) for t in p) for p in e[fi]}
        cx, cy = c["at"]
        assert (cx, cy) in pts
        other = (pts - {(cx, cy)} or {(cx, cy)}).pop()
        assert (other[0] - cx, other[1] - cy) == c["vec"], c["tag"]
        seen.add((c["vec"], c["rev"]))
        ys, xs = np.nonzero(img[cy - 8:cy + 8, cx - 8:cx + 8])
        sets[(c["vec"], c["rev"])] = {(int(x) - 8, int(y) - 8) for x, y in zip(xs, ys)}
        dmaj, dmin = max(abs(c["vec"][0]), abs(c["vec"][1])), min(abs(c["vec"][0]), abs(c["vec"][1]))
        if not c["rev"] and dmaj and dmaj % 2 == 0:
            ties += sum((2 * dmin * k + dmaj) % (2 * dmaj) == 0 for k in range(dmaj + 1))
        on64 += cx % 64 == 0; on16 += cy % 16 == 0
    assert len(seen) == 450
    for vec in WS.L_VECTORS:
        assert sets[(vec, False)] == sets[(vec, True)] and len(sets[(vec, False)]) == max(abs(vec[0]), abs(vec[1])) + 1, vec
    print(f"L-{proj}: half-step ties {ties}, centres on a 64-column boundary {on64}, on a 16-row boundary {on16}")
    assert ties == 80 and on64 >= 100 and on16 == 450
    borders = {c["border"] for c in sh.cells if "border" in c}
    assert {b[0] for b in WS.L_BORDER} <= borders
    if proj == "float":
        scr, _ = sh.projected()
        x, y = scr[:, 0], scr[:, 1]
        for lo, hi, want in ((-1.0, -0.8, 0), (-1.6, -1.4, -1), (10.9, 11.0, 10), (-7.0, -6.9, -6), (-7.1, -7.0, -7)):
            hit = [float(t) for t in np.concatenate([x, y]) if lo < t < hi]
            assert hit and all(M._as_i32(t) == want for t in hit), (lo, hi)
        assert ((x % 1 != 0) & (x > 30)).sum() > 900          # the cells' own vertices are fractional too


def _occurrence_edges(sh):
    """per cell of sheet O: the pixels of the edge A-B that belong to no other edge of the cell"""
    e = sh.edges_i32()
    out = []
    for c in sh.cells:
        a = (c["at"][0] + WS.O_POINTS["A"][0] + c["shift"], c["at"][1] + WS.O_POINTS["A"][1])
        b = (c["at"][0] + WS.O_POINTS["B"][0] + c["shift"], c["at"][1] + WS.O_POINTS["B"][1])
        for fi in c["occ"]:
            pts = [tuple(int(t) for t in p) for p in e[fi]]
            assert a in pts and b in pts, (c["tag"], pts)
        xs, ys, _ = M.line_points(a[0], a[1], b[0], b[1])
        out.append([(int(x), int(y)) for x, y in zip(xs[2:-2], ys[2:-2])])
    return out


O_DIFFERS = {"ends": 2, "pair": 140, "triple": 5, "near": 5, "fog": 4}      # (of 2, 140, 15, 10 and 9 cells: measured from `wire_phases`, asserted)


def test_census_o(oracle):
    """every cell's occurrences carry the edge A-B by their projected integers; a hidden first occurrence leaves the edge's interior
    undrawn, a visible one draws it, whatever follows; faces 0, 1, nf-2 and nf-1 carry two of the edges; the mesh has more than 1024
    faces; with culling off no back edge is drawn; in x-ray mode none either; with the overlay on the shared edge has the overlay's colour"""
    sh = WS.sheet("O")
    assert sh.n > 1024
    inner = _occurrence_edges(sh)
    z = _drawn(sh.oracle(oracle))
    kinds = {}
    for c, px in zip(sh.cells, inner):
        got = [bool(z[y, x]) for x, y in px]
        first = c["tag"]
        if c["kind"] in ("pair", "ends"):
            want = "visible first" in first
        elif c["kind"] == "triple":
            want = first.split("(")[1].startswith(str(WS.O_NEAR))
        elif c["kind"] in ("near", "fog"):
            want = first.endswith(str(WS.O_NEAR))            # the rejected face does not own the edge: its successor does
        else:
            want = True
        assert all(g == want for g in got), (c["tag"], got)
        kinds[c["kind"]] = kinds.get(c["kind"], 0) + 1
    assert set(kinds) == {"pair", "triple", "ends", "near", "fog", "overlay"} and sh.cells[0]["occ"][0] == 0 and sh.cells[1]["occ"][-1] == sh.n - 1
    print("O cells by kind:", kinds)
    # edges whose drawn set differs between "first" and "last occurrence wins", per kind; a near-rejected or fog-culled first occurrence
    # is not in the list at all (one occurrence is left: first = last), so there the count is of "the rejected face claims the edge"
    base = restated(sh, oracle, {})
    differs = {}
    for mut, which in (("last_occurrence", ("pair", "triple", "ends")), ("rejected_claims", ("near", "fog"))):
        other = (restated(sh, oracle, {}, mut) != base).any(axis=2)
        for c, px in zip(sh.cells, inner):
            if c["kind"] in which:
                differs[c["kind"]] = differs.get(c["kind"], 0) + any(bool(other[y, x]) for x, y in px)
    print("O edges whose drawn set depends on the occurrence, by kind:", differs)
    assert differs == O_DIFFERS, differs
    assert not _drawn(sh.oracle(oracle, cull=False)).any() and not _drawn(sh.oracle(oracle, xray=True)).any()
    ov = sh.oracle(oracle, overlay=True)
    for c, px in zip(sh.cells, inner):
        if c["kind"] == "overlay":
            assert all(tuple(ov["px"][y, x, :3]) == WS.COL_FRONT for x, y in px), c["tag"]
    assert _drawn(ov).any()


def test_census_z(oracle):
    """by the stored bits of the oracle's z-buffer: pixels of a line exactly at the stored depth (never drawn), one ulp below (drawn), one
    ulp above (not); crossing lines are part drawn; the fused form changes a verdict in both directions (exact rational arithmetic)"""
    from fractions import Fraction
    sh = WS.sheet("Z")
    o = sh.oracle(oracle)
    zb = o["zb"]; zbf = zb.view(np.float32); drawn = _drawn(o)
    scr, _ = sh.projected()
    e32 = sh.edges_i32()
    count = {k: 0 for k in ("at", "below", "above", "cross", "cross-reversed", "fused-a", "fused-b", "point-at", "point-below", "point-above")}
    for c in sh.cells:
        fi = c["faces"][0]
        vz = [f32(scr[int(i)][2]) for i in sh.faces["v"][fi]]
        (x0, y0), (x1, y1) = c["lo"], c["hi"]
        xs, ys, ks = M.line_points(x0, y0, x1, y1)
        kind = c["kind"]
        if kind.split("-")[-1] in ("at", "below", "above"):
            d = {"at": 0, "below": -1, "above": 1}[kind.split("-")[-1]]
            hit = [(x, y) for x, y in zip(xs, ys) if int(zb[y, x]) + d == FS.bits(vz[0])]
            assert hit and all(bool(drawn[y, x]) == (d < 0) for x, y in hit), c["tag"]
            count[kind] += len(hit)
        elif kind.startswith("cross"):
            got = [bool(drawn[y, x]) for x, y in zip(xs, ys)]
            assert got[0] and not got[-1], (c["tag"], got)
            count[kind] += 1
        else:
            n = max(abs(x1 - x0), abs(y1 - y0))
            pts = [tuple(int(t) for t in p) for p in e32[fi]]
            z_lo = next(v for v, p in zip(vz, pts) if p == (x0, y0)); z_hi = next(v for v, p in zip(vz, pts) if p == (x1, y1))
            dz = f32(z_hi - z_lo)
            differ = 0
            for x, y, k in zip(xs, ys, ks):
                t = f32(k) / f32(n)
                unf = FS.rne32(Fraction(float(z_lo)) + Fraction(float(FS.rne32(Fraction(float(t)) * Fraction(float(dz))))))
                fus = FS.rne32(Fraction(float(z_lo)) + Fraction(float(t)) * Fraction(float(dz)))
                cur = zbf[y, x]
                if (unf < cur) != (fus < cur):
                    differ += 1
                    assert bool(unf < cur) == (kind == "fused-a") and bool(drawn[y, x]) == bool(unf < cur), c["tag"]
            assert differ, c["tag"]
            count[kind] += differ
    print("Z census (pixels, or cells for the crossing lines):", count)
    assert all(count.values()), count


def test_census_z_ortho(oracle):
    """by their bits: FLT_MAX does not pass the cleared z-buffer (strict `<`), its lower neighbour does; -FLT_MAX to FLT_MAX has an
    infinite difference: after the first step z is +inf (undrawn) or, from the other end, -inf (drawn)"""
    sh = WS.sheet("Z-ortho")
    scr, _ = sh.projected()
    drawn = _drawn(sh.oracle(oracle))
    seen, overflow = set(), set()
    for c in sh.cells:
        (x0, y0), (x1, y1) = c["lo"], c["hi"]
        xs, ys, _ = M.line_points(x0, y0, x1, y1)
        got = [bool(drawn[y, x]) for x, y in zip(xs, ys)]
        vz = {FS.bits(scr[int(i)][2]) for i in sh.faces["v"][c["faces"][0]]}
        case = c["case"]; seen.add(case)
        if case == "FLT_MAX" and not c["floor"]:
            assert vz == {0x7F7FFFFF} and not any(got)
        if case == "below FLT_MAX" and not c["floor"]:
            assert vz == {0x7F7FFFFE} and all(got)
        if case in ("-FLT_MAX to FLT_MAX", "FLT_MAX to -FLT_MAX"):      # (the end points also carry the face's point edge B-B: the interior decides)
            assert vz == {0x7F7FFFFF, 0xFF7FFFFF} and len(set(got[1:-1])) == 1, (case, got)
            overflow.add(got[1])
        if case == "negative" and c["floor"]:
            assert any(got)
    assert seen == {t[0] for t in WS.ZO_CASES} and overflow == {True, False}      # z = +inf (undrawn) and z = -inf (drawn) after the first step


def _tiles(sh, p, q):
    """tiles of the box of the edge p-q clipped to the frame (64 x 16 tiles)"""
    x0, x1 = max(min(p[0], q[0]), 0), min(max(p[0], q[0]), sh.width - 1)
    y0, y1 = max(min(p[1], q[1]), 0), min(max(p[1], q[1]), sh.height - 1)
    return (x1 // 64 - x0 // 64 + 1, y1 // 16 - y0 // 16 + 1) if x0 <= x1 and y0 <= y1 else (0, 0)


def _segments(sh):
    """segments of 16 steps inside the one tile of a 64 x 16 sheet, summed over the distinct back edges (np_model.line_points, clipped)"""
    e = sh.edges_i32()
    scr, _ = sh.projected()
    seen, total = set(), 0
    for fi in range(sh.n):
        if sh.tags[fi].startswith("floor"):
            continue
        for j in range(3):
            p, q = tuple(int(t) for t in e[fi][j]), tuple(int(t) for t in e[fi][(j + 1) % 3])
            key = (min(p, q), max(p, q))
            if key in seen:
                continue
            seen.add(key)
            xs, ys, _ = M.line_points(*key[0], *key[1])
            inside = int(((xs >= 0) & (xs < 64) & (ys >= 0) & (ys < 16)).sum())
            total += -(-inside // 16)
    return total, len(seen)


def test_census_t():
    """the thresholds by the projected integers: boxes of 64 and 65 tiles; union boxes of 128, 144 and 256 tiles around two small boxes and
    a big third edge; lists of 256 and 257 faces with 768 and 771 distinct edges; 1536, 1537 and 2288 segments; extents of 2^14 - 1 and
    2^14, starts beyond +-2^20, an extent above 2^24 whose visible steps are all above 2^24; chains of three equal hashes modulo 1024"""
    sh = WS.sheet("T-box"); e = sh.edges_i32()
    boxes = {c["tag"]: _tiles(sh, *[tuple(int(t) for t in p) for p in (e[c["faces"][0]][0], e[c["faces"][0]][1])]) for c in sh.cells if "box" in c}
    assert boxes["T box 64 tiles"] == (4, 16) and boxes["T box 65 tiles"] == (5, 13) and boxes["T front 65 tiles"] == (5, 13), boxes
    sh = WS.sheet("T-union"); e = sh.edges_i32()
    for c in sh.cells:
        tri = [tuple(int(t) for t in p) for p in e[c["faces"][0]]]
        bx = sorted((_tiles(sh, tri[j], tri[(j + 1) % 3]) for j in range(3)), key=lambda b: b[0] * b[1])
        assert bx[0][0] * bx[0][1] <= 16 and bx[1][0] * bx[1][1] <= 16 and bx[2][0] * bx[2][1] > 64, (c["tag"], bx)
        assert max(b[0] for b in bx[:2]) * max(b[1] for b in bx[:2]) == c["union"], (c["tag"], bx)
    assert {c["union"] for c in sh.cells} == {128, 144, 256} and {c["winding"] for c in sh.cells} == {"back", "front"}
    for name, faces, edges in (("T-cap-256", 256, 768), ("T-cap-257", 257, 771)):
        sh = WS.sheet(name)
        segs, distinct = _segments(sh)
        assert sh.n - 2 == faces and distinct == edges, (name, sh.n, distinct)
        e = sh.edges_i32()[2:]                           # (without the floor) all in the one tile
        assert e.min() >= 0 and e[..., 0].max() < 64 and e[..., 1].max() < 16
    got = {name: _segments(WS.sheet(name))[0] for name in ("T-seg-1536", "T-seg-1537", "T-seg-max")}
    print("segments in the one tile:", got)
    assert got == {"T-seg-1536": 1536, "T-seg-1537": 1537, "T-seg-max": 2288}, got      # (2304 less the third edges that repeat or have no step inside)
    sh = WS.sheet("T-walk"); e = sh.edges_i32()
    ext = {}
    for c in sh.cells:
        pts = {tuple(int(t) for t in p) for p in e[c["faces"][0]]}
        p, q = min(pts), max(pts)
        ext[c["case"]] = (max(abs(q[0] - p[0]), abs(q[1] - p[1])), p, q)
    print("T-walk reached:", ext)
    assert ext["extent 16383"][0] == 16383 and ext["extent 16384"][0] == 16384 and ext["extent 20000"][0] == 20000
    assert ext["start beyond -2^20"][1][0] < -(1 << 20) and ext["start beyond -2^20 in y"][0] > 1 << 20 and ext["end beyond +2^20"][2][0] > 1 << 20
    ex, p, q = ext["saturated"]
    assert ex > 1 << 24 and -p[0] > 1 << 24 and q[0] >= 0
    sh = WS.sheet("T-hash")
    chains = [c for c in sh.cells if "chain" in c]
    assert len(chains) == 18 and sh.n * 6 <= 1024
    e = sh.edges_i32()
    for c in chains:
        hs = set()
        for fi in c["faces"][:3]:
            pts = sorted({tuple(int(t) for t in p) for p in e[fi]})
            hs.add(WS.edge_hash(*pts[0], *pts[1]) & 1023)
        assert len(hs) == 1 and len({tuple(x) for x in c["chain"]}) == 3, c


# ------------------------------------------------------------------------------------------------ CPU: the refusal rule
def _literal_overflow(dx, dy, word):
    """render.rs:720-750 with Python integers: does `2 * err` or `err` leave a signed word of that many bits before the loop ends?"""
    lim = 1 << (word - 1)
    a, b = dx, -dy
    err, x, y = a + b, 0, 0
    while not (x == dx and y == dy):
        e2 = 2 * err
        if not -lim <= e2 < lim:
            return True
        if e2 >= b:
            err += b; x += 1
        if e2 <= a:
            err += a; y += 1
        if not -lim <= err < lim:
            return True
    return False


def test_overflow_rule_equals_the_literal_loop_in_a_short_word(oracle):
    """np_model.edge_overflows below its flat limit of 2^(word-2) against the literal loop in words of 8 bits (every line) and 10 bits
    (extents of 150 to 255, where the rule bites); the C oracle's form against the model's on 20 000 random 32-bit lines, and at the
    extents found by sheet T-refuse: 700 000 000 with one minor step is drawn, 720 000 000 is not (its literal loop never ends)"""
    for word, extents in ((8, range(64)), (10, range(150, 256))):
        for dx in extents:
            for dy in extents:
                assert M.edge_overflows(0, 0, dx, dy, word=word) == _literal_overflow(dx, dy, word), (word, dx, dy)
    L = oracle.lib()
    rng = np.random.default_rng(30)
    for _ in range(20000):
        dx = int(rng.integers(0, 1 << 30)); dy = int(rng.integers(0, dx + 1))
        if rng.integers(2):
            dx, dy = dy, dx
        assert bool(L.b32o_wire_edge_overflows(5, -7, 5 + dx, -7 - dy)) == M.edge_overflows(5, -7, 5 + dx, -7 - dy), (dx, dy)
    assert not M.edge_overflows(0, 0, 700_000_000, 1) and M.edge_overflows(0, 0, 720_000_000, 1)
    assert not M.edge_overflows(0, 0, 715_827_883, 1) and M.edge_overflows(0, 0, 715_827_884, 1)
    assert M.edge_overflows(0, 0, 1 << 30, 1 << 30) and not M.edge_overflows(0, 0, (1 << 30) - 1, 0)


@pytest.mark.parametrize("case", list(WS.REFUSE_CASES))
def test_refusal_rule(oracle, case):
    """the extents are the projection's (census); the C oracle -- the only reference here: np_model.line_points allocates per step --
    refuses exactly the refused cases with B32_E_UNSUPPORTED and draws the others with its literal loop (about a second each);
    `wire_phases` agrees in the verdict and, walking the visible steps alone, in the frame"""
    ax, bx, minor, refused = WS.REFUSE_CASES[case]
    sh = WS.sheet("T-refuse-" + case)
    pts = sorted({tuple(int(t) for t in p) for p in sh.edges_i32()[-1]})
    assert pts == [(ax, 8), (bx, 8 + minor)], pts
    print(f"T-refuse-{case}: reached extent {bx - ax}, minor extent {minor}")
    o = sh.oracle(oracle)
    assert o["rc"] == (abi.B32_E_UNSUPPORTED if refused else 0)
    rc, img = restated(sh, oracle, {}, with_rc=True)
    assert rc == o["rc"]
    if not refused:
        msg = sh.first_difference(img, o["px"], "wire_phases")
        assert not msg, msg
        assert _drawn(o).sum() == bx + 1


def test_mutation_refusal_at_gt(oracle):
    """mutation 14, refusal at `> 2^30` instead of `>=`: the stated change is the return code of sheet T-refuse-flat-2^30, -5 -> 0"""
    sh = WS.sheet("T-refuse-flat-2^30")
    assert restated(sh, oracle, {}, with_rc=True)[0] == abi.B32_E_UNSUPPORTED == -5
    assert restated(sh, oracle, {}, "refuse_gt", with_rc=True)[0] == 0


# ------------------------------------------------------------------------------------------------ CPU: a second draw onto kept depths
def second_draw_oracle(O):
    """(pixels, z-buffer bits) after sheet O and then sheet Z on one framebuffer, z-buffer mode, no clear in between"""
    fb = O.Framebuffer(WS.Z_W, WS.Z_H)
    fb.clear(FS.CLEAR)
    for sh in (WS.sheet("O"), WS.sheet("Z")):
        assert O.render_mesh_15(fb, sh.vertices, sh.faces, [], sh.camera, sh.settings(), sh.fog({}))[0] == 0
    return fb.image().copy(), fb.zbuffer.view(np.uint32).reshape(WS.Z_H, WS.Z_W).copy()


def test_second_draw_tests_lines_against_the_kept_depths(oracle):
    """sheet Z drawn onto what sheet O left: Z's floors (depths of 10 and more) lose against or tie with O's at 10, so Z's lines -- chosen
    against Z's own floors -- are tested against the kept depth 10: the oracle and the model agree, and the number of Z's line pixels whose
    verdict differs from sheet Z on a cleared framebuffer is stated"""
    px, zb = second_draw_oracle(oracle)
    mpx = np.zeros(WS.Z_W * WS.Z_H * 4, np.uint8); mpx.reshape(-1, 4)[:] = [FS.CLEAR.r, FS.CLEAR.g, FS.CLEAR.b, 255]
    mzb = np.full(WS.Z_W * WS.Z_H, np.finfo(f32).max, f32)
    for sh in (WS.sheet("O"), WS.sheet("Z")):
        with np.errstate(all="ignore"):
            M.render_mesh_15(mpx, sh.width, sh.height, sh.vertices, sh.faces, [], sh.camera, sh.settings(), sh.fog({}), zbuffer=mzb)
    assert np.array_equal(mpx.reshape(px.shape), px) and np.array_equal(mzb.view(np.uint32).reshape(zb.shape), zb)
    alone = _drawn(WS.sheet("Z").oracle(oracle))
    both = (px[..., :3] == WS.COL_BACK).all(axis=2)
    o_lines = _drawn(WS.sheet("O").oracle(oracle))
    lost = int((alone & ~both).sum()); kept = int((alone & both & ~o_lines).sum())
    print(f"second draw: {lost} of sheet Z's line pixels are hidden by the kept depths, {kept} are drawn again")
    assert (lost, kept) == SECOND_DRAW, (lost, kept)


SECOND_DRAW = (493, 126)          # (measured from the oracle's two frames, asserted)


# ------------------------------------------------------------------------------------------------ CPU: mutations
MUTATIONS = {      # name: (sheet, mode)
    "no_normalise": ("L-fixed", {}),
    "last_occurrence": ("O", {}),
    "depths_not_swapped": ("Z", {}),
    "le": ("Z", {}),
    "half_down": ("L-fixed", {}),
    "floor_i32": ("L-float", {}),
    "no_max1": ("Z", {}),
    "no_saturate": ("T-walk", {}),
    "back_after_overlay": ("O", {"overlay": True}),
    "fused": ("Z", {}),
    "zero_area_front": ("L-fixed", {}),
    "rejected_claims": ("O", {}),
    "joint_dedupe": ("O", {"overlay": True}),
}
# pixels changed (measured from `wire_phases`, asserted)
MEASURED_MUTATIONS = {"no_normalise": 161, "last_occurrence": 1414, "depths_not_swapped": 343, "le": 288, "half_down": 322, "floor_i32": 21, "no_max1": 19,
                      "no_saturate": 201, "back_after_overlay": 838, "fused": 38, "zero_area_front": 3543, "rejected_claims": 255, "joint_dedupe": 272}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_changes_a_named_sheet(oracle, mut):
    name, mode = MUTATIONS[mut]
    n = changed(WS.sheet(name), oracle, mode, mut)
    print(f"mutation {mut}: {n} pixels of sheet {name} {mode or ''}")
    assert n > 0 and n == MEASURED_MUTATIONS[mut], (mut, n)


def test_mutation_rejected_claims_in_xray(oracle):
    """x-ray mode drops every back face from the list: were they to claim their edges all the same, the sheet's lines would appear"""
    sh = WS.sheet("O")
    assert changed(sh, oracle, {"xray": True}, "rejected_claims") > 1000


# ------------------------------------------------------------------------------------------------ GPU
def _same(sh, got, want, what):
    msg = sh.first_difference(got, want, what)
    assert not msg, msg


def _check(sh, oracle, what, mode, fb, tm):
    o = sh.oracle(oracle, **mode)
    _same(sh, fb.pixels, o["px"], what)
    _same(sh, fb.zbuffer.view(np.uint32), o["zb"], what + ", depths")
    assert tm.triangles_drawn == o["tm"].triangles_drawn, what


@gpu
@pytest.mark.parametrize("name", WS.NAMES)
def test_sheet_on_both_routes(oracle, name):
    """a context of its own per route (the global table keeps its smallest size, 1024 slots, for the small sheets): every mode, drop-in
    and resident, twice -- the tile counters must come back to zero by themselves; the route counter moves on the tile route only"""
    from bonnie32_amd import rasterizer as R
    sh = WS.sheet(name)
    for off in (0, R.Context.ROUTE_WIRE_TILES):
        ctx = R.Context(0); ctx.set_routes(off)
        try:
            for label, mode in all_modes(sh):
                for resident in (False, True):
                    for again in range(2):
                        fb, tm = FS.gpu_draw(ctx, sh, resident=resident, fog_name=None if mode.get("fmt8") else sh.fog_name, **mode)
                        _check(sh, oracle, f"{label}, routes off {off}, resident={resident}, draw {again}", mode, fb, tm)
            count = ctx.route_counts()["wire_tiles"]
            print(f"{name}: routes off {off}: wire_tiles {count}")
            assert (count > 0) == (off == 0)
        finally:
            ctx.close()


@gpu
def test_overflowing_frame_then_a_small_one(oracle):
    """T-cap-257 overflows its one tile list (the whole frame falls back to the global kernels); on the SAME context T-follow, T-cap-256
    and T-cap-257 again must each be their own frame: the counters are zero again and the overflow flag is the earlier epoch's"""
    from bonnie32_amd import rasterizer as R
    ctx = R.Context(0)
    try:
        for name in ("T-cap-257", "T-follow", "T-cap-256", "T-cap-257", "T-seg-max", "T-follow"):
            sh = WS.sheet(name)
            fb, tm = FS.gpu_draw(ctx, sh, resident=True)
            _check(sh, oracle, f"after an overflowing frame: {name}", {}, fb, tm)
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("name", ["L-fixed", "L-float", "O"])
def test_sheet_in_three_ragged_bands(gpu_ctx, oracle, name):
    """bands (0, 21), (21, 22), (22, H), each with its own clear: the first tile row is no band start, one band is a single row"""
    sh = WS.sheet(name)
    o = sh.oracle(oracle)
    row = sh.width * 4
    assembled = np.zeros(sh.width * sh.height * 4, np.uint8)
    depths = np.zeros(sh.width * sh.height, np.uint32)
    for y0, y1 in WS.BANDS:
        y1 = sh.height if y1 is None else y1
        fb, tm = FS.gpu_draw(gpu_ctx, sh, resident=True, band=(y0, y1), fog_name=sh.fog_name)
        assembled[y0 * row:y1 * row] = fb.pixels[y0 * row:y1 * row]
        depths[y0 * sh.width:y1 * sh.width] = fb.zbuffer.view(np.uint32)[y0 * sh.width:y1 * sh.width]
        assert tm.triangles_drawn == o["tm"].triangles_drawn
    _same(sh, assembled, o["px"], "bands")
    _same(sh, depths, o["zb"], "bands, depths")


def placed_o():
    """(local vertices, Placement, placed vertices): a rotation about Y by 0.3 rad and an offset in all three axes; the local vertices
    are sheet O's taken back through the inverse in float64, so that the placed ones (Placement.apply: three roundings per coordinate)
    are the sheet's up to an ulp"""
    from bonnie32_amd import rasterizer as R
    sh = WS.sheet("O")
    c, s = f32(np.cos(0.3)), f32(np.sin(0.3))
    pl = R.Placement(cos_f=c, sin_f=s, world_pos=(0.5, -0.25, 0.75))
    P = sh.vertices["pos"].astype(np.float64)
    x, y, z = P[:, 0] - 0.5, P[:, 1] + 0.25, P[:, 2] - 0.75
    local = np.array(sh.vertices, copy=True)
    local["pos"] = np.stack([x * float(c) + z * float(s), y, -x * float(s) + z * float(c)], axis=1).astype(np.float32)
    return local, pl, pl.apply(local)


def test_census_o_placed(oracle):
    """the screen points stay: the placed vertices project to the sheet's integers; the oracle's frame of the placed vertices still has
    hidden and visible first occurrences (the depths are 9, 10 and 11 up to an ulp)"""
    sh = WS.sheet("O")
    local, pl, placed = placed_o()
    assert pl.has_transform and np.abs(local["pos"] - sh.vertices["pos"]).max() > 1.0
    scr, _ = FS.project(placed["pos"], sh.camera, sh.proj, sh.width, sh.height)
    want, _ = sh.projected()
    assert np.array_equal(scr[:, :2], want[:, :2]) and np.abs(scr[:, 2] - want[:, 2]).max() <= 2e-6
    ofb = oracle.Framebuffer(sh.width, sh.height); ofb.clear(FS.CLEAR)
    assert oracle.render_mesh_15(ofb, placed, sh.faces, [], sh.camera, sh.settings(), FS.fog(sh.fog_name))[0] == 0
    assert np.array_equal(ofb.image(), sh.oracle(oracle)["px"])


@gpu
def test_sheet_o_as_a_placed_draw(gpu_ctx, oracle):
    """render_async(placement=...) of the local vertices: the frame is the oracle's of the placed ones (test_census_o_placed)"""
    from bonnie32_amd import rasterizer as R
    sh = WS.sheet("O")
    local, pl, placed = placed_o()
    ofb = oracle.Framebuffer(sh.width, sh.height); ofb.clear(FS.CLEAR)
    rc, otm = oracle.render_mesh_15(ofb, placed, sh.faces, [], sh.camera, sh.settings(), FS.fog(sh.fog_name))
    assert rc == 0
    fb = R.Framebuffer(sh.width, sh.height, gpu_ctx); fb.clear(FS.CLEAR)
    rs = R.ResidentScene(fb, local, sh.faces, [])
    rs.render_async(sh.camera, sh.settings(), FS.fog(sh.fog_name), placement=pl)
    tm = rs.finish()
    _same(sh, fb.pixels, ofb.pixels, "placed")
    _same(sh, fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32), "placed, depths")
    assert tm.triangles_drawn == otm.triangles_drawn


@gpu
def test_two_sheets_as_one_batched_frame(gpu_ctx, oracle):
    """frame_begin / frame_add / frame_end with sheet O (built for sheet L's frame size: a frame has one size) and sheet L as two culled
    meshes: equal to the oracle's two sequential calls on one framebuffer"""
    from bonnie32_amd import rasterizer as R
    a, b = WS.sheet("O-on-L"), WS.sheet("L-fixed")
    assert (a.width, a.height) == (b.width, b.height) and np.array_equal(a.edges_i32(), WS.sheet("O").edges_i32())
    st = a.settings()
    ofb = oracle.Framebuffer(a.width, a.height); ofb.clear(FS.CLEAR)
    for sh in (a, b):
        assert oracle.render_mesh_15(ofb, sh.vertices, sh.faces, [], sh.camera, st, None)[0] == 0
    fb = R.Framebuffer(a.width, a.height, gpu_ctx)
    slots = [R.ResidentScene(fb, sh.vertices, sh.faces, []).detach() for sh in (a, b)]
    try:
        fb.clear(FS.CLEAR)
        gpu_ctx.frame_begin(a.camera, st)
        for rs in slots:
            gpu_ctx.frame_add(rs, backface_cull=True)
        gpu_ctx.frame_end()
        gpu_ctx.finish()
        _same(a, fb.pixels, ofb.pixels, "batched frame")
        _same(a, fb.zbuffer.view(np.uint32), ofb.zbuffer.view(np.uint32), "batched frame, depths")
    finally:
        for rs in slots:
            rs.close()


@gpu
def test_second_draw_onto_the_kept_zbuffer(oracle):
    """sheet O, then sheet Z without a clear (test_second_draw_tests_lines_against_the_kept_depths), drop-in and resident, on both routes"""
    from bonnie32_amd import rasterizer as R
    want, wantz = second_draw_oracle(oracle)
    first, second = WS.sheet("O"), WS.sheet("Z")
    for off in (0, R.Context.ROUTE_WIRE_TILES):
        ctx = R.Context(0); ctx.set_routes(off)
        try:
            for resident in (False, True):
                fb, _ = FS.gpu_draw(ctx, first, resident=resident, fog_name=first.fog_name)
                fb, _ = FS.gpu_draw(ctx, second, resident=resident, fb=fb)
                _same(first, fb.pixels, want, f"second draw, routes off {off}, resident={resident}")
                _same(first, fb.zbuffer.view(np.uint32), wantz, f"second draw depths, routes off {off}, resident={resident}")
        finally:
            ctx.close()


@gpu
@pytest.mark.parametrize("case", list(WS.REFUSE_CASES))
def test_refusal_on_both_routes(oracle, case):
    """a refused edge returns B32_E_UNSUPPORTED from the tile route (k_wire_bin) and from the global kernels (draw_line_dev); its drawn
    neighbour is the oracle's frame on both"""
    from bonnie32_amd import rasterizer as R
    sh = WS.sheet("T-refuse-" + case)
    refused = WS.REFUSE_CASES[case][3]
    for off in (0, R.Context.ROUTE_WIRE_TILES):
        ctx = R.Context(0); ctx.set_routes(off)
        try:
            for resident in (False, True):
                if refused:
                    with pytest.raises(R.B32Error) as e:
                        FS.gpu_draw(ctx, sh, resident=resident)
                    assert e.value.code == abi.B32_E_UNSUPPORTED, (case, off, resident)
                else:
                    fb, tm = FS.gpu_draw(ctx, sh, resident=resident)
                    _check(sh, oracle, f"{case}, routes off {off}, resident={resident}", {}, fb, tm)
        finally:
            ctx.close()


def alternating_oracle(O, rounds):
    """(pixels, z-buffer bits) after `rounds` times (O-big-a, O-big-b) on one framebuffer, z-buffer mode, no clear.  A round that leaves
    the framebuffer as it found it ends the drawing: every later round would too."""
    a, b = WS.sheet("O-big-a"), WS.sheet("O-big-b")
    fb = O.Framebuffer(a.width, a.height); fb.clear(FS.CLEAR)
    for _ in range(rounds):
        before = (fb.pixels.copy(), fb.zbuffer.copy())
        for sh in (a, b):
            assert O.render_mesh_15(fb, sh.vertices, sh.faces, [], sh.camera, a.settings(), None)[0] == 0
        if np.array_equal(before[0], fb.pixels) and np.array_equal(before[1].view(np.uint32), fb.zbuffer.view(np.uint32)):
            break
    return fb.pixels.copy(), fb.zbuffer.view(np.uint32).copy()


def test_census_big_sheets(oracle):
    """the two meshes of the frames-in-flight test: more than 8192 faces each (the direct-binning route) on a frame of more than 512 fill
    tiles (two per CU of an MI355X: plan_pipe_hint), every cell's occurrences on the edge A-B by their projected integers, the second
    sheet's floors nearer than the first's, and the frame still changes after the first round of the alternation (depths do not): the
    later frames matter"""
    a, b = WS.sheet("O-big-a"), WS.sheet("O-big-b")
    assert a.n > 8192 and b.n > 8192 and ((a.width + 63) // 64) * ((a.height + 63) // 64) > 512
    for sh in (a, b):
        assert len(_occurrence_edges(sh)) == 9 * 192
    za, zb = a.oracle(oracle)["zb"].view(np.float32), b.oracle(oracle)["zb"].view(np.float32)
    assert float(zb.min()) < float(za.min()) and not np.array_equal(_drawn(a.oracle(oracle)), _drawn(b.oracle(oracle)))
    one, five = alternating_oracle(oracle, 1), alternating_oracle(oracle, 5)
    changed_later = int((one[0].reshape(-1, 4) != five[0].reshape(-1, 4)).any(axis=1).sum())
    print(f"alternation: {changed_later} pixels change after the first round")
    assert changed_later > 0 and np.array_equal(one[1], five[1])          # (the second sheet's floors paint over the first's lines, which the next round draws again)


@gpu
def test_two_sheets_alternating_back_to_back(oracle):
    """Two large meshes (O-big-a, O-big-b: nine blocks of sheet O's cells on 1920 x 1440) alternating four times on one context with no
    host wait between the submissions, z-buffer mode, no clear, each in a slot of its own swapped in per frame (an undetached
    ResidentScene IS the context's one current scene).  As in test_wireframe_frames_two_in_flight every scene is settled by one finished
    frame first.  Of the eight frames after that the first finds no frame pending; the other seven take the other frame set, run their
    setup kernel and their wire binning on the side stream beside the previous frame's fill and wire kernels -- the `pipelined` counter
    says so -- and all ten go through the tile route.  Depths and line pixels accumulate: every frame's wire kernels must have read their
    own frame's list, their own epoch's flags and the kept depths.
    (Sheets of at most about 1 500 faces cannot enter this route -- choose_frame_set wants more than 2048 faces, plan_pipe_hint the
    direct-binning route and more than two tiles per CU -- hence the large meshes.)"""
    from bonnie32_amd import rasterizer as R
    a, b = WS.sheet("O-big-a"), WS.sheet("O-big-b")
    st = a.settings()
    want, wantz = alternating_oracle(oracle, 5)
    ctx = R.Context(0)
    scenes = []
    try:
        ctx.set_async_depth(1); ctx.set_pipeline_depth(2)
        fb = R.Framebuffer(a.width, a.height, ctx); fb.clear(FS.CLEAR)
        scenes = [R.ResidentScene(fb, sh.vertices, sh.faces, []).detach() for sh in (a, b)]
        for rs in scenes:
            rs.render_async(a.camera, st); rs.finish()
        before = ctx.route_counts()
        for _ in range(4):
            for rs in scenes:
                rs.render_async(a.camera, st)
        scenes[-1].finish()
        after = ctx.route_counts()
        moved = {k: after[k] - before[k] for k in ("pipelined", "wire_tiles", "direct_bin")}
        print("alternating frames, counters moved by", moved)
        _same(a, fb.pixels, want, "alternating")
        _same(a, fb.zbuffer.view(np.uint32), wantz, "alternating, depths")
        assert moved == {"pipelined": 7, "wire_tiles": 8, "direct_bin": 8}, moved
    finally:
        for rs in scenes:
            rs.close()
        ctx.close()
