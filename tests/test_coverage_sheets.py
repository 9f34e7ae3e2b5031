"""Fill coverage per triangle, without overdraw, at the limits where its routes change hands (tests/coverage_sheets.py builds the sheets).

The fill decides which pixels a triangle covers in five ways (per-pixel toleranced test, row trimming in front of it, exact row intervals
of the span route, the literal edge walk of F_SLOW surfaces, the closed form of the shading step); all must reproduce render.rs:1536-1542
pixel for pixel.  In a frame of overlapping triangles a coverage decision shows only where its triangle is on top; on a sheet every
triangle has a cell of its own, so every decision of every route is a pixel of the frame, which is compared bit for bit with the oracle's.

CPU tests (no mark) keep the sheets honest against the oracle; GPU tests run every sheet through fragment counting on and off, the route
masks of b32_set_routes, resident and drop-in draws, z-buffer mode, the 8-bit-colour path and row bands."""
import numpy as np
import pytest

from tests import coverage_sheets as CS

gpu = pytest.mark.gpu
CLOSED = [n for n in CS.NAMES if n[0] in "ABD" and n != "B-outside"]       # (the "outside" sheet holds no eligible triangle)
AB = [n for n in CS.NAMES if n[0] in "AB"]


# ------------------------------------------------------------------------------------------------ CPU: what the sheets are
@pytest.mark.parametrize("name", CS.NAMES)
def test_placement(oracle, name):
    """Every vertex hit its integer target, and no pixel carries the colour of a triangle that does not own its cell (family F: of
    one of the two that do); without overlap the oracle's store count is the number of coloured pixels: nothing is drawn twice."""
    sh = CS.sheet(name)
    idx = CS.check_placement(sh, oracle)
    _, _, tm, _ = sh.oracle(oracle)
    assert tm.triangles_drawn == sh.n
    drawn = int((idx >= 0).sum())
    print(f"{name}: {sh.n} triangles, {sh.width} x {sh.height}, {tm.fragments} fragments, {drawn} pixels drawn")
    if not sh.overlap:
        assert tm.fragments == drawn
    else:
        assert tm.fragments > drawn


@pytest.mark.parametrize("name", CLOSED)
def test_reference_covers_the_closed_integer_triangle(oracle, name):
    """Claim (1) of tests/test_span_cover.py through the reference restatement: for A <= 8192 and extent <= 512 the toleranced float
    test passes exactly on  s*w0 >= 0, s*w1 >= 0, A - s*w0 - s*w1 >= 0  -- over the whole cell, not only the triangle's box."""
    sh = CS.sheet(name)
    px, _, _, _ = sh.oracle(oracle)
    idx = sh.decode(px)
    checked = 0
    for i in range(sh.n):
        if not CS.span_eligible(sh.tris[i]):
            continue
        got, win = sh.covered(idx, i)
        assert np.array_equal(got, CS.int_inside(sh.tris[i], *win)), sh.describe(i)
        checked += 1
    assert checked == sh.n or (name == "B-mixed" and checked == CS.sheet("B-inside").n)


def test_outside_sheet_shows_pixels_beyond_the_integer_triangle(oracle):
    """Beyond the span route's limit the tolerance admits pixels outside the integer triangle: the triangles of the "outside" sheet with
    A >= 10000 carry such pixels, so a device that took row intervals for them would draw another frame."""
    sh = CS.sheet("B-outside")
    px, _, _, _ = sh.oracle(oracle)
    idx = sh.decode(px)
    extra = missing = big = 0
    for i in range(sh.n):
        if CS.doubled_area(sh.tris[i]) < 10000:
            continue
        got, win = sh.covered(idx, i)
        want = CS.int_inside(sh.tris[i], *win)
        extra += int((got & ~want).sum()); missing += int((want & ~got).sum()); big += 1
    print(f"B-outside: {extra} oracle pixels outside and {missing} missing from the integer triangles of {big} triangles with A >= 10000")
    assert big > 0 and extra > 0


def test_far_vertex_cases_are_on_the_side_they_claim():
    """Family E labels (plain integers, b32_setup.hip's guard restated): both sides of the 16-bit vertex form, of 2 * amax * dmax = 2^24
    and of the corner products = 2^24 (F_SLOW) are present."""
    for name in ("E-rows", "E-columns"):
        labels = CS.sheet(name).labels
        narrow = {q["narrow"] for l, q in labels if l == "cmax16"}
        quick = {q["quick"] >= 1 << 24 for l, q in labels if l == "quick"}
        slow = {q["slow"] for l, q in labels if l == "corner"}
        assert narrow == quick == slow == {False, True}
        assert all(q["quick"] >= 1 << 24 for l, q in labels if l == "corner")


# ------------------------------------------------------------------------------------------------ GPU: every route, bit for bit
def _same(sh, got, want, route):
    msg = sh.first_difference(got, want, route)
    assert not msg, msg


@gpu
@pytest.mark.parametrize("name", CS.NAMES)
def test_sheet_with_and_without_fragment_counting(gpu_ctx, oracle, name):
    """EXACT coverage (counting on: the store count is the oracle's) and CHEAP / span coverage (counting off), drop-in and resident."""
    sh = CS.sheet(name)
    want, _, etm, _ = sh.oracle(oracle)
    try:
        for counting in (1, 0):
            gpu_ctx.set_fragment_counting(counting)
            for resident in (False, True):
                fb, tm = CS.gpu_draw(gpu_ctx, sh, resident=resident)
                _same(sh, fb.pixels, want, f"counting={counting} resident={resident}")
                assert tm.triangles_drawn == etm.triangles_drawn
                if counting:
                    assert tm.fragments == etm.fragments, (name, resident)
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", CS.NAMES)
def test_sheet_on_every_route(gpu_ctx, oracle, name):
    """b32_set_routes switches one route off at a time, counting off; b32_route_count shows that the span route ran exactly when it was on."""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    sh = CS.sheet(name)
    want, _, etm, _ = sh.oracle(oracle)
    try:
        gpu_ctx.set_fragment_counting(0)
        for off in (0, C.ROUTE_SPAN_COVER, C.ROUTE_DIRECT_BIN, C.ROUTE_INLINE_BIN, C.ROUTE_CUT_TILES, C.ROUTE_WIDE_GROUPS, C.ROUTE_SORT_FREE):
            gpu_ctx.set_routes(off)
            before = gpu_ctx.route_counts()
            fb, tm = CS.gpu_draw(gpu_ctx, sh, resident=True)
            after = gpu_ctx.route_counts()
            _same(sh, fb.pixels, want, f"routes off: {off}")
            assert tm.triangles_drawn == etm.triangles_drawn
            span_on = not (off & (C.ROUTE_SPAN_COVER | C.ROUTE_SORT_FREE))        # (the span route is part of the sort-free path)
            assert (after["span_cover"] > before["span_cover"]) == span_on, (off, before, after)
            if off & C.ROUTE_DIRECT_BIN:
                assert after["direct_bin"] == before["direct_bin"]
            if off & C.ROUTE_INLINE_BIN:
                assert after["inline_bin"] == before["inline_bin"]
            if off & C.ROUTE_SORT_FREE:
                assert after["keyed"] > before["keyed"] and after["direct_bin"] == before["direct_bin"] and after["inline_bin"] == before["inline_bin"]
    finally:
        gpu_ctx.set_routes(0)
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", CS.NAMES)
def test_sheet_in_zbuffer_mode(gpu_ctx, oracle, name):
    """use_zbuffer: framebuffer AND z-buffer bit-equal.  All depths are equal, so family F is the tie case: strict `<`, the first face wins."""
    sh = CS.sheet(name)
    want, wantz, etm, _ = sh.oracle(oracle, zbuffer=True)
    try:
        for counting in (1, 0):
            gpu_ctx.set_fragment_counting(counting)
            for resident in (False, True):
                fb, tm = CS.gpu_draw(gpu_ctx, sh, resident=resident, zbuffer=True)
                _same(sh, fb.pixels, want, f"z-buffer counting={counting} resident={resident}")
                _same(sh, fb.zbuffer.view(np.uint32), wantz, f"z-buffer depths counting={counting} resident={resident}")
                assert tm.triangles_drawn == etm.triangles_drawn
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", AB)
def test_sheet_on_the_8bit_colour_path(gpu_ctx, oracle, name):
    """render_mesh (no texture bound) for families A and B."""
    sh = CS.sheet(name)
    want, _, etm, _ = sh.oracle(oracle, fmt8=True)
    try:
        for counting in (1, 0):
            gpu_ctx.set_fragment_counting(counting)
            for resident in (False, True):
                fb, tm = CS.gpu_draw(gpu_ctx, sh, resident=resident, fmt8=True)
                _same(sh, fb.pixels, want, f"8-bit counting={counting} resident={resident}")
                assert tm.triangles_drawn == etm.triangles_drawn
                if tm.fragments:
                    assert tm.fragments == etm.fragments
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", ["A", "B-inside"])
def test_sheet_in_row_bands(gpu_ctx, oracle, name):
    """Bands (0, 37), (37, 38), (38, H): the second is a single row through the middle of a row of cells; the three partial frames
    assemble to the oracle's."""
    sh = CS.sheet(name)
    want, _, etm, _ = sh.oracle(oracle)
    row = sh.width * 4
    try:
        for counting in (0, 1):
            gpu_ctx.set_fragment_counting(counting)
            assembled = np.zeros(sh.width * sh.height * 4, np.uint8)
            for y0, y1 in ((0, 37), (37, 38), (38, sh.height)):
                fb, tm = CS.gpu_draw(gpu_ctx, sh, resident=True, band=(y0, y1))
                assembled[y0 * row:y1 * row] = fb.pixels[y0 * row:y1 * row]
                assert tm.triangles_drawn == etm.triangles_drawn
            _same(sh, assembled, want, f"bands counting={counting}")
    finally:
        gpu_ctx.set_fragment_counting(1)
