"""Merged runs member by member (b32_frame_begin / _add_scene[_placed] / _end, b32_frame_submit[_placed]; csrc/b32_batch.hip, k_merge_mesh,
k_offset_tex and the batched branch of k_setup) on the frames of tests/run_sheets.py, always against the oracle's sequential calls, bit
for bit in pixels and depth.

CPU tests (the oracle alone): the census -- every cell a family claims is what it claims --, the named mutations of the call sequence
-- each error the GPU tests are there to catch changes a cell of its family --, and plan_runs, a restatement of the run rule written
from the paragraph on merged runs in include/b32raster.h.

GPU tests: every frame through both entry points with fragment counting on and off and the exact batch counters; families R, T, Z and B on
every route a merged run can take; family L at the face counts where the route changes and through the global-sort redraw; T and Z in two
ragged bands; the error contract of a run (B32_E_INDEX, B32_E_NAN_KEY: the run undrawn, the others drawn, the next frame clean; B32_E_ARG
for a slot that does not hold its scene); the 64-entry cache of merged meshes under deep asynchronous mode.  Eviction under deep mode and
the redraw of a merged run are checked for equality only, never for speed."""
import numpy as np
import pytest

from bonnie32_amd import abi
from tests import run_sheets as RS

gpu = pytest.mark.gpu
BIN_ROUTES = ("direct_bin", "inline_bin", "counting_sort", "keyed")
REDRAWS = ("redraw_region", "redraw_global_sort", "redraw_pairs")
CLEAR_RGB = np.array([RS.CLEAR.r, RS.CLEAR.g, RS.CLEAR.b], np.uint8)
MAX_RUN = 32                                     # "At most 32 meshes are merged into one draw; longer runs are split."
CENSUS_FRAMES = list(RS.frames()) + list(RS.L_FRAMES) + ["L-stack", "T-error"] + [f"NaN-{k}" for k in RS.NAN_KINDS]


# ------------------------------------------------------------------------------------------------ the run rule, from b32raster.h
def plan_runs(fr):
    """The runs of a frame as the header states them: in z-buffer mode with RGB555 output, runs of meshes, each run ended by (and holding) the
    first mesh that has a transparent pass; at most 32 meshes per run; painter's mode, x-ray, orthographic views, the wireframe overlay (and
    batching switched off) draw mesh by mesh; an 8-bit-colour slot, a slot with a wireframe phase (base backface_wireframe and its own
    culling) and an empty slot are drawn on their own and end the run in front of them; a run of one is a draw on its own.
    -> [[draw, ...], ...]"""
    st = fr.base
    merging = st.use_zbuffer and st.use_rgb555 and not st.xray_mode and st.ortho_projection is None and not st.wireframe_overlay and \
        not fr.routes_off & RS.ROUTE_BATCH
    runs, cur = [], []
    for i, d in enumerate(fr.draws):
        m = fr.members[d.member]
        alone = not merging or m.fmt8 or m.nf == 0 or (st.backface_wireframe and d.cull)
        if alone:
            if cur:
                runs.append(cur); cur = []
            runs.append([i])
            continue
        cur.append(i)
        if m.blends or len(cur) == MAX_RUN:
            runs.append(cur); cur = []
    if cur:
        runs.append(cur)
    return runs


def expected_counts(fr, seen=None):
    """merged draws, draws on their own and merged meshes built by one frame; seen: the runs (tuples of members) this context has merged"""
    runs = plan_runs(fr)
    merged = [tuple(fr.draws[i].member for i in r) for r in runs if len(r) > 1]
    seen = set() if seen is None else seen
    built = len(set(merged) - seen)
    seen |= set(merged)
    return dict(merged_draws=len(merged), single_draws=sum(len(r) == 1 for r in runs), merged_built=built)


def test_plan_runs_against_counts_written_out_by_hand():
    want = {"R-2": [2], "R-31": [31], "R-32": [32], "R-33": [32, 1], "R-64": [32, 32], "R-65": [32, 32, 1],
            "T": [6], "Z-two": [2], "Z-three": [3], "Z-same": [3], "Z-placed": [3], "Z-runs": [2, 2],
            "B": [3, 3, 1, 2, 2],
            "S-8bit": [2, 1, 2], "S-empty": [2, 1, 2], "S-wire": [2, 1, 2], "S-leftover": [3, 1], "S-blend-first-and-last": [1, 3],
            "S-painter": [1, 1, 1], "S-ortho": [1, 1, 1], "S-xray": [1, 1, 1], "S-overlay": [1, 1, 1], "S-batch-off": [1, 1, 1],
            "L-8192": [32], "L-8193": [32], "L-2048-blend": [32], "L-2049-blend": [32], "L-stack": [2], "T-error": [3, 3, 2]}
    for name, lengths in want.items():
        fr = RS.frame(name)
        runs = plan_runs(fr)
        assert [len(r) for r in runs] == lengths, (name, runs)
        assert [i for r in runs for i in r] == list(range(len(fr.draws))), name
    b = RS.frame("B")
    assert [tuple(RS.B_ORDER[i] for i in r) for r in plan_runs(b)] == list(RS.B_RUNS)
    assert expected_counts(RS.frame("R-65")) == dict(merged_draws=2, single_draws=1, merged_built=2)
    assert expected_counts(RS.frame("R-33")) == dict(merged_draws=1, single_draws=1, merged_built=1)
    assert expected_counts(b) == dict(merged_draws=4, single_draws=1, merged_built=4)
    assert expected_counts(RS.frame("S-wire")) == dict(merged_draws=2, single_draws=1, merged_built=2)
    assert expected_counts(RS.frame("S-xray")) == dict(merged_draws=0, single_draws=3, merged_built=0)
    seen = set()
    assert expected_counts(RS.frame("Z-same"), seen)["merged_built"] == 1 and expected_counts(RS.frame("Z-same"), seen)["merged_built"] == 0
    for kind in RS.NAN_KINDS:
        assert [len(r) for r in plan_runs(RS.frame(f"NaN-{kind}"))] == [3, 3, 2]


# ------------------------------------------------------------------------------------------------ census
def _covered(res, win):
    return (res["px"][win][..., :3] != CLEAR_RGB).any(axis=2)


def _without_texture(oracle, fr, j, cell):
    """draw j alone, the face of that cell untextured"""
    c = fr.calls()[j]
    f = np.array(c["f"], copy=True)
    f["texture_id"][fr.members[fr.draws[j].member].cells.index(cell)] = abi.NO_TEXTURE
    c["f"] = f
    return RS.render_calls(oracle, [c])


def _check_claim(oracle, fr, claim):
    kind = claim[0]
    full = fr.oracle(oracle)
    what = f"[{fr.name}] {claim}: cell '{fr.cell_tags[claim[2] if kind not in ('tie', 'no_tie', 'empty') else claim[1]]}'"
    if kind in ("drawn", "absent"):
        _, j, c = claim
        assert _covered(fr.solo(oracle, j), fr.window(c)).any() == (kind == "drawn"), what
    elif kind in ("textured", "untextured"):
        _, j, c = claim
        win = fr.window(c)
        solo, plain = fr.solo(oracle, j), _without_texture(oracle, fr, j, c)
        assert _covered(solo, win).any(), what
        assert np.array_equal(solo["px"][win], plain["px"][win]) == (kind == "untextured"), what
    elif kind == "tie":
        _, c, who = claim
        win = fr.window(c)
        first = fr.solo(oracle, who[0])
        assert _covered(first, win).sum() > 20, what
        for j in who[1:]:
            other = fr.solo(oracle, j)
            assert np.array_equal(_covered(first, win), _covered(other, win)), what
            assert np.array_equal(first["zb"].reshape(RS.H, RS.W)[win], other["zb"].reshape(RS.H, RS.W)[win]), what + ": the depths differ at some fragment"
            assert not np.array_equal(first["px"][win], other["px"][win]), what + ": the tying faces look the same"
        assert np.array_equal(full["px"][win], first["px"][win]), what + ": the earlier member does not win in the oracle's frame"
    elif kind == "no_tie":
        _, c, j = claim
        win = fr.window(c)
        first, later = fr.solo(oracle, 0), fr.solo(oracle, j)
        won = (full["px"][win] != first["px"][win]).any(axis=2)
        assert won.any() and np.array_equal(full["px"][win][won], later["px"][win][won]), what
    elif kind == "empty":
        assert not _covered(full, fr.window(claim[1])).any(), what
    elif kind == "wins":
        _, j, c = claim
        win = fr.window(c)
        assert _covered(full, win).any() and np.array_equal(full["px"][win], fr.solo(oracle, j)["px"][win]), what
    elif kind in ("blended", "not_blended"):
        _, j, c, _under = claim
        calls = fr.calls()[:j + 1]
        with_pass = RS.render_calls(oracle, calls)
        calls[j] = dict(calls[j]); calls[j]["f"] = RS._split(fr.members[j], False)
        without = RS.render_calls(oracle, calls)
        win = fr.window(c)
        assert _covered(without, win).any(), what
        assert np.array_equal(with_pass["px"][win], without["px"][win]) == (kind == "not_blended"), what
        calls[j] = RS.solid_call(fr.calls()[j])
        solid = RS.render_calls(oracle, calls)                         # the same faces drawn as opaque ones: a blended cell is neither
        assert np.array_equal(with_pass["px"][win], solid["px"][win]) == (kind == "not_blended"), what
        assert np.array_equal(with_pass["zb"], without["zb"]), what + ": the transparent pass wrote depth"
    else:
        raise AssertionError(f"unknown claim {claim}")


@pytest.mark.parametrize("name", CENSUS_FRAMES)
def test_census(oracle, name):
    """every cell is what its family says, in the oracle's frame (no claim is waived: a sheet that misses its census is rebuilt)"""
    fr = RS.frame(name)
    full = fr.oracle(oracle)
    for m in fr.members:
        assert (m.faces["_pad"][1::2] == 0xFF).all() and (m.faces["_pad"][0::2] == 0).all()
    for claim in fr.claims:
        _check_claim(oracle, fr, claim)
    if fr.family in ("R", "T", "Z", "B") and name != "T-error":
        assert fr.claims and all(rc == 0 for rc in full["rcs"]), name
        claimed = {c[2] if c[0] not in ("tie", "no_tie", "empty") else c[1] for c in fr.claims}
        used = {c for m in fr.members for c in m.cells}
        assert used <= claimed | {c for c in used if "own" in fr.cell_tags[c]}, (name, sorted(used - claimed))
    if name.startswith("R-"):
        culled = sum(c[0] == "absent" for c in fr.claims)
        assert sum(full["drawn"]) == 3 * len(fr.draws) - culled and culled >= len(fr.draws) // 2
        assert sum(d.placement is not None for d in fr.draws) == len(fr.draws) // 3
    if name == "T":
        for m, size in zip(fr.members, RS.t_pool_sizes()):
            pool = np.concatenate([t.pixels for t in m.textures] + [np.zeros(0, np.uint16)])
            assert len(pool) == size
            assert size == 0 or (pool[0] == RS.FIRST_TEXEL and pool[-1] == RS.LAST_TEXEL), m.name
        device_bases = np.cumsum(RS.t_pool_sizes(padded=True))[:-1]
        assert all(b % 32 for b in device_bases), device_bases           # a skip-mask word straddles two members' pools
        assert {(t.width, t.height) for m in fr.members for t in m.textures} == {(1, 1), (3, 5), (7, 9), (8, 8), (0, 0)}
        assert fr.members[5].textures[0].blend_mode == abi.AVERAGE and not fr.members[4].blends
    if name == "B":
        assert sum(c[0] == "blended" for c in fr.claims) == 15 and sum(c[0] == "not_blended" for c in fr.claims) == 30
        assert [m.blends for m in fr.members] == [n in "CFGU" for n in RS.B_ORDER]
        u = fr.members[RS.B_ORDER.index("U")]
        assert not len(RS._split(u, True)) and u.textures[0].blend_mode != abi.OPAQUE
    if fr.family == "L" and name != "L-stack":
        assert sum(m.nf for m in fr.members) == fr.total == sum(full["drawn"])
        assert max(m.nf for m in fr.members) <= 257
        z = full["zb"].view(np.float32).reshape(RS.H, RS.W)
        i = np.arange(fr.total)
        if name.endswith("-blend"):                      # the last face is the transparent one: it writes no depth, its pixel shows it
            x, y = RS._tiny_origin(fr.total - 1)
            assert (full["px"][y, x, :3] != CLEAR_RGB).any()
            i = i[:-1]
        xs, ys = 2 * (i % (RS.W // 2)), 2 * (i // (RS.W // 2))
        # the depth at a face's origin pixel names its depth class i % 5, which none of its four neighbours on the grid shares
        assert np.array_equal(np.rint(z[ys, xs]).astype(np.int64), 14 + i % 5), f"{name}: a face owns no pixel"
    if name == "L-stack":
        assert len(RS._split(fr.members[1], True)) == RS.STACK == 2049 and len({tuple(p) for p in fr.members[1].vertices["pos"][:, 2:3].tolist()}) == RS.STACK
    if name == "T-error":
        assert [rc for rc in full["rcs"]] == [0, 0, 0, 0, abi.B32_E_INDEX, 0, 0, 0]
        assert not _covered(full, fr.window(fr.error_cell)).any()
    if name.startswith("NaN-"):
        want = [0] * 8
        if name == "NaN-pair":
            want[5] = abi.B32_E_NAN_KEY
        assert full["rcs"] == want, (name, full["rcs"])
    if fr.family == "S":
        assert all(rc == 0 for rc in full["rcs"]) and _covered(full, (slice(None), slice(None))).any()


def test_census_of_the_cache_runs(oracle):
    pairs = RS.c_pairs()
    assert len(pairs) == 66 == len(set(pairs)) and all(a < b for a, b in pairs)
    members = RS.c_members()[0]
    assert len({m.nf for m in members}) == RS.C_SLOTS
    sizes = [members[a].nf + members[b].nf for a, b in pairs]
    assert sizes[0] == max(sizes) and sizes[64] < sizes[0]        # the 65th run is rebuilt into the entry of the largest
    for a, b in (pairs[0], pairs[64], pairs[65]):
        fr = RS.family_c(a, b)
        for claim in fr.claims:
            _check_claim(oracle, fr, claim)
        swapped = RS.render_calls(oracle, fr.calls()[::-1])
        assert [t for _, t in fr.changed_cells(fr.oracle(oracle), swapped)] == ["C tie cell shared by every member"]


# ------------------------------------------------------------------------------------------------ mutations
MUTATION_CELLS = {          # a cell every mutation must change (a substring of its tag), beside belonging to the family
    "rows_shifted": "R member 0 front", "rows_mod_16": "R member 16 front", "row_32_aliases_0": "R member 32 front",
    "placement_of_neighbour": "R member 1 front", "tex_unbounded": "T member 4 texture id id = nt", "pool_base_rounded_to_2": "T member 3 identity",
    "pool_base_rounded_to_32": "T member 3 identity", "mask_of_neighbour": "T member 1 last texel", "vert_unbounded": "error cell",
    "tie_later": "Z tie of all members", "tie_by_face_index": "face 70", "blend_not_last": "B C's add face in front of B",
    "transparent_writes_depth": "B C's add face in front of B",
}


@pytest.mark.parametrize("name", list(RS.MUTATIONS))
def test_named_mutation_changes_a_cell_of_its_family(oracle, name):
    frame_name, fn = RS.MUTATIONS[name]
    fr = RS.frame(frame_name)
    changed = fr.changed_cells(fr.oracle(oracle), fn(oracle, fr))
    print(f"mutation {name} on {frame_name}: {len(changed)} cells change, first: {changed[:3]}")
    assert changed, f"{name} changes nothing on {frame_name}: the sheet cannot show this error"
    assert all(c < len(fr.cell_tags) for c, _ in changed), (name, "a pixel outside every cell changed")
    assert any(MUTATION_CELLS[name] in tag for _, tag in changed), (name, changed)
    if name == "row_32_aliases_0":
        assert {tag.split(" front")[0].split(" back")[0].split(" deep")[0] for _, tag in changed} == {"R member 32"}
    if name == "tie_by_face_index":
        assert all(tag.startswith("Z ") for _, tag in changed)
    if name == "vert_unbounded":                  # (and the member's valid face: the call no longer fails)
        assert fr.error_cell in [c for c, _ in changed] and all("error cell" in t or "bad-index member" in t for _, t in changed)
    if name == "transparent_writes_depth":
        assert fr.d_cells[1] in [c for c, _ in changed]


# ------------------------------------------------------------------------------------------------ the device
_slots = {}


def _slots_of(ctx, fb, fr):
    """the frame's members resident in that context, uploaded once per context and member"""
    out = []
    for m in fr.members:
        key = (id(ctx), id(m))
        if key not in _slots:
            one = RS.Frame("one", fr.family, [m], [], fr.cell, [])
            _slots[key] = (RS.upload(fb, one)[0], m)
        out.append(_slots[key][0])
    return out


def _new_fb(ctx):
    from bonnie32_amd import rasterizer as R
    return R.Framebuffer(RS.W, RS.H, ctx)


def _same(fr, fb, want, what):
    msg = fr.first_difference(fb.pixels, want["px"], what)
    assert not msg, msg
    msg = fr.first_difference(fb.zbuffer.view(np.uint32), want["zb"], what + ", depth")
    assert not msg, msg


def _last_run_drawn(fr, o):
    return sum(o["drawn"][i] for i in plan_runs(fr)[-1])


@gpu
@pytest.mark.parametrize("name", list(RS.frames()) + list(RS.L_FRAMES))
def test_every_sheet_through_both_entry_points(oracle, name):
    """frame_begin / frame_add / frame_end and frame_submit, fragment counting on and off, in a context of the test's own: pixels and depth
    bits of the oracle's sequential calls, the exact movement of the batch counters as plan_runs gives it, the last draw's triangle count"""
    from bonnie32_amd import rasterizer as R
    import __graft_entry__ as g
    g.build()
    fr = RS.frame(name)
    o = fr.oracle(oracle)
    ctx = R.Context(0)
    try:
        ctx.set_routes(fr.routes_off)
        fb = R.Framebuffer(RS.W, RS.H, ctx)
        slots = RS.upload(fb, fr)
        seen, frames = set(), 0
        for counting in (1, 0):
            ctx.set_fragment_counting(counting)
            for entry in ("begin", "submit"):
                before = ctx.batch_counts()
                tm = RS.gpu_frame(ctx, fb, fr, slots, entry)
                frames += 1
                _same(fr, fb, o, f"{entry}, counting={counting}")
                after = ctx.batch_counts()
                want = expected_counts(fr, seen)
                assert {k: after[k] - before[k] for k in want} == want, (name, entry, counting)
                assert after["frames"] == frames
                assert tm.triangles_drawn == _last_run_drawn(fr, o), (name, entry, counting)
        for rs in slots:
            rs.close()
    finally:
        ctx.close()


def _route_case(ctx, oracle, name, off, expect, counting=(1, 0), restore=0):
    from bonnie32_amd import rasterizer as R
    fr = RS.frame(name)
    o = fr.oracle(oracle)
    fb = _new_fb(ctx)
    slots = _slots_of(ctx, fb, fr)
    draws = len(plan_runs(fr))
    try:
        ctx.set_routes(off)
        for c in counting:
            ctx.set_fragment_counting(c)
            before = ctx.route_counts()
            RS.gpu_frame(ctx, fb, fr, slots, "begin")
            after = ctx.route_counts()
            _same(fr, fb, o, f"routes off {off}, counting={c}")
            moved = {k: after[k] - before[k] for k in BIN_ROUTES + REDRAWS if after[k] != before[k]}
            assert moved == {expect: draws}, (name, off, c, moved)
            if off & R.Context.ROUTE_PIPELINE:
                assert after["pipelined"] == before["pipelined"], (name, off)
    finally:
        ctx.set_routes(restore)
        ctx.set_fragment_counting(1)


ROUTE_FRAMES = [f"R-{n}" for n in RS.R_COUNTS] + ["T", "B"] + [f"Z-{v}" for v in RS.Z_VARIANTS]


@gpu
@pytest.mark.parametrize("name", ROUTE_FRAMES)
def test_merged_runs_on_every_sort_free_route(gpu_ctx, oracle, name):
    """default (in-fill list collection), ROUTE_INLINE_BIN off (k_setup's direct binning), ROUTE_DIRECT_BIN off as well (the counting sort),
    ROUTE_PIPELINE off: after each frame the counter of that route, and of no other, has moved once per draw"""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    for off, expect in ((0, "inline_bin"), (C.ROUTE_INLINE_BIN, "direct_bin"), (C.ROUTE_INLINE_BIN | C.ROUTE_DIRECT_BIN, "counting_sort"),
                        (C.ROUTE_PIPELINE, "inline_bin")):
        _route_case(gpu_ctx, oracle, name, off, expect)


@gpu
@pytest.mark.parametrize("name", ROUTE_FRAMES)
def test_merged_runs_through_the_keyed_context(keyed_ctx, oracle, name):
    """ROUTE_SORT_FREE off from the start: the keyed z-buffer kernel draws the merged mesh with the frame's MeshTable"""
    from bonnie32_amd import rasterizer as R
    _route_case(keyed_ctx, oracle, name, R.Context.ROUTE_SORT_FREE, "keyed", restore=R.Context.ROUTE_SORT_FREE)


@gpu
@pytest.mark.parametrize("name,expect", [("L-8192", "inline_bin"), ("L-8193", "direct_bin"), ("L-2048-blend", "inline_bin"), ("L-2049-blend", "direct_bin")])
def test_large_runs_of_small_members_change_route_at_the_merged_face_count(gpu_ctx, oracle, name, expect):
    """8192 faces (2048 with the class split) are the last run the fill collects itself; one more face takes k_setup's direct binning.  Every
    member has at most 257 faces: only the merged count can decide.  Then without the packed position streams."""
    from bonnie32_amd import rasterizer as R
    _route_case(gpu_ctx, oracle, name, 0, expect)
    _route_case(gpu_ctx, oracle, name, R.Context.ROUTE_PACKED_STREAMS, expect, counting=(0,))


@gpu
def test_stack_of_2049_transparent_faces_in_a_run_is_redrawn_through_the_global_sort(oracle):
    """safe mode: the run's transparent list on one tile exceeds the rank sort, the frame is redrawn once with the global sort -- with the run's
    MeshTable -- and is not lost.  (Equality only: the redraw is not timed.)"""
    from bonnie32_amd import rasterizer as R
    import __graft_entry__ as g
    g.build()
    fr = RS.frame("L-stack")
    o = fr.oracle(oracle)
    ctx = R.Context(0)
    try:
        fb = R.Framebuffer(RS.W, RS.H, ctx)
        slots = RS.upload(fb, fr)
        for counting in (0, 1):
            ctx.set_fragment_counting(counting)
            before = ctx.route_counts()
            tm = RS.gpu_frame(ctx, fb, fr, slots, "begin")
            after = ctx.route_counts()
            _same(fr, fb, o, f"stack, counting={counting}")
            assert tm.triangles_drawn == sum(o["drawn"])
            if counting == 0:
                assert after["redraw_global_sort"] - before["redraw_global_sort"] == 1, {k: after[k] - before[k] for k in after if after[k] != before[k]}
        assert ctx.batch_counts()["merged_draws"] == 2
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("name", ["T"] + [f"Z-{v}" for v in RS.Z_VARIANTS])
def test_merged_runs_in_two_ragged_bands(gpu_ctx, oracle, name):
    """bands (0, 37) and (37, H): the rows of the two partial frames assemble to the oracle's, pixels and depth"""
    fr = RS.frame(name)
    o = fr.oracle(oracle)
    for counting in (1, 0):
        gpu_ctx.set_fragment_counting(counting)
        try:
            px = np.zeros((RS.H, RS.W, 4), np.uint8)
            zb = np.zeros((RS.H, RS.W), np.uint32)
            for y0, y1 in ((0, 37), (37, RS.H)):
                fb = _new_fb(gpu_ctx)
                slots = _slots_of(gpu_ctx, fb, fr)
                tm = RS.gpu_frame(gpu_ctx, fb, fr, slots, "begin", band=(y0, y1))
                px[y0:y1] = fb.pixels.reshape(RS.H, RS.W, 4)[y0:y1]
                zb[y0:y1] = fb.zbuffer.view(np.uint32).reshape(RS.H, RS.W)[y0:y1]
                assert tm.triangles_drawn == _last_run_drawn(fr, o)
            msg = fr.first_difference(px, o["px"], f"bands, counting={counting}") or fr.first_difference(zb, o["zb"], "bands, depth")
            assert not msg, msg
        finally:
            gpu_ctx.set_fragment_counting(1)
            _new_fb(gpu_ctx)                       # (a new framebuffer owns all its rows again)


def _error_case(ctx, oracle, fr, code):
    """the frame's middle run holds the error: finish raises `code` once, that run's cells keep the clear colour, the other runs are the oracle's,
    the next frame (the same one without the failing run) is clean"""
    from bonnie32_amd import rasterizer as R
    calls = fr.calls()
    want = RS.render_calls(oracle, [c for i, c in enumerate(calls) if i not in fr.error_run])
    fb = _new_fb(ctx)
    slots = RS.upload(fb, fr)
    try:
        for entry in ("begin", "submit"):
            with pytest.raises(R.B32Error) as e:
                RS.gpu_frame(ctx, fb, fr, slots, entry)
            assert e.value.code == code, (fr.name, entry, e.value.code)
            _same(fr, fb, want, f"{entry}: the run with the error undrawn, the others drawn")
            ctx.finish()                                         # (reported once)
            rest = RS.Frame(fr.name + "-rest", fr.family, fr.members, [d for i, d in enumerate(fr.draws) if i not in fr.error_run], fr.cell, fr.cell_tags)
            RS.gpu_frame(ctx, fb, rest, slots, entry)
            _same(rest, fb, want, f"{entry}: the next frame")
    finally:
        for rs in slots:
            rs.close()


@gpu
def test_vertex_index_equal_to_the_members_own_count_leaves_its_run_undrawn(gpu_ctx, oracle):
    """In merged space the index nv of a member is vertex 0 of the next member.  k_merge_mesh maps it to 0xFFFFFFFF, which k_setup's index check
    (load_face: before any vertex load) reports: B32_E_INDEX, the middle run undrawn, the runs before and after drawn (b32raster.h)."""
    _error_case(gpu_ctx, oracle, RS.frame("T-error"), abi.B32_E_INDEX)


@gpu
def test_two_nan_keyed_transparent_faces_in_the_last_member_leave_the_run_undrawn(gpu_ctx, oracle):
    _error_case(gpu_ctx, oracle, RS.frame("NaN-pair"), abi.B32_E_NAN_KEY)


@gpu
@pytest.mark.parametrize("kind", ["alone", "opaque"])
def test_nan_depths_that_no_sort_compares_draw_the_run(gpu_ctx, oracle, kind):
    """one transparent NaN face alone in its list; opaque NaN faces in two members (z-buffer mode never sorts them)"""
    fr = RS.frame(f"NaN-{kind}")
    fb = _new_fb(gpu_ctx)
    slots = _slots_of(gpu_ctx, fb, fr)
    for entry in ("begin", "submit"):
        RS.gpu_frame(gpu_ctx, fb, fr, slots, entry)
        _same(fr, fb, fr.oracle(oracle), f"{entry}")


@gpu
def test_slot_that_does_not_hold_its_scene_is_an_argument_error(gpu_ctx, oracle):
    """frame_end answers B32_E_ARG, and the context draws the next frame"""
    from bonnie32_amd import rasterizer as R
    fr = RS.frame("Z-runs")
    fb = _new_fb(gpu_ctx)
    slots = RS.upload(fb, fr)
    try:
        slots[2]._swap()                                         # the scene is in the context now, the slot holds what the context held
        fb.clear(RS.CLEAR)
        gpu_ctx.frame_begin(RS.CAM, fr.base)
        for d in fr.draws:
            gpu_ctx.frame_add(slots[d.member], ambient=d.ambient, backface_cull=d.cull)
        with pytest.raises(R.B32Error) as e:
            gpu_ctx.frame_end()
        assert e.value.code == abi.B32_E_ARG
        gpu_ctx.finish()
        slots[2]._swap()
        RS.gpu_frame(gpu_ctx, fb, fr, slots, "begin")
        _same(fr, fb, fr.oracle(oracle), "after the refused frame")
    finally:
        for rs in slots:
            rs.close()


@gpu
def test_finish_reports_the_counters_of_a_draw_that_the_swap_settled(gpu_ctx, oracle):
    """b32raster.h: "its counters are those of the most recent frame".  A draw that may need a redraw (here: x-ray, the ordered walk) is
    finished by the b32_scene_swap that puts its slot back; the finish that ends the frame still reports its triangle count, and a draw
    that follows replaces it."""
    fr = RS.frame("S-xray")
    o = fr.oracle(oracle)
    fb = _new_fb(gpu_ctx)
    slots = _slots_of(gpu_ctx, fb, fr)
    tm = RS.gpu_frame(gpu_ctx, fb, fr, slots, "begin")
    assert tm.triangles_drawn == o["drawn"][-1] != 0
    assert gpu_ctx.finish().triangles_drawn == 0                      # (nothing pending any more: reported once)
    merged = RS.frame("Z-two")
    tm = RS.gpu_frame(gpu_ctx, fb, merged, _slots_of(gpu_ctx, fb, merged), "begin")
    assert tm.triangles_drawn == sum(merged.oracle(oracle)["drawn"])


@gpu
def test_cache_of_merged_meshes_over_66_runs_in_deep_mode(oracle):
    """66 distinct two-member runs, one frame each, back to back in deep asynchronous mode, every frame delivered by ticket and compared.  The
    65th run evicts the first (the largest) and is built into its entry; run 1 again is a rebuild, run 66 again a hit; the members of run 1
    in the other order are another run, and the tie cell flips.  (Equality only: eviction is not timed.)"""
    from bonnie32_amd import rasterizer as R
    import __graft_entry__ as g
    g.build()
    members = RS.c_members()[0]
    pairs = RS.c_pairs()
    ctx = R.Context(0)
    ctx.set_async_depth(1)
    ctx.set_fragment_counting(0)
    fb = R.Framebuffer(RS.W, RS.H, ctx)
    slots = RS.upload(fb, RS.Frame("C", "C", members, [], 8, []))
    bufs = [ctx.host_alloc(RS.W * RS.H * 4) for _ in range(2)]
    try:
        pending = None

        def deliver():
            i, fr, ticket = pending
            ctx.ticket_wait(ticket)
            msg = fr.first_difference(bufs[i & 1][0], fr.oracle(oracle)["px"], f"run {i + 1} by ticket")
            assert not msg, msg

        def enqueue(i, a, b, swapped=False):
            fr = RS.family_c(a, b)
            if swapped:
                fr = RS.Frame(fr.name + "-swapped", "C", fr.members[::-1], [RS.Draw(0, fr.draws[1].ambient), RS.Draw(1, fr.draws[0].ambient)], fr.cell, fr.cell_tags)
            RS.gpu_frame(ctx, fb, fr, [slots[b], slots[a]] if swapped else [slots[a], slots[b]], "submit", finish=False)
            return i, fr, ctx.download_async(bufs[i & 1][1])
        for i, (a, b) in enumerate(pairs):
            nxt = enqueue(i, a, b)
            if pending:
                deliver()
            pending = nxt
        deliver()
        ctx.finish()
        assert ctx.batch_counts()["merged_built"] == 66 and ctx.batch_counts()["merged_draws"] == 66
        pending = enqueue(66, *pairs[0]); deliver(); ctx.finish()
        assert ctx.batch_counts()["merged_built"] == 67, "run 1 was evicted by the 65th run: drawing it again rebuilds it"
        pending = enqueue(67, *pairs[65]); deliver(); ctx.finish()
        assert ctx.batch_counts()["merged_built"] == 67, "run 66 is in the cache"
        straight = RS.family_c(*pairs[0]).oracle(oracle)
        pending = enqueue(68, *pairs[0], swapped=True); deliver(); ctx.finish()
        assert ctx.batch_counts()["merged_built"] == 68, "the same members in the other order are another run"
        fr = pending[1]
        assert [t for _, t in fr.changed_cells(straight, fr.oracle(oracle))] == ["C tie cell shared by every member"]
        _same(fr, fb, fr.oracle(oracle), "swapped members")
    finally:
        for _, p in bufs:
            ctx.host_free(p)
        ctx.close()
