"""The transparent pass fragment by fragment: order, batches, caps (tests/blend_stacks.py builds the sheets and the replay).

k_blend (csrc/b32_blend.hip) applies, per pixel, the fragments of the transparent pass in painter's order, each exactly once: a rank sort
of 64-bit priorities in LDS (GATHER, at most BLEND_SORT_CAP = 2048 entries), batches of 64 surfaces per tile, row and column candidate
masks, per-lane fragment lists of BLEND_LIST_CAP = 8 entries per round, a depth test that differs between plain and editor-alpha stores,
a running depth on the 8-bit path, the walk of both lists under x-ray.  On these sheets every one of those is a pixel of the frame.

MEASURED_PILE, the census of what the random pile scene sees (test_census_of_the_random_pile_scene; the scene of
tests/test_gpu_parity.py::test_transparent_pile_on_the_sort_free_path, painter's mode, rebuilt from the numpy model's tap and replayed to
the model's frame): 1500 faces, 756 drawn, 30 339 fragments on 25 071 covered pixels of 320 x 240 -- 1.21 fragments per covered pixel, at
most 5.  scenegen's `bbox_px` is the SQUARE of the mean bounding-box side: bbox_px = 120 gives triangles 11 pixels wide, not 120.  Dropping
a fragment changes the final pixel in 100 % of the 25 071 top fragments, 15.1 % of the 4678 fragments one below the top (708), 3.0 % of
the 542 two below (16), none of the 47 three below and not the one four below.  No tile list of that scene reaches a second batch of 64
and hardly a lane notes more than eight fragments: the scene does not test what its docstring names.  Its GPU run stays as it is (the
library's `fragments` there: see test_pile_scene_fragment_count).

The sheets (all 64 to 70 pixels wide, at most 208 rows, at most 400 faces but the cap sheets' 2057; a wider frame only for the taller cut
tiles) and the conditions that hold on them, all asserted below:
  * the C oracle and the numpy model agree on frame, z-buffer, fragment count and draw order, and the oracle's draw order is the one the
    key schedule intends (along, against, equal, permuted: four meshes, one frame); a replay of the tap's records reproduces the frame;
  * swapping any two layers that are adjacent in draw order changes the frame, on the ladder (at least 35 pixels) and on the window (33);
    dropping any layer changes it (at least 39 pixels on either); applying a layer twice leaves the frame unchanged exactly for the 40
    plain-store layers -- a store of the same value -- and changes the fragment count for every layer (MEASURED_MUTATIONS);
  * per tile of 64 rows with more than 64 entries: applying the 64-entry batches in reverse order and skipping every lane's 9th fragment
    of a batch each change the frame on every such tile of ladder, ladder70 and window; swapping entries 64 and 65 of the ordered list
    changes tile (0, 0) of the ladder (1 pixel) and of the window (13): layer 0 is a lone face, so the pair is the second face of layer
    32 and the first of layer 33.  PROVEN INVISIBLE (test_swaps_of_entries_64_and_65_that_no_frame_can_see): on the other tiles the
    two entries are either the two faces of one layer, whose fragments on their shared diagonal are equal, or lie under a later plain
    store on every pixel they share;
  * census of the ladder's tiles: pixel depths 1 .. 64 all occur on tile (0, 0) and every value between a tile's least and greatest depth
    on every tile (a ladder's lower tiles start deeper than 1); list lengths 95, 127, 191, 255, 287, 299, 383, 399: one in each of
    (64, 128], (128, 192], (192, 256] and three beyond.  Lanes: on a ladder every lane of every wave notes more than 8 fragments in every
    batch (100 to 528: a lane has 16 rows), so "a lane below 8 beside one above 8" does not occur on the 64 columns of tile column 0;
    what holds there is that the lanes of each wave differ in their totals and in their number of rounds (the columns 0..23 and 40..63
    miss every other odd layer) and that last rounds of every length 0..7 occur.  A total below 8 beside totals in the hundreds is
    ladder70's second tile column: 6 lanes work (each above 8 in every batch, asserted), 58 have no pixel.  The window's tiles (0, 1) and (0, 2) end in a batch of 10 entries in
    which a lane notes at most 8 fragments: exactly full lists beside shorter ones (test_census_of_the_window_tail);
  * cap sheets: exactly 2048 and 2049 transparent entries on the one tile, counted from the clipped boxes;
  * depth sheet: over the occluder at the layers' own depth 360 plain-mode and 402 editor-alpha fragments have the occluder's depth bit
    for bit and are rejected (`z < zb`, `!(z >= zb)`), 1266 are an ulp nearer and stored; none is stored over the nearer occluder.
NaN depths: a face with a NaN vertex depth has a NaN key, which the reference accepts only alone in its list.  "depth-nan-plain" and
"depth-nan-alpha" hold one such lone transparent face over the occluders: every fragment's depth is NaN, `z < zb` stores none of the
1282 fragments and `!(z >= zb)` stores all of them.

GPU cases, by kernel instantiation and route counter:
  k_blend<GATHER>   the sort-free path, RGB555 painter's and z-buffer mode: every ladder / window schedule, cap and depth sheet with
                    `inline_bin` (lists collected in the fill; its copy of the cap rule is plan_route's nf <= 2048: "cap2048-bare", 2048
                    faces, is the longest list that route can meet), `direct_bin` (k_setup's bin_span append, b32_setup.hip: position >=
                    cap_transparent raises Events::long_transparent; cap2048 fits, cap2049 redraws) and `counting_sort` (k_place_spans,
                    b32_sort.hip: longest_tr > blend_cap; the same two sheets.  k_bin_small's copy of the rule serves meshes of at most 2048
                    faces, where no list can be longer: it cannot fire).  With ROUTE_CUT_TILES off the tiles have 64 rows and the census
                    above is the kernel's; with it on these frames get 8-row tiles, and the ladder in a frame of ceil(n_cu / 13) or
                    ceil(n_cu / 7) tile columns gets 16- and 32-row tiles (plan_cut_grid, restated in _cut_tile_h with the device's count
                    of compute units; `inline_bin` moves, `keyed` does not).
  k_blend<>         keyed_ctx (`keyed`), RGB555: counting on -- global sort, ordered lists; counting off -- per-tile LDS sort of the whole
                    list (LOCAL_SORT_CAP = 2048 in tile_list_range, b32_fill.hip: "cap2048-bare" fits, cap2049 redraws); x-ray sheet
                    (`keyed`, ordered_all: the opaque list, then the transparent one)
  k_blend<FMT8>     depth8 (`keyed`, ordered_all, depth tile): in z-buffer mode the reference draws the 8-bit path's one list in face order
                    (it sorts in painter's mode only), every store writes the running depth and the later member of a crossing pair is
                    rejected on one side; in painter's mode the same sheet is ordered by mean depth
`fragments` is compared, and must not be 0, wherever the library counts stores exactly: fragment counting on in painter's mode, and always
under x-ray and on the 8-bit path (one case stores nothing by construction: the second z-buffer frame of depth8).  Measured on an MI355X:
with counting off, or in z-buffer mode on RGB555, these sheets report 0.  Every sheet but the cap sheets runs in every GPU test; the cap
sheets have their own; the cut-tile test takes the permuted ladder.

What a lost fragment does to these tests, to be redone by hand (b32_blend.hip, loop (A) of k_blend): let a lane go on when its list is
full and drop what it finds -- `can = n <= BLEND_LIST_CAP && ...`, `if (pass) { if (n < BLEND_LIST_CAP) mylist[...] = ...; ++n; }`, and
`n = min(n, BLEND_LIST_CAP)` in front of `nmax` -- so that the candidate a lane pops when it already holds 8 is lost.  Measured once: 56 of
the then 61 GPU tests of this module fail (first cell: ladder, pixel (0, 6), six layers deep);
test_transparent_pile_on_the_sort_free_path passes."""
import numpy as np
import pytest
import torch         # (here, before anything loads the HIP library of the package: imported behind it, torch finds no device)

from tests import blend_stacks as BS

gpu = pytest.mark.gpu
BIN_ROUTES = ("direct_bin", "inline_bin", "counting_sort", "keyed")

SHEETS = {f"ladder-{s}": (lambda s=s: BS.ladder(s)) for s in BS.SCHEDULES}
SHEETS.update({f"window-{s}": (lambda s=s: BS.window(s)) for s in BS.SCHEDULES})
SHEETS.update({"ladder70-along": lambda: BS.ladder("along", 70), "cap2048": lambda: BS.cap(0), "cap2049": lambda: BS.cap(1),
               "cap2048-bare": lambda: BS.cap(0, bare=True), "depth": BS.depth, "depth-nan-plain": lambda: BS.depth("plain"),
               "depth-nan-alpha": lambda: BS.depth("alpha"), "depth8": BS.depth8, "xray": BS.xray})
MUTATED = ("ladder-along", "window-along")
# least number of pixels an adjacent swap / a drop / a repeat of a blending layer changes, and the layers whose repeat changes nothing
MEASURED_MUTATIONS = {"ladder-along": dict(swap=35, drop=39, repeat=33), "window-along": dict(swap=33, drop=39, repeat=33)}
MEASURED_PILE = dict(fragments=30339, max_depth=5, by_distance=[(25071, 25071), (4678, 708), (542, 16), (47, 0), (1, 0)])


def _sheet(name):
    st = SHEETS[name]()
    assert st.name == name
    return st


# ------------------------------------------------------------------------------------------------ CPU: restatements and replay
@pytest.mark.parametrize("name", list(SHEETS))
def test_oracle_and_model_agree(oracle, name):
    st = _sheet(name)
    assert 64 <= st.width <= 70 and st.height <= 256
    o, m = st.oracle(oracle), st.model()
    BS.check_placement(st, m["res"])
    msg = st.first_difference(m["px"], o["px"], "numpy model against the C oracle")
    assert not msg, msg
    assert np.array_equal(m["zb"], o["zb"])
    assert m["res"]["fragments"] == o["tm"].fragments > 0
    assert m["res"]["triangles_drawn"] == o["tm"].triangles_drawn == st.n
    assert np.array_equal(m["res"]["draw_order"], o["dump"]["draw_order"])
    if st.schedule:
        assert np.array_equal(o["dump"]["draw_order"], st.intended_order()), f"{name}: the draw order is not the schedule's"
        assert np.array_equal(st.intended_order(), np.arange(st.n)) == (st.schedule in ("along", "equal"))


@pytest.mark.parametrize("kind", ["ladder", "window"])
def test_the_four_schedules_draw_one_frame(oracle, kind):
    want = _sheet(f"{kind}-along").oracle(oracle)
    for s in BS.SCHEDULES[1:]:
        o = _sheet(f"{kind}-{s}").oracle(oracle)
        assert np.array_equal(o["px"], want["px"]) and o["tm"].fragments == want["tm"].fragments, s


@pytest.mark.parametrize("name", list(SHEETS))
def test_replay_reproduces_the_frame(name):
    st = _sheet(name)
    m = st.model()
    rp = BS.replay_of(st)
    assert rp.fragments == m["res"]["fragments"]
    got = rp.frame().reshape(st.height, st.width, 3)
    msg = st.first_difference(got, m["px"][..., :3], "replay against the numpy model")
    assert not msg, msg


def test_census_of_the_random_pile_scene():
    """Task 0: what the random pile scene of test_gpu_parity.py lets a frame comparison see.  A measurement, recorded in the module
    docstring; asserted only so that the record cannot go stale."""
    c = BS.pile_census()
    assert c["frame_ok"], "the replay of the tap does not reproduce the model's frame"
    print(f"pile scene: {c['fragments']} fragments, {c['mean_depth']:.3f} per covered pixel, at most {c['max_depth']}; "
          f"(fragments, visible drops) by distance from the top: {c['by_distance']}")
    assert {k: c[k] for k in MEASURED_PILE} == MEASURED_PILE, (
        "the pile scene no longer measures what this module's docstring records (scenegen or the scene of test_gpu_parity.py changed?): "
        "nothing is wrong with the library; measure again and update MEASURED_PILE and the docstring")


# ------------------------------------------------------------------------------------------------ CPU: mutations of the replay
_MUT = {}


def _mutations(name):
    """per sheet: changed-pixel counts of every adjacent swap, drop and repeat -> dict(swap [n - 1], drop {k}, repeat {k}, frags {k})"""
    if name not in _MUT:
        st = _sheet(name)
        rp = BS.replay_of(st)
        runs = BS.layer_runs(st, rp)
        assert [k for k, _, _ in runs] == list(range(BS.N_LAYERS))
        swap = [rp.mutant(runs[i][1], runs[i + 1][2], list(range(runs[i + 1][1], runs[i + 1][2])) + list(range(runs[i][1], runs[i][2])))
                for i in range(len(runs) - 1)]
        drop = {k: rp.mutant(a, b, []) for k, a, b in runs}
        repeat = {k: rp.mutant(a, b, list(range(a, b)) * 2) for k, a, b in runs}
        frags = {k: sum(len(rp.recs[r]["pix"]) for r in range(a, b)) for k, a, b in runs}
        _MUT[name] = dict(swap=swap, drop=drop, repeat=repeat, frags=frags)
    return _MUT[name]


@pytest.mark.parametrize("name", MUTATED)
def test_no_swap_of_adjacent_layers_is_invisible(name):
    sw = _mutations(name)["swap"]
    assert len(sw) == BS.N_LAYERS - 1
    assert min(sw) == MEASURED_MUTATIONS[name]["swap"] > 0, [i for i, c in enumerate(sw) if c == 0]


@pytest.mark.parametrize("name", MUTATED)
def test_no_dropped_layer_is_invisible(name):
    dr = _mutations(name)["drop"]
    assert len(dr) == BS.N_LAYERS
    assert min(dr.values()) == MEASURED_MUTATIONS[name]["drop"] > 0, [k for k, c in dr.items() if c == 0]


@pytest.mark.parametrize("name", MUTATED)
def test_a_repeated_layer_is_invisible_only_as_a_plain_store(name):
    st, mu = _sheet(name), _mutations(name)
    plain = sorted(L.k for L in st.layers if L.plain)
    assert len(plain) == 40
    assert sorted(k for k, c in mu["repeat"].items() if c == 0) == plain
    assert min(c for c in mu["repeat"].values() if c) == MEASURED_MUTATIONS[name]["repeat"]
    assert all(mu["frags"][k] > 0 for k in range(BS.N_LAYERS))           # (a repeat adds the layer's fragments to the count)


def _full_tiles(st):
    return [(tx, ty) for ty in range(st.height // BS.TILE) for tx in range(-(-st.width // BS.TILE))]


TILE_SHEETS = ("ladder-along", "ladder70-along", "window-along")


@pytest.mark.parametrize("mut", ["reverse_batches", "skip_9th"])
@pytest.mark.parametrize("name", TILE_SHEETS)
def test_tile_mutation_changes_every_full_tile(name, mut):
    st = _sheet(name)
    rp = BS.replay_of(st)
    final = rp.frame()
    seen = 0
    for tx, ty in _full_tiles(st):
        base, n = BS.tile_walk(st, rp, tx, ty)
        assert np.array_equal(base, final[BS.tile_pixels(st, tx, ty)]), "the tile's walk in batches does not give the frame"
        if n <= BS.BATCH:
            continue
        got, _ = BS.tile_walk(st, rp, tx, ty, mut)
        assert (got != base).any(), (name, mut, tx, ty, n)
        seen += 1
    assert seen >= 3


def _swap_64_65(name):
    st = _sheet(name)
    rp = BS.replay_of(st)
    out = {}
    for tx, ty in _full_tiles(st):
        base, n = BS.tile_walk(st, rp, tx, ty)
        if n > 65:
            got, _ = BS.tile_walk(st, rp, tx, ty, "swap_64_65")
            out[(tx, ty)] = int((got != base).any(axis=1).sum())
    return st, rp, out


@pytest.mark.parametrize("name", ["ladder-along", "window-along"])
def test_swap_of_entries_64_and_65_changes_the_first_tile(name):
    st, rp, out = _swap_64_65(name)
    assert out[(0, 0)] > 0, out


@pytest.mark.parametrize("name", TILE_SHEETS)
def test_swaps_of_entries_64_and_65_that_no_frame_can_see(name):
    """Where the swap changes nothing, it cannot: on every pixel of the tile that both entries touch, either the two fragments are
    the same store (the two faces of one layer on their shared diagonal), or a later entry of the list is a plain store at alpha 255,
    which replaces whatever the pair left."""
    st, rp, out = _swap_64_65(name)
    order = [int(f) for f in st.model()["res"]["draw_order"]]
    proven = 0
    for (tx, ty), changed in out.items():
        if changed:
            continue
        entries = set(BS.tile_entries(st, tx, ty))
        lst = [f for f in order if f in entries]
        a, b = (rp.recs[rp.of_face[f]] for f in lst[64:66])
        shared = np.intersect1d(np.intersect1d(a["pix"], b["pix"]), BS.tile_pixels(st, tx, ty))
        ia, ib = np.searchsorted(a["pix"], shared), np.searchsorted(b["pix"], shared)
        same = (a["front"][ia] == b["front"][ib]).all(axis=1) & (a["flag"][ia] == b["flag"][ib]) & (a["mode"][ia] == b["mode"][ib]) & (a["alpha"][ia] == b["alpha"][ib])
        erased = np.zeros(len(shared), bool)
        for f in lst[66:]:
            r = rp.recs[rp.of_face[f]]
            stores = r["pix"][~r["flag"] & (r["alpha"] == 255)]
            erased |= np.isin(shared, stores)
        assert (same | erased).all(), (name, tx, ty)
        proven += 1
    assert proven == len([c for c in out.values() if c == 0])


# ------------------------------------------------------------------------------------------------ CPU: census
def _lane_totals(st, rp, order, tx, ty):
    """{(batch, wave): [columns of the tile inside the frame] fragments a lane notes in that batch}: a lane is column x of the rows w, w + 4, ..."""
    ent = set(BS.tile_entries(st, tx, ty))
    lst = [f for f in order if f in ent]
    out = {}
    for b in range(0, len(lst), BS.BATCH):
        cnt = np.zeros(st.width * st.height, np.int64)
        for f in lst[b:b + BS.BATCH]:
            cnt[rp.recs[rp.of_face[f]]["pix"]] += 1
        cnt = cnt.reshape(st.height, st.width)[ty * BS.TILE:(ty + 1) * BS.TILE, tx * BS.TILE:min((tx + 1) * BS.TILE, st.width)]
        for w in range(BS.WAVES):
            out[(b // BS.BATCH, w)] = cnt[w::BS.WAVES].sum(axis=0)
    return out


def test_census_of_the_ladder_tiles():
    lengths = []
    for name in ("ladder-along", "ladder70-along"):
        st = _sheet(name)
        rp = BS.replay_of(st)
        depth = np.zeros(st.width * st.height, np.int64)            # layers per pixel
        for k, a, b in BS.layer_runs(st, rp):
            depth[np.unique(np.concatenate([rp.recs[r]["pix"] for r in range(a, b)]))] += 1
        for ty in range(-(-st.height // BS.TILE)):
            for tx in range(-(-st.width // BS.TILE)):
                lengths.append(len(BS.tile_entries(st, tx, ty)))
                if (tx, ty) not in _full_tiles(st):
                    continue
                pix = BS.tile_pixels(st, tx, ty)
                d = depth[pix]
                assert set(range(int(d.min()), int(d.max()) + 1)) == set(d.tolist()), (name, tx, ty)
                if (tx, ty) == (0, 0):
                    assert d.min() == 1 and d.max() == 64
        order = [int(f) for f in st.model()["res"]["draw_order"]]
        for tx, ty in _full_tiles(st):
            totals = _lane_totals(st, rp, order, tx, ty)
            residues = set()
            for (batch, w), lane in totals.items():
                residues |= set((lane % BS.LIST_CAP).tolist())
                assert lane.min() > BS.LIST_CAP, (name, tx, ty, batch, w)           # every lane's list overflows, round after round
                if tx == 0:
                    assert len(set((-(-lane // BS.LIST_CAP)).tolist())) > 1, (name, tx, ty, batch, w)      # the lanes of the wave end in different rounds
            if tx == 0:
                assert residues == set(range(BS.LIST_CAP)), (name, tx, ty, residues)       # last rounds of every length, 8 included
            else:                                                            # six lanes work, 58 have no pixel: totals of 0 beside hundreds
                assert st.width - tx * BS.TILE == 6
                assert all(len(lane) == 6 and lane.min() > BS.LIST_CAP for lane in totals.values()), (name, tx, ty)
    assert sorted(set(lengths)) == [95, 127, 191, 255, 287, 299, 383, 399], sorted(set(lengths))
    for lo in (64, 128, 192):
        assert any(lo < n <= lo + 64 for n in lengths), lo


def test_census_of_the_window_tail():
    """the window's tiles (0, 1) and (0, 2) end in a batch of 10 entries: no lane notes more than 8 fragments, some exactly 8 -- lists that
    are exactly full, and shorter ones beside them, in one round"""
    st = _sheet("window-along")
    rp = BS.replay_of(st)
    order = [int(f) for f in st.model()["res"]["draw_order"]]
    for ty in (1, 2):
        totals = _lane_totals(st, rp, order, 0, ty)
        last = max(b for b, _ in totals)
        tail = np.concatenate([totals[(last, w)] for w in range(BS.WAVES)])
        assert last == 2 and tail.max() == BS.LIST_CAP and 0 < tail.min() < BS.LIST_CAP, (ty, tail.min(), tail.max())


def test_census_of_the_cap_sheets():
    for name, want in (("cap2048", 2048), ("cap2049", 2049), ("cap2048-bare", 2048)):
        st = _sheet(name)
        assert len(BS.tile_entries(st, 0, 0)) == want
        assert len(BS.tile_entries(st, 0, 0, transparent_only=False)) == st.n == want + (0 if name.endswith("bare") else 8)
        per_pixel = np.zeros(64 * 64, np.int64)
        for r in BS.replay_of(st).recs:
            per_pixel[r["pix"]] += 1
        assert per_pixel.max() <= 40                                 # small quads, not a deep pile: the length is in the list, not the pixel


def test_census_of_the_depth_sheets():
    st = _sheet("depth")
    m = st.model()
    zb = m["zb"].view(np.float32).reshape(64, 64)
    for lo, z in ((2, 45.0), (23, 65.0), (44, 85.0)):                 # the occluders' depths, to an ulp of the 1 / (sum of bc / z) they come from
        assert np.abs(zb[:, lo:lo + 19] - z).max() < 1e-4
    flat = {L.k for L in st.layers if L.transparent and np.ndim(L.z) == 0 and L.z == 60.0}
    stored = {"nearer": 0, "equal": 0, "farther": 0}
    kinds = set()
    for t in m["tap"]:
        k = int(st.layer_of_face[t["face"]])
        if k in flat:
            L = next(l for l in st.layers if l.k == k)
            kinds.add((L.plain, L.alpha < 255))
            for nm, lo in (("nearer", 2), ("equal", 23), ("farther", 44)):
                stored[nm] += int(((t["x"] >= lo) & (t["x"] < lo + 19)).sum())
    # (at the occluder's own depth the two interpolated depths differ by an ulp either way, pixel by pixel: some fragments pass)
    print("depth sheet, fragments stored over the nearer / equal / farther occluder:", stored)
    assert stored["nearer"] == 0 and 0 < stored["equal"] < stored["farther"], stored
    assert {(False, False), (False, True), (True, False), (True, True)} <= kinds      # blending / plain texels, each with and without editor alpha
    # the equal-depth case itself: fragments whose interpolated depth has the occluder's bits are rejected by `z < zb` and by `!(z >= zb)`
    # alike, their neighbours an ulp nearer are stored (a `<=` in either predicate would store the equal ones)
    FLT_MAX = np.float32(np.finfo(np.float32).max)
    equal = {False: 0, True: 0}                                       # by store kind: plain-mode stores, editor-alpha stores
    nearer_stored = 0
    stored_at = {int(t["face"]): set(zip(t["x"].tolist(), t["y"].tolist())) for t in m["tap"]}
    for fi in range(st.n):
        L = next(l for l in st.layers if l.k == int(st.layer_of_face[fi]))
        if L.k not in flat:
            continue
        zl = BS.face_depths(st, fi)
        ys, xs = np.nonzero((zl != FLT_MAX) & (np.arange(64)[None, :] >= 23) & (np.arange(64)[None, :] < 42))
        for x, y in zip(xs.tolist(), ys.tolist()):
            got = (x, y) in stored_at.get(fi, ())
            if zl[y, x].view(np.uint32) == zb[y, x].view(np.uint32):
                assert not got, (fi, x, y)
                equal[L.alpha < 255] += 1
            else:
                assert got == bool(zl[y, x] < zb[y, x]), (fi, x, y)
                nearer_stored += got
    print("depth sheet, middle band: fragments at exactly the occluder's depth (plain, alpha):", equal, "stored an ulp nearer:", nearer_stored)
    assert equal[False] > 0 and equal[True] > 0 and nearer_stored == stored["equal"]
    sloped = [t for t in m["tap"] if np.ndim(next(l for l in st.layers if l.k == int(st.layer_of_face[t["face"]])).z)]
    assert sloped and all(0 < len(t["x"]) for t in sloped)
    # NaN depths: the two store predicates part
    plain, alpha = _sheet("depth-nan-plain"), _sheet("depth-nan-alpha")
    lone = [t for t in alpha.model()["tap"] if alpha.layer_of_face[t["face"]] == 3]
    assert len(lone) == 1 and len(lone[0]["x"]) == 1282
    assert all(plain.layer_of_face[t["face"]] != 3 for t in plain.model()["tap"])
    # the 8-bit pairs: the later member of the draw order is rejected on part of the quad, and depth was written by the earlier one
    d8 = _sheet("depth8")
    m8 = d8.model()
    order = [int(d8.layer_of_face[f]) for f in m8["res"]["draw_order"]]
    frag = {}
    for t in m8["tap"]:
        frag[int(d8.layer_of_face[t["face"]])] = frag.get(int(d8.layer_of_face[t["face"]]), 0) + len(t["x"])
    partial = 0
    for k in range(1, 21, 2):
        first, second = sorted((k, k + 1), key=order.index)
        partial += 0 < frag.get(second, 0) < frag[first]
    assert partial == 10, partial
    assert np.array_equal(order, sorted(order))                      # face order: the reference sorts the 8-bit path's one list in painter's mode only


# ------------------------------------------------------------------------------------------------ GPU
def _same(st, got, want, what):
    msg = st.first_difference(got, want, what)
    assert not msg, msg


def _counts_exactly(st, counting, kw):
    """where the library's `fragments` is the reference's store count"""
    zb = st.zbuffer if kw.get("zbuffer") is None else kw["zbuffer"]
    return st.xray or st.fmt8 or (counting and not zb)


def _check(ctx, st, oracle, what, fb, tm, counting, frames=1, stores_nothing=False, **kw):
    """stores_nothing: the one case whose exact store count is 0 by construction (the caller asserts that of the oracle)"""
    o = st.oracle(oracle, frames=frames, **kw)
    tag = f"{what}, counting={counting}, {kw}"
    _same(st, fb.pixels, o["px"], tag)
    if st.settings(**kw).use_zbuffer:
        _same(st, fb.zbuffer.view(np.uint32), o["zb"], tag + ", depths")
    assert tm.triangles_drawn == o["tm"].triangles_drawn, tag
    assert np.array_equal(ctx.last_draw_order(st.n), o["dump"]["draw_order"]), f"[{st.name} {tag}] draw order differs from the oracle's"
    print(f"[{st.name} {tag}] fragments: library {tm.fragments}, oracle {o['tm'].fragments}")
    if _counts_exactly(st, counting, kw):
        assert tm.fragments == o["tm"].fragments, tag
        assert (tm.fragments == 0) == stores_nothing, tag


def _expected_route(st, off, C):
    if st.xray or st.fmt8 or off & C.ROUTE_SORT_FREE:
        return "keyed"
    if st.n <= 2048 and not off & C.ROUTE_INLINE_BIN:
        return "inline_bin"
    return "counting_sort" if off & C.ROUTE_DIRECT_BIN else "direct_bin"


def _route_masks(C):
    return (0, C.ROUTE_INLINE_BIN, C.ROUTE_INLINE_BIN | C.ROUTE_DIRECT_BIN)


PLAIN_SHEETS = [n for n in SHEETS if not n.startswith("cap")]


@gpu
@pytest.mark.parametrize("name", PLAIN_SHEETS)
def test_stack_on_every_binning_route(gpu_ctx, oracle, name):
    """in-fill list collection, k_setup's direct binning and the counting-sort launches, each on 64-row tiles (ROUTE_CUT_TILES off: the
    census of the CPU tests is the kernel's) and on the cut tiles these small frames get by default, fragment counting off and on,
    resident; the counter of the intended route, and of no other, moves (x-ray and the 8-bit path: the keyed pipeline, whatever is off)"""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    st = _sheet(name)
    try:
        for off in _route_masks(C)[:1 if (st.xray or st.fmt8) else 3]:
            for cut in (C.ROUTE_CUT_TILES, 0):
                for counting in (0, 1):
                    gpu_ctx.set_fragment_counting(counting)
                    gpu_ctx.set_routes(off | cut)
                    before = gpu_ctx.route_counts()
                    fb, tm = BS.gpu_draw(gpu_ctx, st, resident=True)
                    after = gpu_ctx.route_counts()
                    _check(gpu_ctx, st, oracle, f"routes off: {off | cut}", fb, tm, counting)
                    moved = sorted(k for k in BIN_ROUTES if after[k] != before[k])
                    assert moved == [_expected_route(st, off, C)], (name, off, cut, counting, moved)
                    assert after["redraw_global_sort"] == before["redraw_global_sort"]
    finally:
        gpu_ctx.set_routes(0)
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", PLAIN_SHEETS)
def test_stack_per_call_resident_and_in_both_depth_modes(gpu_ctx, oracle, name):
    """drop-in and resident, painter's and z-buffer mode (the ladder's transparent pass tests against, and never writes, the cleared
    depths), counting on and off"""
    st = _sheet(name)
    try:
        for zbuffer in (False, True):
            for counting in (1, 0):
                gpu_ctx.set_fragment_counting(counting)
                for resident in (False, True):
                    fb, tm = BS.gpu_draw(gpu_ctx, st, resident=resident, zbuffer=zbuffer)
                    _check(gpu_ctx, st, oracle, f"resident={resident}", fb, tm, counting, zbuffer=zbuffer)
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", PLAIN_SHEETS)
def test_stack_through_the_keyed_context(keyed_ctx, oracle, name):
    """the sort-free path off from the start: global painter's sort with counting on, per-tile LDS sort with it off; k_blend without GATHER"""
    st = _sheet(name)
    try:
        for counting in (1, 0):
            keyed_ctx.set_fragment_counting(counting)
            before = keyed_ctx.route_counts()
            fb, tm = BS.gpu_draw(keyed_ctx, st, resident=True)
            after = keyed_ctx.route_counts()
            _check(keyed_ctx, st, oracle, "keyed context", fb, tm, counting)
            assert sorted(k for k in BIN_ROUTES if after[k] != before[k]) == ["keyed"]
    finally:
        keyed_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", PLAIN_SHEETS)
def test_stack_in_two_ragged_row_bands(gpu_ctx, oracle, name):
    """bands (0, 37) and (37, H): the cut is no multiple of 8 and runs through the layers.  The pixel rows and, on the z-buffer sheets, the
    depth rows of the two partial frames assemble to the oracle's (the 8-bit path writes its depth tile back per band: nothing outside the
    band, nothing stale inside); either band reports the whole draw order and triangle count, and where the library counts stores
    exactly the two bands' `fragments` add up to the oracle's"""
    st = _sheet(name)
    o = st.oracle(oracle)
    row = st.width * 4
    untouched = np.float32(np.finfo(np.float32).max).view(np.uint32)
    try:
        for counting in (0, 1):
            gpu_ctx.set_fragment_counting(counting)
            assembled = np.zeros(st.width * st.height * 4, np.uint8)
            depths = np.zeros(st.width * st.height, np.uint32)
            fragments = 0
            for y0, y1 in ((0, 37), (37, st.height)):
                fb, tm = BS.gpu_draw(gpu_ctx, st, resident=True, band=(y0, y1))
                assembled[y0 * row:y1 * row] = fb.pixels[y0 * row:y1 * row]
                zb = fb.zbuffer.view(np.uint32)
                depths[y0 * st.width:y1 * st.width] = zb[y0 * st.width:y1 * st.width]
                if st.zbuffer:
                    outside = np.concatenate([zb[:y0 * st.width], zb[y1 * st.width:]])
                    assert (outside == untouched).all(), f"[{name} band ({y0}, {y1}) counting={counting}] depth written outside the band"
                assert tm.triangles_drawn == o["tm"].triangles_drawn
                assert np.array_equal(gpu_ctx.last_draw_order(st.n), o["dump"]["draw_order"]), f"[{name} band ({y0}, {y1})] draw order differs from the oracle's"
                fragments += tm.fragments
            _same(st, assembled, o["px"], f"bands counting={counting}")
            if st.zbuffer:
                _same(st, depths, o["zb"], f"bands counting={counting}, depths")
            print(f"[{name} bands counting={counting}] fragments: library {fragments}, oracle {o['tm'].fragments}")
            if _counts_exactly(st, counting, {}):
                assert fragments == o["tm"].fragments != 0, (name, counting)
    finally:
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name", PLAIN_SHEETS)
def test_stack_two_frames_back_to_back(gpu_ctx, oracle, name):
    """the same resident scene drawn twice onto one framebuffer, in the sheet's own mode: the second frame blends over the first; nothing
    of the first frame's lists, ranks or masks may be left behind.  The 8-bit sheet runs twice.  In painter's mode its second frame blends
    again.  In z-buffer mode the depths the first frame wrote reject every fragment of the second (the oracle counts 0 stores, asserted):
    frame and depth bits must stay as the first frame left them."""
    st = _sheet(name)
    try:
        for counting in (1, 0):
            gpu_ctx.set_fragment_counting(counting)
            for kw in ([{"zbuffer": False}, {"zbuffer": True}] if st.fmt8 else [{}]):
                fb, tm = BS.gpu_draw(gpu_ctx, st, frames=2, **kw)
                if st.fmt8 and kw["zbuffer"]:
                    o1, o2 = st.oracle(oracle, **kw), st.oracle(oracle, frames=2, **kw)
                    assert o2["tm"].fragments == 0 and np.array_equal(o1["px"], o2["px"]) and np.array_equal(o1["zb"], o2["zb"])
                    _check(gpu_ctx, st, oracle, "second frame", fb, tm, counting, frames=2, stores_nothing=True, **kw)
                else:
                    _check(gpu_ctx, st, oracle, "second frame", fb, tm, counting, frames=2, **kw)
    finally:
        gpu_ctx.set_fragment_counting(1)


def _cut_tile_h(tiles_x, rows, n_cu):
    """plan_cut_grid (csrc/b32_frame_plan.h) for a whole frame of `rows` rows"""
    th = 64
    while th > 8 and tiles_x * -(-rows // th) < (2 if th == 64 else 1) * n_cu and rows // (th // 2) + 2 <= 255:
        th //= 2
    return th


@gpu
@pytest.mark.parametrize("want_h", [8, 16, 32])
def test_ladder_on_cut_tiles(gpu_ctx, oracle, want_h):
    """The sort-free path cuts the tiles of a frame that has too few of them for the device's compute units: 8 rows on the 64-pixel
    sheets; the same ladder at the left of a frame of ceil(n_cu / 13) or ceil(n_cu / 7) tile columns (20 or 37 on an MI355X) keeps 16
    or 32 rows (plan_cut_grid, restated above and fed with the device's own count).  TH < 64: the `rows` mask of a lane has 2, 4 or 8
    bits, the tile's list holds the layers of its rows only.  The frame takes the in-fill list collection of the sort-free path
    (`inline_bin` moves; `keyed`, which never cuts tiles, and `redraw_global_sort` do not).  Frame only."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count        # (the library reads the same count and has no accessor for it)
    rows = BS.N_LAYERS + 8
    tiles_x = {8: 1, 16: -(-n_cu // 13), 32: -(-n_cu // 7)}[want_h]
    assert _cut_tile_h(tiles_x, rows, n_cu) == want_h, (tiles_x, n_cu)
    st = BS.ladder("permuted", 64, None if want_h == 8 else 64 * tiles_x)
    try:
        for counting in (0, 1):
            gpu_ctx.set_fragment_counting(counting)
            before = gpu_ctx.route_counts()
            fb, tm = BS.gpu_draw(gpu_ctx, st, resident=True)
            after = gpu_ctx.route_counts()
            _same(st, fb.pixels, st.oracle(oracle)["px"], f"{want_h}-row tiles, counting={counting}")
            moved = sorted(k for k in BIN_ROUTES + ("redraw_global_sort", "redraw_region", "redraw_pairs") if after[k] != before[k])
            assert moved == ["inline_bin"], (want_h, counting, moved)
    finally:
        gpu_ctx.set_fragment_counting(1)


def _cap_case(ctx, oracle, name, redraws, route, counting):
    """a fresh upload (local_sort_ok sticks to a scene), two frames of it: -> the route counters' movement over the first frame"""
    from bonnie32_amd import rasterizer as R
    st = _sheet(name)
    ctx.set_fragment_counting(counting)
    fb = R.Framebuffer(st.width, st.height, ctx)
    fb.upload(st.back)
    rs = R.ResidentScene(fb, st.vertices, st.faces, st.textures)
    before = ctx.route_counts()
    tm = rs.render(BS.Camera(), st.settings())
    mid = ctx.route_counts()
    _check(ctx, st, oracle, f"cap on {route}", fb, tm, counting)
    assert mid["redraw_global_sort"] - before["redraw_global_sort"] == redraws, (name, route, counting)
    assert mid[route] > before[route], (name, route, {k: mid[k] - before[k] for k in BIN_ROUTES})
    if not redraws and route != "keyed":
        assert mid["keyed"] == before["keyed"], (name, route)
    tm = rs.render(BS.Camera(), st.settings())
    after = ctx.route_counts()
    _check(ctx, st, oracle, f"cap on {route}, second frame", fb, tm, counting, frames=2)
    assert after["redraw_global_sort"] == mid["redraw_global_sort"], (name, route, "the second frame was redrawn again")


@gpu
@pytest.mark.parametrize("name,redraws", [("cap2048", 0), ("cap2049", 1), ("cap2048-bare", 0)])
def test_cap_of_the_rank_sort_on_the_sort_free_routes(gpu_ctx, oracle, name, redraws):
    """2048 transparent entries on one tile are ranked in LDS (the sort buffer fills the colour tile's 16 KB to the byte), 2049 redraw the
    frame once with the global sort, and the scene's next frame goes there directly.  direct_bin: bin_span's `pos < cap` (b32_setup.hip);
    counting_sort: k_place_spans' `longest_tr > blend_cap` (b32_sort.hip); inline_bin: reachable with at most 2048 faces only (plan_route)"""
    from bonnie32_amd import rasterizer as R
    C = R.Context
    try:
        for off in _route_masks(C):
            route = _expected_route(_sheet(name), off, C)
            if name == "cap2048-bare" and route != "inline_bin":
                continue
            gpu_ctx.set_routes(off | C.ROUTE_CUT_TILES)          # one 64 x 64 tile: all 2048 / 2049 entries in one list
            _cap_case(gpu_ctx, oracle, name, redraws, route, counting=0)
            _cap_case(gpu_ctx, oracle, name, redraws, route, counting=1)
    finally:
        gpu_ctx.set_routes(0)
        gpu_ctx.set_fragment_counting(1)


@gpu
@pytest.mark.parametrize("name,redraws", [("cap2048-bare", 0), ("cap2049", 1)])
def test_cap_of_the_local_sort_in_the_keyed_context(keyed_ctx, oracle, name, redraws):
    """counting off: the keyed pipeline sorts a tile's whole list in LDS (LOCAL_SORT_CAP = 2048, tile_list_range in b32_fill.hip): 2048
    faces fit, 2057 redraw once with the global sort; counting on: the global sort from the start, never a redraw"""
    try:
        _cap_case(keyed_ctx, oracle, name, redraws, "keyed", counting=0)
        _cap_case(keyed_ctx, oracle, name, 0, "keyed", counting=1)
    finally:
        keyed_ctx.set_fragment_counting(1)


@gpu
def test_pile_scene_fragment_count(gpu_ctx, oracle):
    """The two pile tests of test_gpu_parity.py run with fragment counting off (fast_ctx).  What the library reports as `fragments` for
    the pile scene there, and with counting on, against the oracle's 30 339.  Measured: 30 339 both ways in painter's mode (resident or not), 0 in
    z-buffer mode; test_fast_path_transparent_lists: 0 for its C5 scene in either mode, the oracle's 458 921 for its redrawn scene.  The two
    existing tests now compare the count where it is exact and not 0."""
    from bonnie32_amd import rasterizer as R
    sc = BS.pile_scene()
    ofb = oracle.Framebuffer(sc.width, sc.height); ofb.clear(sc.clear_color)
    rc, etm = oracle.render_mesh_15(ofb, sc.vertices, sc.faces, sc.textures, sc.camera, sc.settings)
    assert rc == 0 and etm.fragments == MEASURED_PILE["fragments"]
    try:
        got = {}
        for counting in (0, 1):
            gpu_ctx.set_fragment_counting(counting)
            fb = R.Framebuffer(sc.width, sc.height, gpu_ctx); fb.clear(sc.clear_color)
            tm = R.ResidentScene(fb, sc.vertices, sc.faces, sc.textures).render(sc.camera, sc.settings)
            assert np.array_equal(fb.pixels, ofb.pixels)
            got[counting] = tm.fragments
        print(f"pile scene fragments: counting off {got[0]}, counting on {got[1]}, oracle {etm.fragments}")
        assert got[1] == etm.fragments
    finally:
        gpu_ctx.set_fragment_counting(1)
