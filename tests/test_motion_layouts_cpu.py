"""The layouts of tests/motion_layouts.py on the host: (1) for every layout and every frame the oracle tracker, orc.segment_motion on
the computed history and py_segment give the same list; (2) every layout is in the regime it is named for -- the facts come from
tile_model and are asserted as numbers, so that tests/test_gpu_motion_layouts.py cannot pass on an empty or degenerate case."""
import numpy as np
import pytest

import motion_layouts as M


def _area_ok(boxes, params):
    a = boxes[:, 2].astype(np.int64) * boxes[:, 3]
    return boxes[(a > params["min_area"]) & (a < params["max_area"])]


@pytest.mark.parametrize("name", M.NAMES)
def test_three_statements_agree(name):
    """orc.Tracker.process on the painted frames == orc.segment_motion on history() == py_segment on history(), frame by frame; with
    distance 0 __join_objects only applies the area window"""
    import orc
    age, K, tss, params = M.LAYOUTS[name]
    assert params["distance"] == 0
    exp = M.expected(name)
    assert len(exp) == K + 1 and len(exp[0]) == 0
    for k in range(1, K + 1):
        mhi = M.history(age, tss, k, params["mhi_duration"])
        seg = orc.segment_motion(mhi.copy(), tss[k], params["seg_thresh"], cap=1 << 16)
        mine = M.py_segment(mhi, tss[k], params["seg_thresh"])
        assert np.array_equal(seg, mine), (name, k, len(seg), len(mine))
        assert np.array_equal(exp[k], _area_ok(mine, params)), (name, k, len(exp[k]), len(mine))
        if tss[k] == 0.0:
            assert len(exp[k]) == 0 and (age == k).any(), (name, k)
        else:
            assert len(exp[k]) >= 1, (name, k)


def test_history_expiry_edge():
    """a value equal to float32(ts - duration) stays, the next smaller float32 goes"""
    age = np.array([[1, 2, 3]], np.uint8)
    tss = (0.0, 1000.0, 1032.0, 1096.0)
    assert M.history(age, tss, 3, 64.0).tolist() == [[0.0, 1032.0, 1096.0]]
    assert M.history(age, tss, 3, 64.0 + 1e-3).tolist() == [[0.0, 1032.0, 1096.0]]          # float32(1031.999) is below 1032
    assert M.history(age, tss, 3, 96.0).tolist() == [[1000.0, 1032.0, 1096.0]]
    fr = M.paint(age, 3)
    assert [f[0, :, 0].tolist() for f in fr] == [[0, 0, 0], [255, 0, 0], [255, 255, 0], [255, 255, 255]]
    assert all((f[..., 3] == 255).all() for f in fr)


def _last(name):
    return M.model(name, M.LAYOUTS[name][1])


@pytest.mark.parametrize("name", ["serpentine", "serpentine@513x49"])
def test_serpentine_spans_every_tile(name):
    m = M.model(name, 1)
    assert len(m["components"]) == 1
    assert m["components"][0]["tiles"] == set(range(m["ntx"] * m["nty"])) and m["ntx"] == 3 and m["nty"] == 7
    assert (m["tile_roots"] >= 1).all()


@pytest.mark.parametrize("name", ["spirals", "spirals@513x49"])
def test_spirals_are_two_nested_components(name):
    m = M.model(name, 1)
    w, h = M.size(name)
    assert len(m["components"]) == 2
    assert M.expected(name)[1].tolist() == [[0, 0, w, h], [2, 2, w - 4, h - 4]]
    # the outer one spans every tile, the inner one every tile its box meets
    assert sorted(len(c["tiles"]) for c in m["components"]) == [((w - 3) // 256 + 1) * ((h - 3) // 8 + 1), m["ntx"] * m["nty"]]


@pytest.mark.parametrize("name,teeth,tile_roots,seed_tile", [("comb", 260, 6 * 260 + 3, 20), ("comb@513x49", 257, 5 * 257 + 3, 17),
                                                            ("comb_up", 260, 6 * 260 + 3, 20), ("comb_up@513x49", 257, 5 * 257 + 3, 17)])
def test_combs_fold_hundreds_of_tile_roots_and_seed_far_from_the_root(name, teeth, tile_roots, seed_tile):
    """a tooth is a tile root in every tile row it reaches but the spine's, which holds one root per tile (520 x 50: rows 1 .. 48, seven
    tile rows; 513 x 49: rows 1 .. 47, six)"""
    w, h = M.size(name)
    m1, m = M.model(name, 1), M.model(name, 2)
    # frame 1: at 513 x 49 the comb's last tooth hangs on the spine's missing end: a component of its own that the seed of frame 2 joins
    assert len(m1["components"]) == (2 if name == "comb@513x49" else 1), name
    assert tile_roots - 1 <= int(m1["tile_roots"].sum()) <= tile_roots
    assert len(m["components"]) == 1, name
    c = m["components"][0]
    assert c["local_roots"] == tile_roots == int(m["tile_roots"].sum()), (name, c["local_roots"])
    assert tile_roots < M.roots_cap(w, h)
    assert c["root_tile"] == 0 and c["seed_tile"] == seed_tile and c["seed_tile"] != c["root_tile"]
    assert int(M._seeds(M.history(*_hist_args(name, 2)), M.LAYOUTS[name][2][2]).sum()) == 1
    assert M.expected(name)[2].tolist() == [[0, 1, w, h - 2]]


def _hist_args(name, k):
    age, K, tss, params = M.LAYOUTS[name]
    return age, tss, k, params["mhi_duration"]


@pytest.mark.parametrize("name", ["unseeded_neighbours", "unseeded_neighbours@513x49"])
def test_unseeded_components_touch_seeded_ones(name):
    m = _last(name)
    lab = m["label"]
    seeded = {c["root"] for c in m["components"] if c["seed"] is not None}
    unseeded = {c["root"] for c in m["components"] if c["seed"] is None}
    assert len(seeded) >= 20 and len(unseeded) >= 10
    touching = set()
    for a, b in ((lab[:, 1:], lab[:, :-1]), (lab[1:, :], lab[:-1, :])):
        for x, y in ((a, b), (b, a)):
            hit = np.isin(x, list(unseeded)) & np.isin(y, list(seeded))
            touching |= set(x[hit].tolist())
    assert len(touching) >= 10, len(touching)
    # ... and the blobs 32 older lend their extent: some seeded component reaches beyond its own seeds
    age, K, tss, params = M.LAYOUTS[name]
    grown = sum(1 for c in m["components"] if c["seed"] is not None and (age[lab == c["root"]] == 2).any())
    assert grown >= 10, grown


@pytest.mark.parametrize("name", ["chain_of_ages", "chain_of_ages@513x49"])
def test_chains_join_stepwise_and_cross_every_boundary(name):
    age, K, tss, params = M.LAYOUTS[name]
    m = _last(name)
    mhi = M.history(*_hist_args(name, K))
    lab = m["label"]
    # components that hold all four ages although their ends do not join each other
    full = [c for c in m["components"] if set(np.unique(age[lab == c["root"]]).tolist()) == {1, 2, 3, 4}]
    assert len(full) >= 20, len(full)
    assert not M._joined(np.float32([tss[4]]), np.float32([tss[1]]), params["seg_thresh"])[0]
    # links between different ages across a wave boundary, a tile's left column and a tile's top row
    differ_h = M._joined(mhi[:, 1:], mhi[:, :-1], 32.0) & (mhi[:, 1:] != mhi[:, :-1])
    differ_v = M._joined(mhi[1:, :], mhi[:-1, :], 32.0) & (mhi[1:, :] != mhi[:-1, :])
    xs = np.arange(1, mhi.shape[1])
    assert differ_h[:, xs % 256 == 0].sum() >= 6 and differ_h[:, (xs % 64 == 0) & (xs % 256 != 0)].sum() >= 6
    assert differ_v[np.arange(1, mhi.shape[0]) % 8 == 0, :].sum() >= 6


def test_every_2x2_pattern_in_every_position():
    """interior: no pixel pair of the pattern straddles a wave boundary, a tile column or a tile row"""
    seen = {k: set() for k in ("interior", "wave", "tile_column", "tile_row")}
    for c in range(M.PAT_COPIES):
        age = M.LAYOUTS["patterns_2x2/%d@%dx%d" % (c, M.PAT_W, M.PAT_H)][0]
        for p, (x, y) in enumerate(M.pattern_origins(c).tolist()):
            assert 0 <= x and x + 2 <= M.PAT_W and 0 <= y and y + 2 <= M.PAT_H
            assert np.array_equal(age[y:y + 2, x:x + 2], M.PALETTE_AGE[M.pattern_cells(p)])
            assert not age[max(y - 1, 0):y + 3, max(x - 1, 0):x + 3].sum() - age[y:y + 2, x:x + 2].sum(), "patterns touch"
            if x % 256 == 255: seen["tile_column"].add(p)
            elif x % 64 == 63: seen["wave"].add(p)
            if y % 8 == 7: seen["tile_row"].add(p)
            if x % 64 != 63 and y % 8 != 7: seen["interior"].add(p)
    assert {k: len(v) for k, v in seen.items()} == dict(interior=625, wave=625, tile_column=625, tile_row=625)
    assert len({tuple(M.pattern_cells(p).reshape(-1).tolist()) for p in range(625)}) == 625


def test_tied_rule_holds_and_fails_inside_tiles_and_on_top_rows():
    """over the random fields and the 2 x 2 patterns: among the pixels joined to the one above, the rule applies to some and not to
    others, in tile interiors and on tiles' top rows (k_ccl_border), and at a tile's first column only on a top row"""
    cnt = dict(in_tied=0, in_not=0, top_tied=0, top_not=0, top_tied_col0=0)
    for name in M.NAMES:
        if not name.startswith(("random_fields", "patterns_2x2")):
            continue
        m = _last(name)
        h, w = m["vu"].shape
        top = (np.arange(h) % 8 == 0)[:, None] & np.ones((1, w), bool)
        col0 = (np.arange(w) % 256 == 0)[None, :] & np.ones((h, 1), bool)
        vu, tied = m["vu"], m["tied"]
        assert not (tied & ~vu).any() and not (tied & col0 & ~top).any() and not tied[:, 0].any()
        cnt["in_tied"] += int((vu & tied & ~top).sum()); cnt["in_not"] += int((vu & ~tied & ~top).sum())
        cnt["top_tied"] += int((vu & tied & top).sum()); cnt["top_not"] += int((vu & ~tied & top).sum())
        cnt["top_tied_col0"] += int((vu & tied & top & col0).sum())
    assert all(v >= 10 for v in cnt.values()), cnt


def test_random_fields_sizes_and_regimes():
    sizes = {M.size(n) for n in M.NAMES if n.startswith("random_fields")}
    assert sizes == {(5, 3), (64, 8), (256, 8), (257, 9), (513, 49), (520, 50)}
    m = _last("random_fields/1")
    assert (m["label"] >= 0).all()
    # the relation is not transitive and the fields show it: one component holds values further apart than seg_thresh
    mhi = M.history(*_hist_args("random_fields/1", 4))
    big = max(m["components"], key=lambda c: len(c["tiles"]))
    vals = mhi[m["label"] == big["root"]]
    assert vals.max() - vals.min() == 60.0 and len(big["tiles"]) == 21


def test_random_fields_lie_on_both_sides_of_the_root_list():
    """tile roots of the 520 x 50 fields after frames 1 .. 4 against the 3250 entries of a single slot's list: alone, each field is
    answered by the folded path on some frames and by the fallback on others; eight slots together (26 000 entries) always fit"""
    roots = {d: [int(M.model("random_fields/" + d, k)["tile_roots"].sum()) for k in (1, 2, 3, 4)] for d in ("0.35", "0.7", "1")}
    assert roots == {"0.35": [1845, 2998, 4185, 5430], "0.7": [3070, 3511, 4122, 4722], "1": [3479, 2406, 1924, 1758]}
    assert all(min(r) <= M.roots_cap(520, 50) < max(r) for r in roots.values())
    assert sum(max(r) for r in roots.values()) + 5 * 1563 < M.roots_cap(520, 50, 8)


def test_expiring_component_loses_parts_and_tiles_die_beside_live_ones():
    age, K, tss, params = M.LAYOUTS["expiring"]
    live_tiles = []
    for k in range(1, K + 1):
        mhi = M.history(age, tss, k, params["mhi_duration"])
        assert sorted(np.unique(age[mhi != 0]).tolist()) == [j for j in (k - 2, k - 1, k) if j >= 1], k
        if k >= 3:
            assert (mhi[age == k - 2] == np.float32(tss[k] - params["mhi_duration"])).all()       # exactly on the bound: stays
        live_tiles.append(M.model("expiring", k)["tile_roots"] > 0)
    died = [(a & ~b) for a, b in zip(live_tiles, live_tiles[1:])]
    assert sum(int(d.sum()) for d in died) >= 4
    # a tile that died lies beside one that lives (same tile row, neighbouring column)
    assert any((d[:, :-1] & l[:, 1:]).any() or (d[:, 1:] & l[:, :-1]).any() for d, l in zip(died, live_tiles[1:]))


@pytest.mark.parametrize("name", ["seg_edge", "seg_edge_2p24", "seg_edge@513x49", "seg_edge_2p24@513x49"])
def test_seg_edge_values(name):
    age, K, tss, params = M.LAYOUTS[name]
    f = [np.float32(t) for t in tss]
    assert all(float(x) == t for x, t in zip(f, tss))          # every timestamp is a float32
    assert f[3] - f[2] == 32.0 and f[2] - f[1] in (32.5, 34.0)
    if tss[0] >= 1 << 24:
        assert np.nextafter(f[1], np.float32(np.inf)) - f[1] == 2.0
    m = _last(name)
    lab = m["label"]
    for c in m["components"]:
        ages = set(np.unique(age[lab == c["root"]]).tolist())
        assert ages in ({1}, {2, 3}), ages
    assert sum(1 for c in m["components"] if c["seed"] is not None) >= 8


@pytest.mark.parametrize("name", ["clock_oddities", "clock_oddities@513x49"])
def test_clock_oddities_script(name):
    age, K, tss, params = M.LAYOUTS[name]
    assert tss[2] == tss[1] and tss[3] < tss[2] and tss[4] == 0.0 and tss[5] > tss[3]
    s2 = M._seeds(M.history(*_hist_args(name, 2)), tss[2])
    assert (s2 & (age == 1)).any() and (s2 & (age == 2)).any()             # the previous frame's pixels are seeds too
    mhi4 = M.history(*_hist_args(name, 4))
    assert (mhi4[age == 4] == 0).all() and (mhi4 != 0).any() and not M._seeds(mhi4, 0.0).any()
    assert [len(e) > 0 for e in M.expected(name)] == [False, True, True, True, False, True]


def test_area_edges():
    name = "area_edges@%dx%d" % (M.AREA_W, M.AREA_H)
    age, K, tss, params = M.LAYOUTS[name]
    raw = M.py_segment(M.history(*_hist_args(name, 1)), tss[1], 32.0)
    assert sorted((int(b[2]), int(b[3])) for b in raw) == [(3, 17), (5, 10), (20, 30), (599, 1)]
    assert sorted((int(b[2]), int(b[3])) for b in M.expected(name)[1]) == [(3, 17), (599, 1)]


@pytest.mark.parametrize("name,n", [("readback_1024", 1024), ("readback_1025", 1025), ("roots_at_cap", 3250), ("roots_over_cap", 3251),
                                    ("roots_full_lattice", 6500)])
def test_lattice_counts(name, n):
    """frame 1: n single pixels, n tile roots, n boxes of 1 x 1; the root list of one 520 x 50 slot holds 3250 entries, of two 6500"""
    w, h = M.size(name)
    assert (w, h) == (520, 50) and M.roots_cap(w, h) == 3250 and M.roots_cap(w, h, 2) == 6500
    m = M.model(name, 1)
    assert int(m["tile_roots"].sum()) == n == len(m["components"]) == len(M.expected(name)[1])
    assert (M.expected(name)[1][:, 2:] == 1).all()
    if name == "roots_at_cap": assert n == M.roots_cap(w, h)
    if name == "roots_over_cap": assert n == M.roots_cap(w, h) + 1
    if name == "roots_full_lattice": assert n == M.roots_cap(w, h, 2)
    # frame 2 still holds the lattice (a blob over some of it), frame 3 has dropped it
    assert int(M.model(name, 2)["tile_roots"].sum()) > n - 20
    assert int(M.model(name, 3)["tile_roots"].sum()) == 2 and len(M.expected(name)[3]) == 1       # (the blob of frame 2, unseeded now, and frame 3's)


def test_one_blob_is_one_root_a_frame():
    assert int(M.model("one_blob", 1)["tile_roots"].sum()) == 1
    assert [len(e) for e in M.expected("one_blob")] == [0, 1, 1, 1]
    assert int(M.model("roots_full_lattice", 1)["tile_roots"].sum()) + 1 == M.roots_cap(520, 50, 2) + 1


def test_size_twins_exist():
    for base in ("serpentine", "spirals", "comb", "comb_up", "unseeded_neighbours", "chain_of_ages", "expiring", "seg_edge", "clock_oddities"):
        assert M.size(base) == (520, 50) and M.size(base + "@513x49") == (513, 49)
