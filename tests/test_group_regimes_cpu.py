"""The premises of tests/test_gpu_group_regimes.py, on the CPU oracle and py_group alone (tests/marker_cascades.py):

  * every single-scale layout leaves exactly the candidate list it was built for, one window per dot, in scan order;
  * the oracle's groupRectangles and py_group -- two statements of the operation written apart -- agree on every layout, boxes
    and weights, for the thresholds 1, 2, 3, 5 and 9;
  * every layout is in the regime it is named for: its counts sit on k_group's limits (conditions on the inputs: if a kernel constant
    moves, move the layout);
  * the frames of the threshold tests give another box list for every threshold used, so a stale threshold cannot hide.

The host library's group_rectangles needs a context (a device) to be reached; it is fed the same lists in the GPU file."""
import numpy as np
import pytest

import marker_cascades as M

NAMES = sorted(M.LAYOUTS)


@pytest.mark.parametrize("name", NAMES)
def test_raw_list_is_the_constructed_one(name):
    l = M.LAYOUTS[name]
    raw = M.expected_raw(name)
    if l.single_scale:
        assert np.array_equal(raw, M.dot_windows(l.dots)), (len(raw), len(l.dots))
    else:
        assert len(raw) > len(l.dots) and len(set(raw[:, 2].tolist())) >= 6          # several candidates a dot, many scales
    assert len(raw) < 4096          # the oracle's grouping is quadratic


@pytest.mark.parametrize("thr", M.THRESHOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_groups_as_py_group(name, thr):
    boxes, weights = M.expected_grouped(name, thr)
    g = M.facts(name, thr)
    assert np.array_equal(boxes, g.boxes), (boxes.tolist(), g.boxes.tolist())
    assert np.array_equal(weights, g.weights)
    assert len(g.boxes) == sum(v in ("free", "contained_kept") for v in g.verdict)


def test_py_group_scalar_and_row_similarity_agree():
    """_similar is SimilarRects as OpenCV writes it; the row-wise form py_group uses gives the same pairs"""
    for name in ("rounding", "filter_small", "corners"):
        r = np.array(M.expected_raw(name))
        pairs = set(M._similar_pairs(r, 0.2))
        for i in range(len(r)):
            for j in range(i + 1, len(r)):
                assert M._similar(r[i].tolist(), r[j].tolist(), 0.2) == ((i, j) in pairs), (name, i, j)


# ---------------------------------------------------------------- the regimes
def _counts(name, thr=1):
    g = M.facts(name, thr)
    return g.n, len(g.sizes), len(g.boxes)


def test_sort_switch():
    assert _counts("sort256") == (M.GROUP_SORT, 32, 32)
    assert _counts("sort257") == (M.GROUP_SORT + 1, 33, 32)
    assert M.facts("sort256", 1).sizes == [8] * 32
    # the clusters share their rows: keys of different classes interleave in scan order
    labels = M.facts("sort256", 1).labels
    assert labels[:4] == [0, 0, 0, 0] and labels[4] == 1 and labels.count(0) == 8 and labels.index(0, 4) > labels.index(15)


def test_candidate_limit():
    assert _counts("cand2048") == (M.GROUP_MAX, 64, 64) and M.facts("cand2048", 1).sizes == [32] * 64
    assert _counts("cand2049") == (M.GROUP_MAX + 1, 65, 64)
    assert len(M.facts("cand2048", 9).boxes) == M.GROUP_OUT          # exactly as many boxes as the device's table holds
    for n in (M.GROUP_MAX - 1, M.GROUP_MAX, M.GROUP_MAX + 1):
        assert _counts("chain%d" % n) == (n, 1, 1)
    ends = M.LAYOUTS["chain2048"].dots
    assert abs(ends[0][0] - ends[-1][0]) >= 600          # one class whose members are far from similar: only the chain joins them


def test_class_limit():
    assert _counts("cls256") == (312, M.GROUP_CLASSES, 56)
    assert _counts("cls257") == (313, M.GROUP_CLASSES + 1, 56)
    for n in (255, 256, 257):
        assert _counts("singles%d" % n) == (n, n, 0)
    # the kept classes fall in all four 64-class waves, each with dropped classes before, between and behind them
    g = M.facts("cls256", 1)
    kept = [c for c, v in enumerate(g.verdict) if v == "free"]
    for wave in range(4):
        inside = [c for c in kept if c // 64 == wave]
        assert len(inside) >= 10 and min(inside) > 64 * wave and max(inside) < 64 * wave + 63
        assert any(b - a > 1 for a, b in zip(inside, inside[1:]))
    assert 0 < len(g.boxes) <= M.GROUP_OUT          # few enough boxes that the device's answer is the one used


def test_box_limit():
    assert _counts("box64") == (128, 64, M.GROUP_OUT)
    assert _counts("box65") == (130, 65, M.GROUP_OUT + 1)


def test_rounding():
    g = M.facts("rounding", 1)
    assert g.sizes == [4, 4, 4, 4, 3, 5, 6, 7, 12]
    four = [(c, k, v) for (c, k, v) in g.ties if g.sizes[c] == 4]
    assert any(v % 2 == 0 for (_, _, v) in four) and any(v % 2 == 1 for (_, _, v) in four)          # both tie directions
    assert {c for (c, _, _) in four} == {0, 1, 2, 3}
    # truncation and round-half-up would each move a box
    r = np.array(M.expected_raw("rounding")).astype(np.int64)
    for wrong in (np.floor, lambda v: np.floor(v + 0.5)):
        moved = 0
        for c, size in enumerate(g.sizes):
            m = np.array(g.labels) == c
            moved += int((wrong(r[m].sum(0) / size).astype(np.int64) != g.avg[c]).any())
        assert moved >= 2
    # 1.f / n inexact: the 12-dot cluster's x average is a tie in exact arithmetic and is reported as one in float as well
    assert (8, 0, 355) in g.ties and g.avg[8, 0] == 356


FILTER = ("filter_pair", "filter_block", "filter_small")


def test_filter_branches():
    seen, boundary = set(), 0
    for name in FILTER:
        for thr in (1, 2, 3, 5):
            g = M.facts(name, thr)
            seen |= set(g.verdict)
            boundary += len(g.boundary)
    assert {"removed_small", "removed_outvoted", "removed_both", "contained_kept", "free", "weak"} <= seen, seen
    assert boundary > 0          # a class inside one of exactly max(3, n1) members: '>' keeps it, '>=' would not
    assert M.facts("filter_pair", 1).sizes == [2, 6, 6, 6, 6, 4, 2]
    lists = [M.expected_grouped("filter_pair", thr)[0].tolist() for thr in (1, 2, 5)]
    assert lists[0] != lists[1] != lists[2] != lists[0]


def test_key_decode_layout():
    l = M.LAYOUTS["corners"]
    raw = M.expected_raw("corners")
    assert (l.W, l.H) == (1920, 1080) and len(M.facts("corners", 1).boxes) == 5
    assert raw[:, 0].min() <= 4 and raw[:, 1].min() <= 4 and (raw[:, 0] + raw[:, 2]).max() >= l.W - 4 and (raw[:, 1] + raw[:, 3]).max() >= l.H - 4
    assert len(set(raw[:, 2].tolist())) >= 30          # the middle pair is seen at every scale of the plan


def test_degenerate():
    assert _counts("empty") == (0, 0, 0)
    assert _counts("one_dot") == (1, 1, 0)
    assert _counts("one_class8", 9) == (8, 1, 0) and _counts("one_class8", 5) == (8, 1, 1)


# ---------------------------------------------------------------- frames of the batched face path
def test_face_frames_are_in_their_regimes():
    n = {k: len(M.face_raw(k)) for k in M.FACE_FRAMES}
    assert n["black"] == 0
    assert 0 < n["three"] < 256          # an oracle stream with min_neighbors 0 keeps 256 faces: the raw slot stays below
    assert M.GROUP_MAX < n["grid36"] < 4096
    assert n["edge70"] <= M.GROUP_MAX and len(M.face_expected("edge70", 1)[0]) == 70 > M.GROUP_OUT
    assert len(M.face_expected("three", 3)[0]) == 2 and len(M.face_expected("grid36", 3)[0]) >= 20
    b, ids = M.face_expected("three", 0)
    assert np.array_equal(b, M.face_raw("three")) and np.array_equal(ids, np.arange(n["three"]))
    for k in M.FACE_FRAMES:          # a stream groups its frame's raw list
        if n[k]:
            assert np.array_equal(M.face_expected(k, 2)[0], M.py_group(M.face_raw(k), 2).boxes), k


@pytest.mark.parametrize("name", [k for k in M.FACE_FRAMES if k.startswith("ladder")])
def test_every_threshold_gives_another_box_list(name):
    """a stale or misplaced threshold must show: the boxes of a ladder frame differ between every two min_neighbors used, and
    between every two ladder frames"""
    lists = {mn: M.face_expected(name, mn)[0].tolist() for mn in M.FACE_MIN_NEIGHBORS}
    assert [len(lists[mn]) for mn in M.FACE_MIN_NEIGHBORS] == [5, 4, 3, 2]
    for a in M.FACE_MIN_NEIGHBORS:
        for b in M.FACE_MIN_NEIGHBORS:
            assert a == b or lists[a] != lists[b], (a, b)
    for other in M.FACE_FRAMES:
        if other.startswith("ladder") and other != name:
            for mn in M.FACE_MIN_NEIGHBORS:
                assert M.face_expected(other, mn)[0].tolist() != lists[mn]


def test_threshold_script_shows_every_threshold():
    """every batch of the script: a slot's box count names the min_neighbors it was grouped with (the temporal logic keeps one face
    per detection), so a slot answered with another slot's or an earlier batch's threshold cannot pass"""
    batches = M.threshold_script_expected()
    assert len(batches) == 5 + 2 * 3
    for idx, thr, res in batches:
        assert [len(b) for (b, _) in res] == [M.BOXES_AT[t] for t in thr], (idx, thr)
    sync = [b for b in batches[:5]]
    assert [len(b[0]) for b in sync] == [6, 6, 3, 12, 6]
    assert sync[0][1] != sync[1][1] and sync[2][1] != sync[1][1][:3] and sync[3][1][:6] == sync[4][1]
    a, b = batches[5], batches[6]
    assert a[1] != b[1]          # two batches in flight that carry different thresholds
