"""The premises of tests/test_gpu_raw_batch.py, on the CPU oracle alone:

  * prefix() cuts a cascade to its first k stages and both XML readers take the result;
  * a fresh face stream with min_neighbors = 0 returns the raw candidate list of its working image, in scan order;
  * grouped boxes do not notice a lost or an added candidate (why the raw lists are compared at all);
  * the inputs of the GPU tests fill the tile grid of the product's plan (conditions on the inputs, not measurements of a kernel:
    if a change of plan.cpp moves the grid below them, change frames or prefix, not the percentages)."""
import ctypes as C

import numpy as np
import pytest

import prefix_cascades as P

ARRAYS = ("stage_ncls", "stage_thr", "cls_nnodes", "rects", "rweights", "tilted", "node_thr", "left", "right", "alpha")


@pytest.mark.parametrize("name", sorted(P.CASCADES))
def test_prefix_round_trips(name):
    import __graft_entry__ as ge
    import orc
    ge.build()
    from nubovca import capi
    lib = capi.load()
    full = P.oracle_cascade(name)
    n = full.n_stages
    same = orc.parse_cascade_xml(P.prefix(P.cascade_xml(name), n))
    for a in ARRAYS:
        assert np.array_equal(getattr(same, a), getattr(full, a)), a
    for k in (1, 2, 3, 5, 8, 12):
        xml = P.cascade_xml(name, k)
        cut = orc.parse_cascade_xml(xml)
        ncls = int(full.stage_ncls[:k].sum())
        nnodes = int(full.cls_nnodes[:ncls].sum())
        assert cut.n_stages == k and (cut.ow, cut.oh) == (full.ow, full.oh)
        assert np.array_equal(cut.stage_ncls, full.stage_ncls[:k]) and np.array_equal(cut.stage_thr, full.stage_thr[:k])
        assert np.array_equal(cut.cls_nnodes, full.cls_nnodes[:ncls])
        for a in ("rects", "rweights", "tilted", "node_thr", "left", "right"):
            assert np.array_equal(getattr(cut, a), getattr(full, a)[:nnodes]), (k, a)
        assert np.array_equal(cut.alpha, full.alpha[:len(cut.alpha)]) and len(cut.alpha) >= nnodes
        # the product's loader (host side of the ABI)
        raw = xml.encode()
        w, h, ns, nw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        err = C.create_string_buffer(256)
        rc = lib.nvca_cascade_validate_mem(raw, len(raw), C.byref(w), C.byref(h), C.byref(ns), C.byref(nw), err, 256)
        assert rc == 0, err.value
        assert (w.value, h.value, ns.value, nw.value) == (full.ow, full.oh, k, nnodes)


# the three inputs of the sensitivity table: (cascade, frame set, frame, min_neighbors of the grouped tests that see this shape)
ROWS = [("synthetic", "hd", 0, 3), ("calibrated", "hd", 0, 3), ("synthetic", "sd450", 0, 2)]


def _working_raw(name, k, f, w2p):
    """detect_raw on the working image the reference's frame glue builds (resize, gray, equalizeHist), boxes scaled as the
    stream scales its events"""
    import orc
    H, W = f.shape[:2]
    scale = W // w2p
    cols, rows = (P.cv_round(W / scale), P.cv_round(H / scale)) if scale > 1 else (W, H)
    small = orc.resize_linear(f, cols, rows) if scale > 1 else f
    g = orc.equalize_hist(orc.bgr2gray(small))
    return orc.detect_raw(P.oracle_cascade(name, k), g, 1.1, 0, (cols // 20, rows // 20)) * max(scale, 1)


@pytest.mark.parametrize("name,fset,i,mn", ROWS)
def test_min_neighbors_zero_stream_returns_the_raw_list(name, fset, i, mn):
    import orc
    f = P.frame(fset, i)
    W = f.shape[1]
    boxes, ids = orc.FaceStream(P.oracle_cascade(name), width_to_process=W, scale_factor_pct=10, min_neighbors=0).process(f)
    exp = _working_raw(name, 0, f, W)
    assert 0 < len(exp) < P.ORC_MAX_FACES
    assert np.array_equal(boxes, exp) and np.array_equal(ids, np.arange(len(exp)))
    assert np.array_equal(P.raw_expected(name, 0, fset, i), exp)


def test_min_neighbors_zero_stream_shrinking():
    """shrink-first mode (width_to_process 160 on 640 x 480: working image 160 x 120, boxes times 4)"""
    import orc
    from nubovca import synth
    f = synth.make_bgr(640, 480, synth.frame_seed(0, 0), "natural", [(160, 120, 240)])
    for name in sorted(P.CASCADES):
        boxes, _ = orc.FaceStream(P.oracle_cascade(name), width_to_process=160, scale_factor_pct=10, min_neighbors=0).process(f)
        exp = _working_raw(name, 0, f, 160)
        assert 0 < len(exp) < P.ORC_MAX_FACES and np.array_equal(boxes, exp), (name, len(boxes), len(exp))
    for w2p in (160, 320):          # the 1080p shape of the GPU test
        f = P.frame("hd", 0)
        assert np.array_equal(P.raw_expected("calibrated", 0, "hd", 0, w2p), _working_raw("calibrated", 0, f, w2p))


def test_long_lists_come_from_the_stateless_half():
    """prefix 5 leaves ten thousand candidates on a 1080p frame: the oracle stream keeps 256 of them, frame_detect all"""
    import orc
    f = P.frame("hd", 0)
    exp = _working_raw("calibrated", 5, f, 1920)
    assert len(exp) > 5000
    st = orc.FaceStream(P.oracle_cascade("calibrated", 5), width_to_process=1920, scale_factor_pct=10, min_neighbors=0)
    assert np.array_equal(st.frame_detect(f, cap=1 << 17), exp)
    assert np.array_equal(st.process(f)[0], exp[:P.ORC_MAX_FACES])
    assert np.array_equal(P.raw_expected("calibrated", 5, "hd", 0), exp)


def _isolated_box(raw, W, H):
    """a window-sized box that groupRectangles cannot attach to any candidate of the list"""
    w, h = int(raw[:, 2].min()), int(raw[:, 3].min())
    for y in range(0, H - h, h):
        for x in range(0, W - w, w):
            if ((np.abs(raw[:, 0] - x) > 2 * raw[:, 2]) | (np.abs(raw[:, 1] - y) > 2 * raw[:, 3])).all():
                return np.array([x, y, w, h], np.int32)
    raise AssertionError("no free place")


@pytest.mark.parametrize("name,fset,i,mn", ROWS)
def test_grouped_boxes_do_not_see_single_candidates(name, fset, i, mn):
    """what the grouped tests of the timed path cannot see: drop each raw candidate in turn, add one isolated candidate, and
    group.  Asserted only as 'some drop and the added one go unnoticed'; the counts are printed (README)."""
    import orc
    f = P.frame(fset, i)
    H, W = f.shape[:2]
    raw = np.array(P.raw_expected(name, 0, fset, i))
    grouped, _ = orc.group_rectangles(raw, mn)
    stream, _ = orc.FaceStream(P.oracle_cascade(name), width_to_process=W, scale_factor_pct=10, min_neighbors=mn).process(f)
    assert len(grouped) > 0 and np.array_equal(grouped, stream)          # grouping the raw list is what the stream does
    unnoticed = sum(np.array_equal(orc.group_rectangles(np.delete(raw, j, axis=0), mn)[0], grouped) for j in range(len(raw)))
    extra = _isolated_box(raw, W, H)
    added_unnoticed = np.array_equal(orc.group_rectangles(np.vstack([raw, extra[None]]), mn)[0], grouped)
    print("sensitivity: %s %dx%d min_neighbors %d: %d raw candidates, %d grouped boxes, %d of %d single drops unnoticed, added isolated candidate %s"
          % (name, W, H, mn, len(raw), len(grouped), unnoticed, len(raw), "unnoticed" if added_unnoticed else "noticed"))
    assert unnoticed >= 1 and added_unnoticed


# ---------------------------------------------------------------- coverage conditions of the GPU tests' inputs
HD_BATCH = range(8)          # the frames the prefixes run on


def _coverage(k):
    pl = P.plan("calibrated", k, 1920, 1080)
    if pl is None:
        pytest.skip("no clang++")
    head, scales = pl
    assert head["strips"] == 0 and head["tiles"] == len(P.all_cells(scales)) and head["stages"] == (k or 22)
    cells = P.all_cells(scales)
    per, union, longest = [], set(), 0
    for i in HD_BATCH:
        raw = P.raw_expected("calibrated", k, "hd", i)
        c = P.tile_cells(scales, raw)
        assert c <= cells
        per.append(len(c) / len(cells))
        union |= c
        longest = max(longest, len(raw))
    print("coverage: calibrated prefix %d: %d cells, per frame %s, union %d, longest list %d"
          % (k, len(cells), " ".join("%.1f%%" % (100 * p) for p in per), len(union), longest))
    return per, len(union) / len(cells), len(union) == len(cells), longest


def test_prefix3_fills_every_tile_cell():
    per, union, every, longest = _coverage(3)
    assert min(per) >= 0.95 and every          # every frame is non-degenerate at three stages (frame 3 has no faces, not no candidates)
    assert longest <= P.HIT_CAP


def test_prefix5_fills_most_tile_cells():
    per, union, every, longest = _coverage(5)
    assert min(per) >= 0.75 and union >= 0.95
    assert longest <= P.HIT_CAP


def test_full_cascades_find_something_wherever_there_is_a_face():
    for name in sorted(P.CASCADES):
        for i in range(P.FRAME_SETS["hd"][2]):
            n = len(P.raw_expected(name, 0, "hd", i))
            assert (n > 0) == P.has_faces("hd", i), (name, i, n)
            assert n < P.ORC_MAX_FACES


def test_other_inputs_fit_the_hit_capacity():
    """the remaining batches of the GPU tests: every list below the capacity they set, and long enough to matter"""
    for k, fset, lo in ((8, "hd", 500), (12, "hd", 20), (5, "p720", 5000), (5, "q360", 5000), (5, "q300", 5000)):
        n = [len(P.raw_expected("calibrated", k, fset, i)) for i in (HD_BATCH if fset == "hd" else range(P.FRAME_SETS[fset][2]))]
        assert lo <= min(n) and max(n) <= P.HIT_CAP, (k, fset, min(n), max(n))
    n2 = [len(P.raw_expected("calibrated", 2, "hd", i)) for i in HD_BATCH]
    assert P.HIT_CAP < max(n2) <= 2 * P.HIT_CAP, n2          # prefix 2 needs the doubled capacity its test asks for
