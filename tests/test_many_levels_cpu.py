"""The premises of tests/test_gpu_many_levels.py, asserted on the statements alone (no GPU): every case of tests/many_levels_cases.py has
more than 63 pyramid levels, holds windows in levels of index 63 and up -- counted by level --, and answers differently when the scan is cut
after its first 63 levels, raw and grouped.  That cut is what the large-image routes once did in silence; a device that did it again
would fail every one of the device tests."""
import numpy as np
import pytest

import lbp_part_cases as LP
import lbp_reference as LR
import levels_reference as LV
import many_levels_cases as M
import orc

KEPT = M.KEPT


def _differ(a, b):
    return a.shape != b.shape or not np.array_equal(a, b)


# ------------------------------------------------------------------ new-format cascades, single images
@pytest.mark.parametrize("cid", sorted(M.SINGLE))
def test_single_image_cases_lose_windows_under_the_cut(cid):
    kind, _name, cols, rows, sf, nlev, nraw, beyond = M.SINGLE[cid]
    _xml, ref, gray, sf, exp = M.single(cid)
    assert gray.shape == (rows, cols)
    per = M.single_by_level(cid)
    assert len(per) == nlev > KEPT and len(LR.levels(*ref.size, cols, rows, sf)) == nlev
    assert np.array_equal(M.joined(per), exp) and len(exp) == nraw      # level by level it is the statement's list
    assert sum(len(p) for p in per[KEPT:]) == beyond > 0                # (counted by level; by window width the 1.01 rows look the same)
    cut = M.joined(per[:KEPT])
    assert _differ(cut, exp)
    for mn in M.GROUP_THRESHOLDS:
        assert _differ(M.grouped(cut, mn), M.grouped(exp, mn)), mn


# ------------------------------------------------------------------ the boundary
@pytest.mark.parametrize("kind", [M.LBP, M.HAAR])
def test_boundary_scans_have_63_64_and_65_levels(kind):
    name, cols, rows, sf, mins, maxs = M.BOUNDARY[kind]
    assert (mins, maxs) in M.boundary_found(kind)                      # what the search finds on the CPU
    _xml, ref, gray, sf, mins, scans = M.boundary(kind)
    lists = []
    for (m, exp), n in zip(scans, M.BOUNDARY_LEVELS):
        per = M.by_level(kind, ref, gray, sf, mins, m)
        assert len(per) == n and len(per[-1]) > 0, (m, len(per))
        assert np.array_equal(M.joined(per), exp)
        lists.append(exp)
    assert len(lists[0]) < len(lists[1]) < len(lists[2])
    # the scan of 63 levels is what the cut leaves of the two longer ones: a device that cut would answer all three alike
    assert np.array_equal(lists[1][:len(lists[0])], lists[0]) and np.array_equal(lists[2][:len(lists[0])], lists[0])


# ------------------------------------------------------------------ the plans' host code on such scans (no GPU, no HIP)
def test_host_tables_hold_every_level(tmp_path):
    """csrc/pyr_levels.cpp and csrc/lbp_tables.cpp behind tests/san/lbp_tables_driver.cpp (tests/test_lbp_tables_cpu.py's program and its
    statement of the tables), asked for every level as lbp_plan and si_plan ask: the level lists are the statement's and the oracle's,
    160 levels take eight key bits, and tiles, bit words and scan rows go on past the 63rd level"""
    import json
    import os
    import subprocess
    import test_lbp_tables_cpu as T
    if not os.path.exists(T.CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    driver = T._build_driver()
    xml, ref, gray, sf, _exp = M.single("lbp-w24-160x120-1.01")
    path = str(tmp_path / "w24.xml")
    with open(path, "w") as f:
        f.write(xml)
    (osf, omins), oc = M.OLD_SCANS[1], M.old_cascade("synth")
    lines = ["scan many %s 160 120 %r 0 0 160 120" % (path, sf),
             "rules old %d %d 160 120 %r %d %d 160 120" % (oc.ow, oc.oh, osf, omins[0], omins[1])]
    manifest = str(tmp_path / "manifest.txt")
    with open(manifest, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([driver, manifest], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-1000:], r.stderr[-4000:])
    got = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("{"):
            o = json.loads(ln)
            got[o.pop("case")] = o
    levels = LR.levels(*ref.size, 160, 120, sf)
    assert len(levels) == 160
    many, exp = T._f32(got["many"]), T._f32(T.expected(ref, levels, 160))
    assert not T._diff(many, exp), [(k, many.get(k), exp.get(k)) for k in T._diff(many, exp)[:3]]
    assert many["key_ss"] - many["key_sy"] >= 1 and many["key_ss"] + 8 <= 32 and max(t[0] for t in many["tiles"]) == 159
    assert len(got["old"]["si"]) == M.old_case("synth", osf, omins)[1] > KEPT          # the oracle's level count
    assert got["old"]["lbp"] == [[f, sz[0], sz[1], w[0], w[1]] for f, sz, w in LR.levels(oc.ow, oc.oh, 160, 120, osf, omins)]


# ------------------------------------------------------------------ old-format cascades, CV_HAAR_SCALE_IMAGE
@pytest.mark.parametrize("sf,mins", M.OLD_SCANS)
@pytest.mark.parametrize("which", M.OLD_CASCADES)
def test_old_format_scale_image_cases(which, sf, mins):
    raw, nlev = M.old_case(which, sf, mins)
    assert nlev > KEPT and max(M.old_image().shape) <= 160
    cut = M.old_first_levels(which, sf, mins)                          # the oracle's scan ended behind level 62 by max_size
    assert cut is not None
    # the oracle emits level after level: the first 63 levels' list is the head of the whole one, and the rest lies in levels 63 and up
    assert len(cut) < len(raw) and np.array_equal(raw[:len(cut)], cut)
    c = M.old_cascade(which)
    assert any(_differ(orc.detect_multiscale(c, M.old_image(), sf, mn, orc.HAAR_SCALE_IMAGE, mins), M.grouped(cut, mn)) for mn in M.GROUP_THRESHOLDS)
    for mn in M.GROUP_THRESHOLDS:                                      # (the oracle groups its own raw list)
        assert np.array_equal(orc.detect_multiscale(c, M.old_image(), sf, mn, orc.HAAR_SCALE_IMAGE, mins), M.grouped(raw, mn))


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("kind", [M.LBP, M.HAAR])
def test_batch_images_differ_and_both_lose_windows(kind):
    _xml, ref, grays, sf, exps = M.batch(kind)
    assert grays[0].shape == grays[1].shape and not np.array_equal(grays[0], grays[1]) and _differ(exps[0], exps[1])
    for seed, exp in zip(M.BATCH_SEEDS, exps):
        per = M.single_by_level(M.BATCH[kind], seed)
        assert len(per) > KEPT and np.array_equal(M.joined(per), exp) and sum(len(p) for p in per[KEPT:]) > 0
        assert any(_differ(M.grouped(M.joined(per[:KEPT]), mn), M.grouped(exp, mn)) for mn in M.GROUP_THRESHOLDS)


# ------------------------------------------------------------------ reject levels and level weights
@pytest.mark.parametrize("kind", [M.LBP, M.HAAR])
def test_levels_cases_emit_windows_beyond_level_63(kind):
    _xml, ref, _gray, _sf, (rects, levels, weights) = M.levels_case(kind)
    assert len(ref.stage_sizes) >= 4
    per = M.levels_by_level(kind)
    assert len(per) > KEPT
    for k, whole in enumerate((rects, levels, weights)):
        assert np.array_equal(np.concatenate([p[k] for p in per]), whole)
    assert sum(len(p[0]) for p in per[KEPT:]) > 0
    # the weighted grouping of the whole list and of the cut one
    cut = [np.concatenate([p[k] for p in per[:KEPT]]) for k in range(3)]
    assert any(any(_differ(a, b) for a, b in zip(LV.group_levels(rects, levels, weights, mn), LV.group_levels(*cut, mn))) for mn in M.LEVELS_THRESHOLDS[kind])


# ------------------------------------------------------------------ face streams
@pytest.mark.parametrize("kind", [M.LBP, M.HAAR])
def test_stream_frames_keep_a_window_of_a_late_level_through_the_grouping(kind):
    name, W, H, wtp, _seeds = M.STREAM[kind]
    ref = M.cascade(kind, name)[1]
    assert (W, H, wtp) == (160, 120, 160)
    survives = 0
    ex = M.stream_expected(kind)
    for f, pct in sorted(set(zip(M.stream_frames(kind), M.STREAM_PCT))):          # (the third frame is the second again)
        w, mins = M.stream_working(kind, f)
        assert w.shape == (120, 160)
        per = M.by_level(kind, ref, w, 1 + pct / 100, mins)
        raw = M.stream_raw(kind, f, pct)
        assert len(per) == {1: 160, 2: 81}[pct] and np.array_equal(M.joined(per), raw)
        assert sum(len(p) for p in per[KEPT:]) > 0
        # the boxes of the whole list against those of the cut one: where they differ, windows of levels 63 and up made a box or moved one
        survives += int(_differ(M.grouped(raw, 3), M.grouped(M.joined(per[:KEPT]), 3)))
    assert survives > 0
    for f, pct in zip(M.stream_frames(kind), M.STREAM_PCT):
        ex.p.update(scale_factor_pct=pct)
        assert len(ex.process(f)[0]) > 0                                   # (and every list is one the oracle's stream tracks)


# ------------------------------------------------------------------ a part stream whose face cascade is LBP
@pytest.mark.skipif(LP.shim() is None, reason="no clang++")
def test_part_stream_face_pass_has_windows_beyond_level_63():
    ref = LP.refs()[LP.FACE]
    seen = []

    def face(g, sf, mn, flags, mins, maxs):
        per = M.by_level(M.LBP, ref, g, sf, mins, maxs)
        seen.append((g.shape, sf, len(per), sum(len(p) for p in per[KEPT:])))
        return M.grouped(M.joined(per), mn)

    def face_cut(g, sf, mn, flags, mins, maxs):
        return M.grouped(M.joined(M.by_level(M.LBP, ref, g, sf, mins, maxs)[:KEPT]), mn)

    exp, _ = M.part_expected()
    by_lvl, _ = M.part_expected(LP.Detector(face))
    assert len(seen) == M.PART_FRAMES and all(s[0] == (120, 160) and s[1] == 1.02 and s[2] == 81 and s[3] > 0 for s in seen), seen
    for a, b in zip(exp, by_lvl):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert sum(len(a) + len(b) for a, b in exp) > 0
    cut, _ = M.part_expected(LP.Detector(face_cut))
    assert any(_differ(a[0], b[0]) or _differ(a[1], b[1]) for a, b in zip(exp, cut))
