"""The premises of tests/test_gpu_hnew_roi.py on the CPU, without the kernel under test: every constructed case of
tests/hnew_roi_cases.py is what the numpy statement (tests/haar_new_reference.py) gives, and lies in the regime it is named for (a
reject run across the 64-column chunk, bands of whole rows, queues on both sides of the length that switches the lane mapping, stages
wider than the vote area in both paddings, windows on the nf <= 0 branch, images on both sides of the LDS bound).  The two entry points
of the opt-in are in the binding's symbol list.  And the pure host half of the route (csrc/hnew_roi_tables.cpp, csrc/lbp_roi_tables.cpp
on the window size) under AddressSanitizer + UndefinedBehaviorSanitizer: tests/san/hnew_roi_tables_driver.cpp, a stand-alone program
built as tests/test_lbp_roi_cpu.py builds its driver (no preload, nothing loaded into Python), prints the step records, bands and
cascade table of each case; every field is compared with a statement written here from tests/haar_new_reference.py and the record
comments of csrc/device_records.h."""
import json
import os
import subprocess

import numpy as np
import pytest

import haar_new_cases as K
import haar_new_reference as R
import hnew_roi_cases as RC
from nubovca import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


# ------------------------------------------------------------------ the interface
def test_the_opt_in_entry_points_are_bound():
    assert {"nvca_cascade_set_small_route", "nvca_cascade_get_small_route"} <= set(capi.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "nubovca.h")).read()
    assert "int  nvca_cascade_set_small_route(nvca_cascade *c, int on);" in header and "int  nvca_cascade_get_small_route(const nvca_cascade *c, int *on);" in header
    assert callable(capi.Cascade.set_small_route) and callable(capi.Cascade.small_route)


# ------------------------------------------------------------------ the cases on the statement
@pytest.mark.parametrize("case", RC.hand_cases(), ids=[c[0] for c in RC.hand_cases()])
def test_hand_cases_are_the_statements(case):
    _, cdict, gray, sf, mins, maxs, exp = case
    ref = R.parse_xml(RC.hand_xml(cdict))
    assert R.scan(ref, gray, sf, mins, maxs).tolist() == exp
    rows, cols = gray.shape
    assert RC.fits_lds(cols, rows)


def test_reject_runs_cross_the_chunk_and_change_what_is_emitted():
    """one level of 67 grid columns at step 2; every window of it is on the nf <= 0 branch (vnf = 1: the sign of one pixel difference
    decides); an odd run drops the column behind it, an even run does not; runs end at the chunk's last lane, one before and one behind"""
    ref = R.parse_xml(RC.hand_xml(RC.PAIR_STAGE0))
    for cid, g, exp in RC.skip_chunk_cases():
        assert RC.grid_of(3, 3, g.shape[1], g.shape[0], 4.0) == [(RC.N_COLS, g.shape[0] // 2 - 1)], cid
        stats = {}
        R.scan(ref, g, 4.0, stats=stats)
        assert stats["nf_nonpositive"] == RC.N_COLS * (g.shape[0] // 2 - 1) and stats["levels"] == 1, cid
    by_end = {}
    for end, L in RC.RUNS:
        p, em = RC.run_row(end, L)
        assert (end + 1 in em) == (L % 2 == 0) and all(j in em for j in range(RC.N_COLS) if p[j] and j != end + 1)
        by_end.setdefault(end, set()).add(L % 2)
    assert by_end == {62: {0, 1}, 63: {0, 1}, 64: {0, 1}}
    assert RC.N_COLS > 64 + 2


def test_named_cases_are_in_their_regimes():
    G = {c[0]: RC.grid_of(*K.cascade(c[1])[1].size, c[2], c[3], c[4]) for c in RC.NAMED}
    for c in RC.NAMED:
        xml, gray, sf, exp, stats = RC.named_case(c[0])
        assert len(exp) == RC.NAMED_WINDOWS[c[0]] > 0, c
        assert stats["nf_nonpositive"] > 0, c                                   # the flat corner patch: windows whose vnf is 1
        assert RC.fits_lds(c[2], c[3]) and len(G[c[0]]) <= 63, c
    assert RC.named_case("short-queues-deep-97x83")[4]["nf_nonpositive"] == 85
    g = G["bands-w12-160x90"]
    assert g[0] == (74, 39) and 74 * 39 == 2886 > RC.ROI_MAX_WIN                # its first level goes out as bands of whole rows
    g = G["last-band-one-row-w24-120x110"]
    assert g[0] == (48, 43) and RC.ROI_MAX_WIN // 48 == 42                      # 42 rows, then a band of one
    assert max(nx * ny for nx, ny in G["single-band-w12-97x83"]) <= RC.ROI_MAX_WIN
    assert K.cascade("w20x28")[1].size == (20, 28)
    name, cols, rows, sf = RC.TOO_MANY_LEVELS
    assert len(RC.grid_of(*K.cascade(name)[1].size, cols, rows, sf)) > 63 and RC.fits_lds(cols, rows)


def test_deep_cascade_has_queues_on_both_sides_of_the_lane_mapping_switch():
    xml, gray, sf, exp, stats = RC.named_case("short-queues-deep-97x83")
    ref = K.cascade("deep")[1]
    assert len(ref.stage_sizes) == 20
    depth = np.asarray(stats["depth"])
    alive = [int(np.count_nonzero((depth > 0) | (depth <= -s))) for s in range(10)]
    assert alive == [4138, 3584, 2993, 2993, 2112, 1523, 1195, 772, 535, 335]
    lengths = [n for band in RC.band_queue_lengths(ref, gray, sf) for n in band if n > 0]
    assert 0 < RC.SHORT_WIN and any(n > RC.SHORT_WIN for n in lengths) and any(n <= RC.SHORT_WIN for n in lengths), (RC.SHORT_WIN, sorted(lengths)[-5:])


def test_wide_stages_meet_short_queues_in_both_paddings():
    """the 70- and the 130-stump stage on queues of at most 64 windows (64 stumps a chunk: 2 and 3 chunks) and on queues of 65 .. 256
    windows (32, 21 or 16 stumps a chunk), and on long queues as well (a window per lane)"""
    xml, gray, sf, exp = RC.wide_case()
    ref = RC.wide_cascade()[1]
    assert list(ref.stage_sizes) == [2, 3, 17, 33, 70, 130] and len(exp) == 3939
    assert RC.VOTE_WORDS // 64 == 64 and -(-70 // 64) == 2 and -(-130 // 64) == 3
    q = RC.band_queue_lengths(ref, gray, sf)
    for s in (4, 5):                  # the stages of 70 and 130 stumps; band[s - 1]: the queue in front of stage s
        n = [band[s - 1] for band in q]
        assert any(0 < v <= 64 for v in n) and any(64 < v <= RC.SHORT_WIN for v in n) and any(v > RC.SHORT_WIN for v in n), (s, n)
        for v in n:
            if 64 < v <= RC.SHORT_WIN:
                assert ref.stage_sizes[s] > RC.VOTE_WORDS // ((v + 63) // 64 * 64)          # more stumps than a chunk holds


def test_bound_images_straddle_the_bound():
    inside, outside = RC.bound_images()
    assert (inside, outside) == ((200, 75), (200, 76))
    assert RC.fits_lds(*inside) and not RC.fits_lds(*outside)
    assert RC.MAX_BYTES == 122800 and RC.fits_lds(160, 90) and not RC.fits_lds(160, 120)
    assert RC.roi_lds_bytes((inside[0] + 1) * (inside[1] + 1)) <= 160 * 1024 - 64
    ref = K.cascade("w24")[1]
    assert [len(R.scan(ref, K.image(c, r, 24, 24), RC.BOUND_SF)) for c, r in (inside, outside)] == [126, 103]
    # the u32 squared plane: the most an image inside the bound can total stays below 2^32, and a resized level fits the room it is staged in
    assert 255 * 255 * (RC.MAX_BYTES // 8) < 1 << 32 and RC.MAX_BYTES // 8 <= RC.VOTE_WORDS * 4 + RC.ROI_MAX_WIN * 8


def test_bright_image_is_near_the_largest_squared_sums():
    xml, gray, sf, exp, stats = RC.bright_case()
    assert gray.shape == (75, 200) and gray.min() >= 249 and RC.fits_lds(200, 75)
    total = int((gray.astype(np.int64) ** 2).sum())
    assert 0.92 * 255 * 255 * (RC.MAX_BYTES // 8) < total < 1 << 32
    assert len(exp) > 0 and stats["nf_nonpositive"] == 0


def test_cut_outs_and_the_overflow_case_are_what_the_device_test_takes_them_for():
    """minSize / maxSize leave a proper, non-empty part of the full list; the permissive cascade on 60 x 60 emits more than ten times the 64
    candidates the device test leaves room for, on an image inside the bound"""
    ref = K.cascade("w12")[1]
    full = K.expected_raw("w12", 97, 83, 1.1)
    for mins, maxs in (((16, 16), (0, 0)), ((0, 0), (30, 30)), ((16, 16), (30, 30))):
        assert 0 < len(K.expected_raw("w12", 97, 83, 1.1, mins, maxs)) < len(full), (mins, maxs)
    perm = R.parse_xml(RC.hand_xml(K.permissive(12, 12)))
    assert len(R.scan(perm, np.full((60, 60), 120, np.uint8), 1.2)) > 640 and RC.fits_lds(60, 60)


# ------------------------------------------------------------------ the host half under sanitizers
def _build_driver():
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "hnew_roi_tables_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "hnew_roi_tables_driver.cpp")] + [os.path.join(csrc, f) for f in ("cascade_xml.cpp", "plan.cpp", "pyr_levels.cpp", "lbp_roi_tables.cpp", "hnew_roi_tables.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        # (function sections, unused ones dropped: plan.cpp's table uploads call into the HIP runtime, which is not part of this driver)
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


DEGENERATE = (("window-is-image", 12, 12, 1.1, (0, 0), (12, 12)), ("one-by-one", 1, 1, 1.1, (0, 0), (1, 1)),
              ("one-level", 13, 13, 1.1, (0, 0), (13, 13)), ("one-level-by-size", 60, 60, 1.99, (24, 24), (24, 24)),
              ("no-level-by-size", 60, 60, 1.99, (25, 25), (30, 30)))


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    d = tmp_path_factory.mktemp("hnew_roi")
    xmls = {}

    def path(name, text):
        if name not in xmls:
            xmls[name] = str(d / (name + ".xml"))
            open(xmls[name], "w").write(text)
        return xmls[name]

    inside, outside = RC.bound_images()
    lines = ["consts consts", "fits inside %d %d" % inside, "fits outside %d %d" % outside, "fits 160x120 160 120", "fits 160x90 160 90", "fits 1x1 1 1"]
    casc_of = {}
    for cid, name, cols, rows, sf in RC.NAMED:
        lines.append("steps %s %s %d %d %r 0 0 %d %d" % (cid, path(name, K.cascade(name)[0]), cols, rows, sf, cols, rows))
        casc_of[cid] = K.cascade(name)[1]
    name, cols, rows, sf = RC.TOO_MANY_LEVELS
    lines.append("steps too-many-levels %s %d %d %r 0 0 %d %d" % (path(name, K.cascade(name)[0]), cols, rows, sf, cols, rows))
    casc_of["too-many-levels"] = K.cascade(name)[1]
    cols, rows, sf = RC.WIDE_IMAGE
    lines.append("steps wide %s %d %d %r 0 0 %d %d" % (path("wide", RC.wide_cascade()[0]), cols, rows, sf, cols, rows))
    casc_of["wide"] = RC.wide_cascade()[1]
    lines.append("steps skip-chunk %s %d %d 4.0 0 0 %d %d" % (path("pair", RC.hand_xml(RC.PAIR_STAGE0)), 2 * RC.N_COLS + 2, 8, 2 * RC.N_COLS + 2, 8))
    casc_of["skip-chunk"] = R.parse_xml(RC.hand_xml(RC.PAIR_STAGE0))
    for (c, r), cid in zip((inside, outside), ("inside-bound", "outside-bound")):
        lines.append("steps %s %s %d %d %r 0 0 %d %d" % (cid, path("w24", K.cascade("w24")[0]), c, r, RC.BOUND_SF, c, r))
        casc_of[cid] = K.cascade("w24")[1]
    w12 = path("w12", K.cascade("w12")[0])
    # degenerate sizes (tests/test_lbp_roi_cpu.py's): the window is the image, a 1 x 1 image, one level, minSize / maxSize that leave one level or none
    for cid, cols, rows, sf, mins, maxs in DEGENERATE:
        lines.append("steps %s %s %d %d %r %d %d %d %d" % (cid, w12, cols, rows, sf, mins[0], mins[1], maxs[0], maxs[1]))
        casc_of[cid] = K.cascade("w12")[1]
    manifest = d / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([_build_driver(), str(manifest)], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "%d cases" % len(lines) in r.stderr
    return {a["case"]: a for a in (json.loads(ln) for ln in r.stdout.splitlines())}, dict((ln.split()[1], ln.split()) for ln in lines), casc_of


def test_constants_are_the_headers(answers):
    a = answers[0]["consts"]
    assert a["max_bytes"] == RC.MAX_BYTES == 122800 and a["short_win"] == RC.SHORT_WIN and a["vote_words"] == RC.VOTE_WORDS and a["max_win"] == RC.ROI_MAX_WIN
    assert a["fixed_bytes"] == RC.FIXED_BYTES == 40976 and a["weak_bytes"] == 80
    assert a["lev_bytes"] == RC.VOTE_WORDS * 4 + RC.ROI_MAX_WIN * 8                 # the level image's room: over votes + vnf
    assert a["max_bytes"] + a["fixed_bytes"] + 64 == 160 * 1024


def test_bound_is_the_stated_arithmetic(answers):
    a = answers[0]
    inside, outside = RC.bound_images()
    assert a["inside"] == dict(case="inside", fits=True, bytes=RC.image_bytes(*inside))
    assert a["outside"] == dict(case="outside", fits=False, bytes=RC.image_bytes(*outside))
    assert a["160x90"] == dict(case="160x90", fits=True, bytes=8 * 14652) and a["160x120"] == dict(case="160x120", fits=False, bytes=8 * 19484)
    assert a["1x1"] == dict(case="1x1", fits=True, bytes=32)


def _expected_steps(ref, cols, rows, sf, mins, maxs):
    ow, oh = ref.size
    lv = R.levels(ow, oh, cols, rows, sf, mins, maxs)
    e = dict(fits=len(lv) <= 63, levels=[], bands=[], plane_words=0, lev_bytes=0)
    if not e["fits"]:
        return e
    for li, (f, sz, win) in enumerate(lv):
        e["levels"].append([f, win[0], win[1]])
        step = 1 if f > 2.0 else 2
        nx, ny = len(range(0, sz[0] - ow, step)), len(range(0, sz[1] - oh, step))
        same, half = (sz[0], sz[1]) == (cols, rows), (2 * sz[0], 2 * sz[1]) == (cols, rows)
        mode = 0 if same else 2 if half else 1
        e["plane_words"] = max(e["plane_words"], (sz[0] + 1) * (sz[1] + 1))
        if not same:
            e["lev_bytes"] = max(e["lev_bytes"], sz[0] * sz[1])
        rows_per = max(1, RC.ROI_MAX_WIN // nx) if nx < RC.ROI_MAX_WIN else 1
        for gy0 in range(0, ny, rows_per):
            y0, y1 = gy0 * step, min(sz[1] - oh, (gy0 + rows_per) * step)
            e["bands"].append([li, sz[0], sz[1], step, mode, 0, sz[0] - ow, y0, y1, 0, step, y0, step])
    return e


def test_steps_bands_and_tables(answers):
    got, lines, casc_of = answers
    for cid, ln in lines.items():
        if ln[0] != "steps":
            continue
        ref = casc_of[cid]
        cols, rows, sf = int(ln[3]), int(ln[4]), float(ln[5])
        mins, maxs = (int(ln[6]), int(ln[7])), (int(ln[8]), int(ln[9]))
        a, e = got[cid], _expected_steps(ref, cols, rows, sf, mins, maxs)
        assert a["fits"] == e["fits"], cid
        if e["fits"]:
            assert a["levels"] == e["levels"] and a["plane_words"] == e["plane_words"] and a["lev_bytes"] == e["lev_bytes"], cid
            assert [b[:13] for b in a["bands"]] == e["bands"] and a["rows_fit"] and a["tabs_aligned"], cid
            for b in a["bands"]:          # a band fits the queues and the vnf array
                nx, ny = len(range(b[5], b[6], b[3])), len(range(b[7], b[8], b[3]))
                assert 0 < nx * ny <= RC.ROI_MAX_WIN, (cid, b)
            assert a["lds"] == RC.roi_lds_bytes(e["plane_words"]), cid
            if RC.fits_lds(cols, rows):         # the workgroup's LDS fits the CU's, and a resized level the room over votes + vnf
                assert a["lds"] <= 160 * 1024 - 64 and e["lev_bytes"] <= RC.VOTE_WORDS * 4 + RC.ROI_MAX_WIN * 8, cid
        else:
            assert a["levels"] == [] and a["bands"] == []
        # the cascade's table: stage records, zeros up to the 64-byte aligned weak records, 64 spare bytes behind the last
        ns, nw = len(ref.stage_sizes), len(ref.feature_idx)
        first = np.concatenate([[0], np.cumsum(ref.stage_sizes)])
        assert a["weak_off"] == (16 * ns + 63) // 64 * 64 and a["table_bytes"] == a["weak_off"] + 80 * nw + 64 and a["tail_bytes"] == 64 and a["slack"] == 0, cid
        assert [[s[0], s[1], np.float32(s[2]), s[3]] for s in a["stages"]] == [[int(first[i]), int(ref.stage_sizes[i]), ref.stage_thr[i], 0] for i in range(ns)], cid
        assert len(a["weak"]) == nw
        for k, w in enumerate(a["weak"]):
            f = int(ref.feature_idx[k])
            n = int(ref.rect_counts[f])
            assert w["rects"] == [[int(v) for v in ref.rects[f, r]] if r < n else [0, 0, 0, 0] for r in range(3)], (cid, k)          # rectangles (x, y, w, h); a missing one all zero
            assert [np.float32(v) for v in w["w"]] == [ref.weights[f, r] if r < n else np.float32(0) for r in range(3)], (cid, k)
            assert np.float32(w["thr"]) == ref.thr[k] and [np.float32(v) for v in w["leaf"]] == [v for v in ref.leaves[k]] and w["pad"] == 0, (cid, k)
    # the degenerate ones are what they are named for
    assert got["window-is-image"]["levels"] == [] and got["one-by-one"]["levels"] == [] and got["no-level-by-size"]["levels"] == []
    assert len(got["one-level"]["levels"]) == 1 and len(got["one-level"]["bands"]) == 1
    assert got["one-level-by-size"]["levels"] == [[1.99, 24, 24]]
    assert len(got["bands-w12-160x90"]["bands"]) > len(got["bands-w12-160x90"]["levels"])
    last = [b for b in got["last-band-one-row-w24-120x110"]["bands"] if b[0] == 0][-1]
    assert len(range(last[7], last[8], last[3])) == 1
    assert len(got["single-band-w12-97x83"]["bands"]) == len(got["single-band-w12-97x83"]["levels"])
    assert got["skip-chunk"]["bands"][0][:9] == [0, 2 * RC.N_COLS + 2, 8, 2, 0, 0, 2 * RC.N_COLS - 1, 0, 5] and len(got["skip-chunk"]["bands"]) == 1
    assert not got["too-many-levels"]["fits"]
    # features of one, two and three rects are among the records compared above
    counts = {int(casc_of[c].rect_counts[f]) for c in casc_of for f in casc_of[c].feature_idx}
    assert counts >= {2, 3}, counts
