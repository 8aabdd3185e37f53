"""The premises of tests/test_gpu_lbp_roi.py on the CPU, without the code under test: every constructed case of tests/lbp_roi_cases.py
is what the numpy statement (tests/lbp_reference.py) gives, and lies in the regime it is named for (a reject run across the 64-column
chunk, bands of whole rows, queues on both sides of the length that switches the lane mapping, images on both sides of the LDS bound).
And the pure host half of the route (csrc/lbp_roi_tables.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer:
tests/san/lbp_roi_tables_driver.cpp, a stand-alone program built as tests/test_lbp_tables_cpu.py builds its driver (no preload, nothing
loaded into Python; plan.cpp, whose build_resize_tab makes the levels' tables, reads the HIP headers, and what of it calls the runtime
is dropped at link time), prints the step records, bands and cascade table of each case; every field is compared with a statement written here from tests/lbp_reference.py and the record comments of csrc/device_records.h."""
import json
import os
import subprocess

import numpy as np
import pytest

import lbp_cases as K
import lbp_reference as R
import lbp_roi_cases as RC
from nubovca import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


# ------------------------------------------------------------------ the cases on the statement
@pytest.mark.parametrize("case", RC.hand_cases(), ids=[c[0] for c in RC.hand_cases()])
def test_hand_cases_are_the_statements(case):
    _, cdict, gray, sf, mins, maxs, exp = case
    ref = R.parse_xml(RC.hand_xml(cdict))
    assert R.scan(ref, gray, sf, mins, maxs).tolist() == exp
    rows, cols = gray.shape
    assert RC.fits_lds(cols, rows)


def test_reject_runs_cross_the_chunk_and_change_what_is_emitted():
    """one level of 67 grid columns; an odd run drops the column behind it, an even run does not; runs end at the chunk's last lane, one
    before it and one behind it"""
    for cid, g, exp in RC.skip_chunk_cases():
        assert RC.grid_of(3, 3, g.shape[1], g.shape[0], 4.0) == [(RC.N_COLS, g.shape[0] // 2 - 1)], cid
    by_end = {}
    for end, L in RC.RUNS:
        p, em = RC.run_row(end, L)
        assert (end + 1 in em) == (L % 2 == 0) and all(j in em for j in range(RC.N_COLS) if p[j] and j != end + 1)
        by_end.setdefault(end, set()).add(L % 2)
    assert by_end == {62: {0, 1}, 63: {0, 1}, 64: {0, 1}}
    assert {L for end, L in RC.RUNS if end == 63} >= {1, 2, 3, 4, 61, 62, 63, 64}
    assert RC.N_COLS > 64 + 2


def test_named_cases_are_in_their_regimes():
    G = {c[0]: RC.grid_of(*K.cascade(c[1])[1].size, c[2], c[3], c[4]) for c in RC.NAMED}
    g = G["bands-w12-160x90"]
    xml, gray, sf, exp, stats = RC.named_case("bands-w12-160x90")
    assert len(g) == 9 and g[0] == (74, 39) and 74 * 39 == 2886 > RC.ROI_MAX_WIN
    assert len(exp) == 436 and stats["skipped_pass"] == 127
    g = G["last-band-one-row-w24-120x110"]
    assert len(g) == 16 and g[0] == (48, 43) and RC.ROI_MAX_WIN // 48 == 42          # 42 rows, then a band of one
    assert len(RC.named_case("last-band-one-row-w24-120x110")[3]) > 0
    g = G["single-band-w12-97x83"]
    assert len(g) == 20 and max(nx * ny for nx, ny in g) == 1548 <= RC.ROI_MAX_WIN
    assert len(RC.named_case("single-band-w12-97x83")[3]) > 0
    for c in RC.NAMED:
        assert RC.fits_lds(c[2], c[3]), c
    assert not RC.haar_fits(160, 120) and RC.fits_lds(160, 120) and RC.haar_fits(160, 90)
    name, cols, rows, sf = RC.TOO_MANY_LEVELS
    assert len(RC.grid_of(*K.cascade(name)[1].size, cols, rows, sf)) > 63 and RC.fits_lds(cols, rows)


def test_deep_cascade_has_queues_on_both_sides_of_the_lane_mapping_switch():
    xml, gray, sf, exp, stats = RC.named_case("short-queues-deep-97x83")
    ref = K.cascade("deep")[1]
    depth = np.asarray(stats["depth"])
    alive = [int(np.count_nonzero((depth > 0) | (depth <= -s))) for s in range(9)]
    assert alive == [3344, 1962, 1287, 744, 409, 208, 134, 93, 70]
    q = RC.band_queue_lengths(ref, gray, sf)
    lengths = [n for band in q for n in band if n > 0]
    assert 0 < RC.SHORT_WIN and any(n > RC.SHORT_WIN for n in lengths) and any(n <= RC.SHORT_WIN for n in lengths), (RC.SHORT_WIN, sorted(lengths)[-5:])
    # the short form holds a stage's votes of a whole-wave-padded queue: every stage of the case's cascades fits at the switch length
    assert max(int(v) for n in ("w12", "w24", "w20x28", "deep") for v in K.cascade(n)[1].stage_sizes) * ((RC.SHORT_WIN + 63) // 64 * 64) <= RC.VOTE_WORDS
    assert len(exp) > 0


def test_bound_images_straddle_the_bound():
    inside, outside = RC.bound_images()
    assert RC.fits_lds(*inside) and not RC.fits_lds(*outside) and outside == (inside[0], inside[1] + 1)
    assert RC.roi_lds_total(*inside) <= 160 * 1024


# ------------------------------------------------------------------ the host half under sanitizers
def _build_driver():
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "lbp_roi_tables_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "lbp_roi_tables_driver.cpp")] + [os.path.join(csrc, f) for f in ("cascade_xml.cpp", "plan.cpp", "pyr_levels.cpp", "lbp_roi_tables.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        # (function sections, unused ones dropped: plan.cpp's table uploads call into the HIP runtime, which is not part of this driver)
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    d = tmp_path_factory.mktemp("lbp_roi")
    xmls = {}

    def path(name, text):
        if name not in xmls:
            xmls[name] = str(d / (name + ".xml"))
            open(xmls[name], "w").write(text)
        return xmls[name]

    inside, outside = RC.bound_images()
    lines = ["consts consts", "fits inside %d %d" % inside, "fits outside %d %d" % outside, "fits 160x120 160 120", "fits 160x90 160 90", "fits 1x1 1 1"]
    for cid, name, cols, rows, sf in RC.NAMED:
        lines.append("steps %s %s %d %d %r 0 0 %d %d" % (cid, path(name, K.cascade(name)[0]), cols, rows, sf, cols, rows))
    name, cols, rows, sf = RC.TOO_MANY_LEVELS
    lines.append("steps too-many-levels %s %d %d %r 0 0 %d %d" % (path(name, K.cascade(name)[0]), cols, rows, sf, cols, rows))
    w12 = path("w12", K.cascade("w12")[0])
    # degenerate sizes: the window is the image, a 1 x 1 image, one level, minSize / maxSize that leave one level or none
    for cid, cols, rows, sf, mins, maxs in (("window-is-image", 12, 12, 1.1, (0, 0), (12, 12)), ("one-by-one", 1, 1, 1.1, (0, 0), (1, 1)),
                                            ("one-level", 13, 13, 1.1, (0, 0), (13, 13)), ("one-level-by-size", 60, 60, 1.99, (24, 24), (24, 24)),
                                            ("no-level-by-size", 60, 60, 1.99, (25, 25), (30, 30)), ("inside-bound", inside[0], inside[1], 1.3, (0, 0), inside)):
        lines.append("steps %s %s %d %d %r %d %d %d %d" % (cid, w12, cols, rows, sf, mins[0], mins[1], maxs[0], maxs[1]))
    manifest = d / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([_build_driver(), str(manifest)], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "%d cases" % len(lines) in r.stderr
    return {a["case"]: a for a in (json.loads(ln) for ln in r.stdout.splitlines())}, dict((ln.split()[1], ln.split()) for ln in lines)


def test_constants_are_the_headers(answers):
    a = answers[0]["consts"]
    assert a["max_bytes"] == RC.MAX_BYTES and a["short_win"] == RC.SHORT_WIN and a["vote_words"] == RC.VOTE_WORDS and a["max_win"] == RC.ROI_MAX_WIN
    assert a["fixed_bytes"] == 2 * RC.ROI_MAX_WIN * 2 + 16 + RC.VOTE_WORDS * 4 and a["weak_bytes"] == 64
    assert a["max_bytes"] + a["fixed_bytes"] + 64 == 160 * 1024


def test_bound_is_the_stated_arithmetic(answers):
    a = answers[0]
    inside, outside = RC.bound_images()
    assert a["inside"] == dict(case="inside", fits=True, bytes=RC.image_bytes(*inside))
    assert a["outside"] == dict(case="outside", fits=False, bytes=RC.image_bytes(*outside))
    assert a["160x120"]["fits"] and a["160x120"]["bytes"] == 97136 and a["160x90"]["bytes"] == 73008 and a["1x1"]["fits"]


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
    got, lines = answers
    for cid, ln in lines.items():
        if ln[0] != "steps":
            continue
        name = next((c[1] for c in RC.NAMED if c[0] == cid), "w12")
        ref = K.cascade(name)[1]
        cols, rows, sf = int(ln[3]), int(ln[4]), float(ln[5])
        mins, maxs = (int(ln[6]), int(ln[7])), (int(ln[8]), int(ln[9]))
        a, e = got[cid], _expected_steps(ref, cols, rows, sf, mins, maxs)
        assert a["fits"] == e["fits"], cid
        if not e["fits"]:
            assert a["levels"] == [] and a["bands"] == []
            continue
        assert a["levels"] == e["levels"] and a["plane_words"] == e["plane_words"] and a["lev_bytes"] == e["lev_bytes"], cid
        assert [b[:13] for b in a["bands"]] == e["bands"] and a["rows_fit"] and a["tabs_aligned"], cid
        for b in a["bands"]:          # a band fits the queues, and the workgroup's LDS fits the CU's
            nx, ny = len(range(b[5], b[6], b[3])), len(range(b[7], b[8], b[3]))
            assert 0 < nx * ny <= RC.ROI_MAX_WIN, (cid, b)
        assert a["lds"] == RC.roi_lds_bytes(e["plane_words"], e["lev_bytes"]) <= 160 * 1024 - 64, cid
        first = np.concatenate([[0], np.cumsum(ref.stage_sizes)])
        assert a["weak_off"] == (16 * len(ref.stage_sizes) + 63) // 64 * 64 and a["table_bytes"] >= a["weak_off"] + 64 * len(ref.feature_idx)
        assert [[s[0], s[1], np.float32(s[2]), s[3]] for s in a["stages"]] == [[int(first[i]), int(ref.stage_sizes[i]), ref.stage_thr[i], 0] for i in range(len(ref.stage_sizes))], cid
        for k, w in enumerate(a["weak"]):
            assert w["rect"] == [int(v) for v in ref.rects[ref.feature_idx[k]]] and w["subset"] == [int(v) for v in ref.subsets[k]] and w["pad"] == 0, (cid, k)
            assert [np.float32(v) for v in w["leaf"]] == [v for v in ref.leaves[k]], (cid, k)
    # the degenerate ones are what they are named for
    assert got["window-is-image"]["levels"] == [] and got["one-by-one"]["levels"] == [] and got["no-level-by-size"]["levels"] == []
    assert len(got["one-level"]["levels"]) == 1 and len(got["one-level"]["bands"]) == 1
    assert got["one-level-by-size"]["levels"] == [[1.99, 24, 24]]
    assert len(got["bands-w12-160x90"]["bands"]) > len(got["bands-w12-160x90"]["levels"])
    last = [b for b in got["last-band-one-row-w24-120x110"]["bands"] if b[0] == 0][-1]
    assert len(range(last[7], last[8], last[3])) == 1
    assert len(got["single-band-w12-97x83"]["bands"]) == len(got["single-band-w12-97x83"]["levels"]) == 20
