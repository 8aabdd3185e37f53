"""The premises of tests/test_gpu_lbp_streams.py, asserted on the statement alone (tests/lbp_stream_cases.py: the numpy LBP reference
between the oracle's gate and finish), so that no case can drift out of the regime it is there for: which branch of k_group a frame's
candidates reach (256 and 2048 are its thresholds, kernels_group.hip), that boxes come out where a comparison needs some, that the raw
lists change when equalisation is left out (a pyramid that forgets the LUT fails), and that the sequences hold what their tests name.
And the tables k_group reads on an LBP scan (csrc/lbp_tables.cpp), through the C++ built on the CPU (tests/san/lbp_group_tables_driver.cpp,
AddressSanitizer + UndefinedBehaviorSanitizer, a stand-alone program): every candidate key of three plans maps to the rectangle
DetectPlan::hit_rect's arithmetic gives."""
import json
import os
import subprocess

import numpy as np
import pytest

import lbp_reference as R
import lbp_stream_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
RANK_SORT_MAX, GROUP_MAX = 256, 2048            # k_group: rank sort up to 256 candidates, bitonic network above; host grouping above 2048

# (raw candidates, boxes at min_neighbors 3) per frame, as the statement answers
TABLE = {
    "identity": ([80, 89, 89], [3, 4, 3]),
    "half": ([41, 57, 48], [1, 4, 3]),
    "bilinear": ([41, 42, 24, 11, 41, 37], [2, 3, 2, 0, 0, 3]),
    "bitonic": ([749, 699, 658], [16, 15, 16]),
    "odd": ([291, 263, 277], [13, 11, 7]),
    "wide": ([105, 150, 118], [8, 12, 12]),
    "deep": ([5, 6, 5], [0, 0, 0]),
}


def _counts(cid):
    name, _W, _H, wtp, pct, _seeds = S.CASES[cid]
    fr = S.frames_of(S.CASES[cid])
    return [len(S.raw(name, f, wtp, pct)) for f in fr], [len(S.detections(name, f, wtp, pct, 3)) for f in fr]


@pytest.mark.parametrize("cid", sorted(S.CASES))
def test_cases_answer_what_their_table_says(cid):
    assert _counts(cid) == TABLE[cid]


def test_cases_lie_in_their_regimes():
    raw = {cid: TABLE[cid][0] for cid in TABLE}
    for cid in ("identity", "half", "bilinear", "wide", "deep"):
        assert 0 < min(raw[cid]) and max(raw[cid]) <= RANK_SORT_MAX, cid
    assert RANK_SORT_MAX < min(raw["bitonic"]) and max(raw["bitonic"]) <= GROUP_MAX
    assert RANK_SORT_MAX < min(raw["odd"]) <= GROUP_MAX                           # several bit words a row AND the bitonic branch
    for cid in ("identity", "half", "bitonic", "odd", "wide"):
        assert min(TABLE[cid][1]) > 0, cid
    # geometry: identity, exact 2x (area), 4x (bilinear), levels wider than 1023, an odd pitch
    assert S.geometry(160, 120, 160) == (160, 120, 1) and S.geometry(320, 240, 160) == (160, 120, 2) and S.geometry(640, 480, 160) == (160, 120, 4)
    assert S.geometry(1500, 240, 1500) == (1500, 240, 1) and S.geometry(333, 251, 333) == (333, 251, 1)
    # minSize (cols // 20, rows // 20) keeps a level only from a window 75 wide on: a 24-pixel window's first level is 404 wide, so the
    # "wide" case's levels all go through the one-launch pyramid; the 78-pixel window's first two levels are wider than 1023
    assert max(sz[0] for _f, sz, _w in R.levels(24, 24, 1500, 240, 1.3, (75, 12))) == 404
    lv = R.levels(78, 78, 1500, 240, 1.3, (75, 12))
    assert [sz[0] for _f, sz, _w in lv][:3] == [1500, 1154, 888] and len(lv) == 5
    assert len(R.levels(24, 24, 160, 120, 1.25, (8, 6))) > 3
    # bit words a row (32 grid columns each, step 2 on the first level): 64 x 48 under the 12 x 12 window one, 160 wide three, 333 wide five
    assert [-(-len(range(0, w - ow, 2)) // 32) for w, ow in ((64, 12), (160, 24), (333, 24))] == [1, 3, 5]


def test_deep_cascade_groups_to_one_box_at_min_neighbors_1():
    name, _W, _H, wtp, pct, _ = S.CASES["deep"]
    fr = S.frames_of(S.CASES["deep"])
    assert [len(S.detections(name, f, wtp, pct, 1)) for f in fr] == [1, 1, 1]
    assert [len(S.detections(name, f, wtp, pct, 0)) for f in fr] == TABLE["deep"][0]
    assert len(S.cascade("deep")[1].stage_sizes) == 20


def test_raw_lists_change_without_equalisation():
    name, _W, _H, wtp, pct, _ = S.CASES["identity"]
    fr = S.frames_of(S.CASES["identity"])
    plain = [S.raw(name, f, wtp, pct, 0, False) for f in fr]
    assert [len(p) for p in plain] == [90, 94, 91]
    for f, p in zip(fr, plain):
        e = S.raw(name, f, wtp, pct)
        assert p.shape != e.shape or not np.array_equal(p, e)
    # and the working image is what the lists are about: the equalised one differs from the plain one
    assert not np.array_equal(S.working(fr[0], wtp), S.working(fr[0], wtp, 0, False))


def test_sequence_with_two_empty_analysed_frames_in_a_row():
    """frames 4 and 5 of the 640 x 480 sequence have no box: the first keeps the faces (hysteresis), the second clears them, and the ids
    go on counting afterwards; at process_x_every_4 2 only every other frame is analysed and neither empty frame is met twice in a row"""
    name, _W, _H, wtp, _pct, _ = S.CASES["bilinear"]
    fr = S.frames_of(S.CASES["bilinear"])
    seq = S.expected_sequence(name, fr, width_to_process=wtp, process_x_every_4=4)
    assert [len(b) for b, _ in seq] == [2, 3, 2, 2, 0, 3]
    assert np.array_equal(seq[3][0], seq[2][0]) and np.array_equal(seq[3][1], seq[2][1])        # kept over the first empty frame
    assert seq[5][1].min() > max(i.max() for _b, i in seq[:4])                                   # new faces after the clear
    assert all((b[:, 2] % 4 == 0).all() for b, _ in seq if len(b))                               # boxes in frame pixels: norm_scale 4
    seq2 = S.expected_sequence(name, fr, width_to_process=wtp, process_x_every_4=2)
    assert [len(b) for b, _ in seq2] == [2, 2, 2, 2, 2, 2] and not np.array_equal(seq2[2][0], seq[2][0])


def test_many_small_streams_all_answer():
    name, _W, _H, wtp, pct, seeds = S.MANY
    n = [len(S.detections(name, f, wtp, pct, 3)) for f in S.frames_of(S.MANY)]
    assert len(seeds) == 33 and min(n) >= 2 and max(n) <= 5
    assert len({S.raw(name, f, wtp, pct).tobytes() for f in S.frames_of(S.MANY)}) == 33           # a slot mix-up changes an answer


def test_wide_window_case():
    name, _W, _H, wtp, pct, _ = S.WIN78
    fr = S.frames_of(S.WIN78)
    assert [(len(S.raw(name, f, wtp, pct)), len(S.detections(name, f, wtp, pct, 3))) for f in fr] == [(498, 20), (230, 16)]      # either sort branch
    assert all(not np.array_equal(S.raw(name, f, wtp, pct), S.raw(name, f, wtp, pct, 0, False)) for f in fr)                      # the LUT matters


def test_empty_and_ungrouped_slots():
    assert len(S.raw("w24", S.FLAT, 160, 25)) == 0
    assert [(len(S.raw("w24", f, 160, 25)), len(S.detections("w24", f, 160, 25, 3))) for f in S.NATURAL] == [(20, 0), (24, 0)]


def test_overflow_case_is_above_the_device_grouping_limit():
    n = [len(S.raw(S.CODE255, f, 160, 25)) for f in (S.FLAT, ("natural", 160, 120, 5), ("ramp", 160, 120))]
    assert n == [8346, 501, 232]
    assert n[0] > GROUP_MAX and n[0] > 256 + 64                # k_group declines; a capacity of 256 a frame overflows
    assert RANK_SORT_MAX < n[1] <= GROUP_MAX and n[2] <= RANK_SORT_MAX
    assert len(S.detections(S.CODE255, S.FLAT, 160, 25, 3)) > 0


def test_neutral_chroma_frames_are_gray():
    """the 4:2:0 cases: the statement's BGR of a frame with neutral chroma has three equal channels (limited-range luma, so not the luma
    plane itself), and the stream's expected lists on it are no empty comparison"""
    f = S.frames_of(S.CASES["identity"])[0]
    for fmt in (1, 2):
        b = S.bgr(f, fmt)
        assert np.array_equal(b[..., 0], b[..., 1]) and np.array_equal(b[..., 1], b[..., 2]) and not np.array_equal(b[..., 0], S.gray(f))
        assert len(S.detections("w24", f, 160, 25, 3, fmt)) > 0
    assert np.array_equal(S.bgr(f, 1), S.bgr(f, 2))


# ------------------------------------------------------------------ the grouping tables, through the C++
PLANS = [("identity", "w24", 160, 120, 1.25), ("bitonic", "w20x28", 160, 120, 1.10), ("wide", "w24", 1500, 240, 1.30)]


def _build_driver():
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "lbp_group_tables_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "lbp_group_tables_driver.cpp")] + [os.path.join(csrc, f) for f in ("cascade_xml.cpp", "pyr_levels.cpp", "lbp_tables.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in ("cascade_model.h", "device_records.h", "pyr_levels.h", "lbp_tables.h", "host_math.h")] + [os.path.join(ROOT, "include", "nubovca.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    tmp = tmp_path_factory.mktemp("lbp_group_tables")
    driver = _build_driver()
    lines = []
    for cid, name, cols, rows, sf in PLANS:
        path = str(tmp / (name + ".xml"))
        with open(path, "w") as f:
            f.write(S.cascade(name)[0])
        lines.append("scan %s %s %d %d %r %d %d %d %d" % (cid, path, cols, rows, sf, cols // 20, rows // 20, cols, rows))      # as face_submit asks for the plan
    manifest = str(tmp / "manifest.txt")
    with open(manifest, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver, manifest], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("{"):
            o = json.loads(ln)
            got[o.pop("case")] = o
    assert len(got) == len(lines)
    return got


@pytest.mark.parametrize("plan", PLANS, ids=[p[0] for p in PLANS])
def test_every_key_maps_to_hit_rects_rectangle(tables, plan):
    """k_group rebuilds a candidate (level, gy, gx) as pos[xpos_off + gx], pos[ypos_off + gy], winw, winh; hit_rect as cvRound(gx * step * f),
    cvRound(gy * step * f), cvRound(ow * f), cvRound(oh * f) -- for EVERY key of the plan, and the tables hold nothing else"""
    cid, name, cols, rows, sf = plan
    t = tables[cid]
    ow, oh = S.cascade(name)[1].size
    lv = R.levels(ow, oh, cols, rows, sf, (cols // 20, rows // 20))
    assert t["rc"] == 0 and len(lv) == len(t["levels"]) == len(t["scales"]) and t["rest_zero"]
    pos, off, nkeys = t["pos"], 0, 0
    for (f, sz, win), (tf, step, nx, ny), sc in zip(lv, t["levels"], t["scales"]):
        assert tf == f and step == (1 if f > 2.0 else 2)
        assert (nx, ny) == (len(range(0, sz[0] - ow, step)), len(range(0, sz[1] - oh, step)))          # the grid of lbp_reference.scan
        winw, winh, endx, endy, xoff, yoff, _plane, _pitch, factor = sc
        assert (winw, winh, endx, endy, factor) == (win[0], win[1], nx, ny, f)
        assert (xoff, yoff) == (off, off + nx)                                                          # level after level, columns then rows
        assert pos[xoff:xoff + nx] == [R.cv_round(gx * step * f) for gx in range(nx)]
        assert pos[yoff:yoff + ny] == [R.cv_round(gy * step * f) for gy in range(ny)]
        off += nx + ny
        nkeys += nx * ny
        assert nx <= 1 << t["key_sy"] and ny <= 1 << (t["key_ss"] - t["key_sy"])                       # every gx, gy fits its key field
    assert off == len(pos) and nkeys > 0 and len(lv) <= 1 << (32 - t["key_ss"])
    if cid == "wide":
        assert t["levels"][0][2] > 32 * 8                   # many bit words a row
    # a half-way coordinate exists somewhere: cvRound's round-half-to-even is exercised (12 * 1.25 = 15 is exact; 2 * 1.25 = 2.5 -> 2)
    if cid == "identity":
        f1 = lv[1][0]
        assert f1 == 1.25 and 2 * f1 == 2.5 and pos[t["scales"][1][4] + 1] == 2
