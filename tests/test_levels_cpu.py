"""detectMultiScale with outputRejectLevels without a device: the numpy statement (tests/levels_reference.py) against
answers derived by hand (tests/levels_cases.py), the weighted groupRectangles of the library (csrc/group_levels.cpp) through its
AddressSanitizer + UndefinedBehaviorSanitizer driver (tests/san/group_levels_driver.cpp) against the statement, and the premises the GPU
tests rely on: every natural case has windows at each of the four emitted levels, a class with an equal-level tie and a class the level
rule drops; the overflow cases emit more than their capacity."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import levels_cases as K
import levels_reference as V
import orc
from nubovca import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _bits(w):
    return np.asarray(w, np.float64).view(np.uint64)


def _same(got, exp):
    return np.array_equal(np.asarray(got[0], np.int32).reshape(-1, 4), np.asarray(exp[0], np.int32).reshape(-1, 4)) and \
        np.array_equal(np.asarray(got[1], np.int32), np.asarray(exp[1], np.int32)) and np.array_equal(_bits(got[2]), _bits(exp[2]))


# ------------------------------------------------------------------ the ABI's new symbols
def test_the_library_exports_the_levels_entry_points():
    L = capi.load()
    assert "nvca_detect_raw_levels" in capi.SYMBOLS and "nvca_detect_multiscale_levels" in capi.SYMBOLS
    n = C.c_int()
    # argument refusals that need no context: n_out NULL, a negative capacity, an output array missing while cap > 0
    rects, lv, wt = (capi.Rect * 4)(), (C.c_int * 4)(), (C.c_double * 4)()
    for out in ((rects, lv, wt, 4, None), (rects, lv, wt, -1, C.byref(n)), (None, lv, wt, 4, C.byref(n)), (rects, None, wt, 4, C.byref(n)),
                (rects, lv, None, 4, C.byref(n))):
        assert L.nvca_detect_raw_levels(None, None, None, 8, 8, 8, capi.MEM_HOST, 1.1, 0, 0, 0, 0, 0, *out) == capi.ERR_ARG
        assert L.nvca_detect_multiscale_levels(None, None, None, 8, 8, 8, capi.MEM_HOST, 1.1, 3, 0, 0, 0, 0, 0, *out) == capi.ERR_ARG


# ------------------------------------------------------------------ the statement against hand-derived answers
@pytest.mark.parametrize("case", K.hand_cases(), ids=[c[0] for c in K.hand_cases()])
def test_hand_made_levels_and_weights(case):
    _, kind, cdict, gray, sf, rects, levels, weights = case
    got = V.scan_levels(K.parse(kind, K.to_xml(kind, cdict)), gray, sf)
    assert _same(got, (rects, levels, weights)), got


def test_a_cascade_of_three_stages_would_emit_stage0_rejects():
    """why fewer than four stages are refused: n + result < 4 holds for result 0"""
    for kind in (K.LBP, K.HAAR):
        c = K.const_cascade(kind, [(0.5, [-1.25]), (0.5, [2.25]), (0.5, [3.25])])
        got = V.scan_levels(K.parse(kind, K.to_xml(kind, c)), K.one_window_image(kind), 2.0)
        assert _same(got, (K.ONE, [0], [-1.25]))


@pytest.mark.parametrize("cid", sorted(K.NATURAL))
def test_level_n_is_the_plain_scan(cid):
    xml, ref, img, sf = K.natural(cid)
    rects, levels, _ = K.expected("natural", cid)
    plain = (V.H if V.is_haar(ref) else V.L).scan(ref, img, sf)
    assert len(plain) > 0 and np.array_equal(rects[levels == len(ref.stage_sizes)], plain)


# ------------------------------------------------------------------ grouping: the statement against hand-derived answers
@pytest.mark.parametrize("case", K.group_cases(), ids=[c[0] for c in K.group_cases()])
def test_group_levels_by_hand(case):
    _, rects, levels, weights, mn, er, el, ew = case
    assert _same(V.group_levels(rects, levels, weights, mn), (er, el, ew))


def test_classes_and_averages_are_the_plain_forms():
    """the statement's partition and averaging against the oracle's groupRectangles: kept by member count and filtered with both counts, the
    classes give the plain answer"""
    for seed in range(6):
        rects, _, _ = K.random_group_lists(seed, 60 + 40 * seed)
        labels, avg, counts = V.classes(rects)
        for thr in (1, 2, 3):
            keep = []
            for i in range(len(counts)):
                if counts[i] <= thr:
                    continue
                r1 = avg[i].astype(np.int64)
                for j in range(len(counts)):
                    if j == i or counts[j] <= thr:
                        continue
                    r2 = avg[j].astype(np.int64)
                    dx, dy = V.L.cv_round(float(r2[2]) * 0.2), V.L.cv_round(float(r2[3]) * 0.2)
                    if r1[0] >= r2[0] - dx and r1[1] >= r2[1] - dy and r1[0] + r1[2] <= r2[0] + r2[2] + dx and r1[1] + r1[3] <= r2[1] + r2[3] + dy and \
                       (counts[j] > max(3, counts[i]) or counts[i] < 3):
                        break
                else:
                    keep.append(i)
            exp, w = orc.group_rectangles(rects, thr, 0.2)
            assert np.array_equal(avg[keep].reshape(-1, 4), np.asarray(exp, np.int32).reshape(-1, 4)) and list(counts[keep]) == list(w)


# ------------------------------------------------------------------ the C++ unit, through its sanitizer driver
def _build_driver():
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "group_levels_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "group_levels_driver.cpp")] + [os.path.join(csrc, f) for f in ("group_levels.cpp", "host_logic.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in ("group_levels.h", "host_logic.h", "pixel_rules.h")] + [os.path.join(ROOT, "include", "nubovca.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


def _driver_cases():
    """id -> (rects, levels, weights, minNeighbors): the hand cases and seeded random lists, n = 0 and one-member inputs among them"""
    cases = {c[0]: (c[1], c[2], c[3], c[4]) for c in K.group_cases()}
    for seed, n in enumerate((0, 1, 1, 2, 7, 40, 150, 400, 900)):
        r, l, w = K.random_group_lists(100 + seed, n)
        for mn in (1, 3, 5):
            cases["random-%d-n%d-mn%d" % (seed, n, mn)] = (r, l, w, mn)
    return cases


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    tmp = tmp_path_factory.mktemp("group_levels")
    driver = _build_driver()
    lines = []
    for cid, (r, l, w, mn) in _driver_cases().items():
        r = np.asarray(r, np.int64).reshape(-1, 4)
        lines.append("case %s %d 0.2 %d" % (cid, mn, len(r)))
        for i in range(len(r)):
            lines.append("%d %d %d %d %d %d" % (r[i, 0], r[i, 1], r[i, 2], r[i, 3], int(l[i]), int(_bits([w[i]])[0])))
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
    return got


def test_the_library_groups_as_the_statement(driver_output):
    cases = _driver_cases()
    assert set(driver_output) == set(cases) | {"unequal-lengths"}
    kept = 0
    for cid, (r, l, w, mn) in cases.items():
        o = driver_output[cid]
        er, el, ew = V.group_levels(r, l, w, mn)
        assert o["ok"] and np.array_equal(np.asarray(o["rects"], np.int32).reshape(-1, 4), er), cid
        assert np.array_equal(np.asarray(o["levels"], np.int32), el) and np.array_equal(np.asarray(o["weights"], np.uint64), _bits(ew)), cid
        kept += len(er)
    assert kept > 20          # (no comparison of empty lists alone)
    o = driver_output["unequal-lengths"]
    assert not o["ok"] and o["rects"] == [[1, 2, 3, 4]] * 3 and o["levels"] == [5, 5] and len(o["weights"]) == 3


# ------------------------------------------------------------------ premises of the GPU cases
def _tie_and_drop(rects, levels, weights, mn):
    """(classes with two or more members at their maxLevel whose weights differ, classes the level rule drops that the count rule would keep or
    not -- any class with maxLevel <= mn)"""
    labels, _, counts = V.classes(rects)
    ties = drops = 0
    for c in range(len(counts)):
        lv, wt = levels[labels == c], weights[labels == c]
        top = wt[lv == lv.max()]
        ties += len(top) >= 2 and len(np.unique(top)) >= 2
        drops += lv.max() <= mn
    return ties, drops


@pytest.mark.parametrize("cid", sorted(K.NATURAL))
def test_natural_cases_reach_every_level_a_tie_and_the_level_rule(cid):
    xml, ref, img, sf = K.natural(cid)
    n = len(ref.stage_sizes)
    rects, levels, weights = K.expected("natural", cid)
    assert n >= 4 and set(levels.tolist()) == set(K.THREE_LEVELS.get(cid, (n - 3, n - 2, n - 1, n)))
    mn = K.group_thresholds(ref)[-1]
    ties, drops = _tie_and_drop(rects, levels, weights, mn)
    assert ties >= 1 and drops >= 1
    g = V.group_levels(rects, levels, weights, mn)
    assert 0 < len(g[0]) < len(V.classes(rects)[2])


@pytest.mark.parametrize("route", K.HI)
def test_hi_plane_cases_emit_rejected_and_passing_windows(route):
    xml, ref, img, sf = K.hi_planes(route)
    rects, levels, weights = K.expected("hi", route)
    n = len(ref.stage_sizes)
    assert n == len(K.HI_STAGES) and n in levels and len(set(levels.tolist())) >= 3
    # (what makes the images a case of their route is the image's own: tests/test_haar_new_cpu.py.)  The grouped comparison is not empty either:
    cls = V.classes(rects)
    assert 0 < len(V.group_levels(rects, levels, weights, n - 1, cls=cls)[0]) < len(cls[2])


@pytest.mark.parametrize("kind", [K.LBP, K.HAAR])
def test_overflow_cases_emit_more_than_their_capacity(kind):
    rects, levels, weights = K.expected("overflow", kind)
    assert len(rects) > 4 * 256 and set(levels.tolist()) == {3, 4}
    assert min(np.count_nonzero(levels == 3), np.count_nonzero(levels == 4)) > 256
