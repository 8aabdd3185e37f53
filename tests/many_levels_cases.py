"""Pyramid scans of more than 63 levels: the cases that tests/test_many_levels_cpu.py (on the statements alone) and
tests/test_gpu_many_levels.py (on the device) share.  The large-image routes once stopped building levels after the 63rd and answered
NVCA_OK from the levels they had; the levels lost were the largest windows.  Every expected list here is a statement's --
tests/lbp_reference.py, tests/haar_new_reference.py, tests/levels_reference.py, the C oracle for old-format cascades -- never a run of
the library.  by_level() walks the statement's own pieces level by level, so that a window can be counted by the index of its level and
the scan can be cut after KEPT levels: the mutation the device tests have to catch.  The CPU test asserts that by_level() put together
is the statement's list, and that every case loses windows under the cut."""
import functools

import numpy as np

import haar_new_cases as HK
import haar_new_reference as HR
import haar_new_stream_cases as HS
import lbp_cases as LK
import lbp_reference as LR
import lbp_stream_cases as LS
import levels_reference as LV
import orc
from nubovca import synth

LBP, HAAR = "lbp", "haar"
KEPT = 63            # levels the large routes used to build
CASES_OF = {LBP: LK, HAAR: HK}
STATEMENT = {LBP: LR, HAAR: HR}


def cascade(kind, name):
    """(xml text, the reference reader's cascade)"""
    return CASES_OF[kind].cascade(name)


def image(kind, cols, rows, size, seed=11):
    """haar_new_cases.image for either format: both formats scan the same picture"""
    return HK.image(cols, rows, size[0], size[1], seed)


def by_level(kind, ref, gray, sf, min_size=(0, 0), max_size=(0, 0)):
    """the statement's raw list, one [n, 4] int32 array per level of the statement's level list: the loop of lbp_reference.scan /
    haar_new_reference.scan on their own pieces (levels, grid_results, walk_row)"""
    gray = np.ascontiguousarray(gray, np.uint8)
    rows, cols = gray.shape
    ow, oh = ref.size
    out = []
    for factor, sz, win in LR.levels(ow, oh, cols, rows, sf, min_size, max_size):
        lev = gray if (sz[0], sz[1]) == (cols, rows) else orc.resize_linear(gray, sz[0], sz[1])
        S, Q = orc.integral(lev)
        step = 1 if factor > 2.0 else 2
        xs, ys = np.arange(0, sz[0] - ow, step), np.arange(0, sz[1] - oh, step)
        res = HR.grid_results(ref, S, Q, xs, ys) if kind == HAAR else LR.grid_results(ref, S, xs, ys)
        rects = []
        for iy, y in enumerate(ys):
            for ix in LR.walk_row(res[iy]):
                if res[iy, ix] > 0:
                    rects.append((LR.cv_round(xs[ix] * factor), LR.cv_round(y * factor), win[0], win[1]))
        out.append(np.asarray(rects, np.int32).reshape(-1, 4))
    return out


def joined(per_level):
    return np.concatenate(per_level).reshape(-1, 4) if per_level else np.zeros((0, 4), np.int32)


def grouped(raw, mn):
    """groupRectangles as detectMultiScale calls it: the oracle's, on a statement's raw list"""
    raw = np.asarray(raw, np.int32).reshape(-1, 4)
    if mn == 0 or len(raw) == 0:
        return raw
    return np.asarray(orc.group_rectangles(raw, max(mn, 1), 0.2)[0], np.int32).reshape(-1, 4)


GROUP_THRESHOLDS = (2, 3)

# ------------------------------------------------------------------ new-format cascades, single images
# id -> (kind, cascade, cols, rows, sf, levels of the statement, its raw windows, those of them in levels 63 and up counted by level).
# The smallest shapes at which the bound is crossed: the 12 x 12 window on 97 x 83 at 1.02, the 24 x 24 window on the face element's
# 160 x 120 working image at its multi-scale-factor 2 and 1.
SINGLE = {
    "haar-w12-97x83-1.02": (HAAR, "w12", 97, 83, 1.02, 96, 1305, 6), "haar-w24-160x120-1.02": (HAAR, "w24", 160, 120, 1.02, 81, 3106, 10),
    "haar-w24-160x120-1.01": (HAAR, "w24", 160, 120, 1.01, 160, 6115, 1400),
    "lbp-w12-97x83-1.02": (LBP, "w12", 97, 83, 1.02, 96, 2413, 171), "lbp-w24-160x120-1.02": (LBP, "w24", 160, 120, 1.02, 81, 1028, 72),
    "lbp-w24-160x120-1.01": (LBP, "w24", 160, 120, 1.01, 160, 2094, 1260),
}
LAYOUTS = ("haar-w12-97x83-1.02", "lbp-w12-97x83-1.02")          # also run from device memory


@functools.lru_cache(maxsize=None)
def single(cid, seed=11):
    """(xml, reference cascade, image, sf, the statement's raw list)"""
    kind, name, cols, rows, sf = SINGLE[cid][:5]
    xml, ref = cascade(kind, name)
    gray = image(kind, cols, rows, ref.size, seed)
    exp = STATEMENT[kind].scan(ref, gray, sf)
    exp.setflags(write=False)
    return xml, ref, gray, sf, exp


@functools.lru_cache(maxsize=None)
def single_by_level(cid, seed=11):
    _xml, ref, gray, sf, _exp = single(cid, seed)
    return by_level(SINGLE[cid][0], ref, gray, sf)


# ------------------------------------------------------------------ the boundary: 63, 64 and 65 levels
# kind -> (cascade, cols, rows, sf, min_size, three max_size).  LBP: the 12 x 12 window on 97 x 83 at 1.02 has 96 levels, with windows
# of cvRound(12 * 1.02^k).  min_size (17, 17) drops the levels whose windows are 12 .. 16 wide; the three max_size values end the scan behind
# windows 57, 59 and 60 wide, each width one level's alone, so the statement has exactly 63, 64 and 65 levels and the three scans differ in
# max_size only.  HAAR: that image leaves the last of 63 levels without a window under every such cut, so the 24 x 24 window on 160 x 120
# at 1.01 (160 levels): min_size (41, 41), windows 75, 76 and 77.  boundary_search() looks for such cuts (on the CPU; what it found is
# written down here); tests/test_many_levels_cpu.py asserts that these two are among them.
BOUNDARY = {LBP: ("w12", 97, 83, 1.02, (17, 17), ((57, 57), (59, 59), (60, 60))),
            HAAR: ("w24", 160, 120, 1.01, (41, 41), ((75, 75), (76, 76), (77, 77)))}
BOUNDARY_LEVELS = (63, 64, 65)


def boundary_search(kind, name, cols, rows, sf):
    """every (min_size, three max_size) of square sizes under which the statement has exactly 63, 64 and 65 levels, the scans differ in
    max_size only, and the last level of each holds a window"""
    xml, ref = cascade(kind, name)
    ow, oh = ref.size
    per = by_level(kind, ref, image(kind, cols, rows, ref.size), sf)
    wins = [w for _, _, w in LR.levels(ow, oh, cols, rows, sf)]
    found = []
    for first in range(len(wins) - 65 + 1):
        if first and wins[first - 1] == wins[first]:
            continue          # min_size cannot cut between two levels of one window
        last = [first + n - 1 for n in BOUNDARY_LEVELS]
        if any(k + 1 < len(wins) and wins[k + 1] == wins[k] for k in last) or any(len(per[k]) == 0 for k in last):
            continue
        found.append((wins[first], tuple(wins[k] for k in last)))
    return found


def boundary_found(kind):
    name, cols, rows, sf, _mins, _maxs = BOUNDARY[kind]
    return boundary_search(kind, name, cols, rows, sf)


@functools.lru_cache(maxsize=None)
def boundary(kind):
    """(xml, reference cascade, image, sf, min_size, [(max_size, the statement's raw list)] x 3)"""
    name, cols, rows, sf, mins, maxs = BOUNDARY[kind]
    xml, ref = cascade(kind, name)
    gray = image(kind, cols, rows, ref.size)
    return xml, ref, gray, sf, mins, [(m, STATEMENT[kind].scan(ref, gray, sf, mins, m)) for m in maxs]


# ------------------------------------------------------------------ old-format cascades, CV_HAAR_SCALE_IMAGE
# The synthetic cascades of tests/test_gpu_parity.py (conftest's synth_xml and small_xml) on ONE 160 x 120 image with one template face 100
# pixels wide: a 100-pixel window is level 81 of the 20-pixel cascades' 1.02 ladder and level 162 of the 1.01 one.  (FIND_BIGGEST | SCALE_IMAGE is not
# here: make_detect_job drops SCALE_IMAGE under FIND_BIGGEST, as cvHaarDetectObjectsForROC does, and the search goes through fb_search.cpp,
# whose ladder never had the bound.)
OLD_IMAGE = (160, 120, 9, "natural", ((30, 10, 100),))
# (sf, min_size).  The 20-pixel window has one size, 37, at levels 62 and 63 of the 1.01 ladder: no max_size ends the scan between them, and
# the CPU test could not cut it after 63 levels.  min_size (21, 21) drops levels 0 .. 2; levels 62 and 63 of what is left are 38 and 39 wide.
OLD_SCANS = ((1.02, (0, 0)), (1.01, (21, 21)))
OLD_CASCADES = ("synth", "small")


@functools.lru_cache(maxsize=None)
def old_xml(which):
    return synth.synthetic_cascade_xml() if which == "synth" else synth.synthetic_cascade_xml(seed=7, stages=[3, 8, 12, 16, 20, 24])


@functools.lru_cache(maxsize=None)
def old_cascade(which):
    return orc.parse_cascade_xml(old_xml(which))


@functools.lru_cache(maxsize=None)
def old_image():
    cols, rows, seed, kind, faces = OLD_IMAGE
    g = orc.equalize_hist(synth.make_gray(cols, rows, seed, kind, list(faces)))
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def old_case(which, sf, mins):
    """(the oracle's raw list, its level count)"""
    raw, st = orc.detect_raw(old_cascade(which), old_image(), sf, orc.HAAR_SCALE_IMAGE, mins, return_stats=True)
    return raw, int(st.n_scales)


def old_first_levels(which, sf, mins, n=KEPT):
    """the oracle's raw list of the first n levels alone: the scan under the max_size that ends it behind level n - 1 (found by its level
    count), or None where levels n - 1 and n have one window size and no max_size separates them"""
    c = old_cascade(which)
    for side in range(c.ow, max(OLD_IMAGE[:2]) + 1):
        m = (side, side * c.oh // c.ow + 1)
        raw, st = orc.detect_raw(c, old_image(), sf, orc.HAAR_SCALE_IMAGE, mins, m, return_stats=True)
        if st.n_scales == n:
            return raw
        if st.n_scales > n:
            return None
    return None


# ------------------------------------------------------------------ batches: two different images in one call
BATCH = {LBP: "lbp-w12-97x83-1.02", HAAR: "haar-w12-97x83-1.02"}
BATCH_SEEDS = (11, 23)


def batch(kind):
    """(xml, reference cascade, [image], sf, [the statement's raw list])"""
    one = [single(BATCH[kind], s) for s in BATCH_SEEDS]
    return one[0][0], one[0][1], [o[2] for o in one], one[0][3], [o[4] for o in one]


# ------------------------------------------------------------------ reject levels and level weights
LEVELS = {LBP: "lbp-w12-97x83-1.02", HAAR: "haar-w12-97x83-1.02"}          # five and nine stages
LEVELS_THRESHOLDS = {LBP: (3, 4), HAAR: (3, 8)}                            # min_neighbors of the weighted grouping: 3 and nstages - 1 (levels_cases.group_thresholds)


@functools.lru_cache(maxsize=None)
def levels_case(kind):
    """(xml, reference cascade, image, sf, the statement's (rects, reject levels, level weights))"""
    xml, ref, gray, sf, _ = single(LEVELS[kind])
    return xml, ref, gray, sf, LV.scan_levels(ref, gray, sf)


def levels_by_level(kind):
    """the statement's triples, one (rects, reject levels, level weights) per level: the loop of levels_reference.scan_levels on its
    own pieces (grid_levels, walk_row)"""
    _, ref, gray, sf, _ = levels_case(kind)
    rows, cols = gray.shape
    ow, oh = ref.size
    n = len(ref.stage_sizes)
    out = []
    for factor, sz, win in LR.levels(ow, oh, cols, rows, sf):
        lev = gray if (sz[0], sz[1]) == (cols, rows) else orc.resize_linear(gray, sz[0], sz[1])
        S, Q = orc.integral(lev)
        step = 1 if factor > 2.0 else 2
        xs, ys = np.arange(0, sz[0] - ow, step), np.arange(0, sz[1] - oh, step)
        res, gyp = LV.grid_levels(ref, S, Q, xs, ys)
        rects, levels, weights = [], [], []
        for iy, y in enumerate(ys):
            for ix in LR.walk_row(res[iy]):
                result = -n if res[iy, ix] == 1 else int(res[iy, ix])
                if n + result < 4:
                    rects.append((LR.cv_round(xs[ix] * factor), LR.cv_round(y * factor), win[0], win[1]))
                    levels.append(-result)
                    weights.append(gyp[iy, ix])
        out.append((np.asarray(rects, np.int32).reshape(-1, 4), np.asarray(levels, np.int32), np.asarray(weights, np.float64)))
    return out


# ------------------------------------------------------------------ face streams at multi-scale-factor 1 and 2
# (cascade, frame width, height, width_to_process, seeds) and the multi_scale_factor of every frame: 160 and 81 levels on the 160 x 120
# working image under the stream's min_size (8, 6), which drops none.  The third frame is the second again, at the second's factor: it
# meets the plan the second frame built, and the ids carry what the stream saw -- a third picture would cost the statement another scan
# and reach nothing more.
STREAM = {LBP: ("w24", 160, 120, 160, (11, 12, 12)), HAAR: ("w24", 160, 120, 160, (11, 12, 12))}
STREAM_PCT = (1, 2, 2)
STREAM_CASES = {LBP: LS, HAAR: HS}


def stream_frames(kind):
    name, W, H, _wtp, seeds = STREAM[kind]
    return [("lbp" if kind == LBP else "hnew", name, W, H, s) for s in seeds]


def stream_expected(kind):
    """a fresh expected stream (lbp_stream_cases.Expected / haar_new_stream_cases.Expected)"""
    name, _W, _H, wtp, _ = STREAM[kind]
    return STREAM_CASES[kind].Expected(name, width_to_process=wtp, scale_factor_pct=STREAM_PCT[0], min_neighbors=3)


def stream_working(kind, frame):
    """the equalised working image of a frame and the stream's min_size"""
    M = STREAM_CASES[kind]
    img = M.bgr(frame)
    cols, rows, _ = LS.geometry(img.shape[1], img.shape[0], STREAM[kind][3])
    w = orc.equalize_hist(orc.bgr2gray(orc.resize_linear(np.array(img), cols, rows)))
    return w, (cols // 20, rows // 20)


def stream_raw(kind, frame, pct):
    """the statement's raw list of an analysed frame (computed once a frame and factor)"""
    return STREAM_CASES[kind].raw(STREAM[kind][0], frame, STREAM[kind][3], pct)


# ------------------------------------------------------------------ a part stream whose face cascade is LBP
# lbp_part_cases' nose stream (every role LBP) on its 320 x 240 frames at scale_factor_pct 2: the face pass scans the 160 x 120 face
# image at 1.02 with min_size (3, 3) -- 81 levels, with windows beyond the 63rd on either frame (58 and 25 of them).  The eye stream's
# face pass has min_size (30, 30) and 70 levels; one kind is enough.
PART_KIND, PART_FRAME, PART_FRAMES, PART_PCT = "nose", (320, 240), 2, 2


def part_frames():
    import lbp_part_cases as LP
    return LP.lbp_frames(*PART_FRAME)[:PART_FRAMES]


def part_expected(face=None):
    """([(list a, list b)] per frame, the detectors) of lbp_part_cases.Harness with the statement's detectors; face: another face detector"""
    import lbp_part_cases as LP
    r = LP.refs()
    dets = (face or LP.lbp_detector(r[LP.FACE]), LP.lbp_detector(r[LP.PART_A]), None)
    h = LP.Harness(PART_KIND, *dets, scale_factor_pct=PART_PCT)
    out = [h.process(f) for f in part_frames()]
    h.close()
    return out, dets
