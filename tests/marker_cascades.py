"""Candidate sets built by construction, for the grouping tests (tests/test_group_regimes_cpu.py, tests/test_gpu_group_regimes.py).

THE MARKER CASCADE.  A 20 x 20 window, old format, two stages of one stump each over the same feature
[(0, 0, 20, 20, +1), (9, 9, 2, 2, -100)], stump threshold 0, stage threshold 0.5:
  * stage 0 votes left = right = 1.0: every window passes;
  * stage 1 votes left = 1.0, right = -1.0: a window passes exactly where its centre 2 x 2 pixels hold light (the feature is
    negative there; with a dark centre it is zero or positive);
  * the stump threshold is 0, so the variance normalisation drops out of the comparison and all arithmetic is exact.
On a black frame with single white pixels ("dots") at even coordinates, scanned at the one scale of 20 x 20 windows
(scale_factor 1.1, max_size (20, 20): step 2), the raw candidate list is exactly one window per dot -- the window
(x - 10, y - 10, 20, 20) of the dot (x, y) -- in scan order (y, then x).  A BGR frame of such dots passes bgr2gray and
equalizeHist unchanged, so a fresh face stream whose working image is the frame sees the same dots.

Two observations that shaped it:
  1. The pass-all first stage is not decoration.  With a one-stage marker the CPU oracle drops most dots: OpenCV 2.4's scan doubles
     its x step after a window that fails stage 0 (ixstep = result != 0 ? 1 : 2), so the grid becomes data-dependent.  With the
     pass-all stage no window fails at stage 0 and the grid is the full one.
  2. With all scales and factor 1.1, consecutive scales are similar and one dot yields ONE class (90 candidates on a 320 x 240
     frame, chained across scales).  With scale_factor 1.5 consecutive scales are not similar: a dot pair gives concentric
     classes of sizes [2, 6, 6, 6, 6, 4, 2], and the contained-box filter of groupRectangles decides which survive -- three
     different box lists for the thresholds 1, 2 and 3.

THE LIMITS the layouts sit on are k_group's (nubomedia-vca_amd/csrc/kernels_group.hip: kGroupMax, the 256 of its rank sort and of
its class tables; nubomedia-vca_amd/csrc/device_records.h: kGroupOutCap).  The counts the layouts promise are conditions on the CPU
oracle and py_group alone (test_group_regimes_cpu.py asserts them); if a kernel constant moves, move the layout.

py_group is a third statement of cv::groupRectangles, written from OpenCV's definition (cascadedetect.cpp groupRectangles,
operations.hpp partition), beside the oracle's (oracle/orc_haar.c) and the host library's (csrc/host_logic.cpp)."""
import functools

import numpy as np

from nubovca import synth

GROUP_MAX = 2048          # kGroupMax: raw candidates of a slot that k_group takes
GROUP_SORT = 256          # up to this many candidates: rank by counting; above: bitonic network
GROUP_CLASSES = 256       # classes k_group holds sums for
GROUP_OUT = 64            # kGroupOutCap: boxes per slot in the device's table

WIN = 20
THRESHOLDS = (1, 2, 3, 5, 9)


# ---------------------------------------------------------------- the cascade
def marker_cascade():
    feat = [(0, 0, WIN, WIN, 1.0), (9, 9, 2, 2, -100.0)]
    stage = lambda right: dict(features=[feat], thresholds=[0.0], left=[1.0], right=[right], stage_threshold=0.5)
    return dict(name="marker", size=(WIN, WIN), stages=[stage(1.0), stage(-1.0)])


@functools.lru_cache(maxsize=None)
def marker_xml():
    return synth.cascade_to_xml(marker_cascade())


@functools.lru_cache(maxsize=None)
def oracle_marker():
    import orc
    return orc.parse_cascade_xml(marker_xml())


# ---------------------------------------------------------------- frames
def dot_frame(W, H, dots, bgr=False):
    """black frame [H, W] (or [H, W, 3]) with a white pixel at every (x, y) of dots"""
    f = np.zeros((H, W, 3) if bgr else (H, W), np.uint8)
    for (x, y) in dots:
        assert 10 <= x < W - 10 and 10 <= y < H - 10, (x, y)
        f[y, x] = 255
    assert int((f[..., 0] if bgr else f).astype(bool).sum()) == len(dots), "two dots on one pixel"
    return f


def dot_windows(dots):
    """the raw list a single-scale scan of the dots leaves: one 20 x 20 window per dot, in scan order"""
    return np.array([[x - 10, y - 10, WIN, WIN] for (x, y) in sorted(dots, key=lambda d: (d[1], d[0]))], np.int32).reshape(-1, 4)


# ---------------------------------------------------------------- groupRectangles, from OpenCV's definition
def _similar(a, b, eps):
    delta = eps * (min(a[2], b[2]) + min(a[3], b[3])) * 0.5
    return (abs(a[0] - b[0]) <= delta and abs(a[1] - b[1]) <= delta and abs(a[0] + a[2] - b[0] - b[2]) <= delta
            and abs(a[1] + a[3] - b[1] - b[3]) <= delta)


def _similar_pairs(r, eps):
    """(i, j), i < j, of all similar pairs: SimilarRects evaluated on whole rows at once (same doubles as _similar)"""
    r = r.astype(np.int64)
    out = []
    x, y, w, h = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    for i in range(len(r) - 1):
        s = slice(i + 1, None)
        delta = eps * (np.minimum(w[i], w[s]) + np.minimum(h[i], h[s])).astype(np.float64) * 0.5
        ok = ((np.abs(x[i] - x[s]) <= delta) & (np.abs(y[i] - y[s]) <= delta) & (np.abs(x[i] + w[i] - x[s] - w[s]) <= delta)
              & (np.abs(y[i] + h[i] - y[s] - h[s]) <= delta))
        out += [(i, i + 1 + int(k)) for k in np.nonzero(ok)[0]]
    return out


def _cv_round(v):
    return int(np.rint(v))          # round half to even, as cvRound / saturate_cast<int>


class Grouped:
    """what py_group found: boxes [m, 4], weights [m], and the facts the regimes are defined by"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def py_group(rects, thr, eps=0.2):
    """cv::groupRectangles(rects, thr, eps).  Returns a Grouped with
      boxes, weights   the result (thr <= 0: the list itself, weights 1)
      n                candidates
      sizes            class sizes in class order (classes numbered by their first member, as cv::partition does)
      labels           class of every candidate
      avg              the class averages [ncls, 4]
      verdict          per class: "weak" (size <= thr), "free" (inside no other class that counts), "contained_kept",
                       "removed_small" (inside another one and n1 < 3 only), "removed_outvoted" (n2 > max(3, n1) only),
                       "removed_both"
      boundary         classes with n1 >= 3 inside a class of exactly max(3, n1) members (kept by '>', lost by '>=')
      ties             (class, coordinate, k) where float(sum) * (1.f / n) is k + 0.5 exactly
    """
    r = np.asarray(rects, np.int32).reshape(-1, 4)
    n = len(r)
    if thr <= 0 or n == 0:
        return Grouped(boxes=r.copy(), weights=np.ones(n, np.int32), n=n, sizes=[], labels=[], avg=np.zeros((0, 4), np.int32),
                       verdict=[], boundary=[], ties=[])
    # partition: serial union-find over every similar pair
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for (i, j) in _similar_pairs(r, eps):
        a, b = find(i), find(j)
        if a != b:
            parent[b] = a
    cls_of_root, labels = {}, []
    for i in range(n):
        labels.append(cls_of_root.setdefault(find(i), len(cls_of_root)))
    ncls = len(cls_of_root)
    sums = np.zeros((ncls, 4), np.int64)
    cnt = np.zeros(ncls, np.int64)
    for i in range(n):
        sums[labels[i]] += r[i]
        cnt[labels[i]] += 1
    avg = np.zeros((ncls, 4), np.int32)
    ties = []
    for c in range(ncls):
        s = np.float32(1) / np.float32(cnt[c])
        for k in range(4):
            v = np.float32(sums[c, k]) * s          # float product, as r.x * s
            assert v.dtype == np.float32
            avg[c, k] = _cv_round(v)
            if float(v) - np.floor(float(v)) == 0.5:
                ties.append((c, k, int(np.floor(float(v)))))
    boxes, weights, verdict, boundary = [], [], [], []
    for i in range(ncls):
        n1, r1 = int(cnt[i]), avg[i].astype(np.int64)
        if n1 <= thr:
            verdict.append("weak")
            continue
        contained, removed = False, None
        for j in range(ncls):
            n2 = int(cnt[j])
            if j == i or n2 <= thr:
                continue
            r2 = avg[j].astype(np.int64)
            dx, dy = _cv_round(float(r2[2]) * eps), _cv_round(float(r2[3]) * eps)
            if r1[0] >= r2[0] - dx and r1[1] >= r2[1] - dy and r1[0] + r1[2] <= r2[0] + r2[2] + dx and r1[1] + r1[3] <= r2[1] + r2[3] + dy:
                contained = True
                if n1 >= 3 and n2 == max(3, n1) and i not in boundary:
                    boundary.append(i)
                if n2 > max(3, n1) or n1 < 3:
                    removed = "removed_both" if (n2 > max(3, n1) and n1 < 3) else "removed_small" if n1 < 3 else "removed_outvoted"
                    break
        if removed:
            verdict.append(removed)
            continue
        verdict.append("contained_kept" if contained else "free")
        boxes.append(avg[i])
        weights.append(n1)
    return Grouped(boxes=np.array(boxes, np.int32).reshape(-1, 4), weights=np.array(weights, np.int32), n=n, sizes=[int(c) for c in cnt],
                   labels=labels, avg=avg, verdict=verdict, boundary=boundary, ties=ties)


# ---------------------------------------------------------------- layouts
def _block(x, y, nx, ny, pitch=2):
    return [(x + pitch * i, y + pitch * j) for j in range(ny) for i in range(nx)]


def _grid(count, per_row, x0, y0, px, py):
    return [(x0 + px * (k % per_row), y0 + py * (k // per_row)) for k in range(count)]


def _clusters(count, per_row, nx, ny, px=40, py=40, x0=20, y0=20):
    return [d for (x, y) in _grid(count, per_row, x0, y0, px, py) for d in _block(x, y, nx, ny)]


def _pairs(count, per_row=30):
    return _clusters(count, per_row, 2, 1)


def _chain(n, W=1280):
    """a serpentine of n dots at 4-pixel pitch: rows 8 pixels apart, joined at alternating ends by one dot between them"""
    per = (W - 40) // 4          # dots of a row
    out, y, k = [], 20, 0
    while len(out) < n:
        xs = [20 + 4 * i for i in range(per)]
        if k % 2:
            xs.reverse()
        out += [(x, y) for x in xs]
        out.append((xs[-1], y + 4))
        y += 8
        k += 1
    return out[:n]


def _mixed(singles, pairs):
    """`pairs` dot pairs among `singles` single dots on a 24-pixel grid, 50 a row: 7 pairs in every run of 32 classes, the
    rest singles, so that the classes a threshold of 1 keeps fall in all four 64-class waves with dropped ones between them"""
    total, out, p, s = singles + pairs, [], 0, 0
    for k, (x, y) in enumerate(_grid(total, 50, 20, 20, 24, 24)):
        pair = (k % 32) in (1, 5, 10, 14, 19, 23, 28) and p < pairs
        if not pair and s >= singles:
            pair = True
        if pair:
            out += [(x, y), (x + 2, y)]
            p += 1
        else:
            out.append((x, y))
            s += 1
    assert (p, s) == (pairs, singles)
    return out


def _rounding():
    """4-dot clusters whose x or y sums are 4 k + 2 (k + 0.5 exactly; dots sit on even pixels, so both parities of k need their
    own shape), clusters of 3, 5, 6 and 7 (1.f / n inexact), and a 12-dot cluster whose x sum is 12 m + 6: a tie in exact
    arithmetic that the float product with 1.f / 12 decides"""
    out = []
    x, y = 40, 40
    out += [(x, y), (x, y + 2), (x, y + 4), (x + 2, y)]                    # x: k even (30.5), y: k odd (31.5)
    x += 40
    out += [(x, y), (x + 2, y), (x + 2, y + 2), (x + 2, y + 4)]            # x: k odd, y: k odd
    x += 40
    out += [(x, y), (x, y + 4), (x + 2, y + 2), (x + 2, y + 4)]            # x: integer, y: k even (32.5)
    x += 40
    out += [(x, y), (x + 2, y), (x + 4, y), (x + 2, y + 2)]                # x: integer, y: k even (30.5)
    x += 40
    out += [(x, y), (x + 2, y), (x + 4, y + 2)]                            # 3
    x += 40
    out += [(x, y), (x + 2, y), (x + 4, y), (x, y + 2), (x + 4, y + 4)]    # 5
    x += 40
    out += _block(x, y, 3, 2)[:5] + [(x + 6, y + 2)]                       # 6
    x += 40
    out += _block(x, y, 4, 2)[:7]                                          # 7
    x += 40
    out += [(x + 2 * i, y) for i in range(6)] + [(x + 2 * i, y + 2) for i in (0, 1, 2, 4, 5, 6)]     # 12, x sum = 12 (x - 10) + 66
    return out


class Layout:
    """a dot frame and the detectMultiScale parameters it is scanned with"""

    def __init__(self, name, dots, W=1280, H=720, scale_factor=1.1, min_size=(0, 0), max_size=(WIN, WIN)):
        self.name, self.dots, self.W, self.H = name, list(dots), W, H
        self.scale_factor, self.min_size, self.max_size = scale_factor, min_size, max_size
        self.single_scale = max_size == (WIN, WIN)
        assert not self.single_scale or all(x % 2 == 0 and y % 2 == 0 for (x, y) in self.dots)          # one window per dot: the scan's step is 2

    def params(self):
        return dict(scale_factor=self.scale_factor, min_size=self.min_size, max_size=self.max_size)

    def gray(self):
        return dot_frame(self.W, self.H, self.dots)

    def bgr(self):
        return dot_frame(self.W, self.H, self.dots, bgr=True)

    def __repr__(self):
        return self.name


FAR = (1200, 700)          # an isolated dot, far from every cluster of the layouts that add one


def _layouts():
    L = [
        # the sort switch
        Layout("sort256", _clusters(32, 16, 4, 2)),
        Layout("sort257", _clusters(32, 16, 4, 2) + [FAR]),
        # the candidate limit
        Layout("cand2048", _clusters(64, 16, 8, 4)),
        Layout("cand2049", _clusters(64, 16, 8, 4) + [FAR]),
        Layout("chain2047", _chain(2047)),
        Layout("chain2048", _chain(2048)),
        Layout("chain2049", _chain(2049)),
        # the class limit
        Layout("cls256", _mixed(200, 56)),
        Layout("cls257", _mixed(201, 56)),
        Layout("singles255", _grid(255, 50, 20, 20, 24, 24)),
        Layout("singles256", _grid(256, 50, 20, 20, 24, 24)),
        Layout("singles257", _grid(257, 50, 20, 20, 24, 24)),
        # the box limit
        Layout("box64", _pairs(64)),
        Layout("box65", _pairs(65)),
        # rounding
        Layout("rounding", _rounding(), W=640, H=480),
        # the contained-box filter: factor 1.5, all scales
        Layout("filter_pair", [(160, 120), (162, 120)], W=320, H=240, scale_factor=1.5, max_size=(0, 0)),
        Layout("filter_block", _block(120, 100, 2, 2) + [(180, 140), (182, 140)], W=320, H=240, scale_factor=1.5, max_size=(0, 0)),
        Layout("filter_small", [(161, 120), (161, 121)], W=320, H=240, scale_factor=1.5, max_size=(0, 0)),          # odd column: classes of 2 inside classes of 2 and 3
        # key decode: every scale of a 1080p plan, windows at all four corners and in the middle
        Layout("corners", [d for (x, y) in ((12, 12), (1904, 12), (12, 1066), (1904, 1066), (960, 540)) for d in ((x, y), (x + 2, y))],
               W=1920, H=1080, max_size=(0, 0)),
        # degenerate
        Layout("empty", [], W=320, H=240),
        Layout("one_dot", [(160, 120)], W=320, H=240),
        Layout("one_class8", _block(160, 120, 4, 2), W=320, H=240),
    ]
    return {l.name: l for l in L}


LAYOUTS = _layouts()


@functools.lru_cache(maxsize=None)
def expected_raw(name):
    """the oracle's raw list of a layout, in scan order"""
    import orc
    l = LAYOUTS[name]
    out = orc.detect_raw(oracle_marker(), l.gray(), l.scale_factor, 0, l.min_size, l.max_size)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_grouped(name, thr):
    """(boxes, weights) the oracle groups the layout's raw list to"""
    import orc
    b, w = orc.group_rectangles(np.array(expected_raw(name)), thr)
    b.setflags(write=False)
    return b, w


@functools.lru_cache(maxsize=None)
def facts(name, thr):
    return py_group(expected_raw(name), thr)


# ---------------------------------------------------------------- frames of the batched face path
# A face stream scans all scales at factor 1.1 (multi_scale_factor 10) from W / 20 x H / 20 up, where one dot yields one class of about
# 90 candidates -- unless the dot sits so close to the frame's edge that only the smallest windows around it fit: 13 pixels from
# the bottom edge leave 2 candidates, 14 leave 3, 15 leave 4, 17 leave 7.  That is how these frames get classes on both sides of
# every min_neighbors used, and more than kGroupOutCap classes on one 320 x 240 frame.
FACE_W, FACE_H = 320, 240
FACE_MIN_NEIGHBORS = (1, 2, 3, 5)


def _ladder(shift=0):
    return [(50 + shift, FACE_H - 13), (110 + shift, FACE_H - 14), (170 + shift, FACE_H - 15), (230 + shift, FACE_H - 17), (160 - shift, 100)]


FACE_FRAMES = {
    "black": [],
    "three": [(100, 100), (102, 100), (220, 140)],                                             # two classes, a device answer
    "grid36": [(30 + 44 * i + 4 * (j % 2), 30 + 36 * j) for j in range(6) for i in range(6)],      # more than kGroupMax candidates
    "edge70": [(x, y) for y in (FACE_H - 13, 13) for x in range(20, FACE_W - 20, 8)],             # more than kGroupOutCap boxes
    "ladder": _ladder(), "ladder6": _ladder(6), "ladder12": _ladder(12), "ladder18": _ladder(18),
    "ladder24": _ladder(24), "ladder30": _ladder(30),     # classes of 2, 3, 4, 7 and ~90: another box list for each of 1, 2, 3, 5
}


@functools.lru_cache(maxsize=None)
def face_frame(name):
    f = dot_frame(FACE_W, FACE_H, FACE_FRAMES[name], bgr=True)
    f.setflags(write=False)
    return f


def oracle_stream(min_neighbors):
    import orc
    return orc.FaceStream(oracle_marker(), width_to_process=FACE_W, scale_factor_pct=10, min_neighbors=min_neighbors)


@functools.lru_cache(maxsize=None)
def face_raw(name):
    """the raw list of a face frame (the stateless half of a stream with min_neighbors 0)"""
    out = oracle_stream(0).frame_detect(face_frame(name), cap=1 << 14)
    assert len(out) < (1 << 14)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def face_expected(name, min_neighbors):
    """(boxes, ids) of a FRESH oracle stream's first frame"""
    return oracle_stream(min_neighbors).process(face_frame(name))


# ---------------------------------------------------------------- the threshold script
# Twelve streams, stream i always on ladder frame i % 6.  ("set", {stream: min_neighbors}) changes properties of living streams,
# ("run", streams) is one synchronous batch, ("pipelined", A, B) two batches in flight at once.  Per-slot thresholds live in a device
# array the host refreshes only when they changed: every run below hands at least one slot another value than the slot held
# before, the batch of 3 moves streams to other slots, the batch of 12 makes the array grow.
LADDERS = ["ladder", "ladder6", "ladder12", "ladder18", "ladder24", "ladder30"]
N_STREAMS = 12
FIRST_THRESHOLDS = [1, 2, 3, 5, 1, 2, 3, 5, 1, 2, 3, 5]
THRESHOLD_SCRIPT = [
    ("run", [0, 1, 2, 3, 4, 5]),
    ("set", {0: 2, 1: 1, 2: 5, 3: 3, 4: 2, 5: 1}),          # reversed
    ("run", [0, 1, 2, 3, 4, 5]),
    ("run", [3, 4, 5]),
    ("run", list(range(12))),
    ("run", [0, 1, 2, 3, 4, 5]),
    ("pipelined", [0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11]),
    ("set", {0: 1, 1: 2, 2: 3, 3: 5, 4: 1, 5: 2, 6: 5, 7: 3, 8: 2, 9: 1, 10: 5, 11: 3}),
    ("pipelined", [0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11]),
    ("set", {6: 1, 7: 2, 8: 3, 9: 5, 10: 1, 11: 2}),
    ("pipelined", [6, 7, 8, 9, 10, 11], [0, 1, 2, 3, 4, 5]),          # the streams change result sets
]
BOXES_AT = {1: 5, 2: 4, 3: 3, 5: 2}          # boxes a ladder frame leaves at each min_neighbors


def stream_frame(i):
    return face_frame(LADDERS[i % len(LADDERS)])


@functools.lru_cache(maxsize=None)
def threshold_script_expected():
    """[(streams, thresholds, [(boxes, ids)])] for every batch of the script, in order (a pipelined step gives two), from oracle
    streams fed the same history"""
    streams = [oracle_stream(t) for t in FIRST_THRESHOLDS]
    memo, out = {}, []
    for op in THRESHOLD_SCRIPT:
        if op[0] == "set":
            for i, t in op[1].items():
                streams[i].p.min_neighbors = t          # frame_detect reads the stream's parameter record
            continue
        for idx in op[1:]:
            res = [streams[i].process_memo((i % len(LADDERS), streams[i].p.min_neighbors), stream_frame(i), memo) for i in idx]
            out.append((list(idx), [int(streams[i].p.min_neighbors) for i in idx], res))
    return out
