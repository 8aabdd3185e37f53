"""cv::CascadeClassifier::detectMultiScale on a new-format HAAR cascade of stumps, stated in numpy: SURVEY.md A.16 (OpenCV 2.4
cascadedetect.cpp / cascadedetect.hpp -- Data::read, HaarEvaluator, predictOrderedStump -- from memory, unpinned).  The scan, its
levels, step, skip rule, emitted rectangles and grouping are A.15's and are taken from tests/lbp_reference.py (levels, walk_row,
cv_round); the shared image pieces are the oracle's (orc.resize_linear, orc.integral, orc.group_rectangles).  What is stated here is
the file reader, the window normalisation, the feature value and the stage."""
import xml.etree.ElementTree as ET

import numpy as np

import lbp_reference as L
import orc

levels, walk_row, cv_round = L.levels, L.walk_row, L.cv_round          # the scan's rules are A.15's: the same CascadeClassifierInvoker


class HaarNewCascade:
    """size (ow, oh); rects [nf, 3, 4] (a missing rect all zero); weights [nf, 3] f32 (a missing rect's 0); rect_counts [nf];
    feature_idx [nw]; thr [nw] f32; leaves [nw, 2] f32; stage_sizes [ns]; stage_thr [ns] f32, as evaluated: (float)value - 1e-5f"""

    def __init__(self, size, rects, weights, rect_counts, feature_idx, thr, leaves, stage_sizes, stage_thr):
        self.size = size
        self.rects = np.asarray(rects, np.int32).reshape(-1, 3, 4)
        self.weights = np.asarray(weights, np.float32).reshape(-1, 3)
        self.rect_counts = np.asarray(rect_counts, np.int32)
        self.feature_idx = np.asarray(feature_idx, np.int32)
        self.thr = np.asarray(thr, np.float32)
        self.leaves = np.asarray(leaves, np.float32).reshape(-1, 2)
        self.stage_sizes = np.asarray(stage_sizes, np.int32)
        self.stage_thr = np.asarray(stage_thr, np.float32)

    def arrays(self):
        return dict(size=self.size, rects=self.rects, weights=self.weights, rect_counts=self.rect_counts, feature_idx=self.feature_idx,
                    thr=self.thr, leaves=self.leaves, stage_sizes=self.stage_sizes, stage_thr=self.stage_thr)


def parse_xml(text):
    root = ET.fromstring(text)
    c = root[0]
    assert c.get("type_id") == "opencv-cascade-classifier" and c.findtext("featureType").strip() == "HAAR"
    assert int(c.find("featureParams").findtext("maxCatCount")) == 0
    ow, oh = int(c.findtext("width")), int(c.findtext("height"))
    rects, weights, counts = [], [], []
    for f in c.find("features"):
        assert int(f.findtext("tilted", "0")) == 0
        rr, ww = np.zeros((3, 4), np.int32), np.zeros(3, np.float32)
        items = list(f.find("rects"))
        assert 1 <= len(items) <= 3
        for k, it in enumerate(items):
            v = it.text.split()
            rr[k] = [int(x) for x in v[:4]]
            ww[k] = np.float32(float(v[4]))          # read as double, kept as float
        rects.append(rr); weights.append(ww); counts.append(len(items))
    fidx, thr, leaves, sizes, sthr = [], [], [], [], []
    for st in c.find("stages"):
        weak = list(st.find("weakClassifiers"))
        sizes.append(len(weak))
        sthr.append(np.float32(np.float32(float(st.findtext("stageThreshold"))) - np.float32(1e-5)))
        for w in weak:
            nodes = w.findtext("internalNodes").split()
            assert len(nodes) == 4 and [int(nodes[0]), int(nodes[1])] == [0, -1]
            fidx.append(int(nodes[2]))
            thr.append(np.float32(float(nodes[3])))
            leaves.append([np.float32(float(v)) for v in w.findtext("leafValues").split()])
    return HaarNewCascade((ow, oh), rects, weights, counts, fidx, thr, leaves, sizes, sthr)


def rect_sum(A, rect, xs, ys):
    """A(x, y) - A(x + w, y) - A(x, y + h) + A(x + w, y + h) at the window origins ys x xs, in A's own type (CALC_SUM)"""
    x, y, w, h = (int(v) for v in rect)
    return A[np.ix_(ys + y, xs + x)] - A[np.ix_(ys + y, xs + x + w)] - A[np.ix_(ys + y + h, xs + x)] + A[np.ix_(ys + y + h, xs + x + w)]


def window_vnf(S, Q, ow, oh, xs, ys, stats=None):
    """HaarEvaluator::setWindow: varianceNormFactor = 1. / nf of every window of the grid, f64"""
    norm = (1, 1, ow - 2, oh - 2)
    valsum = rect_sum(S, norm, xs, ys)                                  # int
    valsq = rect_sum(Q, norm, xs, ys)                                   # double; exact integers
    area = np.float64((ow - 2) * (oh - 2))
    nf = area * valsq - valsum.astype(np.float64) * valsum.astype(np.float64)
    pos = nf > 0
    if stats is not None:
        stats["nf_nonpositive"] = stats.get("nf_nonpositive", 0) + int(np.count_nonzero(~pos))
    nf = np.where(pos, np.sqrt(np.where(pos, nf, 1.0)), 1.0)
    return 1.0 / nf


def feature_values(casc, k, S, xs, ys, stats=None):
    """HaarEvaluator::operator(): float ret = w0 * sum0 + w1 * sum1 (+ w2 * sum2 when w2 != 0), every product and addition rounded to f32"""
    f = int(casc.feature_idx[k])
    w = casc.weights[f]
    sums = [rect_sum(S, casc.rects[f, r], xs, ys) for r in range(3)]       # (a missing rect is all zero: its sum is 0)
    if stats is not None:
        stats["sum_above_2p24"] = stats.get("sum_above_2p24", 0) + sum(int(np.count_nonzero(np.abs(s.astype(np.int64)) > (1 << 24))) for s in sums)
    ret = (w[0] * sums[0].astype(np.float32)).astype(np.float32) + (w[1] * sums[1].astype(np.float32)).astype(np.float32)
    ret = ret.astype(np.float32)
    if w[2] != np.float32(0):
        ret = (ret + (w[2] * sums[2].astype(np.float32)).astype(np.float32)).astype(np.float32)
    return ret


def grid_results(casc, S, Q, xs, ys, stats=None):
    """the result of every window of the grid: 1 passed every stage, -si rejected by stage si (0: by stage 0)"""
    ow, oh = casc.size
    vnf = window_vnf(S, Q, ow, oh, xs, ys, stats)
    res = np.ones((len(ys), len(xs)), np.int64)
    alive = np.ones(res.shape, bool)
    first = 0
    for si, n in enumerate(casc.stage_sizes):
        total = np.zeros(res.shape, np.float64)
        for k in range(first, first + int(n)):
            value = feature_values(casc, k, S, xs, ys, stats).astype(np.float64) * vnf
            total = total + np.where(value < np.float64(casc.thr[k]), casc.leaves[k, 0], casc.leaves[k, 1]).astype(np.float64)      # a tie takes leaf 1
        rej = alive & (total < np.float64(casc.stage_thr[si]))
        res[rej] = -si
        alive &= ~rej
        first += int(n)
    return res


def scan(casc, gray, scale_factor=1.1, min_size=(0, 0), max_size=(0, 0), stats=None):
    """the raw list in (level, y, x) order, [n, 4] int32; stats as lbp_reference.scan's ('depth', 'skipped_pass', 'levels'), and
    'nf_nonpositive' -- grid windows on the nf <= 0 branch --, 'sum_above_2p24' -- rect sums whose conversion to f32 is inexact"""
    gray = np.ascontiguousarray(gray, np.uint8)
    rows, cols = gray.shape
    ow, oh = casc.size
    out = []
    for factor, sz, win in L.levels(ow, oh, cols, rows, scale_factor, min_size, max_size):
        lev = gray if (sz[0], sz[1]) == (cols, rows) else orc.resize_linear(gray, sz[0], sz[1])
        S, Q = orc.integral(lev)
        step = 1 if factor > 2.0 else 2
        xs, ys = np.arange(0, sz[0] - ow, step), np.arange(0, sz[1] - oh, step)
        res = grid_results(casc, S, Q, xs, ys, stats)
        for iy, y in enumerate(ys):
            vis = L.walk_row(res[iy])
            for ix in vis:
                if res[iy, ix] > 0:
                    out.append((L.cv_round(xs[ix] * factor), L.cv_round(y * factor), win[0], win[1]))
            if stats is not None:
                stats.setdefault("depth", []).extend(int(res[iy, ix]) for ix in vis)
                skipped = np.ones(len(xs), bool)
                skipped[vis] = False
                stats["skipped_pass"] = stats.get("skipped_pass", 0) + int(np.count_nonzero(skipped & (res[iy] > 0)))
        if stats is not None:
            stats["levels"] = stats.get("levels", 0) + 1
    return np.asarray(out, np.int32).reshape(-1, 4)


def detect(casc, gray, scale_factor=1.1, min_neighbors=3, min_size=(0, 0), max_size=(0, 0)):
    raw = scan(casc, gray, scale_factor, min_size, max_size)
    if min_neighbors == 0 or len(raw) == 0:
        return raw
    return np.asarray(orc.group_rectangles(raw, max(min_neighbors, 1), 0.2)[0], np.int32).reshape(-1, 4)
