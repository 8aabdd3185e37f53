"""cv::CascadeClassifier::detectMultiScale on a new-format LBP cascade of stumps, stated in numpy: SURVEY.md A.15 (OpenCV 2.4
cascadedetect.cpp / cascadedetect.hpp, from memory, unpinned).  The pieces shared with the Haar path are the oracle's
(orc.resize_linear, orc.integral, orc.group_rectangles); the XML reader is this file's own, on xml.etree.  A level's grid is
evaluated per weak classifier over every grid position at once; the serial walk's skip rule is applied per row afterwards."""
import xml.etree.ElementTree as ET

import numpy as np

import orc

BITS = ((0, 0, 128), (0, 1, 64), (0, 2, 32), (1, 2, 16), (2, 2, 8), (2, 1, 4), (2, 0, 2), (1, 0, 1))


class LbpCascade:
    """size (ow, oh); rects [nf, 4]; feature_idx [nw]; subsets [nw, 8] int32; leaves [nw, 2] f32; stage_sizes [ns]; stage_thr [ns] f32,
    as evaluated: (float)value - 1e-5f"""

    def __init__(self, size, rects, feature_idx, subsets, leaves, stage_sizes, stage_thr):
        self.size = size
        self.rects = np.asarray(rects, np.int32).reshape(-1, 4)
        self.feature_idx = np.asarray(feature_idx, np.int32)
        self.subsets = np.asarray(subsets, np.int32).reshape(-1, 8)
        self.leaves = np.asarray(leaves, np.float32).reshape(-1, 2)
        self.stage_sizes = np.asarray(stage_sizes, np.int32)
        self.stage_thr = np.asarray(stage_thr, np.float32)

    def arrays(self):
        return dict(size=self.size, rects=self.rects, feature_idx=self.feature_idx, subsets=self.subsets, leaves=self.leaves,
                    stage_sizes=self.stage_sizes, stage_thr=self.stage_thr)


def parse_xml(text):
    root = ET.fromstring(text)
    c = root[0]
    assert c.get("type_id") == "opencv-cascade-classifier" and c.findtext("featureType").strip() == "LBP"
    ow, oh = int(c.findtext("width")), int(c.findtext("height"))
    rects = [[int(v) for v in f.findtext("rect").split()] for f in c.find("features")]
    fidx, subsets, leaves, sizes, thr = [], [], [], [], []
    for st in c.find("stages"):
        weak = list(st.find("weakClassifiers"))
        sizes.append(len(weak))
        thr.append(np.float32(np.float32(float(st.findtext("stageThreshold"))) - np.float32(1e-5)))
        for w in weak:
            nodes = [int(v) for v in w.findtext("internalNodes").split()]
            assert len(nodes) == 11 and nodes[:2] == [0, -1]
            fidx.append(nodes[2])
            subsets.append(nodes[3:])
            leaves.append([np.float32(float(v)) for v in w.findtext("leafValues").split()])
    return LbpCascade((ow, oh), rects, fidx, subsets, leaves, sizes, thr)


def cv_round(v):
    return np.rint(v).astype(np.int64) if isinstance(v, np.ndarray) else int(np.rint(v))


def codes(S, rect, xs, ys):
    """LBP codes of the feature at the window origins ys x xs of the level with integral S"""
    x, y, w, h = (int(v) for v in rect)
    P = [[S[np.ix_(ys + y + r * h, xs + x + c * w)].astype(np.int64) for c in range(4)] for r in range(4)]
    cell = [[P[r][c] - P[r][c + 1] - P[r + 1][c] + P[r + 1][c + 1] for c in range(3)] for r in range(3)]
    code = np.zeros(cell[0][0].shape, np.int64)
    for r, c, bit in BITS:
        code += bit * (cell[r][c] >= cell[1][1])
    return code


def grid_results(casc, S, xs, ys):
    """the result of every window of the grid: 1 passed every stage, -si rejected by stage si (0: by stage 0)"""
    res = np.ones((len(ys), len(xs)), np.int64)
    alive = np.ones(res.shape, bool)
    first = 0
    for si, n in enumerate(casc.stage_sizes):
        tmp = np.zeros(res.shape, np.float32)
        for k in range(first, first + int(n)):
            code = codes(S, casc.rects[casc.feature_idx[k]], xs, ys)
            word = casc.subsets[k].view(np.uint32)[code >> 5]
            bit = (word >> (code & 31).astype(np.uint32)) & 1
            tmp = (tmp + np.where(bit != 0, casc.leaves[k, 0], casc.leaves[k, 1]).astype(np.float32)).astype(np.float32)     # one f32 addition per vote, in file order
        rej = alive & (tmp < casc.stage_thr[si])
        res[rej] = -si
        alive &= ~rej
        first += int(n)
    return res


def levels(ow, oh, cols, rows, sf, min_size=(0, 0), max_size=(0, 0)):
    maxw, maxh = max_size if max_size[0] and max_size[1] else (cols, rows)
    out, factor = [], 1.0
    while True:
        win = (cv_round(ow * factor), cv_round(oh * factor))
        sz = (cv_round(cols / factor), cv_round(rows / factor))
        if sz[0] - ow <= 0 or sz[1] - oh <= 0:
            break
        if win[0] > maxw or win[1] > maxh:
            break
        if not (win[0] < min_size[0] or win[1] < min_size[1]):
            out.append((factor, sz, win))
        factor *= sf
    return out


def walk_row(res_row):
    """grid columns the serial walk visits in a row: a stage-0 reject (result 0) skips the next one"""
    vis, i = [], 0
    while i < len(res_row):
        vis.append(i)
        i += 2 if res_row[i] == 0 else 1
    return vis


def scan(casc, gray, scale_factor=1.1, min_size=(0, 0), max_size=(0, 0), stats=None):
    """the raw list in (level, y, x) order, [n, 4] int32.  stats (a dict, optional) collects: 'depth' -- results of the visited windows,
    'skipped_pass' -- windows the skip rule jumped over that would have passed every stage, 'levels'."""
    gray = np.ascontiguousarray(gray, np.uint8)
    rows, cols = gray.shape
    ow, oh = casc.size
    out = []
    for factor, sz, win in levels(ow, oh, cols, rows, scale_factor, min_size, max_size):
        lev = gray if (sz[0], sz[1]) == (cols, rows) else orc.resize_linear(gray, sz[0], sz[1])
        S = orc.integral(lev)[0]
        step = 1 if factor > 2.0 else 2
        xs, ys = np.arange(0, sz[0] - ow, step), np.arange(0, sz[1] - oh, step)
        res = grid_results(casc, S, xs, ys)
        for iy, y in enumerate(ys):
            vis = walk_row(res[iy])
            for ix in vis:
                if res[iy, ix] > 0:
                    out.append((cv_round(xs[ix] * factor), cv_round(y * factor), win[0], win[1]))
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
