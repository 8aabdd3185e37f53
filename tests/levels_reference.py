"""cv::CascadeClassifier::detectMultiScale(image, objects, rejectLevels, levelWeights, ..., outputRejectLevels = true) on a new-format
cascade, stated in numpy: SURVEY.md A.17 (OpenCV 2.4 cascadedetect.cpp, from memory, unpinned).  The scan -- levels, step, visit order,
skip rule, features, vnf -- is tests/lbp_reference.py's (A.15) and tests/haar_new_reference.py's (A.16); what is stated here is the
stage sum a window ends with (gypWeight), which windows are emitted with which reject level, and the weighted groupRectangles."""
import numpy as np

import haar_new_reference as H
import lbp_reference as L
import orc

DBL_MIN = np.finfo(np.float64).tiny


def is_haar(casc):
    return isinstance(casc, H.HaarNewCascade)


def stage_sums(casc, S, Q, xs, ys):
    """per stage, the sum every window of the grid would compare with the stage threshold: LBP f32 (one addition per vote, in file
    order), HAAR f64 -- the loops of L.grid_results / H.grid_results"""
    shape = (len(ys), len(xs))
    first = 0
    if is_haar(casc):
        vnf = H.window_vnf(S, Q, casc.size[0], casc.size[1], xs, ys)
        for n in casc.stage_sizes:
            total = np.zeros(shape, np.float64)
            for k in range(first, first + int(n)):
                value = H.feature_values(casc, k, S, xs, ys).astype(np.float64) * vnf
                total = total + np.where(value < np.float64(casc.thr[k]), casc.leaves[k, 0], casc.leaves[k, 1]).astype(np.float64)
            yield total
            first += int(n)
    else:
        for n in casc.stage_sizes:
            tmp = np.zeros(shape, np.float32)
            for k in range(first, first + int(n)):
                code = L.codes(S, casc.rects[casc.feature_idx[k]], xs, ys)
                word = casc.subsets[k].view(np.uint32)[code >> 5]
                bit = (word >> (code & 31).astype(np.uint32)) & 1
                tmp = (tmp + np.where(bit != 0, casc.leaves[k, 0], casc.leaves[k, 1]).astype(np.float32)).astype(np.float32)
            yield tmp
            first += int(n)


def grid_levels(casc, S, Q, xs, ys):
    """(result, gypWeight) of every window of the grid: result 1 passed every stage, -si rejected by stage si; gypWeight the sum of the
    last stage evaluated (the rejecting stage's, or the last stage's on a pass), widened to f64"""
    res = np.ones((len(ys), len(xs)), np.int64)
    alive = np.ones(res.shape, bool)
    gyp = np.zeros(res.shape, np.float64)
    for si, total in enumerate(stage_sums(casc, S, Q, xs, ys)):
        gyp = np.where(alive, total.astype(np.float64), gyp)
        thr = np.float64(casc.stage_thr[si]) if is_haar(casc) else casc.stage_thr[si]          # (f64 sum < (double)thr; f32 sum < f32 thr)
        rej = alive & (total < thr)
        res[rej] = -si
        alive &= ~rej
    return res, gyp


def scan_levels(casc, gray, scale_factor=1.1, min_size=(0, 0), max_size=(0, 0)):
    """(rects [n, 4] int32, reject levels [n] int32, level weights [n] float64) in (level, y, x) order: every visited window with
    nstages + result < 4 after result 1 has become -nstages"""
    gray = np.ascontiguousarray(gray, np.uint8)
    rows, cols = gray.shape
    ow, oh = casc.size
    n = len(casc.stage_sizes)
    rects, levels, weights = [], [], []
    for factor, sz, win in L.levels(ow, oh, cols, rows, scale_factor, min_size, max_size):
        lev = gray if (sz[0], sz[1]) == (cols, rows) else orc.resize_linear(gray, sz[0], sz[1])
        S, Q = orc.integral(lev)
        step = 1 if factor > 2.0 else 2
        xs, ys = np.arange(0, sz[0] - ow, step), np.arange(0, sz[1] - oh, step)
        res, gyp = grid_levels(casc, S, Q, xs, ys)
        for iy, y in enumerate(ys):
            for ix in L.walk_row(res[iy]):          # (the skip rule reads the result BEFORE it is rewritten: a pass is 1, never 0)
                result = int(res[iy, ix])
                if result == 1:
                    result = -n
                if n + result < 4:
                    rects.append((L.cv_round(xs[ix] * factor), L.cv_round(y * factor), win[0], win[1]))
                    levels.append(-result)
                    weights.append(gyp[iy, ix])
    return np.asarray(rects, np.int32).reshape(-1, 4), np.asarray(levels, np.int32), np.asarray(weights, np.float64)


# ------------------------------------------------------------------ groupRectangles(rects, rejectLevels, levelWeights, groupThreshold, eps)
def classes(rects, eps=0.2):
    """cv::partition under SimilarRects(eps) and the per-class average: (labels [n], averaged rects [nc, 4] int32, member counts [nc]);
    classes are numbered in order of their first member"""
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    n = len(r)
    # The classes are the connected components of SimilarRects.  A partner of a lies within delta <= eps (w_a + h_a) / 2 of it in x, so the
    # rectangles are looked through in x order and a member is compared with that stretch alone (the predicate itself is tested in full).
    order = np.argsort(r[:, 0], kind="stable")
    place = np.empty(n, np.int64)
    place[order] = np.arange(n)
    x, y, w, h = (np.ascontiguousarray(r[order, k]) for k in range(4))
    lab = np.full(n, -1, np.int64)          # (in x order)
    nc = 0
    for i in range(n):
        if lab[place[i]] >= 0:
            continue
        lab[place[i]] = nc
        todo = [int(place[i])]
        while todo:          # the connected component of i
            a = todo.pop()
            reach = eps * (w[a] + h[a]) * 0.5
            lo, hi = np.searchsorted(x, x[a] - reach, "left"), np.searchsorted(x, x[a] + reach, "right")
            xs, ys, ws, hs = x[lo:hi], y[lo:hi], w[lo:hi], h[lo:hi]
            delta = eps * (np.minimum(w[a], ws) + np.minimum(h[a], hs)) * 0.5
            near = (np.abs(x[a] - xs) <= delta) & (np.abs(y[a] - ys) <= delta) & (np.abs(x[a] + w[a] - xs - ws) <= delta) & \
                   (np.abs(y[a] + h[a] - ys - hs) <= delta) & (lab[lo:hi] < 0)
            for b in np.nonzero(near)[0]:
                lab[lo + b] = nc
                todo.append(int(lo + b))
        nc += 1
    labels = lab[place]
    sums = np.zeros((nc, 4), np.int64)
    np.add.at(sums, labels, r)
    counts = np.bincount(labels, minlength=nc).astype(np.int64)
    s = (np.float32(1) / counts.astype(np.float32)).astype(np.float32)                    # float s = 1.f / n; cvRound(int * s): an f32 product
    avg = np.rint((sums.astype(np.float32) * s[:, None]).astype(np.float32)).astype(np.int32)
    return labels, avg, counts


def group_levels(rects, levels, weights, min_neighbors, eps=0.2, cls=None):
    """the weighted form; min_neighbors <= 0 returns the triples untouched (the library's choice).  cls: classes(rects, eps),
    where a caller groups one list with several thresholds"""
    rects = np.asarray(rects, np.int32).reshape(-1, 4)
    levels, weights = np.asarray(levels, np.int32), np.asarray(weights, np.float64)
    if min_neighbors <= 0 or len(rects) == 0:
        return rects, levels, weights
    labels, avg, counts = classes(rects, eps) if cls is None else cls
    nc = len(counts)
    max_level, max_weight = [0] * nc, [DBL_MIN] * nc
    for i in range(len(rects)):
        c = labels[i]
        if levels[i] > max_level[c]:
            max_level[c], max_weight[c] = int(levels[i]), float(weights[i])
        elif levels[i] == max_level[c] and weights[i] > max_weight[c]:
            max_weight[c] = float(weights[i])
    out_r, out_l, out_w = [], [], []
    for i in range(nc):
        r1, n1 = avg[i].astype(np.int64), max_level[i]          # the quirk: a class's own n1 is its level ...
        if n1 <= min_neighbors:
            continue
        for j in range(nc):
            n2 = int(counts[j])                                 # ... the other class's n2 its member count
            if j == i or n2 <= min_neighbors:
                continue
            r2 = avg[j].astype(np.int64)
            dx, dy = L.cv_round(float(r2[2]) * eps), L.cv_round(float(r2[3]) * eps)
            if r1[0] >= r2[0] - dx and r1[1] >= r2[1] - dy and r1[0] + r1[2] <= r2[0] + r2[2] + dx and r1[1] + r1[3] <= r2[1] + r2[3] + dy and \
               (n2 > max(3, n1) or n1 < 3):
                break
        else:
            out_r.append(avg[i]); out_l.append(n1); out_w.append(max_weight[i])
    return np.asarray(out_r, np.int32).reshape(-1, 4), np.asarray(out_l, np.int32), np.asarray(out_w, np.float64)


def detect_levels(casc, gray, scale_factor=1.1, min_neighbors=3, min_size=(0, 0), max_size=(0, 0)):
    return group_levels(*scan_levels(casc, gray, scale_factor, min_size, max_size), min_neighbors)
