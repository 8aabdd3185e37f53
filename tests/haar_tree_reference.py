"""cv::CascadeClassifier::detectMultiScale on a GENERAL new-format HAAR cascade -- tree weak classifiers, tilted features -- stated in
numpy: SURVEY.md A.19 (OpenCV 2.4 cascadedetect.cpp / cascadedetect.hpp: Data::read, predictOrdered<HaarEvaluator>, CV_TILTED_PTRS; from
memory, unpinned).  Everything A.19 does not name is A.16's and is taken from tests/haar_new_reference.py (levels, step, skip rule, the
normaliser, the f32 feature sum over upright rects).  Stated here: the file reader, the tilted integral from its definition, a tilted
rect's value, the tree walk -- vectorised over a grid, and once more for ONE window in plain Python integers and floats."""
import xml.etree.ElementTree as ET

import numpy as np

import haar_new_reference as H
import lbp_reference as L
import orc

TILE_STAGES = 3          # the stages the device evaluates at every grid position (what `stats` counts as "tile")


class HaarTreeCascade:
    """size (ow, oh); rects [nf, 3, 4]; weights [nf, 3] f32; rect_counts [nf]; tilted [nf]; node_counts [nw]; nodes [nn, 3] = left, right,
    feature as the file has them; node_thr [nn] f32; leaves [nn + nw] f32; stage_sizes [ns]; stage_thr [ns] f32 as evaluated"""
    KEYS = ("rects", "weights", "rect_counts", "tilted", "node_counts", "nodes", "node_thr", "leaves", "stage_sizes", "stage_thr")

    def __init__(self, size, rects, weights, rect_counts, tilted, node_counts, nodes, node_thr, leaves, stage_sizes, stage_thr):
        self.size = size
        self.rects = np.asarray(rects, np.int32).reshape(-1, 3, 4)
        self.weights = np.asarray(weights, np.float32).reshape(-1, 3)
        self.rect_counts = np.asarray(rect_counts, np.int32)
        self.tilted = np.asarray(tilted, np.int32)
        self.node_counts = np.asarray(node_counts, np.int32)
        self.nodes = np.asarray(nodes, np.int32).reshape(-1, 3)
        self.node_thr = np.asarray(node_thr, np.float32)
        self.leaves = np.asarray(leaves, np.float32)
        self.stage_sizes = np.asarray(stage_sizes, np.int32)
        self.stage_thr = np.asarray(stage_thr, np.float32)
        self.first_node = np.concatenate([[0], np.cumsum(self.node_counts)[:-1]]).astype(np.int64)
        self.first_leaf = np.concatenate([[0], np.cumsum(self.node_counts + 1)[:-1]]).astype(np.int64)

    def arrays(self):
        return dict(size=self.size, **{k: getattr(self, k) for k in self.KEYS})


def parse_xml(text):
    root = ET.fromstring(text)
    c = root[0]
    assert c.get("type_id") == "opencv-cascade-classifier" and c.findtext("featureType").strip() == "HAAR"
    assert int(c.find("featureParams").findtext("maxCatCount")) == 0
    ow, oh = int(c.findtext("width")), int(c.findtext("height"))
    rects, weights, counts, tilted = [], [], [], []
    for f in c.find("features"):
        rr, ww = np.zeros((3, 4), np.int32), np.zeros(3, np.float32)
        items = list(f.find("rects"))
        assert 1 <= len(items) <= 3
        for k, it in enumerate(items):
            v = it.text.split()
            rr[k] = [int(x) for x in v[:4]]
            ww[k] = np.float32(float(v[4]))          # read as double, kept as float
        rects.append(rr); weights.append(ww); counts.append(len(items)); tilted.append(int(f.findtext("tilted", "0")) != 0)
    ncnt, nodes, nthr, leaves, sizes, sthr = [], [], [], [], [], []
    for st in c.find("stages"):
        weak = list(st.find("weakClassifiers"))
        sizes.append(len(weak))
        sthr.append(np.float32(np.float32(float(st.findtext("stageThreshold"))) - np.float32(1e-5)))
        for w in weak:
            v = w.findtext("internalNodes").split()
            lv = w.findtext("leafValues").split()
            assert len(v) % 4 == 0 and len(lv) == len(v) // 4 + 1
            ncnt.append(len(v) // 4)
            for j in range(len(v) // 4):
                nodes.append([int(v[4 * j]), int(v[4 * j + 1]), int(v[4 * j + 2])])
                nthr.append(np.float32(float(v[4 * j + 3])))
            leaves += [np.float32(float(x)) for x in lv]
    return HaarTreeCascade((ow, oh), rects, weights, counts, tilted, ncnt, nodes, nthr, leaves, sizes, sthr)


def tilted_integral(img):
    """cv::integral's third plane from its definition (oracle/nvca_oracle.h): T(X, Y) = the sum of img(x, y) over y < Y,
    abs(x - X + 1) <= Y - y - 1; int32, (h + 1) x (w + 1).  Row y gives T(X, Y) its pixels x in [X - 1 - r, X - 1 + r], r = Y - y - 1."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    cs = np.zeros((h, w + 1), np.int64)
    cs[:, 1:] = np.cumsum(img.astype(np.int64), axis=1)          # cs[y, k] = img[y, :k].sum()
    T = np.zeros((h + 1, w + 1), np.int64)
    X = np.arange(w + 1)
    for Y in range(1, h + 1):
        for y in range(Y):
            r = Y - y - 1
            T[Y] += cs[y, np.clip(X + r, 0, w)] - cs[y, np.clip(X - 1 - r, 0, w)]
    assert T.max(initial=0) < 2 ** 31
    return T.astype(np.int32)


def tilted_rect_sum(T, rect, xs, ys):
    """CV_TILTED_PTRS / CALC_SUM: T(x, y) - T(x - h, y + h) - T(x + w, y + w) + T(x + w - h, y + w + h) at the window origins, int32"""
    x, y, w, h = (int(v) for v in rect)
    return T[np.ix_(ys + y, xs + x)] - T[np.ix_(ys + y + h, xs + x - h)] - T[np.ix_(ys + y + w, xs + x + w)] + T[np.ix_(ys + y + w + h, xs + x + w - h)]


def feature_values(casc, f, S, T, xs, ys):
    """HaarEvaluator::operator() of feature f: ret = w0 * sum0 + w1 * sum1 (+ w2 * sum2 when w2 != 0), every product and addition rounded
    to f32; a tilted feature's sums are tilted_rect_sum's, its weights the file's (no halving)"""
    w = casc.weights[f]
    one = (lambda r: tilted_rect_sum(T, r, xs, ys)) if casc.tilted[f] else (lambda r: H.rect_sum(S, r, xs, ys))
    sums = [one(casc.rects[f, r]) if r < casc.rect_counts[f] else np.zeros((len(ys), len(xs)), np.int32) for r in range(3)]
    ret = ((w[0] * sums[0].astype(np.float32)).astype(np.float32) + (w[1] * sums[1].astype(np.float32)).astype(np.float32)).astype(np.float32)
    if w[2] != np.float32(0):
        ret = (ret + (w[2] * sums[2].astype(np.float32)).astype(np.float32)).astype(np.float32)
    return ret


def tree_walk(casc, t, S, T, vnf, xs, ys, alive):
    """predictOrdered on weak classifier t for the windows in `alive`: (leaf [ny, nx] -- the tree's leaf each took, -1 where not alive --,
    visits {node: mask of the windows that evaluated it}).  idx = 0; do { idx = value(node[idx]) < thr ? left : right } while (idx > 0)"""
    n0, nn = int(casc.first_node[t]), int(casc.node_counts[t])
    idx = np.where(alive, 0, -1 - nn)                      # > 0 or the root's turn: at a node; <= 0 afterwards: leaf -idx (-1 - nn: none)
    todo = alive.copy()
    visits = {}
    for j in range(nn):                                    # children lie behind parents: one forward pass visits every path
        here = todo & (idx == j)
        if not here.any():
            continue
        visits[j] = here
        left, right, f = (int(v) for v in casc.nodes[n0 + j])
        value = feature_values(casc, f, S, T, xs, ys).astype(np.float64) * vnf
        nxt = np.where(value < np.float64(casc.node_thr[n0 + j]), left, right)          # a tie goes right
        idx = np.where(here, nxt, idx)
        todo = todo & ~(here & (nxt <= 0))
    assert not todo.any()
    return np.where(alive, -idx, -1), visits


def grid_results(casc, S, Q, T, xs, ys, trace=None):
    """the result of every window of the grid: 1 passed every stage, -si rejected by stage si (0: by stage 0).  trace (a dict) receives
    'leaf' {tree: leaf array}, 'visits' {tree: {node: mask}} for the trees of the first TILE_STAGES stages, and 'pairs' [ns][ny, nx]: the
    nodes stage si evaluated for the window (0 where it did not reach the stage)"""
    ow, oh = casc.size
    vnf = H.window_vnf(S, Q, ow, oh, xs, ys)
    res = np.ones((len(ys), len(xs)), np.int64)
    alive = np.ones(res.shape, bool)
    t = 0
    for si, n in enumerate(casc.stage_sizes):
        total = np.zeros(res.shape, np.float64)
        pairs = np.zeros(res.shape, np.int64)
        for _ in range(int(n)):
            leaf, visits = tree_walk(casc, t, S, T, vnf, xs, ys, alive)
            vote = casc.leaves[int(casc.first_leaf[t]) + np.maximum(leaf, 0)].astype(np.float64)
            total = total + np.where(alive, vote, 0.0)          # f64, in file order
            if trace is not None:
                for m in visits.values():
                    pairs += m
                if si < TILE_STAGES:
                    trace.setdefault("leaf", {})[t] = leaf
                    trace.setdefault("visits", {})[t] = visits
            t += 1
        if trace is not None:
            trace.setdefault("pairs", []).append(pairs)
            trace["gyp"] = np.where(alive, total, trace.get("gyp", np.zeros(res.shape, np.float64)))          # the last stage sum a window formed
        rej = alive & (total < np.float64(casc.stage_thr[si]))
        res[rej] = -si
        alive &= ~rej
    return res


def f32(v):
    return float(np.float32(v))


def window_result_scalar(casc, S, Q, T, X, Y):
    """grid_results for ONE window at (X, Y), in plain Python integers and floats (a product or a sum of two f32 values formed in f64 and
    rounded once to f32 is the f32 operation's result): (result, [stage sums reached])"""
    ow, oh = casc.size
    S, T = [[int(v) for v in row] for row in S], [[int(v) for v in row] for row in T]
    Qi = [[int(v) for v in row] for row in np.asarray(Q, np.float64)]

    def up(A, x, y, w, h):
        return A[Y + y][X + x] - A[Y + y][X + x + w] - A[Y + y + h][X + x] + A[Y + y + h][X + x + w]

    def tl(x, y, w, h):
        return T[Y + y][X + x] - T[Y + y + h][X + x - h] - T[Y + y + w][X + x + w] + T[Y + y + w + h][X + x + w - h]
    valsum, valsq = up(S, 1, 1, ow - 2, oh - 2), up(Qi, 1, 1, ow - 2, oh - 2)
    nf = float((ow - 2) * (oh - 2)) * float(valsq) - float(valsum) * float(valsum)
    vnf = 1.0 / (nf ** 0.5 if nf > 0 else 1.0)
    t, sums = 0, []
    for si, n in enumerate(casc.stage_sizes):
        total = 0.0
        for _ in range(int(n)):
            n0, l0 = int(casc.first_node[t]), int(casc.first_leaf[t])
            idx = 0
            while True:
                left, right, f = (int(v) for v in casc.nodes[n0 + idx])
                w = [float(v) for v in casc.weights[f]]
                s = [(tl(*casc.rects[f, r].tolist()) if casc.tilted[f] else up(S, *casc.rects[f, r].tolist())) if r < casc.rect_counts[f] else 0 for r in range(3)]
                ret = f32(f32(w[0] * f32(s[0])) + f32(w[1] * f32(s[1])))
                if w[2] != 0.0:
                    ret = f32(ret + f32(w[2] * f32(s[2])))
                idx = left if ret * vnf < float(casc.node_thr[n0 + idx]) else right
                if idx <= 0:
                    break
            total += float(casc.leaves[l0 - idx])
            t += 1
        sums.append(total)
        if total < float(casc.stage_thr[si]):
            return -si, sums
    return 1, sums


def scan(casc, gray, scale_factor=1.1, min_size=(0, 0), max_size=(0, 0), stats=None):
    """the raw list in (level, y, x) order, [n, 4] int32.  stats (a dict) receives 'depth' (the result of every visited window), 'levels',
    'node_hits' / 'leaf_hits' [nn] / [nl] -- visited windows that evaluated the node / took the leaf, for the trees of the first TILE_STAGES
    stages --, 'wave_split' -- trees of stage 0 for which some 32 x 2 block of grid positions (a wave of the stage-0 kernel) holds windows
    that left by different leaves --, 'pairs_tile' -- (window, node) evaluations of the first TILE_STAGES stages at EVERY grid position --
    and 'pairs_rest' -- those of the later stages on visited windows"""
    gray = np.ascontiguousarray(gray, np.uint8)
    rows, cols = gray.shape
    ow, oh = casc.size
    out = []
    if stats is not None:
        stats.setdefault("node_hits", np.zeros(len(casc.nodes), np.int64)); stats.setdefault("leaf_hits", np.zeros(len(casc.leaves), np.int64))
        stats.setdefault("wave_split", set())
    for factor, sz, win in L.levels(ow, oh, cols, rows, scale_factor, min_size, max_size):
        lev = gray if (sz[0], sz[1]) == (cols, rows) else orc.resize_linear(gray, sz[0], sz[1])
        S, Q = orc.integral(lev)
        T = tilted_integral(lev) if casc.tilted.any() else np.zeros(S.shape, np.int32)
        step = 1 if factor > 2.0 else 2
        xs, ys = np.arange(0, sz[0] - ow, step), np.arange(0, sz[1] - oh, step)
        trace = {} if stats is not None else None
        res = grid_results(casc, S, Q, T, xs, ys, trace)
        visited = np.zeros(res.shape, bool)
        for iy, y in enumerate(ys):
            vis = L.walk_row(res[iy])
            visited[iy, vis] = True
            for ix in vis:
                if res[iy, ix] > 0:
                    out.append((L.cv_round(xs[ix] * factor), L.cv_round(y * factor), win[0], win[1]))
            if stats is not None:
                stats.setdefault("depth", []).extend(int(res[iy, ix]) for ix in vis)
        if stats is not None:
            stats["levels"] = stats.get("levels", 0) + 1
            for t, visits in trace.get("visits", {}).items():
                for j, m in visits.items():
                    stats["node_hits"][int(casc.first_node[t]) + j] += int(np.count_nonzero(m & visited))
                leaf = trace["leaf"][t]
                for k in range(int(casc.node_counts[t]) + 1):
                    stats["leaf_hits"][int(casc.first_leaf[t]) + k] += int(np.count_nonzero((leaf == k) & visited))
                if t < int(casc.stage_sizes[0]):
                    for by in range(0, leaf.shape[0], 2):
                        for bx in range(0, leaf.shape[1], 32):
                            if len(np.unique(leaf[by:by + 2, bx:bx + 32])) > 1:
                                stats["wave_split"].add(t)
            for si, pairs in enumerate(trace["pairs"]):
                if si < TILE_STAGES:
                    stats["pairs_tile"] = stats.get("pairs_tile", 0) + int(pairs.sum())
                else:
                    stats["pairs_rest"] = stats.get("pairs_rest", 0) + int(pairs[visited].sum())
    return np.asarray(out, np.int32).reshape(-1, 4)


def scan_levels(casc, gray, scale_factor=1.1, min_size=(0, 0), max_size=(0, 0)):
    """levels_reference.scan_levels with this evaluator: (rects [n, 4] int32, reject levels [n] int32, level weights [n]
    float64) of every visited window that reached one of the last three stages"""
    gray = np.ascontiguousarray(gray, np.uint8)
    rows, cols = gray.shape
    ow, oh = casc.size
    n = len(casc.stage_sizes)
    rects, levels, weights = [], [], []
    for factor, sz, win in L.levels(ow, oh, cols, rows, scale_factor, min_size, max_size):
        lev = gray if (sz[0], sz[1]) == (cols, rows) else orc.resize_linear(gray, sz[0], sz[1])
        S, Q = orc.integral(lev)
        T = tilted_integral(lev) if casc.tilted.any() else np.zeros(S.shape, np.int32)
        step = 1 if factor > 2.0 else 2
        xs, ys = np.arange(0, sz[0] - ow, step), np.arange(0, sz[1] - oh, step)
        trace = {}
        res = grid_results(casc, S, Q, T, xs, ys, trace)
        for iy, y in enumerate(ys):
            for ix in L.walk_row(res[iy]):
                result = -n if res[iy, ix] == 1 else int(res[iy, ix])
                if n + result < 4:
                    rects.append((L.cv_round(xs[ix] * factor), L.cv_round(y * factor), win[0], win[1]))
                    levels.append(-result)
                    weights.append(trace["gyp"][iy, ix])
    return np.asarray(rects, np.int32).reshape(-1, 4), np.asarray(levels, np.int32), np.asarray(weights, np.float64)


def detect(casc, gray, scale_factor=1.1, min_neighbors=3, min_size=(0, 0), max_size=(0, 0)):
    raw = scan(casc, gray, scale_factor, min_size, max_size)
    if min_neighbors == 0 or len(raw) == 0:
        return raw
    return np.asarray(orc.group_rectangles(raw, max(min_neighbors, 1), 0.2)[0], np.int32).reshape(-1, 4)
