"""Synthetic inputs for the Haar hot path: a seeded stump cascade written in
OpenCV's old-format XML (the reference hard-codes
/usr/share/opencv/haarcascades/haarcascade_frontalface_alt.xml,
FACE/kmsfacedetect.cpp:40, which is not available offline) and seeded frames.

The cascade has the *shape* of haarcascade_frontalface_alt (20x20 window,
22 stages, 2135 stumps, first stages 3/16/21) and is constructed so that
  * i.i.d. noise windows are rejected with ~50 % probability per stage
    (the per-stage false-alarm rate haartraining aims for), and
  * windows resembling TEMPLATE (a 20x20 face-like pattern) pass every stage.
It is a workload generator, not a face model.
"""
import numpy as np

FRONTALFACE_ALT_STAGES = [3, 16, 21, 39, 33, 44, 50, 51, 56, 71, 80, 103, 111, 102,
                          135, 137, 140, 160, 177, 182, 211, 213]
WIN = 20


def template(win=WIN):
    """20x20 face-like luminance pattern, float64 in [0,255]."""
    y, x = np.mgrid[0:win, 0:win].astype(np.float64)
    s = win / 20.0

    def blob(cx, cy, sx, sy, amp):
        return amp * np.exp(-(((x - cx * s) / (sx * s)) ** 2 + ((y - cy * s) / (sy * s)) ** 2))

    t = np.full((win, win), 150.0)
    t += blob(9.5, 9.5, 9, 11, 40)           # bright face oval
    t += blob(5.5, 7.0, 2.2, 1.4, -95)       # left eye
    t += blob(13.5, 7.0, 2.2, 1.4, -95)      # right eye
    t += blob(5.5, 4.6, 2.8, 0.9, -45)       # brows
    t += blob(13.5, 4.6, 2.8, 0.9, -45)
    t += blob(9.5, 10.0, 1.3, 3.0, 45)       # nose bridge
    t += blob(9.5, 15.2, 3.4, 1.2, -80)      # mouth
    t += blob(9.5, 0.5, 9, 2.0, -60)         # hair line
    return np.clip(t, 0, 255)


def _rand_feature(rng, win):
    """One Haar-like feature inside the [1, win-1) interior.
    Returns list of (x, y, w, h, weight) with rect[0] the whole support."""
    lo, hi = 1, win - 1
    kind = rng.integers(0, 5)
    for _ in range(100):
        if kind == 0:      # x2
            w, h = rng.integers(1, 9), rng.integers(1, 17)
            W, H = 2 * w, h
        elif kind == 1:    # y2
            w, h = rng.integers(1, 17), rng.integers(1, 9)
            W, H = w, 2 * h
        elif kind == 2:    # x3
            w, h = rng.integers(1, 6), rng.integers(1, 17)
            W, H = 3 * w, h
        elif kind == 3:    # y3
            w, h = rng.integers(1, 17), rng.integers(1, 6)
            W, H = w, 3 * h
        else:              # x2_y2
            w, h = rng.integers(1, 9), rng.integers(1, 9)
            W, H = 2 * w, 2 * h
        if W * H < 8 or W > hi - lo or H > hi - lo:
            continue
        x = rng.integers(lo, hi - W + 1)
        y = rng.integers(lo, hi - H + 1)
        if kind == 0:
            return [(x, y, W, H, -1.0), (x + w, y, w, h, 2.0)]
        if kind == 1:
            return [(x, y, W, H, -1.0), (x, y + h, w, h, 2.0)]
        if kind == 2:
            return [(x, y, W, H, -1.0), (x + w, y, w, h, 3.0)]
        if kind == 3:
            return [(x, y, W, H, -1.0), (x, y + h, w, h, 3.0)]
        return [(x, y, W, H, -1.0), (x, y, w, h, 2.0), (x + w, y + h, w, h, 2.0)]
    raise RuntimeError("feature sampling failed")


def _pixel_coeffs(feat, win):
    """Per-pixel coefficient image of a feature at scale 1 with OpenCV's weight
    normalisation (rect0 weight recomputed so the feature is zero-mean)."""
    inv_area = 1.0 / ((win - 2) * (win - 2))
    c = np.zeros((win, win))
    w = [r[4] * inv_area for r in feat]
    w[0] = -sum(w[k] * feat[k][2] * feat[k][3] for k in range(1, len(feat))) / (feat[0][2] * feat[0][3])
    for k, (x, y, rw, rh, _) in enumerate(feat):
        c[y:y + rh, x:x + rw] += w[k]
    return c


def _norm_values(coefs, windows):
    """Normalised feature values v = sum(c*img)/std(img[1:-1,1:-1]) for a stack of
    windows [N,win,win] and coefficient images [F,win,win] -> [N,F]."""
    inner = windows[:, 1:-1, 1:-1].reshape(len(windows), -1)
    std = inner.std(axis=1)
    std = np.where(std > 0, std, 1.0)
    vals = windows.reshape(len(windows), -1) @ coefs.reshape(len(coefs), -1).T
    return vals / std[:, None]


def part_template(name, win=WIN):
    """20x20 crop of the 4x up-sampled face TEMPLATE around a face part: what the synthetic
    stand-ins for haarcascade_mcs_{righteye,lefteye,nose,mouth,leftear,rightear} respond to.
    (x0, y0) are in the 80x80 face; a part therefore spans a quarter of the face width."""
    big = template(4 * win)
    x0, y0 = {"righteye": (12, 18), "lefteye": (44, 18), "nose": (28, 32), "mouth": (28, 50),
              "leftear": (0, 28), "rightear": (60, 28)}[name]
    return big[y0:y0 + win, x0:x0 + win].copy()


def make_cascade(seed=2016, stages=None, win=WIN, n_mc=3000, pass_rate=0.5, open_stages=4,
                 agree_lo=0.52, agree_hi=0.60, tmpl=None, calib=None):
    """Returns a dict describing a stump cascade (see cascade_to_xml).

    Every stump separates TEMPLATE's normalised feature value v_T from zero
    (threshold 0.4*v_T, |v_T| >= 1.5 noise sigmas).  The first `open_stages`
    stages get the stage threshold that passes ~pass_rate of noise windows (the
    bulk of the work on any frame, as with a trained cascade); later stages
    additionally demand that agree_lo..agree_hi of the vote weight sides with
    the template, which makes the cascade specific.

    calib: a WindowSample (below) -- windows of real frame content at the scan's own scales.  The stage thresholds are then
    chosen stage by stage on the windows that passed every stage before (what haartraining does with its negatives): each
    stage lets ~pass_rate of what reaches it through, for as many stages as the sample still holds a few hundred windows;
    the stages behind them keep the template-agreement rule.  Features, stump thresholds and votes are the same as without
    calib (same seed, same draws).
    """
    stages = list(FRONTALFACE_ALT_STAGES if stages is None else stages)
    rng = np.random.default_rng(seed)
    T = template(win) if tmpl is None else np.asarray(tmpl, np.float64)
    negs = rng.integers(0, 256, size=(n_mc, win, win)).astype(np.float64)
    Tn = T[None]
    out_stages = []
    for si, ncls in enumerate(stages):
        feats, thr, lv, rv = [], [], [], []
        coefs = []
        while len(feats) < ncls:
            f = _rand_feature(rng, win)
            c = _pixel_coeffs(f, win)
            vT = _norm_values(c[None], Tn)[0, 0]
            sf = np.sqrt((c ** 2).sum())             # std of v on unit-variance noise
            if abs(vT) < 1.5 * sf:
                continue                             # not discriminative for the template
            t = 0.4 * vT
            a = rng.uniform(0.4, 1.0)
            feats.append(f); coefs.append(c); thr.append(t)
            if vT >= t:      # template on the "right" (>= t) side
                lv.append(-a); rv.append(a)
            else:
                lv.append(a); rv.append(-a)
        coefs = np.stack(coefs)
        s_T = sum(abs(a) for a in rv)
        calibrated = False
        if calib is not None and calib.alive_count() >= 256:
            # the votes are float32 in the file and in every evaluator: calibrate on exactly those
            votes = calib.stage_votes(feats, thr, np.float32(lv).astype(np.float64), np.float32(rv).astype(np.float64))
            cand = np.unique(votes)
            rates = np.array([(votes >= cnd).mean() for cnd in cand])
            st_thr = cand[np.argmin(np.abs(rates - pass_rate))] - 1e-3
            st_thr = min(st_thr, 0.6 * s_T)
            calib.keep(votes >= float(np.float32(st_thr)) - 1e-4)
            calibrated = True
        else:
            v = _norm_values(coefs, negs)
            votes = np.where(v >= np.array(thr)[None], np.array(rv)[None], np.array(lv)[None]).sum(axis=1)
            # achievable vote sums are discrete: take the cut whose noise pass rate is closest
            cand = np.unique(votes)
            rates = np.array([(votes >= cnd).mean() for cnd in cand])
            st_thr = cand[np.argmin(np.abs(rates - pass_rate))] - 1e-3
        if not calibrated and (si >= open_stages or calib is not None):
            frac = agree_lo + (agree_hi - agree_lo) * min(1.0, max(0, si - open_stages) / 6.0)
            st_thr = max(st_thr, s_T * (2 * frac - 1))
        st_thr = min(st_thr, 0.6 * s_T)              # the template keeps a wide margin
        out_stages.append(dict(features=feats, thresholds=thr, left=lv, right=rv,
                               stage_threshold=float(st_thr)))
    return dict(name="synthetic_frontalface", size=(win, win), stages=out_stages)


def _f(v):
    return "%.9g" % float(np.float32(v))


def cascade_to_xml(casc):
    """Old-format OpenCV Haar cascade XML (type_id opencv-haar-classifier).

    A stage is either the stump form {features, thresholds, left, right, stage_threshold [, tilted]} (one root node per
    weak classifier; `tilted`: per-feature 0/1) or the general form {trees, stage_threshold}: `trees` is a list of weak
    classifiers, each a list of nodes {feature, tilted, threshold, left, right} whose left / right is ("val", v) for a
    leaf or ("node", i) for the index of a later node of the same tree (icvReadHaarClassifier's <left_node>)."""
    L = ['<?xml version="1.0"?>', "<opencv_storage>",
         '<%s type_id="opencv-haar-classifier">' % casc["name"],
         "  <size>%d %d</size>" % casc["size"], "  <stages>"]
    for si, st in enumerate(casc["stages"]):
        if "trees" in st:
            trees = st["trees"]
        else:
            tl = st.get("tilted", [0] * len(st["features"]))
            trees = [[dict(feature=f, tilted=tl[j], threshold=st["thresholds"][j], left=("val", st["left"][j]),
                           right=("val", st["right"][j]))] for j, f in enumerate(st["features"])]
        L += ["    <_>", "      <!-- stage %d -->" % si, "      <trees>"]
        for j, tree in enumerate(trees):
            L += ["        <_>", "          <!-- tree %d -->" % j]
            for k, nd in enumerate(tree):
                L += ["          <_>", "            <!-- %s -->" % ("root node" if k == 0 else "node %d" % k), "            <feature>", "              <rects>"]
                for (x, y, w, h, wt) in nd["feature"]:
                    L.append("                <_>%d %d %d %d %d.</_>" % (x, y, w, h, int(wt)))
                L += ["              </rects>", "              <tilted>%d</tilted></feature>" % int(nd.get("tilted", 0)),
                      "            <threshold>%s</threshold>" % _f(nd["threshold"])]
                for side in ("left", "right"):
                    kind, v = nd[side]
                    L.append("            <%s_%s>%s</%s_%s>" % (side, kind, _f(v) if kind == "val" else "%d" % v, side, kind))
                L[-1] += "</_>"
            L[-1] += "</_>"
        L += ["      </trees>", "      <stage_threshold>%s</stage_threshold>" % _f(st["stage_threshold"]),
              "      <parent>%d</parent>" % (si - 1), "      <next>-1</next></_>"]
    L += ["  </stages></%s>" % casc["name"], "</opencv_storage>", ""]
    return "\n".join(L)


def _rand_tilted_feature(rng, ow, oh):
    """A tilted (45 degree) two-rectangle feature inside the window: rect (x, y, w, h) tilted covers columns x-h .. x+w and
    rows y .. y+w+h (OpenCV's convention: w along the down-right diagonal, h along the down-left one)."""
    for _ in range(200):
        w, h = int(rng.randint(1, max(2, ow // 3))) * 2, int(rng.randint(1, max(2, oh // 3)))
        x, y = int(rng.randint(0, ow)), int(rng.randint(0, oh))
        if x - h < 1 or x + w > ow - 1 or y < 1 or y + w + h > oh - 1:
            continue
        if rng.rand() < 0.5:       # halves along w
            return [(x, y, w, h, -1.0), (x, y, w // 2, h, 2.0)]
        if h % 2 == 0:             # halves along h
            return [(x, y, w, h, -1.0), (x, y, w, h // 2, 2.0)]
    raise RuntimeError("tilted feature sampling failed")


def _rand_upright_feature(rng, ow, oh):
    while True:
        w, h = int(rng.randint(2, ow + 1)), int(rng.randint(2, oh + 1))
        x, y = int(rng.randint(0, ow - w + 1)), int(rng.randint(0, oh - h + 1))
        kind = int(rng.randint(0, 4))
        if kind == 0 and w % 2 == 0:
            return [(x, y, w, h, -1.0), (x + w // 2, y, w // 2, h, 2.0)]
        if kind == 1 and h % 2 == 0:
            return [(x, y, w, h, -1.0), (x, y + h // 2, w, h // 2, 2.0)]
        if kind == 2 and w % 3 == 0:
            return [(x, y, w, h, -1.0), (x + w // 3, y, w // 3, h, 3.0)]
        if kind == 3 and w % 2 == 0 and h % 2 == 0:
            return [(x, y, w, h, -1.0), (x, y, w // 2, h // 2, 2.0), (x + w // 2, y + h // 2, w // 2, h // 2, 2.0)]


def make_generic_cascade(ow=20, oh=20, seed=1, stage_sizes=(3, 8, 12, 16, 20, 24, 28), tilt_frac=0.25, tree_frac=0.35, max_nodes=3):
    """A lenient cascade that exercises what haarcascade_profileface / the mcs_* files may contain:
    tilted features and tree-structured weak classifiers (up to `max_nodes` nodes, children always later nodes).  Votes are
    symmetric around zero and thresholds near zero, so about half of all windows pass each stage on any image and a handful
    survive every stage.  A workload / parity generator, not a detector."""
    rng = np.random.RandomState(seed)
    stages = []
    for n in stage_sizes:
        trees = []
        for _ in range(n):
            nn = int(rng.randint(2, max_nodes + 1)) if rng.rand() < tree_frac else 1
            nodes = []
            next_free = 1                       # nodes are handed out to parents in index order: a proper binary tree, nn + 1 leaves
            for k in range(nn):
                tilted = 1 if rng.rand() < tilt_frac else 0
                feat = _rand_tilted_feature(rng, ow, oh) if tilted else _rand_upright_feature(rng, ow, oh)
                a = float(rng.uniform(0.3, 1.0))
                avail = nn - next_free
                lo = 1 if (next_free == k + 1 and avail > 0) else 0      # the next node must hang somewhere before its turn comes
                take = int(rng.randint(lo, min(2, avail) + 1)) if avail > 0 else 0
                sides = [("node", next_free + j) for j in range(take)]
                next_free += take
                v = a if rng.rand() < 0.5 else -a
                while len(sides) < 2:
                    sides.append(("val", v)); v = -v
                if rng.rand() < 0.5:
                    sides.reverse()
                nodes.append(dict(feature=feat, tilted=tilted, threshold=float(rng.normal(0, 0.02)), left=sides[0], right=sides[1]))
            trees.append(nodes)
        stages.append(dict(trees=trees, stage_threshold=float(rng.uniform(-0.3, 0.1))))
    return dict(name="generic_%dx%d" % (ow, oh), size=(ow, oh), stages=stages)


def generic_cascade_xml(**kw):
    return cascade_to_xml(make_generic_cascade(**kw))


def synthetic_cascade_xml(seed=2016, stages=None):
    return cascade_to_xml(make_cascade(seed=seed, stages=stages))


# ------------------------------------------------------------------ calibration on frame content
def equalize_np(g):
    """cv::equalizeHist as numpy (workload generation only: the checker and the kernels have their own)."""
    hist = np.bincount(g.ravel(), minlength=256)
    nz = np.nonzero(hist)[0]
    if len(nz) <= 1:
        return g.copy()
    i0 = nz[0]
    scale = 255.0 / (g.size - hist[i0])
    c = np.cumsum(hist) - hist[:i0 + 1].sum()
    lut = np.clip(np.rint(np.maximum(c, 0) * scale), 0, 255).astype(np.uint8)
    lut[:i0 + 1] = 0
    return lut[g]


def scan_ladder(ow, oh, cols, rows, scale_factor=1.1, min_size=(0, 0)):
    """The factors cvHaarDetectObjectsForROC's scale-cascade branch evaluates."""
    n, f = 0, 1.0
    while f * ow < cols - 10 and f * oh < rows - 10:
        n += 1; f *= scale_factor
    out, f = [], 1.0
    for _ in range(n):
        if int(np.rint(ow * f)) >= min_size[0] and int(np.rint(oh * f)) >= min_size[1]:
            out.append(f)
        f *= scale_factor
    return out


class WindowSample:
    """Every window a scale-cascade scan visits on a few gray images (OpenCV's grid: stride max(2, factor), origins cvRound(i * stride)),
    with the arithmetic of cvSetImagesForHaarClassifierCascade / cvRunHaarClassifierCascadeSum in float64: scaled rectangles
    cvRound(v * factor), weights over the variance window's area with rectangle 0 re-balanced, value compared with
    threshold * std of the window.  make_cascade() walks it stage by stage, keeping the windows that pass."""

    def __init__(self, images, win=WIN, scale_factor=1.1, min_size=None):
        self.win = win
        self.planes = []          # (S flat, pitch)
        self.groups = []          # per (image, factor): dict(img, f, off [n] int64, vnf [n])
        rnd = lambda v: int(np.rint(v))
        for gi, g in enumerate(images):
            g = np.asarray(g, np.uint8)
            H, W = g.shape
            S = np.zeros((H + 1, W + 1), np.int64); S[1:, 1:] = g.astype(np.int64).cumsum(0).cumsum(1)
            Q = np.zeros((H + 1, W + 1), np.int64); Q[1:, 1:] = (g.astype(np.int64) ** 2).cumsum(0).cumsum(1)
            P = W + 1
            self.planes.append((S.ravel(), P))
            ms = (W // 20, H // 20) if min_size is None else min_size
            for f in scan_ladder(win, win, W, H, scale_factor, ms):
                step = max(2.0, f)
                ww = rnd(win * f)
                ex = np.rint(np.arange(rnd((W - ww) / step)) * step).astype(np.int64)
                ey = np.rint(np.arange(rnd((H - ww) / step)) * step).astype(np.int64)
                if not len(ex) or not len(ey):
                    continue
                off = (ey[:, None] * P + ex[None, :]).ravel()
                e0, ew = rnd(f), rnd((win - 2) * f)
                inv = 1.0 / (ew * ew)
                c = [off + e0 * P + e0, off + e0 * P + e0 + ew, off + (e0 + ew) * P + e0, off + (e0 + ew) * P + e0 + ew]
                Sf, Qf = S.ravel(), Q.ravel()
                mean = (Sf[c[0]] - Sf[c[1]] - Sf[c[2]] + Sf[c[3]]) * inv
                var = (Qf[c[0]] - Qf[c[1]] - Qf[c[2]] + Qf[c[3]]) * inv - mean * mean
                vnf = np.where(var >= 0, np.sqrt(np.maximum(var, 0)), 1.0)
                self.groups.append(dict(img=gi, f=f, off=off, vnf=vnf, inv=inv))
        self.total = self.alive_count()

    def alive_count(self):
        return int(sum(len(g["off"]) for g in self.groups))

    def stage_votes(self, feats, thr, lv, rv):
        rnd = lambda v: int(np.rint(v))
        out = []
        for g in self.groups:
            Sf, P = self.planes[g["img"]]
            f, off, inv = g["f"], g["off"], g["inv"]
            tot = np.zeros(len(off))
            if len(off):
                for feat, t, a0, a1 in zip(feats, thr, lv, rv):
                    rs, ws = [], []
                    for (x, y, w, h, wt) in feat:
                        tx, ty, tw, th = rnd(x * f), rnd(y * f), rnd(w * f), rnd(h * f)
                        rs.append((tx, ty, tw, th)); ws.append(wt * inv)
                    ws[0] = -sum(ws[k] * rs[k][2] * rs[k][3] for k in range(1, len(rs))) / (rs[0][2] * rs[0][3])
                    val = np.zeros(len(off))
                    for (tx, ty, tw, th), wk in zip(rs, ws):
                        o = off + ty * P + tx
                        val += wk * (Sf[o] - Sf[o + tw] - Sf[o + th * P] + Sf[o + th * P + tw])
                    tot += np.where(val >= np.float32(t) * g["vnf"], a1, a0)
            out.append(tot)
        return np.concatenate(out) if out else np.zeros(0)

    def keep(self, mask):
        k = 0
        for g in self.groups:
            n = len(g["off"]); m = mask[k:k + n]; k += n
            g["off"] = g["off"][m]; g["vnf"] = g["vnf"][m]


_CALIB_CACHE = {}


def calibrated_cascade_xml(seed=2016, stages=None, W=1920, H=1080, n_images=2, content="natural", scale_factor=1.1):
    """The stand-in cascade with its stage thresholds calibrated on the bench's own content: every stage lets about half of
    the windows that reach it through (windows of the equalised 1/f field at the scan's own scales -- haartraining's
    false-alarm target per stage), for as many stages as the sample supports (ten at 2 x 1080p); pasted templates still pass
    everything.  A trained cascade's selectivity profile: monotone, no stage that a re-ordering could exploit."""
    key = (seed, tuple(stages) if stages else None, W, H, n_images, content, scale_factor)
    if key not in _CALIB_CACHE:
        imgs = [equalize_np(make_gray(W, H, frame_seed(0, 1000 + i), content)) for i in range(n_images)]
        c = make_cascade(seed=seed, stages=stages, calib=WindowSample(imgs, scale_factor=scale_factor))
        c["name"] = "synthetic_frontalface_calibrated"
        _CALIB_CACHE[key] = cascade_to_xml(c)
    return _CALIB_CACHE[key]


PART_STAGES = [3, 9, 14, 19, 20, 27, 31, 34, 37, 42, 47, 50]     # a shorter cascade, like the mcs_* files


def synthetic_part_cascade_xml(name, seed=None):
    seed = {"righteye": 101, "lefteye": 102, "nose": 103, "mouth": 104, "leftear": 105, "rightear": 106}[name] if seed is None else seed
    c = make_cascade(seed=seed, stages=PART_STAGES, tmpl=part_template(name))
    c["name"] = "synthetic_" + name
    return cascade_to_xml(c)


# ------------------------------------------------------------------ frames
def _resize_bilinear_f(img, size):
    h, w = img.shape
    ys = (np.arange(size) + 0.5) * h / size - 0.5
    xs = (np.arange(size) + 0.5) * w / size - 0.5
    y0 = np.clip(np.floor(ys).astype(int), 0, h - 1); y1 = np.clip(y0 + 1, 0, h - 1)
    x0 = np.clip(np.floor(xs).astype(int), 0, w - 1); x1 = np.clip(x0 + 1, 0, w - 1)
    fy = np.clip(ys - np.floor(ys), 0, 1)[:, None]; fx = np.clip(xs - np.floor(xs), 0, 1)[None, :]
    a = img[y0][:, x0]; b = img[y0][:, x1]; c = img[y1][:, x0]; d = img[y1][:, x1]
    return (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy


def make_gray(W, H, seed, kind="noise", faces=()):
    """Seeded luminance field, uint8 [H,W].
    kind: 'noise' uniform u8; 'natural' 1/f multi-octave noise; 'gradient' smooth ramp +
    mild noise; 'flat'.
    faces: iterable of (x, y, size): TEMPLATE pasted at that box."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        g = rng.integers(0, 256, size=(H, W)).astype(np.float64)
    elif kind == "gradient":
        yy, xx = np.mgrid[0:H, 0:W]
        g = 40 + 170.0 * (0.6 * xx / max(W - 1, 1) + 0.4 * yy / max(H - 1, 1)) + rng.normal(0, 3.0, size=(H, W))
    elif kind == "natural":
        # 1/f-like field: equal-amplitude octaves of bilinearly upsampled value noise, so that
        # Haar responses do not vanish at large window scales the way they do on white noise
        g = np.zeros((H, W))
        cell, n_oct = 2, 0
        while cell <= max(W, H):
            gh, gw = H // cell + 3, W // cell + 3
            grid = rng.uniform(-1, 1, size=(gh, gw))
            ys = np.arange(H) / cell; xs = np.arange(W) / cell
            y0 = ys.astype(int); x0 = xs.astype(int)
            fy = (ys - y0)[:, None]; fx = (xs - x0)[None, :]
            top = grid[y0][:, x0] * (1 - fx) + grid[y0][:, x0 + 1] * fx
            bot = grid[y0 + 1][:, x0] * (1 - fx) + grid[y0 + 1][:, x0 + 1] * fx
            g += top * (1 - fy) + bot * fy
            cell *= 2; n_oct += 1
        g += rng.uniform(-1, 1, size=(H, W))
        g = 128 + g * (100.0 / np.sqrt(n_oct + 1))
    elif kind == "flat":
        g = np.full((H, W), 128.0)
    else:
        raise ValueError(kind)
    g = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    return paste_faces(g, faces, seed) if len(faces) else g


def paste_faces(gray, faces, seed=0):
    """copy of `gray` with TEMPLATE pasted at every (x, y, size)"""
    rng = np.random.default_rng(seed ^ 0xFACE)
    g = gray.astype(np.float64)
    H, W = g.shape
    T = template()
    for (x, y, size) in faces:
        patch = _resize_bilinear_f(T, int(size)) + rng.normal(0, 2.0, size=(int(size), int(size)))
        g[y:y + size, x:x + size] = patch[:max(0, min(size, H - y)), :max(0, min(size, W - x))]
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def make_bgr(W, H, seed, kind="noise", faces=(), channels=3):
    """BGR (or BGRA) frame whose BGR2GRAY is close to make_gray's field."""
    return gray_to_bgr(make_gray(W, H, seed, kind, faces), seed, channels)


def gray_to_bgr(g, seed, channels=3):
    H, W = g.shape
    rng = np.random.default_rng(seed ^ 0x5EED)
    out = np.empty((H, W, channels), np.uint8)
    jitter = rng.integers(-6, 7, size=(H, W, 2))
    out[..., 0] = np.clip(g.astype(np.int32) + jitter[..., 0], 0, 255)
    out[..., 1] = g
    out[..., 2] = np.clip(g.astype(np.int32) + jitter[..., 1], 0, 255)
    if channels == 4:
        out[..., 3] = 255
    return out


def make_yuv420(W, H, seed, fmt, kind="natural", faces=(), pad=0, luma_rows=None, gap=0, chroma_pad=None):
    """A 4:2:0 frame as a decoder lays it out: (flat uint8 buffer, (format, offsets, strides)) with format 1 = NV12, 2 = I420 (the
    values of NVCA_PIX_*).  Y = 16 + gray * 219 / 255 of make_gray's field (limited range), chroma near 128 with small seeded
    noise.  pad: bytes added to every plane's row (chroma_pad: to the chroma planes' rows, where that differs); luma_rows: rows the luma plane is allocated with (1080 in 1088; the chroma
    planes likewise); gap: unused bytes between planes.  What no pixel lies in holds 0xA5."""
    assert W % 2 == 0 and H % 2 == 0 and fmt in (1, 2)
    g = make_gray(W, H, seed, kind, faces).astype(np.int32)
    rng = np.random.default_rng(seed ^ 0xC420)
    y = (16 + (g * 219 + 127) // 255).astype(np.uint8)
    u = (128 + rng.integers(-9, 10, size=(H // 2, W // 2))).astype(np.uint8)
    v = (128 + rng.integers(-9, 10, size=(H // 2, W // 2))).astype(np.uint8)
    rows = luma_rows or H
    assert rows >= H and rows % 2 == 0
    ys, cpad = W + pad, pad if chroma_pad is None else chroma_pad
    if fmt == 1:
        planes = [(y, ys, rows), (np.stack([u, v], axis=-1).reshape(H // 2, W), W + cpad, rows // 2)]
    else:
        planes = [(y, ys, rows), (u, W // 2 + cpad, rows // 2), (v, W // 2 + cpad, rows // 2)]
    offsets, strides, off = [], [], 0
    for (_, st, nr) in planes:
        offsets.append(off); strides.append(st)
        off += st * nr + gap
    buf = np.full(off - gap, 0xA5, np.uint8)
    for (p, st, nr), o in zip(planes, offsets):
        view = buf[o:o + st * nr].reshape(nr, st)
        view[:p.shape[0], :p.shape[1]] = p
    return buf, (fmt, offsets, strides)


# packed 4:2:2: format (the values of NVCA_PIX_YUY2 / _UYVY / _YVYU) -> positions of (Y0, U, V) within a pixel pair's four bytes; Y1 lies
# two bytes behind Y0
YUV422_POS = {4: (0, 1, 3), 5: (1, 0, 2), 6: (0, 3, 1)}


def pack_yuv422(y, u, v, fmt, pad=0, base=0, seed=0):
    """The planes y [H, W], u and v [H, W / 2] (a chroma sample per row and pixel pair) as a packed 4:2:2 buffer: (flat uint8 buffer,
    (format, offsets, strides)) with rows of 2 W + pad bytes from byte `base` on.  The buffer ends with the last row's last pixel; every
    byte that is no pixel (the bytes in front of the base, the row padding) holds seeded noise."""
    y, u, v = (np.asarray(a, np.uint8) for a in (y, u, v))
    H, W = y.shape
    assert W % 2 == 0 and u.shape == v.shape == (H, W // 2) and fmt in YUV422_POS
    py, pu, pv = YUV422_POS[fmt]
    stride = 2 * W + pad
    buf = np.random.default_rng(seed ^ 0xC422).integers(0, 256, size=base + stride * (H - 1) + 2 * W).astype(np.uint8)
    rows = np.zeros((H, W // 2, 4), np.uint8)
    rows[..., py], rows[..., py + 2], rows[..., pu], rows[..., pv] = y[:, 0::2], y[:, 1::2], u, v
    idx = base + np.arange(H)[:, None] * stride + np.arange(2 * W)[None, :]
    buf[idx] = rows.reshape(H, 2 * W)
    return buf, (fmt, [base, 0, 0], [stride, 0, 0])


def make_yuv422(W, H, seed, fmt, kind="natural", faces=(), pad=0, base=0):
    """A packed 4:2:2 frame as a camera lays it out (pack_yuv422's arrangement: byte order `fmt`, row padding, base offset, seeded noise
    in every byte that is no pixel).  Y = 16 + gray * 219 / 255 of make_gray's field, as make_yuv420; chroma around 128 with seeded noise
    that differs from ROW to row, one pair in eight at an extreme (16 or 240: a channel of the converted pixel saturates, and its gray value
    moves with the chroma): a reader that shares chroma between rows 2k and 2k + 1 converts another image."""
    assert W % 2 == 0
    g = make_gray(W, H, seed, kind, faces).astype(np.int32)
    rng = np.random.default_rng(seed ^ 0xC420)
    y = (16 + (g * 219 + 127) // 255).astype(np.uint8)
    u = (128 + rng.integers(-40, 41, size=(H, W // 2))).astype(np.uint8)
    v = (128 + rng.integers(-40, 41, size=(H, W // 2))).astype(np.uint8)
    salt = rng.integers(0, 8, size=(H, W // 2)) == 0
    u[salt] = rng.choice(np.array([16, 240], np.uint8), size=int(salt.sum()))
    v[salt] = rng.choice(np.array([16, 240], np.uint8), size=int(salt.sum()))
    return pack_yuv422(y, u, v, fmt, pad=pad, base=base, seed=seed)


def frame_seed(stream_id, frame_idx):
    """seed = 0xC0FFEE + stream_id*1000 + frame_idx."""
    return 0xC0FFEE + stream_id * 1000 + frame_idx


def calibrated_part_cascade_xml(name, seed=None, n_images=8, pass_rate=0.65):
    """A part detector's stand-in cascade with its stage thresholds calibrated the way calibrated_cascade_xml does it, on what the part
    searches scan: face regions of the working image (the face TEMPLATE at 88 .. 104 pixels -- a 560 .. 620-pixel face of a 1080p frame
    on the 320-pixel working image -- on the 1/f field, equalised), windows from 20 pixels up at OpenCV's grid.  Every early stage
    lets about two thirds of what reaches it through (pass_rate 0.65: with 0.5 the parts of the bench's faces lose neighbours to the
    stricter stages and a quarter of them falls below minNeighbors; the mcs_* files are short, lenient cascades too); the part's
    own template keeps its margin."""
    key = ("part", name, seed, n_images, pass_rate)
    if key not in _CALIB_CACHE:
        pseed = {"righteye": 101, "lefteye": 102, "nose": 103, "mouth": 104, "leftear": 105, "rightear": 106}[name] if seed is None else seed
        imgs = []
        for i in range(n_images):
            size = 88 + 2 * i
            g = make_gray(176, 176, 7000 + 13 * i + pseed, "natural", [(176 // 2 - size // 2, 176 // 2 - size // 2 + (i % 3) - 1, size)])
            imgs.append(equalize_np(g))
        c = make_cascade(seed=pseed, stages=PART_STAGES, tmpl=part_template(name), calib=WindowSample(imgs, scale_factor=1.1, min_size=(20, 20)), pass_rate=pass_rate)
        c["name"] = "synthetic_%s_calibrated" % name
        _CALIB_CACHE[key] = cascade_to_xml(c)
    return _CALIB_CACHE[key]


# ------------------------------------------------------------------ new-format LBP cascades
_LBP_BITS = ((0, 0, 128), (0, 1, 64), (0, 2, 32), (1, 2, 16), (2, 2, 8), (2, 1, 4), (2, 0, 2), (1, 0, 1))


def _lbp_codes(S, feat, xs, ys):
    """LBP codes of feature (x, y, w, h) at the window origins ys x xs of an image with integral S: [len(ys), len(xs)] ints"""
    x, y, w, h = feat
    P = [[S[np.ix_(ys + y + r * h, xs + x + c * w)] for c in range(4)] for r in range(4)]
    cell = [[P[r][c] - P[r][c + 1] - P[r + 1][c] + P[r + 1][c + 1] for c in range(3)] for r in range(3)]
    code = np.zeros(cell[0][0].shape, np.int64)
    for r, c, bit in _LBP_BITS:
        code += bit * (cell[r][c] >= cell[1][1])
    return code


def _integral_np(img):
    S = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(img.astype(np.int64), axis=0), axis=1)
    return S


def lbp_template(ow, oh):
    """TEMPLATE stretched to an ow x oh window (float)"""
    T = template()
    n = T.shape[0]
    ys = (np.arange(oh) + 0.5) * n / oh - 0.5
    xs = (np.arange(ow) + 0.5) * n / ow - 0.5
    y0 = np.clip(np.floor(ys).astype(int), 0, n - 2); x0 = np.clip(np.floor(xs).astype(int), 0, n - 2)
    fy = np.clip(ys - y0, 0, 1)[:, None]; fx = np.clip(xs - x0, 0, 1)[None, :]
    return (T[y0][:, x0] * (1 - fx) + T[y0][:, x0 + 1] * fx) * (1 - fy) + (T[y0 + 1][:, x0] * (1 - fx) + T[y0 + 1][:, x0 + 1] * fx) * fy


def paste_lbp_faces(gray, faces, ow, oh, seed=0):
    """copy of `gray` with the ow x oh template pasted at every (x, y, scale): a box of round(ow * scale) x round(oh * scale)"""
    rng = np.random.default_rng(seed ^ 0x1B9)
    g = gray.astype(np.float64)
    H, W = g.shape
    for (x, y, scale) in faces:
        w, h = int(round(ow * scale)), int(round(oh * scale))
        patch = lbp_template(w, h) + rng.normal(0, 1.0, size=(h, w))
        g[y:y + h, x:x + w] = patch[:max(0, min(h, H - y)), :max(0, min(w, W - x))]
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def lbp_calibration_images(n=4, W=320, H=240):
    """the images make_lbp_cascade calibrates on by default: seeds no test image uses (frame_seed(7, 9000 + i))"""
    return [make_gray(W, H, frame_seed(7, 9000 + i), "natural") for i in range(n)]


def make_lbp_cascade(ow=24, oh=24, seed=1, stage_sizes=(3, 4, 5, 6, 7, 8, 9), pass_rate=0.5, calibrate_on=None):
    """A new-format LBP cascade of stumps as a dict: size=(ow, oh), features=[(x, y, w, h)], stages=[dict(threshold=the file's
    value, weak=[dict(feature=index, subset=[8 int32], leaves=(l0, l1))])].  Every weak classifier votes its higher leaf for the
    stretched TEMPLATE (and for the codes one bit away from the template's), so pasted templates pass every stage; the stage
    thresholds are calibrated on `calibrate_on` (gray images disjoint from any test image; default lbp_calibration_images()) so
    that each stage passes about `pass_rate` of the windows that reach it, for as long as the sample lasts."""
    rng = np.random.default_rng(seed)
    imgs = lbp_calibration_images() if calibrate_on is None else list(calibrate_on)
    tmpl = np.clip(np.rint(lbp_template(ow, oh)), 0, 255).astype(np.uint8)
    St = _integral_np(tmpl)
    z = np.zeros(1, np.int64)
    # the calibration sample: every second window of each image and of its 2x decimation
    sample = []
    for im in imgs:
        for lev in (im, im[::2, ::2]):
            if lev.shape[0] > oh and lev.shape[1] > ow:
                sample.append((_integral_np(lev), np.arange(0, lev.shape[1] - ow, 2), np.arange(0, lev.shape[0] - oh, 2)))
    alive = [np.ones((len(ys), len(xs)), bool) for (_, xs, ys) in sample]
    features, stages = [], []
    for n in stage_sizes:
        weak, sums, hi = [], [np.zeros(a.shape, np.float32) for a in alive], np.float32(0)
        for _ in range(n):
            w = int(rng.integers(1, max(2, ow // 3 + 1))); h = int(rng.integers(1, max(2, oh // 3 + 1)))
            x = int(rng.integers(0, ow - 3 * w + 1)); y = int(rng.integers(0, oh - 3 * h + 1))
            features.append((x, y, w, h))
            ct = int(_lbp_codes(St, features[-1], z, z)[0, 0])
            good = np.zeros(256, bool)
            good[rng.random(256) < 0.3] = True
            good[[ct] + [ct ^ (1 << b) for b in range(8)]] = True
            a, b = np.float32(rng.uniform(0.3, 1.0)), np.float32(rng.uniform(0.3, 1.0))
            flip = bool(rng.integers(0, 2))                 # which leaf is the high one: a set subset bit selects leaves[0]
            bits = good if not flip else ~good
            words = np.packbits(bits.reshape(8, 32), axis=1, bitorder="little").view("<u4").reshape(8).astype(np.uint32).view(np.int32)
            leaves = (float(a), float(-b)) if not flip else (float(-b), float(a))
            weak.append(dict(feature=len(features) - 1, subset=[int(v) for v in words], leaves=leaves))
            hi = np.float32(hi + a)
            lut = np.where(bits, np.float32(leaves[0]), np.float32(leaves[1])).astype(np.float32)
            for k, (S, xs, ys) in enumerate(sample):
                sums[k] = (sums[k] + lut[_lbp_codes(S, features[-1], xs, ys)]).astype(np.float32)
        reach = np.concatenate([s[a] for s, a in zip(sums, alive)]) if alive else np.zeros(0, np.float32)
        thr = float(np.quantile(reach, 1.0 - pass_rate)) if len(reach) >= 16 else 0.35 * float(hi)
        thr = min(thr, 0.7 * float(hi))                     # pasted templates (every vote high, but for noise) stay in
        thr = float(np.float32(thr))
        alive = [a & (s >= np.float32(thr)) for s, a in zip(sums, alive)]
        stages.append(dict(threshold=thr, weak=weak))
    return dict(name="synthetic_lbp", size=(ow, oh), features=features, stages=stages)


def lbp_cascade_to_xml(casc, style="traincascade"):
    """The cascade as opencv_traincascade writes it (style "traincascade": every stageParams / featureParams field, stage
    comments) or as lbpcascade_frontalface.xml holds it (style "minimal": stageParams with maxWeakCount alone)."""
    assert style in ("traincascade", "minimal")
    ow, oh = casc["size"]
    mwc = max(len(s["weak"]) for s in casc["stages"])
    o = ['<?xml version="1.0"?>', "<opencv_storage>", '<cascade type_id="opencv-cascade-classifier">', "  <stageType>BOOST</stageType>",
         "  <featureType>LBP</featureType>", "  <height>%d</height>" % oh, "  <width>%d</width>" % ow, "  <stageParams>"]
    if style == "traincascade":
        o += ["    <boostType>GAB</boostType>", "    <minHitRate>9.9500000476837158e-01</minHitRate>", "    <maxFalseAlarm>5.0000000000000000e-01</maxFalseAlarm>",
              "    <weightTrimRate>9.4999999999999996e-01</weightTrimRate>", "    <maxDepth>1</maxDepth>"]
    o += ["    <maxWeakCount>%d</maxWeakCount></stageParams>" % mwc, "  <featureParams>", "    <maxCatCount>256</maxCatCount>"]
    if style == "traincascade":
        o += ["    <featSize>1</featSize>"]
    o[-1] += "</featureParams>"
    o += ["  <stageNum>%d</stageNum>" % len(casc["stages"]), "  <stages>"]
    for si, st in enumerate(casc["stages"]):
        if style == "traincascade":
            o.append("    <!-- stage %d -->" % si)
        o += ["    <_>", "      <maxWeakCount>%d</maxWeakCount>" % len(st["weak"]), "      <stageThreshold>%s</stageThreshold>" % _f(st["threshold"]), "      <weakClassifiers>"]
        for w in st["weak"]:
            o += ["        <_>", "          <internalNodes>", "            0 -1 %d %s</internalNodes>" % (w["feature"], " ".join(str(int(v)) for v in w["subset"])),
                  "          <leafValues>", "            %s %s</leafValues></_>" % (_f(w["leaves"][0]), _f(w["leaves"][1]))]
        o += ["      </weakClassifiers></_>"]
    o += ["  </stages>", "  <features>"]
    for (x, y, w, h) in casc["features"]:
        o += ["    <_>", "      <rect>", "        %d %d %d %d</rect></_>" % (x, y, w, h)]
    o += ["  </features></cascade>", "</opencv_storage>", ""]
    return "\n".join(o)


def lbp_cascade_xml(style="traincascade", **kw):
    return lbp_cascade_to_xml(make_lbp_cascade(**kw), style)


# ------------------------------------------------------------------ new-format HAAR cascades
def _rand_haar_new_feature(rng, ow, oh):
    """rects [(x, y, w, h, weight)] of a feature as opencv_traincascade's HAAR set has them (whole support -1, a part +2 / +3), one in
    ten a single rect of weight 1"""
    for _ in range(1000):
        w, h = int(rng.integers(2, ow + 1)), int(rng.integers(2, oh + 1))
        x, y = int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1))
        kind = int(rng.integers(0, 10))
        if kind in (0, 1) and w % 2 == 0:
            return [(x, y, w, h, -1.0), (x + w // 2, y, w // 2, h, 2.0)]
        if kind in (2, 3) and h % 2 == 0:
            return [(x, y, w, h, -1.0), (x, y + h // 2, w, h // 2, 2.0)]
        if kind == 4 and w % 3 == 0:
            return [(x, y, w, h, -1.0), (x + w // 3, y, w // 3, h, 3.0)]
        if kind == 5 and h % 3 == 0:
            return [(x, y, w, h, -1.0), (x, y + h // 3, w, h // 3, 3.0)]
        if kind in (6, 7, 8) and w % 2 == 0 and h % 2 == 0:
            return [(x, y, w, h, -1.0), (x, y, w // 2, h // 2, 2.0), (x + w // 2, y + h // 2, w // 2, h // 2, 2.0)]
        if kind == 9:
            return [(x, y, w, h, 1.0)]
    raise RuntimeError("feature sampling failed")


def _haar_new_values(S, Q, rects, ow, oh, xs, ys):
    """feature value * vnf at the window origins ys x xs (f64: good enough to calibrate thresholds on, not the evaluator's arithmetic)"""
    def rs(A, x, y, w, h):
        return A[np.ix_(ys + y, xs + x)] - A[np.ix_(ys + y, xs + x + w)] - A[np.ix_(ys + y + h, xs + x)] + A[np.ix_(ys + y + h, xs + x + w)]
    vs, vq = rs(S, 1, 1, ow - 2, oh - 2).astype(np.float64), rs(Q, 1, 1, ow - 2, oh - 2).astype(np.float64)
    nf = (ow - 2) * (oh - 2) * vq - vs * vs
    nf = np.where(nf > 0, np.sqrt(np.maximum(nf, 0)), 1.0)
    v = sum(wt * rs(S, x, y, w, h).astype(np.float64) for (x, y, w, h, wt) in rects)
    return v / nf


def _integral_pair_np(img):
    return _integral_np(img), _integral_np(img.astype(np.int64) ** 2)


def make_haar_new_cascade(ow=24, oh=24, seed=1, stage_sizes=(3, 4, 5, 6, 7, 8, 9), pass_rate=0.5, calibrate_on=None):
    """A new-format HAAR cascade of stumps as a dict: size=(ow, oh), features=[[(x, y, w, h, weight)] of 1 to 3 rects], stages=[dict(
    threshold=the file's value, weak=[dict(feature=index, threshold=t, leaves=(l0, l1))])].  Every stump puts the stretched TEMPLATE on
    the side of its higher leaf, with a margin, so pasted templates pass every stage; the stage thresholds are calibrated the way
    make_lbp_cascade's are: on `calibrate_on` (default lbp_calibration_images()), each stage passing about `pass_rate` of the windows
    that reach it, for as long as the sample lasts."""
    rng = np.random.default_rng(seed)
    imgs = lbp_calibration_images() if calibrate_on is None else list(calibrate_on)
    tmpl = np.clip(np.rint(lbp_template(ow, oh)), 0, 255).astype(np.uint8)
    St, Qt = _integral_pair_np(tmpl)
    z = np.zeros(1, np.int64)
    sample = []
    for im in imgs:
        for lev in (im, im[::2, ::2]):
            if lev.shape[0] > oh and lev.shape[1] > ow:
                sample.append(_integral_pair_np(lev) + (np.arange(0, lev.shape[1] - ow, 2), np.arange(0, lev.shape[0] - oh, 2)))
    alive = [np.ones((len(ys), len(xs)), bool) for (_, _, xs, ys) in sample]
    features, stages = [], []
    for n in stage_sizes:
        weak, sums, hi = [], [np.zeros(a.shape, np.float64) for a in alive], 0.0
        while len(weak) < n:
            rects = _rand_haar_new_feature(rng, ow, oh)
            vT = float(_haar_new_values(St, Qt, rects, ow, oh, z, z)[0, 0])
            if abs(vT) < 1e-3:
                continue                                    # the template does not tell the sides of this feature apart
            thr = float(np.float32(0.4 * vT if len(rects) > 1 else vT * (0.8 if vT > 0 else 1.2)))
            a, b = float(np.float32(rng.uniform(0.3, 1.0))), float(np.float32(rng.uniform(0.3, 1.0)))
            leaves = (-b, a) if vT >= thr else (a, -b)      # value < threshold takes leaves[0]
            features.append(rects)
            weak.append(dict(feature=len(features) - 1, threshold=thr, leaves=leaves))
            hi += a
            for k, (S, Q, xs, ys) in enumerate(sample):
                sums[k] = sums[k] + np.where(_haar_new_values(S, Q, rects, ow, oh, xs, ys) < thr, leaves[0], leaves[1])
        reach = np.concatenate([s[a] for s, a in zip(sums, alive)]) if alive else np.zeros(0)
        st_thr = float(np.quantile(reach, 1.0 - pass_rate)) if len(reach) >= 16 else 0.35 * hi
        st_thr = float(np.float32(min(st_thr, 0.7 * hi)))    # pasted templates (every vote high, but for noise) stay in
        alive = [a & (s >= st_thr) for s, a in zip(sums, alive)]
        stages.append(dict(threshold=st_thr, weak=weak))
    return dict(name="synthetic_haar_new", size=(ow, oh), features=features, stages=stages)


def haar_new_cascade_to_xml(casc, style="traincascade"):
    """The cascade as opencv_traincascade -featureType HAAR writes it (style "traincascade": every stageParams / featureParams field,
    stage comments) or as OpenCV's own converted haarcascade_*.xml hold it (style "minimal": maxWeakCount and maxCatCount alone)."""
    assert style in ("traincascade", "minimal")
    ow, oh = casc["size"]
    mwc = max(len(s["weak"]) for s in casc["stages"])
    o = ['<?xml version="1.0"?>', "<opencv_storage>", '<cascade type_id="opencv-cascade-classifier">', "  <stageType>BOOST</stageType>",
         "  <featureType>HAAR</featureType>", "  <height>%d</height>" % oh, "  <width>%d</width>" % ow, "  <stageParams>"]
    if style == "traincascade":
        o += ["    <boostType>GAB</boostType>", "    <minHitRate>9.9500000476837158e-01</minHitRate>", "    <maxFalseAlarm>5.0000000000000000e-01</maxFalseAlarm>",
              "    <weightTrimRate>9.4999999999999996e-01</weightTrimRate>", "    <maxDepth>1</maxDepth>"]
    o += ["    <maxWeakCount>%d</maxWeakCount></stageParams>" % mwc, "  <featureParams>", "    <maxCatCount>0</maxCatCount>"]
    if style == "traincascade":
        o += ["    <featSize>1</featSize>", "    <mode>ALL</mode>"]
    o[-1] += "</featureParams>"
    o += ["  <stageNum>%d</stageNum>" % len(casc["stages"]), "  <stages>"]
    for si, st in enumerate(casc["stages"]):
        if style == "traincascade":
            o.append("    <!-- stage %d -->" % si)
        o += ["    <_>", "      <maxWeakCount>%d</maxWeakCount>" % len(st["weak"]), "      <stageThreshold>%s</stageThreshold>" % _f(st["threshold"]), "      <weakClassifiers>"]
        for w in st["weak"]:
            o += ["        <_>", "          <internalNodes>", "            0 -1 %d %s</internalNodes>" % (w["feature"], _f(w["threshold"])),
                  "          <leafValues>", "            %s %s</leafValues></_>" % (_f(w["leaves"][0]), _f(w["leaves"][1]))]
        o += ["      </weakClassifiers></_>"]
    o += ["  </stages>", "  <features>"]
    for rects in casc["features"]:
        o += ["    <_>", "      <rects>"]
        for (x, y, w, h, wt) in rects:
            o += ["        <_>", "          %d %d %d %d %s</_>" % (x, y, w, h, _f(wt) + ("." if float(wt) == int(wt) and abs(float(wt)) < 1e6 else ""))]
        o += ["      </rects>", "      <tilted>0</tilted></_>"]
    o += ["  </features></cascade>", "</opencv_storage>", ""]
    return "\n".join(o)


def haar_new_cascade_xml(style="traincascade", **kw):
    return haar_new_cascade_to_xml(make_haar_new_cascade(**kw), style)


def haar_old_to_new_dict(casc):
    """An old-format cascade dict of stumps on upright features (make_cascade's: per stage features / thresholds / left / right /
    stage_threshold) as a new-format HAAR dict: one feature per stump, in file order; rects, weights, thresholds and votes as they
    stand.  The two formats are evaluated by different arithmetic, so this carries the workload's shape, not the answers."""
    features, stages = [], []
    for st in casc["stages"]:
        assert "trees" not in st and not any(st.get("tilted", [])), "stumps on upright features only"
        weak = []
        for j, f in enumerate(st["features"]):
            features.append([tuple(r) for r in f])
            weak.append(dict(feature=len(features) - 1, threshold=st["thresholds"][j], leaves=(st["left"][j], st["right"][j])))
        stages.append(dict(threshold=st["stage_threshold"], weak=weak))
    return dict(name=casc.get("name", "converted") + "_new", size=tuple(casc["size"]), features=features, stages=stages)


def haar_old_xml_to_new_xml(xml, style="minimal"):
    """the same for an old-format XML text of stumps on upright features (synthetic_cascade_xml's, calibrated_cascade_xml's)"""
    import xml.etree.ElementTree as ET
    c = ET.fromstring(xml)[0]
    assert c.get("type_id") == "opencv-haar-classifier"
    ow, oh = (int(v) for v in c.findtext("size").split())
    stages = []
    for st in c.find("stages"):
        feats, thr, lv, rv = [], [], [], []
        for tree in st.find("trees"):
            nodes = list(tree)
            assert len(nodes) == 1 and int(nodes[0].find("feature").findtext("tilted")) == 0, "stumps on upright features only"
            nd = nodes[0]
            feats.append([tuple([int(v) for v in r.text.split()[:4]] + [float(r.text.split()[4])]) for r in nd.find("feature").find("rects")])
            thr.append(float(nd.findtext("threshold"))); lv.append(float(nd.findtext("left_val"))); rv.append(float(nd.findtext("right_val")))
        stages.append(dict(features=feats, thresholds=thr, left=lv, right=rv, stage_threshold=float(st.findtext("stage_threshold"))))
    return haar_new_cascade_to_xml(haar_old_to_new_dict(dict(name=c.tag, size=(ow, oh), stages=stages)), style)


# ------------------------------------------------------------------ general new-format HAAR cascades: trees, tilted features
def _tilted_integral_np(img):
    """cv::integral's third plane, (h + 1) x (w + 1) int64, by its row recurrence T(X, Y) = T(X - 1, Y - 1) + T(X + 1, Y - 1) - T(X, Y - 2)
    + p(X - 1, Y - 1) + p(X - 1, Y - 2) on an image padded with h + 1 zero columns either side (calibration only; the statement of the
    definition is tests/haar_tree_reference.py's)"""
    h, w = img.shape
    pad = h + 1
    p = np.zeros((h + 1, w + 2 * pad + 2), np.int64)          # p[y + 1, X]: pixel (X - 1 - pad, y); row 0: the row above the image
    p[1:, pad + 1:pad + 1 + w] = img
    T = np.zeros((h + 1, w + 2 * pad + 2), np.int64)
    for Y in range(1, h + 1):
        T[Y, 1:-1] = T[Y - 1, :-2] + T[Y - 1, 2:] + p[Y, 1:-1] + p[Y - 1, 1:-1]
        if Y >= 2:
            T[Y, 1:-1] -= T[Y - 2, 1:-1]
    return T[:, pad:pad + w + 1].copy()


def _haar_tree_values(S, Q, T, rects, tilted, ow, oh, xs, ys):
    """_haar_new_values for a feature that may be tilted: its rects on T by CV_TILTED_PTRS, the file's weights as they stand"""
    if not tilted:
        return _haar_new_values(S, Q, rects, ow, oh, xs, ys)

    def at(A, x, y):
        return A[np.ix_(ys + y, xs + x)].astype(np.float64)

    def norm(A):
        return at(A, 1, 1) - at(A, ow - 1, 1) - at(A, 1, oh - 1) + at(A, ow - 1, oh - 1)
    vs, vq = norm(S), norm(Q)
    nf = (ow - 2) * (oh - 2) * vq - vs * vs
    nf = np.where(nf > 0, np.sqrt(np.maximum(nf, 0)), 1.0)
    v = sum(wt * (at(T, x, y) - at(T, x - h, y + h) - at(T, x + w, y + w) + at(T, x + w - h, y + w + h)) for (x, y, w, h, wt) in rects)
    return v / nf


def _rand_tree_shape(rng, nn):
    """[(left, right)] of a binary tree of nn nodes: a child > 0 is a later node, <= 0 the leaf -child (nn + 1 leaves, numbered as they come)"""
    next_free, next_leaf, out = 1, 0, []
    for k in range(nn):
        avail = nn - next_free
        lo = 1 if (next_free == k + 1 and avail > 0) else 0          # the next node must hang somewhere before its turn comes
        take = int(rng.randint(lo, min(2, avail) + 1)) if avail > 0 else 0
        sides = [next_free + j for j in range(take)]
        next_free += take
        while len(sides) < 2:
            sides.append(-next_leaf); next_leaf += 1
        if rng.rand() < 0.5:
            sides.reverse()
        out.append((sides[0], sides[1]))
    return out


def make_haar_tree_cascade(ow=24, oh=24, seed=1, stage_sizes=(3, 4, 5, 6, 7, 8), pass_rate=0.5, tilt_frac=0.25, tree_frac=0.5, max_nodes=3,
                           calibrate_on=None):
    """A general new-format HAAR cascade as a dict: size, features=[[(x, y, w, h, weight)]], tilted=[0 | 1 per feature], stages=[dict(
    threshold, weak=[dict(nodes=[(left, right, feature, threshold)], leaves=[nodes + 1 values])])].  Calibrated the way
    make_haar_new_cascade is, on `calibrate_on` (default lbp_calibration_images()): a node's threshold is the median of its feature over the
    sample windows that reach the node, so both of its children are taken; a stage passes about `pass_rate` of the windows that reach it.
    A workload / parity generator, not a detector."""
    rng = np.random.RandomState(seed)
    imgs = lbp_calibration_images() if calibrate_on is None else list(calibrate_on)
    sample = []
    for im in imgs:
        for lev in (im, im[::2, ::2]):
            if lev.shape[0] > oh and lev.shape[1] > ow:
                sample.append(_integral_pair_np(lev) + (_tilted_integral_np(lev), np.arange(0, lev.shape[1] - ow, 2), np.arange(0, lev.shape[0] - oh, 2)))
    alive = [np.ones((len(ys), len(xs)), bool) for (_, _, _, xs, ys) in sample]
    features, tilted, stages = [], [], []
    for n in stage_sizes:
        weak, sums = [], [np.zeros(a.shape, np.float64) for a in alive]
        for _ in range(n):
            nn = int(rng.randint(2, max_nodes + 1)) if rng.rand() < tree_frac else 1
            shape = _rand_tree_shape(rng, nn)
            leaves = [float(np.float32(rng.uniform(0.3, 1.0) * (1 if rng.rand() < 0.5 else -1))) for _ in range(nn + 1)]
            at = [np.where(a, 0, -1) for a in alive]          # the node a sample window stands at (-1: not in this tree any more)
            nodes = []
            for k in range(nn):
                tl = 1 if rng.rand() < tilt_frac else 0
                rects = _rand_tilted_feature(rng, ow, oh) if tl else _rand_upright_feature(rng, ow, oh)
                vals = [_haar_tree_values(S, Q, T, rects, tl, ow, oh, xs, ys) for (S, Q, T, xs, ys) in sample]
                here = np.concatenate([v[a == k] for v, a in zip(vals, at)]) if sample else np.zeros(0)
                allv = np.concatenate([v.ravel() for v in vals]) if sample else np.zeros(1)
                thr = float(np.float32(np.median(here if len(here) >= 8 else allv)))
                features.append(rects); tilted.append(tl)
                nodes.append((shape[k][0], shape[k][1], len(features) - 1, thr))
                for i, (v, a) in enumerate(zip(vals, at)):
                    m = a == k
                    child = np.where(v < thr, shape[k][0], shape[k][1])
                    for c in set(shape[k]):
                        if c <= 0:
                            sums[i][m & (child == c)] += leaves[-c]
                    a[m] = np.where(child[m] > 0, child[m], -1)
            weak.append(dict(nodes=nodes, leaves=leaves))
        reach = np.concatenate([s[a] for s, a in zip(sums, alive)]) if alive else np.zeros(0)
        st_thr = float(np.float32(np.quantile(reach, 1.0 - pass_rate))) if len(reach) >= 16 else 0.0
        alive = [a & (s >= st_thr) for s, a in zip(sums, alive)]
        stages.append(dict(threshold=st_thr, weak=weak))
    return dict(name="synthetic_haar_tree", size=(ow, oh), features=features, tilted=tilted, stages=stages)


def haar_tree_cascade_to_xml(casc, style="traincascade"):
    """haar_new_cascade_to_xml for a general cascade dict (a stump cascade's dict is taken as well: its weak classifiers are the trees
    "0 -1"): internalNodes holds "left right featureIdx threshold" per node, leafValues one value more; <tilted> per feature; the
    "traincascade" header names the depth of the deepest tree as maxDepth"""
    assert style in ("traincascade", "minimal")
    ow, oh = casc["size"]
    tilted = casc.get("tilted", [0] * len(casc["features"]))

    def tree(w):
        return (w["nodes"], w["leaves"]) if "nodes" in w else ([(0, -1, w["feature"], w["threshold"])], list(w["leaves"]))

    def depth(nodes, k=0):
        return 1 + max([depth(nodes, c) for c in nodes[k][:2] if k < c < len(nodes)] or [0])          # (a damaged file's children are not followed)
    mwc = max(len(s["weak"]) for s in casc["stages"])
    md = max(depth(tree(w)[0]) for s in casc["stages"] for w in s["weak"])
    o = ['<?xml version="1.0"?>', "<opencv_storage>", '<cascade type_id="opencv-cascade-classifier">', "  <stageType>BOOST</stageType>",
         "  <featureType>HAAR</featureType>", "  <height>%d</height>" % oh, "  <width>%d</width>" % ow, "  <stageParams>"]
    if style == "traincascade":
        o += ["    <boostType>GAB</boostType>", "    <minHitRate>9.9500000476837158e-01</minHitRate>", "    <maxFalseAlarm>5.0000000000000000e-01</maxFalseAlarm>",
              "    <weightTrimRate>9.4999999999999996e-01</weightTrimRate>", "    <maxDepth>%d</maxDepth>" % md]
    o += ["    <maxWeakCount>%d</maxWeakCount></stageParams>" % mwc, "  <featureParams>", "    <maxCatCount>0</maxCatCount>"]
    if style == "traincascade":
        o += ["    <featSize>1</featSize>", "    <mode>ALL</mode>"]
    o[-1] += "</featureParams>"
    o += ["  <stageNum>%d</stageNum>" % len(casc["stages"]), "  <stages>"]
    for si, st in enumerate(casc["stages"]):
        if style == "traincascade":
            o.append("    <!-- stage %d -->" % si)
        o += ["    <_>", "      <maxWeakCount>%d</maxWeakCount>" % len(st["weak"]), "      <stageThreshold>%s</stageThreshold>" % _f(st["threshold"]), "      <weakClassifiers>"]
        for w in st["weak"]:
            nodes, leaves = tree(w)
            o += ["        <_>", "          <internalNodes>", "            %s</internalNodes>" % " ".join("%d %d %d %s" % (l, r, f, _f(t)) for (l, r, f, t) in nodes),
                  "          <leafValues>", "            %s</leafValues></_>" % " ".join(_f(v) for v in leaves)]
        o += ["      </weakClassifiers></_>"]
    o += ["  </stages>", "  <features>"]
    for rects, tl in zip(casc["features"], tilted):
        o += ["    <_>", "      <rects>"]
        for (x, y, w, h, wt) in rects:
            o += ["        <_>", "          %d %d %d %d %s</_>" % (x, y, w, h, _f(wt) + ("." if float(wt) == int(wt) and abs(float(wt)) < 1e6 else ""))]
        o += ["      </rects>", "      <tilted>%d</tilted></_>" % int(tl)]
    o += ["  </features></cascade>", "</opencv_storage>", ""]
    return "\n".join(o)


def haar_tree_cascade_xml(style="traincascade", **kw):
    return haar_tree_cascade_to_xml(make_haar_tree_cascade(**kw), style)


def haar_old_xml_to_tree_xml(xml, style="minimal"):
    """An old-format XML text with tree weak classifiers and tilted features (generic_cascade_xml's) as a general new-format HAAR text:
    one feature per node, in file order; a <left_val> / <right_val> becomes the next leaf of its tree, a <left_node> / <right_node> stays
    the node index it is; rects, weights, thresholds and values as they stand.  The two formats are evaluated by different arithmetic
    (no halved tilted weight, its own normaliser and scan), so this carries the workload's shape, not the answers."""
    import xml.etree.ElementTree as ET
    c = ET.fromstring(xml)[0]
    assert c.get("type_id") == "opencv-haar-classifier"
    ow, oh = (int(v) for v in c.findtext("size").split())
    features, tilted, stages = [], [], []
    for st in c.find("stages"):
        weak = []
        for tr in st.find("trees"):
            nodes, leaves = [], []
            for nd in tr:
                f = nd.find("feature")
                features.append([tuple([int(v) for v in r.text.split()[:4]] + [float(r.text.split()[4])]) for r in f.find("rects")])
                tilted.append(int(f.findtext("tilted")))
                sides = []
                for side in ("left", "right"):
                    if nd.find(side + "_node") is not None:
                        sides.append(int(nd.findtext(side + "_node")))
                    else:
                        sides.append(-len(leaves)); leaves.append(float(nd.findtext(side + "_val")))
                nodes.append((sides[0], sides[1], len(features) - 1, float(nd.findtext("threshold"))))
            weak.append(dict(nodes=nodes, leaves=leaves))
        stages.append(dict(threshold=float(st.findtext("stage_threshold")), weak=weak))
    return haar_tree_cascade_to_xml(dict(name=c.tag + "_new", size=(ow, oh), features=features, tilted=tilted, stages=stages), style)
