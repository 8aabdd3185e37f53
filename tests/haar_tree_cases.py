"""Cascades, images and constructed cases that tests/test_haar_tree_cpu.py (on the numpy statement, tests/haar_tree_reference.py) and
tests/test_gpu_haar_tree.py (on the device) share: general new-format HAAR cascades -- tree weak classifiers, tilted features (SURVEY.md
A.19).  Every expected list of a constructed case is written down here by hand, never taken from a run; the arithmetic behind each is
in its comment."""
import functools

import numpy as np

import haar_new_cases as HK
import haar_tree_reference as R
from nubovca import synth

# name -> make_haar_tree_cascade arguments (seeds for which tests/test_haar_tree_cpu.py's premises hold on the statement).  Six stages: the
# tile kernel takes stages 0 .. 2, then the stage groups [3, 5) and [5, 6); "t20": 20 x 20, "t24": 24 x 24, trees of up to 3 nodes;
# "deep4": trees of up to 7 nodes; "w82": a window too large for the LDS tile, stage 0 gathers from the plane
CASCADES = {
    "t20": dict(ow=20, oh=20, seed=5, stage_sizes=(3, 4, 5, 6, 7, 8), pass_rate=0.5),
    "t24": dict(ow=24, oh=24, seed=7, stage_sizes=(3, 4, 5, 6, 7, 8), pass_rate=0.5),
    "deep4": dict(ow=20, oh=20, seed=9, stage_sizes=(2, 3, 4, 5), pass_rate=0.5, max_nodes=7, tree_frac=0.8),
    "w82": dict(ow=82, oh=82, seed=11, stage_sizes=(2, 3, 3, 4), pass_rate=0.6),
}
IMAGES = {"t20": (203, 151, 1.1), "t24": (199, 149, 1.1), "deep4": (160, 120, 1.2), "w82": (260, 200, 1.3)}      # odd pitches, partial tiles on both edges
WIDE = ("t20", 1100, 60, 1.2)            # its first level is wider than 1023: a resize, an integral and a tilted launch per level
BATCH = ("t20", 96, 72, 1.2)             # the images of the 2- and 33-image batches
LEVELS = ("t24", 160, 120, 1.2)          # nvca_detect_raw_levels: six stages, the last three by k_hgen_levels
STREAM = ("t24", 160, 120, 160, 25, (11, 12, 13))      # (cascade, frame width, height, width_to_process, scale_factor_pct, seeds)
PART_W, PART_H = 320, 240


@functools.lru_cache(maxsize=None)
def _dict(name):
    kw = dict(CASCADES[name])
    if kw["ow"] > 64:          # calibration images the large window fits into
        kw["calibrate_on"] = [synth.make_gray(3 * kw["ow"], 3 * kw["oh"], synth.frame_seed(7, 9100 + i), "natural") for i in range(2)]
    return synth.make_haar_tree_cascade(**kw)


@functools.lru_cache(maxsize=None)
def cascade(name, style="traincascade"):
    """(xml text, the reference reader's cascade)"""
    xml = synth.haar_tree_cascade_to_xml(_dict(name), style)
    return xml, R.parse_xml(xml)


def image(cols, rows, ow, oh, seed=11):
    return HK.image(cols, rows, ow, oh, seed)


@functools.lru_cache(maxsize=None)
def expected_raw(name, cols, rows, sf, seed=11):
    c = cascade(name)[1]
    return R.scan(c, image(cols, rows, *c.size, seed), sf)


@functools.lru_cache(maxsize=None)
def stump_xml(style="traincascade"):
    """a file of stumps "0 -1" on upright features: haar_new_cases' w24, which the flag must not change"""
    return HK.cascade("w24", style)[0]


# ------------------------------------------------------------------ constructed cascades
def hand(size, features, stages, tilted=None):
    """features: [[(x, y, w, h, weight)]]; tilted: [0 | 1] per feature; stages: [(file threshold, [([(left, right, feature, thr)], [leaves])])]"""
    return dict(name="hand", size=size, features=[list(f) for f in features], tilted=list(tilted or [0] * len(features)),
                stages=[dict(threshold=t, weak=[dict(nodes=list(n), leaves=list(l)) for (n, l) in w]) for (t, w) in stages])


def window_image(ow, oh, pixels, fill=0):
    return HK.window_image(ow, oh, pixels, fill)


def ONE(ow, oh):
    return [[0, 0, ow, oh]]


def PIX(x, y, wt=1.0):
    return [(x, y, 1, 1, wt)]


# A 4 x 4 window whose normrect (1, 1, 2, 2) holds 0, 0, 2, 2: valsum = 4, valsq = 8, nf = 4 * 8 - 16 = 16 -> 4, vnf = 0.25 exactly
# (haar_new_cases' "w4-nf-16").  The 5 x 5 image is ONE window at sf 2; the pixels outside the normrect are free.
def _g4(extra):
    px = {(1, 1): 0, (2, 1): 0, (1, 2): 2, (2, 2): 2}
    px.update(extra)
    return window_image(4, 4, px, fill=0)


def tilted_cases():
    """(id, cascade dict, image, hand-derived raw list at sf 2).  A tilted rect (x, y, w, h) covers, in pixels, the rows y .. y + w + h - 1
    of a diamond-edged strip: T(X, Y) sums the pixels (x', y') with y' < Y, |x' - X + 1| <= Y - y' - 1, so
      w = h = 1 at (x, y) = (2, 0): T(2,0) - T(1,1) - T(3,1) + T(2,2) = 0 - p(0,0) - p(2,0) + [p(1,1) + p(0,0) + p(1,0) + p(2,0)]
                                      = p(1,0) + p(1,1)                                   -- two pixels, one above the other
      w = 2, h = 1 at (2, 0):       T(2,0) - T(1,1) - T(4,2) + T(3,3)
                                      = - p(0,0) - [p(3,1) + p(2,0) + p(3,0) + p(4,0)] + [p(2,2) + p(1,1) + p(2,1) + p(3,1) + p(0,0) .. p(4,0)]
                                      = p(1,0) + p(1,1) + p(2,1) + p(2,2)                 -- the w = h = 1 pair, and the same pair one step down-right
    With vnf = 0.25 the value is a quarter of that sum, times the file's weight."""
    out = []
    g = _g4({(1, 0): 10, (0, 0): 100, (2, 0): 100, (0, 1): 100, (3, 1): 100})          # p(1,0) + p(1,1) = 10 + 0: value 2.5; the neighbours would add hundreds
    f = [[(2, 0, 1, 1, 1.0)]]
    for thr, leaves, exp, tag in ((2.75, (1.0, -1.0), ONE(4, 4), "below"), (2.5, (1.0, -1.0), [], "tie-goes-right"), (2.25, (1.0, -1.0), [], "above")):
        out.append(("tilted-1x1-" + tag, hand((4, 4), f, [(0.5, [([(0, -1, 0, thr)], leaves)])], [1]), g, exp))
    # w = 2, h = 1: p(1,0) + p(1,1) + p(2,1) + p(2,2) = 10 + 0 + 0 + 2 = 12: value 3
    f = [[(2, 0, 2, 1, 1.0)]]
    for thr, exp, tag in ((3.25, ONE(4, 4), "below"), (3.0, [], "tie-goes-right")):
        out.append(("tilted-2x1-" + tag, hand((4, 4), f, [(0.5, [([(0, -1, 0, thr)], (1.0, -1.0))])], [1]), g, exp))
    # the weight as written: 2.0 on the 1 x 1 rect gives 2 * 10 * 0.25 = 5, not the 2.5 a halved weight would give
    f = [[(2, 0, 1, 1, 2.0)]]
    out.append(("tilted-weight-as-written", hand((4, 4), f, [(0.5, [([(0, -1, 0, 4.0)], (-1.0, 1.0))])], [1]), g, ONE(4, 4)))      # 5 >= 4: right = 1
    out.append(("tilted-weight-not-halved", hand((4, 4), f, [(0.5, [([(0, -1, 0, 4.0)], (1.0, -1.0))])], [1]), g, []))            # (2.5 < 4 would pass)
    # the same rect numbers upright and tilted are different features: upright (2, 0, 1, 1) is the pixel (2, 0) = 100: value 25
    both = [[(2, 0, 1, 1, 1.0)], [(2, 0, 1, 1, 1.0)]]
    out.append(("tilted-flag-belongs-to-the-feature", hand((4, 4), both, [(1.5, [([(0, -1, 0, 10.0)], (-1.0, 1.0)), ([(0, -1, 1, 10.0)], (1.0, -1.0))])], [0, 1]), g, ONE(4, 4)))
    return out


# The three-node tree   node 0: A < 5 ? node 1 : node 2;   node 1: B < 5 ? leaf 0 : leaf 1;   node 2: B < 5 ? leaf 2 : leaf 3
# on A = pixel (0, 0) and B = pixel (3, 0) of the 4 x 4 window above (value = pixel / 4).  Leaf k votes 2^k; the stage threshold picks one.
_A, _B = PIX(0, 0), PIX(3, 0)
_TREE3 = [(1, 2, 0, 5.0), (0, -1, 1, 5.0), (-2, -3, 1, 5.0)]
_LEAVES3 = (1.0, 2.0, 4.0, 8.0)


def _only(leaf_value, nodes=_TREE3, leaves=_LEAVES3):
    """two stages that pass exactly the windows whose tree ends in `leaf_value`: sum >= v, then -sum >= -v"""
    neg = tuple(-v for v in leaves)
    return hand((4, 4), [_A, _B], [(leaf_value - 0.25, [(nodes, leaves)]), (-leaf_value - 0.25, [(nodes, neg)])])


def tree_cases():
    """(id, cascade dict, image, hand-derived raw list at sf 2)"""
    out = []
    # (A, B) pixels -> values (A / 4, B / 4): 0 -> 0 (< 5), 40 -> 10 (>= 5)
    for a, b, leaf in ((0, 0, 1.0), (0, 40, 2.0), (40, 0, 4.0), (40, 40, 8.0)):
        g = _g4({(0, 0): a, (3, 0): b})
        for want in _LEAVES3:
            out.append(("tree3-A%d-B%d-leaf%g-asks-%g" % (a, b, leaf, want), _only(want), g, ONE(4, 4) if want == leaf else []))
    # a tie at the inner node 1: B = 20 -> value 5 == thr: right, leaf 1 (2.0); at the root: A = 20 -> node 2
    g = _g4({(0, 0): 0, (3, 0): 20})
    out += [("tie-at-inner-node-goes-right", _only(2.0), g, ONE(4, 4)), ("tie-at-inner-node-not-left", _only(1.0), g, [])]
    g = _g4({(0, 0): 20, (3, 0): 0})
    out += [("tie-at-root-goes-right", _only(4.0), g, ONE(4, 4)), ("tie-at-root-not-left", _only(1.0), g, [])]
    # both child layouts of a two-node tree: "0 1" (left: leaf 0, right: node 1) and "1 0" (left: node 1, right: leaf 0)
    lay01, lay10 = [(0, 1, 0, 5.0), (-1, -2, 1, 5.0)], [(1, 0, 0, 5.0), (-1, -2, 1, 5.0)]
    lv = (1.0, 2.0, 4.0)
    for a, b, l01, l10 in ((0, 0, 1.0, 2.0), (0, 40, 1.0, 4.0), (40, 0, 2.0, 1.0), (40, 40, 4.0, 1.0)):
        g = _g4({(0, 0): a, (3, 0): b})
        out.append(("layout-0-1-A%d-B%d" % (a, b), _only(l01, lay01, lv), g, ONE(4, 4)))
        out.append(("layout-1-0-A%d-B%d" % (a, b), _only(l10, lay10, lv), g, ONE(4, 4)))
    # an unreachable node: node 1 is nobody's child (node 0 goes to node 2 or leaf 0); its leaves 1, 2 are never taken
    dead = [(0, 2, 0, 5.0), (-1, -2, 1, 5.0), (-3, -3, 1, 5.0)]
    dl = (1.0, 2.0, 4.0, 8.0)
    out.append(("unreachable-node-left", _only(1.0, dead, dl), _g4({(0, 0): 0, (3, 0): 0}), ONE(4, 4)))
    out.append(("unreachable-node-right", _only(8.0, dead, dl), _g4({(0, 0): 40, (3, 0): 40}), ONE(4, 4)))
    # a one-node tree whose leaves are swapped in the file, "-1 0": left is leaf 1, right leaf 0
    sw = [(-1, 0, 0, 5.0)]
    out.append(("stump-with-swapped-leaves-left", _only(2.0, sw, (1.0, 2.0)), _g4({(0, 0): 0}), ONE(4, 4)))
    out.append(("stump-with-swapped-leaves-right", _only(1.0, sw, (1.0, 2.0)), _g4({(0, 0): 40}), ONE(4, 4)))
    return out


# ---- a tree in stage 0 and the skip rule, on lbp_cases.column_image() (16 x 8; column c holds 10 when c % 4 is 1 or 2, else 0) at sf 4:
# 3 x 3 windows at x = 0, 2 .. 12, y = 0, 2, 4; vnf = 1 (haar_new_cases.skip_cases).
#   C = the centre pixel, column x + 1: 10 at x = 0, 4, 8, 12; 0 at x = 2, 6, 10
#   E = the pixel left of it, column x:  0 at x = 0, 4, 8, 12; 10 at x = 2, 6, 10
# The walk: a window rejected by stage 0 (result 0) skips the next grid column; any other result does not.
def skip_cases():
    """(id, cascade dict, hand-written raw list) -- haar_new_cases.skip_cases' lists, reached through a two-node tree "1 0": C >= 5 takes
    leaf 0; C < 5 goes to node 1, which reads E (10 wherever C is 0) and so takes leaf 2"""
    rows = (0, 2, 4)
    C_, E_ = [(1, 1, 1, 1, 1.0)], [(0, 1, 1, 1, 1.0)]
    shape = [(1, 0, 0, 5.0), (-1, -2, 1, 5.0)]
    rej_odd = (shape, (1.0, 1.0, -1.0))            # x = 0, 4, 8, 12 pass by leaf 0; x = 2, 6, 10 are rejected through node 1
    rej_even = (shape, (-1.0, -1.0, 1.0))          # x = 0, 4, 8, 12 rejected at the root's leaf; x = 2, 6, 10 pass through node 1
    all_pass = ([(0, -1, 0, 5.0)], (1.0, 1.0))
    return [
        # x = 0 rejected -> 2 skipped, 4 rejected -> 6 skipped, 8 -> 10 skipped, 12 rejected
        ("tree-in-stage0-rejects-even", hand((3, 3), [C_, E_], [(0.0, [rej_even])]), []),
        # x = 0 passes; 2 rejected -> 4 skipped; 6 rejected -> 8 skipped; 10 rejected -> 12 skipped
        ("tree-in-stage0-rejects-odd", hand((3, 3), [C_, E_], [(0.0, [rej_odd])]), [[0, y, 3, 3] for y in rows]),
        # rejected by stage 1 (result -1): nothing is skipped, every column is visited
        ("tree-in-stage1-rejects-even", hand((3, 3), [C_, E_], [(0.0, [all_pass]), (0.0, [rej_even])]), [[x, y, 3, 3] for y in rows for x in (2, 6, 10)]),
    ]


# ------------------------------------------------------------------ files the loader must refuse (with the flag), by rewriting one weak classifier
def refusal_cases():
    """(id, xml, status name) -- every check that is stricter than OpenCV's, and the node bound"""
    base = hand((4, 4), [_A, _B], [(0.5, [(_TREE3, _LEAVES3)])])

    def with_tree(nodes, leaves, tilted=None, features=None):
        return synth.haar_tree_cascade_to_xml(hand((4, 4), features or [_A, _B], [(0.5, [(nodes, leaves)])], tilted))
    good = synth.haar_tree_cascade_to_xml(base)
    out = [
        ("node-words-not-a-multiple-of-4", good.replace("1 2 0 5 0 -1 1 5 -2 -3 1 5", "1 2 0 5 0 -1 1 5 -2 -3 1"), "PARSE"),
        ("leaf-count-not-nodes-plus-1", good.replace("1 2 4 8</leafValues>", "1 2 4</leafValues>"), "PARSE"),
        ("child-not-behind-its-parent", with_tree([(1, 2, 0, 5.0), (1, -1, 1, 5.0), (-2, -3, 1, 5.0)], _LEAVES3), "PARSE"),
        ("child-points-back", with_tree([(1, 2, 0, 5.0), (0, -1, 1, 5.0), (1, -3, 1, 5.0)], _LEAVES3), "PARSE"),
        ("child-outside-the-tree", with_tree([(1, 3, 0, 5.0), (0, -1, 1, 5.0), (-2, -3, 1, 5.0)], _LEAVES3), "PARSE"),
        ("leaf-index-outside", with_tree([(1, 2, 0, 5.0), (0, -1, 1, 5.0), (-2, -4, 1, 5.0)], _LEAVES3), "PARSE"),
        ("threshold-not-finite", good.replace("1 2 0 5 0", "1 2 0 nan 0"), "PARSE"),
        ("leaf-not-finite", good.replace("1 2 4 8</leafValues>", "1 2 inf 8</leafValues>"), "PARSE"),
        ("feature-index-outside", with_tree([(1, 2, 2, 5.0), (0, -1, 1, 5.0), (-2, -3, 1, 5.0)], _LEAVES3), "PARSE"),
        ("fractional-child", good.replace("1 2 0 5 0", "1.5 2 0 5 0"), "PARSE"),
        # tilted rects (x, y, w, h) in the 4 x 4 window: x - h < 0; x + w > ow; y + w + h > oh
        ("tilted-x-minus-h-negative", with_tree([(0, -1, 0, 5.0)], (1.0, 2.0), [1], [[(0, 0, 1, 1, 1.0)]]), "PARSE"),
        ("tilted-x-plus-w-beyond", with_tree([(0, -1, 0, 5.0)], (1.0, 2.0), [1], [[(3, 0, 2, 1, 1.0)]]), "PARSE"),
        ("tilted-y-plus-w-plus-h-beyond", with_tree([(0, -1, 0, 5.0)], (1.0, 2.0), [1], [[(2, 1, 2, 2, 1.0)]]), "PARSE"),
    ]
    # 16 nodes in one weak classifier: a chain 0 -> 1 -> ... -> 15
    chain = [(-k, k + 1, 0, 5.0) for k in range(15)] + [(-15, -16, 0, 5.0)]
    out.append(("sixteen-nodes", with_tree(chain, tuple(float(k) for k in range(17))), "UNSUPPORTED"))
    return out


def fifteen_node_chain():
    """the bound itself: 15 nodes load"""
    chain = [(-k, k + 1, 0, 5.0) for k in range(14)] + [(-14, -15, 0, 5.0)]
    return synth.haar_tree_cascade_to_xml(hand((4, 4), [_A, _B], [(0.5, [(chain, tuple(float(k) for k in range(16)))])]))


def pinned_refusals():
    """the three files tests/test_haar_new_cpu.py::test_refusals pins as UNSUPPORTED through the plain entry points"""
    stump = synth.haar_new_cascade_to_xml(HK.one_stump((4, 4), HK.PIX00, 2.5))
    return [
        ("tilted", stump.replace("<tilted>0</tilted>", "<tilted>1</tilted>").replace("0 0 1 1 1.", "2 0 1 1 1.")),
        ("maxDepth-2", stump.replace("<maxDepth>1</maxDepth>", "<maxDepth>2</maxDepth>")),
        ("two-internal-nodes", synth.haar_tree_cascade_to_xml(hand((4, 4), [_A, _B], [(0.5, [([(0, 1, 0, 5.0), (-1, -2, 1, 5.0)], (1.0, 2.0, 4.0))])])).replace("<maxDepth>2</maxDepth>", "<maxDepth>1</maxDepth>")),
    ]


# ------------------------------------------------------------------ streams (the way tests/haar_new_stream_cases.py puts its cases together)
def stream_frames():
    name, W, H, _wtp, _pct, seeds = STREAM
    return [("tree", name, W, H, s) for s in seeds]


@functools.lru_cache(maxsize=None)
def stream_gray(frame):
    _, name, W, H, seed = frame
    g = np.array(image(W, H, *cascade(name)[1].size, seed), np.uint8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def stream_yuv(frame, fmt):
    """(buffer, layout tuple) of the 4:2:0 frame whose luma plane is stream_gray(frame) and whose chroma is neutral"""
    import yuv_stream_scenes as S
    g = stream_gray(frame)
    c = np.full((g.shape[0] // 2, g.shape[1] // 2), 128, np.uint8)
    return S.pack_planes(g, c, c, fmt)


@functools.lru_cache(maxsize=None)
def stream_bgr(frame, fmt=0):
    import yuv_reference as Y
    g = stream_gray(frame)
    if fmt:
        buf, lay = stream_yuv(frame, fmt)
        out = Y.bgr(buf, g.shape[1], g.shape[0], lay)
    else:
        out = np.ascontiguousarray(np.dstack([g] * 3))
    out.setflags(write=False)
    return out


class Expected:
    """the expected face stream: the oracle's gate and finish around the statement's detections on the equalised working image"""

    def __init__(self, name, fmt=0, wtp=160, pct=25, mn=3):
        import lbp_stream_cases as LS
        import orc
        self.name, self.fmt, self.wtp, self.pct, self.mn = name, fmt, wtp, pct, mn
        self.s = orc.FaceStream(LS._any_haar(), width_to_process=wtp)

    def process(self, frame, cap=1024):
        import ctypes as C
        import lbp_stream_cases as LS
        import orc
        img = stream_bgr(frame, self.fmt)
        H, W = img.shape[:2]
        L = orc.lib()
        analysed = L.orc_face_stream_gate(self.s.h)
        det = np.zeros((0, 4), np.int32)
        if analysed:
            cols, rows, _ = LS.geometry(W, H, self.wtp)
            w = orc.equalize_hist(orc.bgr2gray(orc.resize_linear(np.array(img), cols, rows)))
            det = R.detect(cascade(self.name)[1], w, 1 + self.pct / 100, self.mn, (cols // 20, rows // 20))
        assert len(det) <= LS.ORC_MAX_FACES
        buf, ids = (orc.Rect * cap)(), (C.c_int * cap)()
        n = L.orc_face_stream_finish(self.s.h, analysed, orc.np_to_rects(det), len(det), W, H, buf, ids, cap)
        return orc.rects_to_np(buf, n), np.array(ids[:n], dtype=np.int32)


# an ear stream whose roles are of three formats: the LBP face cascade, an old-format ear cascade, and the general cascade "t20" in the
# second part role, on regions larger than its window


def part_xmls():
    import lbp_part_cases as LP
    return [LP.K.cascade(LP.FACE)[0], LP.haar_xml()["leftear"], cascade("t20")[0]]


@functools.lru_cache(maxsize=None)
def part_expected():
    """([(list a, list b)] per frame, the three detectors with the sizes they saw)"""
    import lbp_part_cases as LP
    ref = cascade("t20")[1]
    dets = (LP.lbp_detector(LP.K.cascade(LP.FACE)[1]), LP.haar_detector(LP._haar_cpu()["leftear"]),
            LP.Detector(lambda g, sf, mn, flags, mins, maxs: R.detect(ref, g, sf, mn, mins, maxs)))
    h = LP.Harness("ear", *dets)
    out = [h.process(f) for f in LP.lbp_frames(PART_W, PART_H)]
    h.close()
    return out, dets


def permissive_general(ow, oh):
    """one stage that passes every window, through a two-node tree on a tilted and an upright feature: leaves all 1"""
    return hand((ow, oh), [[(2, 0, 1, 1, 1.0)], [(0, 0, 1, 1, 1.0)]], [(-1.0, [([(0, 1, 0, 0.0), (-1, -2, 1, 0.0)], (1.0, 1.0, 1.0))])], [1, 0])
