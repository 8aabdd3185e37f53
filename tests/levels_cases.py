"""Cases that tests/test_levels_cpu.py (on the numpy statement, tests/levels_reference.py) and tests/test_gpu_levels.py (on the device)
share: detectMultiScale with outputRejectLevels, SURVEY.md A.17.  Every expected list of a constructed case is written down here by hand;
a natural case's comes from the statement, once (lru_cache), never from a run of the library."""
import functools

import numpy as np

import haar_new_cases as HK
import lbp_cases as LK
import levels_reference as V
from nubovca import synth

LBP, HAAR = "lbp", "haar"


def to_xml(kind, cdict):
    return synth.lbp_cascade_to_xml(cdict) if kind == LBP else synth.haar_new_cascade_to_xml(cdict)


def parse(kind, xml):
    return (V.L if kind == LBP else V.H).parse_xml(xml)


# ------------------------------------------------------------------ constant votes on ONE 3 x 3 window (a 4 x 4 image at sf 2)
def const_cascade(kind, stages):
    """stages: [(file threshold, [constant votes])] -- every weak classifier answers its vote whatever the window holds"""
    if kind == LBP:
        return LK.hand_cascade((3, 3), [(0, 0, 1, 1)], [(t, [(0, [0] * 8, (v, v)) for v in votes]) for (t, votes) in stages])
    return HK.hand_cascade((3, 3), [HK.PIX00], [(t, [(0, 0.0, (v, v)) for v in votes]) for (t, votes) in stages])


def one_window_image(kind):
    return LK.cell_image({}) if kind == LBP else HK.window_image(3, 3, {(0, 0): 7, (1, 1): 200}, fill=9)


ONE = [[0, 0, 3, 3]]


def hand_cases():
    """(id, kind, cascade dict, image, sf, rects, reject levels, level weights), derived by hand.  Stage k of a constant cascade votes
    k + 1.25 against the file threshold 0.5 and passes; a rejecting stage votes -(k + 1.25): its sum is below the threshold, the window
    ends there with that sum.  Every value is exact in f32."""
    out = []
    for kind in (LBP, HAAR):
        g = one_window_image(kind)
        for n in (4, 5):
            votes = [k + 1.25 for k in range(n)]
            for rej in (n - 3, n - 1):          # rejected by the first / by the last of the three emitted stages: level = that stage, weight = its sum
                st = [(0.5, [-(votes[k]) if k == rej else votes[k]]) for k in range(n)]
                out.append(("%s-const%d-rejected-at-%d" % (kind, n, rej), kind, const_cascade(kind, st), g, 2.0, ONE, [rej], [-votes[rej]]))
            # passes every stage: level n, weight = the LAST stage's sum
            out.append(("%s-const%d-passes" % (kind, n), kind, const_cascade(kind, [(0.5, [v]) for v in votes]), g, 2.0, ONE, [n], [votes[n - 1]]))
            # rejected in front of the last three stages (stage n - 4, which is stage 0 for n = 4): not emitted
            st = [(0.5, [-(votes[k]) if k == n - 4 else votes[k]]) for k in range(n)]
            out.append(("%s-const%d-rejected-early" % (kind, n), kind, const_cascade(kind, st), g, 2.0, [], [], []))
        # the last stage of four sums 1e8 + 1 - 1e8 against 0.5.  LBP: f32, the 1 is lost: 0.0 < 0.5, rejected at stage 3 with weight 0.0.
        # HAAR: f64, 1.0 >= 0.5: passes, level 4 with weight 1.0.
        st = [(0.5, [1.25]), (0.5, [2.25]), (0.5, [3.25]), (0.5, [1e8, 1.0, -1e8])]
        out.append(("%s-sum-precision" % kind, kind, const_cascade(kind, st), g, 2.0, ONE) + (([3], [0.0]) if kind == LBP else ([4], [1.0])))
    # The skip rule on lbp_cases.column_image() at sf 4 (3 x 3 windows at x = 0, 2 .. 12, y = 0, 2, 4), four stages, the last three permissive
    # with constant votes 2.25, 3.25, 4.25.  Stage 0 rejects the even grid columns: column 0 is visited and rejected (result 0: not emitted, n + 0 = 4),
    # column 1 is skipped, 2 rejected, 3 skipped ...: nothing is emitted although every odd column would pass all four stages.
    # Stage 0 rejects the odd grid columns: 0 passes (level 4, weight 4.25), 1 is rejected, 2 skipped, 3 rejected, 4 skipped, 5 rejected, 6 skipped:
    # column 0 alone -- without the skip, columns 2, 4 and 6 would be emitted too.
    rows = (0, 2, 4)
    tail_l = [(0.0, [(0, LK.ALL_CODES, (v, v))]) for v in (2.25, 3.25, 4.25)]
    tail_h = [(0.0, [(0, 5.0, (v, v))]) for v in (2.25, 3.25, 4.25)]
    leaf = (1.0, -1.0)
    for kind, even, odd in ((LBP, LK.hand_cascade((3, 3), [(0, 0, 1, 1)], [(0.0, [(0, LK.ODD_CODES, leaf)])] + tail_l),
                             LK.hand_cascade((3, 3), [(0, 0, 1, 1)], [(0.0, [(0, LK.EVEN_CODES, leaf)])] + tail_l)),
                            (HAAR, HK.hand_cascade((3, 3), [HK.CENTRE], [(0.0, [(0, 5.0, (1.0, -1.0))])] + tail_h),
                             HK.hand_cascade((3, 3), [HK.CENTRE], [(0.0, [(0, 5.0, (-1.0, 1.0))])] + tail_h))):
        out.append(("%s-stage0-rejects-even-skips" % kind, kind, even, LK.column_image(), 4.0, [], [], []))
        out.append(("%s-stage0-rejects-odd-skips" % kind, kind, odd, LK.column_image(), 4.0, [[0, y, 3, 3] for y in rows], [4] * 3, [4.25] * 3))
    return out


# ------------------------------------------------------------------ natural cases: calibrated cascades on images with pasted templates
def truncated(kind, name, n):
    """the first n stages of a calibrated cascade (its features stay: a feature no stage uses is never read)"""
    d = LK._dict(name) if kind == LBP else HK._dict(name)
    return dict(d, stages=d["stages"][:n])


# id -> (kind, cascade dict maker, (cols, rows, sf), image seed).  97 x 83: partial tiles on both edges; w12 / w24 (5 / 8 LBP stages, 9 / 10 HAAR
# stages) and "deep" (20) run several stage groups; 4, 5 and 6 stages make tile_stages 1, 2 and 3 with zero or one stage group.  The image
# seeds are those for which tests/test_levels_cpu.py's premises hold on the statement.
# The LBP "deep" cascade's last stage rejects no window of any image (its calibration sample is used up in front of it: stage 19 passes
# whatever reaches it), so "lbp-deep" has windows at three of the four levels only (THREE_LEVELS); its first 19 stages have all four.
NATURAL = {}
for _kind, _K in ((LBP, LK), (HAAR, HK)):
    for _name in ("w12", "w24"):
        NATURAL["%s-%s" % (_kind, _name)] = (_kind, functools.partial(_K._dict, _name), (97, 83, 1.1), 11)
    NATURAL["%s-deep" % _kind] = (_kind, functools.partial(_K._dict, "deep"), (160, 120, 1.2), 12)
    for _n in (4, 5, 6):
        NATURAL["%s-w24-first%d" % (_kind, _n)] = (_kind, functools.partial(truncated, _kind, "w24", _n), (97, 83, 1.1), 11)
NATURAL["lbp-deep-first19"] = (LBP, functools.partial(truncated, LBP, "deep", 19), (160, 120, 1.2), 12)
NATURAL["haar-w24-first4"] = NATURAL["haar-w24-first4"][:3] + (15,)
THREE_LEVELS = {"lbp-deep": (17, 18, 20)}
PADDED = ("lbp-w24", "haar-w24")          # also run as a sub-matrix of a wider buffer


@functools.lru_cache(maxsize=None)
def natural(cid):
    """(xml, reference cascade, image, sf)"""
    kind, make, (cols, rows, sf), seed = NATURAL[cid]
    xml = to_xml(kind, make())
    ref = parse(kind, xml)
    img = (LK.image if kind == LBP else HK.image)(cols, rows, *ref.size, seed)
    return xml, ref, img, sf


# the two high-byte-plane routes of the squared integral (haar_new_cases.HI_PLANES) with an 81-pixel window, as tests/test_gpu_haar_new.py
# runs them.  Its cascade there ("w81", four stages) would emit nearly every visited window here -- 66 890 of the larger image --; eight stages
# built the same way (haar_new_cases._dict's calibration images) leave 27 165 and 16 162.
HI = sorted(HK.HI_PLANES)
HI_STAGES = (2, 3, 3, 4, 4, 4, 5, 5)


@functools.lru_cache(maxsize=None)
def hi_planes(route):
    cols, rows, sf = HK.HI_PLANES[route]
    cal = [synth.make_gray(243, 243, synth.frame_seed(7, 9100 + i), "natural") for i in range(2)]
    xml = synth.haar_new_cascade_to_xml(synth.make_haar_new_cascade(ow=81, oh=81, seed=10, stage_sizes=HI_STAGES, pass_rate=0.6, calibrate_on=cal))
    return xml, V.H.parse_xml(xml), HK.hi_planes_image(cols, rows), sf


# the overflow re-run: three permissive stages, then one that rejects about half of the windows -- every visited window is emitted, with
# level 3 or 4: far more than a candidate list of 256
def overflow_cascade(kind):
    if kind == LBP:
        perm = (-1.0, [(0, [0] * 8, (1.0, 1.0))])
        return LK.hand_cascade((24, 24), [(0, 0, 1, 1), (3, 3, 6, 6)], [perm] * 3 + [(0.0, [(1, LK.ODD_CODES, (1.0, -1.0))])])
    perm = (-1.0, [(0, 0.0, (1.0, 1.0))])
    # a left-against-right half difference: its sign splits the windows
    return HK.hand_cascade((24, 24), [HK.PIX00, [(2, 2, 20, 20, -1.0), (2, 2, 10, 20, 2.0)]], [perm] * 3 + [(0.0, [(1, 0.0, (1.0, -1.0))])])


OVERFLOW_IMAGE = (160, 120, 1.2)


@functools.lru_cache(maxsize=None)
def overflow(kind):
    cols, rows, sf = OVERFLOW_IMAGE
    xml = to_xml(kind, overflow_cascade(kind))
    return xml, parse(kind, xml), (LK.image if kind == LBP else HK.image)(cols, rows, 24, 24), sf


@functools.lru_cache(maxsize=None)
def expected(group, cid):
    """the statement's raw triples of a natural / hi-planes / overflow case"""
    xml, ref, img, sf = {"natural": natural, "hi": hi_planes, "overflow": overflow}[group](cid)
    return V.scan_levels(ref, img, sf)


def group_thresholds(ref):
    """minNeighbors values a case is grouped with: 0 (raw), 3, and nstages - 1, where the level rule drops every class without a passing window"""
    return (0, 3, len(ref.stage_sizes) - 1)


# ------------------------------------------------------------------ grouping on lists built by hand
def B(x, y, s=40):
    return [x, y, s, s]


def group_cases():
    """(id, rects, levels, weights, minNeighbors, expected rects, levels, weights), derived by hand.  40 x 40 boxes: delta = 0.2 * 40 = 8,
    boxes 0 .. 2 pixels apart are one class; the average of x = 100, 101, 102, 100, 101 is 100.8 -> 101."""
    out = []
    five = [B(100, 100), B(101, 100), B(102, 100), B(100, 100), B(101, 100)]
    # five members, every level 3: maxLevel 3 <= 3: dropped although the plain form (count 5 > 3) would keep it
    out.append(("many-members-low-level-dropped", five, [3] * 5, [1.0, 2.0, 3.0, 4.0, 5.0], 3, [], [], []))
    # one member reaches level 4: kept, with that member's weight (not the largest weight of the class)
    out.append(("one-member-carries-the-class", five, [3, 3, 4, 3, 3], [9.0, 8.0, -2.5, 7.0, 6.0], 3, [B(101, 100)], [4], [-2.5]))
    # a single box of level 9: a class of ONE member is kept (the plain form would drop it)
    out.append(("single-member-high-level-kept", [B(10, 10)], [9], [0.5], 3, [B(10, 10)], [9], [0.5]))
    # an equal-level tie takes the larger weight, whichever comes first; a lower level never replaces
    out.append(("tie-larger-weight-later", five, [4, 5, 5, 4, 5], [99.0, 1.5, 2.5, 98.0, 2.0], 3, [B(101, 100)], [5], [2.5]))
    out.append(("tie-larger-weight-first", five, [5, 5, 4, 5, 4], [2.5, 1.5, 99.0, 2.0, 98.0], 3, [B(101, 100)], [5], [2.5]))
    # negative weights: the first member of a greater level replaces DBL_MIN even with a negative weight; the tie then takes -1 over -3
    out.append(("tie-negative-weights", five[:3], [5, 5, 5], [-3.0, -1.0, -2.0], 3, [B(101, 100)], [5], [-1.0]))
    # The contained-box filter reads the OTHER class's member count.  A small class (2 members, level 7) inside a big one (5 members, level 5),
    # minNeighbors 1: for the small class n1 = 7, the big one's n2 = 5 > max(3, 7) fails and n1 < 3 fails: kept -- by its count (2 < 3) the plain
    # form would drop it.  With the small class at level 4: n2 = 5 > max(3, 4): dropped.  Big: x 100 .. 102 -> 101, 100 x 100; small 20 x 20 at
    # (140, 140), (141, 140) -> cvRound(140.5) = 140 (half to even).
    big = [[100, 100, 100, 100], [101, 100, 100, 100], [102, 100, 100, 100], [100, 100, 100, 100], [101, 100, 100, 100]]
    small = [[140, 140, 20, 20], [141, 140, 20, 20]]
    out.append(("contained-kept-by-its-level", big + small, [5] * 5 + [7, 7], [1.0] * 5 + [2.0, 3.0], 1,
                [[101, 100, 100, 100], [140, 140, 20, 20]], [5, 7], [1.0, 3.0]))
    out.append(("contained-dropped-by-the-others-count", big + small, [5] * 5 + [4, 4], [1.0] * 5 + [2.0, 3.0], 1,
                [[101, 100, 100, 100]], [5], [1.0]))
    # ... and a big class of TWO members (count 2 <= minNeighbors 2) is no partner in the filter, though its level (9) is high: the small
    # class (level 2 would be dropped by its own level; level 3 > 2 is kept) survives inside it
    out.append(("partner-skipped-by-its-count", big[:2] + small, [9, 9, 3, 3], [1.0, 2.0, 3.0, 4.0], 2,
                [[100, 100, 100, 100], [140, 140, 20, 20]], [9, 3], [2.0, 4.0]))
    # minNeighbors 0 and below: the raw triples, untouched
    out.append(("min-neighbors-0-raw", five, [3, 4, 5, 6, 7], [1.0, 2.0, 3.0, 4.0, 5.0], 0, five, [3, 4, 5, 6, 7], [1.0, 2.0, 3.0, 4.0, 5.0]))
    out.append(("min-neighbors-negative-raw", five[:2], [3, 4], [1.0, 2.0], -1, five[:2], [3, 4], [1.0, 2.0]))
    out.append(("empty", [], [], [], 3, [], [], []))
    return out


def random_group_lists(seed, n):
    """a seeded list of n triples around a few centres (clusters, strays, ties in level and weight)"""
    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
    c = rng.integers(0, 6, n)
    s = np.array([24, 24, 40, 40, 80, 26])[c]
    x = np.array([30, 34, 120, 122, 100, 300])[c] + rng.integers(-3, 4, n)
    y = np.array([30, 31, 60, 64, 50, 200])[c] + rng.integers(-3, 4, n)
    rects = np.stack([x, y, s, s], 1).astype(np.int32)
    levels = rng.integers(1, 7, n).astype(np.int32)
    weights = np.round(rng.normal(0, 2, n), 1)          # one decimal: equal weights happen
    return rects, levels, weights
