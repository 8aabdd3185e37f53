"""Cascades, images and constructed cases that tests/test_haar_new_cpu.py (on the numpy statement, tests/haar_new_reference.py) and
tests/test_gpu_haar_new*.py (on the device) share.  Every expected list of a constructed case is written down here by hand, never
taken from a run; the arithmetic behind each is in its comment."""
import functools

import numpy as np

import haar_new_reference as R
import lbp_cases as LK
from nubovca import synth

# name -> make_haar_new_cascade arguments (seeds for which tests/test_haar_new_cpu.py's premises hold on the statement).  Nine stages or more: the tile kernel takes stages 0 .. 2, then stage groups [3, 5), [5, 8), [8, 12) ...
# so three later groups exist; "deep": 20 stages, the last group is [17, 20)
CASCADES = {
    "w24": dict(ow=24, oh=24, seed=12, stage_sizes=(3, 4, 5, 6, 7, 8, 9, 10, 10, 10), pass_rate=0.6),
    "w20x28": dict(ow=20, oh=28, seed=2, stage_sizes=(3, 4, 5, 6, 7, 7, 8, 8, 9), pass_rate=0.6),
    "w12": dict(ow=12, oh=12, seed=3, stage_sizes=(2, 3, 4, 5, 6, 6, 7, 7, 8), pass_rate=0.6),
    "deep": dict(ow=24, oh=24, seed=13, stage_sizes=(3, 4, 4, 5, 5, 6, 6, 6, 7, 7, 7, 8, 8, 8, 8, 9, 9, 9, 10, 10), pass_rate=0.7),
    # on both sides of the tables' LDS bound: (63 + w) (31 + w) words <= 16384 holds at 81 and fails at 82
    "w81": dict(ow=81, oh=81, seed=10, stage_sizes=(2, 3, 3, 4), pass_rate=0.6),
    "w82": dict(ow=82, oh=82, seed=12, stage_sizes=(2, 3, 3, 4), pass_rate=0.6),
}
IMAGES = [(97, 83, 1.1), (160, 120, 1.2), (333, 251, 1.1)]      # partial tiles on both edges, an odd pitch
WIDE = (1500, 240, 1.3)                                         # its first levels are wider than 1023
DEEP_IMAGE = (160, 120, 1.2)
LDS_IMAGE = (260, 200, 1.3)                                     # what the 81- and 82-pixel windows run on
# the squared integral's high-byte planes under both pyramid routes: bright images whose Q passes 2^32 inside levels behind the first, scanned
# with the 81-pixel window (the four corners of its normrect lie far apart: their high bytes differ for many windows).  "per-level": a first level
# wider than 1023, every level integrated by a launch of its own; "one-launch": all levels in one integral launch
HI_PLANES = {"per-level": (1100, 200, 1.3), "one-launch": (640, 400, 1.3)}
BRIGHT = (300, 290)                                             # one level at sf 1.5 for the 264-pixel window


@functools.lru_cache(maxsize=None)
def _dict(name):
    kw = dict(CASCADES[name])
    if kw["ow"] > 64:          # calibration images the large windows fit into
        kw["calibrate_on"] = [synth.make_gray(3 * kw["ow"], 3 * kw["oh"], synth.frame_seed(7, 9100 + i), "natural") for i in range(2)]
    return synth.make_haar_new_cascade(**kw)


@functools.lru_cache(maxsize=None)
def cascade(name, style="traincascade"):
    """(xml text, the reference reader's cascade)"""
    xml = synth.haar_new_cascade_to_xml(_dict(name), style)
    return xml, R.parse_xml(xml)


@functools.lru_cache(maxsize=None)
def image(cols, rows, ow, oh, seed=11):
    """lbp_cases.image (a natural field with the stretched template pasted at up to three scales) with a flat patch in the bottom right
    corner, large enough to hold windows of the first level: those take the nf <= 0 branch"""
    g = LK.image(cols, rows, ow, oh, seed).copy()
    pw, ph = min(cols // 2, ow + 12), min(rows // 2, oh + 12)
    g[rows - ph:, cols - pw:] = 77
    return g


@functools.lru_cache(maxsize=None)
def hi_planes_image(cols, rows):
    """image(cols, rows, 81, 81) at a quarter of its contrast on a floor of 192 (the evaluator's normalisation takes both out again)"""
    return (192 + image(cols, rows, 81, 81) // 4).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def bright_image():
    """300 x 290, every pixel 249 .. 255: a rect of more than 2^24 / 249 = 67 378 pixels (260 x 260, say) sums to more than 2^24 = 16 777 216"""
    rng = np.random.default_rng(77)
    return rng.integers(249, 256, size=(BRIGHT[1], BRIGHT[0])).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def bright_cascade():
    """(xml, reference cascade) of a 264 x 264 window for bright_image(): three stages of three stumps on large rects, every stump's threshold the
    median of its feature over the image's own grid and every stage passing two votes of three, so that about half of the windows go on per
    stage -- thresholds that sit inside the values' spread, where the rounding of a rect sum above 2^24 to f32 can decide a vote"""
    rng = np.random.default_rng(264)
    ow = oh = 264
    g = bright_image()
    S, Q = synth._integral_pair_np(g)
    xs, ys = np.arange(0, g.shape[1] - ow, 2), np.arange(0, g.shape[0] - oh, 2)
    features, stages = [], []
    for _ in range(3):
        weak = []
        while len(weak) < 3:
            rects = synth._rand_haar_new_feature(rng, ow, oh)
            if rects[0][2] * rects[0][3] * 249 <= (1 << 24):
                continue                                    # its largest rect sum would stay below 2^24
            thr = float(np.float32(np.median(synth._haar_new_values(S, Q, rects, ow, oh, xs, ys))))
            features.append(rects)
            weak.append(dict(feature=len(features) - 1, threshold=thr, leaves=(1.0, -1.0) if rng.integers(0, 2) else (-1.0, 1.0)))
        stages.append(dict(threshold=-0.5, weak=weak))
    xml = synth.haar_new_cascade_to_xml(dict(name="bright", size=(ow, oh), features=features, stages=stages))
    return xml, R.parse_xml(xml)


@functools.lru_cache(maxsize=None)
def expected_raw(name, cols, rows, sf, min_size=(0, 0), max_size=(0, 0)):
    c = cascade(name)[1]
    return R.scan(c, image(cols, rows, *c.size), sf, min_size, max_size)


# ------------------------------------------------------------------ constructed cascades
def hand_cascade(size, features, stages):
    """features: [[(x, y, w, h, weight)]]; stages: [(file threshold, [(feature, stump threshold, (leaf0, leaf1))])]"""
    return dict(name="hand", size=size, features=[list(f) for f in features],
                stages=[dict(threshold=t, weak=[dict(feature=f, threshold=th, leaves=l) for (f, th, l) in w]) for (t, w) in stages])


def permissive(ow, oh):
    """one stage that passes every window"""
    return hand_cascade((ow, oh), [[(0, 0, 1, 1, 1.0)]], [(-1.0, [(0, 0.0, (1.0, 1.0))])])


def one_stump(size, feature, thr, leaves=(1.0, -1.0), stage_thr=0.5):
    """value < thr passes (leaves (1, -1) against stage threshold 0.5)"""
    return hand_cascade(size, [feature], [(stage_thr, [(0, thr, leaves)])])


def window_image(ow, oh, pixels, fill=0):
    """an (oh + 1) x (ow + 1) image -- ONE ow x oh window at sf 2, at (0, 0) -- with `pixels` {(x, y): value}"""
    g = np.full((oh + 1, ow + 1), fill, np.uint8)
    for (x, y), v in pixels.items():
        g[y, x] = v
    return g


def ONE(ow, oh):
    return [[0, 0, ow, oh]]


PIX00 = [(0, 0, 1, 1, 1.0)]          # the feature "pixel (0, 0)"
B = float(1 << 24)


def value_cases():
    """(id, cascade dict, image, hand-derived raw list at sf 2)"""
    out = []
    # 3 x 3 window: normrect is the pixel (1, 1) = p: valsum = p, valsq = p^2, nf = 1 * p^2 - p^2 = 0 -> nf = 1, vnf = 1 exactly; value = pixel (0, 0) = 7
    g3 = window_image(3, 3, {(0, 0): 7, (1, 1): 200}, fill=9)
    out.append(("w3-vnf-is-1-below", one_stump((3, 3), PIX00, 7.5), g3, ONE(3, 3)))          # 7 < 7.5: leaf 0 = 1 >= 0.5
    out.append(("w3-vnf-is-1-above", one_stump((3, 3), PIX00, 6.5), g3, []))                 # 7 >= 6.5: leaf 1 = -1
    # value == thr takes leaf 1
    out.append(("tie-takes-leaf1-rejects", one_stump((3, 3), PIX00, 7.0), g3, []))
    out.append(("tie-takes-leaf1-passes", one_stump((3, 3), PIX00, 7.0, (-1.0, 1.0)), g3, ONE(3, 3)))
    # 4 x 4 window: normrect (1, 1, 2, 2) holds 0, 0, 2, 2: valsum = 4, valsq = 8, nf = 4 * 8 - 16 = 16 -> 4, vnf = 0.25; pixel (0, 0) = 10: value = 2.5
    g4 = window_image(4, 4, {(0, 0): 10, (1, 1): 0, (2, 1): 0, (1, 2): 2, (2, 2): 2}, fill=50)
    out.append(("w4-nf-16-below", one_stump((4, 4), PIX00, 2.75), g4, ONE(4, 4)))
    out.append(("w4-nf-16-tie", one_stump((4, 4), PIX00, 2.5), g4, []))
    out.append(("w4-nf-16-above", one_stump((4, 4), PIX00, 2.25), g4, []))
    # a flat window: valsum = 4 * 90, valsq = 4 * 8100, nf = 4 * 32400 - 360^2 = 0: the nf > 0 test fails, nf = 1 (a root of 0 would make value infinite)
    flat = np.full((5, 5), 90, np.uint8)
    out.append(("flat-nf-0-below", one_stump((4, 4), PIX00, 90.5), flat, ONE(4, 4)))
    out.append(("flat-nf-0-above", one_stump((4, 4), PIX00, 89.5), flat, []))
    # third rect: weight 0 is ignored (its pixel is 200), a weight != 0 is added: pixels (0, 0) = 3, (1, 0) = 4, (2, 0) = 200
    g = window_image(3, 3, {(0, 0): 3, (1, 0): 4, (2, 0): 200}, fill=9)
    f0 = [(0, 0, 1, 1, 1.0), (1, 0, 1, 1, 1.0), (2, 0, 1, 1, 0.0)]
    f1 = [(0, 0, 1, 1, 1.0), (1, 0, 1, 1, 1.0), (2, 0, 1, 1, 1.0)]
    out.append(("third-rect-weight-0-ignored", one_stump((3, 3), f0, 7.5), g, ONE(3, 3)))     # 3 + 4 = 7 < 7.5
    out.append(("third-rect-weight-0-ignored-tie", one_stump((3, 3), f0, 7.0), g, []))
    out.append(("third-rect-added", one_stump((3, 3), f1, 207.5), g, ONE(3, 3)))              # 7 + 200 = 207
    out.append(("third-rect-added-above", one_stump((3, 3), f1, 206.5), g, []))
    # ... and added LAST, in f32: pixels 1, 1, 1 with weights 2^24, 1, -(2^24 - 1): (2^24 + 1 -> 2^24) - (2^24 - 1) = 1; exactly, or with the
    # third rect ahead of the second, it is 2.  This is also the f32 feature sum of the weights 16777216 and 1 on two one-pixel rects of
    # value 1: 16777216, not 16777217 -- no f32 threshold lies in (2^24, 2^24 + 1], so the third rect brings the difference down to 1 | 2
    g1 = window_image(3, 3, {(0, 0): 1, (1, 0): 1, (2, 0): 1}, fill=9)
    fb = [(0, 0, 1, 1, B), (1, 0, 1, 1, 1.0), (2, 0, 1, 1, -(B - 1.0))]
    out.append(("f32-feature-sum-third-last", one_stump((3, 3), fb, 1.5), g1, ONE(3, 3)))     # 1 < 1.5
    out.append(("f32-feature-sum-third-last-tie", one_stump((3, 3), fb, 1.0), g1, []))        # 1 == 1: leaf 1
    # the same two rects mirrored, where a threshold does separate them: -2^24 - 1 -> -2^24 in f32, which is not < -2^24; exactly, -16777217 is
    fm = [(0, 0, 1, 1, -B), (1, 0, 1, 1, -1.0)]
    out.append(("f32-feature-sum-two-rects", one_stump((3, 3), fm, -B), g1, []))
    # stage sum in f64: constant votes 1e8, 1, -1e8 against 0.5: 1.0 passes (in f32 the 1 would be lost: the opposite of lbp_cases.vote_order_cascade)
    votes = hand_cascade((3, 3), [PIX00], [(0.5, [(0, 0.0, (v, v)) for v in (1e8, 1.0, -1e8)])])
    out.append(("f64-stage-sum", votes, g3, ONE(3, 3)))
    # the stage threshold is (float)0.5 - 1e-5f: a constant vote of 0.499995 (< 0.5) passes, 0.49998 does not
    out.append(("stage-eps-passes", hand_cascade((3, 3), [PIX00], [(0.5, [(0, 0.0, (0.499995, 0.499995))])]), g3, ONE(3, 3)))
    out.append(("stage-eps-rejects", hand_cascade((3, 3), [PIX00], [(0.5, [(0, 0.0, (0.49998, 0.49998))])]), g3, []))
    return out


# ---- the skip rule on lbp_cases.column_image() (16 x 8, columns repeat 0, 10, 10, 0) at sf 4: 3 x 3 windows at x = 0, 2 .. 12, y = 0, 2, 4; vnf = 1.
# The feature is the window's centre pixel (x + 1, y + 1): 10 at x = 0, 4, 8, 12 (even grid columns), 0 at x = 2, 6, 10 (odd grid columns).
CENTRE = [(1, 1, 1, 1, 1.0)]


def skip_cases():
    """(id, cascade dict, hand-written raw list) -- the lists of lbp_cases.skip_cases, for the same reasons"""
    rows = (0, 2, 4)
    rej_even, rej_odd, all_pass = (0, 5.0, (1.0, -1.0)), (0, 5.0, (-1.0, 1.0)), (0, 5.0, (1.0, 1.0))
    return [
        ("stage0-rejects-even", hand_cascade((3, 3), [CENTRE], [(0.0, [rej_even])]), []),
        ("stage0-rejects-odd", hand_cascade((3, 3), [CENTRE], [(0.0, [rej_odd])]), [[0, y, 3, 3] for y in rows]),
        ("stage1-rejects-even", hand_cascade((3, 3), [CENTRE], [(0.0, [all_pass]), (0.0, [rej_even])]), [[x, y, 3, 3] for y in rows for x in (2, 6, 10)]),
    ]


def scan_rule_cases():
    """lbp_cases.scan_rule_cases with the permissive cascade of the same window as a HAAR one: the hand-derived lists are the scan's, not the evaluator's"""
    return [(cid, permissive(*cd["size"]), shape, sf, mins, maxs, exp) for (cid, cd, shape, sf, mins, maxs, exp) in LK.scan_rule_cases()]
