"""Test cascades whose stage sums depend on the summation order, and cascades whose stage thresholds sit on the vote grid
(tests/test_stage_sums_cpu.py, tests/test_gpu_stage_sums.py).

Every evaluator sums a stage either in an order of its own (lane = (window, stump) rounds, LDS accumulators, several stages per
round) -- allowed where plan.cpp's build_stage_recs proves the re-ordering exact (StageRec flag bit 1: every partial sum of every
subset representable; bit 2: integer votes, thr_i = ceil(thr / 2^e)) -- or in OpenCV's left-to-right order.  The cascades of
synth.make_cascade prove order-free in every stage and keep every stage threshold 1e-3 below an achievable sum, so neither the
ordered paths nor the tie rule !(sum < thr) are reached by them.  Here:

  * "order" cascades: one stage gets two constant-vote stumps (left == right) of +2^52 and -2^52 at its two ends.  While the
    running sum holds 2^52 every addition rounds to an integer, so the stage sum depends on where the ballast sits (its
    `twin` has both ballast stumps at the end of the stage: same votes, same threshold, another order).
  * "tie" cascades: votes rounded to multiples of 2^-3 (the integer path) and every biased stage threshold
    fl32(st - 0.0001f) exactly an achievable sum (twin: each threshold one f32 ulp higher, so that the ties fail).
  * "tie_f64": the same with a +2^28 constant vote in every stage -- the sums leave the 2^31 range of the integer path and
    take the f64 order-free path, still exact, still tying (twin: a -2^-3 constant vote more, which turns every tie into a fail).
  * "cut_lo" / "cut_hi": one stage whose sum of vote magnitudes sits one step below / at the integer path's 2147483000 cut
    (in units of 2^-3), the two sides of the proof's integer bound.

Thresholds of changed stages are re-picked on frame content (synth.WindowSample of IMAGES' geometry) so that about half of a
stage's entrants pass, calibrated on the OpenCV-order sum (a sequential float64 loop over the stump votes)."""
import functools
import xml.etree.ElementTree as ET

import numpy as np

from nubovca import synth

SEED = 7
STAGES = [9, 12, 16, 20, 24, 28, 32, 270]     # stage 7: more than 256 stumps (the 256-vote chunks of k_deep and k_roi)
BALLAST = 2.0 ** 52
TIE_BALLAST = 2.0 ** 28
GRID = 0.125
INT_CUT = 2147483000
BIAS = np.float32(0.0001)

# order-sensitive stage of each "order" cascade: stage 0 (k_stage0, the tile prefix, k_roi's first stage, the dense FIND_BIGGEST
# launch), an early stage between order-free ones (a multi-stage round stops at the spec_run boundary), a stage behind
# deep_stage 6, the last stage (270 stumps)
ORDER_STAGES = {"order_s0": 0, "order_s3": 3, "order_s6": 6, "order_s7": 7}
CUT_STAGE = 4
NAMES = list(ORDER_STAGES) + ["tie", "tie_f64", "cut_lo", "cut_hi"]

# the images the tests detect on (and the cascades are calibrated on): (w, h, kind, seed, faces)
IMAGES = [(320, 240, "natural", 31, [(60, 40, 100), (200, 120, 50)]),
          (640, 480, "natural", 32, [(100, 80, 160), (420, 260, 90)])]

PART_KINDS = {"eye": ("righteye", "lefteye"), "nose": ("nose",)}
PART_ORDER_STAGE = 9


def f32(v):
    return float(np.float32(v))


def biased(st):
    """icv_stage_threshold_bias in float arithmetic: the threshold every evaluator compares with"""
    return float(np.float32(np.float32(st) - BIAS))


def threshold_for(target):
    """an f32 stage threshold whose biased value is exactly `target` (None if there is none)"""
    t = np.float32(target)
    if float(t) != target:
        return None
    st = np.float32(t + BIAS)
    for _ in range(64):
        b = biased(st)
        if b == target:
            return float(st)
        st = np.nextafter(st, np.float32(np.inf) if b < target else np.float32(-np.inf), dtype=np.float32)
    return None


def image(w, h, kind, seed, faces):
    return synth.equalize_np(synth.make_gray(w, h, seed, kind, faces))


def images():
    return [image(*a) for a in IMAGES]


def opencv_sum(votes):
    """[windows, stumps] votes -> the stage sum in OpenCV's order (left to right, float64)"""
    s = np.zeros(votes.shape[0])
    for j in range(votes.shape[1]):
        s = s + votes[:, j]
    return s


def stump_votes(sample, st):
    """per-window, per-stump votes of a stump-form stage on the windows still alive in `sample`"""
    cols = [sample.stage_votes([f], [t], [float(np.float32(a0))], [float(np.float32(a1))])
            for f, t, a0, a1 in zip(st["features"], st["thresholds"], st["left"], st["right"])]
    return np.stack(cols, axis=1) if cols else np.zeros((sample.alive_count(), 0))


def half_cut(sums):
    """the achievable sum at which the pass rate is closest to one half"""
    cand = np.unique(sums)
    rates = np.array([(sums >= c).mean() for c in cand])
    return float(cand[np.argmin(np.abs(rates - 0.5))])


def _const_stump(st, v):
    return dict(feature=st["features"][0], threshold=st["thresholds"][0], left=v, right=v)


def _insert(st, pos, stump):
    pos = len(st["features"]) if pos is None else pos
    st["features"].insert(pos, stump["feature"]); st["thresholds"].insert(pos, stump["threshold"])
    st["left"].insert(pos, stump["left"]); st["right"].insert(pos, stump["right"])


def _grid(v):
    return float(np.sign(v) * max(1, int(np.rint(abs(v) / GRID))) * GRID)


def _copy(c):
    return dict(name=c["name"], size=c["size"],
                stages=[dict(features=list(s["features"]), thresholds=list(s["thresholds"]), left=list(s["left"]),
                             right=list(s["right"]), stage_threshold=s["stage_threshold"]) for s in c["stages"]])


def _cut_ballast(st, target):
    """a constant vote B (f32, a multiple of 16 at most 2^28) and a small constant vote c: sum of |votes| = target * 2^-3"""
    v8 = int(round(sum(max(abs(a), abs(b)) for a, b in zip(st["left"], st["right"])) / GRID))
    B = 2 ** 28
    while target - 8 * B - v8 < 1:
        B -= 16
    c = (target - 8 * B - v8) * GRID
    return float(B), c


def _stage_cut(st, sums, variant, twin_sums=None):
    """the threshold of a changed stage, from the OpenCV-order sums of its entrants"""
    if variant == "order":
        # the sums are integers (pass <=> sum >= the cut): of the cuts that pass 30 .. 70 % of the entrants, the one at which
        # the order matters most
        cand = np.unique(sums)
        rates = np.array([(sums >= c).mean() for c in cand])
        flips = np.array([((sums >= c) != (twin_sums >= c)).sum() for c in cand])
        score = np.where(np.abs(rates - 0.5) <= 0.2, flips, -1) - np.abs(rates - 0.5)
        return float(cand[np.argmax(score)]) - 0.5
    if variant == "tie_f64":
        return TIE_BALLAST                   # f32 neighbours of 2^28 are 32 / 16 apart: the only tie point in reach
    if variant.startswith("cut"):
        B = st["_B"]
        return B if abs((sums >= B).mean() - 0.5) <= abs((sums >= B + 16).mean() - 0.5) else B + 16
    # tie: an achievable sum near the median that many windows hit exactly, whose biased f32 form exists
    cand, cnt = np.unique(sums, return_counts=True)
    rates = np.array([(sums >= c).mean() for c in cand])
    order = np.argsort(np.abs(rates - 0.5) - 0.02 * cnt / max(1, cnt.max()))
    for k in order:
        if threshold_for(float(cand[k])) is not None:
            return float(cand[k])
    raise RuntimeError("no tie threshold")


def build(base, variant, changed, sample, calibrate=True):
    """returns (cascade, twin, summary): `changed` = the stage indices to change (order: one stage; tie: every stage); calibrate:
    the unchanged stages get their thresholds re-picked on `sample` too"""
    casc, twin = _copy(base), _copy(base)
    info = []
    for si, (st, tw) in enumerate(zip(casc["stages"], twin["stages"])):
        if si in changed:
            if variant != "order":
                for s in (st, tw):
                    s["left"] = [_grid(v) for v in s["left"]]; s["right"] = [_grid(v) for v in s["right"]]
            if variant == "order":
                _insert(st, 0, _const_stump(st, BALLAST)); _insert(st, None, _const_stump(st, -BALLAST))
                _insert(tw, None, _const_stump(tw, BALLAST)); _insert(tw, None, _const_stump(tw, -BALLAST))
            elif variant == "tie_f64":
                mid = len(st["features"]) // 2
                _insert(st, mid, _const_stump(st, TIE_BALLAST)); _insert(tw, mid, _const_stump(tw, TIE_BALLAST))
                _insert(tw, None, _const_stump(tw, -GRID))
            elif variant.startswith("cut") and si == CUT_STAGE:
                B, c = _cut_ballast(st, INT_CUT - 1 if variant == "cut_lo" else INT_CUT)
                for s in (st, tw):
                    _insert(s, 1, _const_stump(s, B)); _insert(s, None, _const_stump(s, c))
                st["_B"] = B
            sums = opencv_sum(stump_votes(sample, st))
            twin_sums = opencv_sum(stump_votes(sample, tw)) if variant == "order" else None
            target = _stage_cut(st, sums, variant if not variant.startswith("cut") or si == CUT_STAGE else "tie", twin_sums)
            st.pop("_B", None)
            thr = target if variant == "order" else threshold_for(target)
            assert thr is not None and np.float32(thr) == thr
            st["stage_threshold"] = tw["stage_threshold"] = thr
            if variant == "tie":
                tw["stage_threshold"] = float(np.nextafter(np.float32(thr), np.float32(np.inf), dtype=np.float32))
            thr_b = biased(thr)
            ties = int((sums == thr_b).sum())
            keep = sums >= thr_b
            info.append(dict(stage=si, entrants=len(sums), passed=int(keep.sum()), ties=ties))
        else:
            sums = opencv_sum(stump_votes(sample, st))
            if calibrate:          # as make_cascade(calib=...) does it: about half of the entrants pass, 1e-3 below an achievable sum
                st["stage_threshold"] = tw["stage_threshold"] = f32(half_cut(sums) - 1e-3)
            keep = sums >= biased(st["stage_threshold"])
        sample.keep(keep)
    return casc, twin, info


@functools.lru_cache(maxsize=None)
def _base():
    return synth.make_cascade(seed=SEED, stages=STAGES, open_stages=len(STAGES))


def _sample(imgs):
    return synth.WindowSample(imgs, scale_factor=1.1, min_size=(0, 0))


@functools.lru_cache(maxsize=None)
def variant(name):
    """(xml, twin xml, summary) of one of NAMES"""
    base = _base()
    if name in ORDER_STAGES:
        c, t, info = build(base, "order", {ORDER_STAGES[name]}, _sample(images()))
    else:
        c, t, info = build(base, name, set(range(len(STAGES))), _sample(images()))
    c["name"] = t["name"] = "stage_sums_" + name
    return synth.cascade_to_xml(c), synth.cascade_to_xml(t), info


def part_images():
    """face regions of a part search's working image (as synth.calibrated_part_cascade_xml samples them)"""
    out = []
    for i in range(4):
        size = 88 + 4 * i
        out.append(synth.equalize_np(synth.make_gray(176, 176, 7100 + 13 * i, "natural", [(88 - size // 2, 88 - size // 2 + i % 3 - 1, size)])))
    return out


@functools.lru_cache(maxsize=None)
def part_variant(part, kind):
    """(xml, twin xml, summary) of a part cascade (synth.synthetic_part_cascade_xml's draws): kind 'order' (stage
    PART_ORDER_STAGE) or 'tie' (every stage)"""
    seed = {"righteye": 101, "lefteye": 102, "nose": 103}[part]
    base = synth.make_cascade(seed=seed, stages=synth.PART_STAGES, tmpl=synth.part_template(part))
    sample = synth.WindowSample(part_images(), scale_factor=1.1, min_size=(20, 20))
    changed = {PART_ORDER_STAGE} if kind == "order" else set(range(len(synth.PART_STAGES)))
    c, t, info = build(base, kind, changed, sample, calibrate=False)
    c["name"] = t["name"] = "stage_sums_%s_%s" % (part, kind)
    return synth.cascade_to_xml(c), synth.cascade_to_xml(t), info


# ------------------------------------------------------------------ an XML cascade back to make_cascade's form
def xml_to_cascade(text):
    """stump-form old-format cascade XML (as cascade_to_xml writes it) -> the dict cascade_to_xml takes"""
    root = ET.fromstring(text)
    node = next(k for k in root if k.get("type_id") == "opencv-haar-classifier")
    w, h = (int(v) for v in node.find("size").text.split())
    stages = []
    for st in node.find("stages"):
        d = dict(features=[], thresholds=[], left=[], right=[], stage_threshold=float(st.find("stage_threshold").text))
        for tree in st.find("trees"):
            (nd,) = list(tree)
            rects = []
            for r in nd.find("feature").find("rects"):
                x, y, rw, rh, wt = r.text.split()
                rects.append((int(x), int(y), int(rw), int(rh), float(wt)))
            d["features"].append(rects); d["thresholds"].append(float(nd.find("threshold").text))
            d["left"].append(float(nd.find("left_val").text)); d["right"].append(float(nd.find("right_val").text))
        stages.append(d)
    return dict(name=node.tag, size=(w, h), stages=stages)


FACE_ORDER_STAGE, FACE_TIE_STAGE = 14, 6


def face_variant(calibrated_xml):
    """the calibrated 22-stage cascade with one order-sensitive late stage (ballast at its ends; the integer stage sums keep
    the stage's threshold meaningful) and one vote-grid stage whose biased threshold is an achievable sum"""
    c = xml_to_cascade(calibrated_xml)
    st = c["stages"][FACE_ORDER_STAGE]
    _insert(st, 0, _const_stump(st, BALLAST)); _insert(st, None, _const_stump(st, -BALLAST))
    st = c["stages"][FACE_TIE_STAGE]
    st["left"] = [_grid(v) for v in st["left"]]; st["right"] = [_grid(v) for v in st["right"]]
    target = np.round(st["stage_threshold"] / GRID) * GRID
    while threshold_for(target) is None:
        target += GRID
    st["stage_threshold"] = threshold_for(target)
    c["name"] = "stage_sums_face_1080p"
    return synth.cascade_to_xml(c)
