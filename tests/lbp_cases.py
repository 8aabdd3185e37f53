"""Cascades, images and constructed cases that tests/test_lbp_cpu.py (on the numpy statement, tests/lbp_reference.py) and
tests/test_gpu_lbp.py (on the device) share.  Every expected list of a constructed case is written down here by hand or by the
rule's own closed form, never taken from a run."""
import functools

import numpy as np

import lbp_reference as R
from nubovca import synth

# name -> make_lbp_cascade arguments.  "deep": 20 stages, 139 weak classifiers (the stage-heavy cascade)
CASCADES = {
    "w24": dict(ow=24, oh=24, seed=1, stage_sizes=(3, 4, 5, 6, 7, 8, 9, 10)),
    "w20x28": dict(ow=20, oh=28, seed=2, stage_sizes=(3, 4, 5, 6, 7)),
    "w12": dict(ow=12, oh=12, seed=3, stage_sizes=(2, 3, 4, 5, 6)),
    "deep": dict(ow=24, oh=24, seed=4, stage_sizes=(3, 4, 4, 5, 5, 6, 6, 6, 7, 7, 7, 8, 8, 8, 8, 9, 9, 9, 10, 10)),
}
# (cols, rows, scale factor) of the raw-list cases; the first levels of 1500 x 240 are wider than 1023 (the per-level launches)
IMAGES = [(97, 83, 1.1), (160, 120, 1.2), (333, 251, 1.1), (640, 360, 1.25), (1500, 240, 1.3)]
SMALL_IMAGES = IMAGES[:3]          # what the 20 x 28 and 12 x 12 windows run on


@functools.lru_cache(maxsize=None)
def cascade(name, style="traincascade"):
    """(xml text, the reference reader's cascade)"""
    xml = synth.lbp_cascade_to_xml(_dict(name), style)
    return xml, R.parse_xml(xml)


@functools.lru_cache(maxsize=None)
def _dict(name):
    return synth.make_lbp_cascade(**CASCADES[name])


@functools.lru_cache(maxsize=None)
def image(cols, rows, ow, oh, seed=11):
    """a natural field with the cascade's template pasted at three scales (seeds disjoint from the calibration images')"""
    g = synth.make_gray(cols, rows, synth.frame_seed(3, seed + cols), "natural")
    faces = [(cols // 8, rows // 8, 1.0), (cols // 2, rows // 4, 1.6)]
    if rows >= 3.2 * oh and cols >= 3.2 * ow:
        faces.append((cols // 5, rows // 2 - oh // 2, 2.4))
    faces = [(x, y, s) for (x, y, s) in faces if x + round(ow * s) <= cols and y + round(oh * s) <= rows]
    return synth.paste_lbp_faces(g, faces, ow, oh, seed)


@functools.lru_cache(maxsize=None)
def expected_raw(name, cols, rows, sf, min_size=(0, 0), max_size=(0, 0)):
    c = cascade(name)[1]
    return R.scan(c, image(cols, rows, *c.size), sf, min_size, max_size)


# ------------------------------------------------------------------ constructed cascades
def hand_cascade(size, features, stages):
    """stages: [(file threshold, [(feature, [8 subset words], (leaf0, leaf1))])]"""
    return dict(name="hand", size=size, features=list(features),
                stages=[dict(threshold=t, weak=[dict(feature=f, subset=list(s), leaves=l) for (f, s, l) in w]) for (t, w) in stages])


def only_codes(codes):
    """subset words (as the file writes them: signed 32-bit) with exactly the bits of `codes` set"""
    w = [0] * 8
    for c in codes:
        w[c >> 5] |= 1 << (c & 31)
    return [v - (1 << 32) if v >= (1 << 31) else v for v in w]


def code_cascade(codes):
    """a 3 x 3 window of 1 x 1 cells that passes exactly the windows whose LBP code is one of `codes`"""
    return hand_cascade((3, 3), [(0, 0, 1, 1)], [(0.0, [(0, only_codes(codes), (1.0, -1.0))])])


PERMISSIVE = {}


def permissive(ow, oh):
    """one stage that passes every window"""
    return hand_cascade((ow, oh), [(0, 0, 1, 1)], [(-1.0, [(0, [0] * 8, (1.0, 1.0))])])


# cell (r, c) -> bit of the code
BIT_OF_CELL = {(0, 0): 128, (0, 1): 64, (0, 2): 32, (1, 2): 16, (2, 2): 8, (2, 1): 4, (2, 0): 2, (1, 0): 1}


def cell_image(cells, centre=100, other=50):
    """a 4 x 4 image (ONE 3 x 3 window at sf 2) whose 3 x 3 top-left pixels are `other`, the centre `centre`, and `cells` {(r, c): value}"""
    g = np.full((4, 4), 7, np.uint8)
    g[:3, :3] = other
    g[1, 1] = centre
    for (r, c), v in cells.items():
        g[r, c] = v
    return g


ONE_WINDOW = [[0, 0, 3, 3]]


def code_cases():
    """(id, image, code the single window has) -- derived by hand from the bit table of SURVEY.md A.15"""
    out = []
    for cell, bit in BIT_OF_CELL.items():
        out.append(("bit%d" % bit, cell_image({cell: 200}), bit))                       # that neighbour alone is >= the centre
    out.append(("flat-tie", np.full((4, 4), 90, np.uint8), 255))                       # every cell equals the centre: >= holds everywhere
    out.append(("one-below", cell_image({c: 99 for c in BIT_OF_CELL}), 0))
    out.append(("one-above", cell_image({c: 101 for c in BIT_OF_CELL}), 255))
    out.append(("code31", cell_image({c: 150 for c, b in BIT_OF_CELL.items() if b <= 16}), 31))      # bit 31 of word 0: the word is written negative
    out.append(("code32", cell_image({(0, 2): 150}), 32))                                # bit 0 of word 1
    return out


def vote_order_cascade(order):
    """one stage of three constant votes, threshold 0.5: in f32, 1e8 + 1 - 1e8 = 0 (rejected), 1e8 - 1e8 + 1 = 1 (passes)"""
    votes = {"big-one-minus": (1e8, 1.0, -1e8), "big-minus-one": (1e8, -1e8, 1.0)}[order]
    return hand_cascade((3, 3), [(0, 0, 1, 1)], [(0.5, [(0, [0] * 8, (v, v)) for v in votes])])


# ---- the skip rule.  A 16 x 8 image whose columns repeat 0, 10, 10, 0: at step 2 (one level at sf 4) the 3 x 3 windows of 1 x 1 cells
# at x = 0, 4, 8, 12 (even grid columns) have cell (1, 0) < centre (code even), those at x = 2, 6, 10 (odd grid columns) cell (1, 0) >= centre
# (code odd).  Grid: x = 0, 2 .. 12 (pw = 13), y = 0, 2, 4 (ph = 5).
def column_image():
    g = np.zeros((8, 16), np.uint8)
    g[:, 1::4] = 10
    g[:, 2::4] = 10
    return g


ODD_CODES = only_codes(range(1, 256, 2))
EVEN_CODES = only_codes(range(0, 256, 2))
ALL_CODES = only_codes(range(256))


def skip_cases():
    """(id, cascade dict, hand-written raw list on column_image() at sf 4)"""
    f = [(0, 0, 1, 1)]
    leaf = (1.0, -1.0)
    rows = (0, 2, 4)
    return [
        # stage 0 rejects the even grid columns: column 0 is visited and rejected, 1 is skipped, 2 rejected, 3 skipped ...: nothing, although every odd column would pass
        ("stage0-rejects-even", hand_cascade((3, 3), f, [(0.0, [(0, ODD_CODES, leaf)])]), []),
        # stage 0 rejects the odd grid columns: 0 passes, 1 is rejected, 2 skipped, 3 rejected, 4 skipped, 5 rejected, 6 skipped: column 0 alone
        ("stage0-rejects-odd", hand_cascade((3, 3), f, [(0.0, [(0, EVEN_CODES, leaf)])]), [[0, y, 3, 3] for y in rows]),
        # the same rejections from stage 1 (result -1): nothing is skipped, every odd column is emitted; the last visited column (12) is a reject
        ("stage1-rejects-even", hand_cascade((3, 3), f, [(0.0, [(0, ALL_CODES, leaf)]), (0.0, [(0, ODD_CODES, leaf)])]), [[x, y, 3, 3] for y in rows for x in (2, 6, 10)]),
    ]


def scan_rule_cases():
    """(id, cascade dict, image shape (rows, cols), sf, min_size, max_size, hand-derived raw list) on permissive cascades: every visited window is emitted"""
    out = []
    P24 = permissive(24, 24)
    out.append(("exact-window-no-level", P24, (24, 24), 1.1, (0, 0), (0, 0), []))
    out.append(("one-window", P24, (25, 25), 1.1, (0, 0), (0, 0), [[0, 0, 24, 24]]))          # factor 1.1: sz = 23 < 24, break
    # pw odd (5: x = 0, 2, 4) and even (6: x = 0, 2, 4), ph = 3 (y = 0, 2); sf 4: one level
    out.append(("pw-odd", P24, (27, 29), 4.0, (0, 0), (0, 0), [[x, y, 24, 24] for y in (0, 2) for x in (0, 2, 4)]))
    out.append(("pw-even", P24, (27, 30), 4.0, (0, 0), (0, 0), [[x, y, 24, 24] for y in (0, 2) for x in (0, 2, 4)]))
    # the step changes at factor > 2: a 12 x 12 window on 60 x 60.  sf 1.99: level 2 is 30 x 30 (cvRound(60 / 1.99)), step 2, window 24;
    # sf 2.01: level 2 is 30 x 30 (cvRound(29.85)), step 1, window 24; level 3 (factor ~4) is 15 x 15: 3 x 3 positions at step 1
    P12 = permissive(12, 12)
    l1 = [[x, y, 12, 12] for y in range(0, 48, 2) for x in range(0, 48, 2)]
    for sf, step in ((1.99, 2), (2.01, 1)):
        l2 = [[int(np.rint(x * sf)), int(np.rint(y * sf)), 24, 24] for y in range(0, 18, step) for x in range(0, 18, step)]
        f3 = sf * sf
        l3 = [[int(np.rint(x * f3)), int(np.rint(y * f3)), int(np.rint(12 * f3)), int(np.rint(12 * f3))] for y in range(3) for x in range(3)]
        out.append(("step-at-factor-%g" % sf, P12, (60, 60), sf, (0, 0), (0, 0), l1 + l2 + l3))
        # minSize / maxSize on both sides of level 2's 24 x 24 window
        out.append(("min24-%g" % sf, P12, (60, 60), sf, (24, 24), (0, 0), l2 + l3))
        out.append(("min25-%g" % sf, P12, (60, 60), sf, (25, 25), (0, 0), l3))
        out.append(("max24-%g" % sf, P12, (60, 60), sf, (0, 0), (24, 24), l1 + l2))
        out.append(("max23-%g" % sf, P12, (60, 60), sf, (0, 0), (23, 23), l1))
    return out
