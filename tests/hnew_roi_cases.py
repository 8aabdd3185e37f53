"""Cases of the small-image route of new-format HAAR cascades (csrc/kernels_roi_hnew.hip, roi_batch.cpp on hnew_roi_tables.cpp; opt-in
per cascade through nvca_cascade_set_small_route) that tests/test_hnew_roi_cpu.py (on the numpy statement, tests/haar_new_reference.py)
and tests/test_gpu_hnew_roi.py (on the device) share.  Every expected list is the statement's (R.scan / R.detect) or a closed form
written down here, never a run of the library.  The constants of the route are read from its headers; the CPU test checks them
against a program compiled from the same headers."""
import functools
import os
import re

import numpy as np

import haar_new_cases as K
import haar_new_reference as R
import lbp_roi_cases as LR
from nubovca import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")


def _const(header, pattern):
    return int(re.search(pattern, open(os.path.join(CSRC, header)).read()).group(1))


ROI_MAX_WIN = _const("device_records.h", r"kRoiMaxWin = (\d+);")                       # queue length: grid positions of one workgroup
SHORT_WIN = _const("device_records.h", r"#define NVCA_ROI_HNEW_SHORT_WIN (\d+)")        # queue length up to which a stage spreads its votes over the waves
VOTE_WORDS = _const("device_records.h", r"kRoiHnewVoteWords = (\d+);")                 # f32 votes a chunk of such a stage holds
# device_records.h: roi_hnew_fixed_bytes -- two queues | counters | votes | vnf (an f64 per grid position) -- and hnew_roi_tables.h:
# kRoiHnewMaxBytes, hnew_roi_image_bytes, restated
FIXED_BYTES = 2 * ROI_MAX_WIN * 2 + 16 + VOTE_WORDS * 4 + ROI_MAX_WIN * 8
MAX_BYTES = 160 * 1024 - FIXED_BYTES - 64


def image_bytes(cols, rows):
    """the sum plane and the squared plane of the image: (cols + 1) x (rows + 1) words each, rounded up to 16 bytes"""
    return 8 * (((cols + 1) * (rows + 1) + 3) & ~3)


def fits_lds(cols, rows):
    return image_bytes(cols, rows) <= MAX_BYTES


def roi_lds_bytes(plane_words):
    """roi_hnew_lds_bytes of device_records.h"""
    return 2 * ((plane_words + 3) & ~3) * 4 + FIXED_BYTES


def bound_images():
    """(cols, rows) just inside and just outside the LDS bound, 200 columns wide"""
    rows = 1
    while fits_lds(200, rows + 1):
        rows += 1
    return (200, rows), (200, rows + 1)


# ------------------------------------------------------------------ the skip rule across the 64-column chunk
# stage 0: ONE stump on the two single-pixel rects (0, 1) weight +1 and (1, 1) weight -1, stump threshold 0, leaves (-1, +1), stage
# threshold 0.  In a 3 x 3 window the normrect is the single pixel (1, 1) = p: nf = 1 * p^2 - p^2 = 0, not positive, so vnf = 1 and
# the value is g[y + 1][x] - g[y + 1][x + 1] itself: the window passes iff that difference is not negative.  On
# lbp_roi_cases.pattern_image (windows at x = 2 j, the pairs (2 j, 2 j + 1) disjoint from one grid column to the next) the
# difference is +10 where the pattern passes and -10 where it does not -- the closed forms of lbp_roi_cases carry over unchanged.
PAIR_STAGE0 = K.hand_cascade((3, 3), [[(0, 1, 1, 1, 1.0), (1, 1, 1, 1, -1.0)]], [(0.0, [(0, 0.0, (-1.0, 1.0))])])
N_COLS, RUNS, run_row, pattern_image = LR.N_COLS, LR.RUNS, LR.run_row, LR.pattern_image


def skip_chunk_cases():
    """(id, image, closed-form raw list) on PAIR_STAGE0 at scale factor 4: lbp_roi_cases.skip_chunk_cases' images and lists"""
    return LR.skip_chunk_cases()


# ------------------------------------------------------------------ named cascades on natural images (haar_new_cases.image: a flat corner patch)
# (id, cascade, cols, rows, sf): bands of whole rows / a last band of one row / a single band a level / a window that is not square /
# both lane mappings of the later stages
NAMED = [("bands-w12-160x90", "w12", 160, 90, 1.25), ("last-band-one-row-w24-120x110", "w24", 120, 110, 1.1),
         ("single-band-w12-97x83", "w12", 97, 83, 1.1), ("non-square-w20x28-97x83", "w20x28", 97, 83, 1.1),
         ("short-queues-deep-97x83", "deep", 97, 83, 1.1)]
NAMED_WINDOWS = {"bands-w12-160x90": 138, "last-band-one-row-w24-120x110": 853, "single-band-w12-97x83": 250,
                 "non-square-w20x28-97x83": 88, "short-queues-deep-97x83": 28}
TOO_MANY_LEVELS = ("w12", 97, 83, 1.02)            # more than 63 levels: the job does not fit the candidate key
BOUND_SF = 1.3                                     # what "w24" scans the two bound images with


@functools.lru_cache(maxsize=None)
def named_case(cid):
    """(xml, gray, sf, expected raw list, statistics of the statement's scan)"""
    _, name, cols, rows, sf = next(c for c in NAMED if c[0] == cid)
    xml, ref = K.cascade(name)
    gray = K.image(cols, rows, *ref.size)
    stats = {}
    exp = R.scan(ref, gray, sf, stats=stats)
    return xml, gray, sf, exp, stats


grid_of = LR.grid_of                               # [(grid columns, grid rows)] per level: the scan's levels are A.15's


def band_queue_lengths(ref, gray, sf):
    """per workgroup of the route (a level, or a band of whole rows of at most ROI_MAX_WIN positions) and stage s >= 1: the number of
    visited windows alive in front of stage s -- the queue length the kernel chooses its lane mapping by"""
    import orc
    rows, cols = gray.shape
    ow, oh = ref.size
    out = []
    for factor, sz, _ in R.levels(ow, oh, cols, rows, sf):
        lev = gray if (sz[0], sz[1]) == (cols, rows) else orc.resize_linear(gray, sz[0], sz[1])
        step = 1 if factor > 2.0 else 2
        xs, ys = np.arange(0, sz[0] - ow, step), np.arange(0, sz[1] - oh, step)
        S, Q = orc.integral(lev)
        res = R.grid_results(ref, S, Q, xs, ys)
        vis = np.zeros(res.shape, bool)
        for iy in range(len(ys)):
            vis[iy, R.walk_row(res[iy])] = True
        rows_per = max(1, ROI_MAX_WIN // len(xs))
        for gy0 in range(0, len(ys), rows_per):
            r, v = res[gy0:gy0 + rows_per], vis[gy0:gy0 + rows_per]
            out.append([int(np.count_nonzero(v & ((r > 0) | (r <= -s)))) for s in range(1, len(ref.stage_sizes))])
    return out


# ------------------------------------------------------------------ wide stages: more votes than the vote area holds
# a 12 x 12 cascade whose last two stages have 70 and 130 stumps, on 97 x 83: queues of at most 64 windows meet them in chunks of
# VOTE_WORDS / 64 = 64 stumps (2 and 3 chunks), queues of 65 .. 256 windows in chunks of 32, 21 or 16 -- a chunk boundary inside a
# stage in both paddings (tests/test_hnew_roi_cpu.py asserts both on the statement)
WIDE = dict(ow=12, oh=12, seed=1, stage_sizes=(2, 3, 17, 33, 70, 130), pass_rate=0.7)
WIDE_IMAGE = (97, 83, 1.1)


@functools.lru_cache(maxsize=None)
def wide_cascade():
    """(xml text, the reference reader's cascade)"""
    xml = synth.haar_new_cascade_to_xml(synth.make_haar_new_cascade(**WIDE))
    return xml, R.parse_xml(xml)


@functools.lru_cache(maxsize=None)
def wide_case():
    """(xml, gray, sf, expected raw list)"""
    xml, ref = wide_cascade()
    cols, rows, sf = WIDE_IMAGE
    gray = K.image(cols, rows, *ref.size)
    return xml, gray, sf, R.scan(ref, gray, sf)


# ------------------------------------------------------------------ bright images: squared sums near their largest
@functools.lru_cache(maxsize=None)
def bright_image():
    """noise in 249 .. 255 at the inside-bound size: the squared plane's last word is above 249^2 cols rows -- within 5 % of the most an
    image inside the bound can total -- and a 12 x 12 window's nf is a small difference of two products near 6 * 10^8"""
    cols, rows = bound_images()[0]
    return np.random.default_rng(78).integers(249, 256, size=(rows, cols)).astype(np.uint8)


BRIGHT = ("w12", 1.2)


@functools.lru_cache(maxsize=None)
def bright_case():
    """(xml, gray, sf, expected raw list, stats)"""
    xml, ref = K.cascade(BRIGHT[0])
    stats = {}
    return xml, bright_image(), BRIGHT[1], R.scan(ref, bright_image(), BRIGHT[1], stats=stats), stats


# ------------------------------------------------------------------ every constructed case of the device test
def hand_cases():
    """(id, cascade dict, image, sf, min_size, max_size, expected raw list): the closed forms above and haar_new_cases' hand-written lists,
    all on images that take the small route"""
    out = [(cid, PAIR_STAGE0, g, 4.0, (0, 0), (0, 0), exp) for cid, g, exp in skip_chunk_cases()]
    for cid, cdict, shape, sf, mins, maxs, exp in K.scan_rule_cases():
        out.append((cid, cdict, np.full(shape, 120, np.uint8), sf, mins, maxs, exp))
    for cid, cdict, exp in K.skip_cases():
        out.append((cid, cdict, K.LK.column_image(), 4.0, (0, 0), (0, 0), exp))
    for cid, cdict, gray, exp in K.value_cases():
        out.append((cid, cdict, gray, 2.0, (0, 0), (0, 0), exp))
    return out


def hand_xml(cdict):
    return synth.haar_new_cascade_to_xml(cdict)
