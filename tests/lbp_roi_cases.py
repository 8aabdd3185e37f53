"""Cases of the small-image LBP route (csrc/kernels_roi_lbp.hip, roi_batch.cpp on lbp_roi_tables.cpp) that tests/test_lbp_roi_cpu.py
(on the numpy statement, tests/lbp_reference.py) and tests/test_gpu_lbp_roi.py (on the device) share.  Every expected list is the
statement's (R.scan) or a closed form written down here, never a run of the library.  The constants of the route are read from
its headers; the CPU test checks them against a program compiled from the same headers."""
import functools
import os
import re

import numpy as np

import lbp_cases as K
import lbp_reference as R
from nubovca import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")


def _const(header, pattern):
    return int(re.search(pattern, open(os.path.join(CSRC, header)).read()).group(1))


ROI_MAX_WIN = _const("device_records.h", r"kRoiMaxWin = (\d+);")                      # queue length: grid positions of one workgroup
SHORT_WIN = _const("device_records.h", r"#define NVCA_ROI_LBP_SHORT_WIN (\d+)")        # queue length up to which a stage spreads its votes over the waves
VOTE_WORDS = _const("device_records.h", r"kRoiLbpVoteWords = (\d+);")
HAAR_MAX_WORDS = _const("roi_batch.cpp", r"kRoiMaxWords = (\d+);")                     # k_roi's bound: (cols + 1) * (rows + 2) words
# lbp_roi_tables.h: kRoiLbpMaxBytes and lbp_roi_image_bytes, restated
MAX_BYTES = 160 * 1024 - (2 * ROI_MAX_WIN * 2 + 16 + VOTE_WORDS * 4) - 64


def image_bytes(cols, rows):
    return 4 * (((cols + 1) * (rows + 1) + 3) & ~3) + ((cols * rows + 15) & ~15)


def fits_lds(cols, rows):
    return image_bytes(cols, rows) <= MAX_BYTES


def roi_lds_bytes(plane_words, lev_bytes):
    """roi_lbp_lds_bytes of device_records.h: sum plane | two queues | counters | votes | level image, each a multiple of 16 bytes"""
    return ((plane_words + 3) & ~3) * 4 + 2 * ROI_MAX_WIN * 2 + 16 + VOTE_WORDS * 4 + ((lev_bytes + 15) & ~15)


def roi_lds_total(cols, rows):
    """the most a job on a cols x rows image asks for"""
    return roi_lds_bytes((cols + 1) * (rows + 1), cols * rows)


def haar_fits(cols, rows):
    return (cols + 1) * (rows + 2) <= HAAR_MAX_WORDS


def bound_images():
    """(cols, rows) just inside and just outside the LDS bound, 200 columns wide"""
    rows = 1
    while fits_lds(200, rows + 1):
        rows += 1
    return (200, rows), (200, rows + 1)


# ------------------------------------------------------------------ the skip rule across the 64-column chunk
ODD_STAGE0 = K.hand_cascade((3, 3), [(0, 0, 1, 1)], [(0.0, [(0, K.ODD_CODES, (1.0, -1.0))])])
N_COLS = 67                     # grid columns: one whole chunk of 64 and three more


def pattern_image(passes):
    """passes [grid rows][n] of 0 / 1 -> a (2 * grid rows + 2) x (2 n + 2) image: at scale factor 4 the 3 x 3 window has ONE level at step 2,
    grid column j's window lies at x = 2 j, and its bit 1 is g[y + 1][2 j] >= g[y + 1][2 j + 1] -- pairs disjoint from one column to the next.
    Column j of grid row k passes stage 0 of ODD_STAGE0 iff passes[k][j]."""
    passes = np.atleast_2d(np.asarray(passes, np.uint8))
    gr, n = passes.shape
    g = np.zeros((2 * gr + 2, 2 * n + 2), np.uint8)
    for k in range(gr):
        row = np.zeros(2 * n + 2, np.uint8)
        row[0:2 * n:2] = 10 * passes[k]
        row[1:2 * n:2] = 10 * (1 - passes[k])
        g[2 * k + 1] = row              # the row the windows of grid row k read their bit 1 from
        g[2 * k + 2] = row
    g[0] = g[1]
    return g


def run_row(end, length, n=N_COLS):
    """every column passes but the `length` columns that end at `end`; closed form of what the serial walk emits: every passing column,
    minus the one behind the run when the run is odd (the walk steps over it)"""
    p = np.ones(n, np.uint8)
    p[end - length + 1:end + 1] = 0
    emitted = [j for j in range(n) if p[j] and not (j == end + 1 and length % 2 == 1)]
    return p, emitted


RUNS = [(63, L) for L in (1, 2, 3, 4, 61, 62, 63, 64)] + [(62, L) for L in (1, 2, 62, 63)] + [(64, L) for L in (1, 2, 64, 65)]


def skip_chunk_cases():
    """(id, image, closed-form raw list) on ODD_STAGE0 at scale factor 4"""
    out = []
    for end, L in RUNS:
        p, em = run_row(end, L)
        out.append(("run%d-end%d" % (L, end), pattern_image([p, p, p]), [[2 * j, 2 * k, 3, 3] for k in range(3) for j in em]))
    rows = [run_row(63, 3), run_row(63, 4), run_row(64, 61), run_row(62, 1)]          # rows that differ from one another
    out.append(("rows-differ", pattern_image([r[0] for r in rows]), [[2 * j, 2 * k, 3, 3] for k, r in enumerate(rows) for j in r[1]]))
    return out


# ------------------------------------------------------------------ named cascades on natural images
# (id, cascade, cols, rows, sf): bands of whole rows / a last band of one row / a single band / both lane mappings of the later stages
NAMED = [("bands-w12-160x90", "w12", 160, 90, 1.25), ("last-band-one-row-w24-120x110", "w24", 120, 110, 1.1),
         ("single-band-w12-97x83", "w12", 97, 83, 1.1), ("short-queues-deep-97x83", "deep", 97, 83, 1.1),
         ("outside-haar-bound-w24-160x120", "w24", 160, 120, 1.2)]
TOO_MANY_LEVELS = ("w12", 97, 83, 1.02)            # more than 63 levels: the job does not fit the candidate key


@functools.lru_cache(maxsize=None)
def named_case(cid):
    """(xml, gray, sf, expected raw list, statistics of the statement's scan)"""
    _, name, cols, rows, sf = next(c for c in NAMED if c[0] == cid)
    xml, ref = K.cascade(name)
    gray = K.image(cols, rows, *ref.size)
    stats = {}
    exp = R.scan(ref, gray, sf, stats=stats)
    return xml, gray, sf, exp, stats


def grid_of(ow, oh, cols, rows, sf, min_size=(0, 0), max_size=(0, 0)):
    """[(grid columns, grid rows)] per level"""
    out = []
    for factor, sz, _ in R.levels(ow, oh, cols, rows, sf, min_size, max_size):
        step = 1 if factor > 2.0 else 2
        out.append((len(range(0, sz[0] - ow, step)), len(range(0, sz[1] - oh, step))))
    return out


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
        res = R.grid_results(ref, orc.integral(lev)[0], xs, ys)
        vis = np.zeros(res.shape, bool)
        for iy in range(len(ys)):
            vis[iy, R.walk_row(res[iy])] = True
        rows_per = max(1, ROI_MAX_WIN // len(xs))
        for gy0 in range(0, len(ys), rows_per):
            r, v = res[gy0:gy0 + rows_per], vis[gy0:gy0 + rows_per]
            out.append([int(np.count_nonzero(v & ((r > 0) | (r <= -s)))) for s in range(1, len(ref.stage_sizes))])
    return out


# ------------------------------------------------------------------ every case of the device test
def hand_cases():
    """(id, cascade dict, image, sf, min_size, max_size, expected raw list): the closed forms above and lbp_cases' hand-written lists,
    all on images that take the small route"""
    out = [(cid, ODD_STAGE0, g, 4.0, (0, 0), (0, 0), exp) for cid, g, exp in skip_chunk_cases()]
    for cid, cdict, shape, sf, mins, maxs, exp in K.scan_rule_cases():
        out.append((cid, cdict, np.full(shape, 120, np.uint8), sf, mins, maxs, exp))
    for cid, cdict, exp in K.skip_cases():
        out.append((cid, cdict, K.column_image(), 4.0, (0, 0), (0, 0), exp))
    for cid, gray, code in K.code_cases():
        out.append(("code-" + cid, K.code_cascade([code]), gray, 2.0, (0, 0), (0, 0), K.ONE_WINDOW))
        out.append(("not-code-" + cid, K.code_cascade([c for c in range(256) if c != code]), gray, 2.0, (0, 0), (0, 0), []))
    flat = np.full((4, 4), 90, np.uint8)
    out.append(("vote-order-big-one-minus", K.vote_order_cascade("big-one-minus"), flat, 2.0, (0, 0), (0, 0), []))
    out.append(("vote-order-big-minus-one", K.vote_order_cascade("big-minus-one"), flat, 2.0, (0, 0), (0, 0), K.ONE_WINDOW))
    out += vote_order_stage1_cases()
    return out


def vote_order_stage1_cases():
    """lbp_cases' order-dependent votes (1e8 + 1 - 1e8 = 0 in f32, 1e8 - 1e8 + 1 = 1) as STAGE 1 behind a stage 0 that passes everything,
    on a flat 60 x 60 image at scale factor 4: every window is visited and reaches stage 1.  Level 0 queues 29 x 29 = 841 windows (a
    window per lane), level 1 (15 x 15, step 1) 12 x 12 = 144 and level 2 (4 x 4) one (the votes spread over the waves): in one order
    nothing is emitted, in the other every grid position of every level."""
    every = []
    for f, n, step in ((1.0, 29, 2), (4.0, 12, 1), (16.0, 1, 1)):
        every += [[int(np.rint(x * step * f)), int(np.rint(y * step * f)), int(np.rint(3 * f)), int(np.rint(3 * f))] for y in range(n) for x in range(n)]
    out = []
    for order, exp in (("big-one-minus", []), ("big-minus-one", every)):
        votes = K.vote_order_cascade(order)["stages"][0]
        cdict = K.permissive(3, 3)
        cdict = dict(cdict, stages=cdict["stages"] + [votes])
        out.append(("stage1-vote-order-" + order, cdict, np.full((60, 60), 90, np.uint8), 4.0, (0, 0), (0, 0), exp))
    return out


def hand_xml(cdict):
    return synth.lbp_cascade_to_xml(cdict)
