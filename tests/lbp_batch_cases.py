"""Batches of images that tests/test_lbp_batch_cpu.py (on the numpy statement, tests/lbp_reference.py) and tests/test_gpu_lbp_batch.py
(on the device) share: every slot of a batch holds a different image, and a slot's expected list is computed once, by R.scan on that
image alone."""
import functools

import numpy as np

import lbp_cases as K
import lbp_reference as R
from nubovca import synth

# (cascade of lbp_cases.CASCADES, cols, rows, scale factor, images): the smallest shapes on which the image axis can go wrong --
# one bit word a row; an odd pitch with several words a row; first levels wider than 1023 (the per-level pyramid launches with
# more than one image); 20 stages and about ten candidates an image (the thin late stage groups on the merged list); a window that
# is not square
BATCHES = [("w24", 97, 83, 1.1, 3), ("w24", 333, 251, 1.1, 3), ("w24", 1500, 240, 1.3, 2), ("deep", 160, 120, 1.2, 5), ("w20x28", 97, 83, 1.1, 2)]
BATCH_IDS = ["%s-%dx%d-x%d" % (b[0], b[1], b[2], b[4]) for b in BATCHES]
SEED0 = 11                         # slot i holds K.image(..., seed=SEED0 + i); seed 11 is the single-image tests' image
BOUNDARY = ("w12", 64, 48, 1.2)    # the job-size boundary: 32 images (one job) and 33 (two jobs in one round), seeds 100 ..
BOUNDARY_SEED0 = 100


def images(name, cols, rows, n, seed0=SEED0):
    ow, oh = K.cascade(name)[1].size
    return [K.image(cols, rows, ow, oh, seed0 + i) for i in range(n)]


@functools.lru_cache(maxsize=None)
def expected(name, cols, rows, sf, seed):
    c = K.cascade(name)[1]
    return R.scan(c, K.image(cols, rows, *c.size, seed), sf)


def expected_batch(name, cols, rows, sf, n, seed0=SEED0):
    return [expected(name, cols, rows, sf, seed0 + i) for i in range(n)]


# ---- overflow: a 24 x 24 window of 8 x 8 cells that passes exactly code 255 (every neighbour cell >= the centre cell).  A flat image
# passes everywhere, the other two at a few hundred windows: a batch whose total and whose largest image fall on different sides of
# the candidate capacities 1024 and 4096 per image (tests/test_lbp_batch_cpu.py asserts which)
CODE255_GEOM = (160, 120, 1.2)


def code255_cascade():
    return K.hand_cascade((24, 24), [(0, 0, 8, 8)], [(0.0, [(0, K.only_codes([255]), (1.0, -1.0))])])


@functools.lru_cache(maxsize=None)
def code255_images():
    cols, rows, _ = CODE255_GEOM
    y, x = np.mgrid[0:rows, 0:cols]
    return (synth.make_gray(cols, rows, 5, "natural"), np.full((rows, cols), 120, np.uint8), ((x + 2 * y) % 251).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def code255_expected():
    ref = R.parse_xml(synth.lbp_cascade_to_xml(code255_cascade()))
    return tuple(R.scan(ref, g, CODE255_GEOM[2]) for g in code255_images())


# ---- the skip rule per (image, row): K.column_image() rolled by two columns swaps the codes of the even and the odd grid columns,
# so a batch [column image, rolled, column image] answers differently in its middle slot.  The rolled image's lists, by hand:
def rolled_column_image():
    return np.roll(K.column_image(), 2, axis=1)


ROLLED_EXPECTED = {
    # grid column 0 (odd code now) passes, 1 is rejected by stage 0, 2 is skipped, 3 rejected ...: column 0 alone
    "stage0-rejects-even": [[0, y, 3, 3] for y in (0, 2, 4)],
    # grid column 0 is rejected, 1 skipped, 2 rejected ...: nothing, although every odd grid column would pass
    "stage0-rejects-odd": [],
    # rejections from stage 1 skip nothing: every even grid column is emitted
    "stage1-rejects-even": [[x, y, 3, 3] for y in (0, 2, 4) for x in (0, 4, 8, 12)],
}
