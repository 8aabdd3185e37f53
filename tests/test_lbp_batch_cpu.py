"""The premises of tests/test_gpu_lbp_batch.py, asserted on the numpy statement alone (tests/lbp_reference.py): the slots of every batch
hold different, non-empty answers (so a slot mix-up changes a list), the overflow batch lies where the two candidate capacities need
it, and the rolled column image answers as derived by hand."""
import numpy as np
import pytest

import lbp_batch_cases as B
import lbp_cases as K
import lbp_reference as R
from nubovca import synth


def _pairwise_different(lists):
    keys = [l.tobytes() for l in lists]
    return len(set(keys)) == len(keys)


@pytest.mark.parametrize("case", B.BATCHES, ids=B.BATCH_IDS)
def test_slots_of_a_batch_answer_differently(case):
    name, cols, rows, sf, n = case
    imgs = B.images(name, cols, rows, n)
    assert all(not np.array_equal(imgs[i], imgs[k]) for i in range(n) for k in range(i))
    exp = B.expected_batch(name, cols, rows, sf, n)
    assert all(len(e) > 0 for e in exp) and _pairwise_different(exp), [len(e) for e in exp]
    # reversing the slots therefore reverses a different answer
    assert n < 2 or not np.array_equal(exp[0], exp[-1])


def test_w24_seeds_on_the_smallest_image():
    exp = [B.expected("w24", 97, 83, 1.1, s) for s in (11, 12, 13, 14)]
    assert _pairwise_different(exp) and all(len(e) >= 20 for e in exp), [len(e) for e in exp]


def test_the_stage_heavy_batch_is_thin():
    """20 stages and a handful of candidates an image: the late stage groups run on a few windows of five images together"""
    assert len(K.cascade("deep")[1].stage_sizes) == 20
    counts = [len(e) for e in B.expected_batch("deep", 160, 120, 1.2, 5)]
    assert all(1 <= c <= 40 for c in counts), counts


def test_the_wide_batch_has_levels_beyond_one_launch():
    """levels wider than 1023 columns are resized and integrated level by level: those launches carry both images"""
    widths = [sz[0] for _, sz, _ in R.levels(24, 24, 1500, 240, 1.3)]
    assert widths[0] > 1023 and widths[-1] <= 1023, widths


def test_boundary_batch_of_33():
    name, cols, rows, sf = B.BOUNDARY
    exp = B.expected_batch(name, cols, rows, sf, 33, B.BOUNDARY_SEED0)
    assert all(len(e) > 0 for e in exp) and _pairwise_different(exp), [len(e) for e in exp]
    # the image behind the job boundary (slot 32) differs from the first of either job
    assert not np.array_equal(exp[32], exp[0]) and not np.array_equal(exp[32], exp[31])


def test_overflow_batch_lies_between_the_capacities():
    nat, flat, ramp = (len(e) for e in B.code255_expected())
    assert flat > 4096 and 0 < nat < 1024 and 0 < ramp < 1024 and len({nat, flat, ramp}) == 3
    total = nat + flat + ramp
    assert total > 1024 * 3          # capacity 1024 an image: the job's list overflows, the launch set runs again
    assert total < 4096 * 3          # capacity 4096: no re-run, although one image alone holds more than 4096


@pytest.mark.parametrize("case", K.skip_cases(), ids=[c[0] for c in K.skip_cases()])
def test_rolled_column_image_by_hand(case):
    cid, cdict, exp_plain = case
    ref = R.parse_xml(synth.lbp_cascade_to_xml(cdict))
    assert R.scan(ref, K.column_image(), 4.0).tolist() == exp_plain
    assert R.scan(ref, B.rolled_column_image(), 4.0).tolist() == B.ROLLED_EXPECTED[cid]
    assert B.ROLLED_EXPECTED[cid] != exp_plain
