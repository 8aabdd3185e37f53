"""The 4:2:0 conversion statement (tests/yuv_reference.py) on the CPU: the hand-derived answers, the vectorised
statement against a scalar loop over the buffer's bytes, and the oracle's view of the frames the GPU tests use (so that those
cannot pass on empty outputs)."""
import numpy as np
import pytest

import yuv_cases as Y
import yuv_reference as R
from nubovca import synth


def _one_pixel(yv, u, v, fmt):
    if fmt == R.NV12:
        buf = np.array([yv] * 4 + [u, v], np.uint8)
        lay = (R.NV12, (0, 4), (2, 2))
    else:
        buf = np.array([yv] * 4 + [u] + [v], np.uint8)
        lay = (R.I420, (0, 4, 5), (2, 1, 1))
    return R.bgr(buf, 2, 2, lay), R.bgr_scalar(buf, 2, 2, lay)


@pytest.mark.parametrize("fmt", [R.NV12, R.I420])
@pytest.mark.parametrize("yuv,bgr", [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (0, 0, 254))])
def test_known_answers(yuv, bgr, fmt):
    """(81, 90, 240): G and B shift to -1 (an arithmetic shift of a negative sum) and clamp to 0"""
    a, b = _one_pixel(*yuv, fmt)
    assert (a == np.array(bgr, np.uint8)).all() and (b == a).all(), (a.tolist(), b.tolist())


def test_red_shifts_to_minus_one_before_the_clamp():
    yp = max(0, 81 - 16) * R.CY + (1 << 19)
    assert (yp + R.CUB * (90 - 128)) >> 20 == -1 and (yp + R.CVG * (240 - 128) + R.CUG * (90 - 128)) >> 20 == -1
    assert (yp + R.CVR * (240 - 128)) >> 20 == 254


@pytest.mark.parametrize("fmt", [R.NV12, R.I420])
@pytest.mark.parametrize("pad,rows,gap", [(0, None, 0), (6, 20, 10)])
def test_statement_against_scalar_loop(fmt, pad, rows, gap):
    """every byte value in every plane (a random image with the extremes forced in), padded strides, padded luma height, gaps"""
    w, h = 34, 18
    rng = np.random.default_rng(11 + fmt)
    _, lay = synth.make_yuv420(w, h, 5, fmt, "noise", pad=pad, luma_rows=rows, gap=gap)
    n = max(o + s * (h if p == 0 else h // 2) for p, (o, s) in enumerate(zip(lay[1], lay[2])))
    buf = rng.integers(0, 256, size=n).astype(np.uint8)
    buf[lay[1][0]:lay[1][0] + 4] = [0, 255, 16, 235]
    got, exp = R.bgr(buf, w, h, lay), R.bgr_scalar(buf, w, h, lay)
    assert np.array_equal(got, exp)
    assert got.min() == 0 and got.max() == 255


@pytest.mark.parametrize("fmt", [R.NV12, R.I420])
def test_make_yuv420_layouts(fmt):
    """the two formats of one seed hold the same samples; padding and gaps move them without changing them"""
    w, h = 64, 36
    a = synth.make_yuv420(w, h, 9, fmt, "natural", [(10, 6, 24)])
    b = synth.make_yuv420(w, h, 9, fmt, "natural", [(10, 6, 24)], pad=32, luma_rows=48, gap=128)
    c = synth.make_yuv420(w, h, 9, 3 - fmt, "natural", [(10, 6, 24)])
    pa, pb, pc = R.planes(a[0], w, h, a[1]), R.planes(b[0], w, h, b[1]), R.planes(c[0], w, h, c[1])
    for k in range(3):
        assert np.array_equal(pa[k], pb[k]) and np.array_equal(pa[k], pc[k])
    assert pa[0].min() >= 16 and pa[0].max() <= 235 and abs(int(pa[1].astype(int).mean()) - 128) <= 2
    assert b[1][2][0] == w + 32 and b[1][1][1] == (w + 32) * 48 + 128


@pytest.mark.parametrize("fset,n", [("sd", 9), ("p720", 8), ("tail", 8), ("s5", 6), ("hd160", 6)])
def test_oracle_finds_faces_in_the_stream_sequences(fset, n):
    exp = Y.sequence_expected("synthetic", fset, n)
    with_boxes = [i for i, (b, _) in enumerate(exp) if len(b)]
    assert len(with_boxes) >= n // 2, [len(b) for b, _ in exp]
    assert any(not Y.has_faces(fset, i) for i in range(n))


def test_oracle_finds_faces_in_the_1080p_sequence():
    exp = Y.sequence_expected("synthetic", "hd", 8)
    assert sum(1 for b, _ in exp if len(b)) >= 4, [len(b) for b, _ in exp]
    assert not Y.has_faces("hd", 3)


def test_oracle_raw_lists_of_the_1080p_batch_are_not_empty():
    """three of the 32 frames of the raw-list test with faces in them (the GPU test asks the same of the whole batch)"""
    for i in (0, 9, 17):
        assert Y.has_faces("hd", i) and len(Y.raw_expected("calibrated", 0, "hd", i)) >= 40, i
