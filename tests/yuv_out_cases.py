"""The case table of the drawing calls on 4:2:0 frames, shared by tests/test_yuv_out_cpu.py (host loops through the ABI),
tests/test_yuv_out_san_cpu.py (the same loops under the sanitizers) and tests/test_gpu_yuv_out.py (device frames): frames, layouts,
shape lists and overlay set-ups, all built by construction.  Frames are 64 x 48 -- several chroma blocks a side, small enough for
the statement's long way round -- with every plane byte random over the whole value range and 0xA5 in everything no sample lies in."""
import functools

import numpy as np

import yuv_out_reference as S
from nubovca import synth

W, H = 64, 48
FMTS = [S.NV12, S.I420]
FMT_IDS = ["nv12", "i420"]
# name -> make_yuv420's layout arguments: tight planes; padded rows (odd paddings: nothing stays aligned); more allocated rows than
# the frame has (1080 in 1088, here 48 in 56) with a gap between the planes
LAYOUTS = {"tight": dict(), "padded": dict(pad=7, chroma_pad=3), "rows": dict(pad=16, luma_rows=H + 8, gap=24)}
SENTINEL = 0xA5
FACE = (255, 128, 0, 255)          # FACE/BaseFace.cpp:76-80


def layout_of(w, h, fmt, **kw):
    _, lay = synth.make_yuv420(w, h, 1, fmt, "flat", **kw)
    return (lay[0], tuple(lay[1]), tuple(lay[2]))


def random_frame(w, h, fmt, seed, tail=0, **kw):
    """(buffer, layout): every sample random, 0xA5 wherever no sample lies (row padding, gaps, unused rows, `tail` bytes behind)"""
    buf, lay = synth.make_yuv420(w, h, 1, fmt, "flat", **kw)
    lay = (lay[0], tuple(lay[1]), tuple(lay[2]))
    buf = np.concatenate([np.full(len(buf), SENTINEL, np.uint8), np.full(tail, SENTINEL, np.uint8)])
    rng = np.random.default_rng(seed)
    S.write(buf, w, h, lay, rng.integers(0, 256, (h, w)).astype(np.uint8), rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint8),
            rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint8))
    return buf, lay


@functools.lru_cache(maxsize=None)
def frame(fmt, layout):
    buf, lay = random_frame(W, H, fmt, 77 + fmt + len(layout), tail=5, **LAYOUTS[layout])
    buf.setflags(write=False)
    return buf, lay


def sample_mask(n, w, h, lay):
    """which bytes of an n-byte buffer are samples of the frame"""
    m = np.zeros(n, np.uint8)
    S.write(m, w, h, lay, np.ones((h, w), np.uint8), np.ones((h // 2, w // 2), np.uint8), np.ones((h // 2, w // 2), np.uint8))
    return m == 1


def _col(i):
    rng = np.random.default_rng(900 + i)
    return tuple(int(v) for v in rng.integers(0, 256, 4))


# name -> shapes (kind, x, y, w, h, bgra)
DRAW = {
    # corners at all four (x, y) parities, sizes even and odd
    "parity_ee": [(0, 10, 8, 20, 16, _col(0))], "parity_oe": [(0, 11, 8, 21, 16, _col(1))],
    "parity_eo": [(0, 10, 9, 20, 17, _col(2))], "parity_oo": [(0, 11, 9, 21, 17, _col(3))],
    "left_edge": [(0, -5, 10, 20, 12, _col(4))], "right_edge": [(0, 50, 10, 30, 12, _col(5))],
    "top_edge": [(0, 10, -6, 20, 14, _col(6))], "bottom_edge": [(0, 10, 40, 20, 20, _col(7))],
    "outside": [(0, 100, 100, 10, 10, _col(8)), (0, -50, -50, 10, 10, _col(9)), (1, -40, 20, 10, 0, _col(10))],
    "ring": [(1, 30, 24, 10, 0, _col(11))], "ring_over_edge": [(1, 3, 45, 9, 0, _col(12)), (1, 61, 1, 1, 0, _col(13))],
    "overlap": [(0, 8, 6, 30, 20, FACE), (0, 9, 7, 30, 20, _col(14)), (1, 38, 26, 7, 0, _col(15)), (0, 20, 3, -12, 40, (0, 0, 255, 0))],
    "negative_size": [(0, 40, 30, -21, -13, _col(16))],
    "whole_frame": [(0, 1, 1, W - 3, H - 3, FACE)],
    "none": [],
}


def _image(cn, w, h, seed, zeros=False):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn)).astype(np.uint8)
    if cn == 4 and zeros:          # an alpha plane with runs of zeros, full weights and everything between
        a = img[:, :, 3]
        a[:, : w // 3] = 0
        a[h // 2, :] = 0
        a[: h // 4, w // 2:] = 255
    return img


# name -> (boxes, image, offset_x, offset_y, width_percent, height_percent)
OVERLAY = {}
for _cn in (1, 3, 4):
    OVERLAY["identity_c%d" % _cn] = ([(7, 5, 12, 10)], _image(_cn, 12, 10, 10 + _cn, True), 0.0, 0.0, 1.0, 1.0)          # odd offsets
    OVERLAY["half_c%d" % _cn] = ([(21, 9, 12, 10)], _image(_cn, 24, 20, 20 + _cn, True), 0.0, 0.0, 1.0, 1.0)            # exact 2 x
    OVERLAY["bilinear_c%d" % _cn] = ([(10, 4, 34, 26)], _image(_cn, 12, 10, 30 + _cn, True), 0.1, 0.2, 0.5, 0.5)         # 17 x 13
OVERLAY["overlapping_boxes"] = ([(4, 4, 20, 16), (13, 9, 21, 17), (12, 11, 20, 16)], _image(4, 9, 7, 41), 0.0, 0.0, 1.0, 1.0)
OVERLAY["partly_outside"] = ([(-6, -3, 16, 12), (55, 41, 16, 12), (30, -20, 8, 8)], _image(4, 8, 6, 42), 0.0, 0.0, 1.0, 1.0)
OVERLAY["alpha_zeros"] = ([(1, 1, 40, 30)], _image(4, 20, 15, 43, True), 0.0, 0.0, 1.0, 1.0)
OVERLAY["negative_offset"] = ([(30, 20, 16, 12)], _image(3, 8, 6, 44), -0.5, -0.25, 1.5, 1.25)
OVERLAY["width_zero"] = ([(4, 4, 20, 16)], _image(3, 8, 6, 45), 0.0, 0.0, 0.0, 1.0)
OVERLAY["no_boxes"] = ([], _image(3, 8, 6, 46), 0.0, 0.0, 1.0, 1.0)


@functools.lru_cache(maxsize=None)
def draw_expected(name, fmt, layout):
    buf, lay = frame(fmt, layout)
    out = S.draw(buf, W, H, lay, DRAW[name])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def overlay_expected(name, fmt, layout):
    buf, lay = frame(fmt, layout)
    out = S.overlay(buf, W, H, lay, *OVERLAY[name])
    out.setflags(write=False)
    return out
