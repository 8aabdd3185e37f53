"""The packed 4:2:2 frames and case lists of tests/test_yuv422_cpu.py, tests/test_yuv422_layout_san_cpu.py and tests/test_gpu_yuv422.py,
and what the oracle expects of them.  Two kinds of frames:
  * the 4:2:0 scenes of tests/yuv_cases.py and tests/yuv_stream_scenes.py re-packed as 4:2:2 by repeating every chroma row -- they convert
    to A.13's image exactly (premise (c), tests/test_yuv422_cpu.py), so the existing oracle sequences are their expectations;
  * frames of nubovca.synth.make_yuv422, whose chroma differs from row to row: the image of a reader that shares chroma between rows
    2k and 2k + 1 differs (premise (a)); their expectations are oracle streams of their own fed the statement's image.
Also the two wide-kernel predicates as the tests state them (the C++: yuv_layout_aligned16 + frames_yuv_aligned16, trk_wide_ok), and the
case lists on both sides of every term of them."""
import functools

import numpy as np

import prefix_cascades as P
import yuv_cases as Y
import yuv_reference as R420
import yuv422_reference as R
import yuv_stream_scenes as S
from nubovca import synth

GRAY_WIDE, GRAY_GENERIC = "k_gray_yuv422_16", "k_gray_yuv422_generic"
TRK_WIDE, TRK_GENERIC = "k_trk_pixel_yuv422x4", "k_trk_pixel_yuv422"


def _tuple(lay):
    return (lay[0], tuple(lay[1]), tuple(lay[2]))


# ---------------------------------------------------------------- the predicates, stated here
def gray_wide(lay, identity, mem, ptr):
    """k_gray_yuv422_16 runs: identity geometry, offset[0] and stride[0] on 16 bytes, a device frame's pointer on 16 bytes (a host frame is
    staged on 256 bytes).  Four terms."""
    return bool(identity and lay[1][0] % 16 == 0 and lay[2][0] % 16 == 0 and (mem == "host" or ptr % 16 == 0))


def trk_wide(lay, w, mem, ptr):
    """k_trk_pixel_yuv422x4 runs: w % 4 == 0, the plane's first byte (pointer + offset[0]; a host frame counts as pointer 0) and stride[0]
    on 8 bytes.  Three terms."""
    return bool(w % 4 == 0 and ((0 if mem == "host" else ptr) + lay[1][0]) % 8 == 0 and lay[2][0] % 8 == 0)


# ---------------------------------------------------------------- face frames
@functools.lru_cache(maxsize=256)
def frame(fset, i, fmt, pad=0, base=0):
    """(buffer, layout tuple) of frame i of tests/yuv_cases.py's set, re-packed; read-only"""
    W, H = Y.SETS[fset][:2]
    buf420, lay420 = Y.frame(fset, i, R420.NV12)
    buf, lay = R.from_420(buf420, W, H, lay420, fmt, pad=pad, base=base, seed=i)
    buf.setflags(write=False)
    return buf, lay


# (set, pad, base offset of the layout, bytes the device pointer is shifted by, memory) of the full-resolution / shrinking face cases: both
# sides of each of gray_wide's four terms.  "tail" is 328 x 250: rows of 656 bytes (a multiple of 16) that end in a unit of 8 pixels.
FACE_KERNEL_CASES = [
    ("tail", 0, 0, 0, "device"),        # every term holds: wide, with a short unit at the end of every row
    ("tail", 0, 0, 0, "host"),
    ("tail", 4, 0, 0, "device"),        # stride 660
    ("tail", 16, 0, 0, "device"),       # stride 672: wide again
    ("tail", 0, 8, 0, "device"),        # offset 8
    ("tail", 0, 16, 0, "host"),         # offset 16: wide
    ("tail", 0, 0, 4, "device"),        # pointer 4 off
    ("tail", 0, 0, 16, "device"),       # pointer 16 off: wide
    ("tail", 0, 8, 8, "device"),        # pointer + offset on 16 bytes, neither of them: the terms are separate -- generic
    ("tail", 0, 0, 4, "host"),          # a host pointer's alignment does not count
    ("sd", 0, 0, 0, "device"),          # shrinking geometry
]


def face_kernel(case):
    fset, pad, base, shift, mem = case
    W, _, w2p = Y.SETS[fset][:3]
    return GRAY_WIDE if gray_wide(frame(fset, 0, R.YUY2, pad, base)[1], W == w2p, mem, shift) else GRAY_GENERIC


# a chroma-varying 1080p frame (make_yuv422): the shape the wide kernel is for
HD_FACES = P.FACES_1080


@functools.lru_cache(maxsize=8)
def hd_frame(fmt, i=0):
    buf, lay = synth.make_yuv422(1920, 1080, 6300 + i, fmt, "natural", HD_FACES)
    buf.setflags(write=False)
    return buf, _tuple(lay)


def hd_raw(img):
    """raw candidate list (scan order) of a fresh min_neighbors-0 oracle stream at full resolution on a BGR image, as
    tests/yuv_cases.py's raw_expected: grouped boxes would hide single windows -- and with them gray values that are off by one"""
    import orc
    kw = dict(width_to_process=img.shape[1], scale_factor_pct=10, min_neighbors=0)
    boxes, ids = orc.FaceStream(P.oracle_cascade("calibrated", 0), **kw).process(np.array(img))
    if len(boxes) < P.ORC_MAX_FACES:
        assert np.array_equal(ids, np.arange(len(boxes)))
        return boxes
    out = orc.FaceStream(P.oracle_cascade("calibrated", 0), **kw).frame_detect(np.array(img), cap=1 << 17)
    assert P.ORC_MAX_FACES <= len(out) < (1 << 17) and np.array_equal(out[:P.ORC_MAX_FACES], boxes)
    return out


@functools.lru_cache(maxsize=8)
def hd_expected():
    """the raw list of the statement's image of hd_frame (the same image in any byte order)"""
    buf, lay = hd_frame(R.YUY2)
    return hd_raw(R.bgr(buf, 1920, 1080, lay))


# small chroma-varying frames for the premises and the primitive
@functools.lru_cache(maxsize=64)
def varying_frame(W, H, fmt, pad=0, base=0, seed=5):
    buf, lay = synth.make_yuv422(W, H, seed, fmt, "natural", pad=pad, base=base)
    buf.setflags(write=False)
    return buf, _tuple(lay)


# ---------------------------------------------------------------- primitive cases
PRIM_WIDTHS = [2, 14, 16, 18, 30, 32, 34]
PRIM_HEIGHTS = [1, 2, 3, 17]
# (pad, base): tight rows, rows padded to 4 and to 16 bytes, an odd stride; a base 1, 4 and 16 bytes off alignment
PRIM_LAYOUTS = [(0, 0), (4, 0), (16, 0), (3, 0), (0, 1), (0, 4), (0, 16), (5, 1)]
PRIM_CASES = [(w, h, pad, base) for w in PRIM_WIDTHS for h in PRIM_HEIGHTS for (pad, base) in [PRIM_LAYOUTS[(w + h) % len(PRIM_LAYOUTS)], PRIM_LAYOUTS[(w // 2 + 3 * h + 1) % len(PRIM_LAYOUTS)]]]
PRIM_CASES += [(34, 200, pad, base) for pad, base in PRIM_LAYOUTS] + [(2, 1, 0, 0), (2, 1, 3, 1)]


def random_frame(w, h, fmt, pad, base, seed):
    """every byte random (the whole value range, clamps on both sides included); the padding and the bytes in front of the base too"""
    stride = 2 * w + pad
    buf = np.random.default_rng(seed).integers(0, 256, size=base + stride * (h - 1) + 2 * w).astype(np.uint8)
    return buf, (fmt, (base, 0, 0), (stride, 0, 0))


# ---------------------------------------------------------------- part frames
@functools.lru_cache(maxsize=None)
def part_frame(W, H, i, fmt, pad=0, base=0):
    buf420, lay420 = S.part_frame(W, H, i, R420.NV12)
    buf, lay = R.from_420(buf420, W, H, lay420, fmt, pad=pad, base=base, seed=i)
    buf.setflags(write=False)
    return buf, lay


PART_GEOS = [(640, 480), (322, 242)]
PART_FRAMES = 5


# ---------------------------------------------------------------- tracker frames
def _trk_planes(W, H, i):
    """(Y [H, W], U [H, W/2], V [H, W/2]) of frame i: the scene of tests/yuv_stream_scenes.py of the even height H or H + 1 (its movers
    change the chroma only), every chroma row repeated, cut to H rows"""
    y, u, v = S._trk_planes(W, H + (H & 1))[i]
    return y[:H], np.repeat(u, 2, axis=0)[:H], np.repeat(v, 2, axis=0)[:H]


@functools.lru_cache(maxsize=None)
def trk_frame(W, H, i, fmt, pad=0, base=0):
    buf, lay = synth.pack_yuv422(*_trk_planes(W, H, i), fmt, pad=pad, base=base, seed=i)
    buf.setflags(write=False)
    return buf, _tuple(lay)


@functools.lru_cache(maxsize=None)
def trk_bgra(W, H, i):
    out = np.full((H, W, 4), 255, np.uint8)
    out[..., :3] = R.convert(*_trk_planes(W, H, i))
    out.setflags(write=False)
    return out


def trk_luma_bgra(W, H, i):
    """the frame as a kernel that takes Y for gray would see it"""
    out = np.full((H, W, 4), 255, np.uint8)
    out[..., :3] = _trk_planes(W, H, i)[0][..., None]
    return out


@functools.lru_cache(maxsize=None)
def trk_expected(W, H):
    if H % 2 == 0:
        return S.trk_expected(W, H)          # (premise (c): the same images)
    return S.oracle_tracker_run([trk_bgra(W, H, i) for i in range(S.TRK_FRAMES)])


# (W, H, pad, base offset, pointer shift, memory): both pixel kernels at 160 x 120, 644 x 482 and 160 x 121 (an odd height), the general one
# alone at 322 x 242 (w % 4 == 2); both sides of each of trk_wide's three terms
TRK_CASES = [
    (160, 120, 0, 0, 0, "device"), (160, 120, 0, 0, 0, "host"), (160, 120, 4, 0, 0, "device"),
    (322, 242, 0, 0, 0, "device"), (322, 242, 4, 0, 0, "host"),
    (644, 482, 0, 0, 0, "device"), (644, 482, 2, 0, 0, "device"), (644, 482, 8, 8, 0, "host"),
    (644, 482, 0, 4, 0, "device"), (644, 482, 0, 4, 4, "device"), (644, 482, 0, 0, 4, "device"), (644, 482, 0, 0, 4, "host"),
    (160, 121, 0, 0, 0, "device"), (160, 121, 2, 0, 0, "host"),
]


def trk_kernel(case):
    W, H, pad, base, shift, mem = case
    return TRK_WIDE if trk_wide(trk_frame(W, H, 0, R.UYVY, pad, base)[1], W, mem, shift) else TRK_GENERIC
