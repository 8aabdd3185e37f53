"""The 4:2:0 frames of tests/test_yuv_cpu.py and tests/test_gpu_yuv.py and what the oracle expects of them.  NV12 and I420 frames
of one (set, index) hold the same samples, so they convert to the same BGR image and share one expected result."""
import functools

import numpy as np

import prefix_cascades as P
import yuv_reference as R
from nubovca import synth

FACES_1080 = P.FACES_1080


def _sd(i):          # 640 x 480, analysed at width-to-process 160 (bilinear, shrink-first)
    return 4100 + i, [(120 + 12 * i, 100 + 4 * i, 240)] if i % 4 != 2 else []


def _p720(i):        # 1280 x 720 at 640 (exact 2 x)
    return 5200 + i, [(160 + 16 * i, 120, 240), (760 + 6 * i, 300, 160)] if i % 5 != 3 else []


def _hd(i):          # 1920 x 1080 at full resolution
    return 6300 + i, [(x + 8 * (i % 8), y, s) for (x, y, s) in FACES_1080] if i % 5 != 3 else []


def _tail(i):        # 328 x 250 at full resolution: 20 whole 16-pixel units and one of 8 pixels in every row WHERE the planes take the wide
                     # loads (a luma stride of 336, not the tight 328: tests/test_gpu_yuv.py::test_full_resolution_rows_that_end_in_a_short_unit)
    return 7400 + i, [(40 + 10 * i, 30 + 5 * i, 150)] if i % 3 != 1 else []


def _s5(i):          # 800 x 450 at 160: a shrink by 5, the source rows of the resize come at an odd period
    return 8500 + i, [(100 + 30 * i, 60 + 10 * i, 250)] if i % 4 != 1 else []


def _hd160(i):       # 1920 x 1080 at the default 160: a shrink by 12 (source rows 12 k + 5 and 12 k + 6)
    return 9600 + i, [(260 + 24 * i, 180, 720), (1150, 240 + 12 * i, 600)] if i % 4 != 2 else []


# name -> (W, H, width-to-process, content of frame i)
SETS = {"sd": (640, 480, 160, _sd), "p720": (1280, 720, 640, _p720), "hd": (1920, 1080, 1920, _hd), "tail": (328, 250, 328, _tail),
        "s5": (800, 450, 160, _s5), "hd160": (1920, 1080, 160, _hd160)}


def has_faces(fset, i):
    return len(SETS[fset][3](i)[1]) > 0


@functools.lru_cache(maxsize=256)
def frame(fset, i, fmt, pad=0, luma_rows=None, gap=0, chroma_pad=None):
    """(buffer, layout tuple) of frame i of the set; read-only"""
    W, H, _, content = SETS[fset]
    seed, faces = content(i)
    buf, lay = synth.make_yuv420(W, H, seed, fmt, "natural", faces, pad=pad, luma_rows=luma_rows, gap=gap, chroma_pad=chroma_pad)
    buf.setflags(write=False)
    return buf, (lay[0], tuple(lay[1]), tuple(lay[2]))


@functools.lru_cache(maxsize=256)
def frame_bgr(fset, i):
    """the statement's BGR image of frame i (the same for either format and any padding)"""
    W, H = SETS[fset][:2]
    out = R.bgr(*_args(fset, i))
    out.setflags(write=False)
    return out


def _args(fset, i):
    buf, lay = frame(fset, i, R.NV12)
    W, H = SETS[fset][:2]
    return buf, W, H, lay


def oracle_sequence(name, fset, n, **params):
    """[(boxes, ids)] of an oracle face stream fed the statement's BGR images of frames 0 .. n - 1"""
    import orc
    kw = dict(width_to_process=SETS[fset][2])
    kw.update(params)
    s = orc.FaceStream(P.oracle_cascade(name, 0), **kw)
    return [s.process(np.array(frame_bgr(fset, i))) for i in range(n)]


@functools.lru_cache(maxsize=None)
def sequence_expected(name, fset, n):
    return oracle_sequence(name, fset, n)


@functools.lru_cache(maxsize=None)
def raw_expected(name, k, fset, i):
    """raw candidate list (scan order) of a fresh min_neighbors-0 stream at full resolution, as prefix_cascades.raw_expected"""
    import orc
    f = np.array(frame_bgr(fset, i))
    kw = dict(width_to_process=f.shape[1], scale_factor_pct=10, min_neighbors=0)
    boxes, ids = orc.FaceStream(P.oracle_cascade(name, k), **kw).process(f)
    if len(boxes) < P.ORC_MAX_FACES:
        assert np.array_equal(ids, np.arange(len(boxes)))
        return boxes
    out = orc.FaceStream(P.oracle_cascade(name, k), **kw).frame_detect(f, cap=1 << 17)
    assert P.ORC_MAX_FACES <= len(out) < (1 << 17) and np.array_equal(out[:P.ORC_MAX_FACES], boxes)
    return out
