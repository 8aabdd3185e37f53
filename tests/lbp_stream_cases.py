"""Face streams on new-format LBP cascades (nvca_face_stream_create_any): the frames, the streams' parameters and the expected answers
that tests/test_lbp_streams_cpu.py (on the statement alone) and tests/test_gpu_lbp_streams.py (on the device) share.

The expected stream is put together from parts that exist: orc.FaceStream on any Haar cascade supplies the frame gate and everything
behind the detections (orc_face_stream_gate / orc_face_stream_finish: track_faces, the no-detection hysteresis, the box scaling), and an
analysed frame's detections between the two are tests/lbp_reference.py's detectMultiScale on
orc.equalize_hist(orc.bgr2gray(orc.resize_linear(bgr, cols, rows))) with minSize (cols // 20, rows // 20) -- FACE/kmsfacedetect.cpp:805-811
with a new-format cascade behind cv::CascadeClassifier.  A frame's raw list is computed once (lru_cache) whatever min_neighbors groups it."""
import ctypes as C
import functools

import numpy as np

import lbp_batch_cases as B
import lbp_cases as K
import lbp_reference as R
import orc
import yuv_reference as Y
from nubovca import synth

# ---- the cases: (cascade, frame width, height, width_to_process, scale_factor_pct, seeds).  The smallest shapes at which each piece can go
# wrong; what each one reaches is asserted on the statement by tests/test_lbp_streams_cpu.py
CASES = {
    "identity": ("w24", 160, 120, 160, 25, (11, 12, 13)),          # rank-sort branch of k_group, one bit word a row
    "half": ("w24", 320, 240, 160, 25, (11, 12, 13)),              # exact 2x: cv::resize's area shortcut in front of the LUT tap
    "bilinear": ("w24", 640, 480, 160, 25, (11, 12, 13, 14, 15, 16)),   # two empty analysed frames in a row: hysteresis, faces.clear()
    "bitonic": ("w20x28", 160, 120, 160, 10, (11, 12, 13)),        # more than 256 candidates; a window that is not square
    "odd": ("w24", 333, 251, 333, 25, (11, 12, 13)),               # odd pitch, several bit words a row
    "wide": ("w24", 1500, 240, 1500, 30, (11, 12, 13)),            # a frame wider than 1023 (its scanned levels are not: see WIN78)
    "deep": ("deep", 160, 120, 160, 25, (11, 12, 13)),             # 20 stages
}
MANY = ("w12", 64, 48, 64, 25, tuple(range(100, 133)))              # 33 streams in one call: more images than one job takes
FLAT = ("flat", 160, 120, 120)                                      # a frame of one value: no candidate under w24
NATURAL = (("natural", 160, 120, 5), ("natural", 160, 120, 7))      # no template: candidates, none kept
# levels wider than 1023 under the stream's minSize need a window above 51 pixels (a scanned level is at most 20 windows wide, so the
# 24 x 24 window's "wide" case never has one): a 78 x 78 window that passes where its 26 x 26 cells give code 255 and its 13 x 13 cells
# code 0, on natural fields 1500 wide -- the per-level resize through the LUT, more than one image
WIN78 = ("win78", 1500, 240, 1500, 30, (5, 7))
CODE255 = "code255"                                                 # lbp_batch_cases.code255_cascade(): passes wherever every neighbour cell >= the centre


def frames_of(case):
    name, W, H, _wtp, _pct, seeds = case
    if name == "win78":
        return [("natural", W, H, s) for s in seeds]
    return [("lbp", name, W, H, s) for s in seeds]


@functools.lru_cache(maxsize=None)
def cascade(key):
    """(xml text, the reference reader's cascade)"""
    if key == CODE255:
        xml = synth.lbp_cascade_to_xml(B.code255_cascade())
        return xml, R.parse_xml(xml)
    if key == "win78":
        xml = synth.lbp_cascade_to_xml(K.hand_cascade((78, 78), [(0, 0, 26, 26), (0, 0, 13, 13)],
                                                      [(1.5, [(0, K.only_codes([255]), (1.0, 0.0)), (1, K.only_codes([0]), (1.0, 0.0))])]))
        return xml, R.parse_xml(xml)
    return K.cascade(key)


@functools.lru_cache(maxsize=None)
def gray(frame):
    """the gray image a frame key stands for; read-only"""
    kind = frame[0]
    if kind == "lbp":
        _, name, W, H, seed = frame
        g = K.image(W, H, *K.cascade(name)[1].size, seed)
    elif kind == "flat":
        g = np.full((frame[2], frame[1]), frame[3], np.uint8)
    elif kind == "natural":
        g = synth.make_gray(frame[1], frame[2], frame[3], "natural")
    elif kind == "ramp":
        y, x = np.mgrid[0:frame[2], 0:frame[1]]
        g = ((x + 2 * y) % 251).astype(np.uint8)
    else:
        raise KeyError(frame)
    g = np.array(g, np.uint8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def yuv(frame, fmt):
    """(buffer, layout tuple) of the 4:2:0 frame whose luma plane is gray(frame) and whose chroma is neutral; read-only"""
    import yuv_stream_scenes as S
    g = gray(frame)
    c = np.full((g.shape[0] // 2, g.shape[1] // 2), 128, np.uint8)
    return S.pack_planes(g, c, c, fmt)


@functools.lru_cache(maxsize=None)
def bgr(frame, fmt=0):
    """the frame as the stream's BGR image: the gray image on three channels (bgr2gray returns it unchanged), or the statement's
    conversion of its 4:2:0 form (tests/yuv_reference.py)"""
    if fmt:
        buf, lay = yuv(frame, fmt)
        out = Y.bgr(buf, gray(frame).shape[1], gray(frame).shape[0], lay)
    else:
        out = np.ascontiguousarray(np.dstack([gray(frame)] * 3))
    out.setflags(write=False)
    return out


def geometry(W, H, wtp):
    """(cols, rows, norm_scale) as face_submit computes them (kms_face_detect_conf_images :304, process_frame :770-783)"""
    assert W >= wtp > 0
    norm = W // wtp
    scale = float(np.float32(W // wtp))                  # the INTEGER ratio kept in a float
    cols, rows = W, H
    if R.cv_round(H / scale) > 0:
        rows = R.cv_round(H / scale)
    else:
        scale = 1.0
    if R.cv_round(W / scale) > 0:
        cols = R.cv_round(W / scale)
    return cols, rows, norm


@functools.lru_cache(maxsize=None)
def working(frame, wtp, fmt=0, equalise=True):
    """the image detectMultiScale sees: resize, BGR2GRAY, equalizeHist (:805-807)"""
    img = bgr(frame, fmt)
    cols, rows, _ = geometry(img.shape[1], img.shape[0], wtp)
    g = orc.bgr2gray(orc.resize_linear(np.array(img), cols, rows))
    return orc.equalize_hist(g) if equalise else g


@functools.lru_cache(maxsize=None)
def raw(casc, frame, wtp, pct, fmt=0, equalise=True):
    """the raw list of an analysed frame, (level, y, x) order"""
    w = working(frame, wtp, fmt, equalise)
    rows, cols = w.shape
    out = R.scan(cascade(casc)[1], w, 1 + pct / 100, (cols // 20, rows // 20))
    out.setflags(write=False)
    return out


def detections(casc, frame, wtp, pct, mn, fmt=0):
    r = raw(casc, frame, wtp, pct, fmt)
    if mn == 0 or len(r) == 0:
        return np.array(r)
    return np.asarray(orc.group_rectangles(np.array(r), max(mn, 1), 0.2)[0], np.int32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def _any_haar():
    return orc.parse_cascade_xml(synth.synthetic_cascade_xml())


ORC_MAX_FACES = 256            # oracle/orc_pipe.c


class Expected:
    """the expected LBP stream: the oracle's gate and finish around the statement's detections.  Properties by their FaceParams names;
    scale_factor_pct and min_neighbors may be changed between frames (they reach the detections only)."""

    def __init__(self, casc, fmt=0, **params):
        self.casc, self.fmt = casc, fmt
        self.p = dict(width_to_process=160, scale_factor_pct=25, min_neighbors=3)
        self.p.update(params)
        self.s = orc.FaceStream(_any_haar(), **{k: v for k, v in self.p.items() if k not in ("scale_factor_pct", "min_neighbors")})

    def process(self, frame, cap=1024):
        H, W = gray(frame).shape
        L = orc.lib()
        analysed = L.orc_face_stream_gate(self.s.h)
        det = np.zeros((0, 4), np.int32)
        if analysed:
            det = detections(self.casc, frame, self.p["width_to_process"], self.p["scale_factor_pct"], self.p["min_neighbors"], self.fmt)
        assert len(det) <= ORC_MAX_FACES, "the oracle's stream tracks at most %d faces: a longer list has no expected answer" % ORC_MAX_FACES
        buf, ids = (orc.Rect * cap)(), (C.c_int * cap)()
        n = L.orc_face_stream_finish(self.s.h, analysed, orc.np_to_rects(det), len(det), W, H, buf, ids, cap)
        return orc.rects_to_np(buf, n), np.array(ids[:n], dtype=np.int32)


def expected_sequence(casc, frames, fmt=0, **params):
    e = Expected(casc, fmt, **params)
    return [e.process(f) for f in frames]
