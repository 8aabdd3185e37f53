"""Face and part streams on new-format HAAR cascades: the frames and the expected answers of tests/test_gpu_haar_new_streams.py, put
together the way tests/lbp_stream_cases.py and tests/lbp_part_cases.py put theirs together.  A face stream's expected sequence is the
oracle's gate and finish (orc_face_stream_gate / orc_face_stream_finish) around the numpy statement's detections
(tests/haar_new_reference.py) on orc.equalize_hist(orc.bgr2gray(orc.resize_linear(bgr, cols, rows))) with minSize (cols // 20,
rows // 20); a part stream's is the elements' own per-frame logic (lbp_part_cases.Harness) around one detector per role."""
import ctypes as C
import functools

import numpy as np

import haar_new_cases as K
import haar_new_reference as R
import lbp_part_cases as LP
import lbp_stream_cases as LS
import orc
import yuv_reference as Y

# (cascade, frame width, height, width_to_process, scale_factor_pct, seeds)
CASES = {
    "identity": ("w24", 160, 120, 160, 25, (11, 12, 13)),
    "half": ("w20x28", 320, 240, 160, 10, (11, 12, 13)),          # exact 2x in front of the LUT tap; a window that is not square
}


def frames_of(case):
    name, W, H, _wtp, _pct, seeds = case
    return [("hnew", name, W, H, s) for s in seeds]


@functools.lru_cache(maxsize=None)
def gray(frame):
    _, name, W, H, seed = frame
    g = np.array(K.image(W, H, *K.cascade(name)[1].size, seed), np.uint8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def yuv(frame, fmt):
    """(buffer, layout tuple) of the 4:2:0 frame whose luma plane is gray(frame) and whose chroma is neutral"""
    import yuv_stream_scenes as S
    g = gray(frame)
    c = np.full((g.shape[0] // 2, g.shape[1] // 2), 128, np.uint8)
    return S.pack_planes(g, c, c, fmt)


@functools.lru_cache(maxsize=None)
def bgr(frame, fmt=0):
    if fmt:
        buf, lay = yuv(frame, fmt)
        out = Y.bgr(buf, gray(frame).shape[1], gray(frame).shape[0], lay)
    else:
        out = np.ascontiguousarray(np.dstack([gray(frame)] * 3))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def raw(casc, frame, wtp, pct, fmt=0):
    """the raw list of an analysed frame: the statement on the equalised working image (FACE/kmsfacedetect.cpp:805-811)"""
    img = bgr(frame, fmt)
    cols, rows, _ = LS.geometry(img.shape[1], img.shape[0], wtp)
    w = orc.equalize_hist(orc.bgr2gray(orc.resize_linear(np.array(img), cols, rows)))
    out = R.scan(K.cascade(casc)[1], w, 1 + pct / 100, (cols // 20, rows // 20))
    out.setflags(write=False)
    return out


def detections(casc, frame, wtp, pct, mn, fmt=0):
    r = raw(casc, frame, wtp, pct, fmt)
    if mn == 0 or len(r) == 0:
        return np.array(r)
    return np.asarray(orc.group_rectangles(np.array(r), max(mn, 1), 0.2)[0], np.int32).reshape(-1, 4)


class Expected:
    """the expected stream: the oracle's gate and finish around the statement's detections (lbp_stream_cases.Expected with this file's detections)"""

    def __init__(self, casc, fmt=0, **params):
        self.casc, self.fmt = casc, fmt
        self.p = dict(width_to_process=160, scale_factor_pct=25, min_neighbors=3)
        self.p.update(params)
        self.s = orc.FaceStream(LS._any_haar(), **{k: v for k, v in self.p.items() if k not in ("scale_factor_pct", "min_neighbors")})

    def process(self, frame, cap=1024):
        H, W = gray(frame).shape
        L = orc.lib()
        analysed = L.orc_face_stream_gate(self.s.h)
        det = np.zeros((0, 4), np.int32)
        if analysed:
            det = detections(self.casc, frame, self.p["width_to_process"], self.p["scale_factor_pct"], self.p["min_neighbors"], self.fmt)
        assert len(det) <= LS.ORC_MAX_FACES
        buf, ids = (orc.Rect * cap)(), (C.c_int * cap)()
        n = L.orc_face_stream_finish(self.s.h, analysed, orc.np_to_rects(det), len(det), W, H, buf, ids, cap)
        return orc.rects_to_np(buf, n), np.array(ids[:n], dtype=np.int32)


# ------------------------------------------------------------------ part streams whose three roles are of three formats
# kind -> (face, a, b) as (format, cascade name) on lbp_part_cases.lbp_frames(320, 240).  "eye": the face pass on the new-format HAAR cascade,
# the eye searches (regions of about 32 x 22 pixels: every role runs, little is found) on an LBP and an old-format cascade; "ear": the
# new-format HAAR cascade in a part role, on regions larger than its window, where both lists fill
PART_W, PART_H = 320, 240
PART_ROLES = {
    "eye": (("hnew", "w24"), ("lbp", LP.PART_A), ("haar", "lefteye")),
    "ear": (("lbp", LP.FACE), ("haar", "leftear"), ("hnew", "w20x28")),
}


def hnew_detector(ref):
    """a new-format HAAR role: detectMultiScale on a new-format file -- flags ignored, groupRectangles(max(mn, 1), 0.2)"""
    return LP.Detector(lambda g, sf, mn, flags, mins, maxs: R.detect(ref, g, sf, mn, mins, maxs))


def part_frames():
    return LP.lbp_frames(PART_W, PART_H)


def part_xml(role):
    fmt, name = role
    return {"hnew": lambda: K.cascade(name)[0], "lbp": lambda: LP.K.cascade(name)[0], "haar": lambda: LP.haar_xml()[name]}[fmt]()


@functools.lru_cache(maxsize=None)
def part_expected(kind):
    """([(list a, list b)] per frame, the three detectors with the sizes they saw)"""
    def make(role):
        fmt, name = role
        return hnew_detector(K.cascade(name)[1]) if fmt == "hnew" else LP.lbp_detector(LP.K.cascade(name)[1]) if fmt == "lbp" else LP.haar_detector(LP._haar_cpu()[name])
    dets = tuple(make(r) for r in PART_ROLES[kind])
    h = LP.Harness(kind, *dets)
    out = [h.process(f) for f in part_frames()]
    h.close()
    return out, dets
