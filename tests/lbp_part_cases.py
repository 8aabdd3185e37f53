"""Part streams on new-format LBP cascades: the expected answer and the frames, shared by tests/test_lbp_parts_cpu.py and
tests/test_gpu_lbp_parts.py.  The oracle's part stream cannot take a detector of the caller's, so the expected lists are the project's own
per-frame logic (csrc/part_logic.cpp behind tests/part_logic_shim.cpp, loaded with ctypes) around detections of the caller's choice:
the numpy statement of the LBP scan (tests/lbp_reference.py) for an LBP role, the oracle's detectMultiScale for a Haar role.  The
working images are built with the oracle's primitives, in the order tests/san/parts_driver.cpp builds them.  The CPU test pins the
harness itself against orc.PartStream on Haar cascades."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import lbp_cases as K
import lbp_reference as R
import orc
from nubovca import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
KINDS = {"eye": 0, "nose": 1, "mouth": 2, "ear": 3}
PROPS = {"width_to_process": 320, "process_x_every_4": 4, "scale_factor_pct": 25, "detect_event": 0}
MAX_SEARCHES = 256


@functools.lru_cache(maxsize=None)
def shim():
    """tests/part_logic_shim.cpp as a plain shared library (no sanitizer, nothing preloaded); None where there is no clang++"""
    if not os.path.exists(CLANG):
        return None
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(ROOT, "tests", "san", "build", "part_logic_shim.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "part_logic_shim.cpp")] + [os.path.join(csrc, f) for f in ("part_logic.cpp", "host_logic.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        # (hidden visibility, function sections, unused ones dropped: host_logic.cpp's overlay blend calls into plan.cpp, which is not part of this library)
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-shared", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden", "-ffunction-sections", "-Wl,--gc-sections",
               "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(out)
    ip, dp, vp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p
    L.pls_new.restype = vp
    L.pls_new.argtypes = [C.c_int] * 5
    L.pls_free.argtypes = [vp]
    L.pls_push_faces.argtypes = [vp, ip, C.c_int]
    L.pls_scales.argtypes = [vp, C.c_int, C.c_int, ip]
    L.pls_gate.argtypes = [vp, ip, dp]
    L.pls_pass_rule.argtypes = [C.c_int, ip]
    L.pls_rois.argtypes = [vp, ip, C.c_int, ip, C.c_int, C.c_int, ip, dp]
    L.pls_finish.argtypes = [vp, ip, ip]
    L.pls_list.argtypes = [vp, C.c_int, ip, C.c_int]
    return L


def _ints(a):
    a = np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))
    return a, a.ctypes.data_as(C.POINTER(C.c_int))


class Detector:
    """detectMultiScale of one role: fn(gray, sf, min_neighbors, flags, min_size, max_size) -> [n, 4]; `seen` collects the image
    sizes it was called on"""

    def __init__(self, fn):
        self.fn, self.seen = fn, []

    def __call__(self, gray, sf, mn, flags, mins, maxs):
        gray = np.ascontiguousarray(gray)
        self.seen.append((gray.shape[1], gray.shape[0]))
        return np.asarray(self.fn(gray, sf, mn, flags, mins, maxs), np.int32).reshape(-1, 4)


def lbp_detector(ref):
    """an LBP role: cv::CascadeClassifier::detectMultiScale on a new-format file -- flags ignored, groupRectangles(max(mn, 1), 0.2)"""
    return Detector(lambda g, sf, mn, flags, mins, maxs: R.detect(ref, g, sf, mn, mins, maxs))


def haar_detector(casc):
    return Detector(lambda g, sf, mn, flags, mins, maxs: orc.detect_multiscale(casc, g, sf, mn, flags, mins, maxs))


class Harness:
    """one part stream: csrc/part_logic.cpp's state machine around the given detectors (face, a, b)"""

    def __init__(self, kind, face, a, b=None, **props):
        self.L = shim()
        p = dict(PROPS, **props)
        self.h = self.L.pls_new(KINDS[kind], p["width_to_process"], p["process_x_every_4"], p["scale_factor_pct"], p["detect_event"])
        self.det = (face, a, b)

    def close(self):
        if self.h:
            self.L.pls_free(self.h)
            self.h = None

    def push_faces(self, faces):
        a, p = _ints(faces)
        self.L.pls_push_faces(self.h, p, len(a) // 4)

    def _list(self, which):
        buf = (C.c_int * (4 * 256))()
        n = self.L.pls_list(self.h, which, buf, 256)
        return np.frombuffer(buf, np.int32)[:4 * n].reshape(-1, 4).copy()

    def process(self, bgr):
        L, h = self.L, self.h
        H, W = bgr.shape[:2]
        sizes = (C.c_int * 4)()
        assert L.pls_scales(h, W, H, sizes), "frame too small"
        fw, fh, pw, ph = sizes
        f, sf = (C.c_int * 8)(), C.c_double()
        L.pls_gate(h, f, C.byref(sf))
        _early, run, _popped, eye_chain, face_image, face_post_eq, mirror, npass = f
        nsearch, out, sfs = 0, (C.c_int * (11 * MAX_SEARCHES))(), (C.c_double * MAX_SEARCHES)()
        found, counts = [], []
        if run:
            gray = orc.bgr2gray(bgr)
            if eye_chain:
                gray = orc.equalize_hist(gray)
            faces, faces_m = None, None
            if face_image:
                small = orc.resize_linear(gray, fw, fh)
                if face_post_eq:
                    small = orc.equalize_hist(small)
                r = (C.c_int * 6)()
                L.pls_pass_rule(npass, r)
                maxs = (fw, fh) if r[4] else (0, 0)
                assert bool(mirror) == bool(r[5])
                faces = self.det[0](small, sf.value, r[0], r[1], (r[2], r[3]), maxs)
                if mirror:
                    faces_m = self.det[0](orc.flip_h(small), sf.value, r[0], r[1], (r[2], r[3]), maxs)
            if npass < 0:
                faces = None
            fa, fp = _ints(faces if faces is not None else [])
            ma, mp = _ints(faces_m if faces_m is not None else [])
            nsearch = L.pls_rois(h, fp, len(fa) // 4 if faces is not None else -1, mp, len(ma) // 4 if faces_m is not None else -1, MAX_SEARCHES, out, sfs)
            assert nsearch >= 0
            part = orc.equalize_hist(orc.resize_linear(gray, pw, ph))
            for k in range(nsearch):
                x, y, w, hh, casc, _side, mn, flags, minw, minh, valid = out[11 * k:11 * k + 11]
                if not valid:
                    counts.append(-1)
                    continue
                assert 0 <= x and 0 <= y and x + w <= pw and y + hh <= ph
                got = self.det[2 if casc else 1](part[y:y + hh, x:x + w], sfs[k], mn, flags, (minw, minh), (0, 0))
                counts.append(len(got))
                found.append(got)
        fa, fp = _ints(np.concatenate(found) if found else [])
        ca, cp = _ints(counts)
        L.pls_finish(h, fp, cp)
        return self._list(0), self._list(1)


# ------------------------------------------------------------------ the LBP cascades and frames of the part tests
FACE, PART_A, PART_B = "w24", "w12", "w20x28"          # the roles' cascades (lbp_cases.CASCADES)


def gray_to_bgr(g):
    return np.ascontiguousarray(np.dstack([g, g, g]))


def lbp_frames(W=640, H=480, n=5, seed=31):
    """a natural field with a w24 face template pasted at two sizes; part templates (12 x 12 and 20 x 28, stretched) inside the face
    boxes, where the elements look for eyes, nose, mouth and ears; the face moves a little from frame to frame and is absent on frame 3"""
    frames = []
    for i in range(n):
        g = synth.make_gray(W, H, synth.frame_seed(5, seed + i), "natural")
        if i != 3:
            for (x, y, s) in ((W // 6 + 6 * i, H // 6, H * 0.5 / 24), (W // 2 + 40, H // 3 + 4 * i, H * 0.3 / 24)):
                x, y, side = int(x), int(y), int(round(24 * s))
                g = synth.paste_lbp_faces(g, [(x, y, s)], 24, 24, seed)
                ps = side / 24 * 0.22            # part templates a fifth of the face wide
                spots = [(0.18, 0.22), (0.60, 0.22), (0.39, 0.45), (0.36, 0.70), (0.02, 0.35), (0.78, 0.35)]
                for k, (fx, fy) in enumerate(spots):
                    ow, oh = (12, 12) if k % 2 == 0 else (20, 28)
                    g = synth.paste_lbp_faces(g, [(int(x + fx * side), int(y + fy * side), ps * 24 / ow)], ow, oh, seed + k)
        frames.append(gray_to_bgr(g))
    return frames


@functools.lru_cache(maxsize=None)
def refs():
    return {n: K.cascade(n)[1] for n in (FACE, PART_A, PART_B)}


def roles(kind, face_lbp=True, parts_lbp=True):
    """(face, a, b) cascade names of a kind: LBP names of lbp_cases.CASCADES, or None for the role's Haar cascade"""
    two = kind in ("eye", "ear")
    return (FACE if face_lbp else None, PART_A if parts_lbp else None, (PART_B if parts_lbp else None) if two else False)


@functools.lru_cache(maxsize=None)
def expected_lbp(kind, W=640, H=480, **props):
    """([(list a, list b)] per frame of lbp_frames(W, H), the three detectors with the sizes they saw) with every role LBP"""
    r = refs()
    two = kind in ("eye", "ear")
    dets = (lbp_detector(r[FACE]), lbp_detector(r[PART_A]), lbp_detector(r[PART_B]) if two else None)
    h = Harness(kind, *dets, **props)
    out = [h.process(f) for f in lbp_frames(W, H)]
    h.close()
    return out, dets


def lbp_face_boxes(W, H, i):
    """the face boxes pasted into frame i of lbp_frames(W, H), original-frame pixels: what an upstream face detector would push"""
    if i == 3:
        return []
    return [[int(x), int(y), int(round(24 * s)), int(round(24 * s))] for (x, y, s) in ((W // 6 + 6 * i, H // 6, H * 0.5 / 24), (W // 2 + 40, H // 3 + 4 * i, H * 0.3 / 24))]


def mixed_frames(W=640, H=480, n=4, seed=57):
    """part_scenes.scene's Haar face with LBP part templates pasted over its eye, nose, mouth and ear regions, and a w24 LBP face
    template beside it: frames on which a Haar face pass and an LBP face pass both find a face"""
    frames = []
    for i in range(n):
        s = int(H * 0.5)
        x, y = W // 5 + 5 * i, H // 5
        g = synth.make_gray(W, H, seed + i, "natural", [(x, y, s)])
        for k, (fx, fy) in enumerate([(0.18, 0.22), (0.60, 0.22), (0.39, 0.45), (0.36, 0.70), (0.02, 0.35), (0.78, 0.35)]):
            ow, oh = (12, 12) if k % 2 == 0 else (20, 28)
            g = synth.paste_lbp_faces(g, [(int(x + fx * s), int(y + fy * s), s * 0.22 / ow)], ow, oh, seed + k)
        g = synth.paste_lbp_faces(g, [(W // 2 + 90, H // 2 + 10, H * 0.3 / 24)], 24, 24, seed)
        frames.append(gray_to_bgr(g))
    return frames


HAAR_PARTS = {"eye": ("righteye", "lefteye"), "nose": ("nose", None), "mouth": ("mouth", None), "ear": ("leftear", "rightear")}


@functools.lru_cache(maxsize=None)
def haar_xml():
    """name -> xml of the Haar cascades of the mixed streams"""
    x = {n: synth.synthetic_part_cascade_xml(n) for names in HAAR_PARTS.values() for n in names if n}
    x["face"] = synth.synthetic_cascade_xml()
    return x


@functools.lru_cache(maxsize=None)
def _haar_cpu():
    return {n: orc.parse_cascade_xml(x) for n, x in haar_xml().items()}


def role_names(kind, face_lbp, parts_lbp):
    """(face, a, b) as ("lbp" | "haar", cascade name); b is None for the kinds with one part cascade"""
    ha, hb = HAAR_PARTS[kind]
    two = hb is not None
    face = ("lbp", FACE) if face_lbp else ("haar", "face")
    a = ("lbp", PART_A) if parts_lbp else ("haar", ha)
    b = (("lbp", PART_B) if parts_lbp else ("haar", hb)) if two else None
    return face, a, b


def detectors(kind, face_lbp, parts_lbp):
    def make(role):
        if role is None:
            return None
        return lbp_detector(refs()[role[1]]) if role[0] == "lbp" else haar_detector(_haar_cpu()[role[1]])
    return tuple(make(r) for r in role_names(kind, face_lbp, parts_lbp))


@functools.lru_cache(maxsize=None)
def expected(kind, face_lbp, parts_lbp, scene="lbp", W=640, H=480, event=False, nv12=False):
    """[(list a, list b)] per frame: the harness with the statement's detectors on the scene's frames.  event: detect-event mode, the
    pasted face boxes pushed before every frame but the third.  nv12: the frames as the conversion statement reads their NV12 form."""
    frames = lbp_frames(W, H) if scene == "lbp" else mixed_frames(W, H)
    if nv12:
        frames = [nv12_of(f)[2] for f in frames]
    h = Harness(kind, *detectors(kind, face_lbp, parts_lbp), detect_event=int(event))
    out = []
    for i, f in enumerate(frames):
        if event and i != 2:
            h.push_faces(lbp_face_boxes(W, H, i))
        out.append(h.process(f))
    h.close()
    return out


def nv12_of(bgr):
    """(buffer, layout tuple, the conversion statement's BGR image) of a gray BGR frame as NV12: its luma, neutral chroma"""
    import yuv_reference as Y
    import yuv_stream_scenes as S
    y = np.ascontiguousarray(bgr[:, :, 0])
    H, W = y.shape
    c = np.full((H // 2, W // 2), 128, np.uint8)
    buf, lay = S.pack_planes(y, c, c, Y.NV12, pad=32)
    return buf, lay, Y.bgr(buf, W, H, lay)
