"""What the GStreamer elements hand on for a frame -- downstream event, signal payload, outlines -- is pure code
(nubomedia-vca_amd/gst/element_output.cpp).  tests/san/gst_output_driver.cpp, a stand-alone program linked against GStreamer, runs
it on cases built here; the expectations are a restatement of the reference's own rules, written from the cited lines of
kms{face,eye,nose,mouth,ear}detect.cpp, BaseFace.cpp and gstnubotracker.cpp -- never the shim's output.  No GPU, no library call."""
import os
import string
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nubomedia-vca_amd", "gst"))
import build_gst  # noqa: E402

pytestmark = pytest.mark.skipif(not build_gst.available(), reason="GStreamer dev files not present")
SAN = os.path.join(ROOT, "tests", "san")
GST = os.path.join(ROOT, "nubomedia-vca_amd", "gst")
EYE, NOSE, MOUTH, EAR = 0, 1, 2, 3                              # NVCA_PART_*
RECT3, RING4 = 0, 1                                             # NVCA_SHAPE_*


def rgb(r, g, b):
    return (b, g, r, 0)                                         # CV_RGB(r, g, b) is Scalar(b, g, r, 0): the bytes of a BGR(A) pixel


NOSE_COLORS = [rgb(255, 0, 255), rgb(255, 0, 0), rgb(255, 255, 0), rgb(255, 128, 0), rgb(0, 255, 0), rgb(0, 255, 255), rgb(0, 128, 255), rgb(0, 0, 255)]    # NOSE :808-815
MOUTH_COLORS = [rgb(255, 255, 0), rgb(255, 128, 0), rgb(255, 0, 0), rgb(255, 0, 255), rgb(0, 128, 255), rgb(0, 0, 255), rgb(0, 255, 255), rgb(0, 255, 0)]   # MOUTH :814-821
EAR_COLORS = [rgb(0, 0, 255), rgb(0, 128, 255), rgb(0, 255, 255), rgb(0, 255, 0), rgb(255, 128, 0), rgb(255, 255, 0), rgb(255, 0, 0), rgb(255, 0, 255)]     # EAR :736-743


@pytest.fixture(scope="module")
def driver():
    out = os.path.join(SAN, "build", "gst_output_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "gst_output_driver.cpp"), os.path.join(GST, "element_output.cpp")]
    deps = srcs + [os.path.join(GST, "element_output.h"), os.path.join(ROOT, "include", "nubovca.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-deprecated-declarations"] + srcs + ["-o", out] + build_gst.INC + build_gst.LIBS,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(driver, tmp_path, cases):
    path = tmp_path / "cases.txt"
    path.write_text("".join(c + "\n" for c in cases))
    r = subprocess.run([driver, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout.splitlines()


# ---- GStreamer's own text form of a structure (gst_structure_to_string / gst_value_serialize): "name, field=(type)value, ...;" with a
# nested structure written as a string in which every byte outside [A-Za-z0-9_-+/:.] is backslash-escaped, in double quotes
_PLAIN = set(string.ascii_letters + string.digits + "_-+/:.")


def _wrap(s):
    return s if s and all(c in _PLAIN for c in s) else '"' + "".join(c if c in _PLAIN else "\\" + c for c in s) + '"'


def _structure(name, fields):
    return name + "".join(", %s=(%s)%s" % (k, t, _wrap(str(v))) for k, t, v in fields) + ";"


def _box_field(idx, sname, type_, box, mul=1):
    x, y, w, h = box
    sub = _structure(sname, [("type", "string", type_), ("x", "uint", x * mul), ("y", "uint", y * mul), ("width", "uint", w * mul), ("height", "uint", h * mul)])
    return (str(idx), "structure", sub)


def _stamp(pts):
    return ("timestamp", "structure", _structure("time", [("pts", "guint64", pts)]))


def _payload(boxes):
    return "".join("x:%d,y:%d,width:%d,height:%d;" % tuple(b) for b in boxes)


def _rect(x0, y0, x1, y1, colour):
    """cvRectangle(img, (x0, y0), (x1, y1), colour, 3, 8, 0) as an nvca_shape"""
    return (RECT3, x0, y0, x1 - x0, y1 - y0) + tuple(colour)


def _words(boxes):
    return "%d %s" % (len(boxes), " ".join("%d %d %d %d" % tuple(b) for b in boxes))


def _check(lines, expect, what):
    event, payload, shapes = expect
    assert lines[0] == "event " + (event if event is not None else "none"), (what, lines[0], event)
    assert lines[1] == "payload " + payload, (what, lines[1], payload)
    assert lines[2] == "shapes " + "".join(",".join(str(v) for v in s) + ";" for s in shapes), (what, lines[2], shapes)


# ---- the reference's rules -----------------------------------------------------------------------------------------------------------
def ref_face(working, width, pts, w2p, view, overlay):
    """kms_face_send_event, FACE/kmsfacedetect.cpp:179-249, on the boxes of the working image (width w2p): everything times
    norm_scale = img_width / width2process (int); drawing: Faces::draw -> BaseFace::draw_face_in_image(img, scale), FACE/BaseFace.cpp:70-82,
    (x * scale, y * scale) .. ((x + w - 1) * scale, (y + h - 1) * scale) in colors[1] = CV_RGB(0,128,255); :832-850: drawn when
    view_faces > 0 and no overlay image is set"""
    s = width // w2p
    scaled = [(x * s, y * s, w * s, h * s) for x, y, w, h in working]
    event = _structure("message", [_stamp(pts)] + [_box_field(i, "face", "face", b) for i, b in enumerate(scaled)])
    shapes = []
    if view > 0 and not overlay:
        shapes = [_rect(x * s, y * s, (x + w - 1) * s, (y + h - 1) * s, rgb(0, 128, 255)) for x, y, w, h in working]
    return scaled, (event, _payload(scaled), shapes)


def ref_tracker(boxes, visual):
    """TRK/gstnubotracker.cpp:383-414: cvRectangle(rec.tl(), rec.br(), Scalar(0,0,255), 3) when visual_mode > 0; no downstream event"""
    shapes = [_rect(x, y, x + w, y + h, (0, 0, 255, 0)) for x, y, w, h in boxes] if visual > 0 else []
    return (None, _payload(boxes), shapes)


def ref_eye(right, left, pts, view, overlay):
    """EYE/kmseyedetect.cpp:236-284: eye_left* first, then eye_right*, one running index; :1071-1099: one circle per side around the first
    box, right side first, radius cvRound((w + h) * 0.25) of the RIGHT eye when there is one -- the left eye's own only if not"""
    event = _structure("message", [_stamp(pts)] + [_box_field(i, "eye_left", "eye", b) for i, b in enumerate(left)]
                       + [_box_field(len(left) + i, "eye_right", "eye", b) for i, b in enumerate(right)])
    shapes, radius = [], -1
    if view == 1 and not overlay:
        for side in (right, left):
            if side:
                x, y, w, h = side[0]
                if radius < 0:
                    radius = round((w + h) * 0.25)                     # cvRound: to nearest, ties to even -- as Python's round
                shapes.append((RING4, x + w // 2, y + h // 2, radius, 0, 255, 0, 0, 0))     # Scalar(255, 0, 0), thickness 4
    return (event, _payload(left + right), shapes)


def ref_nose(noses, view, overlay):
    """NOSE/kmsnosedetect.cpp:226-249: a structure "noses" WITHOUT timestamp; :896-905: (x, y) .. (x + w, y + h - 1), colors[j % 8]"""
    event = _structure("noses", [_box_field(i, "noses", "nose", b) for i, b in enumerate(noses)])
    shapes = [_rect(x, y, x + w, y + h - 1, NOSE_COLORS[j % 8]) for j, (x, y, w, h) in enumerate(noses)] if view == 1 and not overlay else []
    return (event, _payload(noses), shapes)


def ref_mouth(faces, mouths, width, pts, detect_event, view, overlay):
    """MOUTH/kmsmouthdetect.cpp:210-256: faces times norm_faces = (int)scale_o2f first, then the mouths, one running index; only mouths in
    the payload; :305-309: scale_o2f = width / width (1) under detect_event, else width / FACE_WIDTH (160); :895-903: (x, y) ..
    (x + w - 1, y + h - 1), colors[j % 8]"""
    norm = 1 if detect_event else int(float(width) / 160.0)
    event = _structure("message", [_stamp(pts)] + [_box_field(i, "face", "face", b, norm) for i, b in enumerate(faces)]
                       + [_box_field(len(faces) + i, "mouth", "mouth", b) for i, b in enumerate(mouths)])
    shapes = [_rect(x, y, x + w - 1, y + h - 1, MOUTH_COLORS[j % 8]) for j, (x, y, w, h) in enumerate(mouths)] if view == 1 and not overlay else []
    return norm, (event, _payload(mouths), shapes)


def ref_ear(left_side, right_side, view, overlay):
    """EAR/kmseardetect.cpp:196-290: the message is built and never pushed; the payload lists rear (RIGHT_SIDE) before lear; :812-816: the
    right side's ears are drawn first, (x, y) .. (x + w, y + h - 1).  The palette index: the shim has always let it run on from the
    right list into the left one (the reference's print_ears starts each side at 0, :735) -- what it draws must not change, so that
    is what is expected here."""
    both = right_side + left_side
    shapes = [_rect(x, y, x + w, y + h - 1, EAR_COLORS[j % 8]) for j, (x, y, w, h) in enumerate(both)] if view == 1 and not overlay else []
    return (None, _payload(both), shapes)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def test_face_and_tracker_output(driver, tmp_path):
    working = [(10, 12, 40, 40), (60, 30, 25, 27), (100, 70, 33, 31)]
    cases, expect = [], []
    for width in (640, 320):
        for n in (0, 1, 3):
            for view, overlay in ((0, 0), (1, 0), (1, 1)):
                pts = 1000 * width + 10 * n + view
                scaled, exp = ref_face(working[:n], width, pts, 160, view, overlay)
                cases.append("face %d %d 160 %d %d %s" % (width, pts, view, overlay, _words(scaled)))
                expect.append(("face", width, n, view, overlay, exp))
    boxes = [(5 + 30 * i, 7 + 11 * i, 20 + i, 30 - i) for i in range(5)]
    for n in (0, 5):
        for visual in (0, 1, 4):
            cases.append("tracker %d %s" % (visual, _words(boxes[:n])))
            expect.append(("tracker", n, visual, ref_tracker(boxes[:n], visual)))
    lines = _run(driver, tmp_path, cases)
    assert len(lines) == 3 * len(cases)
    for k, e in enumerate(expect):
        _check(lines[3 * k:3 * k + 3], e[-1], e[:-1])
    # the quirk is in the cases: at 640 the far corner lies scale = 4 short of x + w, at 320 it lies 2 short
    assert expect[4][-1][2][0][:5] == (RECT3, 40, 48, 156, 156) and expect[13][-1][2][0][:5] == (RECT3, 20, 24, 78, 78)


def test_part_output(driver, tmp_path):
    # eye boxes of different sizes: (w + h) * 0.25 is 7.5 -> 8 for the right eye and 5.5 -> 6 / 6.5 -> 6 for the left ones
    right, left = [(200, 100, 16, 14), (300, 100, 30, 30)], [(120, 104, 12, 10), (50, 60, 13, 13)]
    cases, expect = [], []
    for na, nb in ((0, 0), (1, 0), (0, 1), (2, 2)):
        for view, overlay in ((1, 0), (0, 0), (1, 1)):
            cases.append("part %d 640 77 0 %d %d %s %s 0" % (EYE, view, overlay, _words(right[:na]), _words(left[:nb])))
            expect.append(("eye", na, nb, view, overlay, ref_eye(right[:na], left[:nb], 77, view, overlay)))
    noses = [(100, 120, 30, 24), (300, 200, 21, 19), (10, 20, 5, 6)]
    for n in (0, 3):
        for view in (1, 0):
            cases.append("part %d 640 5 0 %d 0 %s 0 0" % (NOSE, view, _words(noses[:n])))
            expect.append(("nose", n, view, ref_nose(noses[:n], view, 0)))
    faces, mouths = [(20, 15, 50, 50), (90, 40, 44, 44)], [(110, 170, 60, 30), (400, 260, 52, 27)]
    norms = []
    for detect_event in (0, 1):
        norm, exp = ref_mouth(faces, mouths, 640, 9000000000, detect_event, 1, 0)
        norms.append(norm)
        cases.append("part %d 640 9000000000 %d 1 0 %s 0 %s" % (MOUTH, detect_event, _words(mouths), _words(faces)))
        expect.append(("mouth", detect_event, exp))
    assert norms == [4, 1]
    lear = [(10 + 40 * i, 20, 18 + i, 30 + i) for i in range(5)]        # the library's list a: LEFT_SIDE
    rear = [(15 + 40 * i, 200, 17 + i, 29 + i) for i in range(5)]       # list b: RIGHT_SIDE
    for view in (1, 0):
        cases.append("part %d 640 3 0 %d 0 %s %s 0" % (EAR, view, _words(lear), _words(rear)))
        expect.append(("ear", view, ref_ear(lear, rear, view, 0)))
    lines = _run(driver, tmp_path, cases)
    assert len(lines) == 3 * len(cases)
    for k, e in enumerate(expect):
        _check(lines[3 * k:3 * k + 3], e[-1], e[:-1])
    both_eyes = [e for e in expect if e[:5] == ("eye", 2, 2, 1, 0)][0][-1][2]
    assert [s[3] for s in both_eyes] == [8, 8] and round((12 + 10) * 0.25) == 6      # the left ring took the right eye's radius, not its own 6
    ears = [e for e in expect if e[:2] == ("ear", 1)][0][-1]
    assert ears[0] is None and len(ears[2]) == 10 and ears[2][8][5:] == EAR_COLORS[0] and ears[2][5][5:] == EAR_COLORS[5]


def test_signal_throttle(driver, tmp_path):
    """every element's send_event (FACE/kmsfacedetect.cpp:228-241 ...): something found, server_events == 1 and diff_time > events_ms"""
    table = [(n, on, dt, ms) for n in (0, 1, 3) for on in (0, 1, 2) for dt, ms in ((0.0, 0), (0.5, 0), (100.0, 100), (100.5, 100), (29999.0, 30001), (30001.5, 30001))]
    lines = _run(driver, tmp_path, ["due %d %d %r %r %d" % (n, on, 5000000.25 + dt, 5000000.25, ms) for n, on, dt, ms in table])
    assert lines == ["due %d" % (n > 0 and on == 1 and dt > ms) for n, on, dt, ms in table]
    assert lines.count("due 1") == 6


def test_upstream_event_parsers(driver, tmp_path):
    """FACE/kmsfacedetect.cpp:680-712 (a "motion" field holding a structure arms the detector) and EYE/kmseyedetect.cpp:680-724 (the
    sub-structures whose type is "face", "timestamp" skipped), up to the part elements' 64 faces"""
    motion = ("motion", "structure", _structure("motion", [("grid", "string", "0101")]))
    face = lambda i: (7 * i, 3 * i + 1, 40 + i, 41 + i)
    cases = ["motion " + _structure("message", [_stamp(5), motion]),
             "motion " + _structure("message", [_stamp(5), _box_field(0, "face", "face", face(1))]),
             "motion " + _structure("message", [("motion", "int", 1)])]                      # a field of that name that is no structure
    for n in (0, 2, 70):
        fields = [_stamp(11), _box_field(0, "eye_left", "eye", (1, 2, 3, 4))] + [_box_field(i + 1, "face", "face", face(i)) for i in range(n)]
        fields.insert(2, ("count", "int", n))                                                 # neither a structure nor a face
        cases.append("faces 64 " + _structure("message", fields))
    lines = _run(driver, tmp_path, cases)
    assert lines[:3] == ["motion 1", "motion 0", "motion 0"]
    for line, n in zip(lines[3:], (0, 2, 70)):
        assert line == "faces %d " % min(n, 64) + "".join("%d,%d,%d,%d;" % face(i) for i in range(min(n, 64))), (n, line)
