"""The harness of tests/lbp_part_cases.py on the CPU, without the code under test.  (1) With the oracle's detectMultiScale on Haar
cascades as its detector it reproduces orc.PartStream frame by frame on the scenes of tests/part_scenes.py, for all four kinds and in
detect-event mode: the expected lists of tests/test_gpu_lbp_parts.py are the elements' logic and nothing else.  (2) On the LBP frames the
statement alone finds parts: for every kind some frame has a non-empty list on each output, some search region lies inside the small
route's LDS bound, and the face pass is named for the side of the bound it lies on."""
import numpy as np
import pytest

import lbp_part_cases as P
import lbp_roi_cases as RC
import orc
from nubovca import synth
from part_scenes import scene

PARTS = {"eye": ("righteye", "lefteye"), "nose": ("nose", None), "mouth": ("mouth", None), "ear": ("leftear", "rightear")}
NAMES = {"width_to_process": "width_to_process", "process_x_every_4": "process_x_every_4", "scale_factor_pct": "scale_factor_pct", "detect_event": "detect_event"}

pytestmark = pytest.mark.skipif(P.shim() is None, reason="no clang++")


@pytest.fixture(scope="module")
def haar(synth_xml):
    c = {n: orc.parse_cascade_xml(synth.synthetic_part_cascade_xml(n)) for names in PARTS.values() for n in names if n}
    c["face"] = orc.parse_cascade_xml(synth_xml)
    return c


def _pair(haar, kind, **props):
    a, b = PARTS[kind]
    h = P.Harness(kind, P.haar_detector(haar["face"]), P.haar_detector(haar[a]), P.haar_detector(haar[b]) if b else None, **props)
    o = orc.PartStream(P.KINDS[kind], haar["face"], haar[a], haar[b] if b else None, **props)
    return h, o


@pytest.mark.parametrize("kind", list(PARTS))
@pytest.mark.parametrize("W,H,props", [(640, 480, {}), (800, 600, {"process_x_every_4": 2, "scale_factor_pct": 15})])
def test_harness_is_the_oracles_part_stream(haar, kind, W, H, props):
    h, o = _pair(haar, kind, **props)
    seen = 0
    for i, f in enumerate(scene(W, H, 7, 700 + W)):
        ha, hb = h.process(f)
        ea, eb = o.process(f)
        assert np.array_equal(ha, ea) and np.array_equal(hb, eb), (kind, i, ha, ea, hb, eb)
        seen += len(ea) + len(eb)
    assert seen > 0
    h.close()


@pytest.mark.parametrize("kind", ["eye", "nose", "mouth"])
def test_harness_in_detect_event_mode(haar, kind):
    h, o = _pair(haar, kind, detect_event=1)
    fs = orc.FaceStream(haar["face"])
    seen = 0
    for i, f in enumerate(scene(640, 480, 7, 900)):
        boxes, _ = fs.process(f)
        if i % 3 != 2 and len(boxes):
            h.push_faces(boxes)
            o.push_faces(boxes)
        ha, hb = h.process(f)
        ea, eb = o.process(f)
        assert np.array_equal(ha, ea) and np.array_equal(hb, eb), (kind, i)
        seen += len(ea) + len(eb)
    assert seen > 0
    h.close()


@pytest.mark.parametrize("kind", list(PARTS))
def test_lbp_frames_meet_their_condition(kind):
    """all roles LBP: parts are found on both outputs (the kinds with one output: on that one), part regions fit the small route's LDS,
    and the 160 x 120 face pass lies inside the LBP bound and outside the Haar one"""
    exp, dets = P.expected_lbp(kind)
    two = PARTS[kind][1] is not None
    assert any(len(a) for a, b in exp) and (not two or any(len(b) for a, b in exp)), [(len(a), len(b)) for a, b in exp]
    face, a, b = dets
    assert (160, 120) in face.seen and RC.fits_lds(160, 120) and not RC.haar_fits(160, 120)
    regions = a.seen + (b.seen if b else [])
    assert regions and any(RC.fits_lds(w, h) for w, h in regions) and all(w <= 320 and h <= 240 for w, h in regions), regions


@pytest.mark.parametrize("kind,face_lbp,parts_lbp,scene", [("eye", False, True, "mixed"), ("nose", False, True, "mixed"), ("mouth", True, False, "mixed"),
                                                           ("ear", True, False, "mixed"), ("nose", True, True, "event"), ("eye", True, True, "event")])
def test_mixed_and_event_sequences_search_something(kind, face_lbp, parts_lbp, scene):
    """what the mixed-role and detect-event configurations of the GPU test compare is not a run of empty frames: the harness issues
    part searches on these frames (a face was found or pushed), whether or not a part comes out of them"""
    dets = P.detectors(kind, face_lbp, parts_lbp)
    h = P.Harness(kind, *dets, detect_event=int(scene == "event"))
    frames = P.lbp_frames() if scene == "event" else P.mixed_frames()
    for i, f in enumerate(frames):
        if scene == "event" and i != 2:
            h.push_faces(P.lbp_face_boxes(640, 480, i))
        h.process(f)
    h.close()
    assert dets[1].seen, (kind, scene)
    assert (not dets[0].seen) == (scene == "event")
