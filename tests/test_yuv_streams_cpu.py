"""4:2:0 part streams and trackers (nvca_part_stream_set_input, nvca_tracker_set_input) on the CPU: the ABI is there, and the oracle's
view of the scenes the GPU tests use (tests/yuv_stream_scenes.py) -- so that those cannot pass on empty lists, and so that the tracker
scenes cannot pass on a kernel that takes the luma for the gray value."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import yuv_reference as R
import yuv_stream_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nvca_part_stream_set_input", "nvca_tracker_set_input")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from nubovca import capi
    return capi.load()


def test_header_declares_and_the_library_exports_the_entry_points(lib):
    hdr = open(os.path.join(ROOT, "include", "nubovca.h")).read()
    assert re.search(r"int\s+nvca_part_stream_set_input\(nvca_part_stream \*s, const nvca_pixel_layout \*layout\);", hdr)
    assert re.search(r"int\s+nvca_tracker_set_input\(nvca_tracker \*t, const nvca_pixel_layout \*layout\);", hdr)
    from nubovca import capi
    raw = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in capi.SYMBOLS
        assert getattr(raw, name) is not None          # (an AttributeError where the symbol is missing)


def test_binding_declares_the_argument_types(lib):
    from nubovca import capi
    for name in NEW:
        assert getattr(lib, name).argtypes == [C.c_void_p, C.POINTER(capi.PixelLayout)], name
    assert callable(capi.PartStream.set_input) and callable(capi.Tracker.set_input)


def test_null_handles_are_refused_without_a_device(lib):
    from nubovca import capi
    lay = capi.pixel_layout(R.NV12, (0, 640 * 480), (640, 640))
    for name in NEW:
        assert getattr(lib, name)(None, C.byref(lay)) == capi.ERR_ARG
        assert getattr(lib, name)(None, None) == capi.ERR_ARG


@pytest.mark.parametrize("W,H", S.PART_GEOS, ids=lambda v: str(v))
def test_oracle_finds_parts_in_the_part_scenes(W, H):
    """eye and ear: at least one part on every one of the 9 frames (their lists carry over the frame without a face); nose and mouth:
    one part on every frame but frame 4"""
    for kind in ("eye", "ear"):
        exp = S.part_expected(kind, W, H)
        assert all(len(a) + len(b) >= 1 for a, b in exp), (kind, [(len(a), len(b)) for a, b in exp])
    for kind in ("nose", "mouth"):
        exp = S.part_expected(kind, W, H)
        assert [len(a) + len(b) for a, b in exp] == [0 if i == 4 else 1 for i in range(S.PART_FRAMES)], (kind, [(len(a), len(b)) for a, b in exp])


def test_part_frames_of_both_formats_and_any_padding_hold_the_same_samples():
    W, H = 322, 242
    ref = S.part_bgr(W, H, 3)
    for fmt, kw in ((R.NV12, {}), (R.I420, {}), (R.NV12, dict(pad=6, luma_rows=256, gap=64)), (R.I420, dict(pad=6, luma_rows=256, gap=64, chroma_pad=2))):
        buf, lay = S.part_frame(W, H, 3, fmt, **kw)
        assert np.array_equal(R.bgr(buf, W, H, lay), ref), (fmt, kw)


@pytest.mark.parametrize("W,H", S.TRK_GEOS, ids=lambda v: str(v))
def test_tracker_scenes_need_the_chroma(W, H):
    """every frame after the first gives boxes, and a tracker that takes Y for gray gives another number of them on some frame: the
    chroma-only movers are seen through the conversion only"""
    exp = S.trk_expected(W, H)
    luma = S.oracle_tracker_run([S.trk_luma_bgra(W, H, i) for i in range(S.TRK_FRAMES)])
    n_exp, n_luma = [len(b) for b in exp], [len(b) for b in luma]
    print(W, H, "components per frame:", n_exp, "with luma taken as gray:", n_luma)
    assert n_exp[0] == 0 and all(n >= 1 for n in n_exp[1:]), n_exp
    assert n_exp != n_luma and sum(n_exp) > sum(n_luma), (n_exp, n_luma)
    assert sum(1 for a, b in zip(exp[1:], luma[1:]) if not np.array_equal(a, b)) >= 3, (n_exp, n_luma)


def test_tracker_frames_of_both_formats_and_any_padding_hold_the_same_samples():
    W, H = 644, 482
    ref = S.trk_bgra(W, H, 2)[..., :3]
    for fmt, kw in ((R.NV12, {}), (R.I420, {}), (R.NV12, dict(pad=5)), (R.I420, dict(pad=5)), (R.NV12, dict(pad=4)), (R.I420, dict(pad=4, chroma_pad=2, gap=8))):
        buf, lay = S.trk_frame(W, H, 2, fmt, **kw)
        assert np.array_equal(R.bgr(buf, W, H, lay), ref), (fmt, kw)
