"""detectMultiScale with outputRejectLevels on the device (nvca_detect_raw_levels / nvca_detect_multiscale_levels: lbp_job.cpp's levels launch
set, k_lbp_levels / k_hnew_levels, group_levels.cpp) against the numpy statement of SURVEY.md A.17 (tests/levels_reference.py): bit for bit --
rectangles, reject levels, and the level weights viewed as uint64 --, raw and grouped, from host and from device memory.  The cases and the
hand-derived lists are tests/levels_cases.py's; tests/test_levels_cpu.py asserts on the statement alone that they reach what they are meant
to reach."""
import ctypes as C

import numpy as np
import pytest

import lbp_cases as LK
import levels_cases as K
import levels_reference as V
from nubovca import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def loaded(ctx):
    """xml -> the device's cascade, loaded once"""
    cache = {}

    def get(xml):
        if xml not in cache:
            cache[xml] = ctx.load_cascade_xml(xml)
        return cache[xml]
    return get


def _bits(w):
    return np.asarray(w, np.float64).view(np.uint64)


def _assert_same(got, exp, what):
    assert got[0].shape == np.asarray(exp[0]).reshape(-1, 4).shape, (what, len(got[0]), len(exp[0]))
    assert np.array_equal(got[0], np.asarray(exp[0], np.int32).reshape(-1, 4)), what
    assert np.array_equal(got[1], np.asarray(exp[1], np.int32)), what
    assert np.array_equal(_bits(got[2]), _bits(exp[2])), what


def _views(img, pad=0):
    """(name, call arguments) of the image in host and in device memory; pad > 0: as a sub-matrix of a buffer `pad` bytes wider"""
    import torch
    rows, cols = img.shape
    host = np.full((rows, cols + pad), 201, np.uint8)
    host[:, :cols] = img
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return [("host", host, host.ctypes.data, dict(mem=capi.MEM_HOST, shape=(rows, cols), stride=cols + pad)),
            ("device", dev, dev.data_ptr(), dict(mem=capi.MEM_DEVICE, shape=(rows, cols), stride=cols + pad))]


def _check(ctx, casc, img, sf, exp, thresholds, pad=0):
    """raw and grouped answers from both memories against the statement's"""
    cls = V.classes(exp[0]) if any(mn > 0 for mn in thresholds) and len(exp[0]) else None
    grouped = {mn: V.group_levels(*exp, mn, cls=cls) for mn in thresholds}
    for name, keep, ptr, where in _views(img, pad):
        _assert_same(ctx.detect_raw_levels(casc, ptr, sf, **where), exp, (name, "raw"))
        for mn in thresholds:
            _assert_same(ctx.detect_multiscale_levels(casc, ptr, sf, mn, **where), grouped[mn], (name, mn))


# ------------------------------------------------------------------ the hand-made cases of tests/test_levels_cpu.py
@pytest.mark.parametrize("case", K.hand_cases(), ids=[c[0] for c in K.hand_cases()])
def test_hand_made_levels_and_weights(ctx, case):
    _, kind, cdict, gray, sf, rects, levels, weights = case
    casc = ctx.load_cascade_xml(K.to_xml(kind, cdict))
    try:
        _check(ctx, casc, gray, sf, (rects, levels, weights), (0, 1, 4))          # (every window is a class of its own: its level alone decides)
    finally:
        casc.free()


# ------------------------------------------------------------------ calibrated cascades on images with pasted templates
@pytest.mark.parametrize("cid", sorted(K.NATURAL))
def test_natural_cases_raw_and_grouped(ctx, loaded, cid):
    xml, ref, img, sf = K.natural(cid)
    exp = K.expected("natural", cid)
    assert len(exp[0]) > 0
    _check(ctx, loaded(xml), img, sf, exp, K.group_thresholds(ref))


@pytest.mark.parametrize("cid", K.PADDED)
def test_a_padded_sub_matrix(ctx, loaded, cid):
    xml, ref, img, sf = K.natural(cid)
    _check(ctx, loaded(xml), img, sf, K.expected("natural", cid), (0, len(ref.stage_sizes) - 1), pad=19)


@pytest.mark.parametrize("route", K.HI)
def test_high_byte_planes_of_the_squared_integral(ctx, loaded, route):
    xml, ref, img, sf = K.hi_planes(route)
    exp = K.expected("hi", route)
    assert len(exp[0]) > 0
    _check(ctx, loaded(xml), img, sf, exp, K.group_thresholds(ref))


@pytest.mark.parametrize("kind", [K.LBP, K.HAAR])
def test_candidate_overflow_rerun_answers_exactly(ctx, loaded, kind):
    xml, ref, img, sf = K.overflow(kind)
    exp = K.expected("overflow", kind)
    assert len(exp[0]) > 4 * 256
    ctx.set_hit_capacity(256)
    try:
        _assert_same(ctx.detect_raw_levels(loaded(xml), img, sf), exp, "raw")
        _assert_same(ctx.detect_multiscale_levels(loaded(xml), img, sf, 3), V.group_levels(*exp, 3), "grouped")
    finally:
        ctx.set_hit_capacity(16384)


def test_min_and_max_size_and_every_flags_value(ctx, loaded):
    """the levels scan is the plain scan's: minSize / maxSize cut levels at both ends, flags are ignored"""
    xml, ref, img, sf = K.natural("haar-w24")
    full = K.expected("natural", "haar-w24")
    exp = V.scan_levels(ref, img, sf, (30, 30), (60, 60))
    assert 0 < len(exp[0]) < len(full[0])
    _assert_same(ctx.detect_raw_levels(loaded(xml), img, sf, 0, (30, 30), (60, 60)), exp, "sizes")
    for fl in (capi.HAAR_SCALE_IMAGE, capi.HAAR_FIND_BIGGEST_OBJECT, 15):
        _assert_same(ctx.detect_raw_levels(loaded(xml), img, sf, fl), full, fl)


def test_a_short_output_array_gets_the_first_triples_and_the_full_count(ctx, loaded):
    xml, ref, img, sf = K.natural("lbp-w24")
    exp = K.expected("natural", "lbp-w24")
    cap = 5
    assert len(exp[0]) > cap
    buf, lv, wt, n = (capi.Rect * cap)(), (C.c_int * cap)(), (C.c_double * cap)(), C.c_int()
    g = np.ascontiguousarray(img)
    ctx.check(ctx.L.nvca_detect_raw_levels(ctx.h, loaded(xml).h, g.ctypes.data, g.shape[1], g.shape[0], g.strides[0], capi.MEM_HOST, sf, 0, 0, 0, 0, 0,
                                           buf, lv, wt, cap, C.byref(n)))
    assert n.value == len(exp[0])
    _assert_same((np.frombuffer(buf, np.int32).reshape(-1, 4), np.array(lv[:], np.int32), np.array(wt[:], np.float64)),
                 (exp[0][:cap], exp[1][:cap], exp[2][:cap]), "cap")
    ctx.check(ctx.L.nvca_detect_raw_levels(ctx.h, loaded(xml).h, g.ctypes.data, g.shape[1], g.shape[0], g.strides[0], capi.MEM_HOST, sf, 0, 0, 0, 0, 0,
                                           None, None, None, 0, C.byref(n)))
    assert n.value == len(exp[0])


# ------------------------------------------------------------------ route
@pytest.mark.parametrize("cid", ["lbp-w24", "haar-w24"])
def test_a_levels_job_takes_the_large_image_route(ctx, loaded, cid):
    """97 x 83 fits the small-image route's LDS: a plain scan of an LBP cascade is one NVCA_K_ROI launch there; a levels job is never"""
    xml, ref, img, sf = K.natural(cid)
    ctx.enable_kernel_timing(True)
    try:
        ctx.kernel_timing()
        _assert_same(ctx.detect_raw_levels(loaded(xml), img, sf), K.expected("natural", cid), cid)
        booked = ctx.kernel_timing()          # {kernel name: (ms, launches)} of the slots that launched
    finally:
        ctx.enable_kernel_timing(False)
    assert "cascade_roi" not in booked and booked["cascade_strip"][1] >= 1


@pytest.mark.parametrize("cid", ["lbp-w24", "haar-w24", "lbp-w24-first4"])
def test_plain_scans_around_a_levels_call_answer_as_before(ctx, loaded, cid):
    """one cascade, one geometry, one context: the plan is shared, and a plain job is never handed a levels job's launch set"""
    xml, ref, img, sf = K.natural(cid)
    plain = (V.H if V.is_haar(ref) else V.L).scan(ref, img, sf)
    exp = K.expected("natural", cid)
    assert len(plain) > 0
    for _ in range(2):
        assert np.array_equal(ctx.detect_raw(loaded(xml), img, sf), plain)
        _assert_same(ctx.detect_raw_levels(loaded(xml), img, sf), exp, cid)
    assert np.array_equal(ctx.detect_raw(loaded(xml), img, sf), plain)
    assert np.array_equal(np.asarray(ctx.detect_multiscale(loaded(xml), img, sf, 2), np.int32).reshape(-1, 4),
                          (V.H if V.is_haar(ref) else V.L).detect(ref, img, sf, 2))


# ------------------------------------------------------------------ refusals
def _call(ctx, casc, img, out=True):
    g = np.ascontiguousarray(img)
    cap = 16
    buf, lv, wt, n = (capi.Rect * cap)(), (C.c_int * cap)(), (C.c_double * cap)(), C.c_int()
    a = (ctx.h, casc.h, g.ctypes.data, g.shape[1], g.shape[0], g.strides[0], capi.MEM_HOST, 1.1)
    tails = [(buf, lv, wt, cap, C.byref(n))] if out is True else out(buf, lv, wt, cap, C.byref(n))
    return [(ctx.L.nvca_detect_raw_levels(*a, 0, 0, 0, 0, 0, *t), ctx.L.nvca_detect_multiscale_levels(*a, 3, 0, 0, 0, 0, 0, *t)) for t in tails]


def test_an_old_format_cascade_is_refused(ctx, synth_xml):
    casc = ctx.load_cascade_xml(synth_xml)
    try:
        assert _call(ctx, casc, LK.image(97, 83, 24, 24)) == [(capi.ERR_UNSUPPORTED, capi.ERR_UNSUPPORTED)]
        assert ctx.L.nvca_last_error(ctx.h)
    finally:
        casc.free()


@pytest.mark.parametrize("kind", [K.LBP, K.HAAR])
def test_a_cascade_of_three_stages_is_refused(ctx, kind):
    casc = ctx.load_cascade_xml(K.to_xml(kind, K.truncated(kind, "w24", 3)))
    try:
        assert _call(ctx, casc, LK.image(97, 83, 24, 24)) == [(capi.ERR_UNSUPPORTED, capi.ERR_UNSUPPORTED)]
        # ... by the new entry points only
        assert len(ctx.detect_raw(casc, LK.image(97, 83, 24, 24), 1.1)) > 0
    finally:
        casc.free()


def test_null_output_arrays_are_refused(ctx, loaded):
    xml, ref, img, sf = K.natural("lbp-w24")
    got = _call(ctx, loaded(xml), img, lambda buf, lv, wt, cap, n: [(None, lv, wt, cap, n), (buf, None, wt, cap, n), (buf, lv, None, cap, n),
                                                                    (buf, lv, wt, cap, None), (buf, lv, wt, -1, n)])
    assert got == [(capi.ERR_ARG, capi.ERR_ARG)] * 5
