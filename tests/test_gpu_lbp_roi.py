"""The small-image route of new-format LBP cascades on the device (csrc/kernels_roi_lbp.hip, launched by roi_batch.cpp beside k_roi)
against the numpy statement of SURVEY.md A.15 (tests/lbp_reference.py) and the closed forms of tests/lbp_roi_cases.py: bit for bit, raw
lists and grouped boxes, from host memory, from device memory and as a sub-matrix of a larger device image.  Which route answered is
read from the kernel timers: the small route books cascade_roi, the large one cascade_strip.  tests/test_lbp_roi_cpu.py asserts on the
statement alone that the cases are in the regimes they are named for."""
import ctypes as C

import numpy as np
import pytest

import lbp_cases as K
import lbp_reference as R
import lbp_roi_cases as RC
import orc
from nubovca import capi, synth
from test_gpu_lbp import FLAGS

pytestmark = pytest.mark.gpu
CAP = 1 << 16


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def loaded(ctx):
    """xml text -> the device's cascade, loaded once"""
    cache = {}

    def get(xml):
        if xml not in cache:
            cache[xml] = ctx.load_cascade_xml(xml)
        return cache[xml]
    yield get
    for c in cache.values():
        c.free()


def _layouts(gray):
    """(name, keep-alive, pointer, stride, mem): host memory, device memory, a sub-matrix of a larger device image at a padded stride
    and an odd column offset (what a part detector's search region is)"""
    import torch
    rows, cols = gray.shape
    host = np.ascontiguousarray(gray)
    dev = torch.from_numpy(host).cuda()
    big = np.full((rows + 5, cols + 41), 173, np.uint8)
    big[2:2 + rows, 3:3 + cols] = gray
    dbig = torch.from_numpy(big).cuda()
    torch.cuda.synchronize()
    return [("host", host, host.ctypes.data, cols, capi.MEM_HOST), ("device", dev, dev.data_ptr(), cols, capi.MEM_DEVICE),
            ("sub-matrix", dbig, dbig.data_ptr() + 2 * (cols + 41) + 3, cols + 41, capi.MEM_DEVICE)]


def _raw(ctx, casc, ptr, cols, rows, stride, mem, sf, flags=0, mins=(0, 0), maxs=(0, 0)):
    buf, n = (capi.Rect * CAP)(), C.c_int()
    ctx.check(ctx.L.nvca_detect_raw(ctx.h, casc.h, ptr, cols, rows, stride, mem, sf, flags, mins[0], mins[1], maxs[0], maxs[1], buf, CAP, C.byref(n)))
    return np.frombuffer(buf, np.int32).reshape(-1, 4)[:n.value].copy()


def _grouped(ctx, casc, ptr, cols, rows, stride, mem, sf, mn, flags=0, mins=(0, 0), maxs=(0, 0)):
    buf, n = (capi.Rect * CAP)(), C.c_int()
    ctx.check(ctx.L.nvca_detect_multiscale(ctx.h, casc.h, ptr, cols, rows, stride, mem, sf, mn, flags, mins[0], mins[1], maxs[0], maxs[1], buf, CAP, C.byref(n)))
    return np.frombuffer(buf, np.int32).reshape(-1, 4)[:n.value].copy()


def _expected_grouped(raw, mn):
    if mn == 0 or len(raw) == 0:
        return raw
    return np.asarray(orc.group_rectangles(raw, max(mn, 1), 0.2)[0], np.int32).reshape(-1, 4)


def _booked(ctx, fn):
    """the timing slots whose launch count moved while fn ran"""
    ctx.enable_kernel_timing(1)
    before = ctx.kernel_timing()
    out = fn()
    after = ctx.kernel_timing()
    ctx.enable_kernel_timing(0)
    return out, {k for k, v in after.items() if v[1] > before.get(k, (0, 0))[1]}


def _check_everywhere(ctx, casc, gray, sf, mins, maxs, exp, small=True):
    """raw list and grouped boxes (min_neighbors 0, 1, 3) in every layout, on the route the case is named for and with roi = 0"""
    exp = np.asarray(exp, np.int32).reshape(-1, 4)
    rows, cols = gray.shape
    for name, _keep, ptr, stride, mem in _layouts(gray):
        for on in (1, 0):
            with ctx.options(roi=on):
                got, booked = _booked(ctx, lambda: _raw(ctx, casc, ptr, cols, rows, stride, mem, sf, 0, mins, maxs))
                assert got.shape == exp.shape and np.array_equal(got, exp), (name, on)
                if len(R.levels(*_size(casc), cols, rows, sf, mins, maxs)):            # (a call without a level launches nothing)
                    want = "cascade_roi" if on and small else "cascade_strip"
                    other = "cascade_strip" if on and small else "cascade_roi"
                    assert want in booked and other not in booked, (name, on, booked)
                for mn in (0, 1, 3):
                    assert np.array_equal(_grouped(ctx, casc, ptr, cols, rows, stride, mem, sf, mn, 0, mins, maxs), _expected_grouped(exp, mn)), (name, on, mn)


def _size(casc):
    return casc.info()[:2]


# ------------------------------------------------------------------ every constructed case, bit for bit, on both routes
@pytest.mark.parametrize("case", RC.hand_cases(), ids=[c[0] for c in RC.hand_cases()])
def test_hand_cases(ctx, loaded, case):
    _, cdict, gray, sf, mins, maxs, exp = case
    _check_everywhere(ctx, loaded(RC.hand_xml(cdict)), gray, sf, mins, maxs, exp)


@pytest.mark.parametrize("cid", [c[0] for c in RC.NAMED])
def test_named_cases(ctx, loaded, cid):
    xml, gray, sf, exp, _stats = RC.named_case(cid)
    assert len(exp) > 0
    _check_everywhere(ctx, loaded(xml), gray, sf, (0, 0), (0, 0), exp)


def test_min_and_max_size_on_the_small_route(ctx, loaded):
    xml, ref = K.cascade("w12")
    gray = K.image(97, 83, 12, 12)
    full = K.expected_raw("w12", 97, 83, 1.1)
    for mins, maxs in (((16, 16), (0, 0)), ((0, 0), (30, 30)), ((16, 16), (30, 30))):
        exp = K.expected_raw("w12", 97, 83, 1.1, mins, maxs)
        assert 0 < len(exp) < len(full)
        _check_everywhere(ctx, loaded(xml), gray, 1.1, mins, maxs, exp)


# ------------------------------------------------------------------ the bound, the key, the switches
def test_images_on_both_sides_of_the_lds_bound(ctx, loaded):
    xml, ref = K.cascade("w24")
    for (cols, rows), small in zip(RC.bound_images(), (True, False)):
        gray = K.image(cols, rows, 24, 24)
        exp = R.scan(ref, gray, 1.3)
        assert len(exp) > 0
        _check_everywhere(ctx, loaded(xml), gray, 1.3, (0, 0), (0, 0), exp, small=small)


def test_more_levels_than_the_key_holds_takes_the_large_route(ctx, loaded):
    """more than 63 levels (96): the job does not fit the small route's key; the large route answers it in full, the statement's list,
    as with roi = 0"""
    name, cols, rows, sf = RC.TOO_MANY_LEVELS
    xml, ref = K.cascade(name)
    gray = K.image(cols, rows, *ref.size)
    exp = R.scan(ref, gray, sf)
    assert len(R.levels(*ref.size, cols, rows, sf)) > 63 and len(exp) > 0
    for on in (1, 0):
        with ctx.options(roi=on):
            buf, n = (capi.Rect * CAP)(), C.c_int()
            rc, booked = _booked(ctx, lambda: ctx.L.nvca_detect_raw(ctx.h, loaded(xml).h, gray.ctypes.data, cols, rows, cols, capi.MEM_HOST, sf, 0, 0, 0, 0, 0, buf, CAP, C.byref(n)))
            assert rc == capi.OK, (on, rc, ctx.L.nvca_last_error(ctx.h))
            assert "cascade_roi" not in booked and "cascade_strip" in booked, (on, booked)
            got = np.frombuffer(buf, np.int32).reshape(-1, 4)[:max(n.value, 0)].copy()
            assert got.shape == exp.shape and np.array_equal(got, exp), on
    # and the context goes on answering on the small route
    exp = K.expected_raw(name, cols, rows, 1.1)
    got, booked = _booked(ctx, lambda: np.asarray(ctx.detect_raw(loaded(xml), gray, 1.1), np.int32).reshape(-1, 4))
    assert np.array_equal(got, exp) and "cascade_roi" in booked


def test_roi_switch_turns_the_route_off_and_on(ctx, loaded):
    """the route has no switch of its own: "roi" = 0 sends small LBP images down the large-image route as it does small Haar images"""
    xml, gray, sf, exp, _ = RC.named_case("single-band-w12-97x83")
    for opts, small in (({"roi": 0}, False), ({"roi": 1}, True), ({"roi": 0}, False), ({}, True)):
        with ctx.options(**opts):
            got, booked = _booked(ctx, lambda: np.asarray(ctx.detect_raw(loaded(xml), gray, sf), np.int32).reshape(-1, 4))
        assert np.array_equal(got, exp), opts
        assert ("cascade_roi" in booked) == small and ("cascade_strip" in booked) == (not small), (opts, booked)
    assert ctx.get_option("roi") == 1


def test_every_flags_value_answers_as_zero(ctx, loaded):
    xml, gray, sf, exp, _ = RC.named_case("single-band-w12-97x83")
    rows, cols = gray.shape
    for fl in FLAGS:
        for name, _keep, ptr, stride, mem in _layouts(gray)[:2]:
            got, booked = _booked(ctx, lambda: _raw(ctx, loaded(xml), ptr, cols, rows, stride, mem, sf, fl))
            assert np.array_equal(got, exp) and "cascade_roi" in booked and "cascade_strip" not in booked, (fl, name)
            assert np.array_equal(_grouped(ctx, loaded(xml), ptr, cols, rows, stride, mem, sf, 3, fl), _expected_grouped(exp, 3)), (fl, name)


def test_candidate_overflow_rerun_answers_exactly(ctx, loaded):
    """a permissive 12 x 12 cascade on 60 x 60 with room for 64 candidates: the complete list comes back through the re-run"""
    cdict = K.permissive(12, 12)
    ref = R.parse_xml(RC.hand_xml(cdict))
    gray = np.full((60, 60), 120, np.uint8)
    exp = R.scan(ref, gray, 1.2)
    assert len(exp) > 640
    ctx.set_hit_capacity(64)
    try:
        got, booked = _booked(ctx, lambda: np.asarray(ctx.detect_raw(loaded(RC.hand_xml(cdict)), gray, 1.2), np.int32).reshape(-1, 4))
        assert np.array_equal(got, exp) and "cascade_roi" in booked and "cascade_strip" not in booked
        assert np.array_equal(np.asarray(ctx.detect_multiscale(loaded(RC.hand_xml(cdict)), gray, 1.2, 3, cap=CAP), np.int32).reshape(-1, 4), _expected_grouped(exp, 3))
    finally:
        ctx.set_hit_capacity(16384)


def test_haar_and_lbp_small_calls_alternate_on_one_context(ctx, loaded, synth_xml, orc_cascade):
    haar = ctx.load_cascade_xml(synth_xml)
    xml, gray, sf, exp, _ = RC.named_case("single-band-w12-97x83")
    hg = synth.make_gray(120, 90, 5, "natural", [(30, 20, 48)])
    for _ in range(2):
        for fl in (0, capi.HAAR_SCALE_IMAGE, capi.HAAR_FIND_BIGGEST_OBJECT):
            assert np.array_equal(ctx.detect_multiscale(haar, hg, 1.2, 2, fl), orc.detect_multiscale(orc_cascade, hg, 1.2, 2, fl)), fl
            assert np.array_equal(np.asarray(ctx.detect_raw(loaded(xml), gray, sf), np.int32).reshape(-1, 4), exp)
    haar.free()
