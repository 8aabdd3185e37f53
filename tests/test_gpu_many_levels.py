"""Pyramid scans of more than 63 levels on the device, held to the statements bit for bit: equal shape, then np.array_equal.  The
large-image routes (si_plan in csrc/detect_job.cpp for CV_HAAR_SCALE_IMAGE on old-format cascades, lbp_plan in csrc/lbp_job.cpp for every
scan of a new-format LBP or HAAR cascade: single images, batches, reject levels, face streams, part streams) build every level a call
has; the small-image routes decline a job of more than 63 steps and hand it to them.  The cases are tests/many_levels_cases.py's;
tests/test_many_levels_cpu.py asserts on the statements alone that each of them has more than 63 levels and answers differently when the
scan is cut after the 63rd -- which a library that stopped there, and said NVCA_OK, once did.  Which route answered is read from the
kernel timers.  What no plan holds comes back as NVCA_ERR_ARG with nvca_last_error set, never as a shorter list."""
import ctypes as C

import numpy as np
import pytest

import lbp_part_cases as LP
import levels_reference as LV
import many_levels_cases as M
import orc
from nubovca import capi

pytestmark = pytest.mark.gpu
CAP = 1 << 16
LARGE = {"cascade_stage0", "cascade_strip", "cascade_tile", "cascade_band"}          # what the large-image routes book their evaluators under


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def loaded(ctx):
    """xml text -> the device's cascade, loaded once; opt_in: a new-format HAAR cascade opted into the small route (another instance)"""
    cache = {}

    def get(xml, opt_in=False):
        if (xml, opt_in) not in cache:
            cache[(xml, opt_in)] = ctx.load_cascade_xml(xml)
            if opt_in:
                cache[(xml, opt_in)].set_small_route(1)
        return cache[(xml, opt_in)]
    yield get
    for c in cache.values():
        c.free()


def _instances(loaded, kind, xml):
    """the cascade as the routes see it: an LBP cascade, or a new-format HAAR one opted into the small route and not"""
    return [loaded(xml)] if kind == M.LBP else [loaded(xml, True), loaded(xml, False)]


def _host(gray):
    g = np.ascontiguousarray(gray)
    return g, g.ctypes.data, g.strides[0], capi.MEM_HOST


def _device(gray):
    import torch
    g = np.ascontiguousarray(gray)
    t = torch.from_numpy(g).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr(), g.strides[0], capi.MEM_DEVICE


def _call(ctx, fn, casc, where, shape, sf, mid, flags, mins, maxs):
    _keep, ptr, stride, mem = where
    rows, cols = shape
    buf, n = (capi.Rect * CAP)(), C.c_int()
    rc = fn(ctx.h, casc.h, ptr, cols, rows, stride, mem, sf, *mid, flags, mins[0], mins[1], maxs[0], maxs[1], buf, CAP, C.byref(n))
    assert rc == capi.OK, (rc, ctx.L.nvca_last_error(ctx.h))
    assert 0 <= n.value <= CAP
    return np.frombuffer(buf, np.int32).reshape(-1, 4)[:n.value].copy()


def _raw(ctx, casc, where, shape, sf, flags=0, mins=(0, 0), maxs=(0, 0)):
    return _call(ctx, ctx.L.nvca_detect_raw, casc, where, shape, sf, (), flags, mins, maxs)


def _grouped(ctx, casc, where, shape, sf, mn, flags=0, mins=(0, 0), maxs=(0, 0)):
    return _call(ctx, ctx.L.nvca_detect_multiscale, casc, where, shape, sf, (mn,), flags, mins, maxs)


def _booked(ctx, fn):
    """the timing slots whose launch count moved while fn ran, with the count"""
    ctx.enable_kernel_timing(1)
    before = ctx.kernel_timing()
    out = fn()
    after = ctx.kernel_timing()
    ctx.enable_kernel_timing(0)
    return out, {k: v[1] - before.get(k, (0, 0))[1] for k, v in after.items() if v[1] > before.get(k, (0, 0))[1]}


def _same(got, exp, what):
    exp = np.asarray(exp, np.int32).reshape(-1, 4)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert np.array_equal(got, exp), what


def _large_only(booked, what):
    assert "cascade_roi" not in booked and LARGE & set(booked), (what, booked)


# ------------------------------------------------------------------ new-format cascades, single images
@pytest.mark.parametrize("cid", sorted(M.SINGLE))
def test_single_image_raw_and_grouped(ctx, loaded, cid):
    kind = M.SINGLE[cid][0]
    xml, _ref, gray, sf, exp = M.single(cid)
    wheres = [("host", _host(gray))] + ([("device", _device(gray))] if cid in M.LAYOUTS else [])
    for casc in _instances(loaded, kind, xml):
        for name, where in wheres:
            for on in (1, 0):
                what = (cid, casc.small_route(), name, on)
                with ctx.options(roi=on):
                    got, booked = _booked(ctx, lambda: _raw(ctx, casc, where, gray.shape, sf))
                    _same(got, exp, what)
                    _large_only(booked, what)
                    assert "cascade_strip" in booked, booked
                    for mn in M.GROUP_THRESHOLDS:
                        _same(_grouped(ctx, casc, where, gray.shape, sf, mn), M.grouped(exp, mn), what + (mn,))


# ------------------------------------------------------------------ the boundary
@pytest.mark.parametrize("kind", [M.LBP, M.HAAR])
def test_63_64_and_65_levels(ctx, loaded, kind):
    """three scans that differ in max_size only.  The LBP one's image is inside the small route's bound: 63 levels are that route's most,
    64 the first job it hands on; the HAAR one's is outside, all three take the large route"""
    xml, _ref, gray, sf, mins, scans = M.boundary(kind)
    where = _host(gray)
    for casc in _instances(loaded, kind, xml):
        for on in (1, 0):
            with ctx.options(roi=on):
                for (maxs, exp), n in zip(scans, M.BOUNDARY_LEVELS):
                    what = (kind, casc.small_route(), on, n)
                    got, booked = _booked(ctx, lambda: _raw(ctx, casc, where, gray.shape, sf, 0, mins, maxs))
                    _same(got, exp, what)
                    if kind == M.LBP and on and n == 63:
                        assert "cascade_roi" in booked and "cascade_strip" not in booked, (what, booked)
                    else:
                        _large_only(booked, what)
                    for mn in M.GROUP_THRESHOLDS:
                        _same(_grouped(ctx, casc, where, gray.shape, sf, mn, 0, mins, maxs), M.grouped(exp, mn), what + (mn,))


# ------------------------------------------------------------------ old-format cascades, CV_HAAR_SCALE_IMAGE
@pytest.mark.parametrize("sf,mins", M.OLD_SCANS)
@pytest.mark.parametrize("which", M.OLD_CASCADES)
def test_old_format_scale_image(ctx, loaded, which, sf, mins):
    casc, oc, gray = loaded(M.old_xml(which)), M.old_cascade(which), M.old_image()
    exp, nlev = M.old_case(which, sf, mins)
    assert nlev > M.KEPT
    where = _host(gray)
    for on in (1, 0):
        with ctx.options(roi=on):
            got, booked = _booked(ctx, lambda: _raw(ctx, casc, where, gray.shape, sf, capi.HAAR_SCALE_IMAGE, mins))
            _same(got, exp, (which, sf, on))
            _large_only(booked, (which, sf, on))
            for mn in M.GROUP_THRESHOLDS:
                _same(_grouped(ctx, casc, where, gray.shape, sf, mn, capi.HAAR_SCALE_IMAGE, mins),
                      orc.detect_multiscale(oc, gray, sf, mn, orc.HAAR_SCALE_IMAGE, mins), (which, sf, on, mn))


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("kind", [M.LBP, M.HAAR])
def test_two_images_in_one_batch_call_in_both_slot_orders(ctx, loaded, kind):
    xml, _ref, grays, sf, exps = M.batch(kind)
    for casc in _instances(loaded, kind, xml):
        for order in (1, -1):
            gs, es = grays[::order], exps[::order]
            got, booked = _booked(ctx, lambda: ctx.detect_raw_batch(casc, gs, sf, cap=CAP))
            _large_only(booked, (kind, order))
            assert len(got) == 2
            for slot in range(2):
                _same(got[slot], es[slot], (kind, order, slot))
            for mn in M.GROUP_THRESHOLDS:
                got = ctx.detect_multiscale_batch(casc, gs, sf, mn, cap=CAP)
                for slot in range(2):
                    _same(got[slot], M.grouped(es[slot], mn), (kind, order, slot, mn))


# ------------------------------------------------------------------ reject levels and level weights
@pytest.mark.parametrize("kind", [M.LBP, M.HAAR])
def test_reject_levels_and_level_weights(ctx, loaded, kind):
    xml, _ref, gray, sf, (rects, levels, weights) = M.levels_case(kind)
    for casc in _instances(loaded, kind, xml):
        (r, l, w), booked = _booked(ctx, lambda: ctx.detect_raw_levels(casc, gray, sf, cap=1 << 18))
        _large_only(booked, kind)
        _same(r, rects, kind)
        assert l.shape == levels.shape and np.array_equal(l, levels) and w.shape == weights.shape and np.array_equal(w, weights)
    cls = LV.classes(rects)
    for mn in M.LEVELS_THRESHOLDS[kind]:
        er, el, ew = LV.group_levels(rects, levels, weights, mn, cls=cls)
        r, l, w = ctx.detect_multiscale_levels(loaded(xml), gray, sf, mn, cap=1 << 18)
        _same(r, er, (kind, mn))
        assert l.shape == el.shape and np.array_equal(l, el) and w.shape == ew.shape and np.array_equal(w, ew), (kind, mn)


# ------------------------------------------------------------------ face streams at multi-scale-factor 1 and 2
def _face_stream(ctx, loaded, kind):
    name, _W, _H, wtp, _ = M.STREAM[kind]
    return capi.FaceStream(ctx, loaded(M.cascade(kind, name)[0]), any_format=True, width_to_process=wtp, multi_scale_factor=M.STREAM_PCT[0],
                           min_neighbors=3, process_x_every_4_frames=4)


def _eq(got, exp, what):
    assert got[0].shape == exp[0].shape and np.array_equal(got[0], exp[0]), (what, got[0].tolist(), exp[0].tolist())
    assert np.array_equal(got[1], exp[1]), (what, got[1].tolist(), exp[1].tolist())


@pytest.mark.parametrize("kind", [M.LBP, M.HAAR])
def test_face_stream_frame_by_frame(ctx, loaded, kind):
    """multi_scale_factor 1 (160 levels), then 2 (81), changed between frames: boxes and ids of every frame"""
    fs, ex = _face_stream(ctx, loaded, kind), M.stream_expected(kind)
    total = {}
    for k, (f, pct) in enumerate(zip(M.stream_frames(kind), M.STREAM_PCT)):
        fs.set_property("multi_scale_factor", pct)
        ex.p.update(scale_factor_pct=pct)
        got, booked = _booked(ctx, lambda: fs.process(np.array(M.STREAM_CASES[kind].bgr(f)), cap=1024))
        exp = ex.process(f)
        assert len(exp[0]) > 0
        _eq(got, exp, (kind, k, pct))
        for name, v in booked.items():
            total[name] = total.get(name, 0) + v
    fs.close()
    _large_only(total, kind)


def test_both_face_streams_in_one_batch_call(ctx, loaded):
    kinds = (M.LBP, M.HAAR)
    streams, expected = [_face_stream(ctx, loaded, k) for k in kinds], [M.stream_expected(k) for k in kinds]
    for r, pct in enumerate(M.STREAM_PCT):
        for s, e in zip(streams, expected):
            s.set_property("multi_scale_factor", pct)
            e.p.update(scale_factor_pct=pct)
        fr = [M.stream_frames(k)[r] for k in kinds]
        res = ctx.face_batch_process(streams, [capi.make_frame(np.array(M.STREAM_CASES[k].bgr(f))) for k, f in zip(kinds, fr)], 1024)
        for i, k in enumerate(kinds):
            _eq(res[i], expected[i].process(fr[i]), (k, r, pct))
    for s in streams:
        s.close()


# ------------------------------------------------------------------ a part stream whose face cascade is LBP
@pytest.mark.skipif(LP.shim() is None, reason="no clang++")
@pytest.mark.parametrize("roi", [1, 0])
def test_part_stream_face_pass_of_81_levels(ctx, loaded, roi):
    """the nose stream at scale_factor_pct 2: its face pass leaves the small route (at 25 it is a small job), its part searches stay"""
    exp, _ = M.part_expected()
    cascs = [loaded(LP.K.cascade(n)[0]) for n in (LP.FACE, LP.PART_A)]
    total = {}
    with ctx.options(roi=roi):
        s = capi.PartStream(ctx, LP.KINDS[M.PART_KIND], cascs[0], cascs[1], None, any_format=True, multi_scale_factor=M.PART_PCT)
        for i, f in enumerate(M.part_frames()):
            got, booked = _booked(ctx, lambda: s.process(f, cap=256))
            assert np.array_equal(got[0], exp[i][0]) and np.array_equal(got[1], exp[i][1]), (roi, i, got[0].tolist(), exp[i][0].tolist())
            for name, v in booked.items():
                total[name] = total.get(name, 0) + v
        s.close()
    assert total.get("cascade_strip", 0) >= M.PART_FRAMES, total                    # a face pass a frame
    assert ("cascade_roi" in total) == bool(roi), total


# ------------------------------------------------------------------ what no plan holds is refused, loudly
def _refused(ctx, call):
    buf, n = (capi.Rect * 64)(), C.c_int(-7)
    rc = call(buf, n)
    assert rc == capi.ERR_ARG, rc
    msg = ctx.L.nvca_last_error(ctx.h)
    assert msg and b"scan too large" in msg, msg
    return msg


def test_more_levels_than_a_plan_holds_is_an_error_not_a_shorter_list(ctx, loaded):
    """a scale factor of 1.0001: thousands of levels.  NVCA_ERR_ARG from either pyramid plan, with roi on and off, and the context
    goes on answering"""
    lbp = loaded(M.cascade(M.LBP, "w12")[0])
    hnew = loaded(M.cascade(M.HAAR, "w12")[0], True)
    old = loaded(M.old_xml("small"))
    g = np.full((50, 50), 120, np.uint8)
    L = ctx.L
    for on in (1, 0):
        with ctx.options(roi=on):
            for casc, flags in ((lbp, 0), (hnew, 0), (old, capi.HAAR_SCALE_IMAGE)):
                msg = _refused(ctx, lambda buf, n: L.nvca_detect_raw(ctx.h, casc.h, g.ctypes.data, 50, 50, 50, capi.MEM_HOST, 1.0001, flags, 0, 0, 0, 0, buf, 64, C.byref(n)))
                assert b"4095" in msg
                _refused(ctx, lambda buf, n: L.nvca_detect_multiscale(ctx.h, casc.h, g.ctypes.data, 50, 50, 50, capi.MEM_HOST, 1.0001, 3, flags, 0, 0, 0, 0, buf, 64, C.byref(n)))
    xml, _ref, gray, sf, exp = M.single("lbp-w12-97x83-1.02")
    _same(_raw(ctx, lbp, _host(gray), gray.shape, sf), exp, "afterwards")


def test_pyramid_planes_beyond_int_offsets_are_refused(ctx, loaded):
    """3000 x 3000 at 1.002: 2763 levels whose planes, each at the full image's pitch, pass 2^31 elements -- refused before anything is built"""
    lbp = loaded(M.cascade(M.LBP, "w12")[0])
    g = np.zeros((3000, 3000), np.uint8)
    msg = _refused(ctx, lambda buf, n: ctx.L.nvca_detect_raw(ctx.h, lbp.h, g.ctypes.data, 3000, 3000, 3000, capi.MEM_HOST, 1.002, 0, 0, 0, 0, 0, buf, 64, C.byref(n)))
    assert b"2^31" in msg


def test_levels_times_images_beyond_one_launch_is_refused(ctx, loaded):
    """32 images of 30 x 30 at 1.0004: 2291 levels an image, more (level, image) pairs than the one-launch resize's grid holds"""
    lbp = loaded(M.cascade(M.LBP, "w12")[0])
    gs = [np.full((30, 30), 100 + k, np.uint8) for k in range(32)]
    ptrs = (C.c_void_p * 32)(*[g.ctypes.data for g in gs])
    buf, cnt = (capi.Rect * (64 * 32))(), (C.c_int * 32)()
    rc = ctx.L.nvca_detect_raw_batch(ctx.h, lbp.h, 32, ptrs, 30, 30, 30, capi.MEM_HOST, 1.0004, 0, 0, 0, 0, 0, buf, 64, cnt)
    msg = ctx.L.nvca_last_error(ctx.h)
    assert rc == capi.ERR_ARG and msg and b"65535" in msg, (rc, msg)
    xml, _ref, gray, sf, exp = M.single("lbp-w12-97x83-1.02")
    _same(_raw(ctx, lbp, _host(gray), gray.shape, sf), exp, "afterwards")
