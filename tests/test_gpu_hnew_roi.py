"""The small-image route of new-format HAAR cascades on the device (csrc/kernels_roi_hnew.hip, launched by roi_batch.cpp beside k_roi
and k_roi_lbp for the cascades opted in through nvca_cascade_set_small_route) against the numpy statement of SURVEY.md A.16
(tests/haar_new_reference.py) and the closed forms of tests/hnew_roi_cases.py: bit for bit, raw lists and grouped boxes, from host
memory, from device memory and as a sub-matrix of a larger device image, with roi 1 and 0.  Which route answered is read from the kernel
timers: the small route books cascade_roi, the large one cascade_strip.  A cascade nobody opted in keeps the large route and gives the
same answers.  tests/test_hnew_roi_cpu.py asserts on the statement alone that the cases are in the regimes they are named for."""
import ctypes as C
import functools

import numpy as np
import pytest

import haar_new_cases as K
import haar_new_reference as R
import haar_new_stream_cases as S
import hnew_roi_cases as RC
import lbp_cases as LK
import lbp_part_cases as LP
import lbp_reference as LBR
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
    """xml text -> the device's cascade, loaded once and opted in; loaded(xml, False): another instance, never opted in"""
    cache = {}

    def get(xml, opt_in=True):
        if (xml, opt_in) not in cache:
            cache[(xml, opt_in)] = ctx.load_cascade_xml(xml)
            if opt_in:
                cache[(xml, opt_in)].set_small_route(1)
        return cache[(xml, opt_in)]
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
    """the timing slots whose launch count moved while fn ran, with the count"""
    ctx.enable_kernel_timing(1)
    before = ctx.kernel_timing()
    out = fn()
    after = ctx.kernel_timing()
    ctx.enable_kernel_timing(0)
    return out, {k: v[1] - before.get(k, (0, 0))[1] for k, v in after.items() if v[1] > before.get(k, (0, 0))[1]}


def _size(casc):
    return casc.info()[:2]


def _check_everywhere(ctx, casc, gray, sf, mins, maxs, exp, small=True):
    """raw list and grouped boxes (min_neighbors 0, 1, 3) in every layout, on the route the case is named for and with roi = 0"""
    exp = np.asarray(exp, np.int32).reshape(-1, 4)
    rows, cols = gray.shape
    levels = len(LBR.levels(*_size(casc), cols, rows, sf, mins, maxs))
    for name, _keep, ptr, stride, mem in _layouts(gray):
        for on in (1, 0):
            with ctx.options(roi=on):
                got, booked = _booked(ctx, lambda: _raw(ctx, casc, ptr, cols, rows, stride, mem, sf, 0, mins, maxs))
                assert got.shape == exp.shape and np.array_equal(got, exp), (name, on)
                if levels:            # (a call without a level launches nothing)
                    want = "cascade_roi" if on and small else "cascade_strip"
                    other = "cascade_strip" if on and small else "cascade_roi"
                    assert want in booked and other not in booked, (name, on, booked)
                    if on and small:
                        assert booked["cascade_roi"] == 1, booked          # one launch for the whole job
                for mn in (0, 1, 3):
                    assert np.array_equal(_grouped(ctx, casc, ptr, cols, rows, stride, mem, sf, mn, 0, mins, maxs), _expected_grouped(exp, mn)), (name, on, mn)


# ------------------------------------------------------------------ every constructed case, bit for bit, on both routes
@pytest.mark.parametrize("case", RC.hand_cases(), ids=[c[0] for c in RC.hand_cases()])
def test_hand_cases(ctx, loaded, case):
    _, cdict, gray, sf, mins, maxs, exp = case
    _check_everywhere(ctx, loaded(RC.hand_xml(cdict)), gray, sf, mins, maxs, exp)


@pytest.mark.parametrize("cid", [c[0] for c in RC.NAMED])
def test_named_cases(ctx, loaded, cid):
    xml, gray, sf, exp, stats = RC.named_case(cid)
    assert len(exp) == RC.NAMED_WINDOWS[cid] and stats["nf_nonpositive"] > 0
    _check_everywhere(ctx, loaded(xml), gray, sf, (0, 0), (0, 0), exp)


def test_stages_wider_than_the_vote_area(ctx, loaded):
    """stages of 70 and 130 stumps on short queues: chunks of stumps, the partial sum carried from chunk to chunk"""
    xml, gray, sf, exp = RC.wide_case()
    assert len(exp) > 3000
    _check_everywhere(ctx, loaded(xml), gray, sf, (0, 0), (0, 0), exp)


def test_bright_image_squared_sums_near_their_largest(ctx, loaded):
    xml, gray, sf, exp, _ = RC.bright_case()
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


# ------------------------------------------------------------------ the bound, the key, the opt-in, the switches
def test_images_on_both_sides_of_the_lds_bound(ctx, loaded):
    xml, ref = K.cascade("w24")
    for (cols, rows), small, n in zip(RC.bound_images(), (True, False), (126, 103)):
        gray = K.image(cols, rows, 24, 24)
        exp = R.scan(ref, gray, RC.BOUND_SF)
        assert len(exp) == n
        _check_everywhere(ctx, loaded(xml), gray, RC.BOUND_SF, (0, 0), (0, 0), exp, small=small)


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


def test_a_cascade_not_opted_in_keeps_the_large_route(ctx, loaded):
    """the same file loaded twice: the instance nobody opted in books cascade_strip only, whatever the other's flag, and answers the same"""
    xml, gray, sf, exp, _ = RC.named_case("single-band-w12-97x83")
    rows, cols = gray.shape
    plain, opted = loaded(xml, False), loaded(xml)
    assert plain.small_route() is False and opted.small_route() is True
    for name, _keep, ptr, stride, mem in _layouts(gray):
        got, booked = _booked(ctx, lambda: _raw(ctx, plain, ptr, cols, rows, stride, mem, sf))
        assert np.array_equal(got, exp) and "cascade_strip" in booked and "cascade_roi" not in booked, (name, booked)
        got, booked = _booked(ctx, lambda: _raw(ctx, opted, ptr, cols, rows, stride, mem, sf))
        assert np.array_equal(got, exp) and "cascade_roi" in booked and "cascade_strip" not in booked, (name, booked)
        for mn in (0, 1, 3):
            assert np.array_equal(_grouped(ctx, plain, ptr, cols, rows, stride, mem, sf, mn), _expected_grouped(exp, mn)), (name, mn)


def test_the_flag_moves_the_route_not_the_answer(ctx):
    xml, gray, sf, exp, _ = RC.named_case("single-band-w12-97x83")
    c = ctx.load_cascade_xml(xml)
    L = ctx.L
    v = C.c_int(-1)
    assert L.nvca_cascade_get_small_route(c.h, C.byref(v)) == capi.OK and v.value == 0           # the default
    for on, want in ((1, True), (0, False), (1, True), (7, True), (0, False)):
        assert L.nvca_cascade_set_small_route(c.h, on) == capi.OK
        assert L.nvca_cascade_get_small_route(c.h, C.byref(v)) == capi.OK and v.value == int(want) and c.small_route() is want
        got, booked = _booked(ctx, lambda: np.asarray(ctx.detect_raw(c, gray, sf), np.int32).reshape(-1, 4))
        assert np.array_equal(got, exp), on
        assert ("cascade_roi" in booked) == want and ("cascade_strip" in booked) == (not want), (on, booked)
    assert L.nvca_cascade_set_small_route(None, 1) == capi.ERR_ARG and L.nvca_cascade_get_small_route(None, C.byref(v)) == capi.ERR_ARG
    assert L.nvca_cascade_get_small_route(c.h, None) == capi.ERR_ARG
    c.free()


def test_setter_on_the_other_formats_changes_nothing(ctx, synth_xml, orc_cascade):
    """an old-format and an LBP cascade: OK, the getter says 1 before and after, the small route and the answer stay"""
    haar = ctx.load_cascade_xml(synth_xml)
    lxml, lref = LK.cascade("w12")
    lbp = ctx.load_cascade_xml(lxml)
    lgray = LK.image(97, 83, 12, 12)
    lexp = LK.expected_raw("w12", 97, 83, 1.1)
    hg = synth.make_gray(120, 90, 5, "natural", [(30, 20, 48)])
    hexp = orc.detect_multiscale(orc_cascade, hg, 1.2, 2, capi.HAAR_SCALE_IMAGE)
    for on in (None, 0, 1, 0):
        for c in (haar, lbp):
            if on is not None:
                assert ctx.L.nvca_cascade_set_small_route(c.h, on) == capi.OK
            assert c.small_route() is True
        got, booked = _booked(ctx, lambda: np.asarray(ctx.detect_raw(lbp, lgray, 1.1), np.int32).reshape(-1, 4))
        assert np.array_equal(got, lexp) and "cascade_roi" in booked and "cascade_strip" not in booked, (on, booked)
        got, booked = _booked(ctx, lambda: ctx.detect_multiscale(haar, hg, 1.2, 2, capi.HAAR_SCALE_IMAGE))
        assert np.array_equal(got, hexp) and "cascade_roi" in booked and "cascade_strip" not in booked, (on, booked)
    haar.free(); lbp.free()


def test_roi_switch_turns_the_route_off_and_on(ctx, loaded):
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


def test_a_levels_call_on_an_opted_in_cascade_takes_the_large_route(ctx, loaded):
    """nvca_detect_raw_levels (outputRejectLevels): k_roi_hnew has no last-stages launch"""
    import levels_reference as LV
    xml, gray, sf, _exp, _ = RC.named_case("single-band-w12-97x83")
    ref = K.cascade("w12")[1]
    rows, cols = gray.shape
    assert loaded(xml).small_route() is True
    want = LV.scan_levels(ref, gray, sf)
    (rects, levels, weights), booked = _booked(ctx, lambda: ctx.detect_raw_levels(loaded(xml), gray, sf, cap=CAP))
    assert "cascade_strip" in booked and "cascade_roi" not in booked, booked
    assert np.array_equal(rects, want[0]) and np.array_equal(levels, want[1]) and np.array_equal(weights, want[2])


def test_three_kinds_of_small_calls_alternate_on_one_context(ctx, loaded, synth_xml, orc_cascade):
    """old-format Haar, LBP and opted-in new-format HAAR small calls in turn: three kernels, one set of launch buffers"""
    haar = ctx.load_cascade_xml(synth_xml)
    lbp = ctx.load_cascade_xml(LK.cascade("w12")[0])
    lgray, lexp = LK.image(97, 83, 12, 12), LK.expected_raw("w12", 97, 83, 1.1)
    xml, gray, sf, exp, _ = RC.named_case("single-band-w12-97x83")
    hg = synth.make_gray(120, 90, 5, "natural", [(30, 20, 48)])
    for _ in range(2):
        for fl in (0, capi.HAAR_SCALE_IMAGE, capi.HAAR_FIND_BIGGEST_OBJECT):
            assert np.array_equal(ctx.detect_multiscale(haar, hg, 1.2, 2, fl), orc.detect_multiscale(orc_cascade, hg, 1.2, 2, fl)), fl
            got, booked = _booked(ctx, lambda: np.asarray(ctx.detect_raw(loaded(xml), gray, sf), np.int32).reshape(-1, 4))
            assert np.array_equal(got, exp) and booked.get("cascade_roi") == 1 and "cascade_strip" not in booked
            assert np.array_equal(np.asarray(ctx.detect_raw(lbp, lgray, 1.1), np.int32).reshape(-1, 4), lexp)
    haar.free(); lbp.free()


# ------------------------------------------------------------------ part streams (the harness of haar_new_stream_cases.py / lbp_part_cases.py)
# kind -> the new-format HAAR cascades of (face, a, b), every one opted in
ALL_HNEW = {"eye": ("w24", "w12", "w12"), "ear": ("w24", "w12", "w20x28"), "nose": ("w24", "w12", None), "mouth": ("w24", "w20x28", None)}
needs_shim = pytest.mark.skipif(LP.shim() is None, reason="no clang++")
PCAP = 256


@functools.lru_cache(maxsize=None)
def _hnew_expected(kind):
    """([(list a, list b)] per frame of haar_new_stream_cases.part_frames(), the detectors with the sizes they saw)"""
    dets = tuple(S.hnew_detector(K.cascade(n)[1]) if n else None for n in ALL_HNEW[kind])
    h = LP.Harness(kind, *dets)
    out = [h.process(f) for f in S.part_frames()]
    h.close()
    return out, dets


def _hnew_stream(ctx, loaded, kind):
    cascs = [loaded(K.cascade(n)[0]) if n else None for n in ALL_HNEW[kind]]
    assert all(c is None or (c.format()[0] == capi.CASCADE_HAAR_NEW and c.small_route()) for c in cascs)
    return capi.PartStream(ctx, LP.KINDS[kind], cascs[0], cascs[1], cascs[2], any_format=True)


def _mixed_stream(ctx, loaded, kind, opt_in=True):
    """haar_new_stream_cases.PART_ROLES: three roles of three formats, the new-format HAAR one opted in (or not); (stream, cascades to free)"""
    own = []
    cascs = []
    for role in S.PART_ROLES[kind]:
        if role[0] == "hnew":
            cascs.append(loaded(S.part_xml(role), opt_in))
        else:
            own.append(ctx.load_cascade_xml(S.part_xml(role)))
            cascs.append(own[-1])
    return capi.PartStream(ctx, LP.KINDS[kind], cascs[0], cascs[1], cascs[2], any_format=True), own


def _same(got, exp, what):
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (what, got[0].tolist(), exp[0].tolist(), got[1].tolist(), exp[1].tolist())


@needs_shim
@pytest.mark.parametrize("kind", ["eye", "ear"])
@pytest.mark.parametrize("roi", [1, 0])
def test_part_stream_with_every_role_opted_in(ctx, loaded, kind, roi):
    """frame by frame against the harness; the part searches -- regions of a few thousand pixels -- book cascade_roi, the 160 x 120
    face pass (outside the bound) cascade_strip; with roi = 0 nothing books cascade_roi"""
    exp, dets = _hnew_expected(kind)
    assert all(len(d.seen) > 0 for d in dets)                       # every role searched
    assert all(RC.fits_lds(w, h) for d in dets[1:] for (w, h) in d.seen) and not any(RC.fits_lds(w, h) for (w, h) in dets[0].seen)
    if kind == "ear":
        assert sum(len(a) for a, b in exp) > 0 and sum(len(b) for a, b in exp) > 0
    with ctx.options(roi=roi):
        s = _hnew_stream(ctx, loaded, kind)
        total = {}
        for i, f in enumerate(S.part_frames()):
            got, booked = _booked(ctx, lambda: s.process(f, cap=PCAP))
            _same(got, exp[i], (kind, roi, i))
            for k, v in booked.items():
                total[k] = total.get(k, 0) + v
        s.close()
    if roi:
        assert total.get("cascade_roi", 0) > 0, total
    else:
        assert "cascade_roi" not in total and total.get("cascade_strip", 0) > 0, total


@needs_shim
@pytest.mark.parametrize("kind", sorted(S.PART_ROLES))
def test_part_stream_with_three_roles_in_three_formats_one_opted_in(ctx, loaded, kind):
    """the same answers with the new-format HAAR cascade opted in and not; "ear" has it in a part role, on regions that are inside the bound but for one:
    opted in, its searches leave the large-image route (fewer cascade_strip bookings over the frames, the rest being the mirrored face
    pass, a two-image job) for the small-image rounds the stream books anyway.  "eye" has it in the face role, on the 160 x 120 image
    outside the bound: nothing moves"""
    exp, dets = S.part_expected(kind)
    assert all(len(d.seen) > 0 for d in dets)
    hnew_role = [r[0] for r in S.PART_ROLES[kind]].index("hnew")
    inside = [RC.fits_lds(w, h) for (w, h) in dets[hnew_role].seen]
    assert sum(inside) > len(inside) // 2 if kind == "ear" else not any(inside)          # ("ear": all of its regions but the largest, 98 x 156)
    totals = []
    for opt_in in (False, True):
        s, own = _mixed_stream(ctx, loaded, kind, opt_in)
        total = {}
        for i, f in enumerate(S.part_frames()):
            got, booked = _booked(ctx, lambda: s.process(f, cap=PCAP))
            _same(got, exp[i], (kind, opt_in, i))
            for k, v in booked.items():
                total[k] = total.get(k, 0) + v
        s.close()
        for c in own:
            c.free()
        totals.append(total)
    plain, opted = totals
    assert plain.get("cascade_roi", 0) > 0 and opted.get("cascade_roi", 0) > 0, totals
    if kind == "ear":
        assert opted.get("cascade_strip", 0) < plain.get("cascade_strip", 0), totals
    else:
        assert opted.get("cascade_strip", 0) == plain.get("cascade_strip", 0) > 0, totals


def _eight(ctx, loaded):
    """(stream, cascades to free, expected lists) x 8: the four kinds with every role opted in, the two three-format mixtures, and a
    second ear and a second eye stream"""
    out = []
    for kind in ("eye", "ear", "nose", "mouth"):
        out.append((_hnew_stream(ctx, loaded, kind), [], _hnew_expected(kind)[0]))
    for kind in ("eye", "ear"):
        s, own = _mixed_stream(ctx, loaded, kind)
        out.append((s, own, S.part_expected(kind)[0]))
    out.append((_hnew_stream(ctx, loaded, "ear"), [], _hnew_expected("ear")[0]))
    out.append((_hnew_stream(ctx, loaded, "eye"), [], _hnew_expected("eye")[0]))
    return out


@needs_shim
def test_eight_streams_in_one_call_in_both_slot_orders(ctx, loaded):
    """every stream's lists are those of the stream alone, in either slot order, and the small jobs of a search phase -- old-format,
    LBP and new-format HAAR -- share small-image rounds: far fewer cascade_roi bookings than streams and searches"""
    frames = S.part_frames()[:3]
    for order in (1, -1):
        eight = _eight(ctx, loaded)[::order]
        for i, f in enumerate(frames):
            res, booked = _booked(ctx, lambda: capi.part_batch_process(ctx, [e[0] for e in eight], [f] * len(eight), cap=PCAP))
            for slot, (e, got) in enumerate(zip(eight, res)):
                _same(got, e[2][i], (order, slot, i))
            if i == 0:
                assert 1 <= booked.get("cascade_roi", 0) <= 4, booked
        for s, own, _ in eight:
            s.close()
            for c in own:
                c.free()


@needs_shim
def test_two_tickets_in_flight(ctx, loaded):
    frames = S.part_frames()[:3]
    a = [(_hnew_stream(ctx, loaded, k), _hnew_expected(k)[0]) for k in ("eye", "nose")]
    b = [(_hnew_stream(ctx, loaded, k), _hnew_expected(k)[0]) for k in ("mouth", "ear")]
    for i, f in enumerate(frames):
        ta = capi.part_batch_submit(ctx, [s for s, _ in a], [f] * 2)
        tb = capi.part_batch_submit(ctx, [s for s, _ in b], [f] * 2)
        for tk, group in ((ta, a), (tb, b)):
            for (s, exp), got in zip(group, capi.part_batch_collect(ctx, tk, cap=PCAP)):
                _same(got, exp[i], i)
    for s, _ in a + b:
        s.close()
