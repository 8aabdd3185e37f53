"""Face streams on new-format LBP cascades (nvca_face_stream_create_any; csrc/face_stream.cpp, lbp_job.cpp, the pyramid through the LUT in
kernels_gray.hip, k_group on LBP candidate keys) through the C ABI, frame by frame against the expected sequence of
tests/lbp_stream_cases.py: boxes AND ids, np.array_equal, no tolerance anywhere.  The expected stream is the oracle's gate and finish around
the numpy statement's detections on the equalised working image; tests/test_lbp_streams_cpu.py asserts on the statement alone that every
case lies in the regime it is here for.  Every test that makes a stream with any_format=True fails without nvca_face_stream_create_any."""
import ctypes as C

import numpy as np
import pytest

import lbp_stream_cases as S
import orc
from nubovca import capi, synth

pytestmark = pytest.mark.gpu
CAP = 1024                                     # boxes a frame (a min_neighbors-0 stream tracks its raw list)
ALL_CASES = dict(S.CASES, win78=S.WIN78)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def loaded(ctx):
    """cascade key -> the device's cascade, loaded once"""
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = ctx.load_cascade_xml(S.cascade(key)[0])
        return cache[key]
    return get


@pytest.fixture(scope="module")
def haar(ctx, synth_xml):
    c = ctx.load_cascade_xml(synth_xml)
    yield c
    c.free()


def _stream(ctx, casc, wtp=160, pct=25, mn=3, px=4, **kw):
    return capi.FaceStream(ctx, casc, any_format=True, width_to_process=wtp, multi_scale_factor=pct, min_neighbors=mn, process_x_every_4_frames=px, **kw)


def _expected(key, wtp=160, pct=25, mn=3, px=4, fmt=0):
    return S.Expected(key, fmt, width_to_process=wtp, scale_factor_pct=pct, min_neighbors=mn, process_x_every_4=px)


def _host(frame):
    return capi.make_frame(np.array(S.bgr(frame)))


class DeviceFrames:
    """frames in HBM, kept alive"""

    def __init__(self):
        self.keep = []

    def __call__(self, frame):
        import torch
        a = np.array(S.bgr(frame))
        t = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        self.keep.append(t)
        return capi.make_frame(t.data_ptr(), a.shape[1], a.shape[0], a.strides[0], capi.MEM_DEVICE)


def _eq(got, exp, what):
    assert got[0].shape == exp[0].shape and np.array_equal(got[0], exp[0]), (what, got[0].tolist(), exp[0].tolist())
    assert np.array_equal(got[1], exp[1]), (what, got[1].tolist(), exp[1].tolist())


def _haar_bgr(i):
    return synth.make_bgr(640, 480, synth.frame_seed(0, i), "natural", [(160 + 8 * i, 120, 240)])


# ------------------------------------------------------------------ nvca_face_stream_process, case by case
@pytest.mark.parametrize("cid", sorted(ALL_CASES))
def test_stream_process_frame_by_frame(ctx, loaded, cid):
    name, _W, _H, wtp, pct, _ = ALL_CASES[cid]
    frames = S.frames_of(ALL_CASES[cid])
    fs, ex = _stream(ctx, loaded(name), wtp, pct), _expected(name, wtp, pct)
    for k, f in enumerate(frames + frames[:1]):
        _eq(fs.process(np.array(S.bgr(f)), cap=CAP), ex.process(f), (cid, k))


@pytest.mark.parametrize("px", [4, 2])
def test_sequence_with_two_empty_analysed_frames(ctx, loaded, px):
    """hysteresis over the first empty frame, faces.clear() at the second, new ids afterwards; every other frame analysed at 2"""
    name, _W, _H, wtp, pct, _ = S.CASES["bilinear"]
    frames = S.frames_of(S.CASES["bilinear"])
    fs, ex = _stream(ctx, loaded(name), wtp, pct, px=px), _expected(name, wtp, pct, px=px)
    for k, f in enumerate(frames + frames):
        _eq(fs.process(np.array(S.bgr(f))), ex.process(f), (px, k))


@pytest.mark.parametrize("mn", [0, 1])
def test_deep_cascade_raw_list_and_one_box(ctx, loaded, mn):
    name, _W, _H, wtp, pct, _ = S.CASES["deep"]
    fs, ex = _stream(ctx, loaded(name), wtp, pct, mn=mn), _expected(name, wtp, pct, mn=mn)
    for k, f in enumerate(S.frames_of(S.CASES["deep"])):
        got, exp = fs.process(np.array(S.bgr(f)), cap=CAP), ex.process(f)
        assert len(exp[0]) > 0
        _eq(got, exp, (mn, k))


# ------------------------------------------------------------------ nvca_face_batch_process
def _run_batch(ctx, streams, expected, frames_of_round, make=_host, rounds=2, order=1, cap=CAP, what=""):
    """rounds of one call over all streams (stream i's frame of round r: frames_of_round(r)[i]), handed in in `order`"""
    for r in range(rounds):
        fr = frames_of_round(r)
        idx = list(range(len(streams)))[::order]
        res = ctx.face_batch_process([streams[i] for i in idx], [make(fr[i]) for i in idx], cap)
        for slot, i in enumerate(idx):
            _eq(res[slot], expected[i].process(fr[i]), (what, r, i))


@pytest.mark.parametrize("order", [1, -1], ids=["slot-order", "reversed"])
@pytest.mark.parametrize("cid", ["identity", "bitonic", "odd", "win78"])
def test_batch_of_one_group(ctx, loaded, cid, order):
    """every slot a different frame; the frames rotate from round to round, so the ids carry what each stream saw before"""
    name, _W, _H, wtp, pct, _ = ALL_CASES[cid]
    frames = S.frames_of(ALL_CASES[cid])
    n = len(frames)
    streams = [_stream(ctx, loaded(name), wtp, pct) for _ in range(n)]
    expected = [_expected(name, wtp, pct) for _ in range(n)]
    _run_batch(ctx, streams, expected, lambda r: [frames[(i + r) % n] for i in range(n)], order=order, what=cid)


def test_more_streams_than_one_job_takes(ctx, loaded):
    name, _W, _H, wtp, pct, _ = S.MANY
    frames = S.frames_of(S.MANY)
    n = len(frames)
    assert n == 33
    streams = [_stream(ctx, loaded(name), wtp, pct) for _ in range(n)]
    expected = [_expected(name, wtp, pct) for _ in range(n)]
    _run_batch(ctx, streams, expected, lambda r: [frames[(i + 5 * r) % n] for i in range(n)], what="33 streams")


def test_empty_and_ungrouped_slots_beside_full_ones(ctx, loaded):
    frames = [S.frames_of(S.CASES["identity"])[0], S.FLAT, S.NATURAL[0], S.frames_of(S.CASES["identity"])[1], S.NATURAL[1]]
    streams = [_stream(ctx, loaded("w24")) for _ in frames]
    expected = [_expected("w24") for _ in frames]
    _run_batch(ctx, streams, expected, lambda r: frames[r:] + frames[:r], rounds=3, what="empty slots")


def test_frame_no_higher_than_the_window_has_no_level(ctx, loaded):
    """40 x 24 under the 24 x 24 window: the scan has no level, the slot answers empty -- alone, and beside a full slot of another group"""
    small, full = ("natural", 40, 24, 5), S.frames_of(S.CASES["identity"])[0]
    assert len(S.raw("w24", small, 40, 25)) == 0
    streams = [_stream(ctx, loaded("w24"), 40), _stream(ctx, loaded("w24"))]
    expected = [_expected("w24", 40), _expected("w24")]
    _eq(streams[0].process(np.array(S.bgr(small))), expected[0].process(small), "alone")
    for r in range(2):
        res = ctx.face_batch_process(streams, [_host(small), _host(full)], CAP)
        _eq(res[0], expected[0].process(small), ("no level", r))
        e = expected[1].process(full)
        assert len(e[0]) > 0
        _eq(res[1], e, ("beside it", r))


def test_lbp_and_haar_streams_and_two_geometries_in_one_call(ctx, loaded, haar, orc_cascade):
    """four launch groups: LBP at 160 x 120, the same cascade on 320 x 240 frames, another LBP cascade at another scale factor, and Haar
    streams, whose slots answer as orc.FaceStream.process"""
    a, b, c = S.CASES["identity"], S.CASES["half"], S.CASES["bitonic"]
    fa, fb, fc = S.frames_of(a), S.frames_of(b), S.frames_of(c)
    lbp = [(a[0], a[3], a[4], fa), (b[0], b[3], b[4], fb), (c[0], c[3], c[4], fc), (a[0], a[3], a[4], fa[1:] + fa[:1])]
    streams = [_stream(ctx, loaded(n), w, p) for n, w, p, _ in lbp]
    expected = [_expected(n, w, p) for n, w, p, _ in lbp]
    hs = [capi.FaceStream(ctx, haar), _stream(ctx, haar)]                      # either constructor
    ohs = [orc.FaceStream(orc_cascade), orc.FaceStream(orc_cascade)]
    for r in range(3):
        fr = [f[r % len(f)] for _n, _w, _p, f in lbp]
        hb = [_haar_bgr(r), _haar_bgr(r + 1)]
        # interleaved: LBP, Haar, LBP, LBP, Haar, LBP
        order = [("l", 0), ("h", 0), ("l", 1), ("l", 2), ("h", 1), ("l", 3)]
        ss = [streams[i] if k == "l" else hs[i] for k, i in order]
        ff = [_host(fr[i]) if k == "l" else capi.make_frame(hb[i]) for k, i in order]
        res = ctx.face_batch_process(ss, ff, CAP)
        any_haar_box = False
        for slot, (k, i) in enumerate(order):
            if k == "l":
                _eq(res[slot], expected[i].process(fr[i]), ("mixed", r, slot))
            else:
                e = ohs[i].process(hb[i])
                any_haar_box = any_haar_box or len(e[0]) > 0
                _eq(res[slot], e, ("mixed haar", r, slot))
        assert any_haar_box


def test_host_and_device_frames(ctx, loaded):
    name, _W, _H, wtp, pct, _ = S.CASES["half"]
    frames = S.frames_of(S.CASES["half"])
    dev = DeviceFrames()
    streams = [_stream(ctx, loaded(name), wtp, pct) for _ in range(4)]
    expected = [_expected(name, wtp, pct) for _ in range(4)]
    for r in range(2):
        fr = [frames[(i + r) % 3] for i in range(4)]
        ff = [dev(fr[i]) if (i + r) % 2 else _host(fr[i]) for i in range(4)]
        res = ctx.face_batch_process(streams, ff, CAP)
        for i in range(4):
            _eq(res[i], expected[i].process(fr[i]), ("host/device", r, i))
    # all in HBM
    ff = [dev(frames[i % 3]) for i in range(4)]
    res = ctx.face_batch_process(streams, ff, CAP)
    for i in range(4):
        _eq(res[i], expected[i].process(frames[i % 3]), ("device", i))


def test_ingest_chunk_two_jobs_of_one_group(ctx, loaded):
    """four host frames at ingest_chunk 2: two jobs of one group, each with its own result slots, box tables and thresholds"""
    frames = S.frames_of(S.CASES["identity"]) + [S.NATURAL[0]]
    streams = [_stream(ctx, loaded("w24"), mn=mn) for mn in (3, 1, 3, 2)]
    expected = [_expected("w24", mn=mn) for mn in (3, 1, 3, 2)]
    with ctx.options(ingest_chunk=2):
        ctx.enable_kernel_timing(1)
        try:
            _run_batch(ctx, streams, expected, lambda r: frames[r:] + frames[:r], what="ingest_chunk 2")
            kt = ctx.kernel_timing()
        finally:
            ctx.enable_kernel_timing(0)
    assert kt["group_rects"][1] == 2 * 2, kt              # two jobs a call, two calls


def test_min_neighbors_side_by_side(ctx, loaded):
    frames = S.frames_of(S.CASES["identity"])
    mns = (0, 1, 3, 0, 3)
    streams = [_stream(ctx, loaded("w24"), mn=mn) for mn in mns]
    expected = [_expected("w24", mn=mn) for mn in mns]
    _run_batch(ctx, streams, expected, lambda r: [frames[(i + r) % 3] for i in range(len(mns))], what="min_neighbors 0 / 1 / 3")


# ------------------------------------------------------------------ where the grouping runs
def _timed_rounds(ctx, loaded, cid, rounds=2, **options):
    name, _W, _H, wtp, pct, _ = ALL_CASES[cid]
    frames = S.frames_of(ALL_CASES[cid])
    streams = [_stream(ctx, loaded(name), wtp, pct) for _ in frames]
    expected = [_expected(name, wtp, pct) for _ in frames]
    out = []
    with ctx.options(**options):
        ctx.enable_kernel_timing(1)
        try:
            for r in range(rounds):
                fr = frames[r:] + frames[:r]
                res = ctx.face_batch_process(streams, [_host(f) for f in fr], CAP)
                for i, f in enumerate(fr):
                    _eq(res[i], expected[i].process(f), (cid, options, r, i))
                out.append(res)
            kt = ctx.kernel_timing()
        finally:
            ctx.enable_kernel_timing(0)
    return out, kt


@pytest.mark.parametrize("cid", ["identity", "bitonic"])
def test_host_group_on_and_off_answer_alike(ctx, loaded, cid):
    dev, kt_dev = _timed_rounds(ctx, loaded, cid)
    cpy, kt_cpy = _timed_rounds(ctx, loaded, cid, group_zerocopy=0)
    host, kt_host = _timed_rounds(ctx, loaded, cid, host_group=1)
    for a, b, c in zip(dev, cpy, host):
        for x, y, z in zip(a, b, c):
            _eq(x, y, "copy route")
            _eq(x, z, "host route")
    # the NVCA_K_GROUP timer: a launch a batch, time above zero, when the device groups; nothing booked under host_group
    for kt in (kt_dev, kt_cpy):
        assert kt["group_rects"][1] == 2 and kt["group_rects"][0] > 0, kt
    assert "group_rects" not in kt_host, kt_host
    assert kt_dev["cascade_strip"][1] == kt_host["cascade_strip"][1] > 0        # the evaluator's launches do not depend on the route


def test_per_level_pyramid_route_reads_through_the_lut(loaded):
    """pyr_off: every plan resizes level by level (launch_resize1) -- the route of plans with a level wider than 1023 -- here with three
    images and the LUT; a context of its own, whose plans are built under the switch"""
    c = capi.Context(0)
    try:
        c.set_option("pyr_off", 1)
        name, _W, _H, wtp, pct, _ = S.CASES["identity"]
        casc = c.load_cascade_xml(S.cascade(name)[0])
        frames = S.frames_of(S.CASES["identity"])
        streams = [_stream(c, casc, wtp, pct) for _ in frames]
        expected = [_expected(name, wtp, pct) for _ in frames]
        _run_batch(c, streams, expected, lambda r: frames[r:] + frames[:r], what="pyr_off")
    finally:
        c.close()


# ------------------------------------------------------------------ submit / collect
def test_two_tickets_in_flight(ctx, loaded, haar, orc_cascade):
    """two submitted batches on two lanes, collected in order; the second one mixes LBP and Haar streams"""
    name, _W, _H, wtp, pct, _ = S.CASES["identity"]
    fa = S.frames_of(S.CASES["identity"])
    fb = S.frames_of(S.CASES["bitonic"])
    sa = [_stream(ctx, loaded(name), wtp, pct) for _ in fa]
    ea = [_expected(name, wtp, pct) for _ in fa]
    sb = [_stream(ctx, loaded("w20x28"), 160, 10), capi.FaceStream(ctx, haar), _stream(ctx, loaded("w20x28"), 160, 10)]
    eb = [_expected("w20x28", 160, 10), orc.FaceStream(orc_cascade), _expected("w20x28", 160, 10)]
    for r in range(3):
        fra = fa[r:] + fa[:r]
        hb = _haar_bgr(r)
        ta = ctx.face_batch_submit(sa, [_host(f) for f in fra])
        tb = ctx.face_batch_submit(sb, [_host(fb[r % 3]), capi.make_frame(hb), _host(fb[(r + 1) % 3])])
        with pytest.raises(capi.NvcaError):
            ctx.face_batch_collect(tb, CAP)                      # in submission order only
        ra = ctx.face_batch_collect(ta, CAP)
        rb = ctx.face_batch_collect(tb, CAP)
        for i, f in enumerate(fra):
            _eq(ra[i], ea[i].process(f), ("ticket 1", r, i))
        _eq(rb[0], eb[0].process(fb[r % 3]), ("ticket 2", r, 0))
        _eq(rb[1], eb[1].process(hb), ("ticket 2 haar", r))
        _eq(rb[2], eb[2].process(fb[(r + 1) % 3]), ("ticket 2", r, 2))


# ------------------------------------------------------------------ 4:2:0 frames
def test_nv12_and_i420_streams(ctx, loaded):
    frames = S.frames_of(S.CASES["identity"])
    fmts = (capi.PIX_NV12, capi.PIX_I420)
    streams = [_stream(ctx, loaded("w24")) for _ in fmts]
    expected = [_expected("w24", fmt=fmt) for fmt in fmts]
    lays = []
    for s, fmt in zip(streams, fmts):
        lay = S.yuv(frames[0], fmt)[1]
        lays.append(capi.pixel_layout(*lay))
        s.set_input(lays[-1])
    for r in range(3):
        f = frames[r]
        ff = [capi.make_planar_frame(np.array(S.yuv(f, fmt)[0]), 160, 120, lay) for fmt, lay in zip(fmts, lays)]
        res = ctx.face_batch_process(streams, ff, CAP)
        for i in range(2):
            e = expected[i].process(f)
            assert r > 0 or len(e[0]) > 0
            _eq(res[i], e, ("4:2:0", fmts[i], r))


# ------------------------------------------------------------------ parameters between frames
def test_scale_factor_and_min_neighbors_change_between_frames(ctx, loaded):
    """two scale factors (two cached plans) and three thresholds on one stream; the raw lists stay within what the oracle's stream tracks"""
    frames = S.frames_of(S.CASES["identity"])
    fs, ex = _stream(ctx, loaded("w24")), _expected("w24")
    for k, (pct, mn) in enumerate([(25, 3), (10, 3), (25, 1), (10, 0), (25, 3), (10, 1)]):
        fs.set_property("multi_scale_factor", pct)
        fs.set_property("min_neighbors", mn)
        ex.p.update(scale_factor_pct=pct, min_neighbors=mn)
        f = frames[k % 3]
        _eq(fs.process(np.array(S.bgr(f)), cap=CAP), ex.process(f), (k, pct, mn))


def test_motion_event_gates_an_lbp_stream(ctx, loaded):
    """detect_event: nothing is analysed (and no counter moves) until a motion event arrives; the frame after it is a fresh stream's first"""
    frames = S.frames_of(S.CASES["identity"])
    fs = _stream(ctx, loaded("w24"), detect_event=1)
    for f in frames[:2]:
        assert len(fs.process(np.array(S.bgr(f)))[0]) == 0
    fs.motion_event()
    ex = _expected("w24")
    for k, f in enumerate(frames):
        e = ex.process(f)
        assert len(e[0]) > 0
        _eq(fs.process(np.array(S.bgr(f))), e, ("after the event", k))


# ------------------------------------------------------------------ the new constructor on a Haar cascade
def test_new_constructor_on_a_haar_cascade_is_the_old_stream(ctx, haar, orc_cascade):
    old, new, ofs = capi.FaceStream(ctx, haar), capi.FaceStream(ctx, haar, any_format=True), orc.FaceStream(orc_cascade)
    seen = 0
    for i in range(5):
        bgr = _haar_bgr(i)
        a, b, e = old.process(bgr), new.process(bgr), ofs.process(bgr)
        _eq(b, a, ("new against old", i))
        _eq(b, e, ("new against the oracle", i))
        seen += len(e[0])
    assert seen > 0


# ------------------------------------------------------------------ overflow
def test_above_the_device_grouping_limit_and_overflow(ctx, loaded):
    """8346 candidates on the flat frame: k_group declines the slot and the host groups; with 256 candidates a frame the batch is refused
    with NVCA_ERR_OVERFLOW -- never a truncated list -- and the next call, its lists sized for what the refused one produced, answers"""
    casc = loaded(S.CODE255)
    others = [("natural", 160, 120, 5), ("ramp", 160, 120)]
    frames = [S.FLAT] + others
    streams = [_stream(ctx, casc) for _ in frames]
    expected = [_expected(S.CODE255) for _ in frames]
    _run_batch(ctx, streams, expected, lambda r: frames[r:] + frames[:r], rounds=2, what="declined slot")
    ctx.set_hit_capacity(256)
    try:
        fs = _stream(ctx, casc)
        with pytest.raises(capi.NvcaError) as e:
            fs.process(np.array(S.bgr(S.FLAT)), cap=CAP)
        assert e.value.code == capi.ERR_OVERFLOW
        ex = _expected(S.CODE255)                          # nothing was tracked for the refused frame: the first tracked frame of either
        exp = ex.process(S.FLAT)
        assert len(exp[0]) > 0
        _eq(fs.process(np.array(S.bgr(S.FLAT)), cap=CAP), exp, "after the overflow")
        _eq(fs.process(np.array(S.bgr(others[0])), cap=CAP), ex.process(others[0]), "and on")
    finally:
        ctx.set_hit_capacity(16384)


# ------------------------------------------------------------------ refusals
def test_refusals_of_the_new_constructor(ctx, loaded):
    L = ctx.L
    lbp = loaded("w24")
    h = C.c_void_p()
    p = capi.FaceParams()
    L.nvca_face_params_default(C.byref(p))
    assert L.nvca_face_stream_create_any(None, lbp.h, C.byref(p), C.byref(h)) == capi.ERR_ARG
    assert L.nvca_face_stream_create_any(ctx.h, None, C.byref(p), C.byref(h)) == capi.ERR_ARG
    assert L.nvca_face_stream_create_any(ctx.h, lbp.h, C.byref(p), None) == capi.ERR_ARG
    assert not h.value
    assert L.nvca_face_stream_create_any(ctx.h, lbp.h, None, C.byref(h)) == capi.OK and h.value          # default parameters
    L.nvca_face_stream_destroy(h)
    other = capi.Context(0)
    try:
        foreign = other.load_cascade_xml(S.cascade("w24")[0])
        h = C.c_void_p()
        assert L.nvca_face_stream_create_any(ctx.h, foreign.h, C.byref(p), C.byref(h)) == capi.ERR_ARG and not h.value
        assert L.nvca_last_error(ctx.h)
        foreign.free()
    finally:
        other.close()


def test_scale_factor_0_is_refused_with_the_gates_rolled_back(ctx, loaded):
    """multi-scale-factor 0 (scaleFactor 1.0): NVCA_ERR_ARG for the batch, and every stream of it as it was before the call -- at
    process_x_every_4 2 the frame after the refusal is the first, analysed one; a gate that had advanced would skip it"""
    frames = S.frames_of(S.CASES["identity"])
    bad = _stream(ctx, loaded("w24"), pct=0, px=2)
    good = _stream(ctx, loaded("w24"), px=2)
    eb, eg = _expected("w24", px=2), _expected("w24", px=2)
    for _ in range(2):
        with pytest.raises(capi.NvcaError) as e:
            ctx.face_batch_process([good, bad], [_host(frames[0]), _host(frames[1])], CAP)
        assert e.value.code == capi.ERR_ARG
    bad.set_property("multi_scale_factor", 25)
    for k in range(4):
        res = ctx.face_batch_process([good, bad], [_host(frames[k % 3]), _host(frames[(k + 1) % 3])], CAP)
        x, y = eg.process(frames[k % 3]), eb.process(frames[(k + 1) % 3])
        assert k > 0 or (len(x[0]) > 0 and len(y[0]) > 0)
        _eq(res[0], x, ("good", k))
        _eq(res[1], y, ("bad, mended", k))


def test_unchanged_refusals(ctx, loaded, haar):
    """nvca_face_stream_create and the part streams keep refusing an LBP cascade"""
    L = ctx.L
    lbp = loaded("w24")
    h = C.c_void_p()
    assert L.nvca_face_stream_create(ctx.h, lbp.h, None, C.byref(h)) == capi.ERR_UNSUPPORTED and L.nvca_last_error(ctx.h) and not h.value
    with pytest.raises(capi.NvcaError) as e:
        capi.FaceStream(ctx, lbp)
    assert e.value.code == capi.ERR_UNSUPPORTED
    p = capi.PartParams()
    L.nvca_part_params_default(C.byref(p), capi.PART_EYE)
    for roles in ((lbp, haar, haar), (haar, lbp, haar), (haar, haar, lbp)):
        assert L.nvca_part_stream_create(ctx.h, C.byref(p), roles[0].h, roles[1].h, roles[2].h, C.byref(h)) == capi.ERR_UNSUPPORTED
