"""Face and part streams on new-format HAAR cascades (nvca_face_stream_create_any / nvca_part_stream_create_any) through the C ABI, against
the expected answers of tests/haar_new_stream_cases.py: boxes AND ids frame by frame, np.array_equal, no tolerance anywhere.  BGR and
NV12 input, one batch that mixes an old-format, an LBP and a new-format HAAR stream, two tickets in flight, part streams whose three
roles are of three formats, and the kernel timers: no small-image launch serves a search on a new-format HAAR cascade."""
import numpy as np
import pytest

import haar_new_stream_cases as S
import lbp_part_cases as LP
import lbp_stream_cases as LS
import orc
from nubovca import capi, synth

pytestmark = pytest.mark.gpu
CAP = 1024


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def loaded(ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ctx.load_cascade_xml(S.K.cascade(name)[0])
        return cache[name]
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


def _eq(got, exp, what):
    assert got[0].shape == exp[0].shape and np.array_equal(got[0], exp[0]), (what, got[0].tolist(), exp[0].tolist())
    assert np.array_equal(got[1], exp[1]), (what, got[1].tolist(), exp[1].tolist())


def _haar_bgr(i):
    return synth.make_bgr(640, 480, synth.frame_seed(0, i), "natural", [(160 + 8 * i, 120, 240)])


# (min_neighbors 0 tracks the raw list: "identity" alone, whose raw lists stay within what the oracle's stream tracks)
@pytest.mark.parametrize("cid,mn", [("identity", 3), ("identity", 0), ("half", 3)])
def test_stream_process_frame_by_frame(ctx, loaded, cid, mn):
    name, _W, _H, wtp, pct, _ = S.CASES[cid]
    frames = S.frames_of(S.CASES[cid])
    fs, ex = _stream(ctx, loaded(name), wtp, pct, mn), _expected(name, wtp, pct, mn)
    seen = 0
    for k, f in enumerate(frames + frames[:1]):
        e = ex.process(f)
        seen += len(e[0])
        _eq(fs.process(np.array(S.bgr(f)), cap=CAP), e, (cid, k))
    assert seen > 0


def test_nv12_stream(ctx, loaded):
    frames = S.frames_of(S.CASES["identity"])
    fs, ex = _stream(ctx, loaded("w24")), _expected("w24", fmt=capi.PIX_NV12)
    lay = capi.pixel_layout(*S.yuv(frames[0], capi.PIX_NV12)[1])
    fs.set_input(lay)
    for r, f in enumerate(frames):
        e = ex.process(f)
        assert r > 0 or len(e[0]) > 0
        res = ctx.face_batch_process([fs], [capi.make_planar_frame(np.array(S.yuv(f, capi.PIX_NV12)[0]), 160, 120, lay)], CAP)
        _eq(res[0], e, ("nv12", r))


def test_three_formats_in_one_batch(ctx, loaded, haar, orc_cascade):
    """an old-format stream, an LBP stream and two new-format HAAR streams (two cascades) in one call, in both slot orders; the HAAR slots
    are grouped on the device with the LBP one's (host_group 0) and on the host (host_group 1)"""
    a, b = S.CASES["identity"], S.CASES["half"]
    fa, fb, fl = S.frames_of(a), S.frames_of(b), LS.frames_of(LS.CASES["identity"])
    lbp = ctx.load_cascade_xml(LS.cascade("w24")[0])
    for hg in (0, 1):
        with ctx.options(host_group=hg):
            streams = [_stream(ctx, loaded(a[0]), a[3], a[4]), capi.FaceStream(ctx, haar), _stream(ctx, lbp), _stream(ctx, loaded(b[0]), b[3], b[4])]
            expected = [_expected(a[0], a[3], a[4]), orc.FaceStream(orc_cascade), LS.Expected("w24", 0, width_to_process=160, scale_factor_pct=25, min_neighbors=3, process_x_every_4=4),
                        _expected(b[0], b[3], b[4])]
            for r in range(3):
                hb = _haar_bgr(r)
                frames = [_host(fa[r % 3]), capi.make_frame(hb), capi.make_frame(np.array(LS.bgr(fl[r % 3]))), _host(fb[r % 3])]
                keys = [fa[r % 3], hb, fl[r % 3], fb[r % 3]]
                order = list(range(4))[::1 if r % 2 == 0 else -1]
                res = ctx.face_batch_process([streams[i] for i in order], [frames[i] for i in order], CAP)
                for slot, i in enumerate(order):
                    _eq(res[slot], expected[i].process(keys[i]), ("mixed", hg, r, i))
    lbp.free()


def test_two_tickets_in_flight(ctx, loaded, haar, orc_cascade):
    a, b = S.CASES["identity"], S.CASES["half"]
    fa, fb = S.frames_of(a), S.frames_of(b)
    sa = [_stream(ctx, loaded(a[0]), a[3], a[4]) for _ in fa]
    ea = [_expected(a[0], a[3], a[4]) for _ in fa]
    sb = [_stream(ctx, loaded(b[0]), b[3], b[4]), capi.FaceStream(ctx, haar)]
    eb = [_expected(b[0], b[3], b[4]), orc.FaceStream(orc_cascade)]
    for r in range(3):
        fra = fa[r:] + fa[:r]
        hb = _haar_bgr(r)
        ta = ctx.face_batch_submit(sa, [_host(f) for f in fra])
        tb = ctx.face_batch_submit(sb, [_host(fb[r % 3]), capi.make_frame(hb)])
        ra = ctx.face_batch_collect(ta, CAP)
        rb = ctx.face_batch_collect(tb, CAP)
        for i, f in enumerate(fra):
            _eq(ra[i], ea[i].process(f), ("ticket 1", r, i))
        _eq(rb[0], eb[0].process(fb[r % 3]), ("ticket 2", r))
        _eq(rb[1], eb[1].process(hb), ("ticket 2 haar", r))


def test_parameters_change_between_frames(ctx, loaded):
    frames = S.frames_of(S.CASES["identity"])
    fs, ex = _stream(ctx, loaded("w24")), _expected("w24")
    for k, (pct, mn) in enumerate([(25, 3), (10, 3), (25, 1), (10, 2)]):
        fs.set_property("multi_scale_factor", pct)
        fs.set_property("min_neighbors", mn)
        ex.p.update(scale_factor_pct=pct, min_neighbors=mn)
        f = frames[k % 3]
        _eq(fs.process(np.array(S.bgr(f)), cap=CAP), ex.process(f), (k, pct, mn))


# ------------------------------------------------------------------ part streams: three roles, three formats
@pytest.mark.skipif(LP.shim() is None, reason="no clang++")
@pytest.mark.parametrize("kind", sorted(S.PART_ROLES))
def test_part_stream_with_three_roles_in_three_formats(ctx, kind):
    exp, dets = S.part_expected(kind)
    assert all(len(d.seen) > 0 for d in dets)                       # every role searched
    if kind == "ear":
        assert sum(len(a) for a, b in exp) > 0 and sum(len(b) for a, b in exp) > 0
    cascs = [ctx.load_cascade_xml(S.part_xml(r)) for r in S.PART_ROLES[kind]]
    assert sorted(c.format()[0] for c in cascs) == [capi.CASCADE_HAAR, capi.CASCADE_LBP, capi.CASCADE_HAAR_NEW]
    s = capi.PartStream(ctx, LP.KINDS[kind], cascs[0], cascs[1], cascs[2], any_format=True)
    ctx.enable_kernel_timing(1)
    try:
        ctx.kernel_timing()
        for i, f in enumerate(S.part_frames()):
            got = s.process(f, cap=256)
            assert np.array_equal(got[0], exp[i][0]) and np.array_equal(got[1], exp[i][1]), (kind, i, got[0].tolist(), exp[i][0].tolist(), got[1].tolist(), exp[i][1].tolist())
        booked = {k: v[1] for k, v in ctx.kernel_timing().items()}
    finally:
        ctx.enable_kernel_timing(0)
        s.close()
    assert booked.get("cascade_strip", 0) > 0, booked               # the new-format HAAR searches: the large-image route


@pytest.mark.skipif(LP.shim() is None, reason="no clang++")
def test_no_small_image_launch_serves_a_new_format_haar_search(ctx):
    """an ear stream with every role on a new-format HAAR cascade: its 160 x 120 face pass and its part searches, all small images, book
    nothing under cascade_roi; the same stream on LBP cascades books its rounds there (tests/test_gpu_lbp_parts.py)"""
    names = ("w24", "w12", "w20x28")
    dets = tuple(S.hnew_detector(S.K.cascade(n)[1]) for n in names)
    h = LP.Harness("ear", *dets)
    frames = S.part_frames()[:2]
    exp = [h.process(f) for f in frames]
    h.close()
    assert all(len(d.seen) > 0 for d in dets)
    cascs = [ctx.load_cascade_xml(S.K.cascade(n)[0]) for n in names]
    s = capi.PartStream(ctx, LP.KINDS["ear"], cascs[0], cascs[1], cascs[2], any_format=True)
    ctx.enable_kernel_timing(1)
    try:
        ctx.kernel_timing()
        for i, f in enumerate(frames):
            got = s.process(f, cap=256)
            assert np.array_equal(got[0], exp[i][0]) and np.array_equal(got[1], exp[i][1]), (i, got[0].tolist(), exp[i][0].tolist())
        booked = {k: v[1] for k, v in ctx.kernel_timing().items()}
    finally:
        ctx.enable_kernel_timing(0)
        s.close()
    assert "cascade_roi" not in booked and booked.get("cascade_strip", 0) > 0, booked
