"""NV12 / I420 part streams (nvca_part_stream_set_input) on the GPU: eye, nose, mouth and ear detectors fed 4:2:0 frames against the
existing oracle streams fed the conversion statement's BGR image (tests/yuv_reference.py), box lists bit for bit, frame by frame.
The scenes and that the oracle finds parts in them: tests/yuv_stream_scenes.py, tests/test_yuv_streams_cpu.py."""
import numpy as np
import pytest

import yuv_reference as R
import yuv_stream_scenes as S
from test_gpu_yuv import _bad_frames

pytestmark = pytest.mark.gpu

FMTS = [R.NV12, R.I420]
FMT_IDS = ["nv12", "i420"]
KIND_LIST = ["eye", "nose", "mouth", "ear"]


@pytest.fixture(scope="module")
def env():
    from nubovca import capi
    ctx = capi.Context(0)
    dev = {n: ctx.load_cascade_xml(x) for n, (x, _) in S.part_cascades().items()}
    yield ctx, dev
    ctx.close()


def _layout(lay):
    from nubovca import capi
    return capi.pixel_layout(*lay)


_KEEP = []


def _frame(buf, W, H, lay, mem):
    """a Frame of the buffer in host memory (a writable copy) or device memory (kept for the module)"""
    from nubovca import capi
    if mem == "host":
        return capi.make_planar_frame(np.array(buf), W, H, _layout(lay))
    import torch
    t = torch.from_numpy(np.array(buf)).cuda()
    torch.cuda.synchronize()
    _KEEP.append(t)
    return capi.make_planar_frame(t.data_ptr(), W, H, _layout(lay), capi.MEM_DEVICE)


def _bgr_frame(img, mem="host"):
    from nubovca import capi
    if mem == "host":
        return capi.make_frame(np.array(img))
    import torch
    t = torch.from_numpy(np.array(img)).cuda()
    torch.cuda.synchronize()
    _KEEP.append(t)
    return capi.make_frame(t.data_ptr(), img.shape[1], img.shape[0], img.shape[1] * 3, capi.MEM_DEVICE)


def _stream(env, kind, lay=None, **props):
    from nubovca import capi
    ctx, dev = env
    k, a, b = S.KINDS[kind]
    s = capi.PartStream(ctx, k, dev["face"], dev[a], dev[b] if b else None, **props)
    if lay is not None:
        s.set_input(_layout(lay))
    return s


def _same(got, exp, what):
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (what, got[0].tolist(), exp[0].tolist(), got[1].tolist(), exp[1].tolist())


def _found(exp):
    return sum(len(a) + len(b) for a, b in exp)


# ---------------------------------------------------------------- 1. sequences
def _pad_kw(fmt):
    return dict(pad=6, luma_rows=496, gap=64, chroma_pad=2 if fmt == R.I420 else None)


SEQ_CASES = [(W, H, False) for W, H in S.PART_GEOS] + [(640, 480, True)]


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("W,H,padded", SEQ_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", KIND_LIST)
def test_part_stream_sequences(env, kind, W, H, padded, fmt, mem):
    """9 frames of a stream per kind, format and geometry -- 640 x 480: the exact-2x resize; 800 x 600: the 2.5 truncation quirk and
    bilinear taps; 322 x 242: every tail, the unaligned eye-gray pitch -- in tight planes, and at 640 x 480 also with padded rows, a
    luma plane of 496 rows and gaps between the planes"""
    kw = _pad_kw(fmt) if padded else {}
    exp = S.part_expected(kind, W, H)
    assert _found(exp) > 0
    lay = S.part_frame(W, H, 0, fmt, **kw)[1]
    s = _stream(env, kind, lay)
    for i in range(S.PART_FRAMES):
        buf, lay_i = S.part_frame(W, H, i, fmt, **kw)
        assert lay_i == lay
        _same(s.process(_frame(buf, W, H, lay, mem)), exp[i], (kind, W, H, padded, fmt, mem, i))
    s.close()


def test_eye_gray_kernel_follows_the_destination_pitch(env, capfd):
    """the eye chain's full-size gray image has pitch w: 640-wide tight planes take k_gray_yuv16; 648-wide planes with rows padded to
    656 bytes take its loads, but the image's rows (648 bytes: no multiple of 16) do not take its stores -- k_gray_yuv_generic.  Same
    lists as the oracle either way."""
    ctx = env[0]
    seen = 0
    for W, H, pad, kernel in ((640, 480, 0, "k_gray_yuv16"), (648, 480, 8, "k_gray_yuv_generic"), (322, 242, 0, "k_gray_yuv_generic")):
        lay = S.part_frame(W, H, 0, R.NV12, pad=pad)[1]
        assert pad == 0 or all(v % 16 == 0 for v in lay[1][:2] + lay[2][:2])
        exp = S.part_expected("eye", W, H, 3)
        capfd.readouterr()
        with ctx.options(plan_debug=1):
            s = _stream(env, "eye", lay)
            for i in range(3):
                _same(s.process(_frame(S.part_frame(W, H, i, R.NV12, pad=pad)[0], W, H, lay, "device")), exp[i], (W, H, pad, i))
            s.close()
        ran = [ln.rsplit(": ", 1)[1] for ln in capfd.readouterr().err.splitlines() if ln.startswith("[nvca plan] 4:2:0 eye gray")]
        assert ran == [kernel] * 3, (W, H, pad, ran)
        seen += _found(exp)
    assert seen > 0


# ---------------------------------------------------------------- 2. detect-event mode
def test_detect_event_mode_with_an_nv12_face_stream(env):
    """an NV12 face stream's boxes (original-frame pixels) pushed into NV12 eye, nose and mouth streams"""
    import orc
    from nubovca import capi
    ctx, dev = env
    W, H = 640, 480
    lay = S.part_frame(W, H, 0, R.NV12)[1]
    fs = capi.FaceStream(ctx, dev["face"])
    fs.set_input(_layout(lay))
    ofs = orc.FaceStream(S.part_cascades()["face"][1])
    pairs = [(_stream(env, k, lay, detect_event=1), S.oracle_part_stream(k, detect_event=1)) for k in ("eye", "nose", "mouth")]
    seen = 0
    for i in range(8):
        buf = S.part_frame(W, H, i, R.NV12)[0]
        bgr = np.array(S.part_bgr(W, H, i))
        boxes, ids = ctx.face_batch_process([fs], [_frame(buf, W, H, lay, "host")])[0]
        eb, eid = ofs.process(bgr)
        assert np.array_equal(boxes, eb) and np.array_equal(ids, eid), i
        for g, o in pairs:
            if i % 3 != 2 and len(boxes):        # some frames come without an upstream message
                g.push_faces(boxes); o.push_faces(boxes)
        res = capi.part_batch_process(ctx, [g for g, _ in pairs], [_frame(buf, W, H, lay, "device" if i % 2 else "host")] * 3)
        for (g, o), got in zip(pairs, res):
            exp = o.process(bgr)
            _same(got, exp, i)
            seen += _found([exp])
    assert seen > 0
    fs.close()
    for g, _ in pairs:
        g.close()


# ---------------------------------------------------------------- 3. one call of BGR, NV12 and I420 streams
def test_batched_call_of_three_formats(env):
    """3 video streams at 640 x 480 with the same content -- the statement's BGR image, an NV12 buffer, an I420 buffer -- and four
    detectors on each: 12 part streams in one nvca_part_batch_process.  Every stream against its own oracle stream; the three formats
    give identical lists."""
    from nubovca import capi
    ctx = env[0]
    W, H = 640, 480
    lays = [None, S.part_frame(W, H, 0, R.NV12)[1], S.part_frame(W, H, 0, R.I420, pad=32)[1]]
    streams = [[_stream(env, k, lay) for k in KIND_LIST] for lay in lays]
    seen = 0
    for i in range(5):
        bgr = np.array(S.part_bgr(W, H, i))
        frames = [_bgr_frame(bgr, "device" if i % 2 else "host"), _frame(S.part_frame(W, H, i, R.NV12)[0], W, H, lays[1], "host" if i % 2 else "device"),
                  _frame(S.part_frame(W, H, i, R.I420, pad=32)[0], W, H, lays[2], "host")]
        res = capi.part_batch_process(ctx, [s for v in streams for s in v], [frames[v] for v in range(3) for _ in KIND_LIST])
        for v in range(3):
            for j, kind in enumerate(KIND_LIST):
                exp = S.part_expected(kind, W, H)[i]             # (the three video streams carry the same content: one oracle sequence per kind)
                _same(res[v * 4 + j], exp, (i, v, kind))
                _same(res[v * 4 + j], res[j], (i, v, kind, "against the BGR stream"))
                seen += _found([exp])
    assert seen > 0
    for v in streams:
        for s in v:
            s.close()


# ---------------------------------------------------------------- 4. sharing
def test_streams_share_a_frame_only_under_one_layout(env):
    """four detectors handed the same NV12 pointer and layout share its upload and work; a fifth stream handed the SAME pointer, size and
    stride with another valid layout -- its luma plane is a second plane behind the chroma plane, the luma of a later frame of the scene
    -- gets the result of its own planes"""
    from nubovca import capi
    ctx = env[0]
    W, H = 640, 480
    lay_a = (R.NV12, (0, W * H, 0), (W, W, 0))
    lay_b = (R.NV12, (W * H * 3 // 2, W * H, 0), (W, W, 0))
    four = [_stream(env, k, lay_a) for k in KIND_LIST]
    fifth = _stream(env, "nose", lay_b)
    o_four = [S.oracle_part_stream(k) for k in KIND_LIST]
    o_fifth = S.oracle_part_stream("nose")
    seen, differ = 0, 0
    for i in range(4):
        first, _ = S.part_frame(W, H, i, R.NV12)
        second, _ = S.part_frame(W, H, i + 4, R.NV12)
        buf = np.concatenate([first, second[:W * H]])
        img_a, img_b = R.bgr(buf, W, H, lay_a), R.bgr(buf, W, H, lay_b)
        assert np.array_equal(img_a, S.part_bgr(W, H, i)) and not np.array_equal(img_a, img_b)
        fa = _frame(buf, W, H, lay_a, "host" if i % 2 else "device")
        fb = capi.Frame(fa.data, W, H, W, fa.mem, 0)              # the same pointer, size, stride and memory kind
        res = capi.part_batch_process(ctx, four + [fifth], [fa] * 4 + [fb])
        for j in range(4):
            exp = o_four[j].process(img_a)
            _same(res[j], exp, (i, KIND_LIST[j]))
            seen += _found([exp])
        exp = o_fifth.process(img_b)
        _same(res[4], exp, (i, "fifth"))
        seen += _found([exp])
        differ += not (np.array_equal(res[4][0], res[1][0]) and np.array_equal(res[4][1], res[1][1]))
    assert seen > 0 and differ > 0
    for s in four + [fifth]:
        s.close()


# ---------------------------------------------------------------- 5. two tickets in flight
def test_two_tickets_in_flight_keep_their_layouts(env):
    """submit(k + 1) before collect(k); between the two submits one stream changes from NV12 to I420 and one from I420 to packed BGR:
    ticket k keeps the layouts it was submitted with"""
    from nubovca import capi
    ctx = env[0]
    W, H = 640, 480
    lay = {R.NV12: S.part_frame(W, H, 0, R.NV12)[1], R.I420: S.part_frame(W, H, 0, R.I420)[1]}
    kinds = ["nose", "eye", "mouth", "ear"]
    fmts = [R.NV12, R.I420, R.NV12, R.I420]              # format of every stream, changed below
    streams = [_stream(env, k, lay[f]) for k, f in zip(kinds, fmts)]
    T = 6

    def submit(i):
        frames = []
        for f in fmts:
            if f is None:
                frames.append(_bgr_frame(S.part_bgr(W, H, i), "host"))
            else:
                frames.append(_frame(S.part_frame(W, H, i, f)[0], W, H, lay[f], "device" if i % 2 else "host"))
        return capi.part_batch_submit(ctx, streams, frames)

    def check(i, res):
        for j, k in enumerate(kinds):
            _same(res[j], S.part_expected(k, W, H)[i], (i, k))
    assert sum(_found(S.part_expected(k, W, H)[:T]) for k in kinds) > 0
    tk = submit(0)
    for i in range(T):
        nxt = None
        if i + 1 < T:
            if i == 1:
                streams[0].set_input(_layout(lay[R.I420])); fmts[0] = R.I420
            if i == 2:
                streams[1].set_input(None); fmts[1] = None
            nxt = submit(i + 1)
        check(i, capi.part_batch_collect(ctx, tk))
        tk = nxt
    for s in streams:
        s.close()


# ---------------------------------------------------------------- 6. back to BGR
@pytest.mark.parametrize("kind", ["eye", "nose"])
def test_stream_goes_back_to_bgr(env, kind):
    """set_input(None) in the middle of a sequence, and on to I420: one oracle stream fed the equivalent frames throughout"""
    W, H = 640, 480
    exp = S.part_expected(kind, W, H)
    assert _found(exp) > 0
    lay_n, lay_i = S.part_frame(W, H, 0, R.NV12)[1], S.part_frame(W, H, 0, R.I420, pad=16)[1]
    s = _stream(env, kind, lay_n)
    for i in range(S.PART_FRAMES):
        if i == 3:
            s.set_input(None)
        if i == 6:
            s.set_input(_layout(lay_i))
        if i < 3:
            fr = _frame(S.part_frame(W, H, i, R.NV12)[0], W, H, lay_n, "device")
        elif i < 6:
            fr = _bgr_frame(S.part_bgr(W, H, i), "host")
        else:
            fr = _frame(S.part_frame(W, H, i, R.I420, pad=16)[0], W, H, lay_i, "host")
        _same(s.process(fr), exp[i], (kind, i))
    s.close()


# ---------------------------------------------------------------- 7. refusals
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_refusals_leave_the_streams_alone(env, fmt):
    """every bad frame nubovca.h lists is NVCA_ERR_ARG with an error text, alone and in the middle of a batch between good streams; the
    refused calls advance no frame gate: with process-x-every-4-frames = 2 (every other frame analysed) the accepted frames give the
    oracle's sequence on every stream"""
    from nubovca import capi
    ctx = env[0]
    W, H = 640, 480
    n = 6
    props = dict(process_x_every_4_frames=2)
    good_lay = S.part_frame(W, H, 0, fmt, pad=16)[1]
    s = _stream(env, "nose", good_lay, **props)
    before, after = _stream(env, "mouth", None, **props), _stream(env, "eye", S.part_frame(W, H, 0, R.NV12)[1], **props)
    oracles = [S.oracle_part_stream(k, **props) for k in ("nose", "mouth", "eye")]
    bad = _bad_frames(W, H, good_lay)
    seen = 0
    for i in range(n):
        buf, lay = S.part_frame(W, H, i, fmt, pad=16)
        bgr = np.array(S.part_bgr(W, H, i))
        f_before, f_after = _bgr_frame(bgr), _frame(S.part_frame(W, H, i, R.NV12)[0], W, H, S.part_frame(W, H, 0, R.NV12)[1], "host")
        for what, blay, bw, bh, bstride in (bad if i in (1, 2) else bad[:2]):
            s.set_input(_layout(blay))
            keep = np.array(buf)
            fr = capi.Frame(keep.ctypes.data, bw, bh, bstride, capi.MEM_HOST, 0)
            fr._keep = keep
            for streams, frames in (([s], [fr]), ([before, s, after], [f_before, fr, f_after])):
                with pytest.raises(capi.NvcaError) as e:
                    capi.part_batch_process(ctx, streams, frames)
                assert e.value.code == capi.ERR_ARG, (what, e.value)
            assert ctx.L.nvca_last_error(ctx.h), what
        s.set_input(_layout(good_lay))
        res = capi.part_batch_process(ctx, [s, before, after], [_frame(buf, W, H, lay, "host"), f_before, f_after])
        for got, o in zip(res, oracles):
            exp = o.process(bgr)
            _same(got, exp, (fmt, i))
            seen += _found([exp])
    assert seen > 0
    for t in (s, before, after):
        t.close()


def test_refusals_of_set_input(env):
    from nubovca import capi
    s = _stream(env, "nose")
    for lay in ((3, (0, 0, 0), (640, 640, 0)), (-1, (0, 0, 0), (640, 640, 0)), (R.NV12, (0, 640 * 480, 0), (640, 0, 0)), (R.I420, (0, 307200, 384000), (640, 320, -320))):
        with pytest.raises(capi.NvcaError) as e:
            s.set_input(_layout(lay))
        assert e.value.code == capi.ERR_ARG, lay
    # the stream still takes packed frames
    exp = S.part_expected("nose", 640, 480)[0]
    _same(s.process(_bgr_frame(S.part_bgr(640, 480, 0))), exp, "after the refusals")
    assert _found([exp]) > 0
    s.close()
