"""NV12 / I420 trackers (nvca_tracker_set_input) on the GPU against the existing oracle tracker fed the conversion statement's image
(tests/yuv_reference.py) with an alpha plane of 255: boxes bit for bit, in order, frame by frame.  The scenes hold movers that change
the chroma only (tests/yuv_stream_scenes.py; that a tracker which takes Y for gray sees fewer components: tests/test_yuv_streams_cpu.py)."""
import numpy as np
import pytest

import yuv_reference as R
import yuv_stream_scenes as S
from test_gpu_yuv import _bad_frames

pytestmark = pytest.mark.gpu

FMTS = [R.NV12, R.I420]
FMT_IDS = ["nv12", "i420"]
WIDE, GENERAL = "k_trk_pixel_yuv8", "k_trk_pixel_yuv"


@pytest.fixture(scope="module")
def ctx():
    from nubovca import capi
    c = capi.Context(0)
    yield c
    c.close()


def _layout(lay):
    from nubovca import capi
    return capi.pixel_layout(*lay)


_KEEP = []


def _frame(buf, W, H, lay, mem):
    from nubovca import capi
    if mem == "host":
        return capi.make_planar_frame(np.array(buf), W, H, _layout(lay))
    import torch
    t = torch.from_numpy(np.array(buf)).cuda()
    torch.cuda.synchronize()
    _KEEP.append(t)
    return capi.make_planar_frame(t.data_ptr(), W, H, _layout(lay), capi.MEM_DEVICE)


def _bgra_frame(img, mem="host"):
    from nubovca import capi
    if mem == "host":
        return capi.make_frame(np.array(img))
    import torch
    t = torch.from_numpy(np.array(img)).cuda()
    torch.cuda.synchronize()
    _KEEP.append(t)
    return capi.make_frame(t.data_ptr(), img.shape[1], img.shape[0], img.shape[1] * 4, capi.MEM_DEVICE)


def _tracker(ctx, lay=None, **props):
    from nubovca import capi
    t = capi.Tracker(ctx, **props)
    if lay is not None:
        t.set_input(_layout(lay))
    return t


def _one(ctx, t, frame, i):
    from nubovca import capi
    return capi.tracker_batch_process(ctx, [t], [frame], [S.trk_ts(i)], cap=1 << 12)[0]


def _kernels(err):
    return [ln.rsplit(": ", 1)[1] for ln in err.splitlines() if ln.startswith("[nvca plan] 4:2:0 tracker pass")]


# ---------------------------------------------------------------- 1. sequences
# (W, H, plane padding per format, the pixel kernel): tight planes take the wide kernel where w % 4 == 0 and every plane row starts on
# the loads' alignment -- 644-wide tight rows (644 = 8 * 80 + 4) do not, they take it with 4 bytes of row padding, and end in a unit of 4 pixels
SEQ = [(160, 120, {}, WIDE), (644, 482, {}, GENERAL), (644, 482, dict(pad=5), GENERAL), (644, 482, dict(pad=4, chroma_pad_i420=2), WIDE), (322, 242, {}, GENERAL)]


def _kw(kw, fmt):
    out = {k: v for k, v in kw.items() if k != "chroma_pad_i420"}
    if fmt == R.I420 and "chroma_pad_i420" in kw:
        out["chroma_pad"] = kw["chroma_pad_i420"]
    return out


def _run_sequence(ctx, W, H, fmt, kw, mem, kernel, capfd):
    exp = S.trk_expected(W, H)
    assert sum(len(e) for e in exp) > 0
    lay = S.trk_frame(W, H, 0, fmt, **kw)[1]
    capfd.readouterr()
    with ctx.options(plan_debug=1):
        t = _tracker(ctx, lay)
        for i in range(S.TRK_FRAMES):
            got = _one(ctx, t, _frame(S.trk_frame(W, H, i, fmt, **kw)[0], W, H, lay, mem), i)
            assert np.array_equal(got, exp[i]), (W, H, fmt, kw, mem, i, got[:5].tolist(), exp[i][:5].tolist())
        t.close()
    ran = _kernels(capfd.readouterr().err)
    assert ran == [kernel] * S.TRK_FRAMES, (W, H, fmt, kw, mem, ran)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("W,H,kw,kernel", SEQ, ids=lambda v: str(v).replace(" ", ""))
def test_tracker_sequences(ctx, W, H, kw, kernel, fmt, mem, capfd):
    _run_sequence(ctx, W, H, fmt, _kw(kw, fmt), mem, kernel, capfd)


def test_tracker_sequence_1080p(ctx, capfd):
    """the headline size: 7.5 segments a row, from device memory, on the wide kernel"""
    _run_sequence(ctx, 1920, 1080, R.NV12, {}, "device", WIDE, capfd)


# ---------------------------------------------------------------- 2. both sets of component kernels behind the 4:2:0 pixel passes
@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("kw,kernel", [({}, GENERAL), (dict(pad=4), WIDE)], ids=["general", "wide"])
def test_component_kernels_behind_the_yuv_pixel_pass(ctx, fold, kw, kernel, capfd):
    """the flags, the live-segment estimate and the live-tile list of either 4:2:0 pixel kernel feed the folded component path (default)
    and the per-pixel component kernels (trk_fold 0) alike"""
    with ctx.options(trk_fold=fold):
        _run_sequence(ctx, 644, 482, R.NV12, kw, "device", kernel, capfd)


# ---------------------------------------------------------------- 3. format change on a living tracker
def test_format_change_keeps_the_history(ctx):
    """640 x 480: ticks 0 - 2 as BGRA (the statement's image), 3 - 5 as NV12, 6 - 8 as I420, tick 9 as BGRA again -- one oracle tracker fed
    the BGRA frames throughout: the previous gray image and the motion history carry over the changes"""
    W, H = 640, 480
    order = [0, 1, 2, 3, 4, 5, 4, 3, 2, 1]                   # 10 ticks over the scene's 6 frames
    exp = S.oracle_tracker_run([S.trk_bgra(W, H, k) for k in order])
    assert all(len(exp[i]) > 0 for i in (3, 4, 6, 7, 9)), [len(e) for e in exp]          # the ticks right behind a change among them
    lay_n, lay_i = S.trk_frame(W, H, 0, R.NV12)[1], S.trk_frame(W, H, 0, R.I420, pad=8)[1]
    t = _tracker(ctx)
    for i, k in enumerate(order):
        mem = "host" if i % 2 else "device"
        if i == 3:
            t.set_input(_layout(lay_n))
        if i == 6:
            t.set_input(_layout(lay_i))
        if i == 9:
            t.set_input(None)
        if i < 3 or i == 9:
            fr = _bgra_frame(S.trk_bgra(W, H, k), mem)
        elif i < 6:
            fr = _frame(S.trk_frame(W, H, k, R.NV12)[0], W, H, lay_n, mem)
        else:
            fr = _frame(S.trk_frame(W, H, k, R.I420, pad=8)[0], W, H, lay_i, mem)
        got = _one(ctx, t, fr, i)
        assert np.array_equal(got, exp[i]), (i, got[:5].tolist(), exp[i][:5].tolist())
    t.close()


# ---------------------------------------------------------------- 4. mixed batch
def test_mixed_batch(ctx):
    """six trackers in one nvca_tracker_batch_process: two each of BGRA, NV12 and I420, at two frame sizes, host and device frames --
    each against its own oracle tracker over 5 ticks.  The two trackers of a format start one frame apart, so no two slots of a
    launch hold the same picture."""
    from nubovca import capi
    spec = [(640, 480, None, "host", 0), (322, 242, None, "device", 1), (640, 480, R.NV12, "device", 1), (322, 242, R.NV12, "host", 0),
            (640, 480, R.I420, "host", 1), (640, 480, R.I420, "device", 0)]
    lays = [S.trk_frame(W, H, 0, f)[1] if f else None for W, H, f, _, _ in spec]
    trks = [_tracker(ctx, lay) for lay in lays]
    exps = [S.oracle_tracker_run([S.trk_bgra(W, H, (i + d) % S.TRK_FRAMES) for i in range(5)]) for W, H, _, _, d in spec]
    assert all(sum(len(e) for e in ex) > 0 for ex in exps)
    for i in range(5):
        frames = []
        for (W, H, f, mem, d), lay in zip(spec, lays):
            k = (i + d) % S.TRK_FRAMES
            frames.append(_bgra_frame(S.trk_bgra(W, H, k), mem) if f is None else _frame(S.trk_frame(W, H, k, f)[0], W, H, lay, mem))
        res = capi.tracker_batch_process(ctx, trks, frames, [S.trk_ts(i)] * len(spec), cap=1 << 12)
        for s, (got, ex) in enumerate(zip(res, exps)):
            assert np.array_equal(got, ex[i]), (i, spec[s], got[:5].tolist(), ex[i][:5].tolist())
    for t in trks:
        t.close()


# ---------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_refusals_leave_every_history_untouched(ctx, fmt):
    """every bad frame nubovca.h lists is NVCA_ERR_ARG with an error text, alone and in the middle of a batch between a packed and an
    NV12 tracker; the refused calls touch no tracker's previous image, motion history or frame count: the good ticks that follow still
    match the oracle"""
    from nubovca import capi
    W, H = 640, 480
    exp = S.trk_expected(W, H)
    good_lay = S.trk_frame(W, H, 0, fmt, pad=16)[1]
    nv_lay = S.trk_frame(W, H, 0, R.NV12)[1]
    t, before, after = _tracker(ctx, good_lay), _tracker(ctx), _tracker(ctx, nv_lay)
    bad = _bad_frames(W, H, good_lay)
    for i in range(S.TRK_FRAMES):
        buf = S.trk_frame(W, H, i, fmt, pad=16)[0]
        f_before, f_after = _bgra_frame(S.trk_bgra(W, H, i)), _frame(S.trk_frame(W, H, i, R.NV12)[0], W, H, nv_lay, "host")
        for what, blay, bw, bh, bstride in (bad if i in (1, 2) else bad[:2]):
            t.set_input(_layout(blay))
            keep = np.array(buf)
            fr = capi.Frame(keep.ctypes.data, bw, bh, bstride, capi.MEM_HOST, 0)
            fr._keep = keep
            for trks, frames in (([t], [fr]), ([before, t, after], [f_before, fr, f_after])):
                with pytest.raises(capi.NvcaError) as e:
                    capi.tracker_batch_process(ctx, trks, frames, [S.trk_ts(i)] * len(trks))
                assert e.value.code == capi.ERR_ARG, (what, e.value)
            assert ctx.L.nvca_last_error(ctx.h), what
        t.set_input(_layout(good_lay))
        res = capi.tracker_batch_process(ctx, [t, before, after], [_frame(buf, W, H, good_lay, "host"), f_before, f_after], [S.trk_ts(i)] * 3, cap=1 << 12)
        for k, got in enumerate(res):
            assert np.array_equal(got, exp[i]), (fmt, i, k, got[:5].tolist(), exp[i][:5].tolist())
    assert sum(len(e) for e in exp) > 0
    for x in (t, before, after):
        x.close()


def test_refusals_of_set_input_and_packed_trackers_stay_strict(ctx):
    from nubovca import capi
    t = _tracker(ctx)
    for lay in ((3, (0, 0, 0), (640, 640, 0)), (-1, (0, 0, 0), (640, 640, 0)), (R.NV12, (0, 640 * 480, 0), (640, 0, 0)), (R.I420, (0, 307200, 384000), (640, 320, -320))):
        with pytest.raises(capi.NvcaError) as e:
            t.set_input(_layout(lay))
        assert e.value.code == capi.ERR_ARG, lay
    # a tracker that went back to packed frames wants stride >= width * 4 again
    lay = S.trk_frame(640, 480, 0, R.NV12)[1]
    t.set_input(_layout(lay))
    assert len(_one(ctx, t, _frame(S.trk_frame(640, 480, 0, R.NV12)[0], 640, 480, lay, "host"), 0)) == 0
    t.set_input(None)
    with pytest.raises(capi.NvcaError) as e:
        _one(ctx, t, _frame(S.trk_frame(640, 480, 1, R.NV12)[0], 640, 480, lay, "host"), 1)
    assert e.value.code == capi.ERR_ARG
    got = _one(ctx, t, _bgra_frame(S.trk_bgra(640, 480, 1)), 1)
    exp = S.trk_expected(640, 480)[1]
    assert np.array_equal(got, exp) and len(exp) > 0
    t.close()
