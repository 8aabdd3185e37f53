"""NV12 / I420 face streams and nvca_yuv420_to_bgr on the GPU, bit for bit against the conversion statement (tests/yuv_reference.py,
SURVEY.md A.13) and the existing oracle fed the statement's BGR image.  No tolerance anywhere: every comparison is np.array_equal.
The frames and what the oracle makes of them: tests/yuv_cases.py; that the oracle finds boxes in them: tests/test_yuv_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import prefix_cascades as P
import yuv_cases as Y
import yuv_reference as R
from nubovca import synth

pytestmark = pytest.mark.gpu

FMTS = [R.NV12, R.I420]
FMT_IDS = ["nv12", "i420"]
DEFAULT_HIT_CAP = 16384          # csrc/context.h


@pytest.fixture(scope="module")
def ctx():
    from nubovca import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cascs(ctx):
    loaded = {}

    def get(name, k=0):
        if (name, k) not in loaded:
            loaded[(name, k)] = ctx.load_cascade_xml(P.cascade_xml(name, k))
        return loaded[(name, k)]
    return get


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


def _bgr_frame(img, mem):
    from nubovca import capi
    if mem == "host":
        return capi.make_frame(np.array(img))
    import torch
    t = torch.from_numpy(np.array(img)).cuda()
    torch.cuda.synchronize()
    _KEEP.append(t)
    return capi.make_frame(t.data_ptr(), img.shape[1], img.shape[0], img.shape[1] * 3, capi.MEM_DEVICE)


def _yuv_stream(ctx, casc, fset, lay, **props):
    from nubovca import capi
    kw = dict(width_to_process=Y.SETS[fset][2])
    kw.update(props)
    s = capi.FaceStream(ctx, casc, **kw)
    if lay is not None:
        s.set_input(_layout(lay))
    return s


def _same(got, exp, what):
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (what, got[0].tolist(), exp[0].tolist(), got[1].tolist(), exp[1].tolist())


# ---------------------------------------------------------------- 1. the primitive
def _random_frame(w, h, fmt, pad, rows, gap, seed):
    """every plane byte random (the whole value range, clamps on both sides included); the padding too"""
    _, lay = synth.make_yuv420(w, h, 1, fmt, "flat", pad=pad, luma_rows=rows, gap=gap)
    n = max(o + s * (h if p == 0 else h // 2) for p, (o, s) in enumerate(zip(lay[1], lay[2])))
    buf = np.random.default_rng(seed).integers(0, 256, size=n).astype(np.uint8)
    return buf, lay


PRIM_CASES = [(2, 2, 0, None, 0), (2, 2, 3, 4, 5), (34, 18, 0, None, 0), (34, 18, 7, 20, 3), (640, 480, 0, None, 0), (640, 480, 32, 480, 64),
              (1920, 1080, 0, None, 0), (1920, 1080, 0, 1088, 0), (1920, 1080, 64, 1088, 256)]


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("case", PRIM_CASES, ids=lambda c: "%dx%d_pad%d_rows%s_gap%d" % c)
def test_primitive_against_the_statement(ctx, case, fmt, mem):
    from nubovca import capi
    w, h, pad, rows, gap = case
    buf, lay = _random_frame(w, h, fmt, pad, rows, gap, 100 + w + fmt)
    exp = R.bgr(buf, w, h, lay)
    if mem == "host":
        got = ctx.yuv420_to_bgr(buf, w, h, _layout(lay))
    else:
        import torch
        src = torch.from_numpy(buf).cuda()
        ds = w * 3 + 5                                            # padded destination rows: the padding stays as it was
        dst = torch.full((h, ds), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.yuv420_to_bgr(src.data_ptr(), w, h, _layout(lay), capi.MEM_DEVICE, dst.data_ptr(), ds)
        out = dst.cpu().numpy()
        assert (out[:, w * 3:] == 0x5A).all()
        got = out[:, :w * 3].reshape(h, w, 3)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:4].tolist()


# ---------------------------------------------------------------- 2. stream sequences
@pytest.mark.parametrize("pad", [0, 6], ids=["tight", "pad6"])
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("fset,n", [("sd", 9), ("p720", 8), ("hd", 8), ("tail", 8)])
def test_stream_sequences(ctx, cascs, fset, n, fmt, pad):
    """boxes and ids of a stream's frames against the oracle: 640 x 480 at 160 (bilinear), 1280 x 720 at 640 (exact 2 x), 1920 x 1080
    and 328 x 250 at full resolution.  The tight 1920-wide planes take the wide loads (16 pixels a thread); a row padding of 6 bytes,
    and both 328-wide layouts (a luma stride of 328 or 334 is no multiple of 16), the one-pixel-per-thread kernel -- the 328-wide
    frames on the wide kernel: test_full_resolution_rows_that_end_in_a_short_unit.  Host and device frames alternate."""
    W, H = Y.SETS[fset][:2]
    exp = Y.sequence_expected("synthetic", fset, n)
    assert any(len(b) for b, _ in exp) and any(not Y.has_faces(fset, i) for i in range(n))
    _, lay = Y.frame(fset, 0, fmt, pad)
    s = _yuv_stream(ctx, cascs("synthetic"), fset, lay)
    for i in range(n):
        buf, lay_i = Y.frame(fset, i, fmt, pad)
        assert lay_i == lay
        got = ctx.face_batch_process([s], [_frame(buf, W, H, lay, "host" if i % 2 == 0 else "device")])[0]
        _same(got, exp[i], (fset, fmt, pad, i))
    s.close()


def _gray_kernels(err):
    """the gray kernel of every launch of 4:2:0 frames, from the library's plan_debug lines"""
    return [ln.rsplit(": ", 1)[1] for ln in err.splitlines() if ln.startswith("[nvca plan] 4:2:0 gray")]


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_full_resolution_rows_that_end_in_a_short_unit(ctx, cascs, fmt, capfd):
    """328 x 250 at full resolution on k_gray_yuv16: 20 whole 16-pixel units and one of 8 pixels -- the byte-wise tail -- in every
    row pair.  The luma stride is 336 and the chroma stride 336 (NV12) / 168 (I420), so every plane offset and stride takes the wide
    loads; that the wide kernel took every launch is read from the library's plan_debug lines.  The same frames in the tight layout
    (luma stride 328) go through k_gray_yuv_generic; both give the oracle's boxes.  Host and device frames alternate; a second
    pass hands 3 frames of 3 streams over in one call (units of one launch in several slots)."""
    W, H = Y.SETS["tail"][:2]
    n = 8
    exp = Y.sequence_expected("synthetic", "tail", n)
    assert any(len(b) for b, _ in exp)
    for kw, kernel in ((dict(pad=8, chroma_pad=8 if fmt == R.NV12 else 4), "k_gray_yuv16"), (dict(pad=0), "k_gray_yuv_generic")):
        lay = Y.frame("tail", 0, fmt, **kw)[1]
        if kernel == "k_gray_yuv16":
            assert lay[2][0] == 336 and lay[2][1] == (336 if fmt == R.NV12 else 168) and W % 16 == 8
            assert all(o % 16 == 0 for o in lay[1][:2]) and all(o % 8 == 0 for o in lay[1])
        capfd.readouterr()
        with ctx.options(plan_debug=1):
            s = _yuv_stream(ctx, cascs("synthetic"), "tail", lay)
            for i in range(n):
                got = ctx.face_batch_process([s], [_frame(Y.frame("tail", i, fmt, **kw)[0], W, H, lay, "host" if i % 2 == 0 else "device")])[0]
                _same(got, exp[i], (fmt, kw, i))
            s.close()
            three = [_yuv_stream(ctx, cascs("synthetic"), "tail", lay) for _ in range(3)]
            for i in range(3):
                res = ctx.face_batch_process(three, [_frame(Y.frame("tail", i, fmt, **kw)[0], W, H, lay, "device" if k != 1 else "host") for k in range(3)])
                for r in res:
                    _same(r, exp[i], (fmt, kw, "three", i))
            for t in three:
                t.close()
        ran = _gray_kernels(capfd.readouterr().err)
        assert len(ran) == n + 3 and set(ran) == {kernel}, (kw, ran)


def test_wide_kernel_takes_the_tight_1080p_planes(ctx, cascs, capfd):
    """the dispatch of the headline geometry, both formats: tight 1920 x 1080 planes -> k_gray_yuv16; a 6-byte row padding, or a
    shrinking geometry, -> k_gray_yuv_generic"""
    for fmt in FMTS:
        for fset, pad, kernel in (("hd", 0, "k_gray_yuv16"), ("hd", 6, "k_gray_yuv_generic"), ("hd160", 0, "k_gray_yuv_generic")):
            W, H = Y.SETS[fset][:2]
            buf, lay = Y.frame(fset, 0, fmt, pad)
            capfd.readouterr()
            with ctx.options(plan_debug=1):
                s = _yuv_stream(ctx, cascs("synthetic"), fset, lay)
                ctx.face_batch_process([s], [_frame(buf, W, H, lay, "device")])
                s.close()
            assert _gray_kernels(capfd.readouterr().err) == [kernel], (fmt, fset, pad)


def test_stream_goes_back_to_bgr(ctx, cascs):
    """set_input(None) in the middle of a sequence: the stream's state carries over"""
    exp = Y.sequence_expected("synthetic", "sd", 9)
    buf, lay = Y.frame("sd", 0, R.NV12)
    s = _yuv_stream(ctx, cascs("synthetic"), "sd", lay)
    for i in range(6):
        if i == 2:
            s.set_input(None)
        if i == 4:
            s.set_input(_layout(Y.frame("sd", 0, R.I420, 16)[1]))
        if 2 <= i < 4:
            fr = _bgr_frame(Y.frame_bgr("sd", i), "host")
        else:
            b, l = Y.frame("sd", i, R.NV12) if i < 2 else Y.frame("sd", i, R.I420, 16)
            fr = _frame(b, 640, 480, l, "device")
        _same(ctx.face_batch_process([s], [fr])[0], exp[i], i)
    s.close()


# ---------------------------------------------------------------- 3. one batch of BGR, NV12 and I420 streams
def _mixed_streams(ctx, cascs):
    """(stream, set, kind, mem): kind None = BGR"""
    spec = [("sd", None, "host"), ("sd", None, "device"), ("sd", R.NV12, "host"), ("sd", R.NV12, "device"), ("sd", R.I420, "host"),
            ("sd", R.I420, "device"), ("hd", R.NV12, "device"), ("hd", R.I420, "host"), ("p720", R.NV12, "host")]
    return [(_yuv_stream(ctx, cascs("synthetic"), fset, Y.frame(fset, 0, fmt)[1] if fmt else None), fset, fmt, mem) for fset, fmt, mem in spec]


def _mixed_frame(fset, fmt, mem, i):
    W, H = Y.SETS[fset][:2]
    if fmt is None:
        return _bgr_frame(Y.frame_bgr(fset, i), mem)
    buf, lay = Y.frame(fset, i, fmt)
    return _frame(buf, W, H, lay, mem)


def test_mixed_batch(ctx, cascs):
    rounds = 5
    batch = _mixed_streams(ctx, cascs)
    single = _mixed_streams(ctx, cascs)
    for i in range(rounds):
        frames = [_mixed_frame(fset, fmt, mem, i) for (_, fset, fmt, mem) in batch]
        got = ctx.face_batch_process([b[0] for b in batch], frames)
        for k, (s, fset, fmt, mem) in enumerate(single):
            exp = Y.sequence_expected("synthetic", fset, {"sd": 9, "hd": 8, "p720": 8}[fset])[i]
            one = ctx.face_batch_process([s], [frames[k]])[0]
            _same(got[k], exp, ("batch", k, fset, fmt, mem, i))
            _same(one, exp, ("single", k, fset, fmt, mem, i))
    for s in batch + single:
        s[0].close()


# ---------------------------------------------------------------- 4. raw candidate lists of a 32-frame 1080p NV12 batch
def test_raw_lists_of_32_nv12_frames(ctx, cascs):
    """as tests/test_gpu_raw_batch.py: fresh streams with min_neighbors 0 return the raw list of their frame in scan order;
    grouped boxes would hide single windows"""
    from nubovca import capi
    ctx.set_hit_capacity(P.HIT_CAP)
    try:
        exp = [Y.raw_expected("calibrated", 0, "hd", i) for i in range(32)]
        assert sum(len(e) for e in exp) >= 24 * 40
        cap = max(len(e) for e in exp) + 64
        lay = Y.frame("hd", 0, R.NV12)[1]
        streams = [capi.FaceStream(ctx, cascs("calibrated"), width_to_process=1920, multi_scale_factor=10, min_neighbors=0) for _ in range(32)]
        for s in streams:
            s.set_input(_layout(lay))
        frames = [_frame(Y.frame("hd", i, R.NV12)[0], 1920, 1080, lay, "device") for i in range(32)]
        ctx.enable_kernel_timing(1)
        res = ctx.face_batch_process(streams, frames, cap=cap)
        kt = ctx.kernel_timing()
        ctx.enable_kernel_timing(0)
        assert kt["gray_resize_hist"][1] == 1 and kt.get("cascade_band", (0, 0))[1] == 1, kt
        for i, ((boxes, ids), e) in enumerate(zip(res, exp)):
            assert np.array_equal(boxes, e), (i, len(boxes), len(e), P.first_difference(boxes, e))
            assert np.array_equal(ids, np.arange(len(e)))
        for s in streams:
            s.close()
    finally:
        ctx.set_hit_capacity(DEFAULT_HIT_CAP)


# ---------------------------------------------------------------- 5. two batches in flight
def test_submit_collect_two_yuv_batches(ctx, cascs):
    spec = [("sd", R.NV12, "host"), ("sd", R.I420, "device"), ("p720", R.NV12, "device"), ("p720", R.I420, "host"), ("hd", R.NV12, "host"),
            ("hd", R.I420, "device")]
    streams = [_yuv_stream(ctx, cascs("synthetic"), fset, Y.frame(fset, 0, fmt)[1]) for fset, fmt, _ in spec]
    n = 6

    def submit(i):
        return ctx.face_batch_submit(streams, [_mixed_frame(fset, fmt, mem, i) for fset, fmt, mem in spec])

    def check(i, res):
        for k, (fset, fmt, mem) in enumerate(spec):
            _same(res[k], Y.sequence_expected("synthetic", fset, {"sd": 9, "hd": 8, "p720": 8}[fset])[i], (k, fset, fmt, mem, i))
    tickets = [submit(0)]
    for i in range(1, n):
        tickets.append(submit(i))                       # two in flight
        check(i - 1, ctx.face_batch_collect(tickets[i - 1]))
    check(n - 1, ctx.face_batch_collect(tickets[n - 1]))
    for s in streams:
        s.close()


# ---------------------------------------------------------------- 6. sparse ingest
def _rows_read(H, rows_dst):
    """source rows cv::resize(INTER_LINEAR) reads for a destination of rows_dst rows: floor((dy + 0.5) * H / rows_dst - 0.5) and the next, clamped"""
    r = set()
    for dy in range(rows_dst):
        sy = int(np.floor((dy + 0.5) * (H / rows_dst) - 0.5))
        r.update((min(max(sy, 0), H - 1), min(max(sy + 1, 0), H - 1)))
    return r


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("fset,n", [("hd160", 6), ("s5", 6)])
def test_sparse_ingest(ctx, cascs, fset, n, fmt):
    """host frames in shrink-first mode: only the luma rows the resize reads and the chroma rows those use cross the bus.  The same
    results with every other row of every plane set to 0x00 / to 0xFF, with sparse_ingest 1 and 0, and those of the oracle on the
    unchanged frames.  hd160: the rows come at period 12; s5: at period 5 (odd: the chroma rows have no period of their own)."""
    W, H, w2p = Y.SETS[fset][:3]
    scale = W // w2p
    rows_dst = int(np.rint(H / float(scale)))
    luma = _rows_read(H, rows_dst)
    chroma = {r >> 1 for r in luma}
    assert len(luma) * 2 <= H
    exp = Y.sequence_expected("synthetic", fset, n)
    assert any(len(b) for b, _ in exp)
    for sparse in (1, 0):
        for fill in (None, 0x00, 0xFF):
            with ctx.options(sparse_ingest=sparse):
                s = _yuv_stream(ctx, cascs("synthetic"), fset, Y.frame(fset, 0, fmt, 32)[1])
                for i in range(n):
                    buf, lay = Y.frame(fset, i, fmt, 32)
                    buf = np.array(buf)
                    if fill is not None:
                        for p, (o, st) in enumerate(zip(lay[1], lay[2])):
                            keep = luma if p == 0 else chroma
                            for r in range(H if p == 0 else H // 2):
                                if r not in keep:
                                    buf[o + r * st:o + (r + 1) * st] = fill
                    got = ctx.face_batch_process([s], [_frame(buf, W, H, lay, "host")])[0]
                    _same(got, exp[i], (fset, fmt, sparse, fill, i))
                s.close()


def test_sparse_ingest_page_locked(ctx, cascs):
    """the same through registered (page-locked) buffers: the strided copies read the caller's memory directly"""
    W, H = 1920, 1080
    exp = Y.sequence_expected("synthetic", "hd160", 6)
    s = _yuv_stream(ctx, cascs("synthetic"), "hd160", Y.frame("hd160", 0, R.NV12)[1])
    for i in range(4):
        buf, lay = Y.frame("hd160", i, R.NV12)
        buf = np.array(buf)
        ctx.host_register(buf)
        try:
            got = ctx.face_batch_process([s], [_frame(buf, W, H, lay, "host")])[0]
        finally:
            ctx.host_unregister(buf)
        _same(got, exp[i], i)
    s.close()


# ---------------------------------------------------------------- 7. refusals
def _bad_frames(W, H, lay):
    """(what, layout tuple, frame width, height, stride) of every refusal nubovca.h lists, from a good NV12 / I420 layout"""
    fmt, off, st = lay
    plane0 = st[0] * H
    short_c = list(st); short_c[1] = (W if fmt == R.NV12 else W // 2) - 2
    short_y = list(st); short_y[0] = W - 2
    over = list(off); over[1] = plane0 - 32
    out = [("odd width", lay, W - 1, H, st[0]), ("odd height", lay, W, H - 1, st[0]),
           ("luma stride shorter than the row", (fmt, off, tuple(short_y)), W, H, W - 2),
           ("chroma stride shorter than the row", (fmt, off, tuple(short_c)), W, H, st[0]),
           ("planes overlap", (fmt, tuple(over), st), W, H, st[0]),
           ("frame stride is not the layout's", lay, W, H, st[0] + 16)]
    if fmt == R.I420:
        over2 = list(off); over2[2] = off[1] + 8
        out.append(("chroma planes overlap", (fmt, tuple(over2), st), W, H, st[0]))
    return out


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_refusals_leave_the_streams_alone(ctx, cascs, fmt):
    """every refusal is NVCA_ERR_ARG with an error text, alone and inside a batch beside a good stream; the refused calls advance no
    frame gate: with process-x-every-4-frames = 2 (every other frame analysed) the accepted frames give the oracle's sequence"""
    from nubovca import capi
    W, H = Y.SETS["sd"][:2]
    n = 6
    exp = Y.oracle_sequence("synthetic", "sd", n, process_x_every_4=2)
    assert any(len(b) for b, _ in exp)
    good_lay = Y.frame("sd", 0, fmt, 16)[1]
    s = _yuv_stream(ctx, cascs("synthetic"), "sd", good_lay, process_x_every_4_frames=2)
    other = _yuv_stream(ctx, cascs("synthetic"), "sd", None, process_x_every_4_frames=2)
    other_got = []
    bad = _bad_frames(W, H, good_lay)
    for i in range(n):
        buf, lay = Y.frame("sd", i, fmt, 16)
        for what, blay, bw, bh, bstride in (bad if i in (1, 2) else bad[:2]):
            s.set_input(_layout(blay))
            keep = np.array(buf)
            fr = capi.Frame(keep.ctypes.data, bw, bh, bstride, capi.MEM_HOST, 0)
            fr._keep = keep
            for streams, frames in (([s], [fr]), ([other, s], [_bgr_frame(Y.frame_bgr("sd", i), "host"), fr])):
                with pytest.raises(capi.NvcaError) as e:
                    ctx.face_batch_process(streams, frames)
                assert e.value.code == capi.ERR_ARG, (what, e.value)
            assert ctx.L.nvca_last_error(ctx.h), what
        s.set_input(_layout(good_lay))
        _same(ctx.face_batch_process([s], [_frame(buf, W, H, lay, "host")])[0], exp[i], (fmt, i))
        other_got.append(ctx.face_batch_process([other], [_bgr_frame(Y.frame_bgr("sd", i), "host")])[0])
    for i in range(n):
        _same(other_got[i], exp[i], ("the BGR stream of the refused batches", i))
    s.close(); other.close()


def test_refusals_of_set_input_and_the_primitive(ctx, cascs):
    from nubovca import capi
    s = _yuv_stream(ctx, cascs("synthetic"), "sd", None)
    for lay in ((3, (0, 0, 0), (640, 640, 0)), (-1, (0, 0, 0), (640, 640, 0)), (R.NV12, (0, 640 * 480, 0), (640, 0, 0)), (R.I420, (0, 307200, 384000), (640, 320, -320))):
        with pytest.raises(capi.NvcaError) as e:
            s.set_input(_layout(lay))
        assert e.value.code == capi.ERR_ARG, lay
    s.close()
    buf, lay = _random_frame(34, 18, R.I420, 0, None, 0, 3)
    for what, blay, bw, bh, _ in _bad_frames(34, 18, lay):
        if what.startswith("frame stride") or what.startswith("luma stride"):
            continue
        out = np.zeros((18, 34, 3), np.uint8)
        rc = ctx.L.nvca_yuv420_to_bgr(ctx.h, buf.ctypes.data, bw, bh, C.byref(_layout(blay)), capi.MEM_HOST, out.ctypes.data, 34 * 3)
        assert rc == capi.ERR_ARG, what
    out = np.zeros((18, 34, 3), np.uint8)
    assert ctx.L.nvca_yuv420_to_bgr(ctx.h, buf.ctypes.data, 34, 18, C.byref(_layout(lay)), capi.MEM_HOST, out.ctypes.data, 34 * 3 - 1) == capi.ERR_ARG
    assert ctx.L.nvca_yuv420_to_bgr(ctx.h, buf.ctypes.data, 34, 18, C.byref(_layout((0, (0, 0, 0), (34, 0, 0)))), capi.MEM_HOST, out.ctypes.data, 34 * 3) == capi.ERR_ARG
    assert ctx.L.nvca_yuv420_to_bgr(ctx.h, buf.ctypes.data, 34, 18, None, capi.MEM_HOST, out.ctypes.data, 34 * 3) == capi.ERR_ARG


def test_part_streams_and_the_tracker_still_want_packed_frames(ctx):
    """they have no set_input; a frame whose stride is a luma stride is refused as before"""
    from nubovca import capi
    t = capi.Tracker(ctx)
    buf, lay = Y.frame("sd", 0, R.NV12)
    with pytest.raises(capi.NvcaError) as e:
        capi.tracker_batch_process(ctx, [t], [_frame(buf, 640, 480, lay, "host")], [0.0])
    assert e.value.code == capi.ERR_ARG
    t.close()
