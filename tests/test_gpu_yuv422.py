"""Packed 4:2:2 frames (YUY2, UYVY, YVYU) on the GPU: nvca_yuv422_to_bgr, face streams, part streams and trackers, bit for bit against
the conversion statement (tests/yuv422_reference.py) and the existing oracle fed the statement's BGR image.  No tolerance
anywhere: every comparison is np.array_equal.  The frames, the case lists and the two wide-kernel predicates: tests/yuv422_cases.py; that
the cases tell a kernel apart which shares chroma between rows, confuses the byte orders or takes Y for gray: tests/test_yuv422_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import prefix_cascades as P
import yuv_cases as Y
import yuv_reference as R420
import yuv422_cases as K
import yuv422_reference as R
import yuv_stream_scenes as S

pytestmark = pytest.mark.gpu

KIND_LIST = ["eye", "nose", "mouth", "ear"]


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


@pytest.fixture(scope="module")
def parts(ctx):
    return {n: ctx.load_cascade_xml(x) for n, (x, _) in S.part_cascades().items()}


def _layout(lay):
    from nubovca import capi
    return capi.pixel_layout(*lay)


_KEEP = []


def _device(buf, shift=0):
    """device address of a copy of the buffer that starts `shift` bytes behind a 256-byte boundary"""
    import torch
    t = torch.empty(len(buf) + shift, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 256 == 0
    t[shift:] = torch.from_numpy(np.array(buf))
    torch.cuda.synchronize()
    _KEEP.append(t)
    return t.data_ptr() + shift


def _frame(buf, W, H, lay, mem, shift=0):
    """a Frame of the buffer in host memory (a writable copy that ends with the last pixel) or device memory (kept for the module); shift:
    bytes its first byte lies behind an aligned address"""
    from nubovca import capi
    if mem == "host":
        keep = np.empty(len(buf) + shift + 64, np.uint8)
        a = (-keep.ctypes.data) % 64 + shift
        view = keep[a:a + len(buf)]
        view[:] = buf
        fr = capi.Frame(view.ctypes.data, W, H, lay[2][0], capi.MEM_HOST, 0)
        fr._keep = keep
        return fr
    return capi.Frame(_device(buf, shift), W, H, lay[2][0], capi.MEM_DEVICE, 0)


def _bgr_frame(img, mem, channels=3):
    from nubovca import capi
    if mem == "host":
        return capi.make_frame(np.array(img))
    return capi.make_frame(_device(np.array(img).reshape(-1)), img.shape[1], img.shape[0], img.shape[1] * channels, capi.MEM_DEVICE)


def _face_stream(ctx, casc, fset, lay, **props):
    from nubovca import capi
    kw = dict(width_to_process=Y.SETS[fset][2])
    kw.update(props)
    s = capi.FaceStream(ctx, casc, **kw)
    if lay is not None:
        s.set_input(_layout(lay))
    return s


def _same(got, exp, what):
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (what, got[0].tolist(), exp[0].tolist(), got[1].tolist(), exp[1].tolist())


def _lines(err, what):
    return [ln.rsplit(": ", 1)[1] for ln in err.splitlines() if ln.startswith("[nvca plan] 4:2:2 " + what)]


# ---------------------------------------------------------------- 1. the primitive
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("fmt", R.FMTS, ids=R.FMT_IDS)
def test_primitive_against_the_statement(ctx, fmt, mem):
    """every case of K.PRIM_CASES: the pixels are the statement's, and every byte of the destination outside them -- the bytes in front of
    the first row, the row padding, the bytes behind the last pixel -- is unchanged"""
    from nubovca import capi
    import torch
    for (w, h, pad, base) in K.PRIM_CASES:
        buf, lay = K.random_frame(w, h, fmt, pad, base, 100 * w + h + fmt)
        assert len(buf) == R.extent(w, h, lay)
        exp = R.bgr(buf, w, h, lay)
        ds, lead = w * 3 + 5, 7
        n = lead + ds * (h - 1) + w * 3 + 9
        canvas = np.random.default_rng(w + h).integers(0, 256, size=n).astype(np.uint8)
        if mem == "host":
            src = _frame(buf, w, h, lay, "host", base)                   # (the pointer as far off alignment as the offset)
            out = canvas.copy()
            rc = ctx.L.nvca_yuv422_to_bgr(ctx.h, src.data, w, h, C.byref(_layout(lay)), capi.MEM_HOST, out.ctypes.data + lead, ds)
            assert rc == 0, (w, h, pad, base, ctx.L.nvca_last_error(ctx.h))
        else:
            dst = torch.from_numpy(canvas).cuda()
            ctx.yuv422_to_bgr(_device(buf, base), w, h, _layout(lay), capi.MEM_DEVICE, dst.data_ptr() + lead, ds)
            out = dst.cpu().numpy()
        want = canvas.copy()
        idx = lead + np.arange(h)[:, None] * ds + np.arange(w * 3)[None, :]
        want[idx] = exp.reshape(h, w * 3)
        assert np.array_equal(out[idx].reshape(h, w, 3), exp), (w, h, pad, base, np.argwhere(out[idx].reshape(h, w, 3) != exp)[:4].tolist())
        assert np.array_equal(out, want), (w, h, pad, base, "bytes outside the pixels changed", np.flatnonzero(out != want)[:8].tolist())
    _KEEP.clear()


def test_primitive_host_binding_and_1080p(ctx):
    buf, lay = K.hd_frame(R.UYVY)
    assert np.array_equal(ctx.yuv422_to_bgr(buf, 1920, 1080, _layout(lay)), R.bgr(buf, 1920, 1080, lay))


# ---------------------------------------------------------------- 2. face streams
@pytest.mark.parametrize("fmt", R.FMTS, ids=R.FMT_IDS)
@pytest.mark.parametrize("fset,n", [("sd", 9), ("p720", 8), ("tail", 8)])
def test_face_stream_sequences(ctx, cascs, fset, n, fmt):
    """640 x 480 at 160 (bilinear shrink), 1280 x 720 at 640 (exact 2 x), 328 x 250 at full resolution; tight rows for one byte order,
    padded rows and a base offset for the others; host and device frames alternate"""
    W, H = Y.SETS[fset][:2]
    exp = Y.sequence_expected("synthetic", fset, n)
    assert any(len(b) for b, _ in exp) and any(not Y.has_faces(fset, i) for i in range(n))
    pad, base = {R.YUY2: (0, 0), R.UYVY: (6, 2), R.YVYU: (16, 32)}[fmt]
    lay = K.frame(fset, 0, fmt, pad, base)[1]
    s = _face_stream(ctx, cascs("synthetic"), fset, lay)
    for i in range(n):
        buf, lay_i = K.frame(fset, i, fmt, pad, base)
        assert lay_i == lay
        _same(ctx.face_batch_process([s], [_frame(buf, W, H, lay, "host" if i % 2 == 0 else "device")])[0], exp[i], (fset, fmt, i))
    s.close()


@pytest.mark.parametrize("fmt", R.FMTS, ids=R.FMT_IDS)
def test_face_stream_on_a_chroma_varying_1080p_frame(ctx, cascs, fmt, capfd):
    """the shape the wide kernel is for, on a frame whose rows carry their own chroma: a kernel that shares chroma between rows computes
    another image and gets another raw list (tests/test_yuv422_cpu.py, premise (a)).  Raw candidate lists of a fresh min_neighbors-0 stream,
    in scan order, as tests/test_gpu_yuv.py compares them: grouped boxes would hide single windows"""
    from nubovca import capi
    buf, lay = K.hd_frame(fmt)
    exp = K.hd_expected()
    assert len(exp) >= 40
    ctx.set_hit_capacity(P.HIT_CAP)
    try:
        capfd.readouterr()
        with ctx.options(plan_debug=1):
            s = capi.FaceStream(ctx, cascs("calibrated"), width_to_process=1920, multi_scale_factor=10, min_neighbors=0)
            s.set_input(_layout(lay))
            boxes, ids = ctx.face_batch_process([s], [_frame(buf, 1920, 1080, lay, "device")], cap=len(exp) + 64)[0]
            s.close()
        assert _lines(capfd.readouterr().err, "gray") == [K.GRAY_WIDE]
        assert np.array_equal(boxes, exp), (fmt, len(boxes), len(exp), P.first_difference(boxes, exp))
        assert np.array_equal(ids, np.arange(len(exp)))
    finally:
        ctx.set_hit_capacity(16384)          # csrc/context.h's default


@pytest.mark.parametrize("case", K.FACE_KERNEL_CASES, ids=lambda c: "%s_pad%d_off%d_ptr%d_%s" % c)
def test_both_gray_kernels_on_both_sides_of_the_predicate(ctx, cascs, case, capfd):
    """the plan_debug line names the kernel the predicate (tests/yuv422_cases.py, gray_wide) asks for, and either kernel gives the oracle's
    boxes; 328-wide rows on the wide kernel end in a unit of 8 pixels; two streams in one call: units of one launch in two slots"""
    fset, pad, base, shift, mem = case
    W, H = Y.SETS[fset][:2]
    exp = Y.sequence_expected("synthetic", fset, {"tail": 8, "sd": 9}[fset])
    fmt = R.FMTS[(pad + base + shift) % 3]
    lay = K.frame(fset, 0, fmt, pad, base)[1]
    capfd.readouterr()
    with ctx.options(plan_debug=1):
        two = [_face_stream(ctx, cascs("synthetic"), fset, lay) for _ in range(2)]
        for i in range(3):
            buf = K.frame(fset, i, fmt, pad, base)[0]
            for r in ctx.face_batch_process(two, [_frame(buf, W, H, lay, mem, shift) for _ in two]):
                _same(r, exp[i], (case, i))
        for s in two:
            s.close()
    assert _lines(capfd.readouterr().err, "gray") == [K.face_kernel(case)] * 3, case


def _rows_read(H, rows_dst):
    r = set()
    for dy in range(rows_dst):
        sy = int(np.floor((dy + 0.5) * (H / rows_dst) - 0.5))
        r.update((min(max(sy, 0), H - 1), min(max(sy + 1, 0), H - 1)))
    return r


@pytest.mark.parametrize("fset,fmt", [("hd160", R.UYVY), ("s5", R.YVYU)])
def test_sparse_ingest(ctx, cascs, fset, fmt):
    """host frames in shrink-first mode: only the rows the resize reads cross the bus (every row carries its own chroma: nothing else is
    needed).  The same results with every other row set to 0x00 / 0xFF, with sparse_ingest 1 and 0"""
    W, H, w2p = Y.SETS[fset][:3]
    rows_dst = int(np.rint(H / float(W // w2p)))
    keep = _rows_read(H, rows_dst)
    assert len(keep) * 2 <= H
    n = 3
    exp = Y.sequence_expected("synthetic", fset, 6)
    assert any(len(b) for b, _ in exp[:n])
    for sparse in (1, 0):
        for fill in (None, 0x00, 0xFF):
            with ctx.options(sparse_ingest=sparse):
                lay = K.frame(fset, 0, fmt, 32, 0)[1]
                s = _face_stream(ctx, cascs("synthetic"), fset, lay)
                for i in range(n):
                    buf = np.array(K.frame(fset, i, fmt, 32, 0)[0])
                    if fill is not None:
                        for r in range(H):
                            if r not in keep:
                                buf[r * lay[2][0]:min((r + 1) * lay[2][0], len(buf))] = fill
                    _same(ctx.face_batch_process([s], [_frame(buf, W, H, lay, "host")])[0], exp[i], (fset, sparse, fill, i))
                s.close()


def test_mixed_batch_of_bgr_nv12_and_two_byte_orders(ctx, cascs):
    """BGR, NV12, YUY2, UYVY and YVYU streams in one call (launch groups of their own per layout), against streams fed alone"""
    spec = [("sd", None, "host"), ("sd", "nv12", "device"), ("sd", R.YUY2, "host"), ("sd", R.UYVY, "device"), ("sd", R.YVYU, "device"), ("tail", R.YVYU, "device"),
            ("tail", R.YUY2, "host"), ("p720", R.UYVY, "host")]

    def lay_of(fset, fmt):
        return None if fmt is None else Y.frame(fset, 0, R420.NV12)[1] if fmt == "nv12" else K.frame(fset, 0, fmt)[1]

    def frame_of(fset, fmt, mem, i):
        W, H = Y.SETS[fset][:2]
        if fmt is None:
            return _bgr_frame(Y.frame_bgr(fset, i), mem)
        buf, lay = Y.frame(fset, i, R420.NV12) if fmt == "nv12" else K.frame(fset, i, fmt)
        return _frame(buf, W, H, lay, mem)
    batch = [_face_stream(ctx, cascs("synthetic"), fset, lay_of(fset, fmt)) for fset, fmt, _ in spec]
    single = [_face_stream(ctx, cascs("synthetic"), fset, lay_of(fset, fmt)) for fset, fmt, _ in spec]
    for i in range(4):
        frames = [frame_of(fset, fmt, mem, i) for fset, fmt, mem in spec]
        got = ctx.face_batch_process(batch, frames)
        for k, (fset, fmt, mem) in enumerate(spec):
            exp = Y.sequence_expected("synthetic", fset, {"sd": 9, "tail": 8, "p720": 8}[fset])[i]
            _same(got[k], exp, ("batch", k, fset, fmt, mem, i))
            _same(ctx.face_batch_process([single[k]], [frames[k]])[0], exp, ("single", k, fset, fmt, mem, i))
    for s in batch + single:
        s.close()


def test_two_tickets_in_flight_across_a_layout_change(ctx, cascs):
    """a submitted ticket keeps the layout it was submitted with: frame i goes in as YUY2, the stream changes to padded UYVY (then to BGR,
    then to YVYU with a base offset), frame i + 1 goes in, and only then ticket i is collected"""
    W, H = Y.SETS["sd"][:2]
    exp = Y.sequence_expected("synthetic", "sd", 9)
    forms = [(R.YUY2, 0, 0), (R.UYVY, 6, 0), None, (R.YVYU, 0, 16)]
    s = _face_stream(ctx, cascs("synthetic"), "sd", None)

    def submit(i):
        form = forms[i % len(forms)]
        if form is None:
            s.set_input(None)
            return ctx.face_batch_submit([s], [_bgr_frame(Y.frame_bgr("sd", i), "host")])
        buf, lay = K.frame("sd", i, *form)
        s.set_input(_layout(lay))
        return ctx.face_batch_submit([s], [_frame(buf, W, H, lay, "device" if i % 2 else "host")])
    n = 8
    tickets = [submit(0)]
    for i in range(1, n):
        tickets.append(submit(i))
        _same(ctx.face_batch_collect(tickets[i - 1])[0], exp[i - 1], i - 1)
    _same(ctx.face_batch_collect(tickets[n - 1])[0], exp[n - 1], n - 1)
    s.close()


def test_lbp_and_new_format_haar_streams(ctx):
    """one LBP and one new-format HAAR stream made with nvca_face_stream_create_any, fed UYVY / YVYU frames in one call"""
    import haar_new_stream_cases as HS
    import lbp_stream_cases as LS
    from nubovca import capi
    pairs = []
    for mod, xml, fmt in ((LS, LS.cascade("w24")[0], R.UYVY), (HS, HS.K.cascade("w24")[0], R.YVYU)):
        frames = mod.frames_of(mod.CASES["identity"])
        casc = ctx.load_cascade_xml(xml)
        s = capi.FaceStream(ctx, casc, any_format=True, width_to_process=160, multi_scale_factor=25, min_neighbors=3, process_x_every_4_frames=4)
        ex = mod.Expected("w24", capi.PIX_NV12, width_to_process=160, scale_factor_pct=25, min_neighbors=3, process_x_every_4=4)
        packed = [R.from_420(*mod.yuv(f, capi.PIX_NV12)[:1], 160, 120, mod.yuv(f, capi.PIX_NV12)[1], fmt, pad=4) for f in frames]
        for (buf, lay), f in zip(packed, frames):
            assert np.array_equal(R.bgr(buf, 160, 120, lay), mod.bgr(f, capi.PIX_NV12))
        s.set_input(_layout(packed[0][1]))
        pairs.append((s, ex, frames, packed))
    seen = 0
    for r in range(3):
        res = ctx.face_batch_process([p[0] for p in pairs], [_frame(p[3][r][0], 160, 120, p[3][r][1], "host" if r % 2 else "device") for p in pairs], 1024)
        for k, (s, ex, frames, _) in enumerate(pairs):
            e = ex.process(frames[r])
            seen += len(e[0])
            _same(res[k], e, (k, r))
    assert seen > 0
    for p in pairs:
        p[0].close()


# ---------------------------------------------------------------- 3. part streams
def _part_stream(ctx, parts, kind, lay=None, **props):
    from nubovca import capi
    k, a, b = S.KINDS[kind]
    s = capi.PartStream(ctx, k, parts["face"], parts[a], parts[b] if b else None, **props)
    if lay is not None:
        s.set_input(_layout(lay))
    return s


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("fmt", R.FMTS, ids=R.FMT_IDS)
@pytest.mark.parametrize("W,H", K.PART_GEOS, ids=lambda v: str(v))
def test_part_stream_sequences(ctx, parts, W, H, fmt, mem, capfd):
    """every kind at 640 x 480 (the exact-2x resize; the eye chain's gray image on the wide kernel where the rows take it) and 322 x 242
    (every tail, the unaligned eye-gray pitch), four streams on one frame in one call"""
    from nubovca import capi
    pad, base = {R.YUY2: (0, 0), R.UYVY: (6, 2), R.YVYU: (16, 16)}[fmt]
    lay = K.part_frame(W, H, 0, fmt, pad, base)[1]
    exps = [S.part_expected(kind, W, H) for kind in KIND_LIST]
    assert all(sum(len(a) + len(b) for a, b in e[:K.PART_FRAMES]) > 0 for e in exps)
    capfd.readouterr()
    with ctx.options(plan_debug=1):
        streams = [_part_stream(ctx, parts, kind, lay) for kind in KIND_LIST]
        for i in range(K.PART_FRAMES):
            fr = _frame(K.part_frame(W, H, i, fmt, pad, base)[0], W, H, lay, mem)
            res = capi.part_batch_process(ctx, streams, [fr] * 4)
            for kind, got, e in zip(KIND_LIST, res, exps):
                _same(got, e[i], (kind, W, H, fmt, mem, i))
        for s in streams:
            s.close()
    ran = _lines(capfd.readouterr().err, "eye gray")
    wide = W % 16 == 0 and lay[1][0] % 16 == 0 and lay[2][0] % 16 == 0
    assert ran and set(ran) == {K.GRAY_WIDE if wide else K.GRAY_GENERIC}, (W, H, fmt, ran)


def test_part_streams_mix_with_bgr_and_nv12_and_go_back_to_bgr(ctx, parts):
    """BGR, NV12, YUY2 and UYVY video streams with the same content, two detectors on each, in one call; then the 4:2:2 streams go back
    to BGR in the middle of the sequence"""
    from nubovca import capi
    W, H = 640, 480
    kinds = ["eye", "nose"]
    lays = [None, S.part_frame(W, H, 0, R420.NV12)[1], K.part_frame(W, H, 0, R.YUY2)[1], K.part_frame(W, H, 0, R.UYVY, 8, 0)[1]]
    streams = [[_part_stream(ctx, parts, k, lay) for k in kinds] for lay in lays]
    seen = 0
    for i in range(K.PART_FRAMES):
        bgr = np.array(S.part_bgr(W, H, i))
        if i == 3:
            for v in (2, 3):
                for s in streams[v]:
                    s.set_input(None)
        frames = [_bgr_frame(bgr, "device" if i % 2 else "host"), _frame(S.part_frame(W, H, i, R420.NV12)[0], W, H, lays[1], "host" if i % 2 else "device")]
        if i < 3:
            frames += [_frame(K.part_frame(W, H, i, R.YUY2)[0], W, H, lays[2], "device"), _frame(K.part_frame(W, H, i, R.UYVY, 8, 0)[0], W, H, lays[3], "host")]
        else:
            frames += [_bgr_frame(bgr, "host"), _bgr_frame(bgr, "device")]
        res = capi.part_batch_process(ctx, [s for v in streams for s in v], [frames[v] for v in range(4) for _ in kinds])
        for v in range(4):
            for j, kind in enumerate(kinds):
                exp = S.part_expected(kind, W, H)[i]
                _same(res[v * 2 + j], exp, (i, v, kind))
                seen += len(exp[0]) + len(exp[1])
    assert seen > 0
    for v in streams:
        for s in v:
            s.close()


# ---------------------------------------------------------------- 4. trackers
def _tracker(ctx, lay=None, **props):
    from nubovca import capi
    t = capi.Tracker(ctx, **props)
    if lay is not None:
        t.set_input(_layout(lay))
    return t


def _track(ctx, trackers, frames, i):
    from nubovca import capi
    return capi.tracker_batch_process(ctx, trackers, frames, [S.trk_ts(i)] * len(trackers), cap=1 << 12)


@pytest.mark.parametrize("case", K.TRK_CASES, ids=lambda c: "%dx%d_pad%d_off%d_ptr%d_%s" % c)
def test_tracker_sequences_on_both_pixel_kernels(ctx, case, capfd):
    """boxes of the 6 frames against the oracle tracker, on the kernel the predicate (tests/yuv422_cases.py, trk_wide) asks for; the scenes'
    odd-numbered movers change the chroma only; 160 x 121: an odd height"""
    W, H, pad, base, shift, mem = case
    fmt = R.FMTS[(W // 2 + pad + base + shift) % 3]
    exp = K.trk_expected(W, H)
    assert sum(len(e) for e in exp) > 0
    lay = K.trk_frame(W, H, 0, fmt, pad, base)[1]
    capfd.readouterr()
    with ctx.options(plan_debug=1):
        t = _tracker(ctx, lay)
        for i in range(S.TRK_FRAMES):
            got = _track(ctx, [t], [_frame(K.trk_frame(W, H, i, fmt, pad, base)[0], W, H, lay, mem, shift)], i)[0]
            assert np.array_equal(got, exp[i]), (case, fmt, i, got[:5].tolist(), exp[i][:5].tolist())
        t.close()
    assert _lines(capfd.readouterr().err, "tracker pass") == [K.trk_kernel(case)] * S.TRK_FRAMES, case


def test_tracker_format_change_keeps_gray_and_history(ctx):
    """BGRA, YUY2, NV12, YVYU, UYVY (padded) and BGRA frames on one living tracker: the boxes of the unbroken sequence"""
    W, H = 644, 482
    exp = K.trk_expected(W, H)
    forms = [None, (R.YUY2, 0, 0), "nv12", (R.YVYU, 0, 0), (R.UYVY, 8, 8), None]
    t = _tracker(ctx)
    for i, form in enumerate(forms):
        if form is None:
            t.set_input(None)
            fr = _bgr_frame(K.trk_bgra(W, H, i), "host" if i else "device", 4)
        elif form == "nv12":
            buf, lay = S.trk_frame(W, H, i, R420.NV12)
            t.set_input(_layout(lay))
            fr = _frame(buf, W, H, lay, "device")
        else:
            buf, lay = K.trk_frame(W, H, i, *form)
            t.set_input(_layout(lay))
            fr = _frame(buf, W, H, lay, "host" if i % 2 else "device")
        got = _track(ctx, [t], [fr], i)[0]
        assert np.array_equal(got, exp[i]), (i, form, got[:5].tolist(), exp[i][:5].tolist())
    t.close()


def test_packed_nv12_and_uyvy_trackers_in_one_call(ctx):
    W, H = 160, 120
    exp = K.trk_expected(W, H)
    lays = [None, S.trk_frame(W, H, 0, R420.NV12)[1], K.trk_frame(W, H, 0, R.UYVY)[1], K.trk_frame(W, H, 0, R.YUY2, 2, 0)[1], K.trk_frame(160, 121, 0, R.UYVY)[1]]
    trackers = [_tracker(ctx, lay) for lay in lays]
    exp121 = K.trk_expected(160, 121)
    for i in range(S.TRK_FRAMES):
        frames = [_bgr_frame(K.trk_bgra(W, H, i), "host", 4), _frame(S.trk_frame(W, H, i, R420.NV12)[0], W, H, lays[1], "device"),
                  _frame(K.trk_frame(W, H, i, R.UYVY)[0], W, H, lays[2], "device"), _frame(K.trk_frame(W, H, i, R.YUY2, 2, 0)[0], W, H, lays[3], "host"),
                  _frame(K.trk_frame(160, 121, i, R.UYVY)[0], 160, 121, lays[4], "host")]
        res = _track(ctx, trackers, frames, i)
        for k in range(4):
            assert np.array_equal(res[k], exp[i]), (i, k)
        assert np.array_equal(res[4], exp121[i]), i
    for t in trackers:
        t.close()


# ---------------------------------------------------------------- 5. refusals
def _bad_422(W, H, lay):
    """(what, layout tuple, frame width, height, stride) of every refusal nubovca.h lists for packed 4:2:2"""
    fmt, off, st = lay
    return [("odd width", lay, W - 1, H, st[0]), ("stride[0] < 2 * w", (fmt, off, (2 * W - 2, 0, 0)), W, H, 2 * W - 2),
            ("frame stride is not the layout's", lay, W, H, st[0] + 16), ("zero height", lay, W, 0, st[0])]


@pytest.mark.parametrize("fmt", R.FMTS, ids=R.FMT_IDS)
def test_refusals_leave_the_streams_alone(ctx, cascs, parts, fmt):
    """every refusal is NVCA_ERR_ARG with an error text, alone and beside a good stream, for face streams, part streams and trackers; no
    stream advances: with every other frame analysed the accepted frames give the oracle's sequence, and the tracker's boxes are those of
    the unbroken sequence"""
    from nubovca import capi
    W, H = Y.SETS["sd"][:2]
    n = 4
    exp = Y.oracle_sequence("synthetic", "sd", n, process_x_every_4=2)
    good_lay = K.frame("sd", 0, fmt, 16, 0)[1]
    s = _face_stream(ctx, cascs("synthetic"), "sd", good_lay, process_x_every_4_frames=2)
    other = _face_stream(ctx, cascs("synthetic"), "sd", None, process_x_every_4_frames=2)
    ps = _part_stream(ctx, parts, "nose", good_lay)
    tw, th = 160, 120
    trk_lay = K.trk_frame(tw, th, 0, fmt)[1]
    t = _tracker(ctx, trk_lay)
    trk_exp = K.trk_expected(tw, th)
    bad = _bad_422(W, H, good_lay)
    other_got = []
    for i in range(n):
        buf = K.frame("sd", i, fmt, 16, 0)[0]
        for what, blay, bw, bh, bstride in bad:
            keep = np.array(buf)
            fr = capi.Frame(keep.ctypes.data, bw, bh, bstride, capi.MEM_HOST, 0)
            fr._keep = keep
            s.set_input(_layout(blay)); ps.set_input(_layout(blay))
            for streams, frames in (([s], [fr]), ([other, s], [_bgr_frame(Y.frame_bgr("sd", i), "host"), fr])):
                with pytest.raises(capi.NvcaError) as e:
                    ctx.face_batch_process(streams, frames)
                assert e.value.code == capi.ERR_ARG and ctx.L.nvca_last_error(ctx.h), (what, e.value)
            with pytest.raises(capi.NvcaError) as e:
                capi.part_batch_process(ctx, [ps], [fr])
            assert e.value.code == capi.ERR_ARG and ctx.L.nvca_last_error(ctx.h), (what, e.value)
        for what, blay, bw, bh, bstride in _bad_422(tw, th, trk_lay):
            keep = np.array(K.trk_frame(tw, th, i, fmt)[0])
            fr = capi.Frame(keep.ctypes.data, bw, bh, bstride, capi.MEM_HOST, 0)
            fr._keep = keep
            t.set_input(_layout(blay))
            with pytest.raises(capi.NvcaError) as e:
                _track(ctx, [t], [fr], i)
            assert e.value.code == capi.ERR_ARG and ctx.L.nvca_last_error(ctx.h), (what, e.value)
        s.set_input(_layout(good_lay)); ps.set_input(_layout(good_lay)); t.set_input(_layout(trk_lay))
        _same(ctx.face_batch_process([s], [_frame(buf, W, H, good_lay, "host")])[0], exp[i], (fmt, i))
        other_got.append(ctx.face_batch_process([other], [_bgr_frame(Y.frame_bgr("sd", i), "host")])[0])
        got = _track(ctx, [t], [_frame(K.trk_frame(tw, th, i, fmt)[0], tw, th, trk_lay, "host")], i)[0]
        assert np.array_equal(got, trk_exp[i]), (fmt, i)
    for i in range(n):
        _same(other_got[i], exp[i], ("the BGR stream of the refused batches", i))
    s.close(); other.close(); ps.close(); t.close()


def test_refusals_of_set_input_and_the_primitive(ctx, cascs, parts):
    """format 3 and format 7 are no formats, for every set_input and for the primitive; the primitive refuses a null layout, a 4:2:0 or
    BGR layout, an odd width, a short stride and a short destination stride -- every time with NVCA_ERR_ARG and, with a layout given, an error text"""
    from nubovca import capi
    s = _face_stream(ctx, cascs("synthetic"), "sd", None)
    ps = _part_stream(ctx, parts, "nose")
    t = _tracker(ctx)
    for fmt in (3, 7, -1):
        for obj in (s, ps, t):
            with pytest.raises(capi.NvcaError) as e:
                obj.set_input(_layout((fmt, (0, 0, 0), (1280, 0, 0))))
            assert e.value.code == capi.ERR_ARG and ctx.L.nvca_last_error(ctx.h), (fmt, obj)
    with pytest.raises(capi.NvcaError) as e:
        s.set_input(_layout((R.YUY2, (0, 0, 0), (0, 0, 0))))
    assert e.value.code == capi.ERR_ARG
    s.set_input(_layout((R.YUY2, (0, 5, 6), (1280, -3, 7))))          # planes 1 .. 2 are ignored
    s.close(); ps.close(); t.close()
    w, h = 34, 17
    buf, lay = K.random_frame(w, h, R.YUY2, 0, 0, 3)
    out = np.zeros((h, w, 3), np.uint8)

    def call(layout, bw=w, bh=h, ds=w * 3):
        return ctx.L.nvca_yuv422_to_bgr(ctx.h, buf.ctypes.data, bw, bh, None if layout is None else C.byref(_layout(layout)), capi.MEM_HOST, out.ctypes.data, ds)
    assert call(lay) == 0
    assert call(None) == capi.ERR_ARG
    for what, bad in (("format 3", (3,) + lay[1:]), ("format 7", (7,) + lay[1:]), ("BGR", (0,) + lay[1:]), ("NV12", (R420.NV12, (0, 34 * 18, 0), (34, 34, 0))),
                      ("short stride", (R.YUY2, (0, 0, 0), (2 * w - 1, 0, 0)))):
        assert call(bad) == capi.ERR_ARG and ctx.L.nvca_last_error(ctx.h), what
    assert call(lay, bw=w - 1) == capi.ERR_ARG and call(lay, bh=0) == capi.ERR_ARG and call(lay, ds=w * 3 - 1) == capi.ERR_ARG
    # the 4:2:0 entry points do not take packed 4:2:2 layouts
    assert ctx.L.nvca_yuv420_to_bgr(ctx.h, buf.ctypes.data, w, 16, C.byref(_layout(lay)), capi.MEM_HOST, out.ctypes.data, w * 3) == capi.ERR_ARG
