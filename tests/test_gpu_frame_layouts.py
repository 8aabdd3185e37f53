"""The packed (gray / BGR / BGRA) entry points on buffers that are not tight, not 16-byte aligned and not a multiple of 4 pixels wide
(tests/frame_layouts.py: the builder, the case lists, the dispatch predicates; tests/test_frame_layouts_cpu.py: the lists cross every
predicate).  Every call goes through the C ABI with an explicit pointer, stride and memory kind; the expected value is the oracle's
answer on the contiguous copy of the same pixels, bit for bit; and every byte of the caller's buffers that is not a pixel the call may
write -- row padding, the margins in front and behind -- must come back as it went in.  All of these are valid inputs under
include/nubovca.h; every byte a correct or a wrongly dispatched kernel can touch lies inside the allocation (frame_layouts.MARGIN)."""
import ctypes as C
import functools

import numpy as np
import pytest

import frame_layouts as FL
from draw_reference import _ref as draw_ref
from overlay_reference import overlay_blend as overlay_ref

pytestmark = pytest.mark.gpu
HOST, DEV = FL.HOST, FL.DEVICE


@pytest.fixture(scope="module")
def ctx():
    from nubovca import capi
    assert (capi.MEM_HOST, capi.MEM_DEVICE) == (HOST, DEV)
    c = capi.Context(0)
    yield c
    c.close()


class Buf:
    """an image in a buffer (frame_layouts.build) in host or device memory: the pointer to hand over, the image and the guard bytes back"""

    def __init__(self, px, stride, off, mem, seed=0, fill=None):
        px = np.asarray(px, np.uint8)
        self.h, self.w = px.shape[:2]
        self.cn = 1 if px.ndim == 2 else px.shape[2]
        self.stride, self.off, self.mem = stride, off, mem
        self.before = FL.build(px, stride, off, seed, fill)
        if mem == DEV:
            import torch
            self.t = torch.from_numpy(self.before.copy()).cuda()
            torch.cuda.synchronize()
            assert self.t.data_ptr() % FL.ALLOC_ALIGN == 0
            self.ptr = self.t.data_ptr() + FL.start(off)
        else:
            self.a = self.before.copy()
            self.ptr = self.a.ctypes.data + FL.start(off)

    def now(self):
        if self.mem == DEV:
            import torch
            torch.cuda.synchronize()
            return self.t.cpu().numpy()
        return self.a

    def image(self):
        return FL.pixels(self.now(), self.h, self.w, self.cn, self.stride, self.off)

    def guards_ok(self):
        return FL.outside_unchanged(self.before, self.now(), self.h, self.w, self.cn, self.stride, self.off)

    def untouched(self):
        return bool(np.array_equal(self.before, self.now()))

    def frame(self, pts=0):
        from nubovca import capi
        f = capi.Frame(self.ptr, self.w, self.h, self.stride, self.mem, pts)
        f._keep = self
        return f


def _show(bad, n=6):
    """the first failing cases, one a line (pytest shortens a list's repr)"""
    return "%d case(s):\n" % len(bad) + "\n".join(repr(b) for b in bad[:n])


def _rand(shape, seed, lo=0, hi=255):
    return np.random.default_rng(seed).integers(lo, hi + 1, shape, dtype=np.uint8)


def _fresh(h, w, cn, seed):
    """what a destination holds before the call: noise, so that a pixel the call did not write shows"""
    return _rand((h, w) if cn == 1 else (h, w, cn), [seed, 99])


# ---------------------------------------------------------------- primitives
@pytest.mark.parametrize("cn", [3, 4])
def test_bgr2gray(ctx, cn):
    import orc
    bad = []
    for i, c in enumerate(FL.GRAY_CASES[cn]):
        w, h, mem = c["w"], c["h"], c["mem"]
        px = _rand((h, w, cn), [cn, i])
        src, dst = Buf(px, c["stride"], c["off"], mem, seed=i), Buf(_fresh(h, w, 1, i), c["dstride"], c["doff"], mem, seed=1000 + i)
        ctx.check(ctx.L.nvca_bgr2gray(ctx.h, src.ptr, w, h, src.stride, cn, mem, dst.ptr, dst.stride))
        ctx.synchronize()
        if not (np.array_equal(dst.image(), orc.bgr2gray(px)) and dst.guards_ok() and src.untouched()):
            bad.append((c, int((dst.image() != orc.bgr2gray(px)).sum()), dst.guards_ok(), src.untouched()))
    assert not bad, _show(bad)


def _plane_call(ctx, fn, c, px, i, fill=None):
    """one call of a gray -> gray primitive on case c: (destination image, guards of the destination intact, source as it must be left)"""
    h, w = px.shape
    src = Buf(px, c["stride"], c["off"], c["mem"], seed=i, fill=fill)
    if c["mode"] == "inplace":
        dst = src
    else:
        dst = Buf(_fresh(h, w, 1, i), c["dstride"], c["doff"], c["mem"], seed=1000 + i, fill=fill)
    ctx.check(fn(ctx.h, src.ptr, w, h, src.stride, c["mem"], dst.ptr, dst.stride))
    ctx.synchronize()
    return dst.image(), dst.guards_ok(), (src.guards_ok() if dst is src else src.untouched())


def test_equalize_hist(ctx):
    import orc
    bad = []
    for i, c in enumerate(FL.EQUALIZE_CASES):
        lo, hi = sorted(int(v) for v in np.random.default_rng([5, i]).integers(0, 256, 2))
        px = _rand((c["h"], c["w"]), [6, i], lo, hi)
        got, guards, src_ok = _plane_call(ctx, ctx.L.nvca_equalize_hist, c, px, i)
        if not (np.array_equal(got, orc.equalize_hist(px)) and guards and src_ok):
            bad.append((c, int((got != orc.equalize_hist(px)).sum()), guards, src_ok))
    assert not bad, _show(bad)


@pytest.mark.parametrize("mode", ["host", "device", "inplace"])
def test_equalize_hist_does_not_count_padding(ctx, mode):
    """padding brighter than every pixel, darker than every pixel, and mid-gray padding around an all-white image (one occupied bin:
    cv::equalizeHist sets the image to that value -- unless the histogram saw anything else)"""
    import orc
    bad = []
    for i, (w, h, sk, off, pix, fill) in enumerate([(255, 9, "plus", 1, (10, 200), 255), (5, 17, "align16", 4, (10, 200), 255), (255, 9, "align16", 0, (10, 200), 0),
                                                    (257, 8, "plus", 8, (255, 255), (10, 200)), (7, 7, "align16", 16, (255, 255), (10, 200))]):
        stride = FL.stride_of(sk, w, 1)
        c = dict(mode=mode, mem=HOST if mode == "host" else DEV, stride=stride, off=off, dstride=FL.stride_of("align4", w, 1) + 4, doff=1)
        px = _rand((h, w), [7, i], *pix)
        got, guards, src_ok = _plane_call(ctx, ctx.L.nvca_equalize_hist, c, px, i, fill=fill)
        if not (np.array_equal(got, orc.equalize_hist(px)) and guards and src_ok):
            bad.append((w, h, stride, off, fill, int((got != orc.equalize_hist(px)).sum()), guards, src_ok))
    assert not bad, _show(bad)


def test_flip_horizontal(ctx):
    import orc
    bad = []
    for i, c in enumerate(FL.FLIP_CASES):
        px = _rand((c["h"], c["w"]), [8, i])
        got, guards, src_ok = _plane_call(ctx, ctx.L.nvca_flip_horizontal, c, px, i)
        if not (np.array_equal(got, orc.flip_h(px)) and guards and src_ok):
            bad.append((c, int((got != orc.flip_h(px)).sum()), guards, src_ok))
    assert not bad, _show(bad)


def test_resize_linear(ctx):
    import orc
    bad = []
    for i, c in enumerate(FL.RESIZE_CASES):
        (sw, sh, dw, dh), cn, mem = c["geo"], c["cn"], c["mem"]
        px = _rand((sh, sw) if cn == 1 else (sh, sw, cn), [9, i])
        src, dst = Buf(px, c["stride"], c["off"], mem, seed=i), Buf(_fresh(dh, dw, cn, i), c["dstride"], c["doff"], mem, seed=1000 + i)
        ctx.check(ctx.L.nvca_resize_linear(ctx.h, src.ptr, sw, sh, src.stride, cn, mem, dst.ptr, dw, dh, dst.stride))
        ctx.synchronize()
        exp = orc.resize_linear(px, dw, dh)
        if not (np.array_equal(dst.image(), exp) and dst.guards_ok() and src.untouched()):
            bad.append((c, int((dst.image() != exp).sum()), dst.guards_ok(), src.untouched()))
    assert not bad, _show(bad)


def test_integrals(ctx):
    import orc
    bad = []
    for i, (w, h, sk, off) in enumerate(FL.INTEGRAL_CASES):
        px = _rand((h, w), [10, i])
        src = Buf(px, FL.stride_of(sk, w, 1), off, HOST, seed=i)
        s, q, t = np.empty((h + 1, w + 1), np.int32), np.empty((h + 1, w + 1), np.float64), np.empty((h + 1, w + 1), np.int32)
        ctx.check(ctx.L.nvca_integral(ctx.h, src.ptr, w, h, src.stride, HOST, s.ctypes.data_as(C.POINTER(C.c_int32)), q.ctypes.data_as(C.POINTER(C.c_double))))
        ctx.check(ctx.L.nvca_integral_tilted(ctx.h, src.ptr, w, h, src.stride, HOST, t.ctypes.data_as(C.POINTER(C.c_int32))))
        es, eq = orc.integral(px)
        ok = (np.array_equal(s, es), np.array_equal(q, eq), np.array_equal(t, orc.integral_tilted(px)), src.untouched())
        if not all(ok):
            bad.append((w, h, sk, off) + ok)
    assert not bad, _show(bad)


# ---------------------------------------------------------------- detection on a view
@functools.lru_cache(maxsize=None)
def _view_parent():
    import orc
    from nubovca import synth
    full = orc.equalize_hist(synth.make_gray(FL.VIEW_PARENT_W, FL.VIEW_PARENT_H, 21, "natural", [(90, 60, 80)]))
    full.setflags(write=False)
    return full


def _crop(view):
    x0, y0, w, h = view
    return np.ascontiguousarray(_view_parent()[y0:y0 + h, x0:x0 + w])


def _detect_on_view(ctx, casc, parent, view, raw, sf, mn, flags, ms):
    from nubovca import capi
    x0, y0, w, h = view
    ptr = parent.ptr + y0 * parent.stride + x0
    cap = 1 << 16
    buf, n = (capi.Rect * cap)(), C.c_int()
    if raw:
        ctx.check(ctx.L.nvca_detect_raw(ctx.h, casc.h, ptr, w, h, parent.stride, parent.mem, sf, flags, ms[0], ms[1], 0, 0, buf, cap, C.byref(n)))
    else:
        ctx.check(ctx.L.nvca_detect_multiscale(ctx.h, casc.h, ptr, w, h, parent.stride, parent.mem, sf, mn, flags, ms[0], ms[1], 0, 0, buf, cap, C.byref(n)))
    assert n.value <= cap
    return np.frombuffer(buf, np.int32).reshape(cap, 4)[:n.value].copy()


_VIEW_EXPECTED = {}          # the oracle's answers, computed once: (cascade name, view, sf, ms, raw or grouped, flags) -> boxes


def _view_expected(name, ocasc, view, sf, ms, raw, fl):
    import orc
    key = (name, view, sf, ms, raw, fl)
    if key not in _VIEW_EXPECTED:
        _VIEW_EXPECTED[key] = orc.detect_raw(ocasc, _crop(view), sf, fl, ms) if raw else orc.detect_multiscale(ocasc, _crop(view), sf, 2, fl, ms)
    return _VIEW_EXPECTED[key]


def _view_sweep(ctx, name, casc, ocasc, parent, view, sf=1.1, ms=(20, 20)):
    """raw lists (flags 0, SCALE_IMAGE) and grouped boxes (0, SCALE_IMAGE, FIND_BIGGEST) of the view against the oracle on the crop"""
    from nubovca import capi
    bad, nraw = [], 0
    for fl in (0, capi.HAAR_SCALE_IMAGE):
        exp = _view_expected(name, ocasc, view, sf, ms, True, fl)
        got = _detect_on_view(ctx, casc, parent, view, True, sf, 0, fl, ms)
        nraw += len(exp)
        if len(exp) < 1 or not np.array_equal(got, exp):
            bad.append(("raw", fl, len(got), len(exp)))
    for fl in (0, capi.HAAR_SCALE_IMAGE, capi.HAAR_FIND_BIGGEST_OBJECT):
        exp = _view_expected(name, ocasc, view, sf, ms, False, fl)
        got = _detect_on_view(ctx, casc, parent, view, False, sf, 2, fl, ms)
        if not np.array_equal(got, exp):
            bad.append(("grouped", fl, got.tolist(), exp.tolist()))
    if not parent.untouched():
        bad.append("the parent image changed")
    return bad, nraw


@pytest.mark.parametrize("which", ["synth", "small"])
@pytest.mark.parametrize("roi", [1, 0])
@pytest.mark.parametrize("mem,pstride,off", FL.VIEW_CASES)
def test_detect_on_a_view(ctx, synth_xml, small_xml, orc_cascade, orc_small, which, roi, mem, pstride, off):
    """a sub-matrix of a parent image that lives in device memory (the pointer is odd) or in host memory with padded rows, at
    160 x 150 -- too large for the one-launch small-image detector (kRoiMaxWords): plan, pre-pass and tiles either way -- at 4-byte
    aligned columns (the integral kernels read a device view where it is) and at 120 x 110, which k_roi takes when "roi" is on: on a device
    view it reads img[y * stride + x] of the caller's memory"""
    casc = ctx.load_cascade_xml(synth_xml if which == "synth" else small_xml)
    ocasc = orc_cascade if which == "synth" else orc_small
    parent = Buf(_view_parent(), pstride, off, mem, seed=3)
    try:
        with ctx.options(roi=roi):
            for view in (FL.VIEW, FL.VIEW_ALIGNED, FL.VIEW_SMALL):
                ctx.enable_kernel_timing(1)
                bad, nraw = _view_sweep(ctx, which, casc, ocasc, parent, view)
                kt = ctx.kernel_timing()
                ctx.enable_kernel_timing(0)
                assert not bad and nraw >= 2, (view, _show(bad))
                if view == FL.VIEW_SMALL and roi:
                    assert kt.get("cascade_roi", (0, 0))[1] >= 5 and "cascade_tile" not in kt, kt
                else:
                    assert "cascade_roi" not in kt, kt
    finally:
        ctx.enable_kernel_timing(0)
        casc.free()


@pytest.mark.parametrize("mem,pstride,off", FL.VIEW_CASES)
def test_detect_on_a_view_tilted_cascade(ctx, mem, pstride, off):
    """a cascade with tilted features: k_tilted / k_pyr_tilted behind the staged copy of a strided view"""
    import orc
    from nubovca import synth
    xml = synth.generic_cascade_xml(seed=11, stage_sizes=(3, 6, 9, 12, 15), tilt_frac=0.3, tree_frac=0.0)
    casc, ocasc = ctx.load_cascade_xml(xml), orc.parse_cascade_xml(xml)
    assert casc.kind()[0]
    parent = Buf(_view_parent(), pstride, off, mem, seed=4)
    try:
        for view in (FL.VIEW, FL.VIEW_ALIGNED):
            bad, nraw = _view_sweep(ctx, "tilted", casc, ocasc, parent, view, sf=1.2, ms=(0, 0))
            assert not bad and nraw >= 2, (view, _show(bad))
    finally:
        casc.free()


# ---------------------------------------------------------------- face streams
def _stream_frame(s, t, seed0, H=FL.STREAM_H):
    from nubovca import synth
    W = FL.STREAM_W
    return synth.make_bgr(W, H, seed0 + 37 * s + t, "natural", [(30 + 12 * t + 9 * s, H // 6, H // 2)])


# the face cascade with the stream's defaults (grouped boxes: what the element emits), and a six-stage cascade at scale factor 1.10 with
# min_neighbors 1: dozens of boxes a frame, down to the window size, up to the frame's last column -- grouped boxes of a strict cascade stay
# what they are when a column of the gray image is wrong, these do not (tried on the oracle: 13 of 16 frames change)
FACE_SETUPS = {"default": ("synth", {}, {}), "lenient": ("small", dict(multi_scale_factor=10, min_neighbors=1), dict(scale_factor_pct=10, min_neighbors=1))}


def _face_run(ctx, xmls, orcs, setup, layouts, w2p, seed0, ticks=4, H=FL.STREAM_H):
    import orc
    from nubovca import capi
    which, props, oprops = FACE_SETUPS[setup]
    casc = ctx.load_cascade_xml(xmls[which])
    streams = [capi.FaceStream(ctx, casc, width_to_process=w2p, **props) for _ in layouts]
    oracles = [orc.FaceStream(orcs[which], width_to_process=w2p, **oprops) for _ in layouts]
    seen, bad = 0, []
    for t in range(ticks):
        px = [_stream_frame(s, t, seed0, H) for s in range(len(layouts))]
        bufs = [Buf(px[s], stride, off, mem, seed=10 * t + s) for s, (mem, stride, off) in enumerate(layouts)]
        res = ctx.face_batch_process(streams, [b.frame() for b in bufs], cap=256)
        for s in range(len(layouts)):
            eb, eid = oracles[s].process(px[s])
            assert len(eb) < 256
            seen += len(eb)
            if not (np.array_equal(res[s][0], eb) and np.array_equal(res[s][1], eid) and bufs[s].untouched()):
                bad.append((t, s, layouts[s], len(res[s][0]), len(eb), res[s][0].tolist()[:3], eb.tolist()[:3], bufs[s].untouched()))
    for st in streams:
        st.close()
    casc.free()
    return seen, bad


@pytest.fixture(scope="module")
def face_cascades(synth_xml, small_xml, orc_cascade, orc_small):
    return {"synth": synth_xml, "small": small_xml}, {"synth": orc_cascade, "small": orc_small}


@pytest.mark.parametrize("setup", sorted(FACE_SETUPS))
@pytest.mark.parametrize("w2p", [FL.STREAM_W, 160])
def test_face_streams_mixed_layouts(ctx, face_cascades, w2p, setup):
    """one batched call per tick over a padded host frame, a tight device frame, and two device frames with 976-byte rows, one of them at
    a base 4 bytes off: three launch sets of the gray kernel (frame_layouts.face_launch_sets), at width-to-process 322 the fast kernel
    with its tail, the generic one by stride and the generic one by base; at 160 the shrinking resize and the sparse ingest of the host
    frame's rows"""
    seen, bad = _face_run(ctx, *face_cascades, setup, FL.STREAM_MIXED, w2p, 8000)
    assert not bad and seen >= 8, (seen, _show(bad, 3))


@pytest.mark.parametrize("setup", sorted(FACE_SETUPS))
def test_face_streams_sparse_ingest_of_padded_rows(ctx, face_cascades, setup):
    """322 x 240 at width-to-process 80: only rows 4 k + 1 and 4 k + 2 of a host frame cross to the device, as one strided copy whose pitch is
    4 * stride (frame_layouts.row_runs) -- here with 968-byte rows, beside device frames of the other layouts; every tick's frame differs,
    so a row that was needed and not copied shows as the row of the tick before"""
    seen, bad = _face_run(ctx, *face_cascades, setup, FL.STREAM_MIXED + FL.STREAM_HOST_PADDED[:1], FL.SPARSE_W2P, 8800, H=FL.SPARSE_H)
    assert not bad and seen >= 8, (seen, _show(bad, 3))


@pytest.mark.parametrize("setup", sorted(FACE_SETUPS))
def test_face_streams_host_frames_padded_to_4(ctx, face_cascades, setup):
    """322-pixel BGR rows 968 bytes apart (GStreamer's align4), identity geometry: k_gray_fast4 with its byte-wise tail behind 80 whole
    vectors of every row, histogram included.  (Face streams take 3-channel frames only -- nvca_frame of a packed stream is BGR,
    face_submit checks stride >= 3 * width and reads 3 bytes a pixel -- so there is no BGRA run here: 4-channel rows go through
    nvca_bgr2gray above and through the tracker below.)"""
    seen, bad = _face_run(ctx, *face_cascades, setup, FL.STREAM_HOST_PADDED, FL.STREAM_W, 8500)
    assert not bad and seen >= 8, (seen, _show(bad, 3))


# ---------------------------------------------------------------- part streams
@pytest.mark.parametrize("kind", ["eye", "nose"])
def test_part_streams_mixed_layouts(ctx, synth_xml, kind):
    """the four layouts in one nvca_part_batch_process call, each stream with a scene of its own: the eye detector's full-size gray
    image, equalization and k_work_resize; the nose detector's kWorkBgr taps on the caller's stride"""
    import orc
    from nubovca import capi, synth
    from part_scenes import scene
    k, a, b = {"eye": (capi.PART_EYE, "righteye", "lefteye"), "nose": (capi.PART_NOSE, "nose", None)}[kind]
    xml = {n: synth.synthetic_part_cascade_xml(n) for n in (a, b) if n}
    xml["face"] = synth_xml
    dev = {n: ctx.load_cascade_xml(x) for n, x in xml.items()}
    cpu = {n: orc.parse_cascade_xml(x) for n, x in xml.items()}
    layouts = FL.STREAM_MIXED
    streams = [capi.PartStream(ctx, k, dev["face"], dev[a], dev[b] if b else None) for _ in layouts]
    oracles = [orc.PartStream(k, cpu["face"], cpu[a], cpu[b] if b else None) for _ in layouts]
    scenes = [scene(FL.STREAM_W, FL.STREAM_H, 4, 7100 + 50 * s) for s in range(len(layouts))]
    seen, bad = 0, []
    for t in range(4):
        bufs = [Buf(scenes[s][t], stride, off, mem, seed=10 * t + s) for s, (mem, stride, off) in enumerate(layouts)]
        res = capi.part_batch_process(ctx, streams, [bf.frame() for bf in bufs])
        for s in range(len(layouts)):
            ea, eb = oracles[s].process(scenes[s][t])
            seen += len(ea) + len(eb)
            if not (np.array_equal(res[s][0], ea) and np.array_equal(res[s][1], eb) and bufs[s].untouched()):
                bad.append((t, s, layouts[s], res[s][0].tolist(), ea.tolist(), res[s][1].tolist(), eb.tolist(), bufs[s].untouched()))
    for st in streams:
        st.close()
    for c in dev.values():
        c.free()
    assert not bad and seen >= 4, (seen, _show(bad, 2))


# ---------------------------------------------------------------- tracker
def _moving_block(W, H, n, seed):
    """BGRA frames: a textured static background and a bright 40 x 20 block that moves 8 pixels a frame"""
    rng = np.random.default_rng(seed)
    bg = rng.integers(60, 120, (H, W, 3), dtype=np.uint8)
    x0, y0 = int(rng.integers(0, W // 4)), int(rng.integers(0, H - 20))
    out = []
    for f in range(n):
        img = np.empty((H, W, 4), np.uint8)
        img[..., :3] = bg
        img[..., 3] = rng.integers(0, 256, (H, W), dtype=np.uint8)          # alpha is not read: let it be anything
        img[y0:y0 + 20, x0 + 8 * f:x0 + 8 * f + 40, :3] = (231, 229, 233)
        out.append(img)
    return out


def _tracker_run(ctx, members, mem, seed0, ticks=5):
    """one batched call a tick over `members` (frame_layouts.TRACKER_CASES rows), each tracker with a scene of its own"""
    import orc
    from nubovca import capi
    trks, otrs = [capi.Tracker(ctx) for _ in members], [orc.Tracker() for _ in members]
    scenes = [_moving_block(w, h, ticks, seed0 + s) for s, (_, w, h, _, _) in enumerate(members)]
    seen, bad = 0, []
    for t in range(ticks):
        ts = 1000.0 + 33.3 * t
        bufs = [Buf(scenes[s][t], stride, off, mem, seed=10 * t + s) for s, (_, _, _, stride, off) in enumerate(members)]
        res = capi.tracker_batch_process(ctx, trks, [b.frame() for b in bufs], [ts] * len(members))
        for s in range(len(members)):
            exp = otrs[s].process(scenes[s][t], ts, cap=1 << 16)
            seen += len(exp)
            if not (np.array_equal(res[s], exp) and bufs[s].untouched()):
                bad.append((t, members[s][0], res[s].tolist()[:4], exp.tolist()[:4], bufs[s].untouched()))
    for tr in trks:
        tr.close()
    return seen, bad


@pytest.mark.parametrize("mem", FL.MEMS)
@pytest.mark.parametrize("case", FL.TRACKER_CASES, ids=[c[0] for c in FL.TRACKER_CASES])
def test_tracker_layouts(ctx, case, mem):
    seen, bad = _tracker_run(ctx, [case], mem, 40)
    assert not bad and seen >= 3, (seen, _show(bad, 3))


@pytest.mark.parametrize("mem", FL.MEMS)
def test_tracker_wide_and_offset_frames_in_one_call(ctx, mem):
    """one launch set whose members could take k_trk_pixel4 but for ONE base 4 bytes off (device memory): the whole launch takes
    k_trk_pixel, and every tracker still answers for its own scene"""
    seen, bad = _tracker_run(ctx, FL.TRACKER_MIXED, mem, 70)
    assert not bad and seen >= 9, (seen, _show(bad, 3))


# ---------------------------------------------------------------- drawing on device frames
@pytest.mark.parametrize("cn,sk,off", FL.DRAW_CASES)
def test_draw_shapes_on_strided_device_frames(ctx, cn, sk, off):
    W, H = FL.DRAW_W, FL.DRAW_H
    px = _rand((H, W, cn), [11, cn, off])
    frame = Buf(px, FL.draw_stride(sk, cn), off, DEV, seed=5)
    ctx.draw_shapes(frame.frame(), cn, FL.DRAW_SHAPES)
    ctx.synchronize()
    exp = draw_ref(px.copy(), FL.DRAW_SHAPES)
    assert (exp != px).any()
    assert np.array_equal(frame.image(), exp), int((frame.image() != exp).sum())
    assert frame.guards_ok()


@pytest.mark.parametrize("ocn", [3, 4])
@pytest.mark.parametrize("cn,sk,off", FL.OVERLAY_CASES)
def test_overlay_on_strided_device_frames(ctx, cn, sk, off, ocn):
    """one box whose scaled image is clipped at the right and at the bottom edge of the frame: the last written byte of every row is the
    row's last pixel, the last written row the frame's last"""
    from nubovca import capi
    W, H = FL.DRAW_W, FL.DRAW_H
    px = _rand((H, W, 3), [12, off, ocn])
    img = _rand((23, 31, ocn), [13, ocn])
    frame = Buf(px, FL.draw_stride(sk, 3), off, DEV, seed=6)
    capi.overlay_blend(ctx, frame.frame(), [FL.OVERLAY_BOX], img)
    ctx.synchronize()
    exp = overlay_ref(px.copy(), [FL.OVERLAY_BOX], img)
    assert (exp[-1, -1] != px[-1, -1]).any() or ocn == 4
    assert np.array_equal(frame.image(), exp), int((frame.image() != exp).sum())
    assert frame.guards_ok()
