"""The way out in 4:2:0 on the GPU: nvca_bgr_to_yuv420 (both kernels, host and device memory), nvca_draw_shapes_yuv420 and
nvca_overlay_blend_yuv420 on device frames, bit for bit against the numpy statement (tests/yuv_out_reference.py) and
the host loops, with 0xA5 in every byte no sample lies in -- in front of the buffer, in the row padding, between the planes, behind
the last one -- which must survive.  Every comparison is np.array_equal but the round trip's derived 2 / 1 / 2 bound.  The shapes are
the smallest at which each kernel can go wrong, plus one 1080p frame a call."""
import numpy as np
import pytest

import draw_reference
import yuv_cases as Y
import yuv_out_cases as K
import yuv_out_reference as S
import yuv_reference as R

pytestmark = pytest.mark.gpu

WIDE, GENERIC = "k_bgr_yuv16", "k_bgr_yuv_generic"
HEAD = 256          # sentinel bytes in front of every destination buffer


@pytest.fixture(scope="module")
def ctx():
    from nubovca import capi
    c = capi.Context(0)
    yield c
    c.close()


def _layout(lay):
    from nubovca import capi
    return capi.pixel_layout(*lay)


def _lay64(w, h, fmt):
    """planes one behind the other, every stride rounded up to 64 bytes"""
    def up(v):
        return (v + 63) // 64 * 64
    if fmt == S.NV12:
        return (fmt, (0, up(w) * h), (up(w), up(w)))
    return (fmt, (0, up(w) * h, up(w) * h + up(w // 2) * (h // 2)), (up(w), up(w // 2), up(w // 2)))


def _dst(w, h, lay, seed, rows=None):
    """a destination buffer: HEAD sentinel bytes, the frame (random samples, 0xA5 elsewhere; `rows`: allocated luma rows), 37 sentinel bytes"""
    fmt, off, st = lay
    n = S.extent(w, h, lay) if rows is None else max(off[p] + st[p] * (rows if p == 0 else rows // 2) for p in range(len(off)))
    buf = np.full(HEAD + n + 37, K.SENTINEL, np.uint8)
    rng = np.random.default_rng(seed)
    S.write(buf[HEAD:], w, h, lay, rng.integers(0, 256, (h, w)).astype(np.uint8), rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint8),
            rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint8))
    return buf


def _kernels(err):
    return [ln.rsplit(": ", 1)[1] for ln in err.splitlines() if ln.startswith("[nvca plan] BGR to 4:2:0")]


# ---------------------------------------------------------------- 1. the conversion
# name -> (w, h, channels, bytes added to a source row, layout maker, allocated luma rows, bytes the destination base is moved by,
#          kernel for device memory, kernel for host memory -- a host frame is staged: its stride and its base play no part)
def _tight(w, h, fmt):
    return K.layout_of(w, h, fmt)


def _rows1088(w, h, fmt):
    return K.layout_of(w, h, fmt, luma_rows=1088)


CONVERT = {
    "2x2": (2, 2, 3, 0, _tight, None, 0, GENERIC, GENERIC),                      # one block: no 16-pixel strip in it
    "16x2": (16, 2, 3, 0, _tight, None, 0, WIDE, WIDE),                          # one strip
    "32x4": (32, 4, 3, 0, _tight, None, 0, WIDE, WIDE),
    "48x34_stride64": (48, 34, 3, 0, _lay64, None, 0, WIDE, WIDE),               # three strips a row, 17 row pairs: more than one workgroup row
    "18x6": (18, 6, 3, 0, _tight, None, 0, GENERIC, GENERIC),                    # tails
    "30x10": (30, 10, 3, 0, _tight, None, 0, GENERIC, GENERIC),
    "32x4_srcstride": (32, 4, 3, 1, _tight, None, 0, GENERIC, WIDE),             # rows 3 * w + 1 bytes apart
    "32x4_base8": (32, 4, 3, 0, _tight, None, 8, GENERIC, WIDE),
    "32x4_bgra": (32, 4, 4, 0, _tight, None, 0, GENERIC, GENERIC),
}


def _convert_case(ctx, capfd, name, case, fmt, mem):
    from nubovca import capi
    w, h, cn, spad, mk, rows, shift, kdev, khost = case
    lay = mk(w, h, fmt)
    rng = np.random.default_rng(w * 131 + h + cn)
    stride = w * cn + spad
    src = rng.integers(0, 256, (h, stride)).astype(np.uint8)
    img = src[:, :w * cn].reshape(h, w, cn)
    dst0 = _dst(w, h, lay, 9 + w, rows)
    exp = np.array(dst0)
    exp[HEAD + shift:] = S.convert(img, dst0[HEAD + shift:], w, h, lay)
    got = np.array(dst0)
    capfd.readouterr()
    with ctx.options(plan_debug=1):
        if mem == "host":
            ctx.bgr_to_yuv420(img, w, h, _layout(lay), got[HEAD + shift:])
        else:
            import torch
            ds, dd = torch.from_numpy(src).cuda(), torch.from_numpy(got).cuda()
            torch.cuda.synchronize()
            assert dd.data_ptr() % 256 == 0 and ds.data_ptr() % 256 == 0
            ctx.bgr_to_yuv420(ds.data_ptr(), w, h, _layout(lay), dd.data_ptr() + HEAD + shift, capi.MEM_DEVICE, stride, cn)
            got = dd.cpu().numpy()
    ran = _kernels(capfd.readouterr().err)
    assert ran == [kdev if mem == "device" else khost], (name, fmt, mem, ran)
    assert np.array_equal(got, exp), (name, fmt, mem, np.flatnonzero(got != exp)[:8].tolist())


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
@pytest.mark.parametrize("name", list(CONVERT))
def test_conversion_against_the_statement(ctx, capfd, name, fmt, mem):
    _convert_case(ctx, capfd, name, CONVERT[name], fmt, mem)


@pytest.mark.parametrize("fmt,mem", [(S.NV12, "device"), (S.I420, "host")], ids=["nv12-device", "i420-host"])
def test_conversion_1080p_in_a_1088_row_layout(ctx, capfd, fmt, mem):
    _convert_case(ctx, capfd, "1080p", (1920, 1080, 3, 0, _rows1088, 1088, 0, WIDE, WIDE), fmt, mem)


@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
def test_round_trip_on_the_device(ctx, fmt):
    """nvca_yuv420_to_bgr(nvca_bgr_to_yuv420(F)) for block-constant F: within 2 / 1 / 2 (B / G / R), the bound that holds over all 2^24 colours"""
    import torch
    from nubovca import capi
    rng = np.random.default_rng(21)
    w, h = 160, 96
    lv = np.arange(0, 256, 17)
    cols = np.concatenate([np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), axis=-1).reshape(-1, 3), rng.integers(0, 256, (w * h, 3))])[:(w // 2) * (h // 2)]
    img = np.repeat(np.repeat(cols.astype(np.uint8).reshape(h // 2, w // 2, 3), 2, axis=0), 2, axis=1)
    lay = K.layout_of(w, h, fmt)
    ds = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    dy = torch.zeros(S.extent(w, h, lay), dtype=torch.uint8, device="cuda")
    db = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.bgr_to_yuv420(ds.data_ptr(), w, h, _layout(lay), dy.data_ptr(), capi.MEM_DEVICE)
    ctx.yuv420_to_bgr(dy.data_ptr(), w, h, _layout(lay), capi.MEM_DEVICE, db.data_ptr(), w * 3)
    d = np.abs(db.cpu().numpy().astype(int) - img.astype(int)).reshape(-1, 3).max(axis=0)
    assert d[0] <= 2 and d[1] <= 1 and d[2] <= 2, d.tolist()


# ---------------------------------------------------------------- 2. drawing on device frames
def _on_device(buf):
    """(tensor, device pointer of the frame) of a host buffer behind HEAD sentinel bytes"""
    import torch
    t = torch.from_numpy(np.concatenate([np.full(HEAD, K.SENTINEL, np.uint8), buf])).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr() + HEAD


def _back(t):
    out = t.cpu().numpy()
    assert (out[:HEAD] == K.SENTINEL).all()
    return out[HEAD:]


@pytest.mark.parametrize("layout", list(K.LAYOUTS))
@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
def test_device_draw_against_the_statement_and_the_host_loops(ctx, fmt, layout):
    from nubovca import capi
    buf, lay = K.frame(fmt, layout)
    L = _layout(lay)
    for name, shapes in K.DRAW.items():
        t, ptr = _on_device(buf)
        ctx.draw_shapes_yuv420(capi.make_planar_frame(ptr, K.W, K.H, L, capi.MEM_DEVICE), L, shapes)
        got = _back(t)
        exp = K.draw_expected(name, fmt, layout)
        assert np.array_equal(got, exp), (name, np.flatnonzero(got != exp)[:8].tolist())
        host = np.array(buf)
        capi.draw_shapes_yuv420_host(capi.make_planar_frame(host, K.W, K.H, L), L, shapes)
        assert np.array_equal(got, host), name


@pytest.mark.parametrize("layout", list(K.LAYOUTS))
@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
def test_device_overlay_against_the_statement_and_the_host_loops(ctx, fmt, layout):
    from nubovca import capi
    buf, lay = K.frame(fmt, layout)
    L = _layout(lay)
    for name, (boxes, image, ox, oy, wp, hp) in K.OVERLAY.items():
        t, ptr = _on_device(buf)
        capi.overlay_blend_yuv420(ctx, capi.make_planar_frame(ptr, K.W, K.H, L, capi.MEM_DEVICE), L, boxes, image, ox, oy, wp, hp)
        got = _back(t)
        exp = K.overlay_expected(name, fmt, layout)
        assert np.array_equal(got, exp), (name, np.flatnonzero(got != exp)[:8].tolist())
        host = np.array(buf)
        capi.overlay_blend_yuv420(None, capi.make_planar_frame(host, K.W, K.H, L), L, boxes, image, ox, oy, wp, hp)
        assert np.array_equal(got, host), name


@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
def test_1024_shapes_in_one_call(ctx, fmt):
    from nubovca import capi
    buf, lay = K.frame(fmt, "padded")
    L = _layout(lay)
    shapes = draw_reference._shapes(np.random.default_rng(31), K.W, K.H, 1024)
    t, ptr = _on_device(buf)
    ctx.draw_shapes_yuv420(capi.make_planar_frame(ptr, K.W, K.H, L, capi.MEM_DEVICE), L, shapes)
    got = _back(t)
    exp = S.draw(buf, K.W, K.H, lay, shapes)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8].tolist()


@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
def test_shapes_whose_bounding_box_is_the_whole_1080p_frame(ctx, fmt):
    from nubovca import capi
    W, H = 1920, 1080
    buf, lay = K.random_frame(W, H, fmt, 41, tail=9, luma_rows=1088)
    L = _layout(lay)
    shapes = [(0, 1, 1, 40, 30, K.FACE), (0, 1870, 1040, 48, 38, (0, 0, 255, 0)), (1, 960, 540, 300, 0, (0, 255, 0, 0)), (0, -10, 500, 1940, 81, (9, 200, 77, 0))]
    t, ptr = _on_device(buf)
    ctx.draw_shapes_yuv420(capi.make_planar_frame(ptr, W, H, L, capi.MEM_DEVICE), L, shapes)
    got = _back(t)
    exp = S.draw(buf, W, H, lay, shapes)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8].tolist()


# ---------------------------------------------------------------- 3. a viewed 4:2:0 face stream
@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
def test_face_stream_draws_its_boxes_on_the_frame_it_analysed(ctx, fmt):
    """decoder -> detect -> draw on one device buffer: the boxes are the oracle's on every frame (a fresh buffer a frame: what was drawn on the
    previous one plays no part), and the buffer after the call is the statement's"""
    import prefix_cascades as P
    from nubovca import capi
    n, W, H = 5, *Y.SETS["sd"][:2]
    exp = Y.sequence_expected("synthetic", "sd", 9)[:n]
    casc = ctx.load_cascade_xml(P.cascade_xml("synthetic", 0))
    _, lay = Y.frame("sd", 0, fmt)
    L = _layout(lay)
    s = capi.FaceStream(ctx, casc, width_to_process=Y.SETS["sd"][2])
    s.set_input(L)
    drawn = 0
    for i in range(n):
        buf, _ = Y.frame("sd", i, fmt)
        t, ptr = _on_device(np.array(buf))
        fr = capi.make_planar_frame(ptr, W, H, L, capi.MEM_DEVICE)
        boxes, ids = ctx.face_batch_process([s], [fr])[0]
        assert np.array_equal(boxes, exp[i][0]) and np.array_equal(ids, exp[i][1]), (i, boxes.tolist(), exp[i][0].tolist())
        shapes = [(0, int(x), int(y), int(w), int(h), K.FACE) for (x, y, w, h) in boxes]
        ctx.draw_shapes_yuv420(fr, L, shapes)
        got = _back(t)
        want = S.draw(buf, W, H, lay, shapes)
        assert np.array_equal(got, want), (i, np.flatnonzero(got != want)[:8].tolist())
        drawn += len(shapes)
    assert drawn >= 2
    s.close()
    casc.free()
