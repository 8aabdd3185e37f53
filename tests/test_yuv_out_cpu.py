"""The way out in 4:2:0 on the CPU: the forward rule by its known answers, ranges and round trip, and the host loops
of nvca_draw_shapes_yuv420 / nvca_overlay_blend_yuv420 (no context, no device) against the numpy statement
(tests/yuv_out_reference.py) on the case table of tests/yuv_out_cases.py.  Every comparison is np.array_equal but the round trip, whose
bound is derived, not tuned.  nvca_bgr_to_yuv420 itself needs a device (tests/test_gpu_yuv_out.py); the rule it shares with the host
loops is reached here through a drawn pixel."""
import ctypes as C

import numpy as np
import pytest

import yuv_out_cases as K
import yuv_out_reference as S
import yuv_reference as R

ERR_ARG = -1


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as ge
    ge.build()
    from nubovca import capi
    capi.load()
    return capi


def _frame(capi, buf, w, h, lay):
    return capi.make_planar_frame(buf, w, h, capi.pixel_layout(*lay)), capi.pixel_layout(*lay)


# ---------------------------------------------------------------- the rule
def test_known_answers_through_the_statement():
    for bgr, yuv in S.KNOWN:
        y, u, v = S.forward(np.full((2, 2, 3), bgr, np.uint8))
        assert (int(y[0, 0]), int(u[0, 0]), int(v[0, 0])) == yuv, (bgr, yuv)
        assert (y == yuv[0]).all()


@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
def test_known_answers_through_the_library_rule(capi, fmt):
    """a 2 x 2 frame with one ring of radius 0 .. 2 around (0, 0) of each colour: every byte of the frame becomes the colour's Y, U, V"""
    lay = K.layout_of(2, 2, fmt)
    for bgr, yuv in S.KNOWN:
        buf = np.zeros(S.extent(2, 2, lay), np.uint8)
        fr, L = _frame(capi, buf, 2, 2, lay)
        capi.draw_shapes_yuv420_host(fr, L, [(1, 0, 0, 0, 0, bgr + (9,))])
        y, u, v = R.planes(buf, 2, 2, lay)
        assert (y == yuv[0]).all() and int(u[0, 0]) == yuv[1] and int(v[0, 0]) == yuv[2], (bgr, yuv, buf.tolist())


def test_output_ranges_on_a_colour_cube():
    """every 5th level of each channel plus both ends (53^3 colours): Y in 16 .. 235, U and V in 16 .. 240 -- nothing to saturate"""
    lv = np.unique(np.concatenate([np.arange(0, 256, 5), [254, 255]]))
    cube = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), axis=-1).reshape(-1, 3)
    y, u, v = S.forward_all(cube)
    assert (y.min(), y.max()) == (16, 235) and (u.min(), u.max()) == (16, 240) and (v.min(), v.max()) == (16, 240)


def test_chroma_comes_from_the_even_even_pixel_only():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (12, 16, 3)).astype(np.uint8)
    b = a.copy()
    for dy, dx in ((0, 1), (1, 0), (1, 1)):
        b[dy::2, dx::2] = rng.integers(0, 256, (6, 8, 3))
    ya, ua, va = S.forward(a)
    yb, ub, vb = S.forward(b)
    assert np.array_equal(ua, ub) and np.array_equal(va, vb) and not np.array_equal(ya, yb)
    assert np.array_equal(ya[0::2, 0::2], yb[0::2, 0::2])


@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
def test_round_trip_on_block_constant_images(fmt):
    """A.13 of A.14 of an image whose 2 x 2 blocks are of one colour: off by at most 2 in B and R and 1 in G (the bound holds over all
    2^24 colours; here a sampled cube and random colours)"""
    rng = np.random.default_rng(11)
    lv = np.arange(0, 256, 15)
    cols = np.concatenate([np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), axis=-1).reshape(-1, 3), rng.integers(0, 256, (3086, 3))]).astype(np.uint8)
    n = len(cols)
    w, h = 2 * 100, 2 * (n // 100)
    blocks = cols[:(w // 2) * (h // 2)].reshape(h // 2, w // 2, 3)
    img = np.repeat(np.repeat(blocks, 2, axis=0), 2, axis=1)
    lay = K.layout_of(w, h, fmt)
    buf = S.convert(img, np.zeros(S.extent(w, h, lay), np.uint8), w, h, lay)
    d = np.abs(R.bgr(buf, w, h, lay).astype(int) - img.astype(int)).reshape(-1, 3).max(axis=0)
    assert d[0] <= 2 and d[1] <= 1 and d[2] <= 2, d.tolist()


# ---------------------------------------------------------------- the host loops against the statement
def _check(got, exp, buf, lay, what):
    assert np.array_equal(got, exp), (what, np.flatnonzero(got != exp)[:8].tolist())
    pad = ~K.sample_mask(len(buf), K.W, K.H, lay)
    assert pad.any() or what[2] == "tight"
    assert (got[pad] == K.SENTINEL).all(), what


@pytest.mark.parametrize("layout", list(K.LAYOUTS))
@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
@pytest.mark.parametrize("name", list(K.DRAW))
def test_host_draw_against_the_statement(capi, name, fmt, layout):
    buf, lay = K.frame(fmt, layout)
    got = np.array(buf)
    fr, L = _frame(capi, got, K.W, K.H, lay)
    capi.draw_shapes_yuv420_host(fr, L, K.DRAW[name])
    _check(got, K.draw_expected(name, fmt, layout), buf, lay, (name, fmt, layout))
    if name in ("outside", "none"):
        assert np.array_equal(got, buf)
    elif name != "negative_size":
        assert not np.array_equal(got, buf)


def test_last_shape_wins_for_luma_and_for_the_anchor(capi):
    """two rectangles over the same pixels: Y and the chroma of the covered even / even pixels are the second colour's"""
    buf, lay = K.frame(S.NV12, "tight")
    got = np.array(buf)
    fr, L = _frame(capi, got, K.W, K.H, lay)
    c1, c2 = (255, 0, 0, 0), (0, 0, 255, 0)
    capi.draw_shapes_yuv420_host(fr, L, [(0, 10, 8, 20, 16, c1), (0, 10, 8, 20, 16, c2)])
    y, u, v = R.planes(got, K.W, K.H, lay)
    assert (int(y[8, 10]), int(u[4, 5]), int(v[4, 5])) == (82, 90, 240)
    assert int(y[9, 11]) == 82 and (int(u[4, 6]), int(v[4, 6])) == (90, 240)          # pixel (12, 8) lies on the top edge


@pytest.mark.parametrize("layout", list(K.LAYOUTS))
@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
@pytest.mark.parametrize("name", list(K.OVERLAY))
def test_host_overlay_against_the_statement(capi, name, fmt, layout):
    buf, lay = K.frame(fmt, layout)
    got = np.array(buf)
    fr, L = _frame(capi, got, K.W, K.H, lay)
    boxes, image, ox, oy, wp, hp = K.OVERLAY[name]
    capi.overlay_blend_yuv420(None, fr, L, boxes, image, ox, oy, wp, hp)
    _check(got, K.overlay_expected(name, fmt, layout), buf, lay, (name, fmt, layout))
    if name in ("width_zero", "no_boxes"):
        assert np.array_equal(got, buf)
    else:
        assert not np.array_equal(got, buf)


def test_pixels_under_a_zero_alpha_keep_their_bytes(capi):
    """an image whose alpha is 0 everywhere touches nothing; with alpha 255 everywhere every pixel under it is the image's"""
    buf, lay = K.frame(S.I420, "padded")
    img = np.random.default_rng(5).integers(0, 256, (10, 12, 4)).astype(np.uint8)
    for alpha in (0, 255):
        img[:, :, 3] = alpha
        got = np.array(buf)
        fr, L = _frame(capi, got, K.W, K.H, lay)
        capi.overlay_blend_yuv420(None, fr, L, [(6, 4, 12, 10)], img)
        if alpha == 0:
            assert np.array_equal(got, buf)
        else:
            y, u, v = S.forward(img[:, :, :3])
            gy, gu, gv = R.planes(got, K.W, K.H, lay)
            assert np.array_equal(gy[4:14, 6:18], y) and np.array_equal(gu[2:7, 3:9], u) and np.array_equal(gv[2:7, 3:9], v)


# ---------------------------------------------------------------- refusals
def _raw_draw(capi, ctx, fr, L, shapes):
    lib = capi.load()
    return lib.nvca_draw_shapes_yuv420(ctx, C.byref(fr) if fr is not None else None, C.byref(L) if L is not None else None, capi._shape_array(shapes), len(shapes))


def _raw_overlay(capi, ctx, fr, L, image=None, boxes=((2, 2, 8, 8),)):
    lib = capi.load()
    image = np.zeros((4, 4, 3), np.uint8) if image is None else image
    cn = 1 if image.ndim == 2 else image.shape[2]
    ov = capi.Overlay(image.ctypes.data, image.shape[1], image.shape[0], image.strides[0], cn, 0.0, 0.0, 1.0, 1.0)
    arr = (capi.Rect * len(boxes))(*[capi.Rect(*b) for b in boxes])
    return lib.nvca_overlay_blend_yuv420(ctx, C.byref(fr) if fr is not None else None, C.byref(L) if L is not None else None, arr, len(boxes), C.byref(ov))


@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
def test_refusals(capi, fmt):
    one = [(0, 2, 2, 8, 8, K.FACE)]
    buf, lay = K.frame(fmt, "rows")
    buf = np.array(buf)

    def both(w, h, lay, stride=None, mem=0):
        L = capi.pixel_layout(*lay)
        fr = capi.make_planar_frame(buf, w, h, L)
        if stride is not None:
            fr.stride = stride
        fr.mem = mem
        return _raw_draw(capi, None, fr, L, one), _raw_overlay(capi, None, fr, L)

    assert both(K.W, K.H, lay) == (0, 0)
    buf[:] = K.frame(fmt, "rows")[0]
    f, off, st = lay
    assert both(K.W - 1, K.H, lay) == (ERR_ARG, ERR_ARG)                                    # odd width
    assert both(K.W, K.H - 1, lay) == (ERR_ARG, ERR_ARG)                                    # odd height
    assert both(K.W, K.H, lay, stride=st[0] + 1) == (ERR_ARG, ERR_ARG)                      # the frame's stride is not stride[0]
    assert both(K.W, K.H, (f, off, (K.W - 1,) + st[1:])) == (ERR_ARG, ERR_ARG)              # short luma stride
    short = K.W - 1 if fmt == S.NV12 else K.W // 2 - 1
    assert both(K.W, K.H, (f, off, (st[0], short) + st[2:])) == (ERR_ARG, ERR_ARG)          # short chroma stride
    assert both(K.W, K.H, (f, (off[0], off[0] + st[0] * (K.H - 1)) + off[2:], st)) == (ERR_ARG, ERR_ARG)   # chroma starts inside the luma plane
    if fmt == S.I420:
        assert both(K.W, K.H, (f, (off[0], off[1], off[1] + 3), st)) == (ERR_ARG, ERR_ARG)  # V inside U
    assert both(K.W, K.H, (0, off, st)) == (ERR_ARG, ERR_ARG)                               # a packed format is no 4:2:0 layout
    assert both(K.W, K.H, lay, mem=1) == (ERR_ARG, ERR_ARG)                                 # a device frame without a context
    assert both(K.W, K.H, lay, mem=7) == (ERR_ARG, ERR_ARG)
    L = capi.pixel_layout(*lay)
    fr = capi.make_planar_frame(buf, K.W, K.H, L)
    assert _raw_draw(capi, None, fr, None, one) == ERR_ARG and _raw_overlay(capi, None, fr, None) == ERR_ARG          # NULL layout
    assert _raw_draw(capi, None, None, L, one) == ERR_ARG and _raw_overlay(capi, None, None, L) == ERR_ARG            # NULL frame
    assert _raw_draw(capi, None, fr, L, [(2, 2, 2, 8, 8, K.FACE)]) == ERR_ARG                                          # unknown shape kind
    assert _raw_draw(capi, None, fr, L, [(0, 1 << 25, 2, 8, 8, K.FACE)]) == ERR_ARG                                    # coordinate bound
    assert _raw_draw(capi, None, fr, L, one * 1025) == ERR_ARG and _raw_draw(capi, None, fr, L, one * 1024) == 0       # n > 1024
    assert _raw_overlay(capi, None, fr, L, boxes=((2, 2, 8, 8),) * 1025) == ERR_ARG
    assert _raw_overlay(capi, None, fr, L, image=np.zeros((4, 4, 2), np.uint8)) == ERR_ARG                             # channels 2
    assert _raw_overlay(capi, None, fr, L, boxes=((2, 2, -8, 8),)) == ERR_ARG
    lib = capi.load()
    src = np.zeros((K.H, K.W, 3), np.uint8)
    assert lib.nvca_bgr_to_yuv420(None, src.ctypes.data, K.W, K.H, K.W * 3, 3, 0, buf.ctypes.data, C.byref(L)) == ERR_ARG   # the conversion runs on the device
    assert (buf[~K.sample_mask(len(buf), K.W, K.H, lay)] == K.SENTINEL).all()
