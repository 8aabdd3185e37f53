"""Numpy statement of the way out in 4:2:0: cv::cvtColor(CV_BGR2YUV_I420) as OpenCV 2.4 color.cpp computes it
(RGB888toYUV420pInvoker) -- BT.601 limited range, shift 20; Y of every pixel, the chroma sample of a 2 x 2 block from the block's
top-left pixel alone -- and of the two drawing calls on a 4:2:0 frame.  Stated from memory of OpenCV 2.4 and pinned by hand-derived
answers only (no OpenCV build is at hand), like tests/yuv_reference.py.

draw() and overlay() are written the long way round, on purpose: the frame is converted to BGR (yuv_reference), drawn on by the BGR
references (draw_reference / overlay_reference), converted forward again, and of that result only the samples whose defining pixel
was drawn are copied into the buffer.  The library never builds a BGR frame; this is a second derivation of what it writes, not a
copy of its shortcut.

A layout is (format, offsets, strides) as nubovca.synth.make_yuv420 returns it: format 1 = NV12, 2 = I420."""
import numpy as np

import draw_reference
import overlay_reference
import yuv_reference as R

NV12, I420 = R.NV12, R.I420
SHIFT = 20
# (B, G, R) -> (Y, U, V), the issue's known answers (the last one: the face outline colour of FACE/BaseFace.cpp:76-80)
KNOWN = [((0, 0, 0), (16, 128, 128)), ((255, 255, 255), (235, 128, 128)), ((255, 0, 0), (41, 240, 110)), ((0, 255, 0), (145, 54, 34)),
         ((0, 0, 255), (82, 90, 240)), ((128, 128, 128), (126, 128, 128)), ((255, 128, 0), (106, 203, 63))]


def forward_all(bgr):
    """(Y, U, V) of every pixel of a [..., 3] BGR array, as int64"""
    a = np.asarray(bgr).astype(np.int64)
    b, g, r = a[..., 0], a[..., 1], a[..., 2]
    half = 1 << (SHIFT - 1)
    y = (269484 * r + 528482 * g + 102760 * b + half + (16 << SHIFT)) >> SHIFT
    u = (-155188 * r - 305135 * g + 460324 * b + half + (128 << SHIFT)) >> SHIFT
    v = (460324 * r - 385875 * g - 74448 * b + half + (128 << SHIFT)) >> SHIFT
    return y, u, v


def forward(bgr):
    """(Y [h, w], U [h/2, w/2], V [h/2, w/2]) uint8 of a BGR (or BGRA: alpha ignored) image of even size"""
    bgr = np.asarray(bgr, np.uint8)
    h, w = bgr.shape[:2]
    assert w % 2 == 0 and h % 2 == 0
    y, u, v = forward_all(bgr[:, :, :3])
    assert y.min() >= 16 and y.max() <= 235 and min(u.min(), v.min()) >= 16 and max(u.max(), v.max()) <= 240
    return y.astype(np.uint8), u[0::2, 0::2].astype(np.uint8), v[0::2, 0::2].astype(np.uint8)


def extent(w, h, layout):
    """bytes from the buffer's base to the end of its last plane's last row"""
    fmt, off, st = layout
    rows = [h, h // 2, h // 2]
    cols = [w, w if fmt == NV12 else w // 2, w // 2]
    return max(off[p] + st[p] * (rows[p] - 1) + cols[p] for p in range(2 if fmt == NV12 else 3))


def _index(o, stride, rows, cols, step=1):
    return o + np.arange(rows)[:, None] * stride + step * np.arange(cols)[None, :]


def write(buf, w, h, layout, y, u, v, ymask=None, cmask=None):
    """the samples (where the masks say so; None: all) into the planes of a flat uint8 buffer, in place"""
    fmt, off, st = layout
    iy = _index(off[0], st[0], h, w)
    if fmt == NV12:
        iu = _index(off[1], st[1], h // 2, w // 2, 2)
        iv = iu + 1
    else:
        iu, iv = _index(off[1], st[1], h // 2, w // 2), _index(off[2], st[2], h // 2, w // 2)
    ymask = np.ones((h, w), bool) if ymask is None else ymask
    cmask = np.ones((h // 2, w // 2), bool) if cmask is None else cmask
    buf[iy[ymask]] = y[ymask]
    buf[iu[cmask]] = u[cmask]
    buf[iv[cmask]] = v[cmask]
    return buf


def convert(bgr, buf, w, h, layout):
    """nvca_bgr_to_yuv420: a copy of `buf` with the planes of the converted image in it"""
    out = np.array(buf, np.uint8)
    return write(out, w, h, layout, *forward(bgr))


def _covered(w, h, shapes):
    """which pixels the shapes cover: draw_reference on a one-channel image of zeros, every colour 1"""
    m = draw_reference._ref(np.zeros((h, w, 1), np.uint8), [(k, x, y, sw, sh, (1,)) for (k, x, y, sw, sh, _) in shapes])
    return m[:, :, 0] == 1


def draw(buf, w, h, layout, shapes):
    """nvca_draw_shapes_yuv420: a copy of `buf` with the shapes drawn"""
    out = np.array(buf, np.uint8)
    if not shapes:
        return out
    F = R.bgr(out, w, h, layout)
    F2 = draw_reference._ref(F.copy(), shapes)
    m = _covered(w, h, shapes)
    y, u, v = forward(F2)
    return write(out, w, h, layout, y, u, v, m, m[0::2, 0::2])


def _touched(w, h, box, image, off_x, off_y, wp, hp):
    """the pixels one box touches: inside the placed image and the frame, the scaled alpha (4 channels) not 0"""
    bx, by, bw, bh = [int(t) for t in box]
    x, y = int(float(bx) + float(bw) * off_x), int(float(by) + float(bh) * off_y)
    ph, pw = int(float(bh) * hp), int(float(bw) * wp)
    m = np.zeros((h, w), bool)
    if pw <= 0 or ph <= 0:
        return m
    inside = np.ones((ph, pw), bool)
    if image.ndim == 3 and image.shape[2] == 4:
        inside = overlay_reference.resize_linear_cn(image, pw, ph)[:, :, 3] != 0
    yy, xx = np.mgrid[0:ph, 0:pw]
    yy, xx = yy + y, xx + x
    ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w) & inside
    m[yy[ok], xx[ok]] = True
    return m


def overlay(buf, w, h, layout, boxes, image, off_x=0.0, off_y=0.0, wp=1.0, hp=1.0):
    """nvca_overlay_blend_yuv420: a copy of `buf` with the image laid over every box, one box at a time"""
    out = np.array(buf, np.uint8)
    image = np.asarray(image, np.uint8)
    if wp == 0 or hp == 0:
        return out
    for box in np.asarray(boxes, np.int64).reshape(-1, 4):
        F = R.bgr(out, w, h, layout)
        F2 = overlay_reference.overlay_blend(F.copy(), [box], image, off_x, off_y, wp, hp)
        m = _touched(w, h, box, image, off_x, off_y, wp, hp)
        assert np.array_equal(F2[~m], F[~m])          # what the BGR reference changed is touched
        y, u, v = forward(F2)
        write(out, w, h, layout, y, u, v, m, m[0::2, 0::2])
    return out


def fnv1a(buf):
    """64-bit FNV-1a of a byte buffer (the checksum tests/san/yuv_out_driver.cpp prints)"""
    hsh = 0xcbf29ce484222325
    for b in np.asarray(buf, np.uint8).tobytes():
        hsh = ((hsh ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return hsh
