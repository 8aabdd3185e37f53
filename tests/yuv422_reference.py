"""Numpy statement of the conversion the library performs on packed 4:2:2 frames: OpenCV 2.4 color.cpp,
cv::cvtColor(CV_YUV2BGR_YUY2 / CV_YUV2BGR_UYVY / CV_YUV2BGR_YVYU).  In row y, pixels 2k and 2k + 1 take U and V from the four bytes
4k .. 4k + 3 of that row; nothing is shared between rows and nothing is interpolated.  Everything else is A.13's (tests/yuv_reference.py):
BT.601 limited range, shift 20, all int32, the shift arithmetic.  Pinned by hand-derived answers only (unpinned against a built OpenCV,
like A.13).

The checker of a 4:2:2 stream is the existing oracle fed bgr(frame).

A layout is (format, offsets, strides) as nubovca.synth.make_yuv422 returns it: format 4 = YUY2 (bytes Y0 U Y1 V), 5 = UYVY (U Y0 V Y1),
6 = YVYU (Y0 V Y1 U); only offsets[0] and strides[0] are read."""
import numpy as np

import yuv_reference as R420

YUY2, UYVY, YVYU = 4, 5, 6
FMTS = [YUY2, UYVY, YVYU]
FMT_IDS = ["yuy2", "uyvy", "yvyu"]
# positions of (Y0, U, V) within a pixel pair's four bytes; Y1 lies two bytes behind Y0
POS = {YUY2: (0, 1, 3), UYVY: (1, 0, 2), YVYU: (0, 3, 1)}
CY, CUB, CUG, CVG, CVR, SHIFT = R420.CY, R420.CUB, R420.CUG, R420.CVG, R420.CVR, R420.SHIFT


def planes(buf, w, h, layout):
    """(Y [h, w], U [h, w/2], V [h, w/2]) of the buffer, as uint8 arrays: a chroma sample per ROW and pixel pair"""
    fmt, off, st = layout
    assert w % 2 == 0 and w > 0 and h > 0 and st[0] >= 2 * w
    py, pu, pv = POS[fmt]
    buf = np.asarray(buf, np.uint8).reshape(-1)
    idx = off[0] + np.arange(h)[:, None] * st[0] + np.arange(2 * w)[None, :]
    rows = buf[idx].reshape(h, w // 2, 4)
    y = np.empty((h, w), np.uint8)
    y[:, 0::2], y[:, 1::2] = rows[..., py], rows[..., py + 2]
    return y, rows[..., pu], rows[..., pv]


def convert(y, u, v, vertical=1):
    """BGR [h, w, 3] uint8 of the planes; vertical: rows a chroma row serves (1: A.18; the 4:2:0 statement's 2 is R420.convert)"""
    i32 = np.int32
    yy = np.maximum(y.astype(i32) - 16, 0) * i32(CY) + i32(1 << (SHIFT - 1))
    uu = np.repeat(np.repeat(u.astype(i32) - 128, vertical, axis=0), 2, axis=1)
    vv = np.repeat(np.repeat(v.astype(i32) - 128, vertical, axis=0), 2, axis=1)
    r = (yy + i32(CVR) * vv) >> SHIFT
    g = (yy + i32(CVG) * vv + i32(CUG) * uu) >> SHIFT
    b = (yy + i32(CUB) * uu) >> SHIFT
    assert r.dtype == g.dtype == b.dtype == np.int32
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def bgr(buf, w, h, layout):
    return convert(*planes(buf, w, h, layout))


def bgr_shared_rows(buf, w, h, layout):
    """what a 4:2:0-style reader makes of the frame: row y with the chroma of row y & ~1 (NOT the statement: the image a kernel that
    shares chroma vertically would compute)"""
    y, u, v = planes(buf, w, h, layout)
    rows = np.arange(h) & ~1
    return convert(y, u[rows], v[rows])


def bgr_scalar(buf, w, h, layout):
    """the statement, one pixel at a time in Python integers, straight from the buffer's bytes"""
    fmt, off, st = layout
    py, pu, pv = POS[fmt]
    buf = [int(b) for b in np.asarray(buf, np.uint8).reshape(-1)]
    out = np.zeros((h, w, 3), np.uint8)

    def sat8(x):
        return 0 if x < 0 else 255 if x > 255 else x
    for y in range(h):
        for x in range(w):
            pair = off[0] + y * st[0] + 4 * (x >> 1)
            Y, U, V = buf[pair + py + 2 * (x & 1)], buf[pair + pu], buf[pair + pv]
            u, v, yp = U - 128, V - 128, max(0, Y - 16) * CY
            out[y, x, 2] = sat8((yp + (1 << 19) + CVR * v) >> 20)            # Python's >> on a negative int is arithmetic
            out[y, x, 1] = sat8((yp + (1 << 19) + CVG * v + CUG * u) >> 20)
            out[y, x, 0] = sat8((yp + (1 << 19) + CUB * u) >> 20)
    return out


def gray(img):
    """cv::cvtColor(CV_BGR2GRAY) of a BGR image (RGB2Gray<uchar>: 1868 / 9617 / 4899, shift 14), for the premises"""
    i = img.astype(np.int32)
    return ((i[..., 0] * 1868 + i[..., 1] * 9617 + i[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def extent(w, h, layout):
    """bytes from the base to the last row's last pixel"""
    return layout[1][0] + layout[2][0] * (h - 1) + 2 * w


def from_420(buf, w, h, layout420, fmt, pad=0, base=0, seed=0):
    """a 4:2:0 frame (tests/yuv_reference.py layout) re-packed as 4:2:2 by repeating every chroma row: (buffer, layout tuple)"""
    from nubovca import synth
    y, u, v = R420.planes(buf, w, h, layout420)
    out, lay = synth.pack_yuv422(y, np.repeat(u, 2, axis=0), np.repeat(v, 2, axis=0), fmt, pad=pad, base=base, seed=seed)
    return out, (lay[0], tuple(lay[1]), tuple(lay[2]))
