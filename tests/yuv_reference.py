"""Numpy statement of the 4:2:0 conversion the library performs on NV12 / I420 frames: OpenCV 2.4 color.cpp,
cv::cvtColor(CV_YUV2BGR_NV12 / CV_YUV2BGR_I420), BT.601 limited range, shift 20, all int32, the shift arithmetic.  Pixel (x, y)
takes the chroma sample (x >> 1, y >> 1); nothing is interpolated.  Pinned by hand-derived answers only (unpinned against a
built OpenCV, like the rest of the checker).

The checker of a 4:2:0 stream is the existing oracle fed bgr(frame).

A layout is (format, offsets, strides) as nubovca.synth.make_yuv420 returns it: format 1 = NV12, 2 = I420."""
import numpy as np

NV12, I420 = 1, 2
CY, CUB, CUG, CVG, CVR = 1220542, 2116026, -409993, -852492, 1673527
SHIFT = 20


def planes(buf, w, h, layout):
    """(Y [h, w], U [h/2, w/2], V [h/2, w/2]) of the buffer, as uint8 arrays"""
    fmt, off, st = layout
    assert w % 2 == 0 and h % 2 == 0
    buf = np.asarray(buf, np.uint8).reshape(-1)

    def plane(o, stride, rows, cols):
        idx = o + np.arange(rows)[:, None] * stride + np.arange(cols)[None, :]
        return buf[idx]
    y = plane(off[0], st[0], h, w)
    if fmt == NV12:
        uv = plane(off[1], st[1], h // 2, w)
        return y, uv[:, 0::2], uv[:, 1::2]
    assert fmt == I420
    return y, plane(off[1], st[1], h // 2, w // 2), plane(off[2], st[2], h // 2, w // 2)


def convert(y, u, v):
    """BGR [h, w, 3] uint8 of the planes"""
    i32 = np.int32
    yy = np.maximum(y.astype(i32) - 16, 0) * i32(CY) + i32(1 << (SHIFT - 1))
    uu = np.repeat(np.repeat(u.astype(i32) - 128, 2, axis=0), 2, axis=1)
    vv = np.repeat(np.repeat(v.astype(i32) - 128, 2, axis=0), 2, axis=1)
    r = (yy + i32(CVR) * vv) >> SHIFT
    g = (yy + i32(CVG) * vv + i32(CUG) * uu) >> SHIFT
    b = (yy + i32(CUB) * uu) >> SHIFT
    assert r.dtype == g.dtype == b.dtype == np.int32
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def bgr(buf, w, h, layout):
    return convert(*planes(buf, w, h, layout))


def bgr_scalar(buf, w, h, layout):
    """the same, one pixel at a time in Python integers, straight from the buffer's bytes"""
    fmt, off, st = layout
    buf = [int(b) for b in np.asarray(buf, np.uint8).reshape(-1)]
    out = np.zeros((h, w, 3), np.uint8)

    def sat8(x):
        return 0 if x < 0 else 255 if x > 255 else x
    for y in range(h):
        for x in range(w):
            Y = buf[off[0] + y * st[0] + x]
            if fmt == NV12:
                c = off[1] + (y >> 1) * st[1] + 2 * (x >> 1)
                U, V = buf[c], buf[c + 1]
            else:
                U = buf[off[1] + (y >> 1) * st[1] + (x >> 1)]
                V = buf[off[2] + (y >> 1) * st[2] + (x >> 1)]
            u, v, yp = U - 128, V - 128, max(0, Y - 16) * CY
            out[y, x, 2] = sat8((yp + (1 << 19) + CVR * v) >> 20)            # Python's >> on a negative int is arithmetic
            out[y, x, 1] = sat8((yp + (1 << 19) + CVG * v + CUG * u) >> 20)
            out[y, x, 0] = sat8((yp + (1 << 19) + CUB * u) >> 20)
    return out
