"""Packed frames (gray, BGR, BGRA) in buffers that are not what torch or numpy hand out by default: padded and odd strides, bases that are
not 16-byte aligned, widths that are no multiple of 4 -- the images of tests/test_gpu_frame_layouts.py, the case lists it runs and the
two dispatch predicates those lists are meant to cross (tests/test_frame_layouts_cpu.py checks the lists against the predicates).  Pure
numpy: nothing here needs a device.

An image in a buffer: `MARGIN` guard bytes, `base_off` more, then the rows `stride` bytes apart, the LAST row only width * cn bytes long
(include/nubovca.h: a buffer need not extend past the last pixel), then `MARGIN` guard bytes.  Every byte that is not a pixel comes from a
seeded random stream, so a kernel that folds padding into a histogram, a sum or a resize tap changes its result, and a store that spills
between rows or past the image changes a byte outside_unchanged() looks at."""
import numpy as np

MARGIN = 128                    # guard bytes in front and behind: a multiple of 16 (the alignment of a device base is base_off's), more than
                                # any base offset and more than the 16 bytes a wrongly chosen wide kernel reads or writes past a row
HOST, DEVICE = 0, 1             # capi.MEM_HOST / MEM_DEVICE
ALLOC_ALIGN = 256               # what the GPU test asserts of every data_ptr() it hands over


def _up(v, a):
    return (v + a - 1) // a * a


# ---------------------------------------------------------------- the builder
def extent(h, w, cn, stride):
    """bytes from the first pixel to the end of the last pixel"""
    return stride * (h - 1) + w * cn


def pixel_index(h, w, cn, stride, base_off=0):
    """[h, w * cn] positions of the pixel bytes in the flat buffer"""
    return (MARGIN + base_off + np.arange(h)[:, None] * stride + np.arange(w * cn)[None, :]).astype(np.int64)


def build(px, stride, base_off=0, seed=0, fill=None):
    """flat uint8 buffer holding the image px ([h, w] or [h, w, cn]) at MARGIN + base_off + y * stride + x * cn; every other byte from a
    seeded random stream (fill: that constant, or the stream held to [lo, hi], instead -- only for the histogram tests that want padding
    brighter or darker than every pixel)"""
    px = np.asarray(px, np.uint8)
    h, w = px.shape[:2]
    cn = 1 if px.ndim == 2 else px.shape[2]
    assert stride >= w * cn and 0 <= base_off < MARGIN
    n = 2 * MARGIN + base_off + extent(h, w, cn, stride)
    lo, hi = fill if isinstance(fill, tuple) else (0, 255)
    if fill is None or isinstance(fill, tuple):
        buf = np.random.default_rng([seed, h, w, cn, stride, base_off]).integers(lo, hi + 1, n, dtype=np.uint8)
    else:
        buf = np.full(n, fill, np.uint8)
    buf[pixel_index(h, w, cn, stride, base_off)] = px.reshape(h, w * cn)
    return buf


def start(base_off=0):
    """offset of the first pixel in the buffer: what is added to the buffer's address"""
    return MARGIN + base_off


def pixels(buf, h, w, cn, stride, base_off=0):
    """the image back as a contiguous copy ([h, w] for cn == 1)"""
    out = np.asarray(buf, np.uint8)[pixel_index(h, w, cn, stride, base_off)]
    return np.ascontiguousarray(out if cn == 1 else out.reshape(h, w, cn))


def outside_unchanged(before, after, h, w, cn, stride, base_off=0):
    """every byte that is not a pixel of the image -- margins, row padding -- is the same in both buffers"""
    before, after = np.asarray(before, np.uint8), np.asarray(after, np.uint8)
    if before.shape != after.shape:
        return False
    keep = np.ones(before.shape, bool)
    keep[pixel_index(h, w, cn, stride, base_off)] = False
    return bool(np.array_equal(before[keep], after[keep]))


# ---------------------------------------------------------------- strides, offsets, memory kinds
STRIDE_KINDS = ("tight", "align4", "align16", "plus")


def stride_of(kind, w, cn):
    """tight; align4(tight); align16(tight), or 16 more where that is align4(tight) already; tight + 1 (odd rows apart for gray and BGR at
    even widths, never a multiple of 4 where tight is one) -- tight + 4 for BGRA, whose rows stay on pixel boundaries"""
    t = w * cn
    if kind == "tight":
        return t
    if kind == "align4":
        return _up(t, 4)
    if kind == "align16":
        return _up(t, 16) if _up(t, 16) != _up(t, 4) else _up(t, 16) + 16
    if kind == "plus":
        return t + (4 if cn == 4 else 1)
    raise KeyError(kind)


def base_offsets(cn):
    return (0, 4, 8, 16) if cn == 4 else (0, 1, 4, 8, 16)


MEMS = (HOST, DEVICE)


# ---------------------------------------------------------------- the two dispatch predicates, as the C++ has them
def aligned4(stride, mem, base):
    """frames_aligned4 (csrc/host_copy.cpp) for ONE frame: k_gray_fast4 takes a batch only if this holds for every frame of it"""
    return not (stride & 3) and not (mem == DEVICE and (base & 15))


def trk_wide(mem, base, stride, width):
    """trk_wide_ok (csrc/trk_host.cpp) for packed BGRA, ONE member of a launch set: k_trk_pixel4 takes the set only if every member holds"""
    if width % 4:
        return False
    if mem != DEVICE:
        base = 0
    return not (stride & 15) and not (base & 15)


def device_base(base_off):
    """the low bits of a device pointer data_ptr() + start(base_off), data_ptr() being ALLOC_ALIGN-aligned"""
    return (MARGIN + base_off) % ALLOC_ALIGN


# ---------------------------------------------------------------- shapes
WIDTHS = (1, 3, 4, 5, 7, 255, 256, 257)          # around 4 pixels a thread and the 256 columns of a block
WIDE_WIDTHS = (1021, 1024, 1027)                 # around the 1024 columns of a k_gray_fast4 block: bgr2gray only
HEIGHTS = (1, 7, 8, 9, 17)                       # around kGrayRows == 8; 17: three blocks of rows


def draw(seed, n, **columns):
    """n cases as dicts: every column's values in turn, each column in a seeded order of its own -- with n at least the longest column
    every value of every column appears; which values meet is the seed's choice (test_frame_layouts_cpu.py checks what must meet)"""
    rng = np.random.default_rng(seed)
    cols = {}
    for name, values in columns.items():
        values = list(values)
        reps = [values[i] for _ in range(-(-n // len(values))) for i in rng.permutation(len(values))]
        cols[name] = reps[:n]
    return [{k: cols[k][i] for k in cols} for i in range(n)]


def _gray_cases(cn, seed):
    """bgr2gray: source stride / base / memory against the destination's stride, both drawn independently"""
    c = draw(seed, 27, w=WIDTHS + WIDE_WIDTHS, h=HEIGHTS, sk=STRIDE_KINDS, off=base_offsets(cn), mem=MEMS, dk=("tight", "align16", "plus"),
             doff=base_offsets(1))
    # what a draw may miss is stated, not hoped for: the k_gray_fast4 tail (3-channel rows padded to 4 bytes at a width that is no
    # multiple of 4, aligned base) in both memories, at one pixel, at the end of a block and one pixel into the next
    if cn == 3:
        c += [dict(w=w, h=h, sk="align4", off=off, mem=mem, dk=dk, doff=0)
              for (w, h, off, mem, dk) in ((1, 1, 0, HOST, "tight"), (5, 9, 16, DEVICE, "plus"), (255, 8, 0, DEVICE, "tight"), (257, 7, 1, HOST, "align16"),
                                          (1021, 9, 0, DEVICE, "align16"), (1027, 1, 16, DEVICE, "tight"))]
    for k in c:
        k["cn"] = cn
        k["stride"], k["dstride"] = stride_of(k["sk"], k["w"], cn), stride_of(k["dk"], k["w"], 1)
    return c


GRAY_CASES = {3: _gray_cases(3, 301), 4: _gray_cases(4, 401)}


def _plane_cases(seed, modes):
    """one-channel primitives: mode "host", "device" (out of place) or "inplace" (device, dst == src: one stride, one offset)"""
    c = draw(seed, 25, w=WIDTHS, h=HEIGHTS, sk=STRIDE_KINDS, off=base_offsets(1), mode=modes, dk=STRIDE_KINDS, doff=base_offsets(1))
    for k in c:
        if k["mode"] == "inplace":
            k["dk"], k["doff"] = k["sk"], k["off"]
        k["stride"], k["dstride"] = stride_of(k["sk"], k["w"], 1), stride_of(k["dk"], k["w"], 1)
        k["mem"] = HOST if k["mode"] == "host" else DEVICE
    return c


EQUALIZE_CASES = _plane_cases(501, ("host", "device", "inplace"))
FLIP_CASES = _plane_cases(601, ("host", "device", "inplace"))

RESIZE_GEOMETRIES = ((97, 61, 41, 29), (33, 2, 7, 1), (50, 40, 120, 90), (257, 9, 256, 8))


def _resize_cases():
    c = draw(701, 24, geo=RESIZE_GEOMETRIES, cn=(1, 3), mem=MEMS, sk=STRIDE_KINDS, off=base_offsets(1), dk=STRIDE_KINDS, doff=base_offsets(1))
    have = {(k["geo"], k["cn"], k["mem"]) for k in c}
    # every geometry in every channel count and memory: the combinations the draw did not bring
    extra = [(g, cn, mem) for g in RESIZE_GEOMETRIES for cn in (1, 3) for mem in MEMS if (g, cn, mem) not in have]
    for i, (g, cn, mem) in enumerate(extra):
        c.append(dict(geo=g, cn=cn, mem=mem, sk=STRIDE_KINDS[(i + 1) % 4], off=base_offsets(1)[i % 5], dk=STRIDE_KINDS[(i + 2) % 4], doff=base_offsets(1)[(i + 3) % 5]))
    for k in c:
        sw, sh, dw, dh = k["geo"]
        k["stride"], k["dstride"] = stride_of(k["sk"], sw, k["cn"]), stride_of(k["dk"], dw, k["cn"])
    return c


RESIZE_CASES = _resize_cases()

# nvca_integral / nvca_integral_tilted: host sources (the API refuses device memory); (w, h, stride kind, base offset)
INTEGRAL_CASES = [(65, 17, "plus", 1), (65, 9, "align16", 0), (257, 8, "plus", 4), (257, 7, "align4", 8), (2049, 3, "plus", 16), (2049, 3, "align16", 1),
                  (65, 1, "tight", 1)]

# ---------------------------------------------------------------- streams: 322 x 242 BGR, (memory, stride, base offset) per stream of the batch
STREAM_W, STREAM_H = 322, 242
STREAM_MIXED = [(HOST, 968, 0), (DEVICE, 966, 0), (DEVICE, 976, 0), (DEVICE, 976, 4)]
STREAM_HOST_PADDED = [(HOST, 968, 0)] * 4          # width-to-process 322: identity geometry, every frame aligned: the k_gray_fast4 tail


# a third geometry for the sparse ingest of a shrinking stream (copy_row_runs, csrc/host_copy.cpp): neither 322 -> 322 nor 322 -> 160 (a shrink by
# 2 reads every row) takes it; 322 x 240 at width-to-process 80 is a shrink by 4 whose resize reads rows 4 k + 1 and 4 k + 2 only
SPARSE_H, SPARSE_W2P = 240, 80


def working_size(W, H, w2p):
    """kms_face_detect_conf_images / process_frame: the integer ratio, then cvRound of each side"""
    scale = float(W // w2p)
    return int(np.rint(W / scale)), int(np.rint(H / scale))


def row_runs(sh, dh):
    """make_rowcopy (csrc/plans.cpp) for the bilinear resize of sh rows to dh: the source rows it reads as (first, period, run, count) where
    they are at most half of all rows and come in equal runs at equal distances, else None (the whole frame is copied)"""
    scale = 1.0 / (dh / sh)
    rows = set()
    for dy in range(dh):
        sy = int(np.floor(np.float32((dy + 0.5) * scale - 0.5)))
        rows.update(min(max(r, 0), sh - 1) for r in (sy, sy + 1))
    rows = sorted(rows)
    if len(rows) * 2 > sh:
        return None
    runs = []
    for r in rows:
        if runs and runs[-1][0] + runs[-1][1] == r:
            runs[-1][1] += 1
        else:
            runs.append([r, 1])
    period = runs[1][0] - runs[0][0] if len(runs) > 1 else sh
    if any(n != runs[0][1] or a != runs[0][0] + i * period for i, (a, n) in enumerate(runs)):
        return None
    return runs[0][0], period, runs[0][1], len(runs)


def face_launch_sets(layouts):
    """the frames of one face batch that share a launch of the gray kernel (face_submit, csrc/face_stream.cpp, groups equal sizes by
    stride) and whether frames_aligned4 holds for the set: [(members, aligned)]"""
    sets = []
    for stride in dict.fromkeys(s for _, s, _ in layouts):
        members = [i for i, (_, s, _) in enumerate(layouts) if s == stride]
        sets.append((members, all(aligned4(layouts[i][1], layouts[i][0], device_base(layouts[i][2])) for i in members)))
    return sets


# ---------------------------------------------------------------- tracker: packed BGRA, (name, w, h, stride, base offset)
TRACKER_H = 48
TRACKER_CASES = [("wide", 320, TRACKER_H, 1280, 0), ("wide-padded", 320, TRACKER_H, 1296, 0), ("narrow-stride", 320, TRACKER_H, 1284, 0),
                 ("narrow-base", 320, TRACKER_H, 1280, 4), ("narrow-width", 322, TRACKER_H, 1288, 0),
                 ("narrow-width-alone", 322, TRACKER_H, 1296, 0)]          # (322 * 4 is no multiple of 16: a stride of 1296 leaves the width as the one failing term)
# one call, one launch set (equal sizes): a frame that could go wide beside one at an offset base
TRACKER_MIXED = [("wide", 320, TRACKER_H, 1280, 0), ("narrow-base", 320, TRACKER_H, 1280, 4), ("wide-padded", 320, TRACKER_H, 1296, 0)]

# ---------------------------------------------------------------- drawing: a 61 x 50 frame, (channels, stride kind, base offset)
DRAW_W, DRAW_H = 61, 50


def draw_stride(kind, cn):
    return DRAW_W * cn + 7 if kind == "plus7" else stride_of(kind, DRAW_W, cn)


DRAW_CASES = [(cn, sk, off) for cn in (3, 4) for sk in ("tight", "align4", "plus7") for off in ((0, 1) if cn == 3 else (0, 4))]
# rectangles and rings that touch the left, top, right and bottom border (and reach past them), then one well inside
DRAW_SHAPES = [(0, 0, 0, DRAW_W - 1, DRAW_H - 1, (11, 22, 33, 44)), (0, -5, 20, 30, 100, (200, 100, 50, 25)), (0, 40, -3, 40, 20, (1, 2, 3, 4)),
               (1, 0, 25, 6, 0, (90, 80, 70, 60)), (1, DRAW_W - 1, DRAW_H - 1, 9, 0, (5, 6, 7, 8)), (1, 30, 0, 3, 0, (250, 251, 252, 253)),
               (0, 20, 15, 10, 12, (128, 64, 32, 16))]
OVERLAY_CASES = [(3, sk, off) for sk in ("tight", "align4", "plus7") for off in (0, 1)]
OVERLAY_BOX = (40, 30, 40, 36)          # reaches 19 columns past the right edge and 16 rows past the bottom one

# ---------------------------------------------------------------- detection on a view: (memory, parent stride, base offset)
VIEW_PARENT_W, VIEW_PARENT_H = 320, 240
VIEW = (71, 41, 160, 150)               # x0, y0 (both odd), width, height of the sub-matrix
VIEW_ALIGNED = (72, 40, 160, 150)       # the same at a 4-byte aligned column: a device view the integral kernels read where it is
VIEW_SMALL = (71, 41, 120, 110)         # (w + 1) * (h + 2) <= ROI_MAX_WORDS: the one-launch small-image detector takes it
ROI_MAX_WORDS = 14848                   # kRoiMaxWords, csrc/roi_batch.cpp
VIEW_CASES = [(DEVICE, 320, 0), (HOST, 336, 0)]
