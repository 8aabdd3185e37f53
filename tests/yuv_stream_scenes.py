"""The 4:2:0 scenes of the part-detector and tracker tests (tests/test_yuv_streams_cpu.py on the CPU, tests/test_gpu_yuv_parts.py and
tests/test_gpu_yuv_tracker.py on the GPU) and what the oracle makes of them.  The checker everywhere is the existing oracle stream
fed the conversion statement's image (tests/yuv_reference.py) -- with an alpha plane of 255 for the tracker.  NV12 and I420 frames of
one scene hold the same samples whatever the padding, so they share one expected result; everything here is computed once."""
import functools

import numpy as np

import yuv_reference as R
from nubovca import synth

PARTS = ("righteye", "lefteye", "nose", "mouth", "leftear", "rightear")
KINDS = {"eye": (0, "righteye", "lefteye"), "nose": (1, "nose", None), "mouth": (2, "mouth", None), "ear": (3, "leftear", "rightear")}
PART_NAMES = {"width_to_process": "width_to_process", "process_x_every_4_frames": "process_x_every_4", "multi_scale_factor": "scale_factor_pct",
              "detect_event": "detect_event"}
# 640 x 480: the exact-2x resize; 800 x 600: the 2.5 truncation quirk and bilinear taps; 322 x 242: the smallest size at which the face
# pass still finds the face -- a width that is no multiple of 4 or 16: every tail, the unaligned eye-gray pitch
PART_GEOS = [(640, 480), (800, 600), (322, 242)]
PART_FRAMES = 9
# 160 x 120 and 1920 x 1080: widths of whole 8-pixel units; 644 x 482: rows that end in a 4-pixel unit and a luma stride that is no
# multiple of 8 unless padded; 322 x 242: w % 4 == 2, the general path whatever the strides
TRK_GEOS = [(160, 120), (644, 482), (1920, 1080), (322, 242)]
TRK_FRAMES = 6


def _tuple(lay):
    return (lay[0], tuple(lay[1]), tuple(lay[2]))


# ---------------------------------------------------------------- part scenes
def _part_faces(W, H, i):
    return [] if i % 6 == 4 else [(W // 5 + 5 * i, H // 5, H // 2)]


def part_has_face(i):
    return i % 6 != 4


@functools.lru_cache(maxsize=None)
def part_frame(W, H, i, fmt, pad=0, luma_rows=None, gap=0, chroma_pad=None):
    """(buffer, layout tuple) of frame i: part_scenes.scene's recipe through synth.make_yuv420; read-only"""
    buf, lay = synth.make_yuv420(W, H, 700 + W + i, fmt, "natural", _part_faces(W, H, i), pad=pad, luma_rows=luma_rows, gap=gap, chroma_pad=chroma_pad)
    buf.setflags(write=False)
    return buf, _tuple(lay)


@functools.lru_cache(maxsize=None)
def part_bgr(W, H, i):
    """the statement's BGR image of frame i"""
    buf, lay = part_frame(W, H, i, R.NV12)
    out = R.bgr(buf, W, H, lay)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def part_cascades():
    """name -> (xml, oracle cascade) of the six part cascades and the face cascade"""
    import orc
    xml = {n: synth.synthetic_part_cascade_xml(n) for n in PARTS}
    xml["face"] = synth.synthetic_cascade_xml()
    return {n: (x, orc.parse_cascade_xml(x)) for n, x in xml.items()}


def oracle_part_stream(kind, **props):
    import orc
    k, a, b = KINDS[kind]
    c = part_cascades()
    return orc.PartStream(k, c["face"][1], c[a][1], c[b][1] if b else None, **{PART_NAMES[n]: v for n, v in props.items()})


@functools.lru_cache(maxsize=None)
def part_expected(kind, W, H, n=PART_FRAMES):
    """[(list A, list B)] of an oracle stream of the kind over frames 0 .. n - 1"""
    o = oracle_part_stream(kind)
    return [o.process(np.array(part_bgr(W, H, i))) for i in range(n)]


# ---------------------------------------------------------------- tracker scenes
@functools.lru_cache(maxsize=None)
def _trk_planes(W, H):
    """[(Y, U, V)] of the 6 frames: a static texture (luma in [60, 120), chroma in [100, 156)) and 6 rectangles with even coordinates
    and sizes that move 8 pixels a frame -- the even-numbered ones set the luma to 210, the odd-numbered ones leave the luma alone and
    set U = 240, V = 16: chroma-only movers, which a kernel that takes Y for gray, or the wrong chroma sample, does not see"""
    rng = np.random.default_rng(11 + W)
    y0 = rng.integers(60, 120, size=(H, W), dtype=np.uint8)
    u0 = rng.integers(100, 156, size=(H // 2, W // 2), dtype=np.uint8)
    v0 = rng.integers(100, 156, size=(H // 2, W // 2), dtype=np.uint8)
    rects = [(2 * int(rng.integers(0, (W - 80) // 2)), 2 * int(rng.integers(0, (H - 60) // 2)), 2 * int(rng.integers(8, 36)), 2 * int(rng.integers(8, 26)),
              int(rng.choice([-8, 8])), int(rng.choice([-8, 0, 8]))) for _ in range(6)]
    frames = []
    for f in range(TRK_FRAMES):
        y, u, v = y0.copy(), u0.copy(), v0.copy()
        for k, (x, yy, w, h, dx, dy) in enumerate(rects):
            px, py = (x + dx * f) % (W - w), (yy + dy * f) % (H - h)
            assert px % 2 == 0 and py % 2 == 0
            if k % 2 == 0:
                y[py:py + h, px:px + w] = 210
            else:
                u[py // 2:(py + h) // 2, px // 2:(px + w) // 2] = 240
                v[py // 2:(py + h) // 2, px // 2:(px + w) // 2] = 16
        frames.append((y, u, v))
    return frames


def pack_planes(y, u, v, fmt, pad=0, chroma_pad=None, gap=0):
    """(buffer, layout tuple) of the planes in make_yuv420's arrangement; what no pixel lies in holds 0xA5; read-only"""
    H, W = y.shape
    cpad = pad if chroma_pad is None else chroma_pad
    if fmt == R.NV12:
        planes = [(y, W + pad), (np.stack([u, v], axis=-1).reshape(H // 2, W), W + cpad)]
    else:
        planes = [(y, W + pad), (u, W // 2 + cpad), (v, W // 2 + cpad)]
    offsets, strides, off = [], [], 0
    for p, st in planes:
        offsets.append(off); strides.append(st)
        off += st * p.shape[0] + gap
    buf = np.full(off - gap, 0xA5, np.uint8)
    for (p, st), o in zip(planes, offsets):
        buf[o:o + st * p.shape[0]].reshape(p.shape[0], st)[:, :p.shape[1]] = p
    buf.setflags(write=False)
    return buf, (fmt, tuple(offsets), tuple(strides))


@functools.lru_cache(maxsize=None)
def trk_frame(W, H, i, fmt, pad=0, chroma_pad=None, gap=0):
    """(buffer, layout tuple) of frame i in make_yuv420's plane arrangement; what no pixel lies in holds 0xA5; read-only"""
    return pack_planes(*_trk_planes(W, H)[i], fmt, pad=pad, chroma_pad=chroma_pad, gap=gap)


@functools.lru_cache(maxsize=None)
def trk_bgra(W, H, i):
    """the statement's image of frame i with an alpha plane of 255"""
    out = np.full((H, W, 4), 255, np.uint8)
    out[..., :3] = R.convert(*_trk_planes(W, H)[i])
    out.setflags(write=False)
    return out


def trk_luma_bgra(W, H, i):
    """the same frame as a kernel that takes Y for gray would see it: B = G = R = Y"""
    out = np.full((H, W, 4), 255, np.uint8)
    out[..., :3] = _trk_planes(W, H)[i][0][..., None]
    return out


def trk_ts(i):
    return 1000.0 + 33.3 * i


def oracle_tracker_run(frames, **props):
    import orc
    t = orc.Tracker(**props)
    return [t.process(np.array(f), trk_ts(i), cap=1 << 16) for i, f in enumerate(frames)]


@functools.lru_cache(maxsize=None)
def trk_expected(W, H):
    """boxes of an oracle tracker over the 6 frames"""
    return oracle_tracker_run([trk_bgra(W, H, i) for i in range(TRK_FRAMES)])
