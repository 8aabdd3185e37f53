"""Stage prefixes of a cascade, the oracle's RAW candidate list of a face stream's frame, and the tile cells of the product's plan
that a list touches (tests/test_raw_batch_cpu.py, tests/test_gpu_raw_batch.py).

A face stream with min_neighbors = 0 skips groupRectangles, and on the first frame of a fresh stream the temporal logic turns
every detection into a new face, in order: the boxes such a stream returns ARE the raw list.  The full cascades leave a hundred
candidates in 3 % of the (scale, tile) cells the tile kernels walk; the first 3 .. 12 stages of the calibrated cascade leave
thousands, in nearly every cell, so that a wrong halo column, last band, edge tile or slot shows as a list that differs instead
of as an isolated false accept that grouping removes."""
import bisect
import functools
import json
import os
import subprocess
import xml.etree.ElementTree as ET

import numpy as np

from nubovca import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = os.path.join(ROOT, "tests", "geom")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

ORC_MAX_FACES = 256          # oracle/orc_pipe.c: an oracle stream keeps (and returns) at most this many faces
HIT_CAP = 65536              # raw candidates per frame the GPU tests size the product's lists for
FACES_1080 = [(200, 150, 300), (900, 400, 180), (1400, 100, 120), (1500, 700, 240)]

CASCADES = {"calibrated": synth.calibrated_cascade_xml, "synthetic": synth.synthetic_cascade_xml}


def prefix(xml, k):
    """the old-format cascade XML cut to its first k stages"""
    root = ET.fromstring(xml)
    node = next(c for c in root if c.get("type_id") == "opencv-haar-classifier")
    stages = node.find("stages")
    kids = list(stages)
    assert 1 <= k <= len(kids), (k, len(kids))
    for st in kids[k:]:
        stages.remove(st)
    return '<?xml version="1.0"?>\n' + ET.tostring(root, encoding="unicode") + "\n"


@functools.lru_cache(maxsize=None)
def cascade_xml(name, k=0):
    """CASCADES[name], whole (k = 0) or cut to its first k stages"""
    xml = CASCADES[name]()
    return prefix(xml, k) if k else xml


@functools.lru_cache(maxsize=None)
def oracle_cascade(name, k=0):
    import orc
    return orc.parse_cascade_xml(cascade_xml(name, k))


# ---------------------------------------------------------------- frames
# name -> (W, H, frames, content of frame i).  "hd": the frames of test_face_batch_1080p_*_vs_oracle (tests/test_gpu_timed_path.py);
# continued to 16; its first 8 are the batch the prefixes run on, all 16 the batch NVCA_BAND_MAP=2 needs.  "p720": one frame of each of 32 streams (BASELINE configs[3]).
def _hd(i):
    return synth.frame_seed(0, i), "natural", [(x + 8 * i, y, s) for (x, y, s) in FACES_1080] if i % 5 != 3 else []


def _p720(s):
    return synth.frame_seed(s, 0), "natural", [(120 + 16 * (s % 7), 100, 200), (600 + 5 * s, 300, 120)] if s % 6 else []


def _q360(i):
    return 300 + i, "natural", [(30 + 9 * i, 40 + (i % 5) * 20, 120 + 4 * i)] if i % 4 != 3 else []


def _q300(i):
    return 900 + i, "natural", [(20 + 10 * i, 30 + (i % 4) * 25, 110 + 5 * i)]


def _sd450(i):
    return 8100 + 7 * i, ["natural", "gradient", "noise"][i % 3], [(40 + 37 * i % 400, 30 + 11 * i % 150, 120 + 9 * (i % 8))] if i % 4 != 2 else []


FRAME_SETS = {"hd": (1920, 1080, 16, _hd), "p720": (1280, 720, 32, _p720), "q360": (480, 360, 21, _q360),
              "q300": (400, 300, 18, _q300), "sd450": (800, 450, 8, _sd450)}


@functools.lru_cache(maxsize=None)
def frame(fset, i):
    W, H, n, content = FRAME_SETS[fset]
    assert 0 <= i < n
    seed, kind, faces = content(i)
    f = synth.make_bgr(W, H, seed, kind, faces)
    f.setflags(write=False)
    return f


def has_faces(fset, i):
    return len(FRAME_SETS[fset][3](i)[2]) > 0


# ---------------------------------------------------------------- expected lists
@functools.lru_cache(maxsize=None)
def raw_expected(name, k, fset, i, width_to_process=0, policy=0):
    """the boxes a fresh face stream (min_neighbors 0, multi-scale-factor 10) returns for frame i of the set: the oracle's raw list
    in scan order, scaled as the stream scales its events.  Lists of 256 or more come from the stream's stateless half
    (the oracle stream itself keeps ORC_MAX_FACES), in full-resolution mode only, where working-image boxes are frame boxes."""
    import orc
    f = frame(fset, i)
    W = f.shape[1]
    w2p = width_to_process or W
    kw = dict(width_to_process=w2p, scale_factor_pct=10, min_neighbors=0, policy=policy)
    boxes, ids = orc.FaceStream(oracle_cascade(name, k), **kw).process(f)
    if len(boxes) < ORC_MAX_FACES:
        assert np.array_equal(ids, np.arange(len(boxes)))
        out = boxes
    else:
        assert w2p == W, "a list the oracle stream truncates is only known in full-resolution mode"
        out = orc.FaceStream(oracle_cascade(name, k), **kw).frame_detect(f, cap=1 << 17)
        assert ORC_MAX_FACES <= len(out) < (1 << 17) and np.array_equal(out[:ORC_MAX_FACES], boxes)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- the product's plan and its tile cells
def geometry_driver():
    """tests/geom/tile_geom_driver built against the product's plan.cpp; None where there is no clang++"""
    if not os.path.exists(CLANG):
        return None
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(GEOM, "build", "tile_geom_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(GEOM, "tile_geom_driver.cpp")] + [os.path.join(csrc, f) for f in ("cascade_xml.cpp", "plan.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = [CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
               "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out + ".tmp"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + ".tmp", out)
    return out


@functools.lru_cache(maxsize=None)
def plan(name, k, W, H):
    """(head, scales) of the plan a full-resolution face stream (sf 1.1, minSize W/20 x H/20) gets for the cascade: the JSON lines of
    the geometry driver; None where the driver cannot be built"""
    import tempfile
    drv = geometry_driver()
    if drv is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "face.xml")
        with open(p, "w") as fh:
            fh.write(cascade_xml(name, k))
        r = subprocess.run([drv, p, str(W), str(H), "1.1", str(W // 20), str(H // 20)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    return lines[0], lines[1:]


def cv_round(v):
    return int(np.rint(v))          # round half to even, as cvRound


def locate(plan_scales, box):
    """(scale, tile column, tile row) of a raw candidate (frame coordinates of a full-resolution stream): the scale by the
    window size cvRound(ow f) x cvRound(oh f), the window index by the scan step max(2, f), the cell by the tile origins"""
    x, y, w, h = (int(v) for v in box)
    hit = [s for s in plan_scales if s["window"] == [w, h]]
    assert len(hit) == 1, (box, [s["window"] for s in plan_scales])
    s = hit[0]
    step = max(2.0, s["factor"])
    ix, iy = int(round(x / step)), int(round(y / step))
    assert cv_round(ix * step) == x and cv_round(iy * step) == y, (box, s["factor"], ix, iy)
    assert 0 <= ix < s["windows"][0] and 0 <= iy < s["windows"][1], (box, ix, iy, s["windows"])
    return s["scale"], bisect.bisect_right(s["xs"], ix) - 1, bisect.bisect_right(s["ys"], iy) - 1


def all_cells(plan_scales):
    return {(s["scale"], tx, ty) for s in plan_scales for tx in range(len(s["xs"])) for ty in range(len(s["ys"]))}


def tile_cells(plan_scales, raw):
    """the set of (scale, tile column, tile row) cells of the plan that hold a candidate of the list"""
    by_size = {tuple(s["window"]): s for s in plan_scales}
    assert len(by_size) == len(plan_scales)
    raw = np.asarray(raw).reshape(-1, 4)
    cells = set()
    for (w, h) in {(int(a), int(b)) for a, b in raw[:, 2:4]}:
        s = by_size[(w, h)]
        sel = raw[(raw[:, 2] == w) & (raw[:, 3] == h)]
        step = max(2.0, s["factor"])
        ix, iy = np.rint(sel[:, 0] / step).astype(int), np.rint(sel[:, 1] / step).astype(int)
        assert np.array_equal(np.rint(ix * step).astype(int), sel[:, 0]) and np.array_equal(np.rint(iy * step).astype(int), sel[:, 1]), (w, h)
        assert ix.min() >= 0 and iy.min() >= 0 and ix.max() < s["windows"][0] and iy.max() < s["windows"][1], (w, h, s["windows"])
        tx = np.searchsorted(np.asarray(s["xs"]), ix, side="right") - 1
        ty = np.searchsorted(np.asarray(s["ys"]), iy, side="right") - 1
        cells.update((s["scale"], int(a), int(b)) for a, b in set(zip(tx.tolist(), ty.tolist())))
    return cells


def first_difference(got, exp):
    """index of the first row in which two ordered lists differ (the shorter list's length if one is a prefix of the other)"""
    n = min(len(got), len(exp))
    d = np.nonzero((np.asarray(got[:n]) != np.asarray(exp[:n])).any(axis=1))[0]
    return int(d[0]) if len(d) else n
