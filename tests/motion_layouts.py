"""Motion histories built by construction for the NuboTracker tests (tests/test_motion_layouts_cpu.py on the CPU,
tests/test_gpu_motion_layouts.py on the GPU).  No test in here.

The ABI takes frames, not a motion history, but the history can be painted exactly.  An AGE MAP A[y, x] holds values 0 .. K: 0 means
the pixel never moves, k that it moves at frame k and never again.  Frame 0 is black BGRA with alpha 255; at frame k exactly the
pixels with A == k go from 0 to 255 in B, G and R (gray 0 -> 255: over any threshold below 255).  With a large mhi_duration the
history after frame k is float32(tss[j]) where A == j <= k and 0 elsewhere; with a small one, ages expire as cvUpdateMotionHistory
says.  min_area = 0, max_area = 1 << 30 and distance = 0 turn the tracker's answer into the raw component list in seed order:
(float)0 > dist never holds in __join_objects, and every area is greater than 0.

  paint(age, K)                    the K + 1 frames
  history(age, tss, k, duration)   the float32 history after frame k
  py_segment(mhi, ts, seg)         a third statement of cvSegmentMotion (beside the oracle's flood fill and the kernels): an edge list
                                   and a union-find
  tile_model(mhi, ts, seg)         the kernels' decomposition into tiles of 256 x 8 pixels, stated on the host
  LAYOUTS                          name -> (age, K, tss, tracker parameters by the oracle's names)

A layout is 520 x 50 unless its name says otherwise ("@513x49", "@5x3", ...): two full tile columns and one of 8 pixels, six full
tile rows and one of 2 rows, w % 4 == 0 (the vectorised pixel pass).  At 513 x 49 the last column is a tile's first column and
x == w - 1 at once, the last tile row has one row, and the scalar pixel pass runs."""
import functools

import numpy as np

TILE_W, TILE_H, WAVE = 256, 8, 64
W0, H0 = 520, 50
W1, H1 = 513, 49
RAW = dict(threshold=20, min_area=0, max_area=1 << 30, distance=0, mhi_duration=1.0e6, seg_thresh=32.0)
# the palette {none, t, t - 20, t - 40, t - 60} as ages 0, 4, 3, 2, 1 of a K = 4 script with timestamps 20 apart and seg_thresh 32:
# neighbours in age join, ages two apart do not
PALETTE_TSS = (920.0, 940.0, 960.0, 980.0, 1000.0)
PALETTE_AGE = np.array([0, 4, 3, 2, 1], np.uint8)
STEP_TSS = (1000.0, 1032.0, 1064.0, 1096.0, 1128.0, 1160.0, 1192.0)           # 32 apart: exactly seg_thresh


def roots_cap(w, h, batch=1):
    """entries of the root list of a launch set, as tracker.cpp computes it"""
    return w * h * batch // 8


# ---------------------------------------------------------------- frames and histories
def paint(age, K):
    """[frame 0 .. frame K], BGRA uint8"""
    age = np.asarray(age)
    assert age.max() <= K
    frames = []
    for k in range(K + 1):
        f = np.zeros(age.shape + (4,), np.uint8)
        f[..., 3] = 255
        f[(age >= 1) & (age <= k), :3] = 255
        frames.append(f)
    return frames


def history(age, tss, k, duration):
    """the float32 motion history after frame k (cvUpdateMotionHistory per frame: a moved pixel takes float32(ts); of the others, a
    value below float32(ts - duration) becomes 0, a value equal to it stays)"""
    age = np.asarray(age)
    mhi = np.zeros(age.shape, np.float32)
    for j in range(1, k + 1):
        ts, delbound = np.float32(tss[j]), np.float32(float(tss[j]) - float(duration))
        mhi = np.where(age == j, ts, np.where(mhi < delbound, np.float32(0), mhi)).astype(np.float32)
    return mhi


# ---------------------------------------------------------------- the relation, as an edge list
def _joined(a, b, seg):
    """both non-zero and -seg <= a - b <= seg, all float32"""
    d = a - b
    assert d.dtype == np.float32
    s = np.float32(seg)
    return (a != 0) & (b != 0) & (-s <= d) & (d <= s)


def _edges(mhi, seg, same_tile=False):
    """(a, b) flat pixel indices of the joined 4-neighbour pairs (b right of or below a); same_tile: only pairs inside one tile"""
    h, w = mhi.shape
    idx = np.arange(h * w).reshape(h, w)
    eh = _joined(mhi[:, 1:], mhi[:, :-1], seg)
    ev = _joined(mhi[1:, :], mhi[:-1, :], seg)
    if same_tile:
        eh = eh & ((np.arange(1, w) % TILE_W) != 0)[None, :]
        ev = ev & ((np.arange(1, h) % TILE_H) != 0)[:, None]
    a = np.concatenate([idx[:, :-1][eh], idx[:-1, :][ev]])
    b = np.concatenate([idx[:, 1:][eh], idx[1:, :][ev]])
    return a, b


def _union_find(n, a, b):
    """root (the smallest index of its set) of every index 0 .. n - 1 under the edges (a[i], b[i])"""
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for x, y in zip(a.tolist(), b.tolist()):
        rx, ry = find(x), find(y)
        if rx < ry:
            parent[ry] = rx
        elif ry < rx:
            parent[rx] = ry
    return np.array([find(i) for i in range(n)], np.int64)


def _seeds(mhi, ts):
    return (mhi.view(np.int32) == np.float32(ts).view(np.int32)) & (mhi != 0)


def py_segment(mhi, ts, seg):
    """boxes (x, y, w, h), int32 [n, 4]: one per component that holds a pixel bit-equal to float32(ts), ordered by that component's
    first such pixel in raster order"""
    mhi = np.ascontiguousarray(mhi, np.float32)
    h, w = mhi.shape
    root = _union_find(h * w, *_edges(mhi, seg))
    seeds = np.flatnonzero(_seeds(mhi, ts).reshape(-1))
    order, seen = [], set()
    for r in root[seeds].tolist():
        if r not in seen:
            seen.add(r)
            order.append(r)
    live = np.flatnonzero(mhi.reshape(-1) != 0)
    pos = {r: k for k, r in enumerate(order)}
    lr = root[live]
    keep = np.isin(lr, np.array(order, np.int64))
    k = np.array([pos[r] for r in lr[keep].tolist()], np.int64)
    ys, xs = live[keep] // w, live[keep] % w
    x0 = np.full(len(order), w); x1 = np.full(len(order), -1); y0 = np.full(len(order), h); y1 = np.full(len(order), -1)
    np.minimum.at(x0, k, xs); np.maximum.at(x1, k, xs); np.minimum.at(y0, k, ys); np.maximum.at(y1, k, ys)
    return np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1], axis=1).astype(np.int32)


# ---------------------------------------------------------------- the kernels' decomposition
def tile_model(mhi, ts, seg):
    """What k_ccl_tile / k_ccl_border / k_ccl_fold meet on this history, as a dict:
      ntx, nty         the tile grid
      tile_roots       [nty, ntx] tile-local components per tile: the entries the root list receives (their sum against roots_cap)
      components       per component of the frame: root (its smallest pixel), seed (its first seed pixel or None), tiles (the set of
                       tile numbers ty * ntx + tx it spans), root_tile, seed_tile, local_roots (tile roots that fold into it)
      label            [h, w] root of every pixel, -1 without motion history
      vu               [h, w] the pixel is joined to the one above it
      tied             [h, w] the kernels' redundancy rule holds there (v ~ l, l ~ ul, ul ~ u with l left, u above, ul above left;
                       inside a tile l must lie in the tile, on a tile's top row -- k_ccl_border -- only in the frame)"""
    mhi = np.ascontiguousarray(mhi, np.float32)
    h, w = mhi.shape
    ntx, nty = (w + TILE_W - 1) // TILE_W, (h + TILE_H - 1) // TILE_H
    n = h * w
    flat = mhi.reshape(-1)
    live = np.flatnonzero(flat != 0)
    root = _union_find(n, *_edges(mhi, seg))
    local = _union_find(n, *_edges(mhi, seg, same_tile=True))
    tile_of = ((np.arange(h) // TILE_H)[:, None] * ntx + (np.arange(w) // TILE_W)[None, :]).reshape(-1)
    lroots = live[local[live] == live]
    tile_roots = np.bincount(tile_of[lroots], minlength=ntx * nty).reshape(nty, ntx)
    seeds = np.flatnonzero(_seeds(mhi, ts).reshape(-1))
    first_seed = {}
    for s, r in zip(seeds.tolist(), root[seeds].tolist()):
        first_seed.setdefault(r, s)
    comps = {}
    for p, r in zip(live.tolist(), root[live].tolist()):
        c = comps.get(r)
        if c is None:
            c = comps[r] = dict(root=r, seed=first_seed.get(r), tiles=set(), root_tile=int(tile_of[r]), local_roots=0,
                                seed_tile=int(tile_of[first_seed[r]]) if r in first_seed else None)
        c["tiles"].add(int(tile_of[p]))
    for p in lroots.tolist():
        comps[int(root[p])]["local_roots"] += 1
    label = np.where(flat != 0, root, -1).reshape(h, w)
    z = np.float32(0)
    l = np.zeros_like(mhi); l[:, 1:] = mhi[:, :-1]
    u = np.zeros_like(mhi); u[1:, :] = mhi[:-1, :]
    ul = np.zeros_like(mhi); ul[1:, 1:] = mhi[:-1, :-1]
    vu = _joined(mhi, u, seg)
    tied = vu & _joined(mhi, l, seg) & (ul != z) & _joined(l, ul, seg) & _joined(u, ul, seg)
    in_tile_row = (np.arange(h) % TILE_H != 0)[:, None]
    tile_first_col = (np.arange(w) % TILE_W == 0)[None, :]
    tied = tied & ~(in_tile_row & tile_first_col)
    return dict(ntx=ntx, nty=nty, tile_roots=tile_roots, components=list(comps.values()), label=label, vu=vu, tied=tied)


# ---------------------------------------------------------------- the layouts
def _blank(w, h):
    return np.zeros((h, w), np.uint8)


def serpentine(w, h):
    """one 1-pixel path: every even row in full, joined at alternating ends through the odd rows; one age"""
    a = _blank(w, h)
    a[0::2, :] = 1
    for y in range(1, h - 1, 2):
        a[y, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    return a, 1, STEP_TSS[:2], dict(RAW)


def _spiral(a, x0, y0, x1, y1, pitch, val):
    """a 1-pixel rectangular spiral from (x0, y0) clockwise inwards, `pitch` between its turns"""
    x, y = x0, y0
    while True:
        if x1 - x < 2: break
        a[y, x:x1 + 1] = val; x = x1                       # right
        if y1 - y < 2: break
        a[y:y1 + 1, x] = val; y = y1                       # down
        if x - x0 < 2: break
        a[y, x0:x + 1] = val; x = x0                       # left
        y0 += pitch
        if y - y0 < 2: break
        a[y0:y + 1, x] = val; y = y0                       # up, to the next turn's top row
        x1 -= pitch; y1 -= pitch; x0 += pitch
    return a


def spirals(w, h):
    """two 1-pixel rectangular spirals of pitch 4, the second one 2 pixels inside the first: nested boxes, never 4-adjacent"""
    a = _blank(w, h)
    _spiral(a, 0, 0, w - 1, h - 1, 4, 1)
    _spiral(a, 2, 2, w - 3, h - 3, 4, 1)
    return a, 1, STEP_TSS[:2], dict(RAW)


def comb(w, h, up=False):
    """teeth in every second column from row 1 to the spine in row h - 2; everything is age 1 but the spine's last pixel, age 2: at
    frame 2 the single seed lies in the last tile, the root in the first, and every tooth of every tile row above the spine's is a
    tile root of its own.  up: the same upside down, the spine in row 1 and the seed at the bottom of the last tooth"""
    a = _blank(w, h)
    a[1:h - 1, 0::2] = 1
    a[h - 2, :] = 1
    a[h - 2, w - 1] = 2
    if up:
        a = a[::-1].copy()
        a[1, w - 1] = 1
        a[h - 2, (w - 1) // 2 * 2] = 2
    return a, 2, STEP_TSS[:3], dict(RAW)


def comb_up(w, h):
    return comb(w, h, True)


UNSEEDED_TSS = (900.0, 967.5, 968.0, 990.0, 1000.0)      # age 4 = t; age 1 = t - 32.5: no link to t; age 2 = t - 32: the last value that links


def unseeded_neighbours(w, h):
    """seeded blobs (age 4) with a blob of age 1 (32.5 older: must neither appear nor lend its extent) or of age 2 (32 older: lends
    its extent) against each of their four sides, on wave boundaries, tile columns, tile rows and in tile interiors"""
    a = _blank(w, h)

    def unit(x, y, side, old):
        a[y:y + 3, x:x + 4] = 4
        if side == "right": a[y - 1:y + 4, x + 4:x + 7] = old
        if side == "left": a[y - 1:y + 4, x - 3:x] = old
        if side == "down": a[y + 3:y + 5, x - 1:x + 5] = old
        if side == "up": a[y - 2:y, x - 1:x + 5] = old
    xs = [12, 61, 125, 253, 380, w - 8]                   # interior, 63|64, 127|128 (the blob's own right edge), 255|256, interior, the frame's last columns
    for i, x in enumerate(xs):
        for j, (y, old) in enumerate([(3, 1), (13, 2), (22, 1), (30, 2), (38, 1)]):
            side = ("right", "left", "down", "up")[(i + j) % 4]
            if x == w - 8 and side == "right":
                side = "left"
            unit(x, y, side, old)
    a[h - 2:, 40:44] = 4; a[h - 2:, 44:50] = 1              # the partial last tile row
    a[2:7, 200:204] = 3                                    # something for frame 3
    return a, 4, UNSEEDED_TSS, dict(RAW)


def chain_of_ages(w, h):
    """staircases 4 3 2 1 of the palette (t, t - 20, t - 40, t - 60; seg 32): each step joins the next, the ends do not join each
    other.  Horizontal ones with each of their three links in turn on x = 63|64, 255|256 and 511|512, vertical ones with each link
    on y = 7|8 (and 15|16 reversed), 2 x 4 blocks of a staircase over its reverse, and rows 4 2 1 3 whose
    neighbours are two steps apart"""
    a = _blank(w, h)
    row = 1
    for bx in (64, 256, 512):
        for sh in (1, 2, 3):
            for rev in (False, True):
                if bx - sh + 4 > w:
                    continue
                a[row, bx - sh:bx - sh + 4] = [4, 3, 2, 1][::-1 if rev else 1]
                row += 2
    for k, (by, rev) in enumerate([(8, False), (8, True), (16, False), (16, True), (24, False), (48, True)]):
        for sh in (1, 2, 3):
            y0 = by - sh
            if y0 + 4 > h:
                continue
            a[y0:y0 + 4, 300 + 20 * k + 2 * sh] = [4, 3, 2, 1][::-1 if rev else 1]
    for bx in (30, 62, 254, min(510, w - 4)):
        a[39:41, bx:bx + 4] = [[4, 3, 2, 1], [1, 2, 3, 4]]
        a[46:48, bx:bx + 4] = [[1, 2, 3, 4], [2, 3, 4, 3]]
        a[43, bx:bx + 4] = [4, 2, 1, 3]                    # broken: three components at seg 32, one at seg 40
    return a, 4, PALETTE_TSS, dict(RAW)


# all 5^4 fillings of a 2 x 2 block: 5 columns and 125 rows of patterns at pitch 3, in ten shifted copies of 270 x 384 pixels.  Copy c
# puts pattern column c % 5 on x = 63|64 (c < 5) or on x = 255|256 (c >= 5), and its rows start at c % 8: every pattern meets a wave
# boundary, a tile's left column, a tile's top row and a tile interior in some copy (tests/test_motion_layouts_cpu.py counts them)
PAT_W, PAT_H, PAT_COPIES = 270, 384, 10


def pattern_cells(p):
    """palette indices of pattern p (0 .. 624): [[top left, top right], [bottom left, bottom right]]"""
    return np.array([[p % 5, p // 5 % 5], [p // 25 % 5, p // 125]])


def pattern_origins(c):
    """[625, 2] (x, y) of the patterns' top left pixels in copy c"""
    sx = (63 if c < 5 else 255) - 3 * (c % 5)
    sy = c % 8
    p = np.arange(625)
    return np.stack([sx + 3 * (p % 5), sy + 3 * (p // 5)], axis=1)


def patterns_2x2(c):
    a = _blank(PAT_W, PAT_H)
    for p, (x, y) in enumerate(pattern_origins(c).tolist()):
        a[y:y + 2, x:x + 2] = PALETTE_AGE[pattern_cells(p)]
    return a, 4, PALETTE_TSS, dict(RAW)


def random_field(w, h, density, seed):
    rng = np.random.default_rng(seed)
    a = PALETTE_AGE[rng.integers(1, 5, size=(h, w))]
    a[rng.random((h, w)) >= density] = 0
    a[0, 0] = 4; a[h - 1, w - 1] = 3; a[h // 2, w // 2] = 2; a[h - 1, 0] = 1          # every frame moves something at every density
    return a, 4, PALETTE_TSS, dict(RAW)


def expiring(w, h):
    """mhi_duration 64 on timestamps 32 apart: age j lives through frames j, j + 1 and j + 2 -- at j + 2 it sits exactly on ts - duration
    and stays -- and is gone at j + 3.  One bar over all tile columns and one over all tile rows, in six sections of ages 1 .. 6 each:
    the component loses its oldest part frame by frame, tiles die beside live ones"""
    a = _blank(w, h)
    K = 6
    for j in range(K):
        a[10:14, j * w // K:(j + 1) * w // K] = j + 1
        a[j * h // K:(j + 1) * h // K, 300:303] = K - j
    a[30:33, 20:40] = 1; a[30:33, 40:60] = 4                # parts that never meet alive
    p = dict(RAW, mhi_duration=64.0)
    return a, K, STEP_TSS[:K + 1], p


def seg_edge(w, h, base=None):
    """bands of ages 1 2 3 side by side and one above the other: 1 -> 2 is 32.5 (34 at 2^24) apart and does not join, 2 -> 3 exactly 32
    and joins"""
    a = _blank(w, h)
    for k, bx in enumerate((20, 63, 255, w - 5)):
        a[2 + 9 * k:6 + 9 * k, bx - 1:bx + 2] = [1, 2, 3] if bx != w - 5 else [3, 2, 1]
        a[2 + 9 * k:6 + 9 * k, bx - 12] = 1
    for k, by in enumerate((8, 24, 48)):
        if by + 1 < h:
            a[by - 2:by + 1, 100 + 30 * k:110 + 30 * k] = np.array([1, 2, 3])[:, None]
            a[by - 2:by + 1, 300 + 30 * k:310 + 30 * k] = np.array([3, 2, 1])[:, None]
    tss = (1000.0, 1032.0, 1064.5, 1096.5) if base is None else tuple(base + d for d in (0.0, 32.0, 66.0, 98.0))
    return a, 3, tss, dict(RAW)


def seg_edge_2p24(w, h):
    return seg_edge(w, h, float(1 << 24))


def clock_oddities(w, h):
    """blobs of ages 1 .. 5 in a touching row, on tile and wave boundaries.  Frame 2 repeats frame 1's timestamp (the pixels of frame 1
    are seeds again), frame 3's goes backwards, frame 4 is processed at ts = 0.0 (its pixels enter the history as 0: no component at
    all), frame 5 is ordinary again"""
    a = _blank(w, h)
    for k, bx in enumerate((10, 54, 246, 500)):
        y = 3 + 11 * k
        for j in range(5):
            a[y:y + 6 + j % 2, bx + 4 * j:bx + 4 * j + 4] = j + 1
    a[6:10, 400:404] = [[1, 2, 3, 5]] * 4
    return a, 5, (1000.0, 1032.0, 1032.0, 1020.0, 0.0, 1050.0), dict(RAW)


AREA_W, AREA_H = 604, 36


def area_edges():
    """604 x 36 (a box of 1 x 599 pixels needs the width).  min_area 50, max_area 600: 5 x 10 = 50 and 20 x 30 = 600 are dropped,
    3 x 17 = 51 and 599 x 1 = 599 are kept (the kernel's own filter and __join_objects ask the same)"""
    a = _blank(AREA_W, AREA_H)
    a[2:12, 10:15] = 1
    a[3:33, 100:120] = 1
    a[4:21, 250:253] = 1
    a[34, 3:602] = 1
    return a, 1, STEP_TSS[:2], dict(RAW, min_area=50, max_area=600)


def lattice(w, h, n, with_later=True):
    """n single pixels (age 1) on the odd / odd lattice, in raster order; mhi_duration 40 on timestamps 32 apart keeps them through
    frame 2, where a blob of age 2 lies over some of them, and drops them at frame 3, where a blob of age 3 moves alone"""
    a = _blank(w, h)
    ys, xs = np.meshgrid(np.arange(1, h, 2), np.arange(1, w, 2), indexing="ij")
    assert n <= ys.size
    a[ys.reshape(-1)[:n], xs.reshape(-1)[:n]] = 1
    if with_later:
        a[0:4, 30:40][a[0:4, 30:40] == 0] = 2
        a[h - 6:h - 2, 300:310][a[h - 6:h - 2, 300:310] == 0] = 3
    return a, 3, STEP_TSS[:4], dict(RAW, mhi_duration=40.0)


def one_blob(w, h):
    """one blob a frame, each inside one tile: a single entry of the root list"""
    a = _blank(w, h)
    a[17:21, 100:108] = 1; a[26:30, 300:308] = 2; a[33:37, 400:408] = 3
    return a, 3, STEP_TSS[:4], dict(RAW, mhi_duration=40.0)


def blank(w, h, K=3):
    """nothing ever moves (not in LAYOUTS: its lists are empty on purpose)"""
    return _blank(w, h), K, STEP_TSS[:K + 1], dict(RAW, mhi_duration=40.0)


def _build():
    L = {}
    both = dict(serpentine=serpentine, spirals=spirals, comb=comb, comb_up=comb_up, unseeded_neighbours=unseeded_neighbours,
                chain_of_ages=chain_of_ages, expiring=expiring, seg_edge=seg_edge, seg_edge_2p24=seg_edge_2p24, clock_oddities=clock_oddities)
    for name, fn in both.items():
        L[name] = fn(W0, H0)
        L["%s@%dx%d" % (name, W1, H1)] = fn(W1, H1)
    # slots of one batched call with parameters of their own: seg_thresh 19.5 (no two ages join), 40 (ages two steps apart join too),
    # and an area window that drops the bare blobs (3 x 4 = 12) and the largest unions (7 x 5 = 35 is kept, 6 x 7 = 42 is not)
    a, K, tss, p = chain_of_ages(W0, H0)
    L["chain_of_ages/seg19.5"] = (a, K, tss, dict(p, seg_thresh=19.5))
    L["chain_of_ages/seg40"] = (a, K, tss, dict(p, seg_thresh=40.0))
    a, K, tss, p = unseeded_neighbours(W0, H0)
    L["unseeded_neighbours/area"] = (a, K, tss, dict(p, min_area=12, max_area=42))
    for c in range(PAT_COPIES):
        L["patterns_2x2/%d@%dx%d" % (c, PAT_W, PAT_H)] = patterns_2x2(c)
    for (w, h) in ((5, 3), (64, 8), (256, 8), (257, 9), (W1, H1), (W0, H0)):
        for d in (0.35, 0.7, 1.0):
            name = "random_fields/%g" % d + ("" if (w, h) == (W0, H0) else "@%dx%d" % (w, h))
            L[name] = random_field(w, h, d, 1000 * w + 10 * h + int(d * 10))
    L["area_edges@%dx%d" % (AREA_W, AREA_H)] = area_edges()
    L["readback_1024"] = lattice(W0, H0, 1024)
    L["readback_1025"] = lattice(W0, H0, 1025)
    L["roots_at_cap"] = lattice(W0, H0, roots_cap(W0, H0))
    L["roots_over_cap"] = lattice(W0, H0, roots_cap(W0, H0) + 1)
    L["roots_full_lattice"] = lattice(W0, H0, (W0 // 2) * (H0 // 2))
    L["one_blob"] = one_blob(W0, H0)
    return L


LAYOUTS = _build()
NAMES = sorted(LAYOUTS)


def size(name):
    h, w = LAYOUTS[name][0].shape
    return w, h


@functools.lru_cache(maxsize=None)
def frames(name):
    age, K = LAYOUTS[name][:2]
    out = paint(age, K)
    for f in out:
        f.setflags(write=False)
    return out


def oracle_run(frame_list, tss, params, cap=1 << 16):
    import orc
    t = orc.Tracker(**params)
    return [t.process(np.array(f), ts, cap=cap) for f, ts in zip(frame_list, tss)]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle tracker's list after every frame of the layout (computed once, shared, left alone)"""
    age, K, tss, params = LAYOUTS[name]
    return oracle_run(frames(name), tss, params)


@functools.lru_cache(maxsize=None)
def model(name, k):
    """tile_model of the layout's history after frame k"""
    age, K, tss, params = LAYOUTS[name]
    return tile_model(history(age, tss, k, params["mhi_duration"]), tss[k], params["seg_thresh"])


def gpu_props(params):
    """the oracle's parameter names as nubovca.capi.Tracker's"""
    names = dict(threshold="set_threshold", min_area="set_min_area", max_area="set_max_area", distance="set_distance",
                 mhi_duration="mhi_duration", seg_thresh="seg_thresh")
    return {names[k]: v for k, v in params.items()}
