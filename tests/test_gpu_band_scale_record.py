"""The scale record the tile kernels hold in registers (k_band: once per band, k_tile: once per workgroup), on the smallest plans
where a wrongly held or wrongly ordered field shows: raw candidate lists and grouped boxes against the CPU oracle, once with
k_band forced ("band" = 1) and once with the per-tile kernels forced ("band" = 0).

Three frames of 704 x 400 in ONE batch (noise, a natural field with two pasted templates, a gradient), full resolution, factor
1.1, the stream's default minSize (W / 20 x H / 20).  The plan of that size (test_plan_is_the_one_the_cases_rely_on checks it
with the geometry driver, on the host) has 26 scales, windows of 35 .. 384 pixels:
  * bands of 11, 10, 9, 8, 6, 5, 4, 3, 2 and 1 tiles, the last tile of a band 1 .. 29 windows wide, the last band 1 .. 16 rows high;
  * variance windows on both sides of the sq32 limit (ew * eh * 255^2 < 2^32: a side of 257 pixels): the variance window
    is 18 / 20 of the window, so the scales up to window 262 read the low words of the squared integral only, those from 288 on
    both planes;
  * three batch slots, so the slot terms of the plane and normaliser pointers formed once per band matter.
Record fields the tile kernels read that take at least two values across this plan's scales: eq[0 .. 3], xpos_off, ypos_off,
sq32, task_off, wpr (1 .. 6 reject words a scan row), inv_area, trecs, lrecs.  Constant in this mode: plane_off (0: every scale
reads the full-image planes), pitch (one integral image per slot; the 120 x 120 case below has another) and adaptive (1 for
every scale of a scale-cascade scan).

One more case: a 120 x 120 image searched at the single window size 84 -- one scale, a 9 x 9 grid, one band of one tile -- so
that what k_band does in front of its tile loop is the whole walk."""
import functools

import numpy as np
import pytest

import prefix_cascades as P

W, H = 704, 400
# (seed, content, templates): slot 1 carries the templates the oracle must find (checked on the host below)
FRAMES = [(4101, "noise", []), (4102, "natural", [(60, 40, 150), (420, 90, 260)]), (4103, "gradient", [])]
SMALL = (120, 84, (4, 4, 100))          # image side, the one window size, template


@functools.lru_cache(maxsize=None)
def frame(i):
    from nubovca import synth
    seed, kind, faces = FRAMES[i]
    f = synth.make_bgr(W, H, seed, kind, faces)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def expected_raw(k, i):
    """the oracle's raw list of frame i in scan order (a fresh stream, min_neighbors 0: tests/prefix_cascades.py)"""
    import orc
    kw = dict(width_to_process=W, scale_factor_pct=10, min_neighbors=0)
    out = orc.FaceStream(P.oracle_cascade("calibrated", k), **kw).frame_detect(frame(i), cap=1 << 17)
    assert len(out) < (1 << 17)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_grouped(i):
    """boxes and ids a fresh stream with the default properties (but factor 1.1, full resolution) reports for frame i"""
    import orc
    return orc.FaceStream(P.oracle_cascade("calibrated", 0), width_to_process=W, scale_factor_pct=10).process(frame(i))


@functools.lru_cache(maxsize=None)
def small_case():
    import orc
    from nubovca import synth
    side, win, face = SMALL
    g = orc.equalize_hist(orc.bgr2gray(synth.make_bgr(side, side, 4104, "natural", [face])))
    exp = orc.detect_raw(P.oracle_cascade("calibrated", 5), g, 1.1, 0, (win, win), (win, win))
    return g, exp


# ---------------------------------------------------------------- host: the cases are what the docstring says
def test_plan_is_the_one_the_cases_rely_on():
    pl = P.plan("calibrated", 0, W, H)
    if pl is None:
        pytest.skip("no clang++ for the geometry driver")
    head, scales = pl
    assert len(scales) == 26 and head["strips"] == 0
    tiles_per_band = {len(s["xs"]) for s in scales}
    assert {1, 2, 11} <= tiles_per_band, tiles_per_band
    assert any(s["windows"][0] - s["xs"][-1] < s["tile"][0] for s in scales if len(s["xs"]) > 1)          # partial last tile of a band
    assert any(s["windows"][1] - s["ys"][-1] < s["tile"][1] for s in scales if len(s["ys"]) > 1)          # partial last band
    wins = [s["window"][0] for s in scales]
    assert min(wins) == 35 and max(wins) == 384 and any(w <= 262 for w in wins) and any(w >= 288 for w in wins)      # variance windows of 236 and 260: both sides of 257
    assert {(s["windows"][0] + 63) // 64 for s in scales} == {1, 2, 3, 4, 5, 6}          # wpr


def test_oracle_alone_finds_candidates():
    """no case can pass as empty == empty: the templated frame has candidates at small and at large windows, in the raw lists of
    the stage prefixes and of the full cascade and after grouping; the single-tile case has some too"""
    for k in (3, 5, 0):
        e = expected_raw(k, 1)
        assert 20 <= len(e) < P.HIT_CAP, (k, len(e))
        assert (e[:, 2] <= 262).any() and (e[:, 2] >= 288).any(), sorted(set(e[:, 2].tolist()))
    assert len(expected_raw(3, 0)) > 0 and len(expected_raw(3, 2)) > 1000          # three stages leave some on the noise and the gradient as well
    assert len(expected_grouped(1)[0]) >= 1
    assert len(small_case()[1]) >= 3 and set(small_case()[1][:, 2].tolist()) == {SMALL[1]}


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ctx():
    from nubovca import capi
    c = capi.Context(0)
    c.set_hit_capacity(P.HIT_CAP)
    try:
        yield c
    finally:
        c.set_hit_capacity(16384)          # csrc/context.h
        c.close()


def _launches(ctx):
    return {k: v[1] for k, v in ctx.kernel_timing().items()}


def _frames():
    import torch
    from nubovca import capi
    keep = [torch.from_numpy(np.array(frame(i))).cuda() for i in range(len(FRAMES))]
    torch.cuda.synchronize()
    return keep, [capi.make_frame(t.data_ptr(), W, H, W * 3, capi.MEM_DEVICE) for t in keep]


KERNEL = {1: ("cascade_band", "cascade_tile"), 0: ("cascade_tile", "cascade_band")}


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 5, 0], ids=["prefix3", "prefix5", "full"])
@pytest.mark.parametrize("band", [1, 0], ids=["k_band", "k_tile"])
def test_raw_lists_three_slots(ctx, band, k):
    from nubovca import capi
    casc = ctx.load_cascade_xml(P.cascade_xml("calibrated", k))
    exp = [expected_raw(k, i) for i in range(len(FRAMES))]
    streams = [capi.FaceStream(ctx, casc, width_to_process=W, multi_scale_factor=10, min_neighbors=0) for _ in FRAMES]
    keep, frames = _frames()
    ctx.enable_kernel_timing(1)
    try:
        with ctx.options(band=band):
            res = ctx.face_batch_process(streams, frames, cap=max(len(e) for e in exp) + 64)
        kt = _launches(ctx)
    finally:
        ctx.enable_kernel_timing(0)
    ran, absent = KERNEL[band]
    assert kt.get(ran, 0) >= 1 and kt.get(absent, 0) == 0, kt
    for slot, ((boxes, ids), e) in enumerate(zip(res, exp)):
        j = P.first_difference(boxes, e)
        assert np.array_equal(boxes, e), "slot %d: %d boxes, the oracle has %d; first difference at index %d: %s / %s" % (
            slot, len(boxes), len(e), j, boxes[j].tolist() if j < len(boxes) else None, e[j].tolist() if j < len(e) else None)
        assert np.array_equal(ids, np.arange(len(e)))
    for s in streams:
        s.close()
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 0], ids=["k_band", "k_tile"])
def test_grouped_boxes_three_slots(ctx, band):
    from nubovca import capi
    casc = ctx.load_cascade_xml(P.cascade_xml("calibrated", 0))
    streams = [capi.FaceStream(ctx, casc, width_to_process=W, multi_scale_factor=10) for _ in FRAMES]
    keep, frames = _frames()
    ctx.enable_kernel_timing(1)
    try:
        with ctx.options(band=band):
            res = ctx.face_batch_process(streams, frames, cap=256)
        kt = _launches(ctx)
    finally:
        ctx.enable_kernel_timing(0)
    ran, absent = KERNEL[band]
    assert kt.get(ran, 0) >= 1 and kt.get(absent, 0) == 0, kt
    for slot, (boxes, ids) in enumerate(res):
        eb, ei = expected_grouped(slot)
        assert np.array_equal(boxes, eb) and np.array_equal(ids, ei), (slot, boxes.tolist(), eb.tolist())
    for s in streams:
        s.close()
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("band", [1, 0], ids=["k_band", "k_tile"])
def test_single_scale_single_tile(ctx, band):
    g, exp = small_case()
    win = SMALL[1]
    casc = ctx.load_cascade_xml(P.cascade_xml("calibrated", 5))
    ctx.enable_kernel_timing(1)
    try:
        with ctx.options(band=band, roi=0):          # roi = 0: not the one-workgroup kernel for images whose integrals fit LDS
            got = ctx.detect_raw(casc, g, 1.1, 0, (win, win), (win, win))
        kt = _launches(ctx)
    finally:
        ctx.enable_kernel_timing(0)
    ran, absent = KERNEL[band]
    assert kt.get(ran, 0) >= 1 and kt.get(absent, 0) == 0, kt
    assert np.array_equal(got, exp), (len(got), len(exp), P.first_difference(got, exp))
