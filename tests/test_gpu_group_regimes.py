"""k_group (csrc/kernels_group.hip) at its limits, on candidate sets built by construction (tests/marker_cascades.py; that the
layouts are in the regimes they are named for is checked on the host, tests/test_group_regimes_cpu.py).

Everything is compared bit for bit and in order against the CPU oracle:
  (a) every layout through nvca_detect_multiscale at the thresholds 1, 2, 3, 5, 9 on three routes: the device's answer stored
      into page-locked host memory, the device's answer through a copy (group_zerocopy = 0), and grouping on the host
      (host_group = 1); the kernel timers say which route ran;
  (b) the raw lists of the same layouts (the cascade kernels deliver these sets at all), with the per-tile kernels and with k_band;
  (c) the same rectangle lists, shuffled, through nvca_group_rectangles (the host implementation);
  (d) one batch of fresh face streams whose slots decline, answer, are empty, skip grouping, overflow the box table and carry four
      different min_neighbors, with both output routes, as device frames and as host frames in chunks (result slots r0 > 0);
  (e) the per-slot threshold array over a script of property changes, smaller and larger batches and two batches in flight.

What these comparisons cannot see: WHICH side grouped a slot.  A slot the kernel declines is grouped by the host from the raw list,
to the same boxes, and nothing in the ABI tells the two apart -- so moving a decline point by one (2048 candidates, 256 classes) in the
harmless direction changes no result here, only who did the work.  The layouts on both sides of each limit check that the answer is
right whoever gives it.  Nor can any input reach the tie term of the rank sort: the keys of a slot are distinct windows."""
import numpy as np
import pytest

import marker_cascades as M

pytestmark = pytest.mark.gpu

NAMES = sorted(M.LAYOUTS)
ROUTES = {"zerocopy": {}, "copy": {"group_zerocopy": 0}, "host": {"host_group": 1}}


@pytest.fixture(scope="module")
def ctx():
    from nubovca import capi
    c = capi.Context(0)
    try:
        yield c
    finally:
        c.close()


@pytest.fixture(scope="module")
def casc(ctx):
    return ctx.load_cascade_xml(M.marker_xml())


class timed:
    """the context's kernel launches inside a with-block (name -> launches)"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.enable_kernel_timing(1)
        return self

    def __exit__(self, *exc):
        self.kt = {k: v[1] for k, v in self.ctx.kernel_timing().items()}
        self.ctx.enable_kernel_timing(0)

    def n(self, name):
        return self.kt.get(name, 0)


def _same(got, exp, what):
    assert np.array_equal(got, exp), "%s: %d boxes, the oracle has %d; first difference at index %d\n got %s\n exp %s" % (
        what, len(got), len(exp), _first_difference(got, exp), got[:8].tolist(), exp[:8].tolist())


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero((a[:n] != b[:n]).any(axis=1))[0]
    return int(d[0]) if len(d) else n


# ---------------------------------------------------------------- (a) detectMultiScale, three routes
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", NAMES)
def test_detect_multiscale(ctx, casc, name, route):
    l = M.LAYOUTS[name]
    g = l.gray()
    with ctx.options(roi=0, **ROUTES[route]), timed(ctx) as t:
        got = [ctx.detect_multiscale(casc, g, l.scale_factor, thr, 0, l.min_size, l.max_size) for thr in M.THRESHOLDS]
    if route == "host":
        assert t.n("group_rects") == 0, t.kt
    else:
        assert t.n("group_rects") == len(M.THRESHOLDS), t.kt
    assert t.n("cascade_roi") == 0, t.kt
    for thr, boxes in zip(M.THRESHOLDS, got):
        _same(boxes, M.expected_grouped(name, thr)[0], "%s, threshold %d, %s" % (name, thr, route))


# ---------------------------------------------------------------- (b) the raw lists
@pytest.mark.parametrize("band", [0, 1], ids=["k_tile", "k_band"])
@pytest.mark.parametrize("name", NAMES)
def test_detect_raw(ctx, casc, name, band):
    l = M.LAYOUTS[name]
    with ctx.options(roi=0, band=band), timed(ctx) as t:
        got = ctx.detect_raw(casc, l.gray(), l.scale_factor, 0, l.min_size, l.max_size, cap=8192)
    ran, absent = ("cascade_band", "cascade_tile") if band else ("cascade_tile", "cascade_band")
    assert t.n(ran) >= 1 and t.n(absent) == 0 and t.n("group_rects") == 0, t.kt
    _same(got, M.expected_raw(name), name)


# ---------------------------------------------------------------- (c) the host implementation, shuffled lists
@pytest.mark.parametrize("name", NAMES)
def test_host_group_rectangles_shuffled(ctx, name):
    import orc
    r = np.array(M.expected_raw(name))
    np.random.default_rng(len(r) + 7).shuffle(r)
    for thr in (0, 1, 2, 3):
        exp, _ = orc.group_rectangles(r, thr)
        _same(ctx.group_rectangles(r, thr), exp, "%s shuffled, threshold %d" % (name, thr))
        assert np.array_equal(exp, M.py_group(r, thr).boxes)


# ---------------------------------------------------------------- (d) the batched face path
# (frame, min_neighbors) per slot
FACE_SLOTS = [("three", 3), ("grid36", 3), ("black", 3), ("three", 0), ("edge70", 1),
              ("ladder", 1), ("ladder", 2), ("ladder", 3), ("ladder", 5)]
FACE_CAP = 256


def _face_streams(ctx, casc, thresholds):
    from nubovca import capi
    return [capi.FaceStream(ctx, casc, width_to_process=M.FACE_W, multi_scale_factor=10, min_neighbors=t) for t in thresholds]


def _frames(arrays, mem):
    """Frame records of the BGR arrays: host memory, or device copies (returned as well: they must outlive the call)"""
    from nubovca import capi
    if mem == "host":
        return None, [capi.make_frame(np.array(a)) for a in arrays]
    import torch
    keep = [torch.from_numpy(np.array(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return keep, [capi.make_frame(t.data_ptr(), M.FACE_W, M.FACE_H, M.FACE_W * 3, capi.MEM_DEVICE) for t in keep]


def _check_slots(res, exp, what):
    assert len(res) == len(exp)
    for slot, ((boxes, ids), (eb, ei)) in enumerate(zip(res, exp)):
        _same(boxes, eb, "%s, slot %d" % (what, slot))
        assert np.array_equal(ids, ei), (what, slot, ids.tolist(), ei.tolist())


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("zerocopy", [1, 0], ids=["zerocopy", "copy"])
def test_face_batch_slots(ctx, casc, zerocopy, mem):
    exp = [M.face_expected(name, mn) for (name, mn) in FACE_SLOTS]
    assert max(len(b) for (b, _) in exp) < FACE_CAP
    streams = _face_streams(ctx, casc, [mn for (_, mn) in FACE_SLOTS])
    keep, frames = _frames([M.face_frame(name) for (name, _) in FACE_SLOTS], mem)
    # host frames go through in chunks of 4: three launch sets with result slots 0, 4 and 8
    with ctx.options(group_zerocopy=zerocopy, ingest_chunk=4), timed(ctx) as t:
        res = ctx.face_batch_process(streams, frames, cap=FACE_CAP)
    assert t.n("group_rects") == (3 if mem == "host" else 1), t.kt
    _check_slots(res, exp, "face batch (%s frames, group_zerocopy %d)" % (mem, zerocopy))
    for s in streams:
        s.close()
    del keep


# ---------------------------------------------------------------- (e) the threshold array
def test_threshold_script(ctx, casc):
    streams = _face_streams(ctx, casc, M.FIRST_THRESHOLDS)
    _, frames = _frames([M.stream_frame(i) for i in range(M.N_STREAMS)], "host")
    expected = iter(M.threshold_script_expected())

    def check(res, idx, step):
        e_idx, thr, exp = next(expected)
        assert e_idx == list(idx)
        _check_slots(res, exp, "step %d, streams %s, min_neighbors %s" % (step, list(idx), thr))

    for step, op in enumerate(M.THRESHOLD_SCRIPT):
        if op[0] == "set":
            for i, t in op[1].items():
                streams[i].set_property("min_neighbors", t)
        elif op[0] == "run":
            idx = op[1]
            with timed(ctx) as t:
                res = ctx.face_batch_process([streams[i] for i in idx], [frames[i] for i in idx], cap=FACE_CAP)
            assert t.n("group_rects") == 1, t.kt
            check(res, idx, step)
        else:
            a, b = op[1], op[2]
            with timed(ctx) as t:
                ta = ctx.face_batch_submit([streams[i] for i in a], [frames[i] for i in a])
                tb = ctx.face_batch_submit([streams[i] for i in b], [frames[i] for i in b])
                ra = ctx.face_batch_collect(ta, cap=FACE_CAP)
                rb = ctx.face_batch_collect(tb, cap=FACE_CAP)
            assert t.n("group_rects") == 2, t.kt
            check(ra, a, step)
            check(rb, b, step)
    assert next(expected, None) is None
    for s in streams:
        s.close()
