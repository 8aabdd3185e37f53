"""RAW candidate lists of the batched face path (nvca_face_batch_process / _submit / _collect), on every tile.

The other tests that reach k_band with a real batch compare grouped boxes and ids: groupRectangles hides 12 % .. 48 % of single lost
windows and every isolated false accept (tests/test_raw_batch_cpu.py prints the counts), and the full cascades leave candidates in
3 % of the (scale, tile) cells the kernel walks.  Here every stream has min_neighbors = 0 and is fresh, so the boxes it returns are
the raw list of its frame in scan order (tests/prefix_cascades.py), and stage prefixes of the calibrated cascade put thousands of
candidates into nearly every tile cell (coverage conditions: test_raw_batch_cpu.py).  Every comparison is np.array_equal on the
ordered list against the CPU oracle; a mismatch names the first differing index and its (slot, scale, tile cell).  Which cascade
kernel ran is read back from the kernel timers."""
import numpy as np
import pytest

import prefix_cascades as P

pytestmark = pytest.mark.gpu

DEFAULT_HIT_CAP = 16384          # csrc/context.h


@pytest.fixture(scope="module")
def ctx():
    from nubovca import capi
    c = capi.Context(0)
    c.set_hit_capacity(P.HIT_CAP)
    try:
        yield c
    finally:
        c.set_hit_capacity(DEFAULT_HIT_CAP)
        c.close()


@pytest.fixture(scope="module")
def cascs(ctx):
    """(cascade name, stages kept or 0) -> device cascade, loaded on first use"""
    loaded = {}

    def get(name, k=0):
        if (name, k) not in loaded:
            loaded[(name, k)] = ctx.load_cascade_xml(P.cascade_xml(name, k))
        return loaded[(name, k)]
    return get


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


_DEVICE = {}


def _device_frame(fset, i):
    """frame i of the set in device memory (kept for the module: the sets are shared between the tests)"""
    import torch
    from nubovca import capi
    if (fset, i) not in _DEVICE:
        _DEVICE[(fset, i)] = torch.from_numpy(np.array(P.frame(fset, i))).cuda()
        torch.cuda.synchronize()
    t = _DEVICE[(fset, i)]
    W, H = P.FRAME_SETS[fset][:2]
    return capi.make_frame(t.data_ptr(), W, H, W * 3, capi.MEM_DEVICE)


def _host_frame(fset, i):
    from nubovca import capi
    return capi.make_frame(np.array(P.frame(fset, i)))          # a writable copy that the Frame keeps alive


class Batch:
    """one batch: frames (set, index) with the cascade each one's FRESH stream scans with, min_neighbors 0"""

    def __init__(self, ctx, cascs, items, mem="device", width_to_process=0, policy=0):
        from nubovca import capi
        self.ctx, self.items, self.w2p, self.policy = ctx, items, width_to_process, policy
        self.exp = [P.raw_expected(name, k, fset, i, width_to_process, policy) for (name, k, fset, i) in items]
        self.cap = max(len(e) for e in self.exp) + 64          # a list that is too long shows as a longer list
        self.streams = [capi.FaceStream(ctx, cascs(name, k), width_to_process=width_to_process or P.FRAME_SETS[fset][0],
                                        multi_scale_factor=10, min_neighbors=0) for (name, k, fset, i) in items]
        self.frames = [(_device_frame if mem == "device" else _host_frame)(fset, i) for (name, k, fset, i) in items]

    def process(self):
        return self.check(self.ctx.face_batch_process(self.streams, self.frames, cap=self.cap))

    def submit(self):
        self.ticket = self.ctx.face_batch_submit(self.streams, self.frames)
        return self

    def collect(self):
        return self.check(self.ctx.face_batch_collect(self.ticket, cap=self.cap))

    def _where(self, slot, box):
        name, k, fset, i = self.items[slot]
        W, H = P.FRAME_SETS[fset][:2]
        if self.w2p not in (0, W):
            return "(shrunk working image)"
        try:
            pl = P.plan(name, k, W, H)
            return "(scale, tile column, tile row) %s" % (P.locate(pl[1], box),) if pl else "(no geometry driver)"
        except AssertionError as e:
            return "not a window of the plan: %s" % (e,)

    def check(self, res):
        assert len(res) == len(self.items)
        for slot, ((boxes, ids), exp) in enumerate(zip(res, self.exp)):
            if not np.array_equal(boxes, exp):
                j = P.first_difference(boxes, exp)
                got = "%s %s" % (boxes[j].tolist(), self._where(slot, boxes[j])) if j < len(boxes) else "nothing"
                want = "%s %s" % (exp[j].tolist(), self._where(slot, exp[j])) if j < len(exp) else "nothing"
                pytest.fail("slot %d %s: %d boxes, the oracle has %d; first difference at index %d: got %s, expected %s"
                            % (slot, self.items[slot], len(boxes), len(exp), j, got, want))
            assert np.array_equal(ids, np.arange(len(exp))), (slot, self.items[slot])          # a fresh stream numbers its faces in order
        return sum(len(e) for e in self.exp)

    def close(self):
        for s in self.streams:
            s.close()


def _hd(name, k, n=8, order=None):
    return [(name, k, "hd", i) for i in (order if order is not None else range(n))]


# ---------------------------------------------------------------- the headline shape with the full cascades
@pytest.mark.parametrize("name", ["calibrated", "synthetic"])
def test_headline_full_cascades(ctx, cascs, name):
    """BASELINE configs[1] as bench.py runs it, but raw: 12 device-resident 1920 x 1080 frames of differing content (two of them
    without faces), one nvca_face_batch_process call -> k_band; then two batches in flight through submit / collect, the
    second with the frames in reverse order (other slots for the same lists), fresh streams per batch"""
    b = Batch(ctx, cascs, _hd(name, 0, 12))
    with timed(ctx) as t:
        seen = b.process()
    assert t.n("cascade_band") == 1 and t.n("cascade_tile") == 0, t.kt
    assert seen >= 10 * 50
    b.close()
    b1, b2 = Batch(ctx, cascs, _hd(name, 0, 12)), Batch(ctx, cascs, _hd(name, 0, order=range(11, -1, -1)))
    with timed(ctx) as t:
        b1.submit(); b2.submit()
        b1.collect(); b2.collect()
    assert t.n("cascade_band") == 2 and t.n("cascade_tile") == 0, t.kt
    b1.close(); b2.close()


# ---------------------------------------------------------------- stage prefixes: candidates in (nearly) every tile cell
@pytest.mark.parametrize("k", [3, 5, 8, 12], ids=lambda k: "prefix%d" % k)
def test_prefixes_through_band(ctx, cascs, k):
    """the first k stages of the calibrated cascade on the 8 frames of test_face_batch_1080p_calibrated_cascade_vs_oracle: the
    batch is large enough for k_band without a switch"""
    b = Batch(ctx, cascs, _hd("calibrated", k))
    with timed(ctx) as t:
        seen = b.process()
    assert t.n("cascade_band") == 1 and t.n("cascade_tile") == 0 and t.n("cascade_deep") == 0, t.kt
    assert seen >= 8 * {3: 30000, 5: 6000, 8: 800, 12: 50}[k]
    b.close()


def _variants(k):
    """evaluator switches for a prefix of k stages: (options, frames, sum policy, kernel that must run, kernels that must not)"""
    return [({"band": 0}, 8, 0, "cascade_tile", ("cascade_band", "cascade_deep")),
            ({"band": 1, "deep_stage": k - 2}, 8, 0, "cascade_band", ("cascade_tile",)),
            ({"tiles": 0}, 8, 0, "cascade_strip", ("cascade_band", "cascade_tile")),
            ({"pair_max": 0}, 8, 0, "cascade_band", ("cascade_tile",)),
            ({"stage_order": 1}, 8, 0, "cascade_band", ("cascade_tile",)),
            ({"band_map": 1}, 8, 0, "cascade_band", ("cascade_tile",)),
            ({"band_map": 2}, 16, 0, "cascade_band", ("cascade_tile",)),          # the remap applies to multiples of 16 frames
            ({}, 8, 1, "cascade_band", ("cascade_tile",))]                          # SUM_F64


VARIANT_IDS = ["band=0", "deep_stage", "tiles=0", "pair_max=0", "stage_order=1", "band_map=1", "band_map=2", "sum_f64"]


@pytest.mark.parametrize("v", range(len(VARIANT_IDS)), ids=VARIANT_IDS)
@pytest.mark.parametrize("k", [5, 8], ids=lambda k: "prefix%d" % k)
def test_prefix_evaluator_switches(ctx, cascs, k, v):
    from nubovca import capi
    opts, n, policy, kernel, absent = _variants(k)[v]
    b = Batch(ctx, cascs, _hd("calibrated", k, n), policy=policy)
    ctx.set_sum_policy(policy)
    try:
        with ctx.options(**opts), timed(ctx) as t:
            b.process()
    finally:
        ctx.set_sum_policy(capi.SUM_F32PAIR)
    assert t.n(kernel) >= 1 and all(t.n(a) == 0 for a in absent), (opts, t.kt)
    # k_deep takes the stages from deep_stage on; the row strips stop in front of stage 6, which a prefix of 5 does not have
    assert (t.n("cascade_deep") > 0) == ("deep_stage" in opts or ("tiles" in opts and k > 6)), (opts, t.kt)
    b.close()


def test_prefix2_with_doubled_capacity(ctx, cascs):
    """two stages leave up to 68 521 candidates on a 1080p frame and 73 495 on an 800 x 450 one: more than the module's 65 536 a
    frame, so the lists are sized for 131 072 here"""
    ctx.set_hit_capacity(2 * P.HIT_CAP)
    try:
        for items in (_hd("calibrated", 2), [("calibrated", 2, "sd450", i) for i in range(8)]):
            b = Batch(ctx, cascs, items)
            assert P.HIT_CAP < b.cap - 64 <= 2 * P.HIT_CAP
            with ctx.options(band=1), timed(ctx) as t:
                b.process()
            assert t.n("cascade_band") == 1 and t.n("cascade_tile") == 0, t.kt
            b.close()
    finally:
        ctx.set_hit_capacity(P.HIT_CAP)


# ---------------------------------------------------------------- slots
def test_32_streams_720p(ctx, cascs):
    """BASELINE configs[3]: 32 streams of 1280 x 720 in one call, every frame different, prefix 5: a slot or plane mix-up moves
    thousands of candidates between frames"""
    b = Batch(ctx, cascs, [("calibrated", 5, "p720", s) for s in range(32)])
    with timed(ctx) as t:
        seen = b.process()
    assert t.n("cascade_band") == 1 and t.n("cascade_tile") == 0, t.kt
    assert seen >= 32 * 5000
    b.close()


# ---------------------------------------------------------------- ingest paths
@pytest.mark.parametrize("k", [5, 0], ids=["prefix5", "full"])
def test_ingest_paths(ctx, cascs, k):
    """the same expected lists for device frames, 21 host frames (chunked ingest: chunks of 8, each with its own candidate list),
    page-locked host frames, and two geometry groups of host frames interleaved in one call"""
    q360 = [("calibrated", k, "q360", i) for i in range(21)]
    q300 = [("calibrated", k, "q300", i) for i in range(18)]
    for items, mem in ((q360, "device"), (q360, "host"), ([x for pair in zip(q360, q300) for x in pair] + q360[18:], "host")):
        b = Batch(ctx, cascs, items, mem=mem)
        with timed(ctx) as t:
            b.process()
        assert t.n("cascade_band") + t.n("cascade_tile") >= 1, t.kt
        b.close()
    b = Batch(ctx, cascs, q300, mem="host")
    arrays = [f._keep for f in b.frames]
    for a in arrays:
        ctx.host_register(a)
    try:
        b.process()
    finally:
        for a in arrays:
            ctx.host_unregister(a)
    b.close()


@pytest.mark.parametrize("w2p", [160, 320])
@pytest.mark.parametrize("name", ["calibrated", "synthetic"])
def test_shrink_first_mode(ctx, cascs, name, w2p):
    """the reference's default mode on 1080p host frames (only the source rows the resize reads cross PCIe): the returned boxes
    are the raw list of the 160 x 90 / 320 x 180 working image times the integer scale"""
    b = Batch(ctx, cascs, _hd(name, 0, 12), mem="host", width_to_process=w2p)
    seen = b.process()
    assert seen >= (10 if w2p == 160 else 200)
    b.close()


# ---------------------------------------------------------------- capacity
def test_overflow_stays_loud_at_1080p(ctx, cascs):
    """test_hit_capacity_overflow_is_answered_or_loud at the real capacity of a 1080p batch: with the default 16 384 a frame a
    prefix-3 batch (280 000 candidates in 8 frames) is refused with NVCA_ERR_OVERFLOW -- never answered with a truncated list --
    and the next batch, of fresh streams, is answered in full"""
    from nubovca import capi
    ctx.set_hit_capacity(DEFAULT_HIT_CAP)
    try:
        b = Batch(ctx, cascs, _hd("calibrated", 3))
        assert sum(len(e) for e in b.exp) > 8 * DEFAULT_HIT_CAP
        with pytest.raises(capi.NvcaError) as e:
            b.process()
        assert e.value.code == capi.ERR_OVERFLOW
        b.close()
        b = Batch(ctx, cascs, _hd("calibrated", 3))
        b.process()
        b.close()
    finally:
        ctx.set_hit_capacity(P.HIT_CAP)


# ---------------------------------------------------------------- the single-slot band launch
@pytest.mark.parametrize("k", [5, 0], ids=["prefix5", "full"])
def test_detect_raw_single_image_band(ctx, cascs, k):
    """nvca_detect_raw on one 1080p image takes the per-tile kernels; band=1 sends it through k_band with one slot"""
    import orc
    f = P.frame("hd", 0)
    g = orc.equalize_hist(orc.bgr2gray(f))
    exp = P.raw_expected("calibrated", k, "hd", 0)
    with ctx.options(band=1), timed(ctx) as t:
        got = ctx.detect_raw(cascs("calibrated", k), g, 1.1, 0, (1920 // 20, 1080 // 20))
    assert t.n("cascade_band") >= 1 and t.n("cascade_tile") == 0, t.kt
    assert np.array_equal(got, exp), (len(got), len(exp), P.first_difference(got, exp))
    assert len(exp) > 50
