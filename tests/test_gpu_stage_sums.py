"""GPU parity on cascades whose stage sums depend on the summation order and whose stage thresholds sit on the vote grid
(tests/stage_sum_cascades.py): every evaluator path -- the order-free rounds and accumulators where plan.cpp proves them exact,
OpenCV's left-to-right sum where it does not, the tie rule !(sum < thr) in every compare -- against the CPU oracle, bit for bit,
raw candidate lists in order and grouped boxes.  tests/test_stage_sums_cpu.py shows on the oracle that these cascades change
the raw lists when their stages are summed in another order or their ties break the other way."""
import functools

import numpy as np
import pytest

import stage_sum_cascades as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from nubovca import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cascades(ctx):
    import orc
    out = {}
    for n in S.NAMES:
        xml = S.variant(n)[0]
        out[n] = (ctx.load_cascade_xml(xml), orc.parse_cascade_xml(xml))
    return out


@functools.lru_cache(maxsize=None)
def _images():
    return S.images()


@functools.lru_cache(maxsize=None)
def _oracle(name, k, flags, policy, grouped):
    import orc
    oc = orc.parse_cascade_xml(S.variant(name)[0])
    g = _images()[k]
    if grouped:
        return orc.detect_multiscale(oc, g, 1.1, 3, flags, (0, 0), policy=policy)
    return orc.detect_raw(oc, g, 1.1, flags, (0, 0), policy=policy)


class timed:
    """the context's kernel launches inside a with-block (name -> launches)"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.enable_kernel_timing(1)          # (re)starts the counts
        return self

    def __exit__(self, *exc):
        self.kt = {k: v[1] for k, v in self.ctx.kernel_timing().items()}
        self.ctx.enable_kernel_timing(0)


def _compare(ctx, cascades, name, k, flags, policy, raw=True):
    from nubovca import capi
    dc = cascades[name][0]
    g = _images()[k]
    ctx.set_sum_policy(policy)
    try:
        if raw:
            got, exp = ctx.detect_raw(dc, g, 1.1, flags, (0, 0)), _oracle(name, k, flags, policy, False)
            assert np.array_equal(got, exp), (name, k, flags, policy, len(got), len(exp))
            assert len(exp) > 0
        got, exp = ctx.detect_multiscale(dc, g, 1.1, 3, flags, (0, 0)), _oracle(name, k, flags, policy, True)
        assert np.array_equal(got, exp), (name, k, flags, policy, got, exp)
    finally:
        ctx.set_sum_policy(capi.SUM_F32PAIR)


POLICIES = [0, 1]          # capi.SUM_F32PAIR, capi.SUM_F64


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("flags", [0, 2, 4])     # 0, HAAR_SCALE_IMAGE, HAAR_FIND_BIGGEST_OBJECT
@pytest.mark.parametrize("name", S.NAMES)
def test_scan_variants(ctx, cascades, name, flags, policy):
    with timed(ctx) as t:
        for k in range(len(S.IMAGES)):
            _compare(ctx, cascades, name, k, flags, policy, raw=flags != 4)
    assert t.kt.get("cascade_tile", 0) + t.kt.get("cascade_band", 0) + t.kt.get("cascade_roi", 0) > 0, t.kt


# evaluator switches (ctx.options) and the kernel each one must reach; the default plan walks the whole cascade on the tiles
SWITCHES = [({}, "cascade_tile"), ({"band": 1}, "cascade_band"), ({"tiles": 0}, "cascade_strip"),
            ({"deep_stage": 1}, "cascade_deep"), ({"deep_stage": 2}, "cascade_deep"), ({"deep_stage": 30}, "cascade_tile"),
            ({"tiles": 0, "deep_stage": 30}, "cascade_strip"), ({"band": 1, "deep_stage": 30}, "cascade_band"),
            ({"band": 1, "deep_stage": 2}, "cascade_deep"), ({"deep_lds": 0, "deep_stage": 2}, "cascade_deep"),
            ({"deep_stage": 20}, "cascade_tile"), ({"deep_stage": 7}, "cascade_deep"), ({"pair_max": 0}, "cascade_tile"),
            ({"stage_order": 1}, "cascade_tile"), ({"band": 1, "pair_max": 0}, "cascade_band")]


@pytest.mark.parametrize("opts,kernel", SWITCHES, ids=[",".join("%s=%d" % kv for kv in o.items()) or "default" for o, _ in SWITCHES])
@pytest.mark.parametrize("name", S.NAMES)
def test_evaluator_switches(ctx, cascades, name, opts, kernel):
    with ctx.options(**opts), timed(ctx) as t:
        for policy in POLICIES:
            _compare(ctx, cascades, name, 1, 0, policy)
    assert t.kt.get(kernel, 0) > 0, (opts, t.kt)


@pytest.mark.parametrize("roi", [1, 0])
def test_small_images(ctx, cascades, roi):
    """the one-launch small-image detector (k_roi, roi=1) and the large-image path on the same small images (roi=0): random
    sizes 21 .. 200 pixels as in test_small_image_path_random_geometries, every scan variant, both sum policies"""
    import orc
    from nubovca import capi, synth
    rng = np.random.RandomState(5)
    hits = 0
    with ctx.options(roi=roi), timed(ctx) as t:
        for it in range(24):
            name = S.NAMES[it % len(S.NAMES)]
            dc, oc = cascades[name]
            w = int(rng.randint(21, 200))
            h = int(rng.randint(21, min(200, 10240 // (w + 1) - 2) + 1))
            s = int(min(w, h) * rng.uniform(0.4, 0.9))
            faces = [(int(rng.randint(0, max(1, w - s))), int(rng.randint(0, max(1, h - s))), s)] if s >= 24 else []
            g = orc.equalize_hist(synth.make_gray(w, h, 5000 + it, "natural", faces))
            pol = it % 2
            ctx.set_sum_policy(pol)
            try:
                for fl in (0, capi.HAAR_SCALE_IMAGE):
                    got, exp = ctx.detect_raw(dc, g, 1.1, fl, (0, 0)), orc.detect_raw(oc, g, 1.1, fl, (0, 0), policy=pol)
                    assert np.array_equal(got, exp), (it, name, w, h, fl, len(got), len(exp))
                    hits += len(exp)
                for fl in (0, capi.HAAR_SCALE_IMAGE, capi.HAAR_FIND_BIGGEST_OBJECT):
                    got, exp = ctx.detect_multiscale(dc, g, 1.1, 2, fl, (0, 0)), orc.detect_multiscale(oc, g, 1.1, 2, fl, (0, 0), policy=pol)
                    assert np.array_equal(got, exp), (it, name, w, h, fl)
            finally:
                ctx.set_sum_policy(capi.SUM_F32PAIR)
    assert hits > 0
    if roi:
        assert t.kt.get("cascade_roi", 0) >= 24 * 3, t.kt
    else:
        assert "cascade_roi" not in t.kt and t.kt.get("cascade_tile", 0) + t.kt.get("cascade_strip", 0) + t.kt.get("cascade_band", 0) > 0, t.kt


def test_face_batch_1080p(ctx, calibrated_xml):
    """the calibrated headline cascade with one order-sensitive late stage and one vote-grid stage: 8 full-resolution 1080p
    frames in one batched call against the oracle's face streams"""
    import orc
    from nubovca import capi, synth
    xml = S.face_variant(calibrated_xml)
    dc, oc = ctx.load_cascade_xml(xml), orc.parse_cascade_xml(xml)
    W, H = 1920, 1080
    frames = [synth.make_bgr(W, H, synth.frame_seed(s, 0), "natural", [(300 + 40 * s, 200, 240 + 8 * s), (1200, 500 - 20 * s, 160)])
              for s in range(8)]
    props = {"width_to_process": W, "multi_scale_factor": 10}
    streams = [capi.FaceStream(ctx, dc, **props) for _ in frames]
    with timed(ctx) as t:
        res = ctx.face_batch_process(streams, [capi.make_frame(f) for f in frames])
    seen = 0
    for f, (boxes, ids) in zip(frames, res):
        eb, eid = orc.FaceStream(oc, width_to_process=W, scale_factor_pct=10).process(f)
        assert np.array_equal(boxes, eb) and np.array_equal(ids, eid), (boxes, eb)
        seen += len(eb)
    assert seen > 0
    assert t.kt.get("cascade_band", 0) + t.kt.get("cascade_tile", 0) > 0, t.kt
    for s in streams:
        s.close()


@pytest.mark.parametrize("variant", ["order", "tie"])
@pytest.mark.parametrize("kind", ["eye", "nose"])
def test_part_streams(ctx, synth_xml, kind, variant):
    """NuboEyeDetector / NuboNoseDetector streams whose part cascades carry an order-sensitive stage or vote-grid thresholds"""
    import orc
    from nubovca import capi, synth
    names = S.PART_KINDS[kind]
    dev = [ctx.load_cascade_xml(S.part_variant(n, variant)[0]) for n in names]
    cpu = [orc.parse_cascade_xml(S.part_variant(n, variant)[0]) for n in names]
    dface, oface = ctx.load_cascade_xml(synth_xml), orc.parse_cascade_xml(synth_xml)
    k = {"eye": 0, "nose": 1}[kind]
    g = capi.PartStream(ctx, k, dface, dev[0], dev[1] if len(dev) > 1 else None)
    o = orc.PartStream(k, oface, cpu[0], cpu[1] if len(cpu) > 1 else None)
    W, H = 640, 480
    faces_seen = 0
    for i in range(6):
        f = synth.make_bgr(W, H, 900 + i, "natural", [(W // 5 + 7 * i, H // 5, int(H * 0.5))])
        ga, gb = g.process(f)
        ea, eb = o.process(f)
        assert np.array_equal(ga, ea) and np.array_equal(gb, eb), (kind, variant, i, ga, ea, gb, eb)
        faces_seen += len(ea) + len(eb)
    g.close()
    assert faces_seen > 0
