"""General new-format HAAR cascades on the device -- tree weak classifiers and tilted features, loaded with NVCA_LOAD_HAAR_GENERAL
(csrc/kernels_cascade_hgen.hip around kernels_cascade_lbp.hip's walk kernel, lbp_job.cpp's plan and launch set on hgen_tables.cpp's
tables) -- against the numpy statement of SURVEY.md A.19 (tests/haar_tree_reference.py): bit for bit, no tolerance anywhere.  The cases
and the hand-derived lists are tests/haar_tree_cases.py's; tests/test_haar_tree_cpu.py asserts on the statement alone that they are
not empty comparisons and reach the branches they are meant to reach."""
import ctypes as C
import os

import numpy as np
import pytest

import haar_new_cases as HK
import haar_tree_cases as K
import haar_tree_reference as R
import lbp_cases as LK
import lbp_part_cases as LP
import lbp_stream_cases as LS
import orc
from nubovca import capi, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newformat_trees_tilted_20x20.xml.txt")
CAP = 1024


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def loaded(ctx):
    """name -> the device's cascade, loaded once with the flag"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ctx.load_cascade_xml(K.cascade(name)[0], general=True)
        return cache[name]
    return get


def _raw(ctx, casc, gray, sf):
    return np.asarray(ctx.detect_raw(casc, gray, sf), np.int32).reshape(-1, 4)


def _grouped(ctx, casc, gray, sf, mn):
    return np.asarray(ctx.detect_multiscale(casc, gray, sf, mn, cap=1 << 16), np.int32).reshape(-1, 4)


def _expected_grouped(raw, mn):
    if mn == 0 or len(raw) == 0:
        return raw
    return np.asarray(orc.group_rectangles(raw, max(mn, 1), 0.2)[0], np.int32).reshape(-1, 4)


def _hand(ctx, cdict, gray, sf):
    casc = ctx.load_cascade_xml(synth.haar_tree_cascade_to_xml(cdict), general=True)
    try:
        return _raw(ctx, casc, gray, sf).tolist()
    finally:
        casc.free()


def _booked(ctx, fn):
    ctx.enable_kernel_timing(True)
    try:
        ctx.kernel_timing()
        out = fn()
        return out, {k: v[1] for k, v in ctx.kernel_timing().items()}
    finally:
        ctx.enable_kernel_timing(False)


# ------------------------------------------------------------------ loader
@pytest.mark.parametrize("style", ["traincascade", "minimal"])
def test_tree_dump_is_the_reference_readers(ctx, style):
    xml, ref = K.cascade("deep4", style)
    casc = ctx.load_cascade_xml(xml, general=True)
    d, e = casc.dump_haar_tree(), ref.arrays()
    assert d["size"] == e["size"]
    for k in R.HaarTreeCascade.KEYS:
        assert d[k].dtype == e[k].dtype and np.array_equal(d[k], e[k]), k
    assert casc.format() == (capi.CASCADE_HAAR_NEW, len(ref.rects))
    assert casc.info() == (20, 20, len(ref.stage_sizes), len(ref.node_counts))
    assert casc.tree_info() == (len(ref.nodes), len(ref.leaves), True) and casc.kind() == (True, True)
    for dump in (casc.dump, casc.dump_lbp, casc.dump_haar_new):
        with pytest.raises(capi.NvcaError) as ei:
            dump()
        assert ei.value.code == capi.ERR_ARG
    casc.free()


def test_plain_load_still_refuses_and_flags_are_checked(ctx):
    xml = K.cascade("t20")[0]
    for load in (lambda: ctx.load_cascade_xml(xml), lambda: ctx.load_cascade_xml(xml, flags=0)):
        with pytest.raises(capi.NvcaError) as ei:
            load()
        assert ei.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.NvcaError) as ei:
        ctx.load_cascade_xml(xml, flags=3)
    assert ei.value.code == capi.ERR_ARG
    with pytest.raises(capi.NvcaError) as ei:
        ctx.load_cascade_file(GOLDEN, flags=2)
    assert ei.value.code == capi.ERR_ARG


def test_golden_file_loads_from_disk_and_scans_as_the_statement(ctx):
    ref = R.parse_xml(open(GOLDEN).read())
    with pytest.raises(capi.NvcaError) as ei:
        ctx.load_cascade_file(GOLDEN)
    assert ei.value.code == capi.ERR_UNSUPPORTED
    casc = ctx.load_cascade_file(GOLDEN, general=True)
    d, e = casc.dump_haar_tree(), ref.arrays()
    for k in R.HaarTreeCascade.KEYS:
        assert np.array_equal(d[k], e[k]), k
    assert casc.info() == (20, 20, 2, 5) and casc.kind() == (True, True)
    gray = K.image(97, 83, 20, 20)
    exp = R.scan(ref, gray, 1.1)
    assert len(exp) > 0 and np.array_equal(_raw(ctx, casc, gray, 1.1), exp)
    casc.free()


def test_other_formats_take_the_flag_and_stay_what_they_are(ctx, synth_xml):
    for xml, fmt in ((synth_xml, capi.CASCADE_HAAR), (LK.cascade("w12")[0], capi.CASCADE_LBP)):
        casc = ctx.load_cascade_xml(xml, general=True)
        assert casc.format()[0] == fmt
        for call in (casc.dump_haar_tree, casc.tree_info):
            with pytest.raises(capi.NvcaError) as ei:
                call()
            assert ei.value.code == capi.ERR_ARG
        casc.free()


# ------------------------------------------------------------------ the hand-made cases of tests/test_haar_tree_cpu.py
HAND = K.tilted_cases() + K.tree_cases()


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made_windows(ctx, case):
    _, cdict, gray, exp = case
    assert _hand(ctx, cdict, gray, 2.0) == exp


@pytest.mark.parametrize("case", K.skip_cases(), ids=[c[0] for c in K.skip_cases()])
def test_a_tree_in_stage_0_and_the_skip_rule(ctx, case):
    _, cdict, exp = case
    assert _hand(ctx, cdict, LK.column_image(), 4.0) == exp


# ------------------------------------------------------------------ raw lists and grouped boxes
@pytest.mark.parametrize("name", list(K.CASCADES))
def test_raw_list_and_grouped_boxes(ctx, loaded, name):
    """t20, t24: the LDS form of stage 0; w82: (63 + 82) (31 + 82) words do not fit 64 KiB, stage 0 gathers; deep4: trees of up to 7 nodes"""
    cols, rows, sf = K.IMAGES[name]
    ref = K.cascade(name)[1]
    assert ((63 + ref.size[0]) * (31 + ref.size[1]) * 4 > 65536) == (name == "w82")
    gray = K.image(cols, rows, *ref.size)
    exp = K.expected_raw(name, cols, rows, sf)
    got = _raw(ctx, loaded(name), gray, sf)
    assert got.shape == exp.shape and np.array_equal(got, exp)
    for mn in (0, 2, 3):
        assert np.array_equal(_grouped(ctx, loaded(name), gray, sf, mn), _expected_grouped(exp, mn)), mn


def test_a_level_wider_than_1023_takes_the_per_level_pyramid(ctx, loaded):
    name, cols, rows, sf = K.WIDE
    exp = K.expected_raw(name, cols, rows, sf)
    assert len(exp) >= 20 and np.array_equal(_raw(ctx, loaded(name), K.image(cols, rows, 20, 20), sf), exp)


def test_host_images_device_images_and_a_padded_sub_matrix(ctx, loaded):
    import torch
    cols, rows, sf = K.IMAGES["t24"]                   # 199 x 149: odd pitch
    gray = K.image(cols, rows, 24, 24)
    exp = K.expected_raw("t24", cols, rows, sf)
    L, cap = ctx.L, 1 << 16
    for stride in (cols, cols + 19):
        host = np.full((rows, stride), 201, np.uint8)
        host[:, :cols] = gray
        dev = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        for mem, ptr in ((capi.MEM_HOST, host.ctypes.data), (capi.MEM_DEVICE, dev.data_ptr())):
            buf, n = (capi.Rect * cap)(), C.c_int()
            ctx.check(L.nvca_detect_raw(ctx.h, loaded("t24").h, ptr, cols, rows, stride, mem, sf, 0, 0, 0, 0, 0, buf, cap, C.byref(n)))
            got = np.frombuffer(buf, np.int32).reshape(-1, 4)[:n.value]
            assert n.value == len(exp) and np.array_equal(got, exp), (stride, mem)
            ctx.check(L.nvca_detect_multiscale(ctx.h, loaded("t24").h, ptr, cols, rows, stride, mem, sf, 3, 0, 0, 0, 0, 0, buf, cap, C.byref(n)))
            got = np.frombuffer(buf, np.int32).reshape(-1, 4)[:n.value]
            assert np.array_equal(got, _expected_grouped(exp, 3)), (stride, mem)


@pytest.mark.parametrize("n", [2, 33])
def test_batches_in_slot_order_and_reversed(ctx, loaded, n):
    name, cols, rows, sf = K.BATCH
    ref = K.cascade(name)[1]
    grays = [K.image(cols, rows, *ref.size, 100 + i % 4) for i in range(n)]
    exp = [K.expected_raw(name, cols, rows, sf, 100 + i % 4) for i in range(n)]
    for order in (list(range(n)), list(range(n))[::-1]):
        raw = ctx.detect_raw_batch(loaded(name), [grays[i] for i in order], sf)
        grp = ctx.detect_multiscale_batch(loaded(name), [grays[i] for i in order], sf, 2)
        for slot, i in enumerate(order):
            assert np.array_equal(raw[slot], exp[i]), (slot, i)
            assert np.array_equal(grp[slot], _expected_grouped(exp[i], 2)), (slot, i)


def test_candidate_overflow_rerun_answers_exactly(ctx):
    cols, rows, sf = 160, 120, 1.2
    gray = K.image(cols, rows, 24, 24)
    xml = synth.haar_tree_cascade_to_xml(K.permissive_general(24, 24))
    casc = ctx.load_cascade_xml(xml, general=True)
    assert casc.tree_info()[2]
    exp = R.scan(R.parse_xml(xml), gray, sf)
    assert len(exp) > 3000
    ctx.set_hit_capacity(256)
    try:
        assert np.array_equal(_raw(ctx, casc, gray, sf), exp)
        assert np.array_equal(_grouped(ctx, casc, gray, sf, 3), _expected_grouped(exp, 3))
    finally:
        ctx.set_hit_capacity(16384)
        casc.free()


def test_reject_levels_and_weights_as_exact_doubles(ctx, loaded):
    name, cols, rows, sf = K.LEVELS
    ref = K.cascade(name)[1]
    gray = K.image(cols, rows, *ref.size)
    er, el, ew = R.scan_levels(ref, gray, sf)
    gr, gl, gw = ctx.detect_raw_levels(loaded(name), gray, sf)
    assert len(er) > 0 and np.array_equal(gr, er) and np.array_equal(gl, el)
    assert gw.dtype == np.float64 and np.array_equal(gw.view(np.uint64), ew.view(np.uint64))          # the same bits


# ------------------------------------------------------------------ streams
def _stream(ctx, casc, wtp=160, pct=25, mn=3):
    return capi.FaceStream(ctx, casc, any_format=True, width_to_process=wtp, multi_scale_factor=pct, min_neighbors=mn, process_x_every_4_frames=4)


def _eq(got, exp, what):
    assert got[0].shape == exp[0].shape and np.array_equal(got[0], exp[0]), (what, got[0].tolist(), exp[0].tolist())
    assert np.array_equal(got[1], exp[1]), (what, got[1].tolist(), exp[1].tolist())


def test_face_stream_with_a_stump_stream_and_an_lbp_stream_in_one_call(ctx, loaded):
    import haar_new_stream_cases as HS
    name, _W, _H, wtp, pct, _ = K.STREAM
    ft, fh, fl = K.stream_frames(), HS.frames_of(HS.CASES["identity"]), LS.frames_of(LS.CASES["identity"])
    stump = ctx.load_cascade_xml(HK.cascade("w24")[0])
    lbp = ctx.load_cascade_xml(LS.cascade("w24")[0])
    streams = [_stream(ctx, loaded(name), wtp, pct), _stream(ctx, stump), _stream(ctx, lbp)]
    expected = [K.Expected(name, 0, wtp, pct), HS.Expected("w24", 0, width_to_process=160, scale_factor_pct=25, min_neighbors=3, process_x_every_4=4),
                LS.Expected("w24", 0, width_to_process=160, scale_factor_pct=25, min_neighbors=3, process_x_every_4=4)]
    seen = 0
    for r in range(3):
        frames = [capi.make_frame(np.array(K.stream_bgr(ft[r]))), capi.make_frame(np.array(HS.bgr(fh[r]))), capi.make_frame(np.array(LS.bgr(fl[r])))]
        keys = [ft[r], fh[r], fl[r]]
        order = [0, 1, 2][::1 if r % 2 == 0 else -1]
        res = ctx.face_batch_process([streams[i] for i in order], [frames[i] for i in order], CAP)
        for slot, i in enumerate(order):
            e = expected[i].process(keys[i])
            seen += len(e[0]) if i == 0 else 0
            _eq(res[slot], e, ("mixed", r, i))
    assert seen > 0
    stump.free()
    lbp.free()


def test_nv12_stream(ctx, loaded):
    name, _W, _H, wtp, pct, _ = K.STREAM
    frames = K.stream_frames()
    fs, ex = _stream(ctx, loaded(name), wtp, pct), K.Expected(name, capi.PIX_NV12, wtp, pct)
    lay = capi.pixel_layout(*K.stream_yuv(frames[0], capi.PIX_NV12)[1])
    fs.set_input(lay)
    for r, f in enumerate(frames):
        e = ex.process(f)
        assert r > 0 or len(e[0]) > 0
        res = ctx.face_batch_process([fs], [capi.make_planar_frame(np.array(K.stream_yuv(f, capi.PIX_NV12)[0]), 160, 120, lay)], CAP)
        _eq(res[0], e, ("nv12", r))


@pytest.mark.skipif(LP.shim() is None, reason="no clang++")
def test_part_stream_with_a_general_cascade_in_a_part_role(ctx):
    exp, dets = K.part_expected()
    assert all(len(d.seen) > 0 for d in dets) and sum(len(b) for a, b in exp) > 0
    xmls = K.part_xmls()
    cascs = [ctx.load_cascade_xml(xmls[0]), ctx.load_cascade_xml(xmls[1]), ctx.load_cascade_xml(xmls[2], general=True)]
    s = capi.PartStream(ctx, LP.KINDS["ear"], cascs[0], cascs[1], cascs[2], any_format=True)
    try:
        for i, f in enumerate(LP.lbp_frames(K.PART_W, K.PART_H)):
            got = s.process(f, cap=256)
            assert np.array_equal(got[0], exp[i][0]) and np.array_equal(got[1], exp[i][1]), (i, got[0].tolist(), exp[i][0].tolist(), got[1].tolist(), exp[i][1].tolist())
    finally:
        s.close()


# ------------------------------------------------------------------ what the flag must not change, and the small route
def test_a_stump_file_is_the_same_cascade_with_and_without_the_flag(ctx):
    xml = K.stump_xml()
    plain, flagged = ctx.load_cascade_xml(xml), ctx.load_cascade_xml(xml, general=True)
    assert flagged.tree_info() == plain.tree_info() and not flagged.tree_info()[2] and flagged.kind() == (False, False)
    dp, df = plain.dump_haar_new(), flagged.dump_haar_new()
    assert all(np.array_equal(dp[k], df[k]) for k in dp if k != "size")
    t = flagged.dump_haar_tree()
    assert t["node_counts"].tolist() == [1] * len(dp["thr"]) and np.array_equal(t["nodes"][:, :2], np.tile([0, -1], (len(dp["thr"]), 1)))
    assert np.array_equal(t["leaves"].reshape(-1, 2), dp["leaves"]) and np.array_equal(t["node_thr"], dp["thr"]) and not t["tilted"].any()
    cols, rows, sf = HK.IMAGES[1]
    gray = HK.image(cols, rows, 24, 24)
    exp = HK.expected_raw("w24", cols, rows, sf)
    (a, ba), (b, bb) = _booked(ctx, lambda: _raw(ctx, plain, gray, sf)), _booked(ctx, lambda: _raw(ctx, flagged, gray, sf))
    assert np.array_equal(a, exp) and np.array_equal(b, exp) and ba == bb and "cascade_roi" not in bb
    # ... and it stays eligible for the small route: a 97 x 83 image is one cascade_roi launch once it is opted in
    flagged.set_small_route(True)
    assert flagged.small_route()
    small = HK.image(97, 83, 24, 24)
    got, booked = _booked(ctx, lambda: _raw(ctx, flagged, small, 1.1))
    assert np.array_equal(got, HK.expected_raw("w24", 97, 83, 1.1)) and booked.get("cascade_roi", 0) >= 1
    plain.free()
    flagged.free()


def test_set_small_route_changes_nothing_on_a_general_cascade(ctx, loaded):
    casc = loaded("t24")
    casc.set_small_route(True)          # NVCA_OK
    assert not casc.small_route()
    ref = K.cascade("t24")[1]
    gray = K.image(97, 83, 24, 24)
    got, booked = _booked(ctx, lambda: _raw(ctx, casc, gray, 1.1))
    exp = R.scan(ref, gray, 1.1)
    assert len(exp) > 0 and np.array_equal(got, exp)
    assert "cascade_roi" not in booked and booked["cascade_strip"] >= 1
