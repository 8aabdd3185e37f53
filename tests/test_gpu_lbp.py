"""New-format LBP cascades on the device (csrc/kernels_cascade_lbp.hip, lbp_job.cpp's lbp_plan / lbp_enqueue on lbp_tables.cpp's
tables) against the numpy statement of SURVEY.md A.15 (tests/lbp_reference.py): bit for bit, raw lists and grouped boxes.  The cases and the hand-derived
lists are tests/lbp_cases.py's; tests/test_lbp_cpu.py asserts on the statement alone that they are not empty comparisons."""
import ctypes as C
import os

import numpy as np
import pytest

import lbp_cases as K
import lbp_reference as R
import orc
from nubovca import capi, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newformat_lbp_24x24.xml.txt")
FLAGS = (capi.HAAR_DO_CANNY_PRUNING, capi.HAAR_SCALE_IMAGE, capi.HAAR_FIND_BIGGEST_OBJECT, capi.HAAR_DO_ROUGH_SEARCH,
         capi.HAAR_FIND_BIGGEST_OBJECT | capi.HAAR_DO_ROUGH_SEARCH, 15)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def loaded(ctx):
    """name -> the device's cascade, loaded once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ctx.load_cascade_xml(K.cascade(name)[0])
        return cache[name]
    return get


def _raw(ctx, casc, gray, sf, flags=0, min_size=(0, 0), max_size=(0, 0)):
    return np.asarray(ctx.detect_raw(casc, gray, sf, flags, min_size, max_size), np.int32).reshape(-1, 4)


def _grouped(ctx, casc, gray, sf, mn, flags=0, min_size=(0, 0), max_size=(0, 0)):
    return np.asarray(ctx.detect_multiscale(casc, gray, sf, mn, flags, min_size, max_size, cap=1 << 16), np.int32).reshape(-1, 4)


def _expected_grouped(raw, mn):
    if mn == 0 or len(raw) == 0:
        return raw
    return np.asarray(orc.group_rectangles(raw, max(mn, 1), 0.2)[0], np.int32).reshape(-1, 4)


def _hand(ctx, cdict, gray, sf, min_size=(0, 0), max_size=(0, 0)):
    casc = ctx.load_cascade_xml(synth.lbp_cascade_to_xml(cdict))
    try:
        return _raw(ctx, casc, gray, sf, 0, min_size, max_size).tolist()
    finally:
        casc.free()


# ------------------------------------------------------------------ loader
@pytest.mark.parametrize("style", ["traincascade", "minimal"])
def test_dump_lbp_is_the_reference_readers(ctx, style):
    xml, ref = K.cascade("w24", style)
    casc = ctx.load_cascade_xml(xml)
    d, e = casc.dump_lbp(), ref.arrays()
    assert d["size"] == e["size"]
    for k in ("rects", "feature_idx", "subsets", "leaves", "stage_sizes", "stage_thr"):
        assert d[k].dtype == e[k].dtype and np.array_equal(d[k], e[k]), k
    assert casc.format() == (capi.CASCADE_LBP, len(ref.rects))
    assert casc.info() == (24, 24, len(ref.stage_sizes), len(ref.feature_idx))
    assert casc.kind() == (False, False)
    with pytest.raises(capi.NvcaError) as ei:
        casc.dump()
    assert ei.value.code == capi.ERR_ARG
    casc.free()


def test_golden_file_loads_from_disk_and_dumps_as_read(ctx):
    ref = R.parse_xml(open(GOLDEN).read())
    casc = ctx.load_cascade_file(GOLDEN)
    d, e = casc.dump_lbp(), ref.arrays()
    for k in ("rects", "feature_idx", "subsets", "leaves", "stage_sizes", "stage_thr"):
        assert np.array_equal(d[k], e[k]), k
    assert casc.format() == (capi.CASCADE_LBP, 6) and casc.info() == (24, 24, 3, 9)
    casc.free()


def test_old_format_cascade_reports_haar_and_refuses_dump_lbp(ctx, synth_xml):
    casc = ctx.load_cascade_xml(synth_xml)
    assert casc.format() == (capi.CASCADE_HAAR, 0)
    with pytest.raises(capi.NvcaError) as ei:
        casc.dump_lbp()
    assert ei.value.code == capi.ERR_ARG
    casc.free()


# ------------------------------------------------------------------ raw lists and grouped boxes
RAW_CASES = [("w24",) + im for im in K.IMAGES] + [(n,) + im for n in ("w20x28", "w12") for im in K.SMALL_IMAGES]


@pytest.mark.parametrize("name,cols,rows,sf", RAW_CASES, ids=["%s-%dx%d" % c[:3] for c in RAW_CASES])
def test_raw_list_and_grouped_boxes(ctx, loaded, name, cols, rows, sf):
    ref = K.cascade(name)[1]
    gray = K.image(cols, rows, *ref.size)
    exp = K.expected_raw(name, cols, rows, sf)
    got = _raw(ctx, loaded(name), gray, sf)
    assert got.shape == exp.shape and np.array_equal(got, exp)
    for mn in (0, 2, 3):
        assert np.array_equal(_grouped(ctx, loaded(name), gray, sf, mn), _expected_grouped(exp, mn)), mn


def test_one_window_permissive(ctx):
    assert _hand(ctx, K.permissive(24, 24), np.full((25, 25), 77, np.uint8), 1.1) == [[0, 0, 24, 24]]


def test_host_group_switch_gives_the_same_boxes(ctx, loaded):
    cols, rows, sf = K.IMAGES[1]
    gray = K.image(cols, rows, 24, 24)
    exp = K.expected_raw("w24", cols, rows, sf)
    for hg in (0, 1):
        with ctx.options(host_group=hg):
            for mn in (0, 2, 3):
                assert np.array_equal(_grouped(ctx, loaded("w24"), gray, sf, mn), _expected_grouped(exp, mn)), (hg, mn)


def test_device_images_and_a_padded_stride(ctx, loaded):
    import torch
    cols, rows, sf = K.IMAGES[2]                   # 333 x 251: odd pitch
    gray = K.image(cols, rows, 24, 24)
    exp = K.expected_raw("w24", cols, rows, sf)
    L, cap = ctx.L, 1 << 16
    for stride in (cols, cols + 19):
        host = np.full((rows, stride), 201, np.uint8)
        host[:, :cols] = gray
        dev = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        for mem, ptr in ((capi.MEM_HOST, host.ctypes.data), (capi.MEM_DEVICE, dev.data_ptr())):
            buf, n = (capi.Rect * cap)(), C.c_int()
            ctx.check(L.nvca_detect_raw(ctx.h, loaded("w24").h, ptr, cols, rows, stride, mem, sf, 0, 0, 0, 0, 0, buf, cap, C.byref(n)))
            got = np.frombuffer(buf, np.int32).reshape(-1, 4)[:n.value]
            assert n.value == len(exp) and np.array_equal(got, exp), (stride, mem)
            ctx.check(L.nvca_detect_multiscale(ctx.h, loaded("w24").h, ptr, cols, rows, stride, mem, sf, 3, 0, 0, 0, 0, 0, buf, cap, C.byref(n)))
            got = np.frombuffer(buf, np.int32).reshape(-1, 4)[:n.value]
            assert np.array_equal(got, _expected_grouped(exp, 3)), (stride, mem)


def test_min_and_max_size_cut_levels_at_both_ends(ctx, loaded):
    cols, rows, sf = K.IMAGES[2]
    gray = K.image(cols, rows, 24, 24)
    full = K.expected_raw("w24", cols, rows, sf)
    for mins, maxs in (((30, 30), (0, 0)), ((0, 0), (60, 60)), ((30, 30), (60, 60))):
        exp = K.expected_raw("w24", cols, rows, sf, mins, maxs)
        assert 0 < len(exp) < len(full)
        assert np.array_equal(_raw(ctx, loaded("w24"), gray, sf, 0, mins, maxs), exp), (mins, maxs)
        assert np.array_equal(_grouped(ctx, loaded("w24"), gray, sf, 2, 0, mins, maxs), _expected_grouped(exp, 2)), (mins, maxs)


def test_every_flags_value_answers_as_zero(ctx, loaded):
    cols, rows, sf = K.IMAGES[0]
    gray = K.image(cols, rows, 24, 24)
    exp = K.expected_raw("w24", cols, rows, sf)
    for fl in FLAGS:
        assert np.array_equal(_raw(ctx, loaded("w24"), gray, sf, fl), exp), fl
        assert np.array_equal(_grouped(ctx, loaded("w24"), gray, sf, 3, fl), _expected_grouped(exp, 3)), fl


# ------------------------------------------------------------------ the constructed cascades of tests/test_lbp_cpu.py
def test_code_bits_ties_and_subset_words(ctx):
    cases = K.code_cases()
    for cid, gray, code in cases:
        assert _hand(ctx, K.code_cascade([code]), gray, 2.0) == K.ONE_WINDOW, cid
        assert _hand(ctx, K.code_cascade([c for c in range(256) if c != code]), gray, 2.0) == [], cid


def test_vote_order(ctx):
    gray = np.full((4, 4), 90, np.uint8)
    assert _hand(ctx, K.vote_order_cascade("big-one-minus"), gray, 2.0) == []
    assert _hand(ctx, K.vote_order_cascade("big-minus-one"), gray, 2.0) == K.ONE_WINDOW


@pytest.mark.parametrize("case", K.skip_cases(), ids=[c[0] for c in K.skip_cases()])
def test_skip_columns(ctx, case):
    _, cdict, exp = case
    assert _hand(ctx, cdict, K.column_image(), 4.0) == exp


@pytest.mark.parametrize("case", K.scan_rule_cases(), ids=[c[0] for c in K.scan_rule_cases()])
def test_scan_rules(ctx, case):
    _, cdict, shape, sf, mins, maxs, exp = case
    assert _hand(ctx, cdict, np.full(shape, 120, np.uint8), sf, mins, maxs) == exp


# ------------------------------------------------------------------ long cascade, overflow, refusals, mixing
def test_stage_heavy_cascade(ctx, loaded):
    cols, rows, sf = K.IMAGES[2]
    gray = K.image(cols, rows, 24, 24)
    exp = K.expected_raw("deep", cols, rows, sf)
    assert np.array_equal(_raw(ctx, loaded("deep"), gray, sf), exp)
    assert np.array_equal(_grouped(ctx, loaded("deep"), gray, sf, 3), _expected_grouped(exp, 3))


def test_candidate_overflow_rerun_answers_exactly(ctx):
    cols, rows, sf = K.IMAGES[1]
    gray = K.image(cols, rows, 24, 24)
    casc = ctx.load_cascade_xml(synth.lbp_cascade_to_xml(K.permissive(24, 24)))
    ref = R.parse_xml(synth.lbp_cascade_to_xml(K.permissive(24, 24)))
    exp = R.scan(ref, gray, sf)
    assert len(exp) > 3000
    ctx.set_hit_capacity(256)
    try:
        assert np.array_equal(_raw(ctx, casc, gray, sf), exp)
        assert np.array_equal(_grouped(ctx, casc, gray, sf, 3), _expected_grouped(exp, 3))
    finally:
        ctx.set_hit_capacity(16384)
        casc.free()


def test_streams_refuse_an_lbp_cascade_in_every_role(ctx, loaded, synth_xml, orc_cascade):
    haar = ctx.load_cascade_xml(synth_xml)
    lbp = loaded("w24")
    L = ctx.L
    h = C.c_void_p()
    assert L.nvca_face_stream_create(ctx.h, lbp.h, None, C.byref(h)) == capi.ERR_UNSUPPORTED and L.nvca_last_error(ctx.h)
    p = capi.PartParams()
    L.nvca_part_params_default(C.byref(p), capi.PART_EYE)
    for roles in ((lbp, haar, haar), (haar, lbp, haar), (haar, haar, lbp)):
        assert L.nvca_part_stream_create(ctx.h, C.byref(p), roles[0].h, roles[1].h, roles[2].h, C.byref(h)) == capi.ERR_UNSUPPORTED
        assert L.nvca_last_error(ctx.h)
    # the context still detects with the old-format cascade
    gray = synth.make_gray(160, 120, 5, "natural", [(40, 30, 48)])
    assert np.array_equal(ctx.detect_multiscale(haar, gray, 1.2, 2), orc.detect_multiscale(orc_cascade, gray, 1.2, 2))
    haar.free()


def test_old_and_lbp_cascades_alternate_on_one_context(ctx, loaded, synth_xml, orc_cascade):
    haar = ctx.load_cascade_xml(synth_xml)
    cols, rows, sf = K.IMAGES[1]
    gray = K.image(cols, rows, 24, 24)
    exp = K.expected_raw("w24", cols, rows, sf)
    for _ in range(2):
        for fl in (0, capi.HAAR_SCALE_IMAGE):
            assert np.array_equal(ctx.detect_raw(haar, gray, sf, fl), orc.detect_raw(orc_cascade, gray, sf, fl)), fl
            assert np.array_equal(_raw(ctx, loaded("w24"), gray, sf), exp)
            assert np.array_equal(ctx.detect_multiscale(haar, gray, sf, 2, fl), orc.detect_multiscale(orc_cascade, gray, sf, 2, fl)), fl
    haar.free()
