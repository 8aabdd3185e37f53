"""New-format HAAR cascades on the device (csrc/kernels_cascade_hnew.hip around kernels_cascade_lbp.hip's walk kernel, lbp_job.cpp's
plan and launch set on hnew_tables.cpp's tables) against the numpy statement of SURVEY.md A.16 (tests/haar_new_reference.py): bit for
bit, raw lists and grouped boxes.  The cases and the hand-derived lists are tests/haar_new_cases.py's; tests/test_haar_new_cpu.py
asserts on the statement alone that they are not empty comparisons and reach the branches they are meant to reach."""
import ctypes as C
import os

import numpy as np
import pytest

import haar_new_cases as K
import haar_new_reference as R
import lbp_cases as LK
import orc
from nubovca import capi, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newformat_haar_20x20.xml.txt")
FLAGS = (capi.HAAR_DO_CANNY_PRUNING, capi.HAAR_SCALE_IMAGE, capi.HAAR_FIND_BIGGEST_OBJECT, capi.HAAR_DO_ROUGH_SEARCH,
         capi.HAAR_FIND_BIGGEST_OBJECT | capi.HAAR_DO_ROUGH_SEARCH, 15)
DUMP_KEYS = ("rects", "weights", "rect_counts", "feature_idx", "thr", "leaves", "stage_sizes", "stage_thr")


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
    casc = ctx.load_cascade_xml(synth.haar_new_cascade_to_xml(cdict))
    try:
        return _raw(ctx, casc, gray, sf, 0, min_size, max_size).tolist()
    finally:
        casc.free()


# ------------------------------------------------------------------ loader
@pytest.mark.parametrize("style", ["traincascade", "minimal"])
def test_dump_haar_new_is_the_reference_readers(ctx, style):
    xml, ref = K.cascade("w24", style)
    casc = ctx.load_cascade_xml(xml)
    d, e = casc.dump_haar_new(), ref.arrays()
    assert d["size"] == e["size"]
    for k in DUMP_KEYS:
        assert d[k].dtype == e[k].dtype and np.array_equal(d[k], e[k]), k
    assert casc.format() == (capi.CASCADE_HAAR_NEW, len(ref.rects))
    assert casc.info() == (24, 24, len(ref.stage_sizes), len(ref.feature_idx))
    assert casc.kind() == (False, False)
    for dump in (casc.dump, casc.dump_lbp):
        with pytest.raises(capi.NvcaError) as ei:
            dump()
        assert ei.value.code == capi.ERR_ARG
    casc.free()


def test_golden_file_loads_from_disk_and_scans_as_the_statement(ctx):
    ref = R.parse_xml(open(GOLDEN).read())
    casc = ctx.load_cascade_file(GOLDEN)
    d, e = casc.dump_haar_new(), ref.arrays()
    for k in DUMP_KEYS:
        assert np.array_equal(d[k], e[k]), k
    assert casc.format() == (capi.CASCADE_HAAR_NEW, 9) and casc.info() == (20, 20, 3, 9)
    gray = K.image(97, 83, 20, 20)
    exp = R.scan(ref, gray, 1.1)
    assert len(exp) > 0 and np.array_equal(_raw(ctx, casc, gray, 1.1), exp)
    casc.free()


def test_other_formats_refuse_dump_haar_new(ctx, synth_xml):
    for xml in (synth_xml, LK.cascade("w12")[0]):
        casc = ctx.load_cascade_xml(xml)
        with pytest.raises(capi.NvcaError) as ei:
            casc.dump_haar_new()
        assert ei.value.code == capi.ERR_ARG
        casc.free()


# ------------------------------------------------------------------ the hand-made cases of tests/test_haar_new_cpu.py
@pytest.mark.parametrize("case", K.value_cases(), ids=[c[0] for c in K.value_cases()])
def test_hand_made_windows(ctx, case):
    _, cdict, gray, exp = case
    assert _hand(ctx, cdict, gray, 2.0) == exp


@pytest.mark.parametrize("case", K.skip_cases(), ids=[c[0] for c in K.skip_cases()])
def test_skip_columns(ctx, case):
    _, cdict, exp = case
    assert _hand(ctx, cdict, LK.column_image(), 4.0) == exp


@pytest.mark.parametrize("case", K.scan_rule_cases(), ids=[c[0] for c in K.scan_rule_cases()])
def test_scan_rules(ctx, case):
    _, cdict, shape, sf, mins, maxs, exp = case
    assert _hand(ctx, cdict, np.full(shape, 120, np.uint8), sf, mins, maxs) == exp


# ------------------------------------------------------------------ raw lists and grouped boxes
RAW_CASES = [(n,) + im for n in ("w24", "w20x28", "w12") for im in K.IMAGES] + [("w24",) + K.WIDE]


@pytest.mark.parametrize("name,cols,rows,sf", RAW_CASES, ids=["%s-%dx%d" % c[:3] for c in RAW_CASES])
def test_raw_list_and_grouped_boxes(ctx, loaded, name, cols, rows, sf):
    ref = K.cascade(name)[1]
    gray = K.image(cols, rows, *ref.size)
    exp = K.expected_raw(name, cols, rows, sf)
    got = _raw(ctx, loaded(name), gray, sf)
    assert got.shape == exp.shape and np.array_equal(got, exp)
    for mn in (0, 2, 3):
        assert np.array_equal(_grouped(ctx, loaded(name), gray, sf, mn), _expected_grouped(exp, mn)), mn


def test_stage_heavy_cascade_reaches_the_last_stage_group(ctx, loaded):
    cols, rows, sf = K.DEEP_IMAGE
    gray = K.image(cols, rows, 24, 24)
    exp = K.expected_raw("deep", cols, rows, sf)
    assert np.array_equal(_raw(ctx, loaded("deep"), gray, sf), exp)
    assert np.array_equal(_grouped(ctx, loaded("deep"), gray, sf, 3), _expected_grouped(exp, 3))


@pytest.mark.parametrize("name", ["w81", "w82"])
def test_windows_on_both_sides_of_the_lds_bound(ctx, loaded, name):
    """81 x 81: the stage-0 tile fits 64 KiB of LDS; 82 x 82: it does not, stage 0 gathers from the plane"""
    cols, rows, sf = K.LDS_IMAGE
    ow = K.CASCADES[name]["ow"]
    exp = K.expected_raw(name, cols, rows, sf)
    assert np.array_equal(_raw(ctx, loaded(name), K.image(cols, rows, ow, ow), sf), exp)


@pytest.mark.parametrize("route", sorted(K.HI_PLANES))
def test_high_byte_planes_of_the_squared_integral(ctx, loaded, route):
    """Q above 2^32 inside levels behind the first, where the two pyramid routes (one integral launch for all levels / one a level) leave
    a level's high-byte plane at different places"""
    cols, rows, sf = K.HI_PLANES[route]
    g = K.hi_planes_image(cols, rows)
    exp = R.scan(K.cascade("w81")[1], g, sf)
    assert len(exp) > 0 and np.array_equal(_raw(ctx, loaded("w81"), g, sf), exp)


def test_rect_sums_above_2p24_on_a_bright_image(ctx):
    xml, ref = K.bright_cascade()
    casc = ctx.load_cascade_xml(xml)
    exp = R.scan(ref, K.bright_image(), 1.5)
    assert np.array_equal(_raw(ctx, casc, K.bright_image(), 1.5), exp)
    casc.free()


def test_host_group_switch_gives_the_same_boxes(ctx, loaded):
    cols, rows, sf = K.IMAGES[1]
    gray = K.image(cols, rows, 24, 24)
    exp = K.expected_raw("w24", cols, rows, sf)
    for hg in (0, 1):
        with ctx.options(host_group=hg):
            for mn in (0, 2, 3):
                assert np.array_equal(_grouped(ctx, loaded("w24"), gray, sf, mn), _expected_grouped(exp, mn)), (hg, mn)


def test_host_images_device_images_and_a_padded_sub_matrix(ctx, loaded):
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


def test_candidate_overflow_rerun_answers_exactly(ctx):
    cols, rows, sf = K.IMAGES[1]
    gray = K.image(cols, rows, 24, 24)
    xml = synth.haar_new_cascade_to_xml(K.permissive(24, 24))
    casc = ctx.load_cascade_xml(xml)
    exp = R.scan(R.parse_xml(xml), gray, sf)
    assert len(exp) > 3000
    ctx.set_hit_capacity(256)
    try:
        assert np.array_equal(_raw(ctx, casc, gray, sf), exp)
        assert np.array_equal(_grouped(ctx, casc, gray, sf, 3), _expected_grouped(exp, 3))
    finally:
        ctx.set_hit_capacity(16384)
        casc.free()


def test_no_small_image_launch_serves_a_new_format_haar_scan(ctx, loaded):
    """97 x 83 fits the small-image route's LDS (an LBP cascade's scan of it is one NVCA_K_ROI launch); a new-format HAAR cascade's takes the
    large-image route: window-per-lane launches, none booked under NVCA_K_ROI"""
    cols, rows, sf = K.IMAGES[0]
    gray = K.image(cols, rows, 24, 24)
    ctx.enable_kernel_timing(True)
    try:
        ctx.kernel_timing()
        assert np.array_equal(_raw(ctx, loaded("w24"), gray, sf), K.expected_raw("w24", cols, rows, sf))
        booked = ctx.kernel_timing()          # {kernel name: (ms, launches)} of the slots that launched
    finally:
        ctx.enable_kernel_timing(False)
    assert "cascade_roi" not in booked and booked["cascade_strip"][1] >= 1


def test_streams_made_without_any_refuse_a_new_format_haar_cascade(ctx, loaded, synth_xml):
    haar = ctx.load_cascade_xml(synth_xml)
    new = loaded("w24")
    L = ctx.L
    h = C.c_void_p()
    assert L.nvca_face_stream_create(ctx.h, new.h, None, C.byref(h)) == capi.ERR_UNSUPPORTED and L.nvca_last_error(ctx.h)
    p = capi.PartParams()
    L.nvca_part_params_default(C.byref(p), capi.PART_EYE)
    for roles in ((new, haar, haar), (haar, new, haar), (haar, haar, new)):
        assert L.nvca_part_stream_create(ctx.h, C.byref(p), roles[0].h, roles[1].h, roles[2].h, C.byref(h)) == capi.ERR_UNSUPPORTED
        assert L.nvca_last_error(ctx.h)
    haar.free()


def test_three_formats_alternate_on_one_context(ctx, loaded, synth_xml, orc_cascade):
    haar = ctx.load_cascade_xml(synth_xml)
    lbp = ctx.load_cascade_xml(LK.cascade("w24")[0])
    cols, rows, sf = K.IMAGES[1]
    gray = K.image(cols, rows, 24, 24)
    exp = K.expected_raw("w24", cols, rows, sf)
    exp_lbp = __import__("lbp_reference").scan(LK.cascade("w24")[1], gray, sf)
    for _ in range(2):
        assert np.array_equal(ctx.detect_raw(haar, gray, sf, capi.HAAR_SCALE_IMAGE), orc.detect_raw(orc_cascade, gray, sf, capi.HAAR_SCALE_IMAGE))
        assert np.array_equal(_raw(ctx, loaded("w24"), gray, sf), exp)
        assert np.array_equal(_raw(ctx, lbp, gray, sf), exp_lbp)
    haar.free()
    lbp.free()
