"""detectMultiScale on batches of images (nvca_detect_raw_batch / nvca_detect_multiscale_batch; csrc/detect.cpp) and the image axis of the
LBP evaluator (csrc/kernels_cascade_lbp.hip, lbp_job.cpp): every slot bit for bit against the numpy statement of SURVEY.md A.15 on that
slot's image alone (tests/lbp_reference.py), Haar cascades against the oracle.  Every batch holds a different image per slot and is run
in reversed slot order as well: a slot mix-up, or a read that runs from one image's planes into the next image's, changes a list.  The
batches are tests/lbp_batch_cases.py's; tests/test_lbp_batch_cpu.py asserts on the statement alone that no comparison here is an empty one."""
import ctypes as C

import numpy as np
import pytest

import lbp_batch_cases as B
import lbp_cases as K
import orc
from nubovca import capi, synth
from test_gpu_lbp import FLAGS

pytestmark = pytest.mark.gpu
CAP = 1 << 14


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


def _grouped(raw, mn):
    if mn == 0 or len(raw) == 0:
        return raw
    return np.asarray(orc.group_rectangles(raw, max(mn, 1), 0.2)[0], np.int32).reshape(-1, 4)


def _same(got, exp):
    return len(got) == len(exp) and all(g.shape == e.shape and np.array_equal(g, e) for g, e in zip(got, exp))


def _check_lbp_batch(ctx, casc, imgs, exp, sf, mns=(0, 2, 3), flags=0, cap=CAP):
    """raw lists and grouped boxes of the batch, in slot order and in reversed slot order"""
    for order in (slice(None), slice(None, None, -1)):
        im, ex = imgs[order], exp[order]
        assert _same(ctx.detect_raw_batch(casc, im, sf, flags, cap=cap), ex), ("raw", order)
        for mn in mns:
            assert _same(ctx.detect_multiscale_batch(casc, im, sf, mn, flags, cap=cap), [_grouped(e, mn) for e in ex]), (mn, order)


def _call(ctx, fn_name, casc, ptrs, w, h, stride, mem, sf, mn, flags, cap):
    """the C entry point on raw pointers: (status, [per-image arrays], counts)"""
    n = len(ptrs)
    arr = (C.c_void_p * max(n, 1))(*ptrs)
    buf, cnt = (capi.Rect * max(cap * n, 1))(), (C.c_int * max(n, 1))()
    if fn_name == "raw":
        rc = ctx.L.nvca_detect_raw_batch(ctx.h, casc.h, n, arr, w, h, stride, mem, sf, flags, 0, 0, 0, 0, buf, cap, cnt)
    else:
        rc = ctx.L.nvca_detect_multiscale_batch(ctx.h, casc.h, n, arr, w, h, stride, mem, sf, mn, flags, 0, 0, 0, 0, buf, cap, cnt)
    flat = np.frombuffer(buf, np.int32).reshape(-1, 4)
    return rc, [flat[i * cap:i * cap + min(cnt[i], cap)].copy() for i in range(n)], list(cnt)[:n]


# ------------------------------------------------------------------ raw and grouped parity
@pytest.mark.parametrize("case", B.BATCHES, ids=B.BATCH_IDS)
def test_raw_lists_and_grouped_boxes_of_a_batch(ctx, loaded, case):
    name, cols, rows, sf, n = case
    _check_lbp_batch(ctx, loaded(name), B.images(name, cols, rows, n), B.expected_batch(name, cols, rows, sf, n), sf)


@pytest.mark.parametrize("n", [32, 33])
def test_job_size_boundary(ctx, loaded, n):
    """32 images fill one job; the 33rd opens a second job of the same round"""
    name, cols, rows, sf = B.BOUNDARY
    imgs = B.images(name, cols, rows, n, B.BOUNDARY_SEED0)
    _check_lbp_batch(ctx, loaded(name), imgs, B.expected_batch(name, cols, rows, sf, n, B.BOUNDARY_SEED0), sf, mns=(3,))


@pytest.mark.parametrize("case", K.skip_cases(), ids=[c[0] for c in K.skip_cases()])
def test_skip_rule_per_image_and_row(ctx, case):
    """the walk's two-state machine starts at 0 for every row of every image: the rolled image in the middle slot answers by its own
    hand-written list, its neighbours by theirs (rows of three images share a wave)"""
    cid, cdict, exp_plain = case
    casc = ctx.load_cascade_xml(synth.lbp_cascade_to_xml(cdict))
    try:
        imgs = [K.column_image(), B.rolled_column_image(), K.column_image()]
        exp = [exp_plain, B.ROLLED_EXPECTED[cid], exp_plain]
        for order in (slice(None), slice(None, None, -1)):
            got = ctx.detect_raw_batch(casc, imgs[order], 4.0)
            assert [g.tolist() for g in got] == exp[order]
        two = ctx.detect_raw_batch(casc, imgs[:2], 4.0)
        assert [g.tolist() for g in two] == exp[:2]
    finally:
        casc.free()


# ------------------------------------------------------------------ overflow
def test_candidate_overflow_of_the_shared_list(ctx, loaded):
    """capacity 1024 an image: the batch's 11984 candidates overflow the job's list of 3072, the launch set runs again and answers exactly;
    capacity 4096: the list of 12288 holds them although one image alone has 10962 -- no re-run, still exact"""
    casc = ctx.load_cascade_xml(synth.lbp_cascade_to_xml(B.code255_cascade()))
    cols, rows, sf = B.CODE255_GEOM
    imgs, exp = list(B.code255_images()), list(B.code255_expected())
    single = K.image(97, 83, 24, 24)
    try:
        for cap in (1024, 4096):
            ctx.set_hit_capacity(cap)
            _check_lbp_batch(ctx, casc, imgs, exp, sf, mns=(3,))
            # the capacity the re-run borrowed is given back: the next single-image call answers as before
            assert np.array_equal(np.asarray(ctx.detect_raw(loaded("w24"), single, 1.1), np.int32).reshape(-1, 4), K.expected_raw("w24", 97, 83, 1.1))
    finally:
        ctx.set_hit_capacity(16384)
        casc.free()
    assert np.array_equal(np.asarray(ctx.detect_raw(loaded("w24"), single, 1.1), np.int32).reshape(-1, 4), K.expected_raw("w24", 97, 83, 1.1))


# ------------------------------------------------------------------ memory and layout
def test_memory_kinds_and_strides(ctx, loaded):
    import torch
    name, cols, rows, sf, n = B.BATCHES[1]                   # 333 x 251: odd pitch
    imgs, exp = B.images(name, cols, rows, n), B.expected_batch(name, cols, rows, sf, n)
    casc = loaded(name)
    rng = np.random.default_rng(7)
    for stride in (cols, cols + 19):
        slot = stride * rows
        # equally spaced in one allocation (read in place); noise in the padding and between the images
        host = rng.integers(0, 256, (n, rows, stride), dtype=np.uint8)
        for i in range(n):
            host[i, :, :cols] = imgs[i]
        dev = torch.from_numpy(host).cuda()
        # unequal distances (copied): image 1 further away than image 0 -> 1
        host2 = rng.integers(0, 256, (n + 2) * slot + 64, dtype=np.uint8)
        offs = [0, slot + 32, 3 * slot + 40][:n]
        for i in range(n):
            host2[offs[i]:offs[i] + slot].reshape(rows, stride)[:, :cols] = imgs[i]
        dev2 = torch.from_numpy(host2).cuda()
        torch.cuda.synchronize()
        layouts = [("host", capi.MEM_HOST, [host[i].ctypes.data for i in range(n)]),
                   ("device-equal", capi.MEM_DEVICE, [dev.data_ptr() + i * slot for i in range(n)]),
                   ("device-unequal", capi.MEM_DEVICE, [dev2.data_ptr() + o for o in offs]),
                   ("host-unequal", capi.MEM_HOST, [host2.ctypes.data + o for o in offs])]
        for lid, mem, ptrs in layouts:
            for order in (1, -1):
                rc, got, cnt = _call(ctx, "raw", casc, ptrs[::order], cols, rows, stride, mem, sf, 0, 0, CAP)
                assert rc == capi.OK and _same(got, exp[::order]), (stride, lid, order)
                rc, got, cnt = _call(ctx, "grouped", casc, ptrs[::order], cols, rows, stride, mem, sf, 3, 0, CAP)
                assert rc == capi.OK and _same(got, [_grouped(e, 3) for e in exp[::order]]), (stride, lid, order)


# ------------------------------------------------------------------ one launch set
def _scopes(ctx, casc, imgs, sf):
    ctx.enable_kernel_timing(1)          # (re)starts the counts
    try:
        got = ctx.detect_raw_batch(casc, imgs, sf)
        return got, {k: v[1] for k, v in ctx.kernel_timing().items()}
    finally:
        ctx.enable_kernel_timing(0)


def test_launch_set_does_not_depend_on_the_number_of_images(ctx, loaded):
    name, cols, rows, sf = "w12", 160, 120, 1.2
    imgs = B.images(name, cols, rows, 33, B.BOUNDARY_SEED0)
    exp = B.expected_batch(name, cols, rows, sf, 33, B.BOUNDARY_SEED0)
    got1, one = _scopes(ctx, loaded(name), imgs[:1], sf)
    got8, eight = _scopes(ctx, loaded(name), imgs[:8], sf)
    got33, two_jobs = _scopes(ctx, loaded(name), imgs, sf)
    assert _same(got1, exp[:1]) and _same(got8, exp[:8]) and _same(got33, exp)
    assert one and "cascade_strip" in one, one
    assert eight == one, (one, eight)
    assert two_jobs == {k: 2 * v for k, v in one.items()}, (one, two_jobs)


# ------------------------------------------------------------------ flags
def test_every_flags_value_answers_as_zero(ctx, loaded):
    name, cols, rows, sf, n = B.BATCHES[0]
    imgs, exp = B.images(name, cols, rows, n), B.expected_batch(name, cols, rows, sf, n)
    for fl in FLAGS:
        _check_lbp_batch(ctx, loaded(name), imgs, exp, sf, mns=(3,), flags=fl)


# ------------------------------------------------------------------ Haar cascades through the same entry points
@pytest.fixture(scope="module")
def haar_images():
    return [synth.make_gray(160, 120, 5 + i, "natural", [(40 + 7 * i, 30 + 3 * i, 48 - 4 * i)]) for i in range(5)]


def test_haar_batches_against_the_oracle(ctx, synth_xml, orc_cascade, haar_images):
    haar = ctx.load_cascade_xml(synth_xml)
    sf = 1.2
    try:
        exp_g = {fl: [orc.detect_multiscale(orc_cascade, g, sf, 2, fl) for g in haar_images]
                 for fl in (0, capi.HAAR_SCALE_IMAGE, capi.HAAR_FIND_BIGGEST_OBJECT)}
        exp_r = {fl: [orc.detect_raw(orc_cascade, g, sf, fl) for g in haar_images] for fl in (0, capi.HAAR_SCALE_IMAGE)}
        assert any(len(e) for e in exp_g[0]) and len({np.asarray(e).tobytes() for e in exp_r[0]}) == len(haar_images)
        for order in (slice(None), slice(None, None, -1)):
            im = haar_images[order]
            for fl, exp in exp_g.items():
                assert _same(ctx.detect_multiscale_batch(haar, im, sf, 2, fl), [np.asarray(e, np.int32).reshape(-1, 4) for e in exp[order]]), (fl, order)
            for fl, exp in exp_r.items():
                assert _same(ctx.detect_raw_batch(haar, im, sf, fl), [np.asarray(e, np.int32).reshape(-1, 4) for e in exp[order]]), (fl, order)
        with pytest.raises(capi.NvcaError) as ei:
            ctx.detect_raw_batch(haar, haar_images, sf, capi.HAAR_FIND_BIGGEST_OBJECT)
        assert ei.value.code == capi.ERR_ARG
    finally:
        haar.free()


# ------------------------------------------------------------------ refusals and edges
def test_refusals_and_edges(ctx, loaded):
    name, cols, rows, sf, n = B.BATCHES[0]
    imgs, exp = B.images(name, cols, rows, n), B.expected_batch(name, cols, rows, sf, n)
    casc, L = loaded(name), ctx.L
    ptrs = [g.ctypes.data for g in imgs]
    arr = (C.c_void_p * n)(*ptrs)
    buf, cnt = (capi.Rect * (CAP * n))(), (C.c_int * n)()

    def raw(n_=n, arr_=arr, sf_=sf, out=buf, cap=CAP, n_out=cnt):
        return L.nvca_detect_raw_batch(ctx.h, casc.h, n_, arr_, cols, rows, cols, capi.MEM_HOST, sf_, 0, 0, 0, 0, 0, out, cap, n_out)

    def grouped(n_=n, arr_=arr, sf_=sf, out=buf, cap=CAP, n_out=cnt):
        return L.nvca_detect_multiscale_batch(ctx.h, casc.h, n_, arr_, cols, rows, cols, capi.MEM_HOST, sf_, 3, 0, 0, 0, 0, 0, out, cap, n_out)

    holed = (C.c_void_p * n)(*(ptrs[:1] + [None] + ptrs[2:]))
    for fn in (raw, grouped):
        assert fn(n_=0) == capi.OK
        assert fn() == capi.OK
        assert fn(n_=-1) == capi.ERR_ARG
        assert fn(arr_=None) == capi.ERR_ARG
        assert fn(arr_=holed) == capi.ERR_ARG
        assert fn(cap=-1) == capi.ERR_ARG
        assert fn(out=None) == capi.ERR_ARG
        assert fn(n_out=None) == capi.ERR_ARG
        assert fn(sf_=1.0) == capi.ERR_ARG and fn(sf_=0.5) == capi.ERR_ARG
        assert fn(out=None, cap=0) == capi.OK          # counts alone
    assert ctx.detect_raw_batch(casc, [], sf) == []
    # a cap below a count: the full count is reported, cap rectangles are written, the next image's region is untouched
    small = min(len(e) for e in exp) - 5
    assert small > 0
    rc, got, counts = _call(ctx, "raw", casc, ptrs, cols, rows, cols, capi.MEM_HOST, sf, 0, 0, small)
    assert rc == capi.OK and counts == [len(e) for e in exp]
    assert _same(got, [e[:small] for e in exp])
    assert raw(out=None, cap=0) == capi.OK and list(cnt) == [len(e) for e in exp]
    # after the refusals the context answers as before
    assert _same(ctx.detect_raw_batch(casc, imgs, sf), exp)


# ------------------------------------------------------------------ alternation
def test_batches_and_single_calls_alternate_on_one_context(ctx, loaded, synth_xml, orc_cascade, haar_images):
    haar = ctx.load_cascade_xml(synth_xml)
    name, cols, rows, sf, n = B.BATCHES[0]
    imgs, exp = B.images(name, cols, rows, n), B.expected_batch(name, cols, rows, sf, n)
    hexp = [np.asarray(orc.detect_multiscale(orc_cascade, g, 1.2, 2, capi.HAAR_SCALE_IMAGE), np.int32).reshape(-1, 4) for g in haar_images]
    try:
        for _ in range(2):
            assert _same(ctx.detect_raw_batch(loaded(name), imgs, sf), exp)
            assert _same(ctx.detect_multiscale_batch(haar, haar_images, 1.2, 2, capi.HAAR_SCALE_IMAGE), hexp)
            assert np.array_equal(np.asarray(ctx.detect_raw(loaded(name), imgs[1], sf), np.int32).reshape(-1, 4), exp[1])
            assert np.array_equal(np.asarray(ctx.detect_multiscale(haar, haar_images[2], 1.2, 2, capi.HAAR_SCALE_IMAGE), np.int32).reshape(-1, 4), hexp[2])
            assert _same(ctx.detect_multiscale_batch(loaded(name), imgs, sf, 3), [_grouped(e, 3) for e in exp])
    finally:
        haar.free()
