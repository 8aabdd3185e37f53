"""detectMultiScale on batches of images (nvca_detect_raw_batch / nvca_detect_multiscale_batch) with a new-format HAAR cascade: the image
axis of csrc/kernels_cascade_hnew.hip (grid.y of stage 0, the merged survivor list, image b's sum AND squared-integral planes).  Every
slot bit for bit against the numpy statement of SURVEY.md A.16 on that slot's image alone (tests/haar_new_reference.py) and against
the single-image call; every batch holds a different image per slot and is run in reversed slot order as well, so a slot mix-up, or a
read that runs from one image's planes into the next image's, changes a list."""
import ctypes as C
import functools

import numpy as np
import pytest

import haar_new_cases as K
import haar_new_reference as R
import lbp_batch_cases as LB
import lbp_cases as LK
import orc
from nubovca import capi, synth

pytestmark = pytest.mark.gpu
CAP = 1 << 14
COLS, ROWS, SF = K.IMAGES[0]          # 97 x 83 at 1.1


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def loaded(ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ctx.load_cascade_xml(K.cascade(name)[0])
        return cache[name]
    return get


def images(name, n, seed0=11):
    ow, oh = K.cascade(name)[1].size
    return [K.image(COLS, ROWS, ow, oh, seed0 + i) for i in range(n)]


@functools.lru_cache(maxsize=None)
def expected(name, seed):
    c = K.cascade(name)[1]
    return R.scan(c, K.image(COLS, ROWS, *c.size, seed), SF)


def expected_batch(name, n, seed0=11):
    return [expected(name, seed0 + i) for i in range(n)]


def _grouped(raw, mn):
    if mn == 0 or len(raw) == 0:
        return raw
    return np.asarray(orc.group_rectangles(raw, max(mn, 1), 0.2)[0], np.int32).reshape(-1, 4)


def _same(got, exp):
    return len(got) == len(exp) and all(g.shape == e.shape and np.array_equal(g, e) for g, e in zip(got, exp))


def _check_batch(ctx, casc, imgs, exp, sf=SF, mns=(0, 2, 3), cap=CAP):
    """raw lists and grouped boxes of the batch, in slot order and in reversed slot order"""
    assert all(len(e) > 0 for e in exp) and len({e.tobytes() for e in exp}) == len(exp)          # no empty and no repeated comparison
    for order in (slice(None), slice(None, None, -1)):
        im, ex = imgs[order], exp[order]
        assert _same(ctx.detect_raw_batch(casc, im, sf, 0, cap=cap), ex), ("raw", order)
        for mn in mns:
            assert _same(ctx.detect_multiscale_batch(casc, im, sf, mn, 0, cap=cap), [_grouped(e, mn) for e in ex]), (mn, order)


@pytest.mark.parametrize("name,n", [("w24", 2), ("w24", 3), ("w20x28", 2)], ids=["w24-x2", "w24-x3", "w20x28-x2"])
def test_raw_lists_and_grouped_boxes_of_a_batch(ctx, loaded, name, n):
    imgs, exp = images(name, n), expected_batch(name, n)
    _check_batch(ctx, loaded(name), imgs, exp)
    for g, e in zip(imgs, exp):           # each slot equals its single-image call
        assert np.array_equal(np.asarray(ctx.detect_raw(loaded(name), g, SF), np.int32).reshape(-1, 4), e)


@pytest.mark.parametrize("n", [32, 33])
def test_job_size_boundary(ctx, loaded, n):
    """32 images fill one job; the 33rd opens a second job of the same round"""
    _check_batch(ctx, loaded("w12"), images("w12", n, 100), expected_batch("w12", n, 100), mns=(3,))


@pytest.mark.parametrize("case", K.skip_cases(), ids=[c[0] for c in K.skip_cases()])
def test_skip_rule_per_image_and_row(ctx, case):
    """the walk starts in state 0 for every row of every image: the rolled image in the middle slot (lbp_batch_cases: the even and the odd grid
    columns swap) answers by its own hand-written list, its neighbours by theirs"""
    cid, cdict, exp_plain = case
    casc = ctx.load_cascade_xml(synth.haar_new_cascade_to_xml(cdict))
    try:
        imgs = [LK.column_image(), LB.rolled_column_image(), LK.column_image()]
        exp = [exp_plain, LB.ROLLED_EXPECTED[cid], exp_plain]
        for order in (slice(None), slice(None, None, -1)):
            assert [g.tolist() for g in ctx.detect_raw_batch(casc, imgs[order], 4.0)] == exp[order]
    finally:
        casc.free()


def test_candidate_overflow_of_the_shared_list(ctx, loaded):
    """capacity 256 an image: the permissive cascade's candidates (over a thousand an image) overflow the job's list of 768, the launch set
    runs again and answers exactly; the capacity the re-run borrowed is given back"""
    xml = synth.haar_new_cascade_to_xml(K.permissive(24, 24))
    casc, ref = ctx.load_cascade_xml(xml), R.parse_xml(xml)
    imgs = images("w24", 3)
    exp = [R.scan(ref, g, SF) for g in imgs]
    assert min(len(e) for e in exp) > 1000
    single = np.asarray(ctx.detect_raw(loaded("w24"), imgs[0], SF), np.int32).reshape(-1, 4)
    ctx.set_hit_capacity(256)
    try:
        for order in (slice(None), slice(None, None, -1)):
            assert _same(ctx.detect_raw_batch(casc, imgs[order], SF, 0, cap=CAP), exp[order])
            assert _same(ctx.detect_multiscale_batch(casc, imgs[order], SF, 3, 0, cap=CAP), [_grouped(e, 3) for e in exp[order]])
        assert np.array_equal(np.asarray(ctx.detect_raw(loaded("w24"), imgs[0], SF), np.int32).reshape(-1, 4), single)
    finally:
        ctx.set_hit_capacity(16384)
        casc.free()
    assert np.array_equal(single, expected("w24", 11))


def test_host_and_device_memory(ctx, loaded):
    import torch
    n = 3
    imgs, exp = images("w24", n), expected_batch("w24", n)
    casc = loaded("w24")
    rng = np.random.default_rng(7)
    for stride in (COLS, COLS + 19):
        slot = stride * ROWS
        host = rng.integers(0, 256, (n, ROWS, stride), dtype=np.uint8)          # noise in the padding
        for i in range(n):
            host[i, :, :COLS] = imgs[i]
        dev = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        for mem, ptrs in ((capi.MEM_HOST, [host[i].ctypes.data for i in range(n)]), (capi.MEM_DEVICE, [dev.data_ptr() + i * slot for i in range(n)])):
            for order in (1, -1):
                arr = (C.c_void_p * n)(*ptrs[::order])
                buf, cnt = (capi.Rect * (CAP * n))(), (C.c_int * n)()
                ctx.check(ctx.L.nvca_detect_raw_batch(ctx.h, casc.h, n, arr, COLS, ROWS, stride, mem, SF, 0, 0, 0, 0, 0, buf, CAP, cnt))
                flat = np.frombuffer(buf, np.int32).reshape(-1, 4)
                assert _same([flat[i * CAP:i * CAP + cnt[i]] for i in range(n)], exp[::order]), (stride, mem, order)
                ctx.check(ctx.L.nvca_detect_multiscale_batch(ctx.h, casc.h, n, arr, COLS, ROWS, stride, mem, SF, 3, 0, 0, 0, 0, 0, buf, CAP, cnt))
                flat = np.frombuffer(buf, np.int32).reshape(-1, 4)
                assert _same([flat[i * CAP:i * CAP + cnt[i]] for i in range(n)], [_grouped(e, 3) for e in exp[::order]]), (stride, mem, order)


def test_launch_set_does_not_depend_on_the_number_of_images(ctx, loaded):
    imgs, exp = images("w12", 33, 100), expected_batch("w12", 33, 100)

    def scopes(batch):
        ctx.enable_kernel_timing(1)
        try:
            got = ctx.detect_raw_batch(loaded("w12"), batch, SF)
            return got, {k: v[1] for k, v in ctx.kernel_timing().items()}
        finally:
            ctx.enable_kernel_timing(0)
    got1, one = scopes(imgs[:1])
    got8, eight = scopes(imgs[:8])
    got33, two_jobs = scopes(imgs)
    assert _same(got1, exp[:1]) and _same(got8, exp[:8]) and _same(got33, exp)
    assert one and "cascade_strip" in one and "cascade_roi" not in one, one
    assert eight == one and two_jobs == {k: 2 * v for k, v in one.items()}, (one, eight, two_jobs)
