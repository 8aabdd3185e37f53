"""cv::resize's 8-bit rule on the GPU, through every kernel that has an entry point returning its image: nvca_resize_linear (k_resize1 from
host and from device memory, k_resize3) against the oracle's cv::resize, and the device overlays (k_overlay on a BGR frame, k_overlay_yuv on
NV12 / I420 frames; images of 1, 3 and 4 channels) against the numpy statements of tests/overlay_reference.py and
tests/yuv_out_reference.py.  The shapes are tests/overlay_reference.py's RULE_SHAPES, the table the host rule is pinned with in
tests/test_overlay_cpu.py: every branch of the rule, and more than one 256-column block.  Every comparison is np.array_equal.
(k_gray_generic, k_gray_yuv_generic and k_work_resize return boxes, not their image: tests/test_gpu_parity.py, test_gpu_yuv.py and
test_gpu_yuv_parts.py hold them.)"""
import functools

import numpy as np
import pytest

import yuv_out_cases as K
import yuv_out_reference as S
from overlay_reference import RULE_SHAPES, overlay_blend as ref_blend, rule_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from nubovca import capi
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _oracle(sw, sh, dw, dh, cn):
    import orc
    out = orc.resize_linear(rule_image(sw, sh, cn), dw, dh)
    out.setflags(write=False)
    return out


def _resize_on_device(ctx, img, dw, dh):
    """nvca_resize_linear of a tightly allocated 1-channel device image into a device image"""
    import torch
    from nubovca import capi
    sh, sw = img.shape
    src, dst = torch.from_numpy(img).cuda(), torch.zeros((dh, dw), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.check(ctx.L.nvca_resize_linear(ctx.h, src.data_ptr(), sw, sh, sw, 1, capi.MEM_DEVICE, dst.data_ptr(), dw, dh, dw))
    ctx.synchronize()
    return dst.cpu().numpy()


SHAPE_IDS = ["%dx%d_to_%dx%d" % s for s in RULE_SHAPES]


@pytest.mark.parametrize("shape", RULE_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("route", ["gray_host", "gray_device", "bgr"])
def test_resize_linear_equals_the_oracle(ctx, route, shape):
    sw, sh, dw, dh = shape
    cn = 3 if route == "bgr" else 1
    img = rule_image(sw, sh, cn)
    got = _resize_on_device(ctx, img, dw, dh) if route == "gray_device" else ctx.resize_linear(img, dw, dh)
    assert np.array_equal(got, _oracle(sw, sh, dw, dh, cn))


@pytest.mark.parametrize("shape", RULE_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_overlay_on_a_bgr_device_frame(ctx, cn, shape):
    import torch
    from nubovca import capi
    sw, sh, dw, dh = shape
    img = rule_image(sw, sh, cn)
    W, H = dw + 7, dh + 5
    frame = np.random.default_rng(dw * 7 + dh).integers(0, 256, (H, W, 3)).astype(np.uint8)
    exp = ref_blend(frame.copy(), [(3, 2, dw, dh)], img)
    dev = torch.from_numpy(frame).cuda()
    torch.cuda.synchronize()
    capi.overlay_blend(ctx, capi.make_frame(dev.data_ptr(), W, H, W * 3, capi.MEM_DEVICE), [(3, 2, dw, dh)], img)
    got = dev.cpu().numpy()
    assert np.array_equal(got, exp), int((got != exp).sum())


@pytest.mark.parametrize("shape", RULE_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("fmt", K.FMTS, ids=K.FMT_IDS)
def test_overlay_on_a_420_device_frame(ctx, fmt, cn, shape):
    """the frame is padded to an even size, not the image; the box sits at odd offsets: blocks covered in part on every side"""
    import torch
    from nubovca import capi
    sw, sh, dw, dh = shape
    img = rule_image(sw, sh, cn)
    W, H = (dw + 8) & ~1, (dh + 6) & ~1
    buf, lay = K.random_frame(W, H, fmt, dw * 7 + dh, tail=5)
    L = capi.pixel_layout(*lay)
    exp = S.overlay(buf, W, H, lay, [(3, 1, dw, dh)], img)
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    capi.overlay_blend_yuv420(ctx, capi.make_planar_frame(dev.data_ptr(), W, H, L, capi.MEM_DEVICE), L, [(3, 1, dw, dh)], img)
    got = dev.cpu().numpy()
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:8].tolist()
