"""Times of the way out in 4:2:0 on one MI355X: nvca_bgr_to_yuv420 on 32 different 1080p frames resident in HBM, NV12 and I420 -- the
wide kernel, the generic kernel (forced by a destination base that is 8 bytes off), and nvca_yuv420_to_bgr on the frames just written --
from the NVCA_K_GRAY timers (event pairs in the dispatch packets: kernel time, no launch gap), beside a device-to-device copy that moves
the same bytes in the same run.  A frame is 6 220 800 bytes read and 3 110 400 written: 9 331 200 bytes, which a copy of 4 665 600 bytes
moves (as many read, as many written); the copy is timed with events around ONE copy of 32 frames' worth (a copy per frame would be
timed by its launch) and divided by 32.  The share of HBM peak is bytes over time over 8 TB/s.  Then one 1080p draw of four rectangles
and one 200 x 200 four-channel overlay, on the BGR frame and on the 4:2:0 frame: host clock around synchronous calls.

    python scripts/bench_yuv_out.py [--rounds 20] > profiles/r06/yuv_out.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nubomedia-vca_amd"))

W, H, F = 1920, 1080, 32
BYTES = W * H * 3 + W * H * 3 // 2
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20, help="timed passes over the 32 frames, after 3 untimed ones")
    args = ap.parse_args()
    import torch
    from nubovca import capi
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(F)]
    back = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    layouts = {"nv12": capi.pixel_layout(capi.PIX_NV12, (0, W * H), (W, W)),
               "i420": capi.pixel_layout(capi.PIX_I420, (0, W * H, W * H * 5 // 4), (W, W // 2, W // 2))}
    dst = [torch.empty(W * H * 3 // 2 + 16, dtype=torch.uint8, device="cuda") for _ in range(F)]
    torch.cuda.synchronize()
    print("# bench_yuv_out: %d x %d, %d frames in HBM, %d timed passes after 3; %d bytes a frame (%d read + %d written)"
          % (W, H, F, args.rounds, BYTES, W * H * 3, W * H * 3 // 2))

    def gray_time(fn, frames=F):
        """per-call kernel time in ms of fn(i) over the frames, from the NVCA_K_GRAY timers"""
        for _ in range(3):
            for i in range(frames):
                fn(i)
        ctx.enable_kernel_timing(1)
        for _ in range(args.rounds):
            for i in range(frames):
                fn(i)
        ms, n = ctx.kernel_timing()["gray_resize_hist"]
        ctx.enable_kernel_timing(0)
        assert n == args.rounds * frames, n
        return ms / n

    def copy_time():
        a = torch.empty(F * (BYTES // 2), dtype=torch.uint8, device="cuda").random_(0, 256)
        b = torch.empty_like(a)
        times = []
        for k in range(3 + args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.copy_(a)
            e1.record()
            torch.cuda.synchronize()
            if k >= 3:
                times.append(e0.elapsed_time(e1) / F)
        return statistics.median(times), min(times)

    def line(what, ms):
        print("%-46s %8.2f us a frame   %6.2f TB/s   %5.1f %% of HBM peak" % (what, ms * 1e3, BYTES / (ms * 1e-3) / 1e12, 100 * BYTES / (ms * 1e-3) / HBM_PEAK), flush=True)

    res = {}
    for fmt, lay in layouts.items():
        res[fmt, "wide"] = gray_time(lambda i: ctx.bgr_to_yuv420(src[i].data_ptr(), W, H, lay, dst[i].data_ptr(), capi.MEM_DEVICE))
        line("nvca_bgr_to_yuv420 %s k_bgr_yuv16" % fmt, res[fmt, "wide"])
        res[fmt, "back"] = gray_time(lambda i: ctx.yuv420_to_bgr(dst[i].data_ptr(), W, H, lay, capi.MEM_DEVICE, back.data_ptr(), W * 3))
        line("nvca_yuv420_to_bgr %s (the same frames)" % fmt, res[fmt, "back"])
        res[fmt, "generic"] = gray_time(lambda i: ctx.bgr_to_yuv420(src[i].data_ptr(), W, H, lay, dst[i].data_ptr() + 8, capi.MEM_DEVICE))
        line("nvca_bgr_to_yuv420 %s k_bgr_yuv_generic" % fmt, res[fmt, "generic"])
    # the same kernel on ONE frame of 8 frames' height (1920 x 8640): what a dispatch costs beyond its bytes shows as the difference
    tall_src = torch.cat(src[:8], dim=0).contiguous()
    tall_dst = torch.empty(W * H * 8 * 3 // 2, dtype=torch.uint8, device="cuda")
    tall_lay = capi.pixel_layout(capi.PIX_NV12, (0, W * H * 8), (W, W))
    torch.cuda.synchronize()
    res["tall"] = gray_time(lambda i: ctx.bgr_to_yuv420(tall_src.data_ptr(), W, H * 8, tall_lay, tall_dst.data_ptr(), capi.MEM_DEVICE), 4) / 8
    line("nvca_bgr_to_yuv420 nv12 k_bgr_yuv16, 1920 x 8640 / 8", res["tall"])
    del tall_src, tall_dst
    med, best = copy_time()
    line("device-to-device copy, same bytes (median)", med)
    line("device-to-device copy, same bytes (fastest)", best)
    for fmt in layouts:
        r = res[fmt, "wide"] / med
        print("yardstick %s: k_bgr_yuv16 takes %.2f x the copy's time: %s 2 x" % (fmt, r, "within" if r <= 2 else "NOT within"))

    # ---- drawing: four rectangles, one 200 x 200 four-channel overlay; BGR frame against 4:2:0 frame
    def wall(fn, n=200):
        for _ in range(20):
            fn()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) / n * 1e6
    shapes = [(0, 200, 150, 300, 300, (255, 128, 0, 255)), (0, 900, 400, 180, 180, (255, 128, 0, 255)), (0, 1400, 100, 120, 120, (255, 128, 0, 255)),
              (0, 1500, 700, 240, 240, (255, 128, 0, 255))]
    image = np.random.default_rng(3).integers(0, 256, (200, 200, 4)).astype(np.uint8)
    boxes = [(860, 440, 200, 200)]
    bgr_frame = capi.make_frame(src[0].data_ptr(), W, H, W * 3, capi.MEM_DEVICE)
    print("draw 4 rectangles    bgr   %8.1f us a call" % wall(lambda: ctx.draw_shapes(bgr_frame, 3, shapes)))
    print("overlay 200 x 200 x4 bgr   %8.1f us a call" % wall(lambda: capi.overlay_blend(ctx, bgr_frame, boxes, image)))
    for fmt, lay in layouts.items():
        fr = capi.make_planar_frame(dst[0].data_ptr(), W, H, lay, capi.MEM_DEVICE)
        print("draw 4 rectangles    %-5s %8.1f us a call" % (fmt, wall(lambda: ctx.draw_shapes_yuv420(fr, lay, shapes))))
        print("overlay 200 x 200 x4 %-5s %8.1f us a call" % (fmt, wall(lambda: capi.overlay_blend_yuv420(ctx, fr, lay, boxes, image))))
    print("(a call: host clock around a synchronous entry point -- upload of the shape table or of the image, one launch, one stream drain)")
    ctx.close()


if __name__ == "__main__":
    main()
