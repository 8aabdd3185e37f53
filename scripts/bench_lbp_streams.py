"""Times of NuboFaceDetector streams on a new-format LBP cascade (nvca_face_stream_create_any) on one MI355X, beside the route a caller
had before them: nvca_bgr2gray + nvca_equalize_hist per frame, then nvca_detect_multiscale_batch on the equalised images (grouping on the
host, no track_faces, no frame gate -- the composed route does LESS than the stream).

32 streams a call, 1920 x 1080 BGR frames resident in HBM, width_to_process 1920 (full resolution), scale factor 1.10 and 1.25,
min_neighbors 3, minSize (96, 54) as the stream sets it; scripts/bench_lbp.py's calibrated 24 x 24 LBP cascade of 20 stages.  Per frame:
host clock around the synchronous call (nvca_face_batch_process), around a serving loop with two tickets in flight
(nvca_face_batch_submit / _collect, two sets of 32 streams), and around the composed route.  Per kernel: nvca_ctx_kernel_timing.  Steady
state: 3 untimed calls, then --repeats groups of --calls calls; median (min, max) over the groups.  A library without
nvca_face_stream_create_any runs the composed route alone (the figure of a parent commit).

    python scripts/bench_lbp_streams.py [--repeats 7] [--calls 4] > profiles/r09/lbp_streams.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nubomedia-vca_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

W, H, N, MN = 1920, 1080, 32, 3
STAGES = (3, 4, 4, 5, 5, 6, 6, 6, 7, 7, 7, 8, 8, 8, 8, 9, 9, 9, 10, 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--pcts", default="10,25")
    args = ap.parse_args()
    import torch
    from nubovca import capi, synth
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    have_streams = hasattr(ctx.L, "nvca_face_stream_create_any")
    faces = [(300, 200, 2.0), (1200, 500, 4.0), (800, 100, 1.0)]
    grays = [synth.paste_lbp_faces(synth.make_gray(W, H, synth.frame_seed(0, 1 + i), "natural"), faces, 24, 24) for i in range(N)]
    bgr = np.ascontiguousarray(np.stack([np.dstack([g] * 3) for g in grays]))
    dev = torch.from_numpy(bgr).cuda()
    gray_dev = torch.empty((N, H, W), dtype=torch.uint8, device="cuda")
    eq_dev = torch.empty((N, H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    calib = [synth.make_gray(W // 2, H // 2, synth.frame_seed(7, 9100 + i), "natural") for i in range(4)]
    lbp = ctx.load_cascade_xml(synth.lbp_cascade_xml(ow=24, oh=24, seed=4, stage_sizes=STAGES, pass_rate=0.5, calibrate_on=calib))
    frames = [capi.make_frame(dev.data_ptr() + i * W * H * 3, W, H, W * 3, capi.MEM_DEVICE) for i in range(N)]
    cap = 1 << 12
    buf, cnt = (capi.Rect * (cap * N))(), (C.c_int * N)()
    ptrs = (C.c_void_p * N)(*[eq_dev.data_ptr() + i * W * H for i in range(N)])

    def measure(fn):
        for _ in range(3):
            boxes = fn()
        wall, kern = [], []
        for _ in range(args.repeats):
            ctx.enable_kernel_timing(1)
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            wall.append((time.perf_counter() - t0) / (args.calls * N) * 1e3)
            kern.append({k: (ms / (args.calls * N), c // args.calls) for k, (ms, c) in ctx.kernel_timing().items()})
            ctx.enable_kernel_timing(0)
        return boxes, wall, kern

    def report(title, boxes, wall, kern):
        print("## %s" % title)
        print("boxes a frame %s ...; per FRAME (host clock, timing events on): median %.3f ms, min %.3f, max %.3f over %d groups of %d calls of %d frames"
              % (boxes[:8], statistics.median(wall), min(wall), max(wall), args.repeats, args.calls, N))
        for k in sorted(kern[0]):
            v = [g[k][0] for g in kern]
            print("  %-18s %8.3f ms a frame (min %.3f, max %.3f), %d scopes a call" % (k, statistics.median(v), min(v), max(v), kern[0][k][1]))
        return statistics.median(wall), min(wall), max(wall)

    print("# bench_lbp_streams: %d streams a call, %d x %d BGR frames in HBM, width_to_process %d, min_neighbors %d; 24 x 24 LBP cascade, %d stages"
          % (N, W, H, W, MN, len(STAGES)))
    if not have_streams:
        print("# this library has no nvca_face_stream_create_any: the composed route alone")
    for pct in [int(v) for v in args.pcts.split(",")]:
        sf = 1 + pct / 100

        def composed():
            for i in range(N):
                ctx.check(ctx.L.nvca_bgr2gray(ctx.h, dev.data_ptr() + i * W * H * 3, W, H, W * 3, 3, capi.MEM_DEVICE, gray_dev.data_ptr() + i * W * H, W))
                ctx.check(ctx.L.nvca_equalize_hist(ctx.h, gray_dev.data_ptr() + i * W * H, W, H, W, capi.MEM_DEVICE, eq_dev.data_ptr() + i * W * H, W))
            ctx.check(ctx.L.nvca_detect_multiscale_batch(ctx.h, lbp.h, N, ptrs, W, H, W, capi.MEM_DEVICE, sf, MN, 0, W // 20, H // 20, 0, 0, buf, cap, cnt))
            return [cnt[i] for i in range(N)]

        comp = report("scale factor %.2f: nvca_bgr2gray + nvca_equalize_hist per frame, then nvca_detect_multiscale_batch (the route before)" % sf, *measure(composed))
        if not have_streams:
            continue
        sets = [[capi.FaceStream(ctx, lbp, any_format=True, width_to_process=W, multi_scale_factor=pct, min_neighbors=MN) for _ in range(N)] for _ in range(2)]

        def sync_call():
            res = ctx.face_batch_process(sets[0], frames, 64)
            return [len(b) for b, _ in res]

        def two_tickets():
            # a serving loop: the next batch is submitted before the previous one is collected
            t = [ctx.face_batch_submit(sets[0], frames), None]
            for k in range(1, 4):
                t[k % 2] = ctx.face_batch_submit(sets[k % 2], frames)
                res = ctx.face_batch_collect(t[(k - 1) % 2], 64)
            last = ctx.face_batch_collect(t[3 % 2], 64)
            return [len(b) for b, _ in last]

        sb = report("scale factor %.2f: nvca_face_batch_process, %d LBP streams" % (sf, N), *measure(sync_call))
        boxes, wall, kern = measure(two_tickets)
        wall = [w / 4 for w in wall]                                   # four batches a round
        kern = [{k: (ms / 4, c) for k, (ms, c) in g.items()} for g in kern]
        tt = report("scale factor %.2f: nvca_face_batch_submit / _collect, two tickets in flight (4 batches a round)" % sf, boxes, wall, kern)
        print("## scale factor %.2f: stream %.3f ms a frame (min %.3f, max %.3f), two tickets %.3f (min %.3f, max %.3f), composed route %.3f (min %.3f, max %.3f): %.2f x / %.2f x%s"
              % ((sf,) + sb + tt + comp + (comp[0] / sb[0], comp[0] / tt[0], "" if sb[0] < comp[0] else "  -- THE STREAM IS NOT FASTER THAN THE COMPOSED ROUTE")))
    ctx.close()


if __name__ == "__main__":
    main()
