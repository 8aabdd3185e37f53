"""Times of the small-image route of new-format HAAR cascades (kernels_roi_hnew.hip, opt-in per cascade through
nvca_cascade_set_small_route) and of part streams on such cascades on one MI355X.  scripts/bench_lbp_parts.py's sibling; the route on
and off are compared in one session on one library, off being the code path of a cascade nobody opted in (the parent commit's).

(a) small calls: nvca_detect_multiscale (min_neighbors 3, scale factor 1.1) on a calibrated 12 x 12 new-format HAAR cascade of 5 stages
    and part-sized device images -- 64 x 48, 120 x 100, 160 x 90.  A group is eight slightly different sizes (w - k, h - g for group g),
    each called --calls times: sizes the context has not seen, as a part detector's face regions are, so the large-image route pays its
    plan and table builds.  The two routes run on two instances of the cascade (one opted in), so neither finds the other's plans.  Per
    call: host clock around the synchronous call; per kernel slot: nvca_ctx_kernel_timing (time and bookings per call).
    --wide adds the cascade of tests/hnew_roi_cases.py whose last stages have 70 and 130 stumps, on its 97 x 83 image (the sizes
    97 - k x 83 - g): where the short-queue form of k_roi_hnew has most to do.
(b) part chain: 8 x 640 x 480 part streams of each kind with every role on a new-format HAAR cascade (nvca_part_stream_create_any),
    device frames, one nvca_part_batch_process a tick: the cascades opted in, the same streams on cascades not opted in, and the
    opted-in ones with "roi" = 0.

Median (min, max) over --repeats groups, warm.  NVCA_LIB=... times another build of the library (the short-queue form off:
NVCA_BUILD_VARIANT=noshort NVCA_BUILD_FLAGS=-DNVCA_ROI_HNEW_SHORT_WIN=0).

    python scripts/bench_hnew_parts.py [--repeats 7] [--calls 4] [--wide] [--skip-chain] > profiles/r13/hnew_roi.txt
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

BASES = [(64, 48), (120, 100), (160, 90)]
SLOTS = ("cascade_roi", "cascade_strip", "resize_gray", "integral_rows")


def fmt(v, unit="us"):
    return "%.1f (%.1f, %.1f) %s" % (statistics.median(v), min(v), max(v), unit)


def _call(ctx, casc, dev, w, h, stride, sf=1.1, mn=3):
    from nubovca import capi
    buf, n = (capi.Rect * 4096)(), C.c_int()
    ctx.check(ctx.L.nvca_detect_multiscale(ctx.h, casc.h, dev.data_ptr(), w, h, stride, capi.MEM_DEVICE, sf, mn, 0, 0, 0, 0, 0, buf, 4096, C.byref(n)))
    return n.value


def small_calls(ctx, args, torch, title, xml, images):
    """images: [(base width, base height, gray)]"""
    on, off = ctx.load_cascade_xml(xml), ctx.load_cascade_xml(xml)
    on.set_small_route(1)
    print(title)
    for bw, bh, field in images:
        dev = torch.from_numpy(np.ascontiguousarray(field)).cuda()
        torch.cuda.synchronize()
        for name, casc in (("route on  (opted in)", on), ("route off (not opted in)", off)):
            wall, launches, kms = [], {}, {}
            for k in range(2):          # warm-up on sizes of their own (the kernels' first launch, the context's buffers)
                _call(ctx, casc, dev, bw - 9 - k, bh - 9, bw)
            for g in range(args.repeats):
                ctx.enable_kernel_timing(1)
                ctx.kernel_timing()
                t0 = time.perf_counter()
                n = 0
                for k in range(8):
                    for _ in range(args.calls):
                        _call(ctx, casc, dev, bw - k, bh - g, bw)
                        n += 1
                wall.append((time.perf_counter() - t0) / n * 1e6)
                for slot, (ms, cnt) in ctx.kernel_timing().items():
                    kms.setdefault(slot, []).append(ms / n * 1e3)
                    launches.setdefault(slot, []).append(cnt / n)
                ctx.enable_kernel_timing(0)
            print("  %3d x %3d  %-26s %s" % (bw, bh, name, fmt(wall)))
            for slot in kms:
                print("               %-16s %s, %.2f bookings a call" % (slot, fmt(kms[slot]), statistics.median(launches[slot])))
    on.free(); off.free()


def chain(ctx, args, torch, capi):
    import haar_new_cases as K
    import lbp_part_cases as P
    names = ("w24", "w12", "w20x28")
    opted = [ctx.load_cascade_xml(K.cascade(n)[0]) for n in names]
    plain = [ctx.load_cascade_xml(K.cascade(n)[0]) for n in names]
    for c in opted:
        c.set_small_route(1)
    frames = P.lbp_frames()
    devf = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    print("(b) 8 x 640 x 480 part streams of a kind, every role a new-format HAAR cascade (w24 face, w12 / w20x28 parts), %d frames a group; per batched call (8 frames)" % len(frames))
    for kind in ("eye", "nose", "mouth", "ear"):
        two = kind in ("eye", "ear")
        print("  %s" % kind)
        for name, cascs, opts in (("opted in", opted, {}), ("not opted in", plain, {}), ("opted in, roi 0", opted, {"roi": 0})):
            with ctx.options(**opts):
                wall, launches, kms = [], {}, {}
                for g in range(args.repeats + 1):
                    streams = [capi.PartStream(ctx, P.KINDS[kind], cascs[0], cascs[1], cascs[2] if two else None, any_format=True) for _ in range(8)]
                    ctx.enable_kernel_timing(1)
                    ctx.kernel_timing()
                    t0 = time.perf_counter()
                    for i in range(len(frames)):
                        fr = [capi.make_frame(devf[i].data_ptr(), 640, 480, 640 * 3, capi.MEM_DEVICE)] * 8
                        capi.part_batch_process(ctx, streams, fr, cap=256)
                    dt = (time.perf_counter() - t0) / len(frames) * 1e6
                    kt = ctx.kernel_timing()
                    ctx.enable_kernel_timing(0)
                    for s in streams:
                        s.close()
                    if g == 0:
                        continue          # warm-up group
                    wall.append(dt)
                    for slot in SLOTS:
                        ms, cnt = kt.get(slot, (0., 0))
                        kms.setdefault(slot, []).append(ms / len(frames) * 1e3)
                        launches.setdefault(slot, []).append(cnt / len(frames))
            print("        %-20s %s" % (name, fmt(wall)))
            for slot in SLOTS:
                if statistics.median(launches[slot]):
                    print("            %-16s %s, %.2f bookings a call" % (slot, fmt(kms[slot]), statistics.median(launches[slot])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--skip-chain", action="store_true")
    args = ap.parse_args()
    import torch
    from nubovca import capi, synth
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    print("library: %s" % os.path.relpath(capi.LIB_PATH, ROOT))
    calib = [synth.make_gray(160, 120, synth.frame_seed(7, 9300 + i), "natural") for i in range(4)]
    xml = synth.haar_new_cascade_to_xml(synth.make_haar_new_cascade(ow=12, oh=12, seed=3, stage_sizes=(2, 3, 4, 5, 6), pass_rate=0.5, calibrate_on=calib))
    images = [(bw, bh, synth.paste_lbp_faces(synth.make_gray(bw, bh, synth.frame_seed(3, bw), "natural"), [(bw // 4, bh // 4, 1.5)], 12, 12, 3)) for bw, bh in BASES]
    small_calls(ctx, args, torch, "(a) nvca_detect_multiscale, calibrated 12 x 12 new-format HAAR cascade of 5 stages, sf 1.1, min_neighbors 3, device images; per call", xml, images)
    if args.wide:
        import hnew_roi_cases as RC
        wxml, gray, _sf, _exp = RC.wide_case()
        small_calls(ctx, args, torch, "(a') the same on the 12 x 12 cascade with stages of 2, 3, 17, 33, 70 and 130 stumps", wxml, [(gray.shape[1], gray.shape[0], gray)])
    if not args.skip_chain:
        chain(ctx, args, torch, capi)


if __name__ == "__main__":
    main()
