"""Times of the small-image LBP route (kernels_roi_lbp.hip) and of part streams on new-format LBP cascades on one MI355X.

(a) small calls: nvca_detect_multiscale (min_neighbors 3, scale factor 1.1) on a calibrated 12 x 12 LBP cascade of 5 stages and
    part-sized device images -- 64 x 48, 120 x 100, 160 x 90.  A group is eight slightly different sizes (w - k, h - g for group g),
    each called --calls times: sizes never seen before, as a part detector's face regions are, so the large-image route pays its plan
    and table builds where it has them.  Per call: host clock around the synchronous call; per kernel slot: nvca_ctx_kernel_timing
    (time and launches per call).  On this library both routes are timed on one context (option "roi" 1 / 0); a library
    without k_roi_lbp (the parent commit, NVCA_LIB=...) times the only route it has.
(b) part chain: 8 x 640 x 480 part streams of each kind with every role LBP (nvca_part_stream_create_any), device frames, through
    nvca_part_batch_process; beside it the same searches -- every stream's face pass and part searches of that frame, recorded from
    the elements' logic (tests/lbp_part_cases.py) -- issued as single nvca_detect_multiscale calls on device images, which is what a
    caller without such streams can do (and all the parent commit offers).

Median (min, max) over --repeats groups.

    python scripts/bench_lbp_parts.py [--repeats 7] [--calls 4] [--skip-chain] > profiles/r10/lbp_parts.txt
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--skip-chain", action="store_true")
    args = ap.parse_args()
    import torch
    from nubovca import capi, synth
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    if hasattr(ctx.L, "nvca_part_stream_create_any"):
        routes = [("small route (roi 1)", {"roi": 1}), ("large route (roi 0)", {"roi": 0})]
    else:
        routes = [("large route (library without k_roi_lbp)", {})]
    print("library: %s" % os.path.relpath(capi.LIB_PATH, ROOT))
    calib = [synth.make_gray(160, 120, synth.frame_seed(7, 9300 + i), "natural") for i in range(4)]
    lbp = ctx.load_cascade_xml(synth.lbp_cascade_xml(ow=12, oh=12, seed=3, stage_sizes=(2, 3, 4, 5, 6), pass_rate=0.5, calibrate_on=calib))

    # ---- (a)
    print("(a) nvca_detect_multiscale, 12 x 12 LBP cascade, sf 1.1, min_neighbors 3, device images; per call")
    for bw, bh in BASES:
        field = synth.paste_lbp_faces(synth.make_gray(bw, bh, synth.frame_seed(3, bw), "natural"), [(bw // 4, bh // 4, 1.5)], 12, 12, 3)
        dev = torch.from_numpy(np.ascontiguousarray(field)).cuda()
        torch.cuda.synchronize()
        for name, opts in routes:
            with ctx.options(**opts):
                wall, launches, kms = [], {}, {}
                # warm-up on sizes of their own (the kernels' first launch, the context's buffers)
                for k in range(2):
                    _call(ctx, lbp, dev, bw - 9 - k, bh - 9, bw)
                for g in range(args.repeats):
                    ctx.enable_kernel_timing(1)
                    t0 = time.perf_counter()
                    n = 0
                    for k in range(8):
                        for _ in range(args.calls):
                            _call(ctx, lbp, dev, bw - k, bh - g, bw)
                            n += 1
                    wall.append((time.perf_counter() - t0) / n * 1e6)
                    for slot, (ms, cnt) in ctx.kernel_timing().items():
                        kms.setdefault(slot, []).append(ms / n * 1e3)
                        launches.setdefault(slot, []).append(cnt / n)
                    ctx.enable_kernel_timing(0)
                print("  %3d x %3d  %-38s %s" % (bw, bh, name, fmt(wall)))
                for slot in kms:
                    print("               %-16s %s, %.2f bookings a call" % (slot, fmt(kms[slot]), statistics.median(launches[slot])))
    if not args.skip_chain:
        chain(ctx, args, torch, capi, single_only=not hasattr(ctx.L, "nvca_part_stream_create_any"))      # (a parent library: the single calls alone)


def _call(ctx, casc, dev, w, h, stride, sf=1.1, mn=3, mins=(0, 0)):
    import ctypes as C
    from nubovca import capi
    buf, n = (capi.Rect * 256)(), C.c_int()
    ctx.check(ctx.L.nvca_detect_multiscale(ctx.h, casc.h, dev.data_ptr() if hasattr(dev, "data_ptr") else dev, w, h, stride, capi.MEM_DEVICE, sf, mn, 0, mins[0], mins[1], 0, 0, buf, 256, C.byref(n)))
    return n.value


def _recorded_searches(ctx, cascs, kind, frames, torch):
    """per frame: [(device image tensor, x, y, w, h, stride, cascade, sf, mn, min_size)] of one stream of the kind -- the face pass and
    every part search the elements' logic issues, with the library's own answers deciding what the next frame does"""
    import lbp_part_cases as P
    calls, cur = [], []

    def det(role):
        def fn(gray, sf, mn, flags, mins, maxs):
            t = torch.from_numpy(np.ascontiguousarray(gray)).cuda()
            cur.append((t, gray.shape[1], gray.shape[0], gray.shape[1], cascs[role], sf, mn, mins))
            return ctx.detect_multiscale(cascs[role], gray, sf, mn, 0, mins, maxs, cap=1 << 12)
        return P.Detector(fn)
    two = kind in ("eye", "ear")
    h = P.Harness(kind, det(0), det(1), det(2) if two else None)
    for f in frames:
        cur = []
        h.process(f)
        calls.append(cur)
    h.close()
    return calls


def chain(ctx, args, torch, capi, single_only=False):
    import lbp_cases as K
    import lbp_part_cases as P
    cascs = [ctx.load_cascade_xml(K.cascade(n)[0]) for n in (P.FACE, P.PART_A, P.PART_B)]
    frames = P.lbp_frames()
    devf = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    print("(b) 8 x 640 x 480 part streams of a kind, every role LBP (w24 face, w12 / w20x28 parts), %d frames a group; per batched call (8 frames)" % len(frames))
    for kind in ("eye", "nose", "mouth", "ear"):
        rec = _recorded_searches(ctx, cascs, kind, frames, torch)
        nsearch = sum(len(c) for c in rec)
        rows = []
        if not single_only:
            two = kind in ("eye", "ear")
            for name, opts in (("part_batch_process, roi 1", {"roi": 1}), ("part_batch_process, roi 0", {"roi": 0})):
                with ctx.options(**opts):
                    wall, launches, kms = [], {}, {}
                    for g in range(args.repeats + 1):
                        streams = [capi.PartStream(ctx, P.KINDS[kind], cascs[0], cascs[1], cascs[2] if two else None, any_format=True) for _ in range(8)]
                        ctx.enable_kernel_timing(1)
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
                    rows.append((name, wall, kms, launches))
        # the same searches as single calls, for 8 streams
        wall = []
        for g in range(args.repeats + 1):
            t0 = time.perf_counter()
            for _ in range(8):
                for cur in rec:
                    for (t, w, h, stride, casc, sf, mn, mins) in cur:
                        _call(ctx, casc, t, w, h, stride, sf, mn, mins)
            if g:
                wall.append((time.perf_counter() - t0) / len(frames) * 1e6)
        print("  %-5s %d searches a stream over the group" % (kind, nsearch))
        for name, w, kms, launches in rows:
            print("        %-34s %s" % (name, fmt(w)))
            for slot in SLOTS:
                if statistics.median(launches[slot]):
                    print("            %-16s %s, %.2f bookings a call" % (slot, fmt(kms[slot]), statistics.median(launches[slot])))
        print("        %-34s %s" % ("single nvca_detect_multiscale calls", fmt(wall)))


if __name__ == "__main__":
    main()
