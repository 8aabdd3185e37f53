"""Times of detectMultiScale with outputRejectLevels (nvca_detect_multiscale_levels) on one MI355X, beside the plain call
(nvca_detect_multiscale) on the same cascade, image, scale factor and context in the same run:

  - the calibrated LBP cascade of scripts/bench_lbp.py,
  - the new-format HAAR stand-in of scripts/bench_haar_new.py.

A 1920 x 1080 gray image resident in HBM, scale factor 1.1, min_neighbors 3.  Per call: host clock around the synchronous entry point.
Per kernel: nvca_ctx_kernel_timing (event pairs in the dispatch packets) -- the evaluators' kernels, k_lbp_levels / k_hnew_levels among
them, are booked under cascade_strip.  Steady state: 5 untimed calls, then --repeats groups of --calls calls; median (min, max) over the
groups.  The plain figures are the single-call figures of bench_lbp.py / bench_haar_new.py, measured the same way; with NVCA_LIB naming a
library without the levels entry points (a parent commit's) the plain calls alone are timed.

    python scripts/bench_levels.py [--repeats 7] [--calls 10] > profiles/r12/levels.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nubomedia-vca_amd", "oracle", "tests", "scripts"):
    sys.path.insert(0, os.path.join(ROOT, p))

import bench_haar_new as BH          # noqa: E402  (its image, its cascades: the HAAR stand-in in the new format, bench_lbp's LBP cascade)

W, H, SF, MN = BH.W, BH.H, BH.SF, BH.MN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    from nubovca import capi
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    gray = BH.image()
    dev = torch.from_numpy(gray).cuda()
    torch.cuda.synchronize()
    new_xml, _, lbp_xml = BH.cascades()
    cap = 1 << 20
    buf, lv, wt, n = (capi.Rect * cap)(), (C.c_int * cap)(), (C.c_double * cap)(), C.c_int()
    have_levels = hasattr(ctx.L, "nvca_detect_multiscale_levels")

    def plain(casc):
        ctx.check(ctx.L.nvca_detect_multiscale(ctx.h, casc.h, dev.data_ptr(), W, H, W, capi.MEM_DEVICE, SF, MN, 0, 0, 0, 0, 0, buf, cap, C.byref(n)))
        return n.value

    def levels(casc):
        ctx.check(ctx.L.nvca_detect_multiscale_levels(ctx.h, casc.h, dev.data_ptr(), W, H, W, capi.MEM_DEVICE, SF, MN, 0, 0, 0, 0, 0, buf, lv, wt, cap, C.byref(n)))
        return n.value

    def raw_levels(casc):
        ctx.check(ctx.L.nvca_detect_raw_levels(ctx.h, casc.h, dev.data_ptr(), W, H, W, capi.MEM_DEVICE, SF, 0, 0, 0, 0, 0, buf, lv, wt, cap, C.byref(n)))
        return n.value

    def measure(call, casc):
        for _ in range(5):
            boxes = call(casc)
        wall, kern = [], []
        for _ in range(args.repeats):
            ctx.enable_kernel_timing(1)
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call(casc)
            wall.append((time.perf_counter() - t0) / args.calls * 1e3)
            kern.append({k: (ms / args.calls, cnt // args.calls) for k, (ms, cnt) in ctx.kernel_timing().items()})
            ctx.enable_kernel_timing(0)
        return boxes, wall, kern

    def report(title, boxes, wall, kern):
        ev = [g["cascade_strip"][0] for g in kern]
        print("## %s: grouped boxes %d; per call median %.3f ms (min %.3f, max %.3f) over %d groups of %d calls; evaluator (cascade_strip, %d launches a call) median %.3f ms (min %.3f, max %.3f)"
              % (title, boxes, statistics.median(wall), min(wall), max(wall), args.repeats, args.calls, kern[0]["cascade_strip"][1],
                 statistics.median(ev), min(ev), max(ev)))
        return statistics.median(wall), statistics.median(ev)

    print("# bench_levels: %d x %d gray image in HBM, scale factor %.2f, min_neighbors %d; library %s" % (W, H, SF, MN, os.path.basename(capi.LIB_PATH)))
    for name, xml in (("LBP (bench_lbp's cascade)", lbp_xml), ("HAAR, new format (bench_haar_new's stand-in)", new_xml)):
        casc = ctx.load_cascade_xml(xml)
        p = report("%s, nvca_detect_multiscale" % name, *measure(plain, casc))
        if have_levels:
            triples = raw_levels(casc)
            q = report("%s, nvca_detect_multiscale_levels (%d triples emitted before grouping)" % (name, triples), *measure(levels, casc))
            print("## %s: the levels call takes %.2f x the plain call's time, its evaluator %.2f x" % (name, q[0] / p[0], q[1] / p[1]))
        casc.free()
    ctx.close()


if __name__ == "__main__":
    main()
