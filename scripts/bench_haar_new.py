"""Times of detectMultiScale on a new-format HAAR cascade on one MI355X, beside two yardsticks measured in the same run on the same
image, scale factor and context:

  - CV_HAAR_SCALE_IMAGE on the SAME cascade in the old format (the calibrated Haar stand-in; synth.haar_old_xml_to_new_xml writes it in
    the new format: the same stumps, rects, weights, thresholds and votes -- the two formats are evaluated by different arithmetic, so
    the lists differ and the work is counted for each on its own);
  - the LBP evaluator on scripts/bench_lbp.py's cascade.

A 1920 x 1080 gray image resident in HBM, scale factor 1.1, min_neighbors 3.  Per call: host clock around the synchronous entry point.
Per kernel: nvca_ctx_kernel_timing (event pairs in the dispatch packets) -- the new-format evaluators' kernels are booked under
cascade_strip, the level resize and integral under resize_gray / integral_rows.  The (window, weak classifier) pairs actually evaluated
are counted on the CPU: for the new-format HAAR cascade by this script's stage-by-stage count on tests/haar_new_reference.py's pieces
(stages 0 .. 2 at every grid position still alive, later stages at the visited survivors), for LBP by bench_lbp.lbp_work, for the old
format by the oracle's statistics.  Steady state: 5 untimed calls, then --repeats groups of --calls calls; median (min, max) over the groups.

    python scripts/bench_haar_new.py [--repeats 7] [--calls 10] > profiles/r11/haar_new.txt

--batch N[,N...]: instead, nvca_detect_multiscale_batch on N images (the same image and seeded siblings, equally spaced in one HBM
allocation) beside a loop of N single calls on the same images.

    python scripts/bench_haar_new.py --batch 1,8,32 >> profiles/r11/haar_new.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("nubomedia-vca_amd", "oracle", "tests", "scripts"):
    sys.path.insert(0, os.path.join(ROOT, p))

import bench_lbp as BL          # noqa: E402  (its image, its LBP cascade, its count of the LBP evaluator's work)

W, H, SF, MN = BL.W, BL.H, BL.SF, BL.MN
TILE_STAGES = 3          # csrc/lbp_tables.cpp, build_scan_tables (tile_stages)
FACES = [(300, 200, 2.0), (1200, 500, 4.0), (800, 100, 1.0)]
PYRAMID = BL.PYRAMID


def image(i=0):
    from nubovca import synth
    return synth.paste_lbp_faces(synth.make_gray(W, H, synth.frame_seed(0, 1 + i), "natural"), FACES, 24, 24)


def hnew_work(ref, gray, sf):
    """(levels, grid positions, windows the serial walk visits, (window, weak) pairs the device evaluates, raw candidates)"""
    import haar_new_reference as R
    import orc
    ow, oh = ref.size
    first = np.concatenate([[0], np.cumsum(ref.stage_sizes)])
    nlev = positions = visited = pairs = raw = 0
    for factor, sz, win in R.levels(ow, oh, gray.shape[1], gray.shape[0], sf):
        lev = gray if (sz[0], sz[1]) == (gray.shape[1], gray.shape[0]) else orc.resize_linear(gray, sz[0], sz[1])
        S, Q = orc.integral(lev)
        step = 1 if factor > 2.0 else 2
        xs, ys = np.arange(0, sz[0] - ow, step), np.arange(0, sz[1] - oh, step)
        nlev += 1
        positions += len(xs) * len(ys)

        def rs(A, r, X, Y):
            x, y, w, h = (int(v) for v in r)
            return A[Y + y, X + x] - A[Y + y, X + x + w] - A[Y + y + h, X + x] + A[Y + y + h, X + x + w]

        def stage(s, X, Y, vnf):
            total = np.zeros(len(X), np.float64)
            for k in range(int(first[s]), int(first[s + 1])):
                f = int(ref.feature_idx[k]); w = ref.weights[f]
                ret = ((w[0] * rs(S, ref.rects[f, 0], X, Y).astype(np.float32)).astype(np.float32) + (w[1] * rs(S, ref.rects[f, 1], X, Y).astype(np.float32)).astype(np.float32)).astype(np.float32)
                if w[2] != 0:
                    ret = (ret + (w[2] * rs(S, ref.rects[f, 2], X, Y).astype(np.float32)).astype(np.float32)).astype(np.float32)
                total += np.where(ret.astype(np.float64) * vnf < np.float64(ref.thr[k]), ref.leaves[k, 0], ref.leaves[k, 1]).astype(np.float64)
            return total >= np.float64(ref.stage_thr[s])

        gx, gy = np.meshgrid(np.arange(len(xs)), np.arange(len(ys)))
        X, Y = xs[gx.ravel()], ys[gy.ravel()]
        norm = (1, 1, ow - 2, oh - 2)
        vs = rs(S, norm, X, Y).astype(np.float64)
        nf = np.float64((ow - 2) * (oh - 2)) * rs(Q, norm, X, Y) - vs * vs
        vnf = 1.0 / np.where(nf > 0, np.sqrt(np.where(nf > 0, nf, 1.0)), 1.0)
        pairs += len(X) * int(ref.stage_sizes[0])
        pass0 = stage(0, X, Y, vnf).reshape(len(ys), len(xs))
        vis = np.zeros(pass0.shape, bool)
        for iy in range(len(ys)):
            vis[iy, R.walk_row(np.where(pass0[iy], 1, 0))] = True
        visited += int(vis.sum())
        alive, seen = pass0.ravel(), vis.ravel()
        X, Y, vnf, seen = X[alive], Y[alive], vnf[alive], seen[alive]
        for s in range(1, len(ref.stage_sizes)):
            if s == TILE_STAGES:
                X, Y, vnf = X[seen], Y[seen], vnf[seen]
            pairs += len(X) * int(ref.stage_sizes[s])
            keep = stage(s, X, Y, vnf)
            X, Y, vnf = X[keep], Y[keep], vnf[keep]
            if s < TILE_STAGES:
                seen = seen[keep]
        if len(ref.stage_sizes) <= TILE_STAGES:
            X = X[seen]
        raw += len(X)
    return nlev, positions, visited, pairs, raw


def cascades():
    """(new-format HAAR xml, the same cascade's old-format xml, bench_lbp's LBP xml)"""
    from nubovca import synth
    old = synth.calibrated_cascade_xml()
    calib = [synth.make_gray(W // 2, H // 2, synth.frame_seed(7, 9100 + i), "natural") for i in range(4)]
    return synth.haar_old_xml_to_new_xml(old), old, synth.lbp_cascade_xml(ow=24, oh=24, seed=4, stage_sizes=BL.STAGES, pass_rate=0.5, calibrate_on=calib)


def bench_batches(args, sizes):
    import torch
    from nubovca import capi
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    nmax = max(sizes)
    dev = torch.from_numpy(np.stack([image(i) for i in range(nmax)])).cuda()
    torch.cuda.synchronize()
    casc = ctx.load_cascade_xml(cascades()[0])
    cap = 1 << 12
    buf, cnt = (capi.Rect * (cap * nmax))(), (C.c_int * nmax)()
    ptrs = (C.c_void_p * nmax)(*[dev.data_ptr() + i * W * H for i in range(nmax)])

    def batch(n):
        ctx.check(ctx.L.nvca_detect_multiscale_batch(ctx.h, casc.h, n, ptrs, W, H, W, capi.MEM_DEVICE, SF, MN, 0, 0, 0, 0, 0, buf, cap, cnt))
        return [cnt[i] for i in range(n)]

    def loop(n):
        out = []
        for i in range(n):
            ctx.check(ctx.L.nvca_detect_multiscale(ctx.h, casc.h, ptrs[i], W, H, W, capi.MEM_DEVICE, SF, MN, 0, 0, 0, 0, 0, buf, cap, cnt))
            out.append(cnt[0])
        return out

    def measure(fn, n):
        rounds = max(2, -(-args.calls // n))
        for _ in range(3):
            boxes = fn(n)
        wall, kern = [], []
        for _ in range(args.repeats):
            ctx.enable_kernel_timing(1)
            t0 = time.perf_counter()
            for _ in range(rounds):
                fn(n)
            wall.append((time.perf_counter() - t0) / (rounds * n) * 1e3)
            kern.append({k: (ms / (rounds * n), c // rounds) for k, (ms, c) in ctx.kernel_timing().items()})
            ctx.enable_kernel_timing(0)
        return boxes, wall, kern, rounds

    def report(title, n, boxes, wall, kern, rounds):
        print("## %s" % title)
        print("grouped boxes %s; per IMAGE (host clock, timing events on): median %.3f ms, min %.3f, max %.3f over %d groups of %d rounds of %d images"
              % (boxes if n <= 8 else "%s ..." % boxes[:8], statistics.median(wall), min(wall), max(wall), args.repeats, rounds, n))
        for name, ks in (("evaluator (cascade_strip)", ("cascade_strip",)), ("pyramid (%s)" % " + ".join(PYRAMID), PYRAMID)):
            v = [sum(g[k][0] for k in ks if k in g) for g in kern]
            print("  %s: median %.3f ms an image (min %.3f, max %.3f)" % (name, statistics.median(v), min(v), max(v)))
        return statistics.median(wall), min(wall), max(wall)

    print("# bench_haar_new --batch: %d x %d gray images in HBM (one allocation, equally spaced), scale factor %.2f, min_neighbors %d; the calibrated Haar stand-in in the new format"
          % (W, H, SF, MN))
    for n in sizes:
        single = report("loop of %d nvca_detect_multiscale calls" % n, n, *measure(loop, n))
        b = report("nvca_detect_multiscale_batch, %d images" % n, n, *measure(batch, n))
        assert batch(n) == loop(n)
        print("## %d images: batch %.3f ms an image (min %.3f, max %.3f) against %.3f (min %.3f, max %.3f) in single calls: %.2f x"
              % ((n,) + b + single + (single[0] / b[0],)))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--batch", default="", help="N[,N...]: time nvca_detect_multiscale_batch on N images beside N single calls, nothing else")
    args = ap.parse_args()
    if args.batch:
        return bench_batches(args, [int(v) for v in args.batch.split(",")])
    import torch
    import haar_new_reference as R
    import lbp_reference as LR
    import orc
    from nubovca import capi
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    gray = image()
    dev = torch.from_numpy(gray).cuda()
    torch.cuda.synchronize()
    new_xml, old_xml, lbp_xml = cascades()
    new, old, lbp = (ctx.load_cascade_xml(x) for x in (new_xml, old_xml, lbp_xml))
    cap = 1 << 16
    buf, n = (capi.Rect * cap)(), C.c_int()

    def call(casc, flags):
        ctx.check(ctx.L.nvca_detect_multiscale(ctx.h, casc.h, dev.data_ptr(), W, H, W, capi.MEM_DEVICE, SF, MN, flags, 0, 0, 0, 0, buf, cap, C.byref(n)))
        return n.value

    def measure(casc, flags):
        for _ in range(5):
            boxes = call(casc, flags)
        wall, kern = [], []
        for _ in range(args.repeats):
            ctx.enable_kernel_timing(1)
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call(casc, flags)
            wall.append((time.perf_counter() - t0) / args.calls * 1e3)
            kern.append({k: (ms / args.calls, cnt // args.calls) for k, (ms, cnt) in ctx.kernel_timing().items()})
            ctx.enable_kernel_timing(0)
        return boxes, wall, kern

    def report(title, boxes, wall, kern, evaluator, pairs):
        print("## %s" % title)
        print("grouped boxes %d; per call (host clock, timing events on): median %.3f ms, min %.3f, max %.3f over %d groups of %d calls"
              % (boxes, statistics.median(wall), min(wall), max(wall), args.repeats, args.calls))
        for k in sorted(kern[0]):
            v = [g[k][0] for g in kern]
            print("  %-18s %8.3f ms a call (min %.3f, max %.3f), %d launches a call" % (k, statistics.median(v), min(v), max(v), kern[0][k][1]))
        ev = [sum(g[k][0] for k in evaluator if k in g) for g in kern]
        per = [e * 1e6 / pairs for e in ev]              # ns per pair
        print("  evaluator (%s): median %.3f ms a call (min %.3f, max %.3f); %d (window, weak) pairs evaluated -> %.4f ns a pair (min %.4f, max %.4f)"
              % (" + ".join(evaluator), statistics.median(ev), min(ev), max(ev), pairs, statistics.median(per), min(per), max(per)))
        return statistics.median(per)

    print("# bench_haar_new: %d x %d gray image in HBM, scale factor %.2f, min_neighbors %d" % (W, H, SF, MN))
    ref = R.parse_xml(new_xml)
    nlev, positions, visited, pairs, raw = hnew_work(ref, gray, SF)
    print("new-format HAAR cascade (the calibrated stand-in, converted): %d x %d, %d stages, %d weak classifiers; %d levels, %d grid positions, %d windows visited by the serial walk, %d raw candidates"
          % (ref.size + (len(ref.stage_sizes), int(ref.stage_sizes.sum()), nlev, positions, visited, raw)))
    got = len(ctx.detect_raw(new, gray, SF, cap=1 << 18))
    print("device raw candidates %d: %s" % (got, "as counted on the statement" if got == raw else "NOT the statement's %d" % raw))
    assert got == raw
    b, wall, kern = measure(new, 0)
    new_ns = report("HAAR (new format), nvca_detect_multiscale", b, wall, kern, ["cascade_strip"], pairs)
    oc = orc.parse_cascade_xml(old_xml)
    _, st = orc.detect_raw(oc, gray, SF, capi.HAAR_SCALE_IMAGE, return_stats=True)
    print("the same cascade in the old format: %d stages; %d levels, %d windows visited, %d raw candidates" % (oc.c.n_stages, st.n_scales, st.windows, st.raw_hits))
    b, wall, kern = measure(old, capi.HAAR_SCALE_IMAGE)
    old_ns = report("Haar (old format), NVCA_HAAR_SCALE_IMAGE", b, wall, kern, ["cascade_stage0", "cascade_tile", "cascade_band", "cascade_strip", "cascade_deep"], int(st.stumps))
    lref = LR.parse_xml(lbp_xml)
    lnlev, lpos, lvis, lpairs, lraw = BL.lbp_work(lref, gray, SF)
    print("LBP cascade (bench_lbp's): 24 x 24, %d stages, %d weak classifiers; %d levels, %d grid positions, %d windows visited, %d raw candidates"
          % (len(lref.stage_sizes), int(lref.stage_sizes.sum()), lnlev, lpos, lvis, lraw))
    b, wall, kern = measure(lbp, 0)
    lbp_ns = report("LBP (new format), nvca_detect_multiscale", b, wall, kern, ["cascade_strip"], lpairs)
    print("## new-format HAAR evaluator: %.4f ns a (window, weak) pair; old-format SCALE_IMAGE evaluator %.4f (%.2f x); LBP evaluator %.4f (%.2f x)"
          % (new_ns, old_ns, new_ns / old_ns, lbp_ns, new_ns / lbp_ns))
    ctx.close()


if __name__ == "__main__":
    main()
