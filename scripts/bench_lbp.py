"""Times of detectMultiScale on a new-format LBP cascade on one MI355X, beside the nearest path the library had before it:
CV_HAAR_SCALE_IMAGE with the calibrated Haar stand-in on the same image, scale factor and context (the same pyramid, integral and
grouping; both cascades are calibrated to pass about half of what reaches a stage).

A 1920 x 1080 gray image resident in HBM, scale factor 1.1, min_neighbors 3; a calibrated 24 x 24 LBP cascade of 20 stages and
139 weak classifiers.  Per call: host clock around the synchronous entry point.  Per kernel: nvca_ctx_kernel_timing (event pairs in
the dispatch packets) -- the LBP evaluator's three kernels are booked under cascade_strip, the level resize and integral under
resize_gray / integral_rows.  The (window, weak classifier) pairs actually evaluated are counted on the CPU: for LBP by this
script's own stage-by-stage count on tests/lbp_reference.py's pieces (stages 0 .. 2 at every grid position still alive, later stages at the visited
survivors); for Haar by the oracle's statistics (stumps evaluated by the serial scan).  Steady state: 5 untimed calls, then
--repeats groups of --calls calls; median and spread over the groups.

    python scripts/bench_lbp.py [--repeats 7] [--calls 10] > profiles/r07/lbp.txt

--batch N[,N...]: instead of the above, nvca_detect_multiscale_batch on N images -- the same cascade, the same 1080p image and seeded
siblings of it, equally spaced in one HBM allocation -- beside a loop of N nvca_detect_multiscale calls on the same images in the same
run.  Per image: host clock around the call (the loop), the evaluator's and the pyramid kernels' times; per call: the timing scopes
booked.  A library without the batch entry points runs the loops alone (the figure of a parent commit).

    python scripts/bench_lbp.py --batch 1,8,32 > profiles/r08/lbp_batch.txt
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

W, H, SF, MN = 1920, 1080, 1.1, 3
TILE_STAGES = 3          # csrc/lbp_tables.cpp, build_lbp_tables (tile_stages): stages the LDS tile kernel evaluates
STAGES = (3, 4, 4, 5, 5, 6, 6, 6, 7, 7, 7, 8, 8, 8, 8, 9, 9, 9, 10, 10)


def lbp_work(ref, gray, sf):
    """(levels, grid positions, windows the serial walk visits, (window, weak) pairs the device evaluates, raw candidates)"""
    import lbp_reference as R
    import orc
    ow, oh = ref.size
    first = np.concatenate([[0], np.cumsum(ref.stage_sizes)])
    nlev = positions = visited = pairs = raw = 0
    for factor, sz, win in R.levels(ow, oh, gray.shape[1], gray.shape[0], sf):
        lev = gray if (sz[0], sz[1]) == (gray.shape[1], gray.shape[0]) else orc.resize_linear(gray, sz[0], sz[1])
        S = orc.integral(lev)[0].astype(np.int64)
        step = 1 if factor > 2.0 else 2
        xs, ys = np.arange(0, sz[0] - ow, step), np.arange(0, sz[1] - oh, step)
        nlev += 1
        positions += len(xs) * len(ys)
        pairs += len(xs) * len(ys) * int(ref.stage_sizes[0])

        def votes(k, X, Y):
            x, y, w, h = (int(v) for v in ref.rects[ref.feature_idx[k]])
            P = [[S[Y + y + r * h, X + x + c * w] for c in range(4)] for r in range(4)]
            cell = [[P[r][c] - P[r][c + 1] - P[r + 1][c] + P[r + 1][c + 1] for c in range(3)] for r in range(3)]
            code = np.zeros(len(X), np.int64)
            for r, c, bit in R.BITS:
                code += bit * (cell[r][c] >= cell[1][1])
            word = ref.subsets[k].view(np.uint32)[code >> 5]
            return np.where((word >> (code & 31).astype(np.uint32)) & 1, ref.leaves[k, 0], ref.leaves[k, 1]).astype(np.float32)

        gx, gy = np.meshgrid(np.arange(len(xs)), np.arange(len(ys)))
        X, Y = xs[gx.ravel()], ys[gy.ravel()]
        tmp = np.zeros(len(X), np.float32)
        for k in range(int(first[0]), int(first[1])):
            tmp = (tmp + votes(k, X, Y)).astype(np.float32)
        pass0 = (tmp >= ref.stage_thr[0]).reshape(len(ys), len(xs))
        vis = np.zeros(pass0.shape, bool)
        for iy in range(len(ys)):
            vis[iy, R.walk_row(np.where(pass0[iy], 1, 0))] = True
        visited += int(vis.sum())
        # the tile kernel runs its stages (the first TILE_STAGES) on every window that is alive, visited or not; the walk drops the rest
        alive, seen = pass0.ravel(), vis.ravel()
        X, Y = X[alive], Y[alive]
        seen = seen[alive]
        for s in range(1, len(ref.stage_sizes)):
            if s == TILE_STAGES:
                X, Y = X[seen], Y[seen]
            pairs += len(X) * int(ref.stage_sizes[s])
            tmp = np.zeros(len(X), np.float32)
            for k in range(int(first[s]), int(first[s + 1])):
                tmp = (tmp + votes(k, X, Y)).astype(np.float32)
            keep = tmp >= ref.stage_thr[s]
            X, Y = X[keep], Y[keep]
            if s < TILE_STAGES:
                seen = seen[keep]
        if len(ref.stage_sizes) <= TILE_STAGES:
            X = X[seen]
        raw += len(X)
    return nlev, positions, visited, pairs, raw


PYRAMID = ("resize_gray", "integral_rows", "integral_colsum", "integral_bandscan")


def bench_batches(args, sizes):
    import torch
    from nubovca import capi, synth
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    nmax = max(sizes)
    faces = [(300, 200, 2.0), (1200, 500, 4.0), (800, 100, 1.0)]
    grays = np.stack([synth.paste_lbp_faces(synth.make_gray(W, H, synth.frame_seed(0, 1 + i), "natural"), faces, 24, 24) for i in range(nmax)])
    dev = torch.from_numpy(grays).cuda()
    torch.cuda.synchronize()
    calib = [synth.make_gray(W // 2, H // 2, synth.frame_seed(7, 9100 + i), "natural") for i in range(4)]
    lbp = ctx.load_cascade_xml(synth.lbp_cascade_xml(ow=24, oh=24, seed=4, stage_sizes=STAGES, pass_rate=0.5, calibrate_on=calib))
    have_batch = hasattr(capi.Context, "detect_multiscale_batch")
    cap = 1 << 12
    buf, cnt = (capi.Rect * (cap * nmax))(), (C.c_int * nmax)()
    ptrs = (C.c_void_p * nmax)(*[dev.data_ptr() + i * W * H for i in range(nmax)])

    def batch(n):
        ctx.check(ctx.L.nvca_detect_multiscale_batch(ctx.h, lbp.h, n, ptrs, W, H, W, capi.MEM_DEVICE, SF, MN, 0, 0, 0, 0, 0, buf, cap, cnt))
        return [cnt[i] for i in range(n)]

    def loop(n):
        out = []
        for i in range(n):
            ctx.check(ctx.L.nvca_detect_multiscale(ctx.h, lbp.h, ptrs[i], W, H, W, capi.MEM_DEVICE, SF, MN, 0, 0, 0, 0, 0, buf, cap, cnt))
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
        for k in sorted(kern[0]):
            v = [g[k][0] for g in kern]
            print("  %-18s %8.3f ms an image (min %.3f, max %.3f), %d scopes a round" % (k, statistics.median(v), min(v), max(v), kern[0][k][1]))
        for name, ks in (("evaluator (cascade_strip)", ("cascade_strip",)), ("pyramid (%s)" % " + ".join(PYRAMID), PYRAMID)):
            v = [sum(g[k][0] for k in ks if k in g) for g in kern]
            print("  %s: median %.3f ms an image (min %.3f, max %.3f)" % (name, statistics.median(v), min(v), max(v)))
        return statistics.median(wall), min(wall), max(wall)

    print("# bench_lbp --batch: %d x %d gray images in HBM (one allocation, equally spaced), scale factor %.2f, min_neighbors %d; 24 x 24 LBP cascade, %d stages"
          % (W, H, SF, MN, len(STAGES)))
    if not have_batch:
        print("# this library has no nvca_detect_multiscale_batch: loops of single calls alone")
    for n in sizes:
        single = report("loop of %d nvca_detect_multiscale calls" % n, n, *measure(loop, n))
        if have_batch:
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
    import lbp_reference as R
    import orc
    from nubovca import capi, synth
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    gray = synth.make_gray(W, H, synth.frame_seed(0, 1), "natural")
    gray = synth.paste_lbp_faces(gray, [(300, 200, 2.0), (1200, 500, 4.0), (800, 100, 1.0)], 24, 24)
    dev = torch.from_numpy(gray).cuda()
    torch.cuda.synchronize()
    calib = [synth.make_gray(W // 2, H // 2, synth.frame_seed(7, 9100 + i), "natural") for i in range(4)]
    lbp_xml = synth.lbp_cascade_xml(ow=24, oh=24, seed=4, stage_sizes=STAGES, pass_rate=0.5, calibrate_on=calib)
    haar_xml = synth.calibrated_cascade_xml()
    lbp, haar = ctx.load_cascade_xml(lbp_xml), ctx.load_cascade_xml(haar_xml)
    ref = R.parse_xml(lbp_xml)
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

    print("# bench_lbp: %d x %d gray image in HBM, scale factor %.2f, min_neighbors %d" % (W, H, SF, MN))
    nlev, positions, visited, pairs, raw = lbp_work(ref, gray, SF)
    print("LBP cascade: 24 x 24, %d stages, %d weak classifiers; %d levels, %d grid positions, %d windows visited by the serial walk, %d raw candidates"
          % (len(ref.stage_sizes), int(ref.stage_sizes.sum()), nlev, positions, visited, raw))
    b, wall, kern = measure(lbp, 0)
    lbp_ns = report("LBP (new format), nvca_detect_multiscale", b, wall, kern, ["cascade_strip"], pairs)
    oc = orc.parse_cascade_xml(haar_xml)
    _, st = orc.detect_raw(oc, gray, SF, capi.HAAR_SCALE_IMAGE, return_stats=True)
    print("Haar cascade (calibrated stand-in): %d stages; %d levels, %d windows visited, %d raw candidates" % (oc.c.n_stages, st.n_scales, st.windows, st.raw_hits))
    b, wall, kern = measure(haar, capi.HAAR_SCALE_IMAGE)
    haar_ns = report("Haar (old format), NVCA_HAAR_SCALE_IMAGE", b, wall, kern, ["cascade_stage0", "cascade_tile", "cascade_band", "cascade_strip", "cascade_deep"], int(st.stumps))
    print("## LBP evaluator time per evaluated (window, weak) pair is %.2f x the Haar SCALE_IMAGE evaluator's: %s"
          % (lbp_ns / haar_ns, "WORSE than the yardstick" if lbp_ns > haar_ns else "no worse than the yardstick"))
    ctx.close()


if __name__ == "__main__":
    main()
