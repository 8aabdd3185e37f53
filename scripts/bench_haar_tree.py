"""Times of detectMultiScale on a GENERAL new-format HAAR cascade (trees, tilted features; kernels_cascade_hgen.hip) on one MI355X,
beside two yardsticks measured in the same run on the same image, scale factor and context:

  (a) CV_HAAR_SCALE_IMAGE on the SAME cascade in the old format (synth.make_generic_cascade's defaults, evaluated by k_gen_*;
      synth.haar_old_xml_to_tree_xml writes it in the new format: the same trees, rects, weights, thresholds and votes -- the two
      formats are evaluated by different arithmetic, so the lists differ and the work is counted for each on its own);
  (b) the stump evaluator (kernels_cascade_hnew.hip) on scripts/bench_haar_new.py's cascade.

bench_haar_new.py's protocol: a 1920 x 1080 gray image resident in HBM, scale factor 1.1, min_neighbors 3; per call the host clock
around the synchronous entry point, per kernel nvca_ctx_kernel_timing; 5 untimed calls, then --repeats groups of --calls calls; median
(min, max) over the groups.  The (window, node) pairs the general evaluator forms are counted on tests/haar_tree_reference.py's
statement (stats 'pairs_tile': stages 0 .. 2 at every grid position still alive; 'pairs_rest': later stages at the visited survivors),
with the oracle's tilted integral in place of the statement's own (tests/test_haar_tree_cpu.py holds the two equal; the definition's
loops are too slow for 1080p).

    python scripts/bench_haar_tree.py [--repeats 7] [--calls 10] > profiles/r15/haar_tree.txt
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

import bench_haar_new as BH          # noqa: E402  (its image, its stump cascade, its count of the stump evaluator's work)

W, H, SF, MN = BH.W, BH.H, BH.SF, BH.MN
OLD_KERNELS = ["cascade_stage0", "cascade_tile", "cascade_band", "cascade_strip", "cascade_deep"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    import haar_new_reference as HR
    import haar_tree_reference as R
    import orc
    from nubovca import capi, synth
    R.tilted_integral = orc.integral_tilted
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    gray = BH.image()
    dev = torch.from_numpy(gray).cuda()
    torch.cuda.synchronize()
    old_xml = synth.generic_cascade_xml()
    tree_xml = synth.haar_old_xml_to_tree_xml(old_xml)
    stump_xml = BH.cascades()[0]
    tree, old, stump = ctx.load_cascade_xml(tree_xml, general=True), ctx.load_cascade_xml(old_xml), ctx.load_cascade_xml(stump_xml)
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

    def report(title, boxes, wall, kern, evaluator, pairs, unit):
        print("## %s" % title)
        print("grouped boxes %d; per call (host clock, timing events on): median %.3f ms, min %.3f, max %.3f over %d groups of %d calls"
              % (boxes, statistics.median(wall), min(wall), max(wall), args.repeats, args.calls))
        for k in sorted(kern[0]):
            v = [g[k][0] for g in kern]
            print("  %-18s %8.3f ms a call (min %.3f, max %.3f), %d launches a call" % (k, statistics.median(v), min(v), max(v), kern[0][k][1]))
        ev = [sum(g[k][0] for k in evaluator if k in g) for g in kern]
        if not pairs:
            print("  evaluator (%s): median %.3f ms a call (min %.3f, max %.3f)" % (" + ".join(evaluator), statistics.median(ev), min(ev), max(ev)))
            return None
        per = [e * 1e6 / pairs for e in ev]              # ns per pair
        print("  evaluator (%s): median %.3f ms a call (min %.3f, max %.3f); %d (window, %s) pairs evaluated -> %.4f ns a pair (min %.4f, max %.4f)"
              % (" + ".join(evaluator), statistics.median(ev), min(ev), max(ev), pairs, unit, statistics.median(per), min(per), max(per)))
        return statistics.median(per)

    print("# bench_haar_tree: %d x %d gray image in HBM, scale factor %.2f, min_neighbors %d" % (W, H, SF, MN))
    ref = R.parse_xml(tree_xml)
    st = {}
    raw = R.scan(ref, gray, SF, stats=st)
    pairs = st["pairs_tile"] + st["pairs_rest"]
    print("general new-format HAAR cascade (make_generic_cascade's defaults, converted): %d x %d, %d stages, %d weak classifiers (%d of them trees), %d nodes, %d on tilted features; "
          "%d levels, %d windows visited by the serial walk, %d raw candidates; (window, node) pairs: %d in the tile stages, %d behind them"
          % (ref.size + (len(ref.stage_sizes), len(ref.node_counts), int((ref.node_counts > 1).sum()), len(ref.nodes), int(ref.tilted[ref.nodes[:, 2]].sum()),
                         st["levels"], len(st["depth"]), len(raw), st["pairs_tile"], st["pairs_rest"])))
    got = ctx.detect_raw(tree, gray, SF, cap=1 << 18)
    same = got.shape == raw.shape and (got == raw).all()
    print("device raw candidates %d: %s" % (len(got), "the statement's list" if same else "NOT the statement's %d" % len(raw)))
    assert same
    b, wall, kern = measure(tree, 0)
    tree_ns = report("general HAAR (new format, trees + tilted), nvca_detect_multiscale", b, wall, kern, ["cascade_strip"], pairs, "node")
    oc = orc.parse_cascade_xml(old_xml)
    try:
        _, ost = orc.detect_raw(oc, gray, SF, capi.HAAR_SCALE_IMAGE, return_stats=True)
        print("(a) the same cascade in the old format: %d levels, %d windows visited, %d raw candidates" % (ost.n_scales, ost.windows, ost.raw_hits))
        old_pairs = int(ost.stumps)
    except Exception as e:          # (the oracle's statistics are those of its stump walk)
        print("(a) the same cascade in the old format: no work count from the oracle (%s)" % type(e).__name__)
        old_pairs = 0
    b, wall, kern = measure(old, capi.HAAR_SCALE_IMAGE)
    old_ns = report("(a) Haar (old format, k_gen_*), NVCA_HAAR_SCALE_IMAGE", b, wall, kern, OLD_KERNELS, old_pairs, "weak")
    sref = HR.parse_xml(stump_xml)
    nlev, positions, visited, spairs, sraw = BH.hnew_work(sref, gray, SF)
    print("(b) stump cascade (bench_haar_new's): %d x %d, %d stages, %d stumps; %d levels, %d windows visited, %d raw candidates"
          % (sref.size + (len(sref.stage_sizes), int(sref.stage_sizes.sum()), nlev, visited, sraw)))
    b, wall, kern = measure(stump, 0)
    stump_ns = report("(b) HAAR (new format, stumps), nvca_detect_multiscale", b, wall, kern, ["cascade_strip"], spairs, "stump")
    print("## general evaluator: %.4f ns a (window, node) pair; stump evaluator in the same run %.4f ns a (window, stump) pair: %.2f x"
          % (tree_ns, stump_ns, tree_ns / stump_ns))
    if old_ns:
        print("## old-format k_gen_* on the same cascade: %.4f ns a pair as the oracle counts them (%.2f x)" % (old_ns, tree_ns / old_ns))
    ctx.close()


if __name__ == "__main__":
    main()
