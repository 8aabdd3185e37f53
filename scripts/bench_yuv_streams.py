"""Packed, NV12 and I420 frames on the two multi-element workloads, each leg measuring the three formats in one run on one MI355X:

  trackers   8 x 1080p NuboTracker streams in one nvca_tracker_batch_process a tick, frames resident in HBM and in pageable host memory
             (packed = BGRA, 4 bytes a pixel; 4:2:0 = 1.5);
  roi chain  8 x 1080p video streams x (eye + nose + mouth + ear detector, own face pass each) in one nvca_part_batch_process a tick,
             frames resident in HBM (packed = BGR).

The scene is static but for two faces that move 8 pixels a frame (what a tracker is for; a scene that changes everywhere is bound
by the component kernels, not by the pixel pass).  Frames per second, and from a run of its own with kernel timing on (event-carrying launches do not overlap their neighbours: its rate
is not a result) the NVCA_K_TRACKER, NVCA_K_RESIZE1 and NVCA_K_GRAY times per tick.  NVCA_K_TRACKER covers the pixel pass AND the
component kernels; the gray values are the same in all three formats, so the component kernels do the same work and the difference
between formats is the pixel pass's.  All formats of a frame hold the same picture: the packed frame is the library's own
nvca_yuv420_to_bgr of the NV12 one.  The box / part count that ends a line is that of one tick at the line's own phase of the frame cycle: it shows
that the work is real, it is not a comparison between formats.  Which pixel / gray kernel a 4:2:0 launch took is read from the library's plan_debug lines.

    python scripts/bench_yuv_streams.py [--steps 40] > profiles/r05/yuv_streams.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nubomedia-vca_amd"))

W, H, V, NF = 1920, 1080, 8, 12
FACES = [(150, 200, 560), (1100, 260, 620)]          # as scripts/bench_roi_chain.py: faces whose parts reach the part cascades' windows
FORMATS = ["packed", "nv12", "i420"]
KINDS = [(0, "righteye", "lefteye"), (1, "nose", None), (2, "mouth", None), (3, "leftear", "rightear")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    import torch
    from nubovca import capi, synth
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    layouts = {"i420": capi.pixel_layout(2, (0, W * H, W * H * 5 // 4), (W, W // 2, W // 2))}
    host = {}
    for i in range(NF):
        buf, lay = synth.make_yuv420(W, H, 40, 1, "natural", [(x + 8 * i, y, s) for x, y, s in FACES])       # one seed: a static scene, the faces move
        layouts["nv12"] = capi.pixel_layout(*lay)
        uv = buf[W * H:].reshape(H // 2, W // 2, 2)          # the same samples, planar
        bgr = ctx.yuv420_to_bgr(buf, W, H, layouts["nv12"])
        host[("nv12", i)] = buf
        host[("i420", i)] = np.concatenate([buf[:W * H], uv[..., 0].reshape(-1), uv[..., 1].reshape(-1)])
        host[("bgr", i)] = bgr
        host[("bgra", i)] = np.concatenate([bgr, np.full((H, W, 1), 255, np.uint8)], axis=2)
    print("# bench_yuv_streams: %d x %d, %d streams, %d distinct frames, %d timed ticks after %d" % (W, H, V, NF, args.steps, args.warmup))

    def frames_of(fmt, bpp, mem):
        """[frame] per distinct picture, and what keeps device copies alive"""
        key = fmt if fmt != "packed" else ("bgra" if bpp == 4 else "bgr")
        keep = [torch.from_numpy(host[(key, i)]).cuda() for i in range(NF)] if mem == "hbm" else None
        torch.cuda.synchronize()
        out = []
        for i in range(NF):
            src = keep[i].data_ptr() if keep else host[(key, i)]
            m = capi.MEM_DEVICE if keep else capi.MEM_HOST
            if fmt == "packed":
                out.append(capi.make_frame(src, W, H, W * bpp, m) if keep else capi.make_frame(src))
            else:
                out.append(capi.make_planar_frame(src, W, H, layouts[fmt], m))
        return out, keep

    clock = [0]                      # ticks so far: the trackers' timestamps only ever grow

    def run(tick, n):
        for _ in range(n):
            tick(clock[0])
            clock[0] += 1

    def measure(tick, names):
        run(tick, args.warmup)
        ctx.synchronize()
        t0 = time.perf_counter()
        run(tick, args.steps)
        ctx.synchronize()
        fps = args.steps * V / (time.perf_counter() - t0)
        ctx.enable_kernel_timing(1)
        run(tick, args.steps)
        ctx.synchronize()
        kt = ctx.kernel_timing()
        ctx.enable_kernel_timing(0)
        return fps, {n: kt.get(n, (0.0, 0))[0] / args.steps for n in names}

    def kernels_of(tick, prefix):
        """the kernels the library's plan_debug lines name for one tick (fd 2 is read back through a pipe)"""
        r, w = os.pipe()
        saved = os.dup(2)
        os.dup2(w, 2)
        try:
            with ctx.options(plan_debug=1):
                run(tick, 1)
        finally:
            os.dup2(saved, 2); os.close(saved); os.close(w)
        text = os.read(r, 1 << 16).decode(errors="replace")
        os.close(r)
        return sorted({ln.rsplit(": ", 1)[1] for ln in text.splitlines() if ln.startswith(prefix)})

    # ---- leg 1: trackers alone
    trk = {}
    for mem in ("hbm", "pageable"):
        for fmt in FORMATS:
            frames, keep = frames_of(fmt, 4, mem)
            trks = [capi.Tracker(ctx) for _ in range(V)]
            if fmt != "packed":
                for t in trks:
                    t.set_input(layouts[fmt])

            def tick(i):
                return capi.tracker_batch_process(ctx, trks, [frames[(i + 3 * v) % NF] for v in range(V)], [33.3 * i] * V)
            fps, kt = measure(tick, ["tracker"])
            ran = kernels_of(tick, "[nvca plan] 4:2:0 tracker pass") if fmt != "packed" else ["k_trk_pixel4"]
            boxes = sum(len(b) for b in tick(clock[0]))
            clock[0] += 1
            trk[(mem, fmt)] = (fps, kt["tracker"])
            print("trackers  %-8s %-6s %10.1f frames/s   NVCA_K_TRACKER %.4f ms a tick   pixel kernel %s   boxes of a tick %d"
                  % (mem, fmt, fps, kt["tracker"], ",".join(ran), boxes), flush=True)
            for t in trks:
                t.close()
            del keep
    a, b = trk[("hbm", "nv12")][1], trk[("hbm", "packed")][1]
    print("expectation NV12 NVCA_K_TRACKER <= BGRA NVCA_K_TRACKER, 8 x 1080p in HBM: %s (%.4f vs %.4f ms)" % ("met" if a <= b else "NOT met", a, b))

    # ---- leg 2: the ROI chain
    face_c = ctx.load_cascade_xml(synth.calibrated_cascade_xml())
    pc = {n: ctx.load_cascade_xml(synth.calibrated_part_cascade_xml(n)) for n in ("righteye", "lefteye", "nose", "mouth", "leftear", "rightear")}
    for fmt in FORMATS:
        frames, keep = frames_of(fmt, 3, "hbm")
        parts = [capi.PartStream(ctx, k, face_c, pc[a], pc[b] if b else None) for _ in range(V) for k, a, b in KINDS]
        if fmt != "packed":
            for p in parts:
                p.set_input(layouts[fmt])
        found = [0]

        def tick(i):
            res = capi.part_batch_process(ctx, parts, [frames[(i + 3 * v) % NF] for v in range(V) for _ in KINDS])
            found[0] = sum(len(x) + len(y) for x, y in res)
        fps, kt = measure(tick, ["resize_gray", "gray_resize_hist"])
        ran = kernels_of(tick, "[nvca plan] 4:2:0 eye gray") if fmt != "packed" else ["k_gray_fast4"]
        print("roi chain hbm      %-6s %10.1f frames/s   NVCA_K_RESIZE1 %.4f ms a tick   NVCA_K_GRAY %.4f ms a tick   eye gray kernel %s   parts of a tick %d"
              % (fmt, fps, kt["resize_gray"], kt["gray_resize_hist"], ",".join(ran), found[0]), flush=True)
        for p in parts:
            p.close()
        del keep
    ctx.close()


if __name__ == "__main__":
    main()
