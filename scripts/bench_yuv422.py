"""Packed 4:2:2 frames (YUY2, UYVY) beside BGR and NV12 on the two 1080p workloads, all formats in one run on one MI355X:

  faces      32 x 1080p face streams at full resolution in one nvca_face_batch_process a tick (the calibrated cascade, scaleFactor 1.1);
  trackers   8 x 1080p NuboTracker streams in one nvca_tracker_batch_process a tick (packed = BGRA);

frames resident in HBM and in pageable host memory.  Per tick, from the kernel timers, NVCA_K_GRAY (the gray kernel: one launch of 32
frames) and NVCA_K_TRACKER (the pixel pass AND the component kernels; the gray values are the same in every format, so the component
kernels do the same work and the difference between two lines is the pixel pass's), as median (min, max) over 7 groups of ticks; frames per
second from a run of its own without timers (event-carrying launches do not overlap their neighbours).  Every format of a frame holds the
same picture: the BGR frame is the library's own nvca_yuv420_to_bgr of the NV12 one, the 4:2:2 frames repeat its chroma rows.

Each wide kernel is held against its generic form on the SAME frames in HBM: the generic form runs where the device pointer is moved 8 bytes
(gray kernels: the base term of the predicate) or 4 bytes (tracker: the 8-byte term) off alignment.  The kernel that ran is read from the
library's plan_debug lines.  A wide kernel is worth keeping where its median lies below the generic form's minimum.

    python scripts/bench_yuv422.py [--steps 8] [--groups 7] > profiles/r14/yuv422.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nubomedia-vca_amd"))

W, H, F, V, NF = 1920, 1080, 32, 8, 8
FACES = [(200, 150, 300), (900, 400, 180), (1400, 100, 120), (1500, 700, 240)]
FORMATS = ["bgr", "nv12", "yuy2", "uyvy"]
PIX = {"nv12": 1, "yuy2": 4, "uyvy": 5}
BYTES = {"bgr": 3.0, "bgra": 4.0, "nv12": 1.5, "yuy2": 2.0, "uyvy": 2.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8, help="ticks a group")
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from nubovca import capi, synth
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    casc = ctx.load_cascade_xml(synth.calibrated_cascade_xml())
    host, layouts = {}, {}
    for i in range(NF):
        buf, lay = synth.make_yuv420(W, H, 40, 1, "natural", [(x + 8 * i, y, s) for x, y, s in FACES])       # one seed: a static scene, the faces move
        layouts["nv12"] = capi.pixel_layout(*lay)
        y = buf[:W * H].reshape(H, W)
        uv = buf[W * H:].reshape(H // 2, W // 2, 2)
        u, v = np.repeat(uv[..., 0], 2, axis=0), np.repeat(uv[..., 1], 2, axis=0)
        host[("nv12", i)] = buf
        for name in ("yuy2", "uyvy"):
            b, l = synth.pack_yuv422(y, u, v, PIX[name])
            layouts[name] = capi.pixel_layout(*l)
            host[(name, i)] = b
        bgr = ctx.yuv420_to_bgr(buf, W, H, layouts["nv12"])
        assert np.array_equal(bgr, ctx.yuv422_to_bgr(host[("yuy2", i)], W, H, layouts["yuy2"])) and np.array_equal(bgr, ctx.yuv422_to_bgr(host[("uyvy", i)], W, H, layouts["uyvy"]))
        host[("bgr", i)] = bgr
        host[("bgra", i)] = np.concatenate([bgr, np.full((H, W, 1), 255, np.uint8)], axis=2)
    print("# bench_yuv422: %d x %d; faces: %d streams a tick, trackers: %d; %d distinct frames; %d groups of %d ticks after %d"
          % (W, H, F, V, NF, args.groups, args.steps, args.warmup))

    def frames_of(fmt, mem, shift):
        """[frame] per distinct picture and what keeps device copies alive; shift: bytes the device pointer lies off a 256-byte boundary"""
        keep, out = [], []
        for i in range(NF):
            a = host[(fmt, i)]
            if mem == "hbm":
                t = torch.empty(a.size + shift, dtype=torch.uint8, device="cuda")
                t[shift:] = torch.from_numpy(a.reshape(-1))
                keep.append(t)
                src, m = t.data_ptr() + shift, capi.MEM_DEVICE
            else:
                src, m = a, capi.MEM_HOST
            if fmt in ("bgr", "bgra"):
                bpp = 3 if fmt == "bgr" else 4
                out.append(capi.make_frame(src, W, H, W * bpp, m) if mem == "hbm" else capi.make_frame(src))
            else:
                out.append(capi.make_planar_frame(src, W, H, layouts[fmt], m))
        torch.cuda.synchronize()
        return out, keep

    clock = [0]

    def run(tick, n):
        for _ in range(n):
            tick(clock[0])
            clock[0] += 1

    def measure(tick, name, per_tick):
        run(tick, args.warmup)
        ctx.synchronize()
        t0 = time.perf_counter()
        run(tick, args.steps * 2)
        ctx.synchronize()
        fps = args.steps * 2 * per_tick / (time.perf_counter() - t0)
        groups = []
        for _ in range(args.groups):
            ctx.enable_kernel_timing(1)
            run(tick, args.steps)
            ctx.synchronize()
            groups.append(ctx.kernel_timing().get(name, (0.0, 0))[0] / args.steps)
            ctx.enable_kernel_timing(0)
        return fps, (float(np.median(groups)), min(groups), max(groups))

    def kernels_of(tick, prefixes):
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
        return sorted({ln.rsplit(": ", 1)[1] for ln in text.splitlines() if ln.startswith(prefixes)})

    def show(work, mem, fmt, ran, fps, t, timer, extra):
        print("%-8s %-8s %-5s %-22s %10.1f frames/s   %s %.4f (%.4f, %.4f) ms a tick   %s" % (work, mem, fmt, ",".join(ran), fps, timer, t[0], t[1], t[2], extra), flush=True)

    # ---- faces
    gray = {}
    for mem, shift in (("hbm", 0), ("hbm", 8), ("pageable", 0)):
        for fmt in FORMATS:
            if shift and fmt == "bgr":
                continue
            frames, keep = frames_of(fmt, mem, shift)
            streams = [capi.FaceStream(ctx, casc, width_to_process=W, multi_scale_factor=10) for _ in range(F)]
            if fmt != "bgr":
                for s in streams:
                    s.set_input(layouts[fmt])
            found = [0]

            def tick(i):
                res = ctx.face_batch_process(streams, [frames[(i + s) % NF] for s in range(F)], cap=64)
                found[0] = sum(len(b) for b, _ in res)
            fps, t = measure(tick, "gray_resize_hist", F)
            ran = kernels_of(tick, ("[nvca plan] 4:2:0 gray", "[nvca plan] 4:2:2 gray")) if fmt != "bgr" else ["k_gray_fast4"]
            gray[(mem, shift, fmt)] = t
            show("faces", mem, fmt, ran, fps, t, "NVCA_K_GRAY", "boxes of a tick %d" % found[0])
            for s in streams:
                s.close()
            del keep
    # ---- trackers
    trk = {}
    for mem, shift in (("hbm", 0), ("hbm", 4), ("pageable", 0)):
        for fmt in ("bgra", "nv12", "yuy2", "uyvy"):
            if shift and fmt == "bgra":
                continue
            frames, keep = frames_of(fmt, mem, shift)
            trks = [capi.Tracker(ctx) for _ in range(V)]
            if fmt != "bgra":
                for t_ in trks:
                    t_.set_input(layouts[fmt])
            boxes = [0]

            def tick(i):
                boxes[0] = sum(len(b) for b in capi.tracker_batch_process(ctx, trks, [frames[(i + 3 * v) % NF] for v in range(V)], [33.3 * i] * V))
            fps, t = measure(tick, "tracker", V)
            ran = kernels_of(tick, ("[nvca plan] 4:2:0 tracker pass", "[nvca plan] 4:2:2 tracker pass")) if fmt != "bgra" else ["k_trk_pixel4"]
            trk[(mem, shift, fmt)] = t
            show("trackers", mem, fmt, ran, fps, t, "NVCA_K_TRACKER", "boxes of a tick %d" % boxes[0])
            for t_ in trks:
                t_.close()
            del keep

    # ---- what each wide kernel is held against
    def line(what, a, b, note):
        print("%s: %.4f (%.4f, %.4f) against %.4f (%.4f, %.4f) ms, ratio of medians %.2f%s" % ((what,) + a + b + (a[0] / b[0], note)))
    for fmt in ("yuy2", "uyvy"):
        line("k_gray_yuv422_16 %s against k_gray_yuv16 nv12, hbm (2 bytes a pixel against 1.5: expect about 1.33)" % fmt, gray[("hbm", 0, fmt)], gray[("hbm", 0, "nv12")], "")
        a, b = gray[("hbm", 0, fmt)], gray[("hbm", 8, fmt)]
        line("k_gray_yuv422_16 %s against k_gray_yuv422_generic on the same frames, hbm" % fmt, a, b, "   keep the wide kernel (median below the generic minimum): %s" % ("yes" if a[0] < b[1] else "NO"))
        a, b = trk[("hbm", 0, fmt)], trk[("hbm", 4, fmt)]
        line("k_trk_pixel_yuv422x4 %s against k_trk_pixel_yuv422 on the same frames, hbm (NVCA_K_TRACKER)" % fmt, a, b, "   keep the wide kernel (median below the generic minimum): %s" % ("yes" if a[0] < b[1] else "NO"))
        line("tracker %s against nv12 (k_trk_pixel_yuv8), hbm (NVCA_K_TRACKER)" % fmt, trk[("hbm", 0, fmt)], trk[("hbm", 0, "nv12")], "")
    ctx.close()


if __name__ == "__main__":
    main()
