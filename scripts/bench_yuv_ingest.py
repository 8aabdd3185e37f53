"""Frames per second of the 1080p face path for BGR, NV12 and I420 frames: the serving loop of `bench.py --host-frames` (one stream,
32 frames a call, two batches in flight through nvca_face_batch_submit / _collect, the calibrated cascade, scaleFactor 1.1) in four
settings -- frames resident in HBM, pageable host memory, page-locked host memory (nvca_host_register), and the reference's default
160-pixel shrink-first mode on pageable host frames -- plus the NVCA_K_GRAY time per 32-frame launch of each format with the
frames in HBM.  One MI355X, one process.  All three formats of a frame hold the same picture: the BGR frame is the library's own
nvca_yuv420_to_bgr of the NV12 one.

    python scripts/bench_yuv_ingest.py [--steps 12] [--sets 2] > profiles/r05/yuv_ingest.txt
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nubomedia-vca_amd"))

W, H, F = 1920, 1080, 32
FACES = [(200, 150, 300), (900, 400, 180), (1400, 100, 120), (1500, 700, 240)]
FORMATS = ["bgr", "nv12", "i420"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sets", type=int, default=2, help="frame sets cycled through (32 different frames each)")
    args = ap.parse_args()
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    os.environ.setdefault("NVCA_HOST_THREADS", str(max(0, min(7, cores - 1))))
    from nubovca import capi, synth
    pool = ThreadPoolExecutor(max(2, min(16, cores)))
    xml_job = pool.submit(synth.calibrated_cascade_xml)

    def content(t, s):
        return synth.frame_seed(0, t * F + s), [(x + 8 * s, y, sz) for (x, y, sz) in FACES]
    jobs = {(t, s): pool.submit(synth.make_yuv420, W, H, content(t, s)[0], 1, "natural", content(t, s)[1]) for t in range(args.sets) for s in range(F)}
    import torch
    torch.cuda.set_device(0)
    ctx = capi.Context(0)
    casc = ctx.load_cascade_xml(xml_job.result())
    host = {}
    layouts = {"i420": capi.pixel_layout(2, (0, W * H, W * H * 5 // 4), (W, W // 2, W // 2))}
    for (t, s), j in jobs.items():
        buf, lay = j.result()
        layouts["nv12"] = capi.pixel_layout(*lay)
        host[("nv12", t, s)] = buf
        uv = buf[W * H:].reshape(H // 2, W // 2, 2)          # the same samples, planar
        host[("i420", t, s)] = np.concatenate([buf[:W * H], uv[..., 0].reshape(-1), uv[..., 1].reshape(-1)])
    pool.shutdown()
    for t in range(args.sets):
        for s in range(F):
            host[("bgr", t, s)] = ctx.yuv420_to_bgr(host[("nv12", t, s)], W, H, layouts["nv12"])
    print("# bench_yuv_ingest: %d x %d, %d frames a call, %d frame sets, %d timed steps after %d; bytes a frame: bgr %d, nv12 %d, i420 %d"
          % (W, H, F, args.sets, args.steps, args.warmup, host[("bgr", 0, 0)].nbytes, host[("nv12", 0, 0)].nbytes, host[("i420", 0, 0)].nbytes))

    def frame_of(fmt, arr_or_ptr, mem):
        if fmt == "bgr":
            return capi.make_frame(arr_or_ptr) if mem == capi.MEM_HOST else capi.make_frame(arr_or_ptr, W, H, W * 3, capi.MEM_DEVICE)
        return capi.make_planar_frame(arr_or_ptr, W, H, layouts[fmt], mem)

    def run(fmt, setting, timing=False):
        w2p = 160 if setting == "shrink160" else W
        stream = capi.FaceStream(ctx, casc, width_to_process=w2p, multi_scale_factor=10)
        if fmt != "bgr":
            stream.set_input(layouts[fmt])
        streams = [stream] * F
        keep = None
        if setting == "hbm":
            keep = [[torch.from_numpy(host[(fmt, t, s)]).cuda() for s in range(F)] for t in range(args.sets)]
            torch.cuda.synchronize()
            frames = [[frame_of(fmt, k.data_ptr(), capi.MEM_DEVICE) for k in row] for row in keep]
        else:
            frames = [[frame_of(fmt, host[(fmt, t, s)], capi.MEM_HOST) for s in range(F)] for t in range(args.sets)]
            if setting == "pinned":
                for t in range(args.sets):
                    for s in range(F):
                        ctx.host_register(host[(fmt, t, s)])
        try:
            tick = 0
            inflight = ctx.face_batch_submit(streams, frames[0])

            def step():
                nonlocal tick, inflight
                tick += 1
                nxt = ctx.face_batch_submit(streams, frames[tick % args.sets])
                res = ctx.face_batch_collect(inflight, cap=64)
                inflight = nxt
                return res
            for _ in range(args.warmup):
                res = step()
            ctx.synchronize()
            if timing:
                ctx.enable_kernel_timing(1)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                res = step()
            ctx.synchronize()
            dt = time.perf_counter() - t0
            out = {"fps": args.steps * F / dt, "boxes_last": [len(b) for b, _ in res][:4]}
            if timing:
                kt = ctx.kernel_timing()
                ctx.enable_kernel_timing(0)
                ms, n = kt["gray_resize_hist"]
                out["gray_ms_per_launch"], out["gray_launches"] = ms / max(n, 1), n
            ctx.face_batch_collect(inflight, cap=64)
            return out
        finally:
            if setting == "pinned":
                for t in range(args.sets):
                    for s in range(F):
                        ctx.host_unregister(host[(fmt, t, s)])
            stream.close()
            del keep

    results = {}
    for setting in ("hbm", "pageable", "pinned", "shrink160"):
        for fmt in FORMATS:
            r = run(fmt, setting)
            results[(setting, fmt)] = r
            print("%-10s %-5s %10.1f frames/s   boxes of the last call's first frames %s" % (setting, fmt, r["fps"], r["boxes_last"]), flush=True)
    for fmt in FORMATS:          # event-carrying launches do not overlap their neighbours: a run of its own, its rate is not a result
        r = run(fmt, "hbm", timing=True)
        results[("gray", fmt)] = r
        print("NVCA_K_GRAY hbm %-5s %8.4f ms per 32-frame launch (%d launches)" % (fmt, r["gray_ms_per_launch"], r["gray_launches"]), flush=True)
    g = {f: results[("gray", f)]["gray_ms_per_launch"] for f in FORMATS}
    print("condition NV12 K_GRAY <= BGR K_GRAY: %s (%.4f vs %.4f ms)" % ("met" if g["nv12"] <= g["bgr"] else "NOT met", g["nv12"], g["bgr"]))
    for setting in ("pageable", "pinned", "shrink160"):
        a, b = results[(setting, "nv12")]["fps"], results[(setting, "bgr")]["fps"]
        print("condition NV12 frames/s >= BGR frames/s, %s: %s (%.1f vs %.1f, x%.2f)" % (setting, "met" if a >= b else "NOT met", a, b, a / b))
    ctx.close()


if __name__ == "__main__":
    main()
