"""The pure host side of the packed 4:2:2 ingest under AddressSanitizer + UndefinedBehaviorSanitizer: tests/san/yuv422_layout_driver.cpp,
a stand-alone program built and run as tests/test_trk_host_cpu.py builds its driver (no preload, nothing loaded into Python), answers a
manifest of cases -- the byte positions, the layout rules, yuv_extent, staged sizes, the row-run copies of a sparse ingest on buffers
that end with the last pixel, trk_wide_ok / trk_staged_bytes -- and every answer must be the one stated here."""
import json
import os
import subprocess

import numpy as np
import pytest

import yuv422_cases as K
import yuv422_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

# (w, h, offset, stride): degenerate ones first -- w = 2, h = 1, a stride of exactly 2 * w, odd heights, a base offset, padded rows
GOOD = [(2, 1, 0, 4), (2, 1, 5, 4), (2, 1, 0, 7), (2, 3, 0, 4), (34, 17, 0, 68), (34, 17, 3, 71), (160, 121, 16, 320), (1920, 1080, 0, 3840), (1920, 1080, 256, 4096)]
# (what, w, h, offset, stride) -> refused
BAD = [("odd width", 33, 17, 0, 68), ("short stride", 34, 17, 0, 67), ("zero stride", 34, 17, 0, 0), ("negative stride", 34, 17, 0, -68), ("zero width", 0, 17, 0, 68),
       ("zero height", 34, 0, 0, 68), ("negative height", 34, -1, 0, 68), ("offset out of range", 34, 17, (1 << 40) + 1, 68)]
# (w, h, offset, stride, first, period, run, count): row runs as a shrink-first resize reads them; runs that end on the last row (the copy
# must stop at the last pixel); one run; one row; count 0 = the whole plane
COPIES = [(2, 1, 0, 4, 0, 1, 1, 0), (2, 1, 3, 4, 0, 1, 1, 1), (34, 17, 0, 68, 0, 1, 17, 0), (34, 17, 5, 75, 0, 1, 17, 0), (34, 17, 0, 68, 1, 4, 2, 4), (34, 17, 0, 75, 3, 4, 2, 4),
          (34, 17, 2, 68, 15, 1, 2, 1), (34, 17, 0, 70, 0, 8, 1, 3), (1920, 1080, 0, 3840, 5, 12, 2, 90), (1920, 1080, 64, 3872, 5, 12, 2, 90), (800, 450, 0, 1600, 2, 5, 2, 90),
          (800, 450, 0, 1600, 448, 1, 2, 1)]
# trk_wide_ok: (mem, pointer, width, offset, stride) -- mem 1 = device
WIDE = [(1, 0, 160, 0, 320), (1, 0, 162, 0, 324), (1, 0, 644, 0, 1288), (1, 0, 644, 0, 1290), (1, 0, 644, 0, 1292), (1, 0, 644, 4, 1288), (1, 4, 644, 4, 1288), (1, 4, 644, 0, 1288),
        (0, 4, 644, 0, 1288), (0, 4, 644, 4, 1288), (1, 8, 160, 8, 328), (1, 1, 160, 0, 320), (1, 0, 2, 0, 4), (1, 0, 4, 0, 8)]


def _build_driver():
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "yuv422_layout_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "yuv422_layout_driver.cpp"), os.path.join(csrc, "trk_host.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in ("trk_host.h", "trk_layout.h", "device_records.h", "yuv_layout.h", "host_math.h", "pixel_rules.h")] + [os.path.join(ROOT, "include", "nubovca.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


def _lay(off, st):
    return [off, 0, 0, st, 0, 0]


def _fnv1a(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def _copy_expected(w, h, off, st, first, period, run, count):
    """(extent, bytes copied, checksum of the copy): the source holds (i * 131 + 7) & 255 at byte i; a copied row goes with its padding unless
    it is the plane's last, which ends with its last pixel; everything else stays 0"""
    n = off + st * (h - 1) + 2 * w
    src = ((np.arange(n, dtype=np.int64) * 131 + 7) & 255).astype(np.uint8)
    dst = np.zeros(n, np.uint8)
    if count == 0:
        rows = [(0, h)]
    else:
        rows = [(first + k * period, run) for k in range(count)]
    copied = 0
    for r0, nr in rows:
        a, b = off + r0 * st, min(off + (r0 + nr) * st, n)
        assert r0 + nr <= h
        dst[a:b] = src[a:b]
        copied += b - a
    return n, copied, _fnv1a(dst)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """every case through the driver, once: {case: the JSON object it printed}"""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    tmp = tmp_path_factory.mktemp("yuv422_san")
    driver = _build_driver()
    lines = []
    for fmt in R.FMTS + [0, 1, 2, 3, 7]:
        lines.append("pos pos-%d %d" % (fmt, fmt))
    for fmt in R.FMTS:
        for k, (w, h, off, st) in enumerate(GOOD):
            lines.append(" ".join(str(t) for t in ["rules", "good-%d-%d" % (fmt, k), fmt, w, h] + _lay(off, st)))
            lines.append(" ".join(str(t) for t in ["rules", "junk-%d-%d" % (fmt, k), fmt, w, h] + [off, 1, 2, st, -5, 1]))         # planes 1 .. 2 are ignored
            lines.append(" ".join(str(t) for t in ["staged", "staged-%d-%d" % (fmt, k), fmt, st, w, h] + _lay(off, st)))
        for k, (_, w, h, off, st) in enumerate(BAD):
            lines.append(" ".join(str(t) for t in ["rules", "bad-%d-%d" % (fmt, k), fmt, w, h] + _lay(off, st)))
        for k, c in enumerate(COPIES):
            lines.append(" ".join(str(t) for t in ["copy", "copy-%d-%d" % (fmt, k), fmt] + list(c)))
        for k, (mem, ptr, w, off, st) in enumerate(WIDE):
            lines.append(" ".join(str(t) for t in ["wide", "wide-%d-%d" % (fmt, k), fmt, mem, ptr, w, st] + _lay(off, st)))
    for fmt in (3, 7, -1):
        lines.append(" ".join(str(t) for t in ["rules", "format-%d" % fmt, fmt, 34, 18] + _lay(0, 68)))
    # the tracker cases of the GPU test, as the library sees them (a device pointer on 256 bytes plus the case's shift)
    for k, c in enumerate(K.TRK_CASES):
        W, H, pad, base, shift, mem = c
        lines.append(" ".join(str(t) for t in ["wide", "trkcase-%d" % k, R.UYVY, 1 if mem == "device" else 0, 4096 + shift, W, 2 * W + pad] + _lay(base, 2 * W + pad)))
    for k, c in enumerate(K.FACE_KERNEL_CASES):
        fset, pad, base, shift, mem = c
        W, H = K.Y.SETS[fset][:2]
        lines.append(" ".join(str(t) for t in ["rules", "facecase-%d" % k, R.YUY2, W, H] + _lay(base, 2 * W + pad)))
    manifest = str(tmp / "manifest.txt")
    with open(manifest, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver, manifest], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("{"):
            o = json.loads(ln)
            got[o["case"]] = o
    assert len(got) == len(lines)
    return got


def test_byte_positions_are_the_statements(run):
    for fmt in R.FMTS:
        assert tuple(run["pos-%d" % fmt]["pos"]) == R.POS[fmt], fmt


def test_layout_rules(run):
    for fmt in R.FMTS:
        for k, (w, h, off, st) in enumerate(GOOD):
            for kind in ("good", "junk"):
                o = run["%s-%d-%d" % (kind, fmt, k)]
                assert o["fault"] == "" and o["planes"] == 1 and o["rows"] == h and o["row_bytes"] == 2 * w, o
                assert o["extent"] == off + st * (h - 1) + 2 * w == R.extent(w, h, (fmt, (off,), (st,))), o
                assert o["aligned16"] == int(off % 16 == 0 and st % 16 == 0), o
        for k, b in enumerate(BAD):
            assert run["bad-%d-%d" % (fmt, k)]["fault"] != "", b
    for fmt in (3, 7, -1):
        assert "format" in run["format-%d" % fmt]["fault"]


def test_staged_sizes_end_with_the_last_pixel(run):
    for fmt in R.FMTS:
        for k, (w, h, off, st) in enumerate(GOOD):
            o = run["staged-%d-%d" % (fmt, k)]
            ext = off + st * (h - 1) + 2 * w
            assert o["extent"] == ext and o["staged"] == (ext + 255) // 256 * 256, o


def test_row_run_copies(run):
    for fmt in R.FMTS:
        for k, c in enumerate(COPIES):
            n, copied, fnv = _copy_expected(*c)
            o = run["copy-%d-%d" % (fmt, k)]
            assert (o["bytes"], o["copied"], o["fnv"]) == (n, copied, fnv), (c, o)


def test_tracker_predicate(run):
    for fmt in R.FMTS:
        for k, (mem, ptr, w, off, st) in enumerate(WIDE):
            lay = (fmt, (off, 0, 0), (st, 0, 0))
            assert run["wide-%d-%d" % (fmt, k)]["wide"] == int(K.trk_wide(lay, w, "device" if mem else "host", ptr)), (fmt, mem, ptr, w, off, st)
    assert {run["wide-%d-%d" % (R.YUY2, k)]["wide"] for k in range(len(WIDE))} == {0, 1}
    for k, c in enumerate(K.TRK_CASES):
        assert run["trkcase-%d" % k]["wide"] == int(K.trk_kernel(c) == K.TRK_WIDE), c


def test_gray_predicates_layout_half(run):
    """yuv_layout_aligned16 on the face cases: with the pointer term and the geometry term it is tests/yuv422_cases.py's gray_wide"""
    for k, c in enumerate(K.FACE_KERNEL_CASES):
        fset, pad, base, shift, mem = c
        W = K.Y.SETS[fset][0]
        assert run["facecase-%d" % k]["aligned16"] == int(base % 16 == 0 and (2 * W + pad) % 16 == 0), c
