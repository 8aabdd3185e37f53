"""The host loops of the way out in 4:2:0 (csrc/yuv_out_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer:
tests/san/yuv_out_driver.cpp, a stand-alone program built and run as tests/test_part_logic_cpu.py builds its driver (no preload,
nothing loaded into Python), runs the case table of tests/yuv_out_cases.py -- and the conversion's host statement -- on frame
buffers that end with the last plane's last byte, and prints a checksum per case that must be the numpy statement's
(tests/yuv_out_reference.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import yuv_out_cases as K
import yuv_out_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
# (w, h, channels, bytes added to the source rows, layout) of the conversion cases: one block, tails, BGRA, padded rows on both sides
CONVERT = [(2, 2, 3, 0, "tight"), (18, 6, 3, 1, "padded"), (30, 10, 4, 0, "tight"), (32, 4, 4, 5, "rows"), (48, 34, 3, 0, "padded")]


def _build_driver():
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "yuv_out_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "yuv_out_driver.cpp")] + [os.path.join(csrc, f) for f in ("yuv_out_host.cpp", "plan.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        # (plan.cpp for build_resize_tab: function sections, the rest of it dropped; its headers name HIP types)
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
               "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


def _lay_words(lay):
    fmt, off, st = lay
    off, st = list(off) + [0] * (3 - len(off)), list(st) + [0] * (3 - len(st))
    return [fmt] + off + st


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """every case through the driver, once: ({case: checksum the driver printed}, {case: the statement's frame})"""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    tmp = tmp_path_factory.mktemp("yuv_out_san")
    driver = _build_driver()
    lines, expected = [], {}

    def put(name, arr):
        path = str(tmp / name)
        np.ascontiguousarray(arr, np.uint8).tofile(path)
        return path

    for fi, fmt in enumerate(K.FMTS):
        for layout in K.LAYOUTS:
            buf, lay = K.frame(fmt, layout)
            n = S.extent(K.W, K.H, lay)                      # to the exact byte: nothing behind the last plane's last row
            fpath = put("frame_%s_%s.raw" % (K.FMT_IDS[fi], layout), buf[:n])
            head = [K.W, K.H] + _lay_words(lay) + [fpath]
            for name, shapes in K.DRAW.items():
                cid = "draw-%s-%s-%s" % (name, K.FMT_IDS[fi], layout)
                words = ["draw", cid] + head + [len(shapes)]
                for (kind, x, y, w, h, col) in shapes:
                    words += [kind, x, y, w, h] + list(col)
                lines.append(" ".join(str(t) for t in words))
                expected[cid] = K.draw_expected(name, fmt, layout)[:n]
            for name, (boxes, image, ox, oy, wp, hp) in K.OVERLAY.items():
                cid = "overlay-%s-%s-%s" % (name, K.FMT_IDS[fi], layout)
                cn = 1 if image.ndim == 2 else image.shape[2]
                words = ["overlay", cid] + head + [put("image_%s.raw" % name, image), image.shape[1], image.shape[0], cn, repr(ox), repr(oy), repr(wp), repr(hp), len(boxes)]
                for b in boxes:
                    words += list(b)
                lines.append(" ".join(str(t) for t in words))
                expected[cid] = K.overlay_expected(name, fmt, layout)[:n]
            for (w, h, cn, spad, lname) in CONVERT:
                if lname != layout:
                    continue
                cid = "convert-%dx%d-c%d-%s-%s" % (w, h, cn, K.FMT_IDS[fi], layout)
                kw = dict(K.LAYOUTS[layout])
                if "luma_rows" in kw:
                    kw["luma_rows"] = h + 8
                dst, dlay = K.random_frame(w, h, fmt, 5 + w, **kw)
                dn = S.extent(w, h, dlay)
                rng = np.random.default_rng(w * h + cn)
                stride = w * cn + spad
                src = rng.integers(0, 256, (h, stride)).astype(np.uint8)
                img = src[:, :w * cn].reshape(h, w, cn)
                words = ["convert", cid, w, h] + _lay_words(dlay) + [put(cid + "_dst.raw", dst[:dn]), put(cid + "_src.raw", src.reshape(-1)[:stride * (h - 1) + w * cn]), cn, stride]
                lines.append(" ".join(str(t) for t in words))
                expected[cid] = S.convert(img, dst[:dn], w, h, dlay)
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
            got[o["case"]] = (o["bytes"], o["fnv"])
    return got, expected


def test_driver_ran_every_case_clean(run):
    got, expected = run
    assert set(got) == set(expected) and len(got) == 2 * (3 * (len(K.DRAW) + len(K.OVERLAY)) + len(CONVERT))


def test_checksums_are_the_statements(run):
    got, expected = run
    bad = [c for c in sorted(expected) if got[c] != (len(expected[c]), "%016x" % S.fnv1a(expected[c]))]
    assert not bad, bad[:10]
