"""The cascade loader (csrc/cascade_xml.cpp, both formats) under AddressSanitizer + UndefinedBehaviorSanitizer:
tests/san/lbp_loader_driver.cpp, a stand-alone program built and run as tests/test_yuv_out_san_cpu.py builds its driver (no preload,
nothing loaded into Python), parses the golden new-format file, the synthetic cascades of both styles, an old-format cascade, the
refusal table of tests/test_lbp_cpu.py and 300 files with random byte damage, each from a heap block of exactly the file's size."""
import json
import os
import subprocess

import numpy as np
import pytest

import lbp_cases as K
import test_lbp_cpu as T
from nubovca import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _build_driver():
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "lbp_loader_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "lbp_loader_driver.cpp"), os.path.join(csrc, "cascade_xml.cpp")]
    deps = srcs + [os.path.join(csrc, "cascade_model.h"), os.path.join(ROOT, "include", "nubovca.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


def _damaged(xml, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        b = bytearray(xml)
        for _k in range(int(rng.integers(1, 6))):
            mode, i = int(rng.integers(0, 3)), int(rng.integers(0, len(b)))
            if mode == 0:
                b[i] = int(rng.integers(0, 256))
            elif mode == 1:
                del b[i:i + int(rng.integers(1, 40))]
            else:
                b[i:i] = bytes(rng.integers(32, 127, int(rng.integers(1, 12))).astype(np.uint8))
        if b:
            out.append(bytes(b))
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory, synth_xml):
    """({case: the driver's answer}, {case: (status, format, shape) expected, or None where only a clean return is asked})"""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    tmp = tmp_path_factory.mktemp("lbp_loader_san")
    driver = _build_driver()
    files, expected = {}, {}
    files["golden"] = open(T.GOLDEN, "rb").read()
    expected["golden"] = (capi.OK, capi.CASCADE_LBP, [24, 24, 3, 9])
    for name, kw in K.CASCADES.items():
        for style in ("traincascade", "minimal"):
            cid = "%s-%s" % (name, style)
            files[cid] = K.cascade(name, style)[0].encode()
            expected[cid] = (capi.OK, capi.CASCADE_LBP, [kw["ow"], kw["oh"], len(kw["stage_sizes"]), sum(kw["stage_sizes"])])
    files["old-format"] = synth_xml.encode()
    expected["old-format"] = (capi.OK, capi.CASCADE_HAAR, [20, 20, 22, 2135])
    for cid, xml, status in T.refusal_table():
        files["refuse-" + cid] = xml.encode()
        expected["refuse-" + cid] = (status, -1, [0, 0, 0, 0])
    for i, b in enumerate(_damaged(K.cascade("w12")[0].encode(), 300, 77)):
        files["damaged-%03d" % i] = b
        expected["damaged-%03d" % i] = None
    lines = []
    for cid, data in files.items():
        path = str(tmp / (cid + ".xml"))
        with open(path, "wb") as f:
            f.write(data)
        lines.append("%s %s" % (cid, path))
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
    return got, expected


def test_driver_parsed_every_file_clean(run):
    got, expected = run
    assert set(got) == set(expected) and len(got) > 340


def test_statuses_and_shapes(run):
    got, expected = run
    bad = [c for c, e in expected.items() if e is not None and (got[c]["rc"], got[c]["format"], got[c]["shape"]) != e]
    assert not bad, [(c, got[c]) for c in bad[:5]]
    assert all(got[c]["err"] for c in got if c.startswith("refuse-"))


def test_damaged_files_return_a_status_with_a_text(run):
    got, _ = run
    d = [o for c, o in got.items() if c.startswith("damaged-")]
    assert len(d) == 300 and all(o["rc"] in (capi.OK, capi.ERR_PARSE, capi.ERR_UNSUPPORTED) and (o["rc"] == capi.OK) == (not o["err"]) for o in d)
    assert any(o["rc"] == capi.ERR_PARSE for o in d)
