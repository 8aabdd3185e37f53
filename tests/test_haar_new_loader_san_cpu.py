"""The cascade loader (csrc/cascade_xml.cpp) on new-format HAAR files and the table builder of their scan (csrc/hnew_tables.cpp) under
AddressSanitizer + UndefinedBehaviorSanitizer: tests/san/haar_new_loader_driver.cpp, a stand-alone program built and run as
tests/test_lbp_loader_san_cpu.py builds its driver (no preload, nothing loaded into Python, no HIP include path), parses the golden
file, the synthetic cascades of both styles, a converted old-format cascade, an LBP and an old-format file, the refusal table of
tests/test_haar_new_cpu.py and 300 files with random byte damage, each from a heap block of exactly the file's size.  The tables it
prints for the good files are compared with a statement written here from the record comments of csrc/device_records.h."""
import json
import os
import subprocess

import numpy as np
import pytest

import haar_new_cases as K
import haar_new_reference as R
import lbp_cases as LK
import test_haar_new_cpu as T
from nubovca import capi, synth
from test_lbp_loader_san_cpu import _damaged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _build_driver():
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "haar_new_loader_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "haar_new_loader_driver.cpp")] + [os.path.join(csrc, f) for f in ("cascade_xml.cpp", "pyr_levels.cpp", "lbp_tables.cpp", "hnew_tables.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in ("cascade_model.h", "device_records.h", "pyr_levels.h", "lbp_tables.h", "hnew_tables.h", "host_math.h")] + [os.path.join(ROOT, "include", "nubovca.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory, synth_xml, small_xml):
    """({case: the driver's answer}, {case: (status, format, shape) expected, or None where only a clean return is asked})"""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    tmp = tmp_path_factory.mktemp("haar_new_loader_san")
    driver = _build_driver()
    files, expected = {}, {}
    files["golden"] = open(T.GOLDEN, "rb").read()
    expected["golden"] = (capi.OK, capi.CASCADE_HAAR_NEW, [20, 20, 3, 9])
    for name, kw in K.CASCADES.items():
        for style in ("traincascade", "minimal"):
            cid = "%s-%s" % (name, style)
            files[cid] = K.cascade(name, style)[0].encode()
            expected[cid] = (capi.OK, capi.CASCADE_HAAR_NEW, [kw["ow"], kw["oh"], len(kw["stage_sizes"]), sum(kw["stage_sizes"])])
    files["converted"] = synth.haar_old_xml_to_new_xml(small_xml).encode()
    expected["converted"] = (capi.OK, capi.CASCADE_HAAR_NEW, [20, 20, 6, 83])
    files["old-format"] = synth_xml.encode()
    expected["old-format"] = (capi.OK, capi.CASCADE_HAAR, [20, 20, 22, 2135])
    files["lbp"] = LK.cascade("w12")[0].encode()
    expected["lbp"] = (capi.OK, capi.CASCADE_LBP, [12, 12, 5, 20])
    for cid, xml, status in T.refusal_table():
        files["refuse-" + cid] = xml.encode()
        expected["refuse-" + cid] = (status, -1, [0, 0, 0, 0])
    for i, b in enumerate(_damaged(K.cascade("w12")[0].encode(), 300, 78)):
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
    return got, expected, files


def test_driver_parsed_every_file_clean(run):
    got, expected, _ = run
    assert set(got) == set(expected) and len(got) > 350


def test_statuses_and_shapes(run):
    got, expected, _ = run
    bad = [c for c, e in expected.items() if e is not None and (got[c]["rc"], got[c]["format"], got[c]["shape"]) != e]
    assert not bad, [(c, got[c]) for c in bad[:5]]
    assert all(got[c]["err"] for c in got if c.startswith("refuse-"))
    assert all(("tables" in got[c]) == (got[c]["format"] == capi.CASCADE_HAAR_NEW) for c in got)


def test_damaged_files_return_a_status_with_a_text(run):
    got, _, _ = run
    d = [o for c, o in got.items() if c.startswith("damaged-")]
    assert len(d) == 300 and all(o["rc"] in (capi.OK, capi.ERR_PARSE, capi.ERR_UNSUPPORTED) and (o["rc"] == capi.OK) == (not o["err"]) for o in d)
    assert any(o["rc"] == capi.ERR_PARSE for o in d)


def _corners(rect, pitch):
    x, y, w, h = (int(v) for v in rect)
    return [y * pitch + x, y * pitch + x + w, (y + h) * pitch + x, (y + h) * pitch + x + w]


@pytest.mark.parametrize("cid", ["golden", "w24-traincascade", "w20x28-minimal", "w82-traincascade", "converted"])
def test_tables_of_a_good_file(run, cid):
    """HnewWeakDev: per rect the corners (x, y), (x + w, y), (x, y + h), (x + w, y + h) as offsets at one pitch, a missing rect four zeros and
    weight 0; normrect (1, 1, ow - 2, oh - 2) the same way; the tile pitch (32 - 1) * 2 + ow + 1; the stage-0 tile's bytes against 64 KiB"""
    got, _, files = run
    t = got[cid]["tables"]
    ref = R.parse_xml(files[cid].decode())
    ow, oh = ref.size
    assert t["rc"] == 0 and t["TP"] == 62 + ow + 1 and t["P"] >= (3 * ow if ow > 30 else 97) + 1
    assert t["stages"] == len(ref.stage_sizes) and t["tile_stages"] == min(3, len(ref.stage_sizes)) and t["scan_weak"] == 0 and t["levels"] >= 1 and t["tiles"] >= t["levels"]
    lds = t["TP"] * (30 + oh + 1) * 4
    assert t["lds"] == (lds if lds <= 65536 else 0)
    assert t["area"] == (ow - 2) * (oh - 2)
    for key, pitch, nr in (("gweak", t["P"], t["nr"]), ("tweak", t["TP"], t["nrt"])):
        assert nr == _corners((1, 1, ow - 2, oh - 2), pitch)
        assert len(t[key]) == len(ref.feature_idx)
        for k, w in enumerate(t[key]):
            f = int(ref.feature_idx[k])
            n = int(ref.rect_counts[f])
            exp = sum((_corners(ref.rects[f, r], pitch) if r < n else [0, 0, 0, 0] for r in range(3)), [])
            assert w["off"] == exp and w["pad"] == 0, (key, k)
            assert [np.float32(v) for v in w["w"]] == [ref.weights[f, r] if r < n else np.float32(0) for r in range(3)], (key, k)
            assert np.float32(w["thr"]) == ref.thr[k] and [np.float32(v) for v in w["leaf"]] == list(ref.leaves[k]), (key, k)
