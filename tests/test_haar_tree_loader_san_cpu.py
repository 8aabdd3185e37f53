"""The cascade loader (csrc/cascade_xml.cpp) with NVCA_LOAD_HAAR_GENERAL and the table builder of a general scan (csrc/hgen_tables.cpp)
under AddressSanitizer + UndefinedBehaviorSanitizer: tests/san/hgen_tables_driver.cpp, a stand-alone program built and run as
tests/test_haar_new_loader_san_cpu.py builds its driver (no preload, nothing loaded into Python, no HIP include path).  It parses the
golden file, the synthetic cascades of both styles, a converted old-format cascade, a stump file with and without the flag, the
refusals of tests/haar_tree_cases.py and 300 files with random byte damage, each from a heap block of exactly the file's size.  The
model and the tables it prints for the good files are compared, field by field, with a statement written here from the record
comments of csrc/device_records.h."""
import json
import os
import subprocess

import numpy as np
import pytest

import haar_tree_cases as K
import haar_tree_reference as R
import lbp_cases as LK
from nubovca import capi, synth
from test_haar_tree_cpu import GOLDEN, STATUS
from test_lbp_loader_san_cpu import _damaged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
GOOD = ["golden", "t20-traincascade", "t24-minimal", "deep4-traincascade", "w82-minimal", "converted"]


def _build_driver():
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "hgen_tables_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "hgen_tables_driver.cpp")] + [os.path.join(csrc, f) for f in ("cascade_xml.cpp", "pyr_levels.cpp", "lbp_tables.cpp", "hnew_tables.cpp", "hgen_tables.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in ("cascade_model.h", "device_records.h", "pyr_levels.h", "lbp_tables.h", "hnew_tables.h", "hgen_tables.h", "host_math.h")] + \
        [os.path.join(ROOT, "include", "nubovca.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory, small_xml):
    """({case: the driver's answer}, {case: (status, format, shape, general) expected, or None where only a clean return is asked}, files)"""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    tmp = tmp_path_factory.mktemp("haar_tree_loader_san")
    driver = _build_driver()
    G = capi.LOAD_HAAR_GENERAL
    files, expected = {}, {}

    def add(cid, data, flags, exp):
        files[cid] = (flags, data if isinstance(data, bytes) else data.encode())
        expected[cid] = exp
    add("golden", open(GOLDEN, "rb").read(), G, (capi.OK, capi.CASCADE_HAAR_NEW, [20, 20, 2, 5], True))
    for name, kw in K.CASCADES.items():
        for style in ("traincascade", "minimal"):
            shape = [kw["ow"], kw["oh"], len(kw["stage_sizes"]), sum(kw["stage_sizes"])]
            add("%s-%s" % (name, style), K.cascade(name, style)[0], G, (capi.OK, capi.CASCADE_HAAR_NEW, shape, True))
            add("plain-%s-%s" % (name, style), K.cascade(name, style)[0], 0, (capi.ERR_UNSUPPORTED, -1, [0, 0, 0, 0], False))
    add("converted", synth.haar_old_xml_to_tree_xml(synth.generic_cascade_xml()), G, (capi.OK, capi.CASCADE_HAAR_NEW, [20, 20, 7, 111], True))
    add("stumps-flagged", K.stump_xml(), G, (capi.OK, capi.CASCADE_HAAR_NEW, [24, 24, 10, 72], False))
    add("stumps-plain", K.stump_xml(), 0, (capi.OK, capi.CASCADE_HAAR_NEW, [24, 24, 10, 72], False))
    add("old-format", small_xml, G, (capi.OK, capi.CASCADE_HAAR, [20, 20, 6, 83], False))
    add("lbp", LK.cascade("w12")[0], G, (capi.OK, capi.CASCADE_LBP, [12, 12, 5, 20], False))
    add("fifteen-nodes", K.fifteen_node_chain(), G, (capi.OK, capi.CASCADE_HAAR_NEW, [4, 4, 1, 1], True))
    for cid, xml, status in K.refusal_cases():
        add("refuse-" + cid, xml, G, (STATUS[status], -1, [0, 0, 0, 0], False))
    for i, b in enumerate(_damaged(K.cascade("deep4")[0].encode(), 300, 79)):
        add("damaged-%03d" % i, b, G, None)
    lines = []
    for cid, (flags, data) in files.items():
        path = str(tmp / (cid + ".xml"))
        with open(path, "wb") as f:
            f.write(data)
        lines.append("%s %d %s" % (cid, flags, path))
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
    assert set(got) == set(expected) and len(got) > 330


def test_statuses_shapes_and_generality(run):
    got, expected, _ = run
    bad = [c for c, e in expected.items() if e is not None and (got[c]["rc"], got[c]["format"], got[c]["shape"], got[c]["general"]) != e]
    assert not bad, [(c, got[c]["rc"], got[c]["format"], got[c]["shape"], got[c]["general"]) for c in bad[:5]]
    assert all(got[c]["err"] for c in got if c.startswith("refuse-") or c.startswith("plain-"))
    assert all(("tables" in got[c]) == got[c]["general"] for c in got)


def test_damaged_files_return_a_status_with_a_text(run):
    got, _, _ = run
    d = [o for c, o in got.items() if c.startswith("damaged-")]
    assert len(d) == 300 and all(o["rc"] in (capi.OK, capi.ERR_PARSE, capi.ERR_UNSUPPORTED) and (o["rc"] == capi.OK) == (not o["err"]) for o in d)
    assert any(o["rc"] == capi.ERR_PARSE for o in d)


def _corners(rect, tilted, pitch):
    x, y, w, h = (int(v) for v in rect)
    if tilted:          # CV_TILTED_PTRS: (x, y), (x - h, y + h), (x + w, y + w), (x + w - h, y + w + h)
        return [y * pitch + x, (y + h) * pitch + x - h, (y + w) * pitch + x + w, (y + w + h) * pitch + x + w - h]
    return [y * pitch + x, y * pitch + x + w, (y + h) * pitch + x, (y + h) * pitch + x + w]


@pytest.mark.parametrize("cid", GOOD)
def test_model_and_tables_of_a_good_file(run, cid):
    """the model: what the tree dump states.  HgenNodeDev: per rect its four corners at the planes' pitch (off) and at the tile's (offt), a
    missing rect four zeros and weight 0; left / right the child's index in the WHOLE node table, or -1 with the leaf's value in lv[];
    HgenWeakDev: first node and node count; the stages index the weak table"""
    got, _, files = run
    ref = R.parse_xml(files[cid][1].decode())
    m, t = got[cid]["model"], got[cid]["tables"]
    assert m["tilted"] == ref.tilted.tolist() and m["node_counts"] == ref.node_counts.tolist()
    assert [n[:3] for n in m["nodes"]] == ref.nodes.tolist() and [np.float32(n[3]) for n in m["nodes"]] == ref.node_thr.tolist()
    assert [np.float32(v) for v in m["leaves"]] == ref.leaves.tolist()
    ow, oh = ref.size
    P, TP = t["P"], t["TP"]
    assert t["rc"] == 0 and TP == 62 + ow + 1 and t["stump_weak"] == 0 and t["levels"] >= 1
    assert t["stages"] == len(ref.stage_sizes) and t["tile_stages"] == min(3, len(ref.stage_sizes))
    lds = TP * (30 + oh + 1) * 4
    assert t["lds"] == (lds if lds <= 65536 else 0) and t["area"] == (ow - 2) * (oh - 2)
    assert t["nr"] == _corners((1, 1, ow - 2, oh - 2), False, P) and t["nrt"] == _corners((1, 1, ow - 2, oh - 2), False, TP)
    firsts = np.concatenate([[0], np.cumsum(ref.stage_sizes)[:-1]]).tolist()
    assert t["stage_first"] == [[f, int(c)] for f, c in zip(firsts, ref.stage_sizes)]
    assert t["weak"] == [[int(f), int(c)] for f, c in zip(ref.first_node, ref.node_counts)]
    assert len(t["nodes"]) == len(ref.nodes)
    for w in range(len(ref.node_counts)):
        n0, l0 = int(ref.first_node[w]), int(ref.first_leaf[w])
        for j in range(int(ref.node_counts[w])):
            d = t["nodes"][n0 + j]
            left, right, f = (int(v) for v in ref.nodes[n0 + j])
            n, tl = int(ref.rect_counts[f]), bool(ref.tilted[f])
            for key, pitch in (("off", P), ("offt", TP)):
                assert d[key] == sum((_corners(ref.rects[f, r], tl, pitch) if r < n else [0, 0, 0, 0] for r in range(3)), []), (w, j, key)
            assert [np.float32(v) for v in d["w"]] == [ref.weights[f, r] if r < n else np.float32(0) for r in range(3)]
            assert np.float32(d["thr"]) == ref.node_thr[n0 + j] and d["tilted"] == int(tl) and d["pad"] == 0
            for side, child in (("left", left), ("right", right)):
                k = 0 if side == "left" else 1
                if child > 0:
                    assert d[side] == n0 + child and d["lv"][k] == 0
                else:
                    assert d[side] == -1 and np.float32(d["lv"][k]) == ref.leaves[l0 - child]
