"""The pyramid rules (csrc/pyr_levels.cpp) and the device tables of a new-format LBP scan (csrc/lbp_tables.cpp) on the CPU:
tests/san/lbp_tables_driver.cpp, a stand-alone program built as tests/test_lbp_loader_san_cpu.py builds its driver (AddressSanitizer +
UndefinedBehaviorSanitizer, no preload, nothing loaded into Python) and WITHOUT any HIP include path, prints what pyr_layout and
build_lbp_tables make of a cascade and an image size; every field is compared with a statement written here from the record comments
of csrc/device_records.h (LbpLevelDev, LbpTile, LbpStageDev, LbpWeakDev, lbp_tile_pitch / lbp_tile_rows, the candidate key) and from
tests/lbp_reference.py (the levels, the grid, the cascade as the reference reader keeps it)."""
import json
import os
import subprocess

import numpy as np
import pytest

import lbp_cases as K
import lbp_reference as R
from nubovca import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
REFUSAL = "scan too large for the candidate key (levels x rows x columns of windows beyond 2^32)"


def _build_driver():
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "lbp_tables_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "lbp_tables_driver.cpp")] + [os.path.join(csrc, f) for f in ("cascade_xml.cpp", "pyr_levels.cpp", "lbp_tables.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in ("cascade_model.h", "device_records.h", "pyr_levels.h", "lbp_tables.h", "host_math.h")] + [os.path.join(ROOT, "include", "nubovca.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


def _up(v, a):
    return (v + a - 1) // a * a


def _field_bits(n):
    """bits of a key field that holds 0 .. n - 1, at least one"""
    return max(1, (n - 1).bit_length())


def expected(ref, levels, cols):
    """what the driver prints for the reference reader's cascade `ref` on `levels` [(factor, (szw, szh), (winw, winh))] of a `cols` wide image"""
    ow, oh = ref.size
    P = _up(cols + 1, 8)                                      # the pitch of the full image's integral: every level's planes have it
    e = dict(levels=[[f, sz[0], sz[1], win[0], win[1]] for f, sz, win in levels], P=P, layout=[], built=bool(levels))
    gray = plane = 0
    for f, sz, win in levels:                                # level after level: gray rows of 64-byte pitch, images 256-byte aligned; planes of szh + 1 rows, 64-element aligned
        gp = _up(sz[0], 64)
        e["layout"].append([f, sz[0], sz[1], win[0], win[1], gray, gp, plane])
        gray += _up(gp * sz[1], 256)
        plane += _up(P * (sz[1] + 1), 64)
    e["gray_total"], e["plane_total"] = gray, plane
    if not levels:
        return e
    lev, tiles, bit_off, row_first, positions = [], [], 0, 0, 0
    for li, (f, sz, _win) in enumerate(levels):
        step = 1 if f > 2.0 else 2
        nx, ny = len(range(0, sz[0] - ow, step)), len(range(0, sz[1] - oh, step))          # the grid of lbp_reference.scan
        wpr = (nx + 31) // 32                                # bit gx & 31 of word gx >> 5 of the row
        lev.append([e["layout"][li][7], sz[0], sz[1], nx, ny, step, wpr, bit_off, row_first, 0])
        tiles += [[li, tx, ty, 0] for ty in range((ny + 15) // 16) for tx in range(wpr)]      # 32 x 16 grid positions from (tx * 32, ty * 16)
        bit_off += wpr * ny
        row_first += ny
        positions += nx * ny
    first = np.concatenate([[0], np.cumsum(ref.stage_sizes)])
    TP = 31 * 2 + ow + 1                                     # every corner a 32-window tile row reads at step 2
    weak = {}
    for name, pitch in (("gweak", P), ("tweak", TP)):
        weak[name] = []
        for k in range(len(ref.feature_idx)):
            x, y, w, h = (int(v) for v in ref.rects[ref.feature_idx[k]])
            weak[name].append(dict(off=[(y + r * h) * pitch + x + c * w for r in range(4) for c in range(4)], subset=[int(v) for v in ref.subsets[k]],
                                   leaf=[float(v) for v in ref.leaves[k]], pad=0))
    bx, by = _field_bits(max(l[3] for l in lev)), _field_bits(max(l[4] for l in lev))
    lds = TP * (15 * 2 + oh + 1) * 4                         # the tile's rows at step 2, 4-byte sums
    e.update(rc=0, err="", lev=lev, tiles=tiles, stages=[[int(first[i]), int(ref.stage_sizes[i]), float(ref.stage_thr[i]), 0] for i in range(len(ref.stage_sizes))],
             TP=TP, nrows=row_first, key_sy=bx, key_ss=bx + by, tile_stages=min(len(ref.stage_sizes), 3), lds=lds if lds <= 65536 else 0,
             bit_words=bit_off, positions=positions, **weak)
    return e


def _f32(o):
    """the floats of an answer as the f32 values they print"""
    for st in o.get("stages", []):
        st[2] = float(np.float32(st[2]))
    for name in ("gweak", "tweak"):
        for w in o.get(name, []):
            w["leaf"] = [float(np.float32(v)) for v in w["leaf"]]
    return o


def _edge_cascade():
    """a 12 x 12 window, two features, two stages"""
    return K.hand_cascade((12, 12), [(0, 0, 4, 4), (3, 1, 2, 3)], [(0.5, [(0, K.ODD_CODES, (1.0, -1.0)), (1, K.only_codes([31, 32]), (0.25, -0.75))]),
                                                                    (-0.5, [(1, K.EVEN_CODES, (0.5, -0.5))])])


def scan_cases():
    """(id, cascade key, cols, rows, sf, min_size, max_size)"""
    out = []
    for name in K.CASCADES:
        for cols, rows, sf in (K.IMAGES if name in ("w24", "deep") else K.SMALL_IMAGES):
            out.append(("%s-%dx%d" % (name, cols, rows), name, cols, rows, sf, (0, 0), (0, 0)))
    for cols in (74, 76, 78):
        for rows in (42, 44, 46):
            out.append(("edge-%dx%d" % (cols, rows), "edge", cols, rows, 4.0, (0, 0), (0, 0)))
    out.append(("edge-two-levels", "edge", 78, 78, 4.0, (0, 0), (0, 0)))
    out.append(("lds-80", "win80", 200, 200, 1.1, (0, 0), (0, 0)))
    out.append(("lds-84", "win84", 200, 200, 1.1, (0, 0), (0, 0)))
    for cid, cdict, (rows, cols), sf, mn, mx, _raw in K.scan_rule_cases():
        out.append(("rule-" + cid, "perm%d" % cdict["size"][0], cols, rows, sf, mn, mx))
    return out


CASCADE_XML = {}


def _xml(key):
    if not CASCADE_XML:
        CASCADE_XML.update({name: K.cascade(name)[0] for name in K.CASCADES})
        CASCADE_XML.update(edge=synth.lbp_cascade_to_xml(_edge_cascade()), win80=synth.lbp_cascade_to_xml(K.permissive(80, 80)),
                           win84=synth.lbp_cascade_to_xml(K.permissive(84, 84)), perm24=synth.lbp_cascade_to_xml(K.permissive(24, 24)),
                           perm12=synth.lbp_cascade_to_xml(K.permissive(12, 12)))
    return CASCADE_XML[key]


SI_VS_LBP = (24, 24, 36, 36, 1.5)                  # ow, oh, cols, rows, sf


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """{case: the driver's answer}"""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    tmp = tmp_path_factory.mktemp("lbp_tables")
    driver = _build_driver()
    paths = {}

    def path(key):
        if key not in paths:
            paths[key] = str(tmp / (key + ".xml"))
            with open(paths[key], "w") as f:
                f.write(_xml(key))
        return paths[key]

    lines = []
    for cid, key, cols, rows, sf, mn, mx in scan_cases():
        maxw, maxh = mx if mx[0] and mx[1] else (cols, rows)                 # as make_detect_job hands them on
        lines.append("scan %s %s %d %d %r %d %d %d %d" % (cid, path(key), cols, rows, sf, mn[0], mn[1], maxw, maxh))
    lines.append("levels refusal %s 1 70000 70000" % path("w12"))
    lines.append("levels given-two-levels %s 2 76 44 45 29" % path("edge"))
    lines.append("rules si-vs-lbp %d %d %d %d %r 0 0 %d %d" % (SI_VS_LBP + SI_VS_LBP[2:4]))
    lines.append("rules si-keeps-a-level 24 24 38 36 1.5 0 0 38 36")
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
            got[o.pop("case")] = o
    assert len(got) == len(lines)
    return got


def _diff(got, exp):
    return [k for k in sorted(set(got) | set(exp)) if got.get(k) != exp.get(k)]


@pytest.mark.parametrize("case", scan_cases(), ids=[c[0] for c in scan_cases()])
def test_tables_of_a_scan(run, case):
    cid, key, cols, rows, sf, mn, mx = case
    ref = R.parse_xml(_xml(key))
    levels = R.levels(ref.size[0], ref.size[1], cols, rows, sf, mn, mx)[:63]
    got, exp = _f32(run[cid]), _f32(expected(ref, levels, cols))
    assert not _diff(got, exp), [(k, got.get(k), exp.get(k)) for k in _diff(got, exp)[:3]]


def test_premises_of_the_cases(run):
    """the cases are what their names say"""
    n = [len(run["%s-%dx%d" % (name, c, r)]["levels"]) for name in ("w24", "deep") for c, r, _ in K.IMAGES]
    assert min(n) >= 3 and max(n) > 20                              # many levels: every cumulative field is exercised
    assert run["rule-exact-window-no-level"] == dict(levels=[], P=32, gray_total=0, plane_total=0, layout=[], built=False)      # lbp_plan builds no tables then
    assert [len(run["rule-" + c]["levels"]) for c in ("min25-1.99", "max23-1.99", "min24-2.01")] == [1, 1, 2]
    assert any(l[5] == 1 for l in run["rule-step-at-factor-2.01"]["lev"]) and all(l[5] == 2 for l in run["rule-step-at-factor-1.99"]["lev"][:2])


@pytest.mark.parametrize("cols,nx,wpr", [(74, 31, 1), (76, 32, 1), (78, 33, 2)])
@pytest.mark.parametrize("rows,ny,trows", [(42, 15, 1), (44, 16, 1), (46, 17, 2)])
def test_word_and_tile_edges(run, cols, nx, wpr, rows, ny, trows):
    """one level at factor 1 and step 2: nx = ceil((cols - 12) / 2) on both sides of a 32-position word, ny of a 16-row tile"""
    o = run["edge-%dx%d" % (cols, rows)]
    assert len(o["lev"]) == 1 and o["lev"][0][3:9] == [nx, ny, 2, wpr, 0, 0]
    assert o["tiles"] == [[0, tx, ty, 0] for ty in range(trows) for tx in range(wpr)]
    assert (o["bit_words"], o["nrows"], o["positions"]) == (wpr * ny, ny, nx * ny)
    assert (o["key_sy"], o["key_ss"]) == (5 if nx <= 32 else 6, (5 if nx <= 32 else 6) + (4 if ny <= 16 else 5))


def test_the_following_level_starts_where_the_first_ends(run):
    # 78 x 78 at sf 4: 33 x 33 positions at step 2 (2 words a row), then cvRound(19.5) = 20: 8 x 8 positions at step 1
    o = run["edge-two-levels"]
    assert [l[3:9] for l in o["lev"]] == [[33, 33, 2, 2, 0, 0], [8, 8, 1, 1, 66, 33]]
    assert len(o["tiles"]) == 2 * 3 + 1 and o["tiles"][-1] == [1, 0, 0, 0] and o["bit_words"] == 66 + 8
    # a list given directly: 32 x 16 positions (exactly one tile), then 17 x 9
    o = run["given-two-levels"]
    assert [l[3:9] for l in o["lev"]] == [[32, 16, 2, 1, 0, 0], [17, 9, 2, 1, 16, 16]] and len(o["tiles"]) == 2
    assert o["lev"][1][0] == o["layout"][1][7] == _up(80 * 45, 64)


def test_lds_boundary(run):
    # TP = 62 + window + 1, rows = 30 + window + 1: 143 * 111 * 4 = 63 492 <= 65 536 < 67 620 = 147 * 115 * 4
    assert (run["lds-80"]["TP"], run["lds-80"]["lds"]) == (143, 63492)
    assert (run["lds-84"]["TP"], run["lds-84"]["lds"]) == (147, 0)


def test_refusal(run):
    # one 70 000 x 70 000 level under a 12 x 12 window: 34 994 positions a side (16 bits each: 2^15 < 34 994 <= 2^16) and one bit of
    # level make 33 key bits; the 1.2e9 positions alone are beyond 2^30 too
    o = run["refusal"]
    assert o["lev"][0][3:5] == [34994, 34994] and 2 * _field_bits(34994) + _field_bits(1) == 33 and o["positions"] > 1 << 30
    assert o["rc"] == capi.ERR_ARG and o["err"] == REFUSAL


def test_si_levels_beside_lbp_levels(run):
    """A 24 x 24 window on 36 x 36 at sf 1.5.  Factor 1: 36 x 36, both rules take it.  Factor 1.5: 24 x 24, exactly the window: the
    new-format rule (sz - window <= 0) breaks, CV_HAAR_SCALE_IMAGE (sz - window + 1 <= 0 breaks) goes on, but its invoker returns
    early on a level no wider than the window (continue).  Factor 2.25: 16 x 16, CV_HAAR_SCALE_IMAGE breaks too."""
    o = run["si-vs-lbp"]
    assert o["lbp"] == [[1.0, 36, 36, 24, 24]] == o["si"]
    assert o["lbp"] == [[f, sz[0], sz[1], w[0], w[1]] for f, sz, w in R.levels(*SI_VS_LBP)]
    assert o["steps"] == [2, 2, 1]                   # factor > 2: every pixel


def test_si_rule_keeps_a_level_the_lbp_rule_drops(run):
    """38 x 36 under the same window: at factor 1.5 the level is 25 x 24 -- wider than the window, exactly as high.  CV_HAAR_SCALE_IMAGE
    keeps it (24 - 24 + 1 > 0, and 25 + 1 > 1 + 24 passes the invoker: a grid of one column and no row); the new-format rule breaks on
    sz - window <= 0.  At factor 2.25 (17 x 16) CV_HAAR_SCALE_IMAGE breaks too."""
    o = run["si-keeps-a-level"]
    assert o["lbp"] == [[1.0, 38, 36, 24, 24]]
    assert o["si"] == [[1.0, 38, 36, 24, 24], [1.5, 25, 24, 36, 36]]
    assert o["lbp"] == [[f, sz[0], sz[1], w[0], w[1]] for f, sz, w in R.levels(24, 24, 38, 36, 1.5)]
