"""The proof behind every re-ordered stage sum, on the CPU: plan.cpp's build_stage_recs (built with the product's sources through
tests/geom/stage_recs_driver.cpp) against exact rational arithmetic, for every cascade the suite loads, the order-sensitive and
vote-grid cascades of tests/stage_sum_cascades.py and a batch of edge-case stages; and, on the oracle, that re-ordering a proven
stage changes nothing while the designed cascades do change the raw candidate lists (so that their GPU comparisons in
tests/test_gpu_stage_sums.py cannot pass vacuously).

StageRec flags: bit 0 every stump has two rectangles, bit 1 (2) the votes may be summed in any order, bit 2 (4) integer votes
(pass <=> sum / 2^vote_exp >= thr_i)."""
import json
import math
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import stage_sum_cascades as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = os.path.join(ROOT, "tests", "geom")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(GEOM, "build", "stage_recs_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(GEOM, "stage_recs_driver.cpp")] + [os.path.join(csrc, f) for f in ("cascade_xml.cpp", "plan.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = [CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
               "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def stage_recs(driver, tmp_path_factory):
    d = tmp_path_factory.mktemp("stage_recs")

    def run(xmls):
        paths = []
        for i, x in enumerate(xmls):
            p = d / ("c%d_%d.xml" % (len(os.listdir(d)), i))
            p.write_text(x)
            paths.append(str(p))
        r = subprocess.run([driver] + paths, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        out = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == len(paths)
        return out
    return run


def hx(s):
    return float.fromhex(s)




def check_stage(rec, rng, draws=24):
    """one StageRec against exact arithmetic on the votes it was built from"""
    votes = [(hx(a), hx(b)) for a, b in rec["votes"]]
    st, thr = hx(rec["stage_threshold"]), hx(rec["thr"])
    assert thr == float(np.float32(np.float32(st) - np.float32(0.0001))), rec
    fl = rec["flags"]
    assert (fl & 1) == (all(n == 2 for n in rec["nrect"])), rec
    finite = all(math.isfinite(v) for ab in votes for v in ab)
    if not finite:
        assert fl & 6 == 0, rec
        return
    if fl & 4:
        assert fl & 2, rec
    if fl & 2:
        # any subset, any order: the sequential f64 sum is the exact sum
        for _ in range(draws):
            pick = [ab[rng.randrange(2)] for ab in votes]
            rng.shuffle(pick)
            s = 0.0
            for v in pick:
                s += v
            assert Fraction(s) == sum(Fraction(v) for v in pick), (rec["first"], pick[:8])
        pick = [max(ab, key=abs) for ab in votes]          # the extreme subset sum
        s = 0.0
        for v in sorted(pick, key=abs):
            s += v
        assert Fraction(s) == sum(Fraction(v) for v in pick), rec["first"]
    if fl & 4:
        e = rec["vote_exp"]
        unit = Fraction(2) ** e
        for ab in votes:
            for v in ab:
                assert (Fraction(v) / unit).denominator == 1, (v, e)
        assert sum(max(abs(Fraction(a)), abs(Fraction(b))) for a, b in votes) / unit < 2 ** 31
        ti = rec["thr_i"]
        for k in range(ti - 3, ti + 4):
            assert (k >= ti) == (k * unit >= Fraction(thr)), (k, ti, thr, e)


def check_cascade(c, rng):
    assert "error" not in c, c
    recs = c["stages"]
    for r in recs:
        check_stage(r, rng)
    run = 0
    for r in reversed(recs):
        run = run + 1 if r["flags"] & 2 else 0
        assert r["spec_run"] == run, [x["spec_run"] for x in recs]
    first = 0
    for r in recs:
        assert r["first"] == first and r["count"] == len(r["votes"])
        first += r["count"]


# ------------------------------------------------------------------ the cascades the suite loads
def suite_cascades():
    from nubovca import synth
    out = {"synthetic": lambda: synth.synthetic_cascade_xml(),
           "small": lambda: synth.synthetic_cascade_xml(seed=7, stages=[3, 8, 12, 16, 20, 24]),
           "calibrated": lambda: synth.calibrated_cascade_xml(),
           "generic": lambda: synth.generic_cascade_xml()}
    for n in ("righteye", "lefteye", "nose", "mouth", "leftear", "rightear"):
        out["part_" + n] = (lambda n=n: synth.synthetic_part_cascade_xml(n))
    for n in ("righteye", "nose"):
        out["part_calibrated_" + n] = (lambda n=n: synth.calibrated_part_cascade_xml(n))
    gold = os.path.join(ROOT, "tests", "golden")
    for f in sorted(os.listdir(gold)):
        if f.endswith(".xml"):
            out["golden_" + f] = (lambda f=f: open(os.path.join(gold, f)).read())
    return out


@pytest.mark.parametrize("name", list(suite_cascades()))
def test_suite_cascades_stage_recs(stage_recs, name):
    (c,) = stage_recs([suite_cascades()[name]()])
    check_cascade(c, random.Random(name))


# ------------------------------------------------------------------ the designed cascades
@pytest.mark.parametrize("name", S.NAMES)
def test_designed_cascades_stage_recs(stage_recs, name):
    xml, twin, _ = S.variant(name)
    c, t = stage_recs([xml, twin])
    rng = random.Random(name)
    check_cascade(c, rng)
    check_cascade(t, rng)
    flags = [r["flags"] for r in c["stages"]]
    if name in S.ORDER_STAGES:
        k = S.ORDER_STAGES[name]
        assert flags[k] & 6 == 0, flags                             # the ballast stage: neither proof
        assert all(f & 2 for i, f in enumerate(flags) if i != k), flags
        assert c["stages"][k - 1]["spec_run"] == 1 if k else True    # a round that reaches stage k - 1 stops there
    elif name == "tie":
        assert all(f & 4 for f in flags), flags
        assert all(r["thr_i"] * 2.0 ** r["vote_exp"] == hx(r["thr"]) for r in c["stages"])     # every threshold on the grid
    elif name == "tie_f64":
        assert all(f & 6 == 2 for f in flags), flags               # order-free, not integer
        assert all(hx(r["thr"]) == S.TIE_BALLAST for r in c["stages"])
    else:
        r = c["stages"][S.CUT_STAGE]
        votes = [(hx(a), hx(b)) for a, b in r["votes"]]
        units = sum(max(abs(Fraction(a)), abs(Fraction(b))) for a, b in votes) / Fraction(S.GRID)
        assert units == (S.INT_CUT - 1 if name == "cut_lo" else S.INT_CUT)
        assert r["flags"] & 6 == (6 if name == "cut_lo" else 2), r["flags"]
        assert all(f & 4 for i, f in enumerate(flags) if i != S.CUT_STAGE), flags


@pytest.mark.parametrize("part", ["righteye", "lefteye", "nose"])
@pytest.mark.parametrize("kind", ["order", "tie"])
def test_part_variants_stage_recs(stage_recs, part, kind):
    xml, twin, _ = S.part_variant(part, kind)
    c, t = stage_recs([xml, twin])
    check_cascade(c, random.Random(part + kind))
    check_cascade(t, random.Random(part + kind))
    flags = [r["flags"] for r in c["stages"]]
    if kind == "order":
        assert flags[S.PART_ORDER_STAGE] & 6 == 0, flags
    else:
        assert all(f & 4 for f in flags), flags


def test_face_variant_stage_recs(stage_recs, calibrated_xml):
    (c,) = stage_recs([S.face_variant(calibrated_xml)])
    check_cascade(c, random.Random(5))
    flags = [r["flags"] for r in c["stages"]]
    assert flags[S.FACE_ORDER_STAGE] & 6 == 0 and flags[S.FACE_TIE_STAGE] & 4, flags


# ------------------------------------------------------------------ edge cases of the proof
def _stage(votes, st_thr, seed=0):
    """a stump-form stage with the given (left, right) votes (features and stump thresholds drawn as make_cascade does)"""
    from nubovca import synth
    rng = np.random.default_rng(seed)
    feats = [synth._rand_feature(rng, 20) for _ in votes]
    return dict(features=feats, thresholds=[0.1] * len(votes), left=[a for a, _ in votes], right=[b for _, b in votes],
                stage_threshold=st_thr)


def edge_stages():
    tiny = float(np.float32(1e-45))                 # the smallest f32 subnormal, 2^-149
    p = lambda k: 2.0 ** k
    return {
        "mixed_exponents": [_stage([(p(-20), -p(10)), (p(3), p(-7)), (-0.75, 0.5)], 0.3)],
        "signed_zeros": [_stage([(0.0, -0.0), (-0.0, 1.0), (0.25, 0.0)], -0.1)],
        "all_zero": [_stage([(0.0, 0.0), (-0.0, -0.0)], 0.0), _stage([(0.0, -0.0)], -1.0)],
        "subnormals": [_stage([(tiny, -3 * tiny), (p(-130), -tiny)], -1e-40), _stage([(tiny, 1.0)], 0.5),
                       _stage([(tiny, -tiny)], 0.0)],
        "flt_max": [_stage([(FLT_MAX, -FLT_MAX), (1.0, -1.0)], 0.0), _stage([(FLT_MAX, FLT_MAX)], FLT_MAX)],
        "negative_thresholds": [_stage([(-0.5, 0.25), (0.125, -1.0)], -0.875), _stage([(-3.0, 1.0)], -2.9999),
                                _stage([(-p(20), p(20))], -float(p(21)))],
        # |votes| summing to one below / one above 2^52 and 2^53 (integer votes: emin 0)
        "bound_2^52-1": [_stage([(p(k), -p(k)) for k in range(52)], 0.5)],
        "bound_2^52+1": [_stage([(p(52), -p(52)), (1.0, -1.0)], 0.5)],
        "bound_2^53-1": [_stage([(p(k), -p(k)) for k in range(53)], 0.5)],
        "bound_2^53+1": [_stage([(p(53), -p(53)), (1.0, -1.0)], 0.5)],
        # the integer cut: |votes| / 2^-3 one below / at 2147483000, and a threshold whose quotient is out of range
        "int_cut_below": [_stage([(268435360.0, 268435360.0), (14.75, -14.75), (0.125, 0.125)], 0.0)],
        "int_cut_at": [_stage([(268435360.0, 268435360.0), (14.875, -14.875), (0.125, 0.125)], 0.0)],
        "int_threshold_range": [_stage([(0.125, -0.125)], 3e8), _stage([(0.125, -0.125)], -3e8)],
    }


@pytest.mark.parametrize("name", list(edge_stages()))
def test_edge_stage_recs(stage_recs, name):
    from nubovca import synth
    stages = edge_stages()[name]
    (c,) = stage_recs([synth.cascade_to_xml(dict(name="edge", size=(20, 20), stages=stages))])
    check_cascade(c, random.Random(name))
    flags = [r["flags"] for r in c["stages"]]
    expect = {"bound_2^52-1": [2], "bound_2^52+1": [0], "bound_2^53+1": [0], "int_cut_below": [6], "int_cut_at": [2],
              "all_zero": [2, 2]}.get(name)
    if expect is not None:
        assert [f & 6 for f in flags] == expect, flags


def test_non_finite_votes_are_never_reordered(stage_recs):
    """the loader accepts inf / nan votes (strtod): such a stage carries neither proof"""
    from nubovca import synth
    stages = [_stage([(float("inf"), -1.0), (0.5, -0.5)], 0.0), _stage([(float("nan"), 0.25)], 0.0),
              _stage([(-float("inf"), float("inf"))], -1.0), _stage([(0.5, -0.5)], 0.0)]
    (c,) = stage_recs([synth.cascade_to_xml(dict(name="nonfinite", size=(20, 20), stages=stages))])
    assert "error" not in c, c
    assert [r["flags"] & 6 for r in c["stages"]] == [0, 0, 0, 6]
    assert [r["spec_run"] for r in c["stages"]] == [0, 0, 0, 1]


# ------------------------------------------------------------------ the oracle: soundness and teeth
def _permuted(casc, proven, rng):
    out = S._copy(casc)
    for si, st in enumerate(out["stages"]):
        if si in proven:
            perm = rng.permutation(len(st["features"]))
            for k in ("features", "thresholds", "left", "right"):
                st[k] = [st[k][j] for j in perm]
    return out


@pytest.mark.parametrize("name", ["small", "tie", "tie_f64", "order_s3"])
def test_permuting_proven_stages_leaves_oracle_unchanged(stage_recs, name):
    import orc
    from nubovca import synth
    xml = synth.synthetic_cascade_xml(seed=7, stages=[3, 8, 12, 16, 20, 24]) if name == "small" else S.variant(name)[0]
    (c,) = stage_recs([xml])
    proven = {i for i, r in enumerate(c["stages"]) if r["flags"] & 2}
    assert proven
    casc = S.xml_to_cascade(xml)
    a = orc.parse_cascade_xml(xml)
    rng = np.random.default_rng(11)
    for k, g in enumerate(S.images()):
        b = orc.parse_cascade_xml(synth.cascade_to_xml(_permuted(casc, proven, rng)))
        for pol in (orc.SUM_F32PAIR, orc.SUM_F64):
            ra = orc.detect_raw(a, g, 1.1, 0, (0, 0), policy=pol)
            assert len(ra) > 0 and np.array_equal(ra, orc.detect_raw(b, g, 1.1, 0, (0, 0), policy=pol)), (k, pol)


# candidates (symmetric difference of the raw lists, both IMAGES together) by which each designed cascade's twin differs at least
TEETH = {"order_s0": 15, "order_s3": 12, "order_s6": 100, "order_s7": 200, "tie": 150, "tie_f64": 30, "cut_lo": 20, "cut_hi": 20}


@pytest.mark.parametrize("name", S.NAMES)
def test_designed_cascades_have_teeth(name):
    """the twin (ballast re-ordered, thresholds one ulp up, a tie-breaking vote; for the cut pair: the other side of the cut)
    changes the oracle's raw lists on the images the GPU tests use: a kernel that summed in another order or broke ties the other
    way could not match the oracle by chance"""
    import orc
    xml, twin, _ = S.variant(name)
    if name.startswith("cut"):
        twin = S.variant("cut_hi" if name == "cut_lo" else "cut_lo")[0]
    a, b = orc.parse_cascade_xml(xml), orc.parse_cascade_xml(twin)
    diff, n = 0, 0
    for g in S.images():
        ra, rb = orc.detect_raw(a, g, 1.1, 0, (0, 0)), orc.detect_raw(b, g, 1.1, 0, (0, 0))
        diff += len(set(map(tuple, ra.tolist())) ^ set(map(tuple, rb.tolist())))
        n += len(ra)
    print("%s: %d raw candidates, twin differs by %d" % (name, n, diff))
    assert diff >= TEETH[name], (name, diff, TEETH[name])
