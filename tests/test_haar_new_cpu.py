"""New-format HAAR cascades without a device: the numpy statement of SURVEY.md A.16 (tests/haar_new_reference.py) against answers
derived by hand (tests/haar_new_cases.py), the loader through nvca_cascade_validate_mem, and the premises the GPU tests rely on
(their comparisons are not [] == [], and the branches they are meant to reach are reached)."""
import ctypes as C
import os

import numpy as np
import pytest

import haar_new_cases as K
import haar_new_reference as R
import lbp_cases as LK
from nubovca import capi, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newformat_haar_20x20.xml.txt")


def _ref(cdict, style="traincascade"):
    return R.parse_xml(synth.haar_new_cascade_to_xml(cdict, style))


def _scan(cdict, gray, sf, mins=(0, 0), maxs=(0, 0)):
    return R.scan(_ref(cdict), gray, sf, mins, maxs).tolist()


def validate(xml):
    """nvca_cascade_validate_mem: (status, (win_w, win_h, n_stages, n_weak), error text)"""
    L = capi.load()
    if isinstance(xml, str):
        xml = xml.encode()
    v = [C.c_int(-1) for _ in range(4)]
    err = C.create_string_buffer(512)
    rc = L.nvca_cascade_validate_mem(xml, len(xml), C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), err, 512)
    return rc, tuple(x.value for x in v), err.value.decode("latin-1")


# ------------------------------------------------------------------ the statement against hand-derived answers
@pytest.mark.parametrize("case", K.value_cases(), ids=[c[0] for c in K.value_cases()])
def test_hand_made_windows(case):
    _, cdict, gray, exp = case
    assert _scan(cdict, gray, 2.0) == exp


def test_premises_of_the_hand_made_windows():
    f32 = np.float32
    assert f32(f32(K.B) + f32(1)) == f32(K.B) and f32(f32(f32(K.B) + f32(1)) - f32(K.B - 1)) == 1          # 2^24 + 1 is lost in f32
    assert f32(f32(-K.B) + f32(-1)) == f32(-K.B)
    assert f32(f32(f32(1e8) + f32(1)) - f32(1e8)) == 0 and (np.float64(f32(1e8)) + 1.0) - np.float64(f32(1e8)) == 1.0
    thr = f32(f32(0.5) - f32(1e-5))
    assert f32(0.49998) < thr <= f32(0.499995) < f32(0.5)
    # the windows' normalisers, by the statement's own function
    for (ow, gray, vnf) in ((3, K.value_cases()[0][2], 1.0), (4, K.value_cases()[4][2], 0.25), (4, np.full((5, 5), 90, np.uint8), 1.0)):
        S = np.zeros((ow + 2, ow + 2), np.int32); Q = np.zeros((ow + 2, ow + 2), np.float64)
        S[1:, 1:] = np.cumsum(np.cumsum(gray.astype(np.int64), 0), 1); Q[1:, 1:] = np.cumsum(np.cumsum(gray.astype(np.float64) ** 2, 0), 1)
        z = np.zeros(1, np.int64)
        assert R.window_vnf(S, Q, ow, ow, z, z)[0, 0] == vnf


def test_stage_threshold_loses_1e5_in_float():
    c = _ref(K.permissive(3, 3))
    assert c.stage_thr[0] == np.float32(np.float32(-1.0) - np.float32(1e-5))
    c = _ref(K.one_stump((3, 3), K.PIX00, 1.0))
    assert c.stage_thr[0] == np.float32(np.float32(0.5) - np.float32(1e-5)) and c.stage_thr[0] < np.float32(0.5)


@pytest.mark.parametrize("case", K.skip_cases(), ids=[c[0] for c in K.skip_cases()])
def test_skip_columns(case):
    _, cdict, exp = case
    assert _scan(cdict, LK.column_image(), 4.0) == exp


@pytest.mark.parametrize("case", K.scan_rule_cases(), ids=[c[0] for c in K.scan_rule_cases()])
def test_scan_rules(case):
    _, cdict, shape, sf, mins, maxs, exp = case
    assert _scan(cdict, np.full(shape, 120, np.uint8), sf, mins, maxs) == exp


# ------------------------------------------------------------------ the loader, through nvca_cascade_validate_mem
@pytest.mark.parametrize("name", list(K.CASCADES))
def test_both_styles_load_with_the_same_shape(name):
    kw = K.CASCADES[name]
    shape = (kw["ow"], kw["oh"], len(kw["stage_sizes"]), sum(kw["stage_sizes"]))
    for style in ("traincascade", "minimal"):
        rc, got, err = validate(K.cascade(name, style)[0])
        assert (rc, got, err) == (capi.OK, shape, ""), style
    assert "boostType" in K.cascade(name, "traincascade")[0] and "boostType" not in K.cascade(name, "minimal")[0]
    assert "maxDepth" not in K.cascade(name, "minimal")[0]          # an absent maxDepth means stumps


def test_golden_file_shape():
    rc, got, err = validate(open(GOLDEN, "rb").read())
    assert (rc, got, err) == (capi.OK, (20, 20, 3, 9), "")
    ref = R.parse_xml(open(GOLDEN).read())
    assert ref.stage_sizes.tolist() == [2, 3, 4] and len(ref.rects) == 9 and sorted(set(ref.rect_counts.tolist())) == [1, 2, 3]
    assert os.path.getsize(GOLDEN) < 8192


def test_a_converted_old_format_cascade_loads(small_xml):
    assert validate(small_xml)[:2] == (capi.OK, (20, 20, 6, 83))
    for style in ("traincascade", "minimal"):
        xml = synth.haar_old_xml_to_new_xml(small_xml, style)
        assert validate(xml) == (capi.OK, (20, 20, 6, 83), "")
        ref = R.parse_xml(xml)
        assert ref.stage_sizes.sum() == 83 and len(ref.rects) == 83 and set(ref.rect_counts.tolist()) <= {2, 3}


def _base():
    return synth.haar_new_cascade_to_xml(K.hand_cascade(
        (24, 24), [[(0, 0, 8, 8, -1.0), (4, 0, 4, 8, 2.0)], [(3, 3, 6, 6, -1.0), (3, 3, 3, 3, 2.0), (6, 6, 3, 3, 2.0)]],
        [(0.5, [(0, 0.25, (1.0, -1.0)), (1, -0.125, (0.5, -0.5))]), (0.25, [(1, 0.75, (1.0, -1.0))])]))


def refusal_table():
    """(id, damaged file, status): every refusal the loader states for a new-format HAAR file"""
    b = _base()
    U, P = capi.ERR_UNSUPPORTED, capi.ERR_PARSE
    r0 = "0 0 8 8 -1.</_>"

    def sub(old, new, count=1):
        assert old in b, old
        return b.replace(old, new, count)
    return [
        ("tilted", sub("<tilted>0", "<tilted>1"), U),
        ("maxDepth-2", sub("<maxDepth>1", "<maxDepth>2"), U),
        ("two-internal-nodes", sub("0 -1 0 0.25</internalNodes>", "0 -1 0 0.25 0 -1 1 0.5</internalNodes>").replace("1 -1</leafValues>", "1 -1 0.5</leafValues>", 1), U),
        ("maxCatCount-256", sub("<maxCatCount>0", "<maxCatCount>256"), U),
        # ... decided before any feature or node is read: the same file with its features and nodes damaged as well is still UNSUPPORTED
        ("maxCatCount-before-features", sub("<maxCatCount>0", "<maxCatCount>256").replace(r0, "0 0 99 8 -1.</_>").replace("0 -1 0 0.25<", "0 -1 7 x<"), U),
        ("featureType-HOG", sub("<featureType>HAAR", "<featureType>HOG"), U),
        ("stageType", sub("<stageType>BOOST", "<stageType>CART"), U),
        ("featureType-unknown", sub("<featureType>HAAR", "<featureType>SURF"), P),
        ("no-features", sub("<features>", "<feats>").replace("</features>", "</feats>"), P),
        ("no-stageNum", sub("<stageNum>2</stageNum>", ""), P),
        ("no-width", sub("<width>24</width>", ""), P),
        ("no-maxCatCount", sub("<maxCatCount>0</maxCatCount>", ""), P),
        ("no-leafValues", sub("<leafValues>", "<leaves>").replace("</leafValues>", "</leaves>", 1), P),
        ("no-stageThreshold", sub("<stageThreshold>0.5</stageThreshold>", ""), P),
        ("no-rects", sub("<rects>", "<rs>").replace("</rects>", "</rs>", 1), P),
        ("nodes-not-0", sub("0 -1 0 0.25<", "1 -1 0 0.25<"), P),
        ("nodes-not-minus-1", sub("0 -1 0 0.25<", "0 -2 0 0.25<"), P),
        ("nodes-three-words", sub("0 -1 0 0.25<", "0 -1 0<"), P),
        ("nodes-five-words", sub("0 -1 0 0.25<", "0 -1 0 0.25 1<"), P),
        ("three-leaves", sub("1 -1</leafValues>", "1 -1 2</leafValues>"), P),
        ("featureIdx-high", sub("0 -1 0 0.25<", "0 -1 2 0.25<"), P),
        ("featureIdx-negative", sub("0 -1 0 0.25<", "0 -1 -1 0.25<"), P),
        ("featureIdx-fraction", sub("0 -1 0 0.25<", "0 -1 0.5 0.25<"), P),
        ("rect-x-negative", sub(r0, "-1 0 8 8 -1.</_>"), P),
        ("rect-y-negative", sub(r0, "0 -1 8 8 -1.</_>"), P),
        ("rect-w-zero", sub(r0, "0 0 0 8 -1.</_>"), P),
        ("rect-h-negative", sub(r0, "0 0 8 -8 -1.</_>"), P),
        ("rect-x-w-outside", sub(r0, "17 0 8 8 -1.</_>"), P),
        ("rect-y-h-outside", sub(r0, "0 17 8 8 -1.</_>"), P),
        ("rect-four-numbers", sub(r0, "0 0 8 8</_>"), P),
        ("rect-six-numbers", sub(r0, "0 0 8 8 -1. 2</_>"), P),
        ("rect-coordinate-fraction", sub(r0, "0 0 8.5 8 -1.</_>"), P),
        ("zero-rects", b[:b.index("<rects>") + 7] + b[b.index("</rects>"):], P),
        ("four-rects", sub("6 6 3 3 2.</_>", "6 6 3 3 2.</_>\n        <_>\n          0 0 1 1 1.</_>"), P),
        ("window-2", sub("<width>24", "<width>2"), P),
        ("window-1025", sub("<height>24", "<height>1025"), P),
        ("stage-maxWeakCount-disagrees", sub("<maxWeakCount>2</maxWeakCount>\n      <stageThreshold>", "<maxWeakCount>3</maxWeakCount>\n      <stageThreshold>"), P),
        ("stageNum-disagrees", sub("<stageNum>2", "<stageNum>3"), P),
        ("empty-stage", b[:b.index("        <_>\n          <internalNodes>")] + b[b.index("</weakClassifiers>"):], P),
        ("no-stages", sub("<stageNum>2", "<stageNum>0").replace(b[b.index("<stages>") + 8:b.index("</stages>")], ""), P),
        ("threshold-not-a-number", sub("0 -1 0 0.25<", "0 -1 0 x<"), P),
        ("threshold-nan", sub("0 -1 0 0.25<", "0 -1 0 nan<"), P),
        ("weight-not-a-number", sub(r0, "0 0 8 8 w</_>"), P),
        ("stageThreshold-not-a-number", sub("<stageThreshold>0.5<", "<stageThreshold>half<"), P),
        ("leaf-not-a-number", sub("1 -1</leafValues>", "1 one</leafValues>"), P),
        ("tilted-not-a-number", sub("<tilted>0", "<tilted>no"), P),
    ]


def test_base_of_the_refusal_table_loads():
    assert validate(_base()) == (capi.OK, (24, 24, 2, 3), "")


@pytest.mark.parametrize("case", refusal_table(), ids=[c[0] for c in refusal_table()])
def test_refusals(case):
    _, xml, status = case
    rc, _, err = validate(xml)
    assert rc == status and err, (rc, err)


def test_random_byte_damage_returns():
    xml = bytearray(K.cascade("w12")[0].encode())
    rng = np.random.default_rng(2025)
    seen = set()
    for _ in range(300):
        b = bytearray(xml)
        for _k in range(int(rng.integers(1, 6))):
            mode = int(rng.integers(0, 3))
            i = int(rng.integers(0, len(b)))
            if mode == 0:
                b[i] = int(rng.integers(0, 256))
            elif mode == 1:
                del b[i:i + int(rng.integers(1, 40))]
            else:
                b[i:i] = bytes(rng.integers(32, 127, int(rng.integers(1, 12))).astype(np.uint8))
        if not b:
            continue
        rc, _, err = validate(bytes(b))
        assert rc in (capi.OK, capi.ERR_PARSE, capi.ERR_UNSUPPORTED) and (rc == capi.OK) == (err == "")
        seen.add(rc)
    assert capi.ERR_PARSE in seen


# ------------------------------------------------------------------ premises of the GPU cases, on the statement alone
def _premises(ref, gray, sf, late):
    """non-empty raw list; visited windows behind the tile stages (stage 3) and behind the stage groups that end at `late`; stage-0 rejects
    among the visited windows (both states of the walk); windows on the nf <= 0 branch"""
    st = {}
    raw = R.scan(ref, gray, sf, stats=st)
    d = np.array(st["depth"])
    reached = lambda s: int(np.count_nonzero((d == 1) | (d <= -s)))          # visited windows that reach stage s
    assert len(raw) > 0
    assert reached(3) > 0 and all(reached(s) > 0 for s in late)
    assert np.count_nonzero(d == 0) > 0 and np.count_nonzero(d != 0) > 0
    assert st["nf_nonpositive"] >= 1
    return st, raw


@pytest.mark.parametrize("name", ["w24", "w20x28", "w12"])
@pytest.mark.parametrize("img", K.IMAGES, ids=["%dx%d" % i[:2] for i in K.IMAGES])
def test_premises_of_the_raw_list_cases(name, img):
    ref = K.cascade(name)[1]
    cols, rows, sf = img
    st, raw = _premises(ref, K.image(cols, rows, *ref.size), sf, late=(5, 8, len(ref.stage_sizes)))        # behind groups [3, 5), [5, 8) and the last
    assert np.array_equal(raw, K.expected_raw(name, cols, rows, sf))


def test_premises_of_the_wide_case():
    cols, rows, sf = K.WIDE
    ref = K.cascade("w24")[1]
    wide = R.levels(24, 24, cols, rows, sf)
    assert wide[0][1][0] > 1023 and wide[1][1][0] > 1023 and wide[-1][1][0] <= 1023
    _premises(ref, K.image(cols, rows, 24, 24), sf, late=(5, 8, 10))


def test_premises_of_the_stage_heavy_cascade():
    """20 stages: the tile kernel takes stages 0 .. 2, then groups [3, 5), [5, 8), [8, 12), [12, 17), [17, 20): the last one must still see windows"""
    ref = K.cascade("deep")[1]
    assert len(ref.stage_sizes) == 20
    cols, rows, sf = K.DEEP_IMAGE
    st, raw = _premises(ref, K.image(cols, rows, 24, 24), sf, late=(5, 8, 12, 17, 20))
    assert np.count_nonzero(np.array(st["depth"]) <= -12) > 0                 # late stages reject as well as pass


@pytest.mark.parametrize("name", ["w81", "w82"])
def test_premises_of_the_lds_bound_cases(name):
    ow = K.CASCADES[name]["ow"]
    words = (31 * 2 + ow + 1) * (15 * 2 + ow + 1)          # the bound as the tables state it: the stage-0 tile at step 2 against 64 KiB
    assert (words * 4 <= 64 * 1024) == (name == "w81")
    cols, rows, sf = K.LDS_IMAGE
    ref = K.cascade(name)[1]
    _premises(ref, K.image(cols, rows, ow, ow), sf, late=(len(ref.stage_sizes),))


@pytest.mark.parametrize("route", sorted(K.HI_PLANES))
def test_premises_of_the_high_byte_plane_cases(route):
    """levels behind the first hold many windows whose four normrect corners of Q differ in their bits above 2^32"""
    import orc
    cols, rows, sf = K.HI_PLANES[route]
    ref, g = K.cascade("w81")[1], K.hi_planes_image(cols, rows)
    lv = R.levels(81, 81, cols, rows, sf)
    assert (lv[0][1][0] > 1023) == (route == "per-level") and len(lv) >= 2
    mixed = 0
    for factor, sz, _win in lv[1:]:
        Q = orc.integral(orc.resize_linear(g, sz[0], sz[1]))[1]
        hi = np.floor(Q / 2.0 ** 32).astype(np.int64)
        xs, ys = np.arange(0, sz[0] - 81, 2 if factor <= 2 else 1), np.arange(0, sz[1] - 81, 2 if factor <= 2 else 1)
        c = [hi[np.ix_(ys + dy, xs + dx)] for dy in (1, 80) for dx in (1, 80)]
        mixed += int(np.count_nonzero((c[0] != c[1]) | (c[0] != c[2]) | (c[0] != c[3])))
    assert mixed > 100
    st = {}
    raw = R.scan(ref, g, sf, stats=st)
    d = np.array(st["depth"])
    assert len(raw) > 0 and np.count_nonzero(d == 0) > 0 and np.count_nonzero(d < 0) > 0


def test_premises_of_the_bright_case():
    ref = K.bright_cascade()[1]
    g = K.bright_image()
    assert len(R.levels(264, 264, g.shape[1], g.shape[0], 1.5)) == 1
    st = {}
    raw = R.scan(ref, g, 1.5, stats=st)
    d = np.array(st["depth"])
    assert 0 < len(raw) < len(d) and st["sum_above_2p24"] > 0 and np.count_nonzero(d == 0) > 0


def test_premise_of_the_overflow_case():
    cols, rows, sf = K.IMAGES[1]
    assert len(R.scan(_ref(K.permissive(24, 24)), K.image(cols, rows, 24, 24), sf)) > 3000 > 256
