"""New-format LBP cascades without a device: the numpy statement of SURVEY.md A.15 (tests/lbp_reference.py) against answers derived
by hand (tests/lbp_cases.py), the loader through nvca_cascade_validate_mem, and the premises tests/test_gpu_lbp.py relies on
(its comparisons are not [] == [])."""
import ctypes as C
import os

import numpy as np
import pytest

import lbp_cases as K
import lbp_reference as R
from nubovca import capi, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newformat_lbp_24x24.xml.txt")


def _ref(cdict, style="traincascade"):
    return R.parse_xml(synth.lbp_cascade_to_xml(cdict, style))


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
@pytest.mark.parametrize("case", K.code_cases(), ids=[c[0] for c in K.code_cases()])
def test_code_of_a_hand_made_window(case):
    _, gray, code = case
    S = np.zeros((5, 5), np.int32)
    S[1:, 1:] = np.cumsum(np.cumsum(gray.astype(np.int64), 0), 1)
    assert int(R.codes(S, (0, 0, 1, 1), np.zeros(1, np.int64), np.zeros(1, np.int64))[0, 0]) == code
    assert _scan(K.code_cascade([code]), gray, 2.0) == K.ONE_WINDOW
    assert _scan(K.code_cascade([c for c in range(256) if c != code]), gray, 2.0) == []


def test_subset_word_written_negative():
    assert K.only_codes([31]) == [-2147483648, 0, 0, 0, 0, 0, 0, 0] and K.only_codes([255])[7] == -2147483648
    xml = synth.lbp_cascade_to_xml(K.code_cascade([31]))
    assert "-2147483648" in xml
    assert R.parse_xml(xml).subsets[0, 0] == -2147483648


def test_stage_sum_depends_on_the_order_of_its_votes():
    gray = np.full((4, 4), 90, np.uint8)
    assert np.float32(np.float32(np.float32(1e8) + np.float32(1)) - np.float32(1e8)) == 0       # the premise, in f32
    assert _scan(K.vote_order_cascade("big-one-minus"), gray, 2.0) == []
    assert _scan(K.vote_order_cascade("big-minus-one"), gray, 2.0) == K.ONE_WINDOW


def test_stage_threshold_loses_1e5_in_float():
    c = _ref(K.hand_cascade((3, 3), [(0, 0, 1, 1)], [(0.5, [(0, [0] * 8, (1.0, 1.0))])]))
    assert c.stage_thr[0] == np.float32(np.float32(0.5) - np.float32(1e-5)) and c.stage_thr[0] < np.float32(0.5)


@pytest.mark.parametrize("case", K.skip_cases(), ids=[c[0] for c in K.skip_cases()])
def test_skip_columns(case):
    _, cdict, exp = case
    assert _scan(cdict, K.column_image(), 4.0) == exp


@pytest.mark.parametrize("case", K.scan_rule_cases(), ids=[c[0] for c in K.scan_rule_cases()])
def test_scan_rules(case):
    _, cdict, shape, sf, mins, maxs, exp = case
    assert _scan(cdict, np.full(shape, 120, np.uint8), sf, mins, maxs) == exp


def test_reject_on_the_last_visited_column_ends_the_row():
    # 7 grid columns (0 .. 6); stage 0 rejects the even ones: the walk visits 0, 2, 4, 6 and its last step (from 6) leaves the row
    res = np.array([0, 1, 0, 1, 0, 1, 0])
    assert R.walk_row(res) == [0, 2, 4, 6]
    assert R.walk_row(np.array([1, 0, 1, 1, 0])) == [0, 1, 3, 4]


# ------------------------------------------------------------------ the loader, through nvca_cascade_validate_mem
@pytest.mark.parametrize("name", list(K.CASCADES))
def test_both_styles_load_with_the_same_shape(name):
    kw = K.CASCADES[name]
    shape = (kw["ow"], kw["oh"], len(kw["stage_sizes"]), sum(kw["stage_sizes"]))
    for style in ("traincascade", "minimal"):
        rc, got, err = validate(K.cascade(name, style)[0])
        assert (rc, got, err) == (capi.OK, shape, ""), style
    assert "boostType" in K.cascade(name, "traincascade")[0] and "boostType" not in K.cascade(name, "minimal")[0]


def test_golden_file_shape():
    rc, got, err = validate(open(GOLDEN, "rb").read())
    assert (rc, got, err) == (capi.OK, (24, 24, 3, 9), "")
    ref = R.parse_xml(open(GOLDEN).read())
    assert ref.stage_sizes.tolist() == [2, 3, 4] and len(ref.rects) == 6 and ref.feature_idx.tolist() == [0, 3, 1, 5, 2, 4, 0, 3, 5]
    assert ref.subsets[0].tolist() == [-1, 0, 2147483647, -2147483648, 16, -256, 65535, 1]
    assert os.path.getsize(GOLDEN) < 8192


def _base():
    return synth.lbp_cascade_to_xml(K.hand_cascade((24, 24), [(0, 0, 8, 8), (3, 3, 2, 2)],
                                                   [(0.5, [(0, [1, 2, 3, 4, 5, 6, 7, 8], (1.0, -1.0)), (1, [0] * 8, (0.5, -0.5))]), (0.25, [(1, [-1] * 8, (1.0, -1.0))])]))


def refusal_table():
    """(id, damaged file, status): every refusal the loader states"""
    b = _base()
    tree = "0 -1 0 1 2 3 4 5 6 7 8 0 -1 1 1 2 3 4 5 6 7 8"
    U, P = capi.ERR_UNSUPPORTED, capi.ERR_PARSE

    def sub(old, new, count=1):
        assert old in b
        return b.replace(old, new, count)
    return [
        ("featureType-HAAR", sub("<featureType>LBP", "<featureType>HAAR"), U),
        ("featureType-HOG", sub("<featureType>LBP", "<featureType>HOG"), U),
        ("stageType", sub("<stageType>BOOST", "<stageType>CART"), U),
        ("maxDepth-2", sub("<maxDepth>1", "<maxDepth>2"), U),
        ("two-internal-nodes", sub("0 -1 0 1 2 3 4 5 6 7 8</internalNodes>", tree + "</internalNodes>").replace("1 -1</leafValues>", "1 -1 0.5</leafValues>", 1), U),
        ("maxCatCount", sub("<maxCatCount>256", "<maxCatCount>0"), U),
        ("no-features", sub("<features>", "<feats>").replace("</features>", "</feats>"), P),
        ("no-stageNum", sub("<stageNum>2</stageNum>", ""), P),
        ("no-width", sub("<width>24</width>", ""), P),
        ("no-leafValues", sub("<leafValues>", "<leaves>").replace("</leafValues>", "</leaves>", 1), P),
        ("no-stageThreshold", sub("<stageThreshold>0.5</stageThreshold>", ""), P),
        ("nodes-not-0", sub("0 -1 0 1 2", "1 -1 0 1 2"), P),
        ("nodes-not-minus-1", sub("0 -1 0 1 2", "0 -2 0 1 2"), P),
        ("nodes-seven-words", sub("0 -1 0 1 2 3 4 5 6 7 8<", "0 -1 0 1 2 3 4 5 6 7<"), P),
        ("nodes-nine-words", sub("0 -1 0 1 2 3 4 5 6 7 8<", "0 -1 0 1 2 3 4 5 6 7 8 9<"), P),
        ("three-leaves", sub("1 -1</leafValues>", "1 -1 2</leafValues>"), P),
        ("featureIdx-high", sub("0 -1 0 1 2", "0 -1 2 1 2"), P),
        ("featureIdx-negative", sub("0 -1 0 1 2", "0 -1 -1 1 2"), P),
        ("rect-x-negative", sub("0 0 8 8</rect>", "-1 0 8 8</rect>"), P),
        ("rect-y-negative", sub("0 0 8 8</rect>", "0 -1 8 8</rect>"), P),
        ("rect-w-zero", sub("0 0 8 8</rect>", "0 0 0 8</rect>"), P),
        ("rect-h-zero", sub("0 0 8 8</rect>", "0 0 8 0</rect>"), P),
        ("rect-x-3w-outside", sub("0 0 8 8</rect>", "1 0 8 8</rect>"), P),
        ("rect-y-3h-outside", sub("0 0 8 8</rect>", "0 1 8 8</rect>"), P),
        ("rect-three-numbers", sub("0 0 8 8</rect>", "0 0 8</rect>"), P),
        ("window-2", sub("<width>24", "<width>2"), P),
        ("window-1025", sub("<height>24", "<height>1025"), P),
        ("stage-maxWeakCount-disagrees", sub("<maxWeakCount>2</maxWeakCount>\n      <stageThreshold>", "<maxWeakCount>3</maxWeakCount>\n      <stageThreshold>"), P),
        ("stageNum-disagrees", sub("<stageNum>2", "<stageNum>3"), P),
        ("empty-stage", b[:b.index("        <_>")] + b[b.index("</weakClassifiers>"):], P),
        ("no-stages", sub("<stageNum>2", "<stageNum>0").replace(b[b.index("<stages>") + 8:b.index("</stages>")], ""), P),
        ("number-not-a-number", sub("0 -1 0 1 2", "0 -1 0 1 x"), P),
        ("word-leaves-int32", sub("0 -1 0 1 2", "0 -1 0 1 2147483648"), P),
        ("word-leaves-int32-negative", sub("0 -1 0 1 2", "0 -1 0 1 -2147483649"), P),
        ("threshold-not-a-number", sub("<stageThreshold>0.5<", "<stageThreshold>half<"), P),
        ("leaf-not-a-number", sub("1 -1</leafValues>", "1 one</leafValues>"), P),
    ]


def test_base_of_the_refusal_table_loads():
    assert validate(_base()) == (capi.OK, (24, 24, 2, 3), "")


@pytest.mark.parametrize("case", refusal_table(), ids=[c[0] for c in refusal_table()])
def test_refusals(case):
    _, xml, status = case
    rc, _, err = validate(xml)
    assert rc == status and err, (rc, err)


def test_old_format_cascades_validate_with_unchanged_shapes(synth_xml, small_xml):
    assert validate(synth_xml)[:2] == (capi.OK, (20, 20, 22, 2135))
    assert validate(small_xml)[:2] == (capi.OK, (20, 20, 6, 83))
    rc, shape, _ = validate(synth.generic_cascade_xml(seed=3))
    assert rc == capi.OK and shape[:3] == (20, 20, 7)
    # a new-format file is no longer the old branch's parse error; a file that is neither still is
    rc, _, err = validate(b"<opencv_storage><x>1</x></opencv_storage>")
    assert rc == capi.ERR_PARSE and "opencv-haar-classifier" in err


def test_random_byte_damage_returns():
    xml = bytearray(K.cascade("w12")[0].encode())
    rng = np.random.default_rng(2024)
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


# ------------------------------------------------------------------ premises of tests/test_gpu_lbp.py, on the statement alone
@pytest.fixture(scope="module")
def premise_stats():
    out = {}
    for name, images in (("w24", K.IMAGES[:3]), ("w20x28", K.SMALL_IMAGES), ("w12", K.SMALL_IMAGES)):
        ref = K.cascade(name)[1]
        st, raws = {}, []
        for (cols, rows, sf) in images:
            raws.append(R.scan(ref, K.image(cols, rows, *ref.size), sf, stats=st))
        out[name] = (st, raws)
    return out


@pytest.mark.parametrize("name", ["w24", "w20x28", "w12"])
def test_premises_of_the_raw_list_cases(premise_stats, name):
    st, raws = premise_stats[name]
    assert sum(len(r) for r in raws) > 100 and all(len(r) > 0 for r in raws)
    assert any(len(R.detect(K.cascade(name)[1], K.image(c, r, *K.cascade(name)[1].size), sf, 3)) >= 1 for (c, r, sf) in K.SMALL_IMAGES[:2])
    assert st["skipped_pass"] >= 1                               # a skip removes a window that would otherwise have passed
    depths = set(st["depth"])
    assert len([d for d in depths if d <= 0]) >= 3 and 0 in depths and 1 in depths        # at least three distinct reject depths


def test_premises_of_the_level_cuts():
    cols, rows, sf = K.IMAGES[2]
    full = R.levels(24, 24, cols, rows, sf)
    assert len(R.levels(24, 24, cols, rows, sf, (30, 30))) < len(full) and len(R.levels(24, 24, cols, rows, sf, (0, 0), (60, 60))) < len(full)
    assert R.levels(24, 24, cols, rows, sf, (30, 30), (60, 60))
    wide = R.levels(24, 24, 1500, 240, 1.3)
    assert wide[0][1][0] > 1023 and wide[1][1][0] > 1023 and wide[-1][1][0] <= 1023     # levels on both sides of the one-launch pyramid's width limit


def test_premises_of_the_stage_heavy_cascade():
    """20 stages / 139 weak classifiers on 333 x 251: the tile kernel takes stages 0 .. 2, then survivor lists are compacted after stages 4, 7, 11, 16
    (groups of 2, 3, 4, 5 stages, then the rest), so late groups must still see windows"""
    ref = K.cascade("deep")[1]
    assert len(ref.stage_sizes) == 20 and 130 <= int(ref.stage_sizes.sum()) <= 150
    cols, rows, sf = K.IMAGES[2]
    st = {}
    raw = R.scan(ref, K.image(cols, rows, 24, 24), sf, stats=st)
    d = np.array(st["depth"])
    reached = lambda s: int(np.count_nonzero((d == 1) | (d <= -s)))          # visited windows that reach stage s
    assert reached(3) > 1000 and reached(5) > 100 and reached(8) > 20 and reached(12) > 0 and reached(17) > 0
    assert len(raw) > 0 and np.count_nonzero(d <= -10) > 0                   # late stages reject as well as pass


def test_premise_of_the_overflow_case():
    cols, rows, sf = K.IMAGES[1]
    assert len(R.scan(_ref(K.permissive(24, 24)), K.image(cols, rows, 24, 24), sf)) > 3000 > 256
