"""General new-format HAAR cascades -- tree weak classifiers, tilted features -- without a device: the numpy statement
(tests/haar_tree_reference.py) against answers derived by hand (tests/haar_tree_cases.py) and against its own scalar walk, the loader
through nvca_cascade_validate_mem_ex, and the premises the GPU tests rely on."""
import ctypes as C
import os

import numpy as np
import pytest

import haar_new_cases as HK
import haar_new_reference as HR
import haar_tree_cases as K
import haar_tree_reference as R
import lbp_cases as LK
import orc
from nubovca import capi, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newformat_trees_tilted_20x20.xml.txt")
GENERAL = capi.LOAD_HAAR_GENERAL
STATUS = {"PARSE": capi.ERR_PARSE, "UNSUPPORTED": capi.ERR_UNSUPPORTED}


def _ref(cdict, style="traincascade"):
    return R.parse_xml(synth.haar_tree_cascade_to_xml(cdict, style))


def validate(xml, flags=GENERAL):
    """nvca_cascade_validate_mem_ex: (status, (win_w, win_h, n_stages, n_weak), error text)"""
    L = capi.load()
    if isinstance(xml, str):
        xml = xml.encode()
    v = [C.c_int(-1) for _ in range(4)]
    err = C.create_string_buffer(512)
    rc = L.nvca_cascade_validate_mem_ex(xml, len(xml), flags, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), err, 512)
    return rc, tuple(x.value for x in v), err.value.decode("latin-1")


def validate_plain(xml):
    L = capi.load()
    if isinstance(xml, str):
        xml = xml.encode()
    v = [C.c_int(-1) for _ in range(4)]
    err = C.create_string_buffer(512)
    rc = L.nvca_cascade_validate_mem(xml, len(xml), C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), err, 512)
    return rc, tuple(x.value for x in v), err.value.decode("latin-1")


# ------------------------------------------------------------------ the tilted integral
def test_tilted_integral_is_the_oracles():
    rng = np.random.default_rng(19)
    for h, w in ((1, 1), (2, 5), (7, 3), (23, 31), (40, 17)):
        g = rng.integers(0, 256, (h, w)).astype(np.uint8)
        T = R.tilted_integral(g)
        assert T.dtype == np.int32 and T.shape == (h + 1, w + 1) and np.array_equal(T, orc.integral_tilted(g))
        assert np.array_equal(synth._tilted_integral_np(g), T)          # (the generator's recurrence)


def test_tilted_rects_on_a_4x4_image_against_the_pixel_sums():
    g = np.arange(1, 26, dtype=np.uint8).reshape(5, 5)          # p(x, y) = 1 + 5 y + x
    T = R.tilted_integral(g)
    z = np.zeros(1, np.int64)
    p = lambda x, y: int(g[y, x])
    assert int(R.tilted_rect_sum(T, (2, 0, 1, 1), z, z)[0, 0]) == p(1, 0) + p(1, 1)
    assert int(R.tilted_rect_sum(T, (2, 0, 2, 1), z, z)[0, 0]) == p(1, 0) + p(1, 1) + p(2, 1) + p(2, 2)
    assert int(R.tilted_rect_sum(T, (2, 1, 1, 2), z, z)[0, 0]) == p(1, 1) + p(1, 2) + p(0, 2) + p(0, 3)          # h = 2: the pair, and the pair one step down-left


# ------------------------------------------------------------------ the statement against hand-derived answers
HAND = K.tilted_cases() + K.tree_cases()


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made_windows(case):
    _, cdict, gray, exp = case
    assert R.scan(_ref(cdict), gray, 2.0).tolist() == exp


@pytest.mark.parametrize("case", K.skip_cases(), ids=[c[0] for c in K.skip_cases()])
def test_a_tree_in_stage_0_and_the_skip_rule(case):
    _, cdict, exp = case
    assert R.scan(_ref(cdict), LK.column_image(), 4.0).tolist() == exp


def test_every_leaf_of_the_three_node_tree_is_reached_by_a_case():
    asked = {c[0].split("-leaf")[1].split("-")[0] for c in K.tree_cases() if c[0].startswith("tree3") and c[3]}
    assert asked == {"1", "2", "4", "8"}


def test_scalar_walk_agrees_with_the_vectorised_one():
    for name in ("t20", "deep4"):
        ref = K.cascade(name)[1]
        ow, oh = ref.size
        g = K.image(61, 47, ow, oh)
        S, Q = orc.integral(g)
        T = R.tilted_integral(g)
        xs, ys = np.arange(0, 61 - ow, 2), np.arange(0, 47 - oh, 2)
        trace = {}
        res = R.grid_results(ref, S, Q, T, xs, ys, trace)
        for iy in range(0, len(ys), 3):
            for ix in range(0, len(xs), 3):
                r, sums = R.window_result_scalar(ref, S, Q, T, int(xs[ix]), int(ys[iy]))
                assert r == res[iy, ix] and sums[-1] == trace["gyp"][iy, ix], (name, ix, iy)


def test_stumps_answer_as_the_stump_statement():
    """a file of stumps "0 -1" on upright features, read by both statements"""
    xml = K.stump_xml()
    g = HK.image(97, 83, 24, 24)
    assert np.array_equal(R.scan(R.parse_xml(xml), g, 1.1), HR.scan(HR.parse_xml(xml), g, 1.1))


# ------------------------------------------------------------------ the loader, through nvca_cascade_validate_mem_ex
@pytest.mark.parametrize("name", list(K.CASCADES))
def test_both_styles_load_with_the_same_shape(name):
    kw = K.CASCADES[name]
    shape = (kw["ow"], kw["oh"], len(kw["stage_sizes"]), sum(kw["stage_sizes"]))
    for style in ("traincascade", "minimal"):
        xml = K.cascade(name, style)[0]
        assert validate(xml) == (capi.OK, shape, ""), style
        rc, _, err = validate_plain(xml)
        assert rc == capi.ERR_UNSUPPORTED and err
    assert "maxDepth" not in K.cascade(name, "minimal")[0] and "<maxDepth>1<" not in K.cascade(name, "traincascade")[0]


@pytest.mark.parametrize("case", K.refusal_cases(), ids=[c[0] for c in K.refusal_cases()])
def test_refusals_with_the_flag(case):
    _, xml, status = case
    rc, _, err = validate(xml)
    assert rc == STATUS[status] and err, (rc, err)


def test_fifteen_nodes_load():
    assert validate(K.fifteen_node_chain()) == (capi.OK, (4, 4, 1, 1), "")


@pytest.mark.parametrize("case", K.pinned_refusals(), ids=[c[0] for c in K.pinned_refusals()])
def test_pinned_refusals_hold_without_the_flag_and_load_with_it(case):
    _, xml = case
    for v in (validate_plain(xml), validate(xml, 0)):
        assert v[0] == capi.ERR_UNSUPPORTED and v[2]
    rc, shape, err = validate(xml)
    assert (rc, err) == (capi.OK, "") and shape[:3] == (4, 4, 1)


def test_unknown_flag_bits():
    xml = K.stump_xml().encode()
    for flags in (2, 3, 0x80000000, 0xfffffffe):
        assert validate(xml, flags)[0] == capi.ERR_ARG
    assert validate(xml, 0) == validate_plain(xml) == validate(xml)


def test_the_flag_changes_nothing_on_old_format_and_lbp_files(small_xml):
    lbp = LK.cascade("w12")[0]
    for xml in (small_xml, lbp, synth.generic_cascade_xml()):
        assert validate(xml) == validate_plain(xml) and validate(xml)[0] == capi.OK
    trees = lbp.replace("<maxDepth>1", "<maxDepth>2")
    assert "<maxDepth>2" in trees
    assert validate(trees)[0] == validate_plain(trees)[0] == capi.ERR_UNSUPPORTED          # LBP trees stay refused


def test_a_converted_generic_cascade_loads():
    old = synth.generic_cascade_xml()
    rc, shape, _ = validate_plain(old)
    assert rc == capi.OK
    for style in ("traincascade", "minimal"):
        xml = synth.haar_old_xml_to_tree_xml(old, style)
        assert validate(xml) == (capi.OK, shape, "")
        ref = R.parse_xml(xml)
        assert ref.tilted.any() and (ref.node_counts > 1).any() and len(ref.nodes) == len(ref.rects)


def test_golden_file_shape():
    text = open(GOLDEN).read()
    assert os.path.getsize(GOLDEN) < 8192
    assert validate(text) == (capi.OK, (20, 20, 2, 5), "")
    assert validate_plain(text)[0] == capi.ERR_UNSUPPORTED
    ref = R.parse_xml(text)
    assert ref.stage_sizes.tolist() == [2, 3] and ref.node_counts.tolist() == [1, 2, 3, 1, 2] and int(ref.tilted.sum()) == 1
    g = K.image(97, 83, 20, 20)
    st = {}
    assert len(R.scan(ref, g, 1.1, stats=st)) > 0 and (st["node_hits"] > 0).all() and (st["leaf_hits"] > 0).all()


def test_random_byte_damage_returns():
    xml = bytearray(K.cascade("deep4")[0].encode())
    rng = np.random.default_rng(2026)
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
def _premises(name, cols, rows, sf):
    ref = K.cascade(name)[1]
    st = {}
    raw = R.scan(ref, K.image(cols, rows, *ref.size), sf, stats=st)
    nt = int(ref.stage_sizes[:R.TILE_STAGES].sum())          # trees, nodes and leaves of the tile stages
    nn = int(ref.node_counts[:nt].sum())
    assert (st["node_hits"][:nn] > 0).all() and (st["leaf_hits"][:nn + nt] > 0).all()
    assert len(st["wave_split"]) > 0                          # in one wave, windows leave a tree by different leaves
    d = np.array(st["depth"])
    assert all(np.count_nonzero(d == -s) > 0 for s in range(len(ref.stage_sizes)))          # every stage rejects a visited window
    assert len(raw) >= 20
    assert ref.tilted[ref.nodes[:nn, 2]].any() and ref.tilted[ref.nodes[nn:, 2]].any()       # tilted features in a tile stage and behind
    assert (ref.node_counts[:nt] > 1).any() and (ref.node_counts[nt:] > 1).any()
    return raw


@pytest.mark.parametrize("name", list(K.CASCADES))
def test_premises_of_the_raw_list_cases(name):
    _premises(name, *K.IMAGES[name])


def test_premises_of_the_other_gpu_cases():
    name, cols, rows, sf = K.WIDE
    ref = K.cascade(name)[1]
    assert len(R.scan(ref, K.image(cols, rows, *ref.size), sf)) >= 20
    name, cols, rows, sf = K.BATCH
    ref = K.cascade(name)[1]
    lists = [R.scan(ref, K.image(cols, rows, *ref.size, 100 + i), sf) for i in range(4)]
    assert all(len(l) > 0 for l in lists) and len({l.tobytes() for l in lists}) == 4          # slots tell each other apart
    name, cols, rows, sf = K.LEVELS
    ref = K.cascade(name)[1]
    rects, lv, wt = R.scan_levels(ref, K.image(cols, rows, *ref.size), sf)
    n = len(ref.stage_sizes)
    assert n >= 4 and set(lv.tolist()) == {n - 3, n - 2, n - 1, n} and len(set(wt.tolist())) > 100          # (many distinct sums to compare)
    assert max(int(c) for c in K.cascade("deep4")[1].node_counts) >= 5
