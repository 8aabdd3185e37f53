"""tests/frame_layouts.py on the CPU: the builder of "an image in a buffer" round-trips, its guard check can fail, and the case lists of
tests/test_gpu_frame_layouts.py lie on both sides of every dispatch predicate they are meant to cross -- asserted from the Python
statements of the predicates, so that a later edit of the lists cannot quietly drop a side.  trk_wide is pinned against trk_wide_ok
(csrc/trk_host.cpp) through the driver tests/test_trk_host_cpu.py builds; aligned4 restates frames_aligned4 (csrc/host_copy.cpp:379-386),
which lives in a file that needs the HIP runtime and has no CPU driver."""
import json
import os
import subprocess

import numpy as np
import pytest

import frame_layouts as FL

HOST, DEV = FL.HOST, FL.DEVICE


def _image(h, w, cn, seed=1):
    return np.random.default_rng([seed, h, w, cn]).integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)


SHAPES = [(h, w) for w in FL.WIDTHS for h in FL.HEIGHTS] + [(h, w) for w in FL.WIDE_WIDTHS for h in (1, 9)] + [(3, 2049)]


# ---------------------------------------------------------------- the builder
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_builder_round_trips_every_stride_and_offset(cn):
    for (h, w) in SHAPES:
        px = _image(h, w, cn)
        for kind in FL.STRIDE_KINDS:
            stride = FL.stride_of(kind, w, cn)
            for off in FL.base_offsets(cn):
                buf = FL.build(px, stride, off, seed=7)
                assert buf.dtype == np.uint8 and buf.ndim == 1
                assert buf.size == 2 * FL.MARGIN + off + stride * (h - 1) + w * cn          # the last row ends with its last pixel
                assert np.array_equal(FL.pixels(buf, h, w, cn, stride, off), px)
                y, x = h - 1, w - 1
                assert buf[FL.start(off) + y * stride + x * cn] == px.reshape(h, w, -1)[y, x, 0]          # the formula, once by hand
                assert FL.outside_unchanged(buf, buf.copy(), h, w, cn, stride, off)


def test_margins_and_fill():
    assert FL.MARGIN >= 64 and FL.MARGIN % 16 == 0 and FL.ALLOC_ALIGN % FL.MARGIN == 0
    assert FL.MARGIN > max(max(FL.base_offsets(cn)) for cn in (1, 3, 4)) + 16
    px = np.full((9, 5, 3), 77, np.uint8)
    a, b = FL.build(px, 32, 4, seed=1), FL.build(px, 32, 4, seed=2)
    pad = np.ones(a.shape, bool)
    pad[FL.pixel_index(9, 5, 3, 32, 4)] = False
    assert len(np.unique(a[pad])) > 100 and not np.array_equal(a[pad], b[pad])          # neither zeros nor a constant, and seeded
    assert np.array_equal(a, FL.build(px, 32, 4, seed=1))
    c = FL.build(px, 32, 4, fill=255)
    assert (c[pad] == 255).all() and np.array_equal(FL.pixels(c, 9, 5, 3, 32, 4), px)
    d = FL.build(px, 32, 4, fill=(10, 200))
    assert d[pad].min() >= 10 and d[pad].max() <= 200 and len(np.unique(d[pad])) > 50


def test_stride_kinds():
    for cn in (1, 3, 4):
        for w in FL.WIDTHS + FL.WIDE_WIDTHS + (61, 322):
            t = w * cn
            s = {k: FL.stride_of(k, w, cn) for k in FL.STRIDE_KINDS}
            assert s["tight"] == t and s["align4"] % 4 == 0 and t <= s["align4"] < t + 4
            assert s["align16"] % 16 == 0 and s["align16"] >= t and s["align16"] != s["align4"] and s["align16"] < t + 32
            assert s["plus"] == t + (4 if cn == 4 else 1)
    assert FL.stride_of("align4", 322, 3) == 968 and FL.stride_of("align16", 322, 3) == 976 and FL.stride_of("align16", 4, 4) == 32


def test_guard_check_reports_one_padding_byte_one_margin_byte_and_no_pixel():
    h, w, cn, stride, off = 9, 5, 3, 20, 1
    before = FL.build(_image(h, w, cn), stride, off)
    row_pad = FL.start(off) + 3 * stride + w * cn            # the first padding byte behind row 3
    for where in (row_pad, row_pad + stride - w * cn - 1, 0, FL.MARGIN + off - 1, FL.start(off) + FL.extent(h, w, cn, stride), before.size - 1):
        after = before.copy()
        after[where] ^= 1
        assert not FL.outside_unchanged(before, after, h, w, cn, stride, off), where
    for where in (FL.start(off), FL.start(off) + 3 * stride + w * cn - 1, FL.start(off) + FL.extent(h, w, cn, stride) - 1):
        after = before.copy()
        after[where] ^= 1
        assert FL.outside_unchanged(before, after, h, w, cn, stride, off), where
    assert not FL.outside_unchanged(before, before[:-1], h, w, cn, stride, off)
    # a store of `stride` bytes a row instead of the row's own bytes, the spill the guard is there for
    after = before.copy()
    after[FL.start(off):FL.start(off) + stride] = 0
    assert not FL.outside_unchanged(before, after, h, w, cn, stride, off)


# ---------------------------------------------------------------- the draws
def _covers(cases, **columns):
    for name, values in columns.items():
        assert {c[name] for c in cases} == set(values), name


@pytest.mark.parametrize("cn", [3, 4])
def test_gray_cases_cover_and_cross_aligned4(cn):
    cases = FL.GRAY_CASES[cn]
    assert 24 <= len(cases) <= 34
    _covers(cases, w=FL.WIDTHS + FL.WIDE_WIDTHS, h=FL.HEIGHTS, sk=FL.STRIDE_KINDS, off=FL.base_offsets(cn), mem=FL.MEMS, dk=("tight", "align16", "plus"))
    side = [FL.aligned4(c["stride"], c["mem"], FL.device_base(c["off"])) for c in cases]
    assert any(side) and not all(side)
    assert any(c["stride"] & 3 for c in cases) == (cn == 3)                                                      # generic by stride (BGRA rows are always 4-byte multiples)
    assert any(not (c["stride"] & 3) and c["mem"] == DEV and c["off"] % 16 for c in cases)                       # generic by base alone
    assert any(s and c["mem"] == DEV for s, c in zip(side, cases)) and any(s and c["mem"] == HOST for s, c in zip(side, cases))
    assert any(s and c["mem"] == HOST and c["off"] % 16 for s, c in zip(side, cases)) or cn == 4                  # a host base never counts
    assert any(c["dstride"] > c["w"] for c in cases) and any(c["dstride"] == c["w"] for c in cases)
    fast = [c for s, c in zip(side, cases) if s]
    assert any(c["w"] % 4 == 0 for c in fast) and any(c["w"] >= 1024 for c in fast)
    if cn == 3:
        # the byte-wise tail of k_gray_fast4: reached only by padded rows; on both memories, below one vector, and behind whole vectors
        tail = [c for c in fast if c["w"] % 4]
        assert {c["mem"] for c in tail} == {HOST, DEV}
        assert any(c["w"] < 4 for c in tail) and any(4 < c["w"] < 1024 for c in tail) and any(c["w"] > 1024 for c in tail)
        assert any(c["h"] > 8 for c in tail)


@pytest.mark.parametrize("name", ["EQUALIZE_CASES", "FLIP_CASES"])
def test_plane_cases_cover(name):
    cases = getattr(FL, name)
    assert len(cases) == 25
    _covers(cases, w=FL.WIDTHS, h=FL.HEIGHTS, sk=FL.STRIDE_KINDS, off=FL.base_offsets(1), mode=("host", "device", "inplace"))
    assert {c["dk"] for c in cases if c["mode"] != "inplace"} == set(FL.STRIDE_KINDS)
    for c in cases:
        assert c["mode"] != "inplace" or (c["dstride"], c["doff"]) == (c["stride"], c["off"])
        assert c["mem"] == (HOST if c["mode"] == "host" else DEV)
        assert c["stride"] >= c["w"] and c["dstride"] >= c["w"]
    assert any(c["mode"] == "device" and c["stride"] != c["dstride"] for c in cases)
    assert any(c["mode"] == "inplace" and c["stride"] > c["w"] for c in cases)
    assert any(c["mode"] != "host" and c["off"] % 4 for c in cases)


def test_resize_cases_cover():
    cases = FL.RESIZE_CASES
    assert 24 <= len(cases) <= 32
    assert {(c["geo"], c["cn"], c["mem"]) for c in cases} == {(g, cn, m) for g in FL.RESIZE_GEOMETRIES for cn in (1, 3) for m in FL.MEMS}
    _covers(cases, sk=FL.STRIDE_KINDS, dk=FL.STRIDE_KINDS, off=FL.base_offsets(1), doff=FL.base_offsets(1))
    for cn in (1, 3):
        for mem in FL.MEMS:
            mine = [c for c in cases if (c["cn"], c["mem"]) == (cn, mem)]
            assert any(c["stride"] > c["geo"][0] * cn for c in mine) and any(c["dstride"] > c["geo"][2] * cn for c in mine), (cn, mem)


def test_integral_cases_cover():
    assert {w for w, _, _, _ in FL.INTEGRAL_CASES} == {65, 257, 2049} and (2049, 3) in {(w, h) for w, h, _, _ in FL.INTEGRAL_CASES}
    for w in (65, 257, 2049):
        kinds = {k for ww, _, k, _ in FL.INTEGRAL_CASES if ww == w}
        assert "plus" in kinds and kinds & {"align4", "align16"}
    assert any(FL.stride_of(k, w, 1) % 2 for w, _, k, _ in FL.INTEGRAL_CASES)


def test_stream_layouts_cross_aligned4():
    W = FL.STREAM_W
    assert W % 4 and W * 3 % 4                                                 # the width whose tight BGR rows are not 4-byte aligned
    assert [FL.aligned4(s, m, FL.device_base(o)) for m, s, o in FL.STREAM_MIXED] == [True, False, True, False]
    assert FL.STREAM_MIXED == [(HOST, FL.stride_of("align4", W, 3), 0), (DEV, W * 3, 0), (DEV, FL.stride_of("align16", W, 3), 0), (DEV, FL.stride_of("align16", W, 3), 4)]
    # launch sets of the mixed batch: the padded host frame alone (fast kernel, with a tail), the tight device frame (generic by
    # stride), the two 976-byte frames together (generic because of ONE base)
    assert FL.face_launch_sets(FL.STREAM_MIXED) == [([0], True), ([1], False), ([2, 3], False)]
    assert FL.face_launch_sets(FL.STREAM_HOST_PADDED) == [([0, 1, 2, 3], True)]
    assert FL.face_launch_sets([(DEV, 976, 0), (DEV, 976, 0)]) == [([0, 1], True)]


def test_stream_geometries_and_the_sparse_ingest():
    W, H = FL.STREAM_W, FL.STREAM_H
    assert FL.working_size(W, H, W) == (W, H) and FL.working_size(W, H, 160) == (161, 121)          # identity; the exact-2x area resize
    assert FL.row_runs(H, 121) is None                                                              # (which reads every row anyway)
    assert FL.working_size(W, FL.SPARSE_H, FL.SPARSE_W2P) == (80, 60)
    assert FL.row_runs(FL.SPARSE_H, 60) == (1, 4, 2, 60)                                            # rows 4 k + 1, 4 k + 2: pitch 4 * stride
    assert FL.row_runs(1080, 90) == (5, 12, 2, 90)                                                  # the known answer tests/test_gpu_parity.py names


def test_tracker_cases_cross_trk_wide():
    by = {n: FL.trk_wide(DEV, FL.device_base(o), s, w) for n, w, _, s, o in FL.TRACKER_CASES}
    assert by == {"wide": True, "wide-padded": True, "narrow-stride": False, "narrow-base": False, "narrow-width": False, "narrow-width-alone": False}
    t = {n: (w, s, o) for n, w, _, s, o in FL.TRACKER_CASES}
    # each narrow case fails ONE term
    w, s, o = t["narrow-stride"]; assert w % 4 == 0 and s % 16 and o % 16 == 0
    w, s, o = t["narrow-base"]; assert w % 4 == 0 and s % 16 == 0 and o % 16
    w, s, o = t["narrow-width"]; assert w % 4 and s == w * 4 and o % 16 == 0
    w, s, o = t["narrow-width-alone"]; assert w % 4 and s % 16 == 0 and o % 16 == 0
    w, s, o = t["wide-padded"]; assert s > w * 4
    for n, w, h, s, o in FL.TRACKER_CASES:
        assert s >= w * 4 and h == FL.TRACKER_H
        host = FL.trk_wide(HOST, FL.device_base(o), s, w)
        assert host == (by[n] or n == "narrow-base")                           # a host frame is staged: its base never counts
    mixed = [FL.trk_wide(DEV, FL.device_base(o), s, w) for _, w, _, s, o in FL.TRACKER_MIXED]
    assert any(mixed) and not all(mixed) and len({(w, h) for _, w, h, _, _ in FL.TRACKER_MIXED}) == 1          # one launch set, sent narrow by one member


def test_draw_cases_cover():
    assert {c[0] for c in FL.DRAW_CASES} == {3, 4} and len(FL.DRAW_CASES) == 12
    for cn in (3, 4):
        strides = {sk: FL.draw_stride(sk, cn) for sk in ("tight", "align4", "plus7")}
        assert strides["tight"] == 61 * cn and strides["align4"] % 4 == 0 and strides["plus7"] == 61 * cn + 7
        assert {off for c, _, off in FL.DRAW_CASES if c == cn} == ({0, 1} if cn == 3 else {0, 4})
    assert len({FL.draw_stride(sk, 3) for sk in ("tight", "align4", "plus7")}) == 3
    # the shapes reach every border of the frame
    from draw_reference import _ref
    img = _ref(np.zeros((FL.DRAW_H, FL.DRAW_W, 3), np.uint8), FL.DRAW_SHAPES)
    m = img.any(axis=2)
    assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any() and not m.all()
    x, y, w, h = FL.OVERLAY_BOX
    assert 0 < x < FL.DRAW_W < x + w and 0 < y < FL.DRAW_H < y + h


def test_view_cases():
    x0, y0, w, h = FL.VIEW
    assert x0 % 2 and y0 % 2 and x0 + w <= FL.VIEW_PARENT_W and y0 + h <= FL.VIEW_PARENT_H
    assert {m for m, _, _ in FL.VIEW_CASES} == {HOST, DEV}
    for (x, y, vw, vh), small in ((FL.VIEW, False), (FL.VIEW_ALIGNED, False), (FL.VIEW_SMALL, True)):
        assert x + vw <= FL.VIEW_PARENT_W and y + vh <= FL.VIEW_PARENT_H and ((vw + 1) * (vh + 2) <= FL.ROI_MAX_WORDS) == small
    assert FL.VIEW_ALIGNED[0] % 4 == 0 and FL.VIEW_SMALL[0] % 2 and FL.VIEW_SMALL[1] % 2
    assert all(s > FL.VIEW_PARENT_W for m, s, _ in FL.VIEW_CASES if m == HOST)


# ---------------------------------------------------------------- trk_wide against trk_wide_ok
def test_trk_wide_is_trk_wide_ok(tmp_path):
    import test_trk_host_cpu as T
    if not os.path.exists(T.CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    driver = T._build_driver()
    B = 0x7f0000000000 + FL.ALLOC_ALIGN * 5
    cases = [("%s-%d" % (n, mem), mem, B + FL.start(o), w, s) for n, w, _, s, o in FL.TRACKER_CASES + FL.TRACKER_MIXED for mem in FL.MEMS]
    cases += [("sweep-%d-%d-%d-%d" % (mem, o, w, s), mem, B + o, w, s) for mem in FL.MEMS for o in (0, 1, 4, 8, 16, 32) for w in (316, 318, 320)
              for s in (1280, 1284, 1288, 1296)]
    lines = ["wide %s %d %d %d %d %d 0 0 0 0 0 0" % (cid, T.BGR, mem, base, w, s) for cid, mem, base, w, s in cases]
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([driver, str(manifest)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    got = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("{"):
            o = json.loads(ln)
            got[o["case"]] = o["wide"]
    assert len(got) == len({c[0] for c in cases})
    for cid, mem, base, w, s in cases:
        assert got[cid] == int(FL.trk_wide(mem, base, s, w)), cid
    assert set(got.values()) == {0, 1}
