"""The packed 4:2:2 conversion statement (tests/yuv422_reference.py) on the CPU: hand-derived answers, the vectorised
statement against a scalar loop over the buffer's bytes on all three byte orders, and the premises of tests/test_gpu_yuv422.py --
  (a) there are frames whose rows 2k and 2k + 1 carry different chroma, and a 4:2:0-style reading of them gives another image;
  (b) each byte order read as each other one gives another gray image;
  (c) a 4:2:0 frame re-packed as 4:2:2 by repeating chroma rows gives A.13's image exactly;
  (d) the tracker scenes' movers change the chroma only: a kernel that takes Y for gray sees fewer components;
  (e) the case lists lie on both sides of every term of the two wide-kernel predicates
-- so that the GPU cases cannot pass on a kernel that shares chroma vertically, confuses the byte orders or ignores the chroma."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import yuv_cases as Y
import yuv_reference as R420
import yuv422_cases as K
import yuv422_reference as R
import yuv_stream_scenes as S
from nubovca import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(y0, y1, u, v, fmt):
    b = [0, 0, 0, 0]
    py, pu, pv = R.POS[fmt]
    b[py], b[py + 2], b[pu], b[pv] = y0, y1, u, v
    buf = np.array(b, np.uint8)
    lay = (fmt, (0, 0, 0), (4, 0, 0))
    return R.bgr(buf, 2, 1, lay), R.bgr_scalar(buf, 2, 1, lay)


# (Y, U, V) -> (B, G, R), derived by hand from A.13's integers; in the comments the value before the clamp where it clamps
KNOWN = [((16, 128, 128), (0, 0, 0)),
         ((235, 128, 128), (255, 255, 255)),          # 219 * 1220542 + 2^19 = 267822986 -> 255 after the shift
         ((235, 255, 128), (255, 205, 255)),          # B 511: saturates upwards
         ((16, 0, 128), (0, 50, 0)),                  # B -258: saturates downwards
         ((235, 128, 255), (255, 152, 255)),          # R 458
         ((16, 128, 0), (0, 104, 0)),                 # R -204
         ((235, 0, 0), (0, 255, 51)),                 # G 409 (and B -3)
         ((16, 255, 255), (255, 0, 203)),             # G -153 (and B 256)
         ((5, 128, 200), (0, 0, 115)),                # Y < 16 counts as 16: the answer of (16, 128, 200)
         ((16, 128, 200), (0, 0, 115)),
         ((81, 90, 240), (0, 0, 254)),                # B and G shift to -1 (an arithmetic shift of a negative sum)
         ((128, 100, 180), (74, 99, 213))]


@pytest.mark.parametrize("fmt", R.FMTS, ids=R.FMT_IDS)
@pytest.mark.parametrize("yuv,bgr", KNOWN, ids=lambda v: "-".join(str(x) for x in v))
def test_known_answers(yuv, bgr, fmt):
    """both pixels of a pair carry the answer of their own luma with the pair's chroma: pixel 1 is (16, U, V)'s"""
    a, b = _pair(yuv[0], 16, yuv[1], yuv[2], fmt)
    assert (a[0, 0] == np.array(bgr, np.uint8)).all() and np.array_equal(a, b), (a.tolist(), b.tolist())
    second = dict(KNOWN).get((16, yuv[1], yuv[2]))
    if second is not None:
        assert (a[0, 1] == np.array(second, np.uint8)).all(), a.tolist()


def test_byte_positions_are_the_formats_names():
    """YUY2 = Y0 U Y1 V, UYVY = U Y0 V Y1, YVYU = Y0 V Y1 U; the package's table is the statement's"""
    assert R.POS == {4: (0, 1, 3), 5: (1, 0, 2), 6: (0, 3, 1)} == synth.YUV422_POS
    from nubovca import capi
    assert (capi.PIX_YUY2, capi.PIX_UYVY, capi.PIX_YVYU) == (R.YUY2, R.UYVY, R.YVYU) == (4, 5, 6)
    hdr = open(os.path.join(ROOT, "include", "nubovca.h")).read()
    for name, val in (("YUY2", 4), ("UYVY", 5), ("YVYU", 6)):
        assert re.search(r"#define NVCA_PIX_%s %d\b" % (name, val), hdr)


@pytest.mark.parametrize("fmt", R.FMTS, ids=R.FMT_IDS)
@pytest.mark.parametrize("w,h,pad,base", [(34, 17, 0, 0), (34, 17, 5, 3), (2, 1, 0, 0), (18, 3, 16, 16)])
def test_statement_against_scalar_loop(fmt, w, h, pad, base):
    """every byte random (the extremes forced in), padded strides, a base offset, odd heights"""
    buf, lay = K.random_frame(w, h, fmt, pad, base, 11 + fmt + w)
    buf[base:base + 4] = [0, 255, 16, 235]
    got, exp = R.bgr(buf, w, h, lay), R.bgr_scalar(buf, w, h, lay)
    assert np.array_equal(got, exp)
    if w * h > 100:
        assert got.min() == 0 and got.max() == 255
    assert R.extent(w, h, lay) == len(buf)


@pytest.mark.parametrize("fmt", R.FMTS, ids=R.FMT_IDS)
def test_make_yuv422_layouts(fmt):
    """the three byte orders of one seed hold the same samples; padding and a base offset move them without changing them; the buffer
    ends with the last pixel; what is no pixel holds noise, not a constant"""
    w, h = 64, 37
    a = synth.make_yuv422(w, h, 9, fmt, "natural", [(10, 6, 24)])
    b = synth.make_yuv422(w, h, 9, fmt, "natural", [(10, 6, 24)], pad=12, base=7)
    c = synth.make_yuv422(w, h, 9, R.FMTS[(R.FMTS.index(fmt) + 1) % 3], "natural", [(10, 6, 24)])
    pa, pb, pc = R.planes(a[0], w, h, a[1]), R.planes(b[0], w, h, b[1]), R.planes(c[0], w, h, c[1])
    for k in range(3):
        assert np.array_equal(pa[k], pb[k]) and np.array_equal(pa[k], pc[k])
    assert pa[0].min() >= 16 and pa[0].max() <= 235
    assert len(a[0]) == 2 * w * h and len(b[0]) == 7 + (2 * w + 12) * (h - 1) + 2 * w and b[1][2][0] == 2 * w + 12 and b[1][1][0] == 7
    padding = np.asarray(b[0])[7:7 + (2 * w + 12) * (h - 1)].reshape(h - 1, 2 * w + 12)[:, 2 * w:]
    assert len(np.unique(padding)) > 16 and len(np.unique(np.asarray(b[0])[:7])) > 2


# ---------------------------------------------------------------- (a)
@pytest.mark.parametrize("fmt", R.FMTS, ids=R.FMT_IDS)
def test_premise_a_rows_carry_their_own_chroma(fmt):
    frames = [K.varying_frame(34, 17, fmt, 3, 1), K.varying_frame(328, 250, fmt), K.hd_frame(fmt)]
    for (buf, lay), (w, h) in zip(frames, [(34, 17), (328, 250), (1920, 1080)]):
        _, u, v = R.planes(buf, w, h, lay)
        assert (u[0::2][:h // 2] != u[1::2]).mean() > 0.5 and (v[0::2][:h // 2] != v[1::2]).mean() > 0.5
        own, shared = R.bgr(buf, w, h, lay), R.bgr_shared_rows(buf, w, h, lay)
        assert np.array_equal(own[0::2], shared[0::2])
        go, gs = R.gray(own)[1::2].astype(int), R.gray(shared)[1::2].astype(int)
        diff, far = (go != gs).mean(), (abs(go - gs) >= 8).mean()
        print(w, h, "odd-row gray pixels a vertically sharing reader gets wrong: %.3f, by 8 or more: %.3f" % (diff, far))
        # gray is nearly blind to chroma (the luma weights undo the conversion) until a channel saturates: one pair in eight does in each row,
        # so about 2 * 1/8 * 7/8 of the odd-row pixels move far and a good part of the rest by a rounding step
        assert diff > 0.25 and far > 0.05


def test_premise_a_a_sharing_reader_gets_another_raw_list_from_the_1080p_frame():
    """the face case on this frame compares raw candidate lists: the statement's list is long, and the list of the image a vertically
    sharing reader computes is another one"""
    raw = K.hd_expected()
    assert len(raw) >= 40
    buf, lay = K.hd_frame(R.YUY2)
    for fmt in R.FMTS[1:]:
        b2, l2 = K.hd_frame(fmt)
        assert np.array_equal(R.bgr(b2, 1920, 1080, l2), R.bgr(buf, 1920, 1080, lay))
    other = K.hd_raw(R.bgr_shared_rows(buf, 1920, 1080, lay))
    print("raw windows", len(raw), "of a vertically sharing reader", len(other))
    assert not np.array_equal(raw, other)


# ---------------------------------------------------------------- (b)
def test_premise_b_byte_orders_are_told_apart():
    frames = {"varying": lambda f: K.varying_frame(328, 250, f), "tail": lambda f: K.frame("tail", 0, f), "trk": lambda f: K.trk_frame(160, 120, 1, f),
              "part": lambda f: K.part_frame(322, 242, 0, f)}
    sizes = {"varying": (328, 250), "tail": (328, 250), "trk": (160, 120), "part": (322, 242)}
    for name, get in frames.items():
        w, h = sizes[name]
        for fmt in R.FMTS:
            buf, lay = get(fmt)
            right = R.gray(R.bgr(buf, w, h, lay))
            for wrong in R.FMTS:
                if wrong != fmt:
                    assert (R.gray(R.bgr(buf, w, h, (wrong,) + lay[1:])) != right).mean() > 0.05, (name, fmt, wrong)


# ---------------------------------------------------------------- (c)
@pytest.mark.parametrize("fmt", R.FMTS, ids=R.FMT_IDS)
def test_premise_c_repacked_420_frames_give_a13s_image(fmt):
    for fset, i, pad, base in (("sd", 0, 0, 0), ("tail", 2, 4, 8), ("p720", 1, 0, 16)):
        W, H = Y.SETS[fset][:2]
        buf, lay = K.frame(fset, i, fmt, pad, base)
        assert np.array_equal(R.bgr(buf, W, H, lay), Y.frame_bgr(fset, i)), (fset, i)
    for W, H in K.PART_GEOS:
        buf, lay = K.part_frame(W, H, 3, fmt, 6, 2)
        assert np.array_equal(R.bgr(buf, W, H, lay), S.part_bgr(W, H, 3))
    for W, H in ((160, 120), (322, 242), (644, 482)):
        buf, lay = K.trk_frame(W, H, 2, fmt, 2, 4)
        assert np.array_equal(R.bgr(buf, W, H, lay), S.trk_bgra(W, H, 2)[..., :3])
        assert np.array_equal(K.trk_bgra(W, H, 2), S.trk_bgra(W, H, 2))
    buf, lay = K.trk_frame(160, 121, 2, fmt)
    assert np.array_equal(R.bgr(buf, 160, 121, lay), S.trk_bgra(160, 122, 2)[:121, :, :3])


def test_oracle_finds_what_the_gpu_cases_look_for():
    for fset, n in (("sd", 9), ("p720", 8), ("tail", 8)):
        assert sum(1 for b, _ in Y.sequence_expected("synthetic", fset, n) if len(b)) >= n // 2
    for W, H in K.PART_GEOS:
        for kind in ("eye", "nose", "mouth", "ear"):
            assert sum(len(a) + len(b) for a, b in S.part_expected(kind, W, H)[:K.PART_FRAMES]) > 0, (kind, W, H)


# ---------------------------------------------------------------- (d)
@pytest.mark.parametrize("W,H", [(160, 120), (322, 242), (644, 482), (160, 121)], ids=lambda v: str(v))
def test_premise_d_tracker_scenes_need_the_chroma(W, H):
    exp = K.trk_expected(W, H)
    luma = S.oracle_tracker_run([K.trk_luma_bgra(W, H, i) for i in range(S.TRK_FRAMES)])
    n_exp, n_luma = [len(b) for b in exp], [len(b) for b in luma]
    print(W, H, "components per frame:", n_exp, "with luma taken as gray:", n_luma)
    assert n_exp[0] == 0 and all(n >= 1 for n in n_exp[1:]), n_exp
    assert n_exp != n_luma and sum(n_exp) > sum(n_luma), (n_exp, n_luma)


# ---------------------------------------------------------------- (e)
def test_premise_e_case_lists_lie_on_both_sides_of_every_predicate_term():
    """for every term of a predicate there is a case the kernel choice of which flips with that term alone"""
    def flips(cases, terms):
        seen = set()
        for c in cases:
            t = terms(c)
            if all(t):
                seen.add("all")
            for k in range(len(t)):
                if not t[k] and all(t[:k] + t[k + 1:]):
                    seen.add(k)
        return seen

    def gray_terms(c):
        fset, pad, base, shift, mem = c
        W, _, w2p = Y.SETS[fset][:3]
        return (W == w2p, base % 16 == 0, (2 * W + pad) % 16 == 0, mem == "host" or shift % 16 == 0)

    def trk_terms(c):
        W, H, pad, base, shift, mem = c
        return (W % 4 == 0, ((0 if mem == "host" else shift) + base) % 8 == 0, (2 * W + pad) % 8 == 0)
    assert flips(K.FACE_KERNEL_CASES, gray_terms) == {"all", 0, 1, 2, 3}
    assert flips(K.TRK_CASES, trk_terms) == {"all", 0, 1, 2}
    for c in K.FACE_KERNEL_CASES:
        assert (K.face_kernel(c) == K.GRAY_WIDE) == all(gray_terms(c)), c
    for c in K.TRK_CASES:
        assert (K.trk_kernel(c) == K.TRK_WIDE) == all(trk_terms(c)), c
    assert {K.trk_kernel(c) for c in K.TRK_CASES if c[:2] == (160, 121)} == {K.TRK_WIDE, K.TRK_GENERIC}
    assert any(Y.SETS[c[0]][0] % 16 for c in K.FACE_KERNEL_CASES if K.face_kernel(c) == K.GRAY_WIDE)         # a short unit ends the wide rows
    # the primitive's list: every width and height the issue names, 34 x 200, every layout kind
    assert {c[0] for c in K.PRIM_CASES} == {2, 14, 16, 18, 30, 32, 34} and {1, 2, 3, 17, 200} <= {c[1] for c in K.PRIM_CASES}
    assert {(p, b) for _, _, p, b in K.PRIM_CASES} >= set(K.PRIM_LAYOUTS)
    for w in K.PRIM_WIDTHS:
        assert len({(p, b) for ww, _, p, b in K.PRIM_CASES if ww == w}) >= 4, w


# ---------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from nubovca import capi
    return capi.load()


def test_header_declares_and_the_library_exports_the_primitive(lib):
    hdr = open(os.path.join(ROOT, "include", "nubovca.h")).read()
    assert re.search(r"int nvca_yuv422_to_bgr\(nvca_ctx \*ctx, const void \*base, int w, int h, const nvca_pixel_layout \*layout, int mem,\s+void \*dst_bgr, int dst_stride\);", hdr)
    from nubovca import capi
    assert "nvca_yuv422_to_bgr" in capi.SYMBOLS and getattr(C.CDLL(capi.LIB_PATH), "nvca_yuv422_to_bgr") is not None
    assert lib.nvca_yuv422_to_bgr.argtypes == lib.nvca_yuv420_to_bgr.argtypes


def test_set_input_refuses_null_handles_without_a_device(lib):
    from nubovca import capi
    lay = capi.pixel_layout(R.YUY2, (0, 0, 0), (1280, 0, 0))
    for name in ("nvca_face_stream_set_input", "nvca_part_stream_set_input", "nvca_tracker_set_input"):
        assert getattr(lib, name)(None, C.byref(lay)) == capi.ERR_ARG
