"""Part streams on new-format LBP cascades (nvca_part_stream_create_any) on the GPU, against the elements' own per-frame logic around
the numpy statement's detections (tests/lbp_part_cases.py: csrc/part_logic.cpp behind tests/part_logic_shim.cpp; pinned against the
oracle's part stream by tests/test_lbp_parts_cpu.py): both output lists, frame by frame, np.array_equal.  Every kind with all roles LBP,
Haar and LBP roles mixed, detect-event mode, NV12 frames, eight streams in one batched call in both slot orders, two tickets in flight,
the same with roi = 0, and the refusals of both entry points.  Every test that makes a stream with any_format=True fails on a
library without the entry point."""
import ctypes as C

import numpy as np
import pytest

import lbp_cases as K
import lbp_part_cases as P
from nubovca import capi

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(P.shim() is None, reason="no clang++")]
CAP = 256
KIND_LIST = ["eye", "nose", "mouth", "ear"]


@pytest.fixture(scope="module")
def env():
    ctx = capi.Context(0)
    dev = {("lbp", n): ctx.load_cascade_xml(K.cascade(n)[0]) for n in (P.FACE, P.PART_A, P.PART_B)}
    dev.update({("haar", n): ctx.load_cascade_xml(x) for n, x in P.haar_xml().items()})
    yield ctx, dev
    ctx.close()


def _stream(env, kind, face_lbp=True, parts_lbp=True, **props):
    ctx, dev = env
    face, a, b = P.role_names(kind, face_lbp, parts_lbp)
    return capi.PartStream(ctx, P.KINDS[kind], dev[face], dev[a], dev[b] if b else None, any_format=True, **props)


def _same(got, exp, what):
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (what, got[0].tolist(), exp[0].tolist(), got[1].tolist(), exp[1].tolist())


def _booked(ctx, fn):
    ctx.enable_kernel_timing(1)
    before = ctx.kernel_timing()
    out = fn()
    after = ctx.kernel_timing()
    ctx.enable_kernel_timing(0)
    return out, {k: v[1] - before.get(k, (0, 0))[1] for k, v in after.items() if v[1] > before.get(k, (0, 0))[1]}


# ------------------------------------------------------------------ single streams
@pytest.mark.parametrize("kind", KIND_LIST)
@pytest.mark.parametrize("roi", [1, 0])
def test_every_kind_with_all_roles_lbp(env, kind, roi):
    exp = P.expected(kind, True, True)
    assert sum(len(a) + len(b) for a, b in exp) > 0
    with env[0].options(roi=roi):
        s = _stream(env, kind)
        for i, f in enumerate(P.lbp_frames()):
            _same(s.process(f, cap=CAP), exp[i], (kind, roi, i))
        s.close()


def test_part_searches_take_the_small_route_and_the_switch_turns_it_off(env):
    """a nose stream's frame: its 160 x 120 face pass and its part searches are small LBP jobs -- one small-image round per phase under
    cascade_roi, nothing under cascade_strip; with roi = 0 it is the other way round"""
    ctx = env[0]
    f = P.lbp_frames()[0]
    for roi in (1, 0):
        with ctx.options(roi=roi):
            s = _stream(env, "nose")
            got, booked = _booked(ctx, lambda: s.process(f, cap=CAP))
            _same(got, P.expected("nose", True, True)[0], roi)
            s.close()
        if roi:
            assert "cascade_strip" not in booked and booked.get("cascade_roi") == 2, booked          # the face pass, the part searches
        else:
            assert "cascade_roi" not in booked and booked.get("cascade_strip", 0) >= 2, booked


@pytest.mark.parametrize("kind,face_lbp,parts_lbp", [("eye", False, True), ("nose", False, True), ("mouth", True, False), ("ear", True, False)])
def test_haar_and_lbp_roles_mix(env, kind, face_lbp, parts_lbp):
    exp = P.expected(kind, face_lbp, parts_lbp, "mixed")
    s = _stream(env, kind, face_lbp, parts_lbp)
    for i, f in enumerate(P.mixed_frames()):
        _same(s.process(f, cap=CAP), exp[i], (kind, i))
    s.close()


@pytest.mark.parametrize("kind", ["eye", "nose", "mouth"])
def test_detect_event_mode_with_pushed_faces(env, kind):
    exp = P.expected(kind, True, True, event=True)
    assert sum(len(a) + len(b) for a, b in exp) > 0
    s = _stream(env, kind, detect_event=1)
    for i, f in enumerate(P.lbp_frames()):
        if i != 2:
            s.push_faces(P.lbp_face_boxes(640, 480, i))
        _same(s.process(f, cap=CAP), exp[i], (kind, i))
    s.close()


def test_a_322_x_242_frame(env):
    exp = P.expected("ear", True, True, W=322, H=242)
    assert sum(len(a) for a, b in exp) > 0 and sum(len(b) for a, b in exp) > 0
    s = _stream(env, "ear")
    for i, f in enumerate(P.lbp_frames(322, 242)):
        _same(s.process(f, cap=CAP), exp[i], i)
    s.close()


def test_nv12_frames(env):
    exp = P.expected("mouth", True, True, nv12=True)
    assert sum(len(a) for a, b in exp) > 0
    s = _stream(env, "mouth")
    lay = P.nv12_of(P.lbp_frames()[0])[1]
    s.set_input(capi.pixel_layout(*lay))
    for i, f in enumerate(P.lbp_frames()):
        buf = np.array(P.nv12_of(f)[0])
        _same(s.process(capi.make_planar_frame(buf, 640, 480, capi.pixel_layout(*lay)), cap=CAP), exp[i], i)
    s.close()


def test_set_params_between_frames(env):
    """set_params on a stream made by the new entry point: the same kind is taken, another kind refused"""
    s = _stream(env, "nose")
    p = capi.PartParams()
    env[0].L.nvca_part_params_default(C.byref(p), capi.PART_NOSE)
    p.scale_factor_pct = 30
    assert env[0].L.nvca_part_stream_set_params(s.h, C.byref(p)) == capi.OK
    p.kind = capi.PART_EYE
    assert env[0].L.nvca_part_stream_set_params(s.h, C.byref(p)) == capi.ERR_ARG
    s.close()


# ------------------------------------------------------------------ batched calls
def _eight(env):
    """(stream, expectation arguments) x 8: the four kinds all-LBP, and four with Haar and LBP roles mixed, all on the mixed frames"""
    cfg = [(k, True, True) for k in KIND_LIST] + [("eye", False, True), ("nose", False, True), ("mouth", True, False), ("ear", False, False)]
    return [(_stream(env, *c), c) for c in cfg]


@pytest.mark.parametrize("roi", [1, 0])
def test_eight_streams_in_one_call_in_both_slot_orders(env, roi):
    """Haar-only, LBP-only and mixed streams in ONE nvca_part_batch_process: every stream's lists are those of the stream alone, in
    either slot order, and the Haar and LBP small jobs of a search phase share ONE small-image round (k_roi and k_roi_lbp under one
    cascade_roi booking), not one per stream"""
    ctx = env[0]
    frames = P.mixed_frames()
    with ctx.options(roi=roi):
        for order in (1, -1):
            pairs = _eight(env)[::order]
            for i, f in enumerate(frames):
                res, booked = _booked(ctx, lambda: capi.part_batch_process(ctx, [s for s, _ in pairs], [f] * len(pairs), cap=CAP))
                for (s, c), got in zip(pairs, res):
                    _same(got, P.expected(*c, "mixed")[i], (roi, order, c, i))
                if roi and i == 0:
                    # frame 0 runs every stream: the face passes in one round, the part searches in one (FIND_BIGGEST searches on the Haar part
                    # cascades that narrow take one more) -- far fewer rounds than the eight streams
                    assert 2 <= booked.get("cascade_roi", 0) <= 4, booked
            for s, _ in pairs:
                s.close()


def test_two_tickets_in_flight(env):
    ctx = env[0]
    frames = P.lbp_frames()
    a = [(_stream(env, k), k) for k in ("eye", "nose")]
    b = [(_stream(env, k), k) for k in ("mouth", "ear")]
    for i in range(0, len(frames)):
        ta = capi.part_batch_submit(ctx, [s for s, _ in a], [frames[i]] * 2)
        tb = capi.part_batch_submit(ctx, [s for s, _ in b], [frames[i]] * 2)
        for tk, group in ((ta, a), (tb, b)):
            for (s, k), got in zip(group, capi.part_batch_collect(ctx, tk, cap=CAP)):
                _same(got, P.expected(k, True, True)[i], (k, i))
    for s, _ in a + b:
        s.close()


# ------------------------------------------------------------------ refusals
def test_refusals_of_both_entry_points(env):
    ctx, dev = env
    L = ctx.L
    lbp, haar = dev[("lbp", P.FACE)], dev[("haar", "face")]
    h = C.c_void_p()
    p = capi.PartParams()
    L.nvca_part_params_default(C.byref(p), capi.PART_EYE)
    # the old entry point still refuses an LBP cascade in every role
    for r in ((lbp, haar, haar), (haar, lbp, haar), (haar, haar, lbp)):
        assert L.nvca_part_stream_create(ctx.h, C.byref(p), r[0].h, r[1].h, r[2].h, C.byref(h)) == capi.ERR_UNSUPPORTED and L.nvca_last_error(ctx.h)
    # the new one makes nvca_part_stream_create's refusals: null arguments, a bad kind, a missing second cascade for EYE / EAR
    create = L.nvca_part_stream_create_any
    assert create(None, C.byref(p), lbp.h, lbp.h, lbp.h, C.byref(h)) == capi.ERR_ARG
    assert create(ctx.h, None, lbp.h, lbp.h, lbp.h, C.byref(h)) == capi.ERR_ARG
    assert create(ctx.h, C.byref(p), None, lbp.h, lbp.h, C.byref(h)) == capi.ERR_ARG
    assert create(ctx.h, C.byref(p), lbp.h, None, lbp.h, C.byref(h)) == capi.ERR_ARG
    assert create(ctx.h, C.byref(p), lbp.h, lbp.h, lbp.h, None) == capi.ERR_ARG
    assert create(ctx.h, C.byref(p), lbp.h, lbp.h, None, C.byref(h)) == capi.ERR_ARG          # EYE needs b
    p.kind = capi.PART_EAR
    assert create(ctx.h, C.byref(p), haar.h, lbp.h, None, C.byref(h)) == capi.ERR_ARG
    for bad in (-1, 4):
        p.kind = bad
        assert create(ctx.h, C.byref(p), lbp.h, lbp.h, lbp.h, C.byref(h)) == capi.ERR_ARG
    p.kind = capi.PART_NOSE
    assert create(ctx.h, C.byref(p), lbp.h, haar.h, None, C.byref(h)) == capi.OK and h.value
    L.nvca_part_stream_destroy(h)


def test_three_haar_cascades_make_the_old_streams_stream(env):
    """on three old-format cascades the new entry point's stream answers as nvca_part_stream_create's -- and as the oracle's part stream --
    on the Haar scenes of tests/part_scenes.py"""
    import orc
    from part_scenes import scene
    ctx, dev = env
    cpu = {n: orc.parse_cascade_xml(x) for n, x in P.haar_xml().items()}
    for kind in ("eye", "nose", "ear"):
        face, a, b = P.role_names(kind, False, False)
        old = capi.PartStream(ctx, P.KINDS[kind], dev[face], dev[a], dev[b] if b else None)
        new = _stream(env, kind, False, False)
        o = orc.PartStream(P.KINDS[kind], cpu[face[1]], cpu[a[1]], cpu[b[1]] if b else None)
        seen = 0
        for i, f in enumerate(scene(640, 480, 6, 700 + 640)):
            eo = o.process(f)
            _same(new.process(f, cap=CAP), eo, (kind, i))
            _same(old.process(f, cap=CAP), eo, (kind, i))
            seen += len(eo[0]) + len(eo[1])
        assert seen > 0
        old.close(); new.close()
