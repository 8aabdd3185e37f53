"""The tracker's component kernels (csrc/kernels_trk_ccl.hip behind the pixel pass of csrc/kernels_trk_pixel.hip) on motion histories built by construction (tests/motion_layouts.py; that
every layout is in the regime it is named for is checked on the host, tests/test_motion_layouts_cpu.py).

Everything goes through the C ABI and is compared with np.array_equal, in order, frame by frame, against the oracle tracker:
  (a) every layout on four routes: the folded path (trk_fold 1) and the per-pixel kernels (trk_fold 0) with trk_order -1, 0 and 1;
  (b) the combs and the 520 x 50 random fields as device frames;
  (c) the 520 x 50 layouts of equal length in batched calls of up to 8 slots, each slot with timestamps and parameters of its own,
      in both slot orders, and one call that mixes 520 x 50 and 513 x 49 trackers (two launch sets);
  (d) the root list on both sides of its limit, by the number of `tracker` launches the kernel timers count: 3250 tile roots answer
      with one launch and 3251 with two (the fallback), 6500 + 0 of a two-slot call with one and 6500 + 1 with two; the frames after a
      fallback match as well (it runs on the history the first launch left);
  (e) 1024 and 1025 components, the end of the host's first read-back;
  (f) serpentine, comb and two copies of the 2 x 2 patterns as NV12 and I420 trackers, behind both 4:2:0 pixel kernels;
  (g) a living tracker through serpentine and comb, a change to 513 x 49 and back.

What these comparisons cannot see is written down in README.md ("tests/test_gpu_motion_layouts.py")."""
import numpy as np
import pytest

import motion_layouts as M
import yuv_reference as R
import yuv_stream_scenes as S

pytestmark = pytest.mark.gpu

CAP = 8192
ROUTES = {"fold": dict(trk_fold=1), "pixel_auto": dict(trk_fold=0, trk_order=-1), "pixel_down": dict(trk_fold=0, trk_order=0),
          "pixel_outside_in": dict(trk_fold=0, trk_order=1)}
WIDE, GENERAL = "k_trk_pixel_yuv8", "k_trk_pixel_yuv"


@pytest.fixture(scope="module")
def ctx():
    from nubovca import capi
    c = capi.Context(0)
    try:
        yield c
    finally:
        c.close()


class timed:
    """the context's kernel launches inside a with-block (name -> launches)"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.enable_kernel_timing(1)
        return self

    def __exit__(self, *exc):
        self.kt = {k: v[1] for k, v in self.ctx.kernel_timing().items()}
        self.ctx.enable_kernel_timing(0)

    def n(self, name):
        return self.kt.get(name, 0)


def _same(got, exp, what):
    n = min(len(got), len(exp))
    d = np.nonzero((got[:n] != exp[:n]).any(axis=1))[0]
    first = int(d[0]) if len(d) else n
    assert np.array_equal(got, exp), "%s: %d boxes, the oracle has %d; first difference at index %d\n got %s\n exp %s" % (
        what, len(got), len(exp), first, got[first:first + 6].tolist(), exp[first:first + 6].tolist())


def _tracker(ctx, name):
    from nubovca import capi
    return capi.Tracker(ctx, **M.gpu_props(M.LAYOUTS[name][3]))


_KEEP = []


def _frame(img, mem="host"):
    from nubovca import capi
    if mem == "host":
        return capi.make_frame(np.array(img))
    import torch
    t = torch.from_numpy(np.array(img)).cuda()
    torch.cuda.synchronize()
    _KEEP.append(t)
    return capi.make_frame(t.data_ptr(), img.shape[1], img.shape[0], img.shape[1] * 4, capi.MEM_DEVICE)


def _call(ctx, trks, frames, tss):
    from nubovca import capi
    return capi.tracker_batch_process(ctx, trks, frames, tss, cap=CAP)


def _launches(names, k):
    """`tracker` launches of one launch set that holds frame k of these layouts on the folded path: a second one when the tile roots
    of all slots together exceed the root list"""
    w, h = M.size(names[0])
    total = sum(int(M.model(n, k)["tile_roots"].sum()) for n in names) if k > 0 else 0
    return 2 if total > M.roots_cap(w, h, len(names)) else 1


def _run_layout(ctx, name, mem="host"):
    age, K, tss, params = M.LAYOUTS[name]
    exp = M.expected(name)
    t = _tracker(ctx, name)
    for k, f in enumerate(M.frames(name)):
        _same(_call(ctx, [t], [_frame(f, mem)], [tss[k]])[0], exp[k], "%s, frame %d, %s" % (name, k, mem))
    t.close()


# ---------------------------------------------------------------- (a) every layout, four routes
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", M.NAMES)
def test_layout(ctx, name, route):
    with ctx.options(**ROUTES[route]):
        _run_layout(ctx, name)


# ---------------------------------------------------------------- (b) device frames
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", ["comb", "comb_up", "random_fields/0.35", "random_fields/0.7", "random_fields/1"])
def test_layout_device_frames(ctx, name, route):
    assert M.size(name) == (M.W0, M.H0)
    with ctx.options(**ROUTES[route]):
        _run_layout(ctx, name, "device")
    _KEEP.clear()


# ---------------------------------------------------------------- (c) batched calls
def _groups():
    """the 520 x 50 layouts by their number of frames, in calls of at most 8 slots"""
    by_k = {}
    for n in M.NAMES:
        if M.size(n) == (M.W0, M.H0):
            by_k.setdefault(M.LAYOUTS[n][1], []).append(n)
    out = []
    for K in sorted(by_k):
        names = by_k[K]
        out += [names[i:i + 8] for i in range(0, len(names), 8)]
    return out


def test_groups_cover_the_slot_parameters():
    g = _groups()
    assert sorted(n for names in g for n in names) == sorted(n for n in M.NAMES if M.size(n) == (M.W0, M.H0))
    assert max(len(names) for names in g) == 8
    full = [names for names in g if len(names) == 8]
    # slots of one call differ in timestamps, seg_thresh, the area window and mhi_duration
    assert any(len({M.LAYOUTS[n][2] for n in names}) >= 3 for names in full)
    assert any(len({M.LAYOUTS[n][3]["seg_thresh"] for n in names}) >= 3 for names in full)
    assert any(len({M.LAYOUTS[n][3]["min_area"] for n in names}) >= 2 for names in full)


def _run_batch(ctx, names, count_launches=False):
    K = M.LAYOUTS[names[0]][1]
    trks = [_tracker(ctx, n) for n in names]
    for k in range(K + 1):
        with timed(ctx) as t:
            res = _call(ctx, trks, [_frame(M.frames(n)[k]) for n in names], [M.LAYOUTS[n][2][k] for n in names])
        for s, n in enumerate(names):
            _same(res[s], M.expected(n)[k], "slot %d of %d (%s), frame %d" % (s, len(names), n, k))
        if count_launches:
            assert t.n("tracker") == _launches(names, k), (names, k, t.kt)
    for x in trks:
        x.close()


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("g", range(len(_groups())))
def test_batched_slots(ctx, g, reverse, route):
    names = _groups()[g]
    with ctx.options(**ROUTES[route]):
        _run_batch(ctx, names[::-1] if reverse else names)


@pytest.mark.parametrize("route", ["fold", "pixel_auto"])
def test_one_call_of_two_sizes(ctx, route):
    """520 x 50 and 513 x 49 trackers alternate in one call: two launch sets that share the workspace, the live-tile list and the root
    list; the combs (3 frames) leave the call early"""
    names = ["chain_of_ages", "chain_of_ages@513x49", "comb", "comb@513x49", "random_fields/0.7@513x49", "random_fields/0.7",
             "unseeded_neighbours@513x49", "unseeded_neighbours", "comb_up@513x49", "comb_up"]
    assert {M.size(n) for n in names} == {(M.W0, M.H0), (M.W1, M.H1)}
    with ctx.options(**ROUTES[route]):
        trks = {n: _tracker(ctx, n) for n in names}
        for k in range(5):
            who = [n for n in names if k <= M.LAYOUTS[n][1]]
            with timed(ctx) as t:
                res = _call(ctx, [trks[n] for n in who], [_frame(M.frames(n)[k]) for n in who], [M.LAYOUTS[n][2][k] for n in who])
            for n, got in zip(who, res):
                _same(got, M.expected(n)[k], "%s, frame %d" % (n, k))
            assert t.n("tracker") == 2, t.kt
        for x in trks.values():
            x.close()


# ---------------------------------------------------------------- (d) the root list at its limit
@pytest.mark.parametrize("name,launches", [("roots_at_cap", 1), ("roots_over_cap", 2)])
def test_root_list_limit_of_one_slot(ctx, name, launches):
    """3250 tile roots fill the list of a 520 x 50 slot, the 3251st sends the frame through the per-pixel kernels: a second launch on
    the history the first one left.  Frames 2 (the lattice still there, a blob over part of it) and 3 (the lattice expired) follow"""
    assert _launches([name], 1) == launches and _launches([name], 3) == 1
    with ctx.options(trk_fold=1):
        _run_batch(ctx, [name], count_launches=True)


@pytest.mark.parametrize("other,launches", [(None, 1), ("one_blob", 2)])
@pytest.mark.parametrize("lattice_slot", [0, 1])
def test_root_list_limit_of_two_slots(ctx, other, launches, lattice_slot):
    """two slots share a list of 6500 entries: 6500 single pixels in one slot and an empty history in the other fit, one blob in the
    other slot does not -- and then both slots' lists come from the fallback"""
    from nubovca import capi
    full = "roots_full_lattice"
    age, K, tss, params = M.LAYOUTS[full]
    b_age, b_K, b_tss, b_params = M.LAYOUTS[other] if other else M.blank(M.W0, M.H0, K)
    b_frames = M.frames(other) if other else M.paint(b_age, b_K)
    b_exp = M.expected(other) if other else [np.zeros((0, 4), np.int32)] * (K + 1)
    assert b_K == K
    with ctx.options(trk_fold=1):
        pair = [capi.Tracker(ctx, **M.gpu_props(params)), capi.Tracker(ctx, **M.gpu_props(b_params))]
        for k in range(K + 1):
            frames, ts, exp = [_frame(M.frames(full)[k]), _frame(b_frames[k])], [tss[k], b_tss[k]], [M.expected(full)[k], b_exp[k]]
            sl = slice(None, None, -1) if lattice_slot else slice(None)
            with timed(ctx) as t:
                res = _call(ctx, pair[sl], frames[sl], ts[sl])
            for s, (got, e) in enumerate(zip(res, exp[sl])):
                _same(got, e, "slot %d, frame %d" % (s, k))
            roots = (int(M.model(full, k)["tile_roots"].sum()) + (int(M.model(other, k)["tile_roots"].sum()) if other else 0)) if k else 0
            assert t.n("tracker") == (2 if roots > M.roots_cap(M.W0, M.H0, 2) else 1), (k, roots, t.kt)
            if k == 1:
                assert roots == 6500 + (1 if other else 0) and t.n("tracker") == launches
        for x in pair:
            x.close()


@pytest.mark.parametrize("name", ["comb", "comb_up", "serpentine"])
def test_layouts_below_the_limit_answer_with_one_launch(ctx, name):
    """1563 tile roots that fold into one root, a component in every tile: one launch a frame"""
    with ctx.options(trk_fold=1):
        assert all(_launches([name], k) == 1 for k in range(M.LAYOUTS[name][1] + 1))
        _run_batch(ctx, [name], count_launches=True)


@pytest.mark.parametrize("name,launches", [("random_fields/0.35", [1, 1, 1, 2, 2]), ("random_fields/0.7", [1, 1, 2, 2, 2]), ("random_fields/1", [1, 2, 1, 1, 1])])
def test_random_fields_alone_meet_the_limit_from_both_sides(ctx, name, launches):
    """a random field alone is answered by the folded path on some frames and by the fallback on others (tile roots against 3250:
    tests/test_motion_layouts_cpu.py); in the 8-slot calls of test_batched_slots the list is 8 times as long and the folded path answers all"""
    assert [_launches([name], k) for k in range(5)] == launches
    with ctx.options(trk_fold=1):
        _run_batch(ctx, [name], count_launches=True)


def test_batched_random_fields_stay_on_the_folded_path(ctx):
    names = [g for g in _groups() if "random_fields/1" in g][0]
    assert len(names) == 8 and all(_launches(names, k) == 1 for k in range(5))
    with ctx.options(trk_fold=1):
        _run_batch(ctx, names, count_launches=True)


# ---------------------------------------------------------------- (e) the host's two-part read-back
@pytest.mark.parametrize("route", ["fold", "pixel_auto"])
@pytest.mark.parametrize("name,n", [("readback_1024", 1024), ("readback_1025", 1025)])
def test_readback_boundary(ctx, name, n, route):
    age, K, tss, params = M.LAYOUTS[name]
    with ctx.options(**ROUTES[route]):
        t = _tracker(ctx, name)
        _call(ctx, [t], [_frame(M.frames(name)[0])], [tss[0]])
        got = _call(ctx, [t], [_frame(M.frames(name)[1])], [tss[1]])[0]
        assert len(got) == n
        _same(got, M.expected(name)[1], name)
        t.close()


# ---------------------------------------------------------------- (f) 4:2:0 trackers
def _planes(img):
    """Y 16 / 235 where the painted frame is 0 / 255, chroma 128: the conversion gives the painted frame back"""
    h, w = img.shape[:2]
    y = np.where(img[..., 0] == 255, 235, 16).astype(np.uint8)
    u = np.full((h // 2, w // 2), 128, np.uint8)
    assert np.array_equal(R.convert(y, u, u), img[..., :3])
    return y, u, u


@pytest.mark.parametrize("fmt", [R.NV12, R.I420], ids=["nv12", "i420"])
@pytest.mark.parametrize("name,kernel", [("serpentine", WIDE), ("comb", WIDE), ("patterns_2x2/0@270x384", GENERAL), ("patterns_2x2/7@270x384", GENERAL)])
def test_layout_as_yuv_tracker(ctx, name, kernel, fmt, capfd):
    from nubovca import capi
    age, K, tss, params = M.LAYOUTS[name]
    w, h = M.size(name)
    exp = M.expected(name)
    capfd.readouterr()
    with ctx.options(plan_debug=1):
        t = _tracker(ctx, name)
        lay = None
        for k, img in enumerate(M.frames(name)):
            buf, ltuple = S.pack_planes(*_planes(img), fmt)
            if lay is None:
                lay = capi.pixel_layout(*ltuple)
                t.set_input(lay)
            _same(_call(ctx, [t], [capi.make_planar_frame(np.array(buf), w, h, lay)], [tss[k]])[0], exp[k], "%s, frame %d" % (name, k))
        t.close()
    ran = [ln.rsplit(": ", 1)[1] for ln in capfd.readouterr().err.splitlines() if ln.startswith("[nvca plan] 4:2:0 tracker pass")]
    assert ran == [kernel] * (K + 1), ran


# ---------------------------------------------------------------- (g) a size change on a living tracker
@pytest.mark.parametrize("route", ["fold", "pixel_auto"])
def test_size_change_resets_the_history(ctx, route):
    """serpentine and comb at 520 x 50, then comb at 513 x 49 (entered at its frame 1: against the zeroed previous image every lit pixel
    moves), then one_blob at 520 x 50 again -- one oracle tracker sees the same frames.  Nothing of the earlier size may survive: the
    serpentine's rows would join the blob (timestamps 20 apart), and its previous image would move where the blob's frame is dark"""
    from nubovca import capi
    script = [("serpentine", 0), ("serpentine", 1), ("comb", 1), ("comb", 2), ("comb@513x49", 1), ("comb@513x49", 2), ("one_blob", 1), ("one_blob", 2), ("one_blob", 3)]
    frames = [M.frames(n)[k] for n, k in script]
    tss = [1000.0 + 20.0 * i for i in range(len(script))]
    params = M.LAYOUTS["comb"][3]
    exp = M.oracle_run(frames, tss, params)
    assert [len(e) for e in exp] == [0, 1, 1, 1, 2, 1, 1, 1, 1]
    assert exp[2].tolist() == [[0, 0, 520, 49]] and exp[6].tolist() == [[100, 17, 8, 4]]       # the comb joins the serpentine; the blob joins nothing
    with ctx.options(**ROUTES[route]):
        t = capi.Tracker(ctx, **M.gpu_props(params))
        for i, f in enumerate(frames):
            _same(_call(ctx, [t], [_frame(f)], [tss[i]])[0], exp[i], "step %d %s" % (i, script[i]))
        t.close()
