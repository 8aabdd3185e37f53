"""NuboTracker's buffer layout (csrc/trk_layout.h) and the pure host parts of nvca_tracker_batch_process (csrc/trk_host.cpp) on the CPU:
tests/san/trk_host_driver.cpp, a stand-alone program built as tests/test_lbp_tables_cpu.py builds its driver (AddressSanitizer +
UndefinedBehaviorSanitizer, no preload, nothing loaded into Python) and WITHOUT any HIP include path, prints every offset and size the
header gives, the wide-kernel predicate, the launch sets, the staged sizes and the component lists; everything is compared with a
statement written here from the record comments of csrc/trk_layout.h and csrc/trk_host.h.  tests/motion_layouts.py keeps tile constants
and a roots_cap of its own: a third statement, compared as well.

What a kernel writing past an allocation would be -- a GPU fault -- is here an inequality: the parts of each buffer are disjoint and lie
inside the allocation, and the largest index a kernel can form (last slot, last row, last segment, last tile, last root entry, last
component) lies inside its part."""
import json
import os
import subprocess

import pytest

import motion_layouts as ML
from nubovca import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SIZES = [(5, 3), (64, 8), (256, 8), (257, 9), (513, 49), (520, 50), (1920, 1080)]
BATCHES = [1, 2, 3, 8]
INT = 4                                  # bytes of a word of the int buffers
BGR, NV12, I420 = capi.PIX_BGR, capi.PIX_NV12, capi.PIX_I420
HOST, DEV = capi.MEM_HOST, capi.MEM_DEVICE


def _build_driver():
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "trk_host_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(SAN, "trk_host_driver.cpp"), os.path.join(csrc, "trk_host.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in ("trk_host.h", "trk_layout.h", "device_records.h", "yuv_layout.h", "host_math.h")] + [os.path.join(ROOT, "include", "nubovca.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


def _up(v, a):
    return (v + a - 1) // a * a


# ---------------------------------------------------------------- the cases
def layout_cases():
    """(id, w, h, batch, div)"""
    out = [("%dx%dx%d" % (w, h, b), w, h, b, 8) for (w, h) in SIZES for b in BATCHES]
    out.append(("div1", 520, 50, 2, 1))
    out.append(("div3", 513, 49, 3, 3))
    out.append(("cap-clamped", 32768, 32768, 2, 1))          # 2^31 pixels in the set: the list stops at 2^30 entries
    return out


def _lay(o=(0, 0, 0), s=(0, 0, 0)):
    return tuple(o) + tuple(s)


def wide_cases():
    """(id, fmt, mem, base, width, stride, layout, expected): every alignment term on both sides of its limit"""
    B = 0x7f0000001000                                       # a 4096-aligned device address
    c = []
    # packed BGRA: w % 4, stride and a device base on 16 bytes
    c += [("bgra", BGR, DEV, B, 64, 256, _lay(), True), ("bgra-w66", BGR, DEV, B, 66, 272, _lay(), False), ("bgra-w68", BGR, DEV, B, 68, 272, _lay(), True),
          ("bgra-stride+8", BGR, DEV, B, 64, 264, _lay(), False), ("bgra-stride+16", BGR, DEV, B, 64, 272, _lay(), True),
          ("bgra-base+8", BGR, DEV, B + 8, 64, 256, _lay(), False), ("bgra-base+16", BGR, DEV, B + 16, 64, 256, _lay(), True),
          ("bgra-host-base+1", BGR, HOST, B + 1, 64, 256, _lay(), True), ("bgra-host-stride+8", BGR, HOST, B, 64, 264, _lay(), False),
          ("bgra-host-w66", BGR, HOST, B, 66, 272, _lay(), False)]
    # NV12: luma and chroma rows on 8 bytes; plane 2 is not read
    n = dict(o=[0, 4096, 0], s=[64, 64, 0])

    def nv(name, mem=DEV, base=B, width=64, o=None, s=None, exp=True):
        oo, ss = list(n["o"]), list(n["s"])
        for k, v in (o or {}).items(): oo[k] = v
        for k, v in (s or {}).items(): ss[k] = v
        c.append(("nv12" + name, NV12, mem, base, width, ss[0], _lay(oo, ss), exp))
    nv("")
    nv("-w66", width=66, exp=False); nv("-w68", width=68)
    nv("-y+4", o={0: 4}, exp=False); nv("-y+8", o={0: 8})
    nv("-ystride+4", s={0: 68}, exp=False); nv("-ystride+8", s={0: 72})
    nv("-uv+4", o={1: 4100}, exp=False); nv("-uv+8", o={1: 4104})
    nv("-uvstride+4", s={1: 68}, exp=False); nv("-uvstride+8", s={1: 72})
    nv("-base+4", base=B + 4, exp=False); nv("-base+8", base=B + 8)
    nv("-plane2-ignored", o={2: 1}, s={2: 1})
    nv("-host-base+3", mem=HOST, base=B + 3); nv("-host-y+4", mem=HOST, o={0: 4}, exp=False); nv("-host-uv+4", mem=HOST, o={1: 4100}, exp=False)
    # I420: luma rows on 8 bytes, both chroma planes on 4
    i = dict(o=[0, 4096, 6144], s=[64, 32, 32])

    def iy(name, mem=DEV, base=B, width=64, o=None, s=None, exp=True):
        oo, ss = list(i["o"]), list(i["s"])
        for k, v in (o or {}).items(): oo[k] = v
        for k, v in (s or {}).items(): ss[k] = v
        c.append(("i420" + name, I420, mem, base, width, ss[0], _lay(oo, ss), exp))
    iy("")
    iy("-w66", width=66, exp=False); iy("-w68", width=68)
    iy("-y+4", o={0: 4}, exp=False); iy("-y+8", o={0: 8})
    iy("-ystride+4", s={0: 68}, exp=False); iy("-ystride+8", s={0: 72})
    iy("-u+2", o={1: 4098}, exp=False); iy("-u+4", o={1: 4100})
    iy("-ustride+2", s={1: 34}, exp=False); iy("-ustride+4", s={1: 36})
    iy("-v+2", o={2: 6146}, exp=False); iy("-v+4", o={2: 6148})
    iy("-vstride+2", s={2: 34}, exp=False); iy("-vstride+4", s={2: 36})
    iy("-base+4", base=B + 4, exp=False); iy("-base+8", base=B + 8)
    iy("-host-base+2", mem=HOST, base=B + 2); iy("-host-v+2", mem=HOST, o={2: 6146}, exp=False)
    return c


def sets_cases():
    """(id, [(w, h, fmt)], expected sets): first-appearance order, members ascending"""
    a, b = (640, 480), (320, 240)
    return [("empty", [], []),
            ("one", [a + (BGR,)], [[0]]),
            ("all-alike", [a + (NV12,)] * 4, [[0, 1, 2, 3]]),
            ("interleaved", [a + (BGR,), b + (BGR,), a + (BGR,), a + (NV12,), b + (BGR,), a + (NV12,), a + (I420,), (640, 482, BGR), b + (BGR,)],
             [[0, 2], [1, 4, 8], [3, 5], [6], [7]]),
            ("width-only-differs", [(640, 480, BGR), (644, 480, BGR), (640, 480, BGR)], [[0, 2], [1]]),
            ("last-first", [b + (I420,), a + (BGR,), a + (BGR,), b + (I420,)], [[0, 3], [1, 2]])]


def staged_cases():
    """(id, fmt, stride, w, h, layout)"""
    return [("packed-exact", BGR, 256, 64, 2, _lay()), ("packed-up", BGR, 260, 64, 3, _lay()), ("packed-1080p", BGR, 7680, 1920, 1080, _lay()),
            ("nv12-tight", NV12, 64, 64, 48, _lay([0, 3072, 0], [64, 64, 0])), ("nv12-padded", NV12, 70, 64, 48, _lay([0, 3400, 0], [70, 70, 0])),
            ("nv12-chroma-first", NV12, 64, 64, 48, _lay([2000, 0, 0], [64, 64, 0])),
            ("i420-tight", I420, 64, 64, 48, _lay([0, 3072, 3840], [64, 32, 32])), ("i420-padded", I420, 72, 64, 48, _lay([16, 3600, 4600], [72, 40, 36])),
            ("i420-1080p", I420, 1920, 1920, 1080, _lay([0, 2073600, 2592000], [1920, 960, 960]))]


COMPS = {
    # id: (batch, [(slot, seed, x, y, w, h)])
    "none": (3, []),
    "one-slot": (1, [(0, 900, 9, 9, 1, 1), (0, 5, 5, 0, 2, 3), (0, 40, 4, 4, 4, 4)]),
    "interleaved-slots": (3, [(2, 70, 1, 2, 3, 4), (0, 300, 5, 6, 7, 8), (2, 7, 9, 10, 11, 12), (0, 2, 13, 14, 15, 16), (2, 8, 17, 18, 19, 20), (0, 299, 21, 22, 23, 24)]),
    "empty-slot-between": (3, [(2, 1, 1, 1, 1, 1), (0, 1, 2, 2, 2, 2)]),
    "slot-negative": (2, [(0, 1, 1, 1, 1, 1), (-1, 2, 2, 2, 2, 2)]),
    "slot-is-batch": (2, [(1, 1, 1, 1, 1, 1), (2, 2, 2, 2, 2, 2)]),
}
COUNTS = {"count-0": 0, "count-cap": 1 << 18, "count-over": (1 << 18) + 1, "count-negative": -1}
ERR_SLOT = "internal: motion component of an unknown slot (device result rejected)"
ERR_NEGATIVE = "internal: negative component count"
ERR_OVER = "tracker: more motion components than the list holds"


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """{case: the driver's answer}"""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    tmp = tmp_path_factory.mktemp("trk_host")
    driver = _build_driver()
    lines = ["layout %s %d %d %d %d" % c for c in layout_cases()]
    lines += ["wide %s %d %d %d %d %d " % c[:6] + " ".join(str(v) for v in c[6]) for c in wide_cases()]
    lines += ["sets %s %d " % (cid, len(keys)) + " ".join("%d %d %d" % k for k in keys) for cid, keys, _ in sets_cases()]
    lines += ["staged %s %d %d %d %d " % c[:5] + " ".join(str(v) for v in c[5]) for c in staged_cases()]
    lines += ["count %s %d" % kv for kv in COUNTS.items()]
    lines += ["comps %s %d %d " % (cid, batch, len(comps)) + " ".join(str(v) for comp in comps for v in comp) for cid, (batch, comps) in COMPS.items()]
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


# ---------------------------------------------------------------- the layout
def expected_layout(w, h, batch, div):
    """trk_layout.h's record comments, restated"""
    nseg, trows = -(-w // 256), -(-h // 8)                   # a segment is 256 pixels of a row, a tile 8 rows of a segment
    per = nseg * trows
    e = dict(seg_per_row=nseg, tile_rows=trows, tiles_per_slot=per, tile_w=256, tile_h=8, tile_waves=4, rows=[8, 2, 16])
    # flag bytes [batch][h][nseg], then on the next multiple of 64 an int per slot; every 16th row is counted
    cells = nseg * h * batch
    e.update(flag_first=0, flag_last=cells - 1, flag_second_row=nseg, count_offset=_up(cells, 64), flag_bytes=_up(cells, 64) + INT * batch,
             counts_at=_up(cells, 64), counted=[1, 0, 1], counted_rows=-(-h // 16))
    # tile list: marks, list, counts of set 0, counts of set 1; tick t counts in set t & 1 and clears set (t + 1) & 1
    marks, lst, cnt0, cnt1 = 0, per * batch, 2 * per * batch, 2 * per * batch + batch
    e.update(tiles_list_offset=lst, tiles_count_offset=[cnt0, cnt1], tiles_words=2 * per * batch + 2 * batch, tile_last=per - 1, tile_second_row=nseg,
             tile_list=[[marks, lst, cnt1, cnt0, per], [marks, lst, cnt0, cnt1, per]])
    cap = min(w * h * batch // div, 1 << 30)
    e["roots"] = dict(entries=0, overflowed=1, error=2, error_words=3, hdr=8, cap=cap, words=8 + cap + 64)
    e["comp"] = dict(count=0, flags=1, hdr=2, bit_overflowed=1, bit_error=2, words=6, cap=1 << 18, first=1024, at=[2, 8, 2 + 6 * 1024, 2 + 6 * (1 << 18)])
    return e


@pytest.mark.parametrize("case", layout_cases(), ids=[c[0] for c in layout_cases()])
def test_every_offset_and_size(run, case):
    cid, w, h, batch, div = case
    got, exp = run[cid], expected_layout(w, h, batch, div)
    bad = [k for k in sorted(set(got) | set(exp)) if got.get(k) != exp.get(k)]
    assert not bad, [(k, got.get(k), exp.get(k)) for k in bad[:3]]


@pytest.mark.parametrize("case", layout_cases(), ids=[c[0] for c in layout_cases()])
def test_parts_are_disjoint_and_the_largest_indices_lie_inside(run, case):
    cid, w, h, batch, div = case
    o = run[cid]
    nseg, per = o["seg_per_row"], o["tiles_per_slot"]
    # flags (bytes): the cells, then the counts
    cells_end = o["flag_last"] + 1
    assert cells_end == nseg * h * batch                                       # last slot, last row, last segment
    assert cells_end <= o["count_offset"] and o["count_offset"] % INT == 0
    assert o["count_offset"] + INT * (batch - 1) + INT <= o["flag_bytes"]        # the last slot's count
    # tiles (words): four parts in order, each as long as what indexes it
    marks, lst, now, nxt, per_slot = o["tile_list"][0]
    assert per_slot == per and o["tile_last"] == per - 1                       # last row, last segment -> the slot's last tile
    parts = sorted([(marks, per * batch), (lst, per * batch), (now, batch), (nxt, batch)])
    assert parts[0][0] == 0 and all(a + n <= b for (a, n), (b, _) in zip(parts, parts[1:])) and parts[-1][0] + parts[-1][1] <= o["tiles_words"]
    assert marks + (batch - 1) * per + o["tile_last"] < lst                      # the last slot's last mark
    assert lst + (batch - 1) * per + (per - 1) < min(now, nxt)                   # a slot lists at most its `per` tiles (a mark admits one entry a tick)
    assert {now, nxt} == set(o["tiles_count_offset"]) and o["tile_list"][1][2:4] == [nxt, now]      # the two sets change places with the tick
    # roots (words): header, error record inside it, entries
    r = o["roots"]
    assert max(r["entries"], r["overflowed"]) < r["error"] and r["error"] + r["error_words"] <= r["hdr"]
    assert r["hdr"] + r["cap"] - 1 < r["words"] and r["cap"] <= 1 << 30
    # component list (words): header, then `words` per component; the last word of the last component, and the first read-back
    c = o["comp"]
    assert c["at"][0] == c["hdr"] and {c["count"], c["flags"]} == {0, 1} and c["bit_overflowed"] & c["bit_error"] == 0
    assert c["hdr"] + c["words"] * (c["cap"] - 1) + c["words"] - 1 < c["at"][3] and c["at"][2] <= c["at"][3]


def test_the_third_statement_agrees(run):
    """tests/motion_layouts.py builds its layouts on constants of its own"""
    for (w, h) in SIZES:
        for b in BATCHES:
            o = run["%dx%dx%d" % (w, h, b)]
            assert (o["tile_w"], o["tile_h"], o["tile_waves"] * ML.WAVE) == (ML.TILE_W, ML.TILE_H, ML.TILE_W)
            assert o["roots"]["cap"] == ML.roots_cap(w, h, b)
            assert o["tiles_per_slot"] == (-(-w // ML.TILE_W)) * (-(-h // ML.TILE_H))
    assert run["cap-clamped"]["roots"]["cap"] == 1 << 30 and run["div1"]["roots"]["cap"] == 520 * 50 * 2 and run["div3"]["roots"]["cap"] == 513 * 49


# ---------------------------------------------------------------- the pure host parts
@pytest.mark.parametrize("case", wide_cases(), ids=[c[0] for c in wide_cases()])
def test_wide_kernel_predicate(run, case):
    assert run[case[0]]["wide"] == int(case[7])


def test_wide_cases_cover_both_sides_of_every_term():
    ids = [c[0] for c in wide_cases()]
    assert len(set(ids)) == len(ids)
    for fmt, terms in (("bgra", ("w66", "stride+8", "base+8")), ("nv12", ("w66", "y+4", "ystride+4", "uv+4", "uvstride+4", "base+4")),
                       ("i420", ("w66", "y+4", "ystride+4", "u+2", "ustride+2", "v+2", "vstride+2", "base+4"))):
        by = {c[0]: c[7] for c in wide_cases() if c[0].startswith(fmt)}
        assert by[fmt] is True
        for t in terms:
            lo = fmt + "-" + t
            hi = fmt + "-" + t[:-1] + str(int(t[-1]) * 2) if "+" in t else fmt + "-w68"
            assert by[lo] is False and by[hi] is True, (lo, hi)
        assert any(k.startswith(fmt + "-host") and v for k, v in by.items()) and any(k.startswith(fmt + "-host") and not v for k, v in by.items())


@pytest.mark.parametrize("case", sets_cases(), ids=[c[0] for c in sets_cases()])
def test_launch_sets(run, case):
    cid, keys, exp = case
    assert run[cid]["sets"] == exp and run[cid]["members"] == len(keys)
    # first-appearance order, members ascending, as a statement of its own
    first = []
    for k in keys:
        if k not in first:
            first.append(k)
    assert exp == [[i for i, k in enumerate(keys) if k == f] for f in first]


def _yuv_extent(fmt, w, h, lay):
    """bytes from the base to the end of the last plane (csrc/yuv_layout.h): plane 0 has h rows of w bytes; NV12's plane 1 h / 2 rows of w;
    I420's planes 1 and 2 h / 2 rows of w / 2"""
    o, s = lay[:3], lay[3:]
    planes = [(0, h, w)] + ([(1, h // 2, w)] if fmt == NV12 else [(1, h // 2, w // 2), (2, h // 2, w // 2)])
    return max(o[p] + s[p] * (rows - 1) + rb for p, rows, rb in planes)


@pytest.mark.parametrize("case", staged_cases(), ids=[c[0] for c in staged_cases()])
def test_staged_bytes(run, case):
    cid, fmt, stride, w, h, lay = case
    o = run[cid]
    if fmt == BGR:
        copied = stride * (h - 1) + w * 4                  # what caller_h2d is asked to copy
        assert o["staged"] == _up(stride * h, 256) and copied <= o["staged"]
    else:
        assert o["extent"] == _yuv_extent(fmt, w, h, lay) and o["staged"] == _up(o["extent"], 256)
    assert o["staged"] % 256 == 0                          # the next frame starts aligned: a staged frame counts as base 0
    assert run["packed-up"]["staged"] == 1024 and run["packed-exact"]["staged"] == 512 and run["nv12-padded"]["staged"] == 5120


@pytest.mark.parametrize("cid", sorted(COMPS))
def test_component_lists(run, cid):
    batch, comps = COMPS[cid]
    o = run[cid]
    if cid.startswith("slot-"):
        assert (o["rc"], o["err"], o["lists"]) == (capi.ERR_INTERNAL, ERR_SLOT, [])
        return
    assert (o["rc"], o["err"]) == (0, "")
    assert o["lists"] == [[list(c[2:]) for c in sorted(comps, key=lambda c: c[1]) if c[0] == b] for b in range(batch)]


def test_component_count_refusals(run):
    assert [run[k]["rc"] for k in ("count-0", "count-cap", "count-over", "count-negative")] == [0, 0, capi.ERR_OVERFLOW, capi.ERR_INTERNAL]
    assert [run[k]["err"] for k in ("count-0", "count-cap", "count-over", "count-negative")] == ["", "", ERR_OVER, ERR_NEGATIVE]
