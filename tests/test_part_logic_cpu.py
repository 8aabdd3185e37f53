"""The per-frame state machine of the eye / nose / mouth / ear elements (csrc/part_logic.cpp: conf_images scales, __receive_event and
the frame gate, face-to-ROI geometry, find_ears, the merge calls, the eye hysteresis, snapshot and roll-back) on the CPU, under
AddressSanitizer + UndefinedBehaviorSanitizer.  tests/san/parts_driver.cpp runs whole streams through it -- gate -> images -> face pass
-> ROIs -> searches -> finish, as the library's batched call does -- with the oracle's image and detection primitives in place of the
GPU; the lists it prints must equal orc.PartStream's frame by frame.  The driver's compile line has no HIP include path and no
-D__HIP_PLATFORM_AMD__: part_logic.cpp, host_logic.cpp and cascade_xml.cpp build without any HIP header."""
import json
import os
import subprocess

import numpy as np
import pytest

from part_scenes import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "san")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

KINDS = {"eye": (0, "righteye", "lefteye"), "nose": (1, "nose", None), "mouth": (2, "mouth", None), "ear": (3, "leftear", "rightear")}
# (name, W, H, properties, two faces); frames: scene(W, H, 9, 700 + W, two) -- the sequences of tests/test_gpu_parts.py
CONFIGS = [
    ("defaults", 640, 480, {}, False),
    ("int_scale", 800, 600, {}, False),                                  # width / 320 = 2.5: the int-scale truncation quirk
    ("every_2nd", 640, 480, {"process_x_every_4": 2, "scale_factor_pct": 15}, False),
    ("width_640", 640, 480, {"width_to_process": 640}, False),
    ("two_faces", 320, 240, {}, True),
]
SEQUENCES = ["%s-%s" % (k, c[0]) for k in KINDS for c in CONFIGS]
EVENTS = ["%s-event" % k for k in ("eye", "nose", "mouth")]
ROLLBACKS = {"nose-rollback": ("nose", {"process_x_every_4": 2}), "mouth-rollback": ("mouth", {"detect_event": 1}), "ear-rollback": ("ear", {})}


def _build_driver():
    import orc
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(SAN, "build", "parts_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    so = orc.build()
    srcs = [os.path.join(SAN, "parts_driver.cpp")] + [os.path.join(csrc, f) for f in ("part_logic.cpp", "host_logic.cpp", "cascade_xml.cpp")]
    deps = srcs + [so, os.path.join(ROOT, "oracle", "nvca_oracle.h")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        # (function sections, unused ones dropped: host_logic.cpp's overlay blend calls into plan.cpp, which is not part of this driver)
        cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
               "-ffp-contract=off", "-ffunction-sections", "-Wl,--gc-sections", "-I", os.path.join(ROOT, "include"), "-w"] + srcs + \
              [so, "-Wl,-rpath," + os.path.dirname(so), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory, synth_xml):
    """every case through the driver (one process, started first) and through the oracle's PartStream (meanwhile):
    {case id: [(list A, list B) per frame]} of each"""
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ with sanitizer runtimes")
    import orc
    from nubovca import synth
    tmp = tmp_path_factory.mktemp("part_logic")
    driver = _build_driver()
    xml = {n: synth.synthetic_part_cascade_xml(n) for names in KINDS.values() for n in names[1:] if n}
    xml["face"] = synth_xml
    paths, cpu = {}, {}
    for n, x in xml.items():
        paths[n] = str(tmp / (n + ".xml"))
        with open(paths[n], "w") as f:
            f.write(x)
        cpu[n] = orc.parse_cascade_xml(x)
    scenes = {}

    def frames_of(W, H, n, seed, two=False):
        key = (W, H, n, seed, two)
        if key not in scenes:
            fr = scene(W, H, n, seed, two)
            raw = str(tmp / ("frames_%d_%d_%d_%d_%d.raw" % (W, H, n, seed, two)))
            with open(raw, "wb") as f:
                for a in fr:
                    f.write(np.ascontiguousarray(a, np.uint8).tobytes())
            scenes[key] = (fr, raw)
        return scenes[key]

    cases, lines = [], []          # (id, kind, properties, frames, {frame: faces pushed before it})

    def add(cid, kind, props, key, pushes=None, twin=0):
        fr, raw = frames_of(*key)
        p = dict(width_to_process=320, process_x_every_4=4, scale_factor_pct=25, detect_event=0)
        p.update(props)
        k, a, b = KINDS[kind]
        lines.append("S %s %d %d %d %d %d %s %s %s %d %d %d %s %d" % (cid, k, p["width_to_process"], p["process_x_every_4"], p["scale_factor_pct"], p["detect_event"],
                                                                    paths["face"], paths[a], paths[b] if b else "-", key[0], key[1], len(fr), raw, twin))
        for i, boxes in sorted((pushes or {}).items()):
            lines.append("F %d %d %s" % (i, len(boxes), " ".join(str(int(v)) for v in np.asarray(boxes).reshape(-1))))
        cases.append((cid, kind, props, fr, pushes or {}))

    for kind in KINDS:
        for name, W, H, props, two in CONFIGS:
            add("%s-%s" % (kind, name), kind, props, (W, H, 9, 700 + W, two))
    # faces arrive from an upstream face detector (original-frame pixels); some frames come without a message
    fs = orc.FaceStream(cpu["face"])
    ev = {i: fs.process(f)[0] for i, f in enumerate(frames_of(640, 480, 8, 900)[0]) if i % 3 != 2}
    for kind in ("eye", "nose", "mouth"):
        add("%s-event" % kind, kind, {"detect_event": 1}, (640, 480, 8, 900), ev)
    # the streams of test_part_batch_late_failure_leaves_every_stream_untouched, each with a twin that is disturbed on frames 1, 2 and 4
    fs = orc.FaceStream(cpu["face"])
    boxes = [fs.process(f)[0] for f in frames_of(640, 480, 6, 5150)[0]]
    rb = {t: b for t, b in enumerate(boxes) if len(b) and t != 3}
    for cid, (kind, props) in ROLLBACKS.items():
        add(cid, kind, props, (640, 480, 6, 5150), rb if props.get("detect_event") else None, twin=1)
    script = tmp / "script.txt"
    script.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.Popen([driver, str(script)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    try:
        expect = {}
        for cid, kind, props, fr, pushes in cases:
            k, a, b = KINDS[kind]
            o = orc.PartStream(k, cpu["face"], cpu[a], cpu[b] if b else None, **props)
            expect[cid] = []
            for i, f in enumerate(fr):
                if i in pushes:
                    o.push_faces(pushes[i])
                ea, eb = o.process(f)
                expect[cid].append((ea.tolist(), eb.tolist()))
        out, err = proc.communicate(timeout=900)
    finally:
        if proc.poll() is None:
            proc.kill()
    assert proc.returncode == 0, (out[-2000:], err[-4000:])
    assert "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err[-4000:]
    got, done = {}, None
    for ln in out.splitlines():
        o = json.loads(ln)
        if "cases" in o:
            done = o["cases"]
            continue
        assert o["frame"] == len(got.setdefault(o["case"], [])), o
        got[o["case"]].append((o["a"], o["b"]))
    assert done == len(cases) == len(SEQUENCES) + len(EVENTS) + len(ROLLBACKS)          # no case is left out
    return got, expect


def _same(got, expect, cid, ref):
    assert len(got[cid]) == len(expect[ref]) > 0
    seen = 0
    for i, ((ga, gb), (ea, eb)) in enumerate(zip(got[cid], expect[ref])):
        assert ga == ea and gb == eb, (cid, i, ga, ea, gb, eb)
        seen += len(ea) + len(eb)
    assert seen > 0, cid


@pytest.mark.parametrize("cid", SEQUENCES)
def test_part_logic_sequence_equals_the_oracle(runs, cid):
    got, expect = runs
    _same(got, expect, cid, cid)


@pytest.mark.parametrize("cid", EVENTS)
def test_part_logic_detect_event_equals_the_oracle(runs, cid):
    got, expect = runs
    _same(got, expect, cid, cid)


@pytest.mark.parametrize("cid", sorted(ROLLBACKS))
def test_part_logic_rollback_leaves_the_stream_untouched(runs, cid):
    """A stream whose frame went through the gate and the ROI step and was then restored from its snapshot -- what a batched call does
    that fails late -- runs on exactly like its undisturbed twin (and both like the oracle's stream, which never saw the failed call):
    frame gates, queued face events (detect-event stream), result lists, the ear detector's no-detection counter.  One call in flight
    only: with two tickets, a failed collect of the second restores the lists to their state before the first was collected."""
    got, expect = runs
    _same(got, expect, cid, cid)
    assert got[cid + "_twin"] == got[cid], (cid, got[cid + "_twin"], got[cid])
