"""bench.py as it is run: a plain line (the timed steps and nothing else), its --dump-outputs arrays (the same on a second run with
the same arguments), and --full (the oracle check of the last step, the CPU baseline) on a small batch.  Each run is a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "3", "--warmup", "1", "--frames-per-step", "4"]


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_line_and_dumped_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench(*SMALL, "--dump-outputs", str(a))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 4 * 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    for k in ("boxes_match", "cpu_baseline", "secondary"):
        assert k not in line, k                     # behind --full
    out = _load(a)
    assert sorted(out) == ["face_boxes", "face_counts", "face_ids"]
    assert all(v.dtype == np.float64 for v in out.values())
    assert out["face_boxes"].shape == (4, 64, 4) and out["face_ids"].shape == (4, 64) and out["face_counts"].shape == (4,)
    for i, n in enumerate(out["face_counts"].astype(int)):
        assert (out["face_boxes"][i, :n, 2:] > 0).all() and (out["face_boxes"][i, n:] == -1).all()
    assert out["face_counts"].sum() >= 4            # every frame holds pasted templates
    _bench(*SMALL, "--dump-outputs", str(b))
    again = _load(b)
    for k in out:
        assert np.array_equal(out[k], again[k]), k


def test_full_line_checks_the_last_step(tmp_path):
    line = _bench(*SMALL, "--full", "--no-secondary", "--dump-outputs", str(tmp_path))
    assert line["boxes_match"] is True, line.get("boxes_checked")
    assert line["boxes_checked"]["frames"] == 4
    assert line["cpu_baseline"]["value"] > 0
    out = _load(tmp_path)
    assert int(out["face_counts"].sum()) == line["boxes_checked"]["boxes"]


def test_face_tracker_dump(tmp_path):
    _bench("--workload", "face_tracker", "--streams-per-gpu", "2", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    out = _load(tmp_path)
    assert sorted(out) == ["face_boxes", "face_counts", "face_ids", "tracker_boxes", "tracker_counts"]
    assert out["tracker_boxes"].shape == (2, 256, 4) and all(v.dtype == np.float64 for v in out.values())
