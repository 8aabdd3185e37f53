"""The parity tests of the primitives and the detectMultiScale variants once more, in a child process whose device buffers are
mapped between unmapped guard ranges and end where their mappings end (NVCA_ALLOC_GUARD=2: csrc/runtime.cpp, "electric fence"; released
buffers are unmapped too): a kernel that reads or writes past one of the library's buffers, or touches a released one, faults at
that access and takes the child down -- every time, not now and then as on an ordinary heap.  (In a child: a fault ends the process.)
A second child runs the raw-list cases of the batched 1080p face path (tests/test_gpu_raw_batch.py): the parity file shows k_band
images of at most 700 x 500, and the tiles of a 1080p plan that hold no candidate are where a read past a plane stays silent."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _guarded_child(test_file, select, timeout, min_guarded):
    env = dict(os.environ, NVCA_ALLOC_GUARD="2", NVCA_ALLOC_LOG="1", HSA_ENABLE_VM_FAULT_MESSAGE="1", NVCA_GUARD_CHILD="1")
    cmd = [sys.executable, "-m", "pytest", "-s", "-x", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", test_file), "-k", select]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    if "guard unavailable" in out:
        pytest.skip("this runtime refuses the virtual-memory calls the guard allocator needs")
    tail = "\n".join(out.splitlines()[-40:])
    summary = [ln for ln in out.splitlines() if " passed" in ln or " failed" in ln]
    print("guarded child:", summary[-1] if summary else "(no summary line)", "| guarded allocations:", out.count("guarded)"))
    assert "Memory access fault" not in out, tail
    assert r.returncode == 0, tail
    assert " passed" in out and out.count("guarded)") > min_guarded, tail


@pytest.mark.gpu
def test_kernels_stay_inside_their_buffers():
    _guarded_child("test_gpu_parity.py", "detect or resize or integral or gray or equalize or flip or group", 900, 20)


@pytest.mark.gpu
def test_batched_1080p_face_path_stays_inside_its_buffers():
    """one run of the full-cascade and prefix-5 1080p batches between guard ranges.  A fault here is a finding: read it from the
    faulting address and the allocation log in the child's output, do not run it again to see it again."""
    _guarded_child("test_gpu_raw_batch.py", "test_headline_full_cascades or (test_prefixes_through_band and prefix5)", 600, 20)
