"""tests/test_gpu_levels.py once more in a child process whose device buffers lie between unmapped guard ranges and end where their
mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py): k_lbp_levels or k_hnew_levels reading past a level's planes or
a survivor list, or writing past the candidate list or its record array, faults at that access.  A fault here is a finding: read it from
the faulting address and the allocation log in the child's output, do not run it again to see it again."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_levels_kernels_stay_inside_their_buffers():
    _guarded_child("test_gpu_levels.py", "test_", 900, 20)
