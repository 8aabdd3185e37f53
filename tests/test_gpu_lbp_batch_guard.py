"""tests/test_gpu_lbp_batch.py once more in a child process whose device buffers lie between unmapped guard ranges and end where their
mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py): with an image axis the LAST image's sum planes, pass bits and
list entries end where their mappings end, so a kernel that steps one image too far, or a survivor or candidate list sized for fewer
images than it serves, faults at that access.  A fault here is a finding: read it from the faulting address and the allocation log in
the child's output, do not run it again to see it again.  The time limit: the unguarded file takes 13 s where tests/test_gpu_lbp.py takes
19 s, and gets that file's 900 s in the same proportion."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_batched_lbp_kernels_stay_inside_their_buffers():
    _guarded_child("test_gpu_lbp_batch.py", "test_", 640, 20)
