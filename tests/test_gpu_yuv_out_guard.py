"""tests/test_gpu_yuv_out.py once more in a child process whose device buffers lie between unmapped guard ranges and end where their
mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py): a kernel of the way out in 4:2:0 that reads past the staged
BGR frame, or writes past the planes, faults at that access.  The host-memory cases are where this bites: the device buffer their
planes are computed in ends with the last chroma row.  A fault here is a finding: read it from the faulting address and the allocation
log in the child's output, do not run it again to see it again."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_yuv_out_kernels_stay_inside_their_buffers():
    _guarded_child("test_gpu_yuv_out.py", "test_", 900, 20)
