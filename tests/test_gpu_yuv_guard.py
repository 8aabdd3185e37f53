"""tests/test_gpu_yuv.py once more in a child process whose device buffers lie between unmapped guard ranges and end where their
mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py): a 4:2:0 kernel that reads past a staged frame's last plane,
or writes past the gray planes, faults at that access.  Staged host frames are where this bites: their staging buffer ends with the
last chroma row.  A fault here is a finding: read it from the faulting address and the allocation log in the child's output, do
not run it again to see it again."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_yuv_kernels_stay_inside_their_buffers():
    _guarded_child("test_gpu_yuv.py", "test_", 900, 20)
