"""tests/test_gpu_yuv422.py once more in a child process whose device buffers lie between unmapped guard ranges and end where their
mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py), as tests/test_gpu_yuv_guard.py does for 4:2:0: a staged
packed 4:2:2 frame ends with its last row's last pixel, so a gray kernel, a working-image kernel or a tracker pixel pass that reads past the
end of a row's last unit, or a row too far, faults at that access.  A fault here is a finding: read it from the faulting address and the
allocation log in the child's output, do not run it again to see it again."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_yuv422_kernels_stay_inside_their_buffers():
    _guarded_child("test_gpu_yuv422.py", "test_", 900, 20)
