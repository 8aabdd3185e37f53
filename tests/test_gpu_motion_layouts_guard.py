"""tests/test_gpu_motion_layouts.py once more, in a child process whose device buffers lie between unmapped guard ranges and end where
their mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py), as tests/test_gpu_yuv_streams_guard.py does for the
4:2:0 streams: the layouts hold the partial tiles at the frame's right and bottom edges (520 x 50: a tile column of 8 pixels and a tile
row of 2 rows; 513 x 49: one of each; 5 x 3), so a component kernel that reads a history, a label or a flag byte past its buffer faults
at that access.  A fault here is a finding: read it from the faulting address and the allocation log in the child's output, do not run
it again to see it again."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_component_kernels_stay_inside_their_buffers():
    _guarded_child("test_gpu_motion_layouts.py", "test_", 900, 20)
