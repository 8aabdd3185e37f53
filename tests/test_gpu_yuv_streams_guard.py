"""tests/test_gpu_yuv_parts.py and tests/test_gpu_yuv_tracker.py once more, each in a child process whose device buffers lie between
unmapped guard ranges and end where their mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py), as
tests/test_gpu_yuv_guard.py does for the face path: a staged 4:2:0 frame ends with its last chroma row, so a tracker pixel pass or a
working-image kernel that reads one chroma row too far, or past the end of a row's last unit, faults at that access.  A fault here is
a finding: read it from the faulting address and the allocation log in the child's output, do not run it again to see it again."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_part_image_kernels_stay_inside_their_buffers():
    _guarded_child("test_gpu_yuv_parts.py", "test_", 900, 20)


@pytest.mark.gpu
def test_tracker_pixel_kernels_stay_inside_their_buffers():
    _guarded_child("test_gpu_yuv_tracker.py", "test_", 900, 20)
