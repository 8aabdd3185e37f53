"""Cases of tests/test_gpu_many_levels.py once more in a child process whose device buffers lie between unmapped guard ranges and end
where their mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py): with 160 levels instead of at most 63, a pyramid
launch, a stage-0 tile, the row walk or k_group that reads past the level tables, the planes or the pass bits, or writes past a list,
faults at that access.  A fault here is a finding: read it from the faulting address and the allocation log in the child's output, do
not run it again to see it again."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_scans_of_many_levels_stay_inside_their_buffers():
    _guarded_child("test_gpu_many_levels.py", "(test_single_image and 1.01) or test_old_format or test_two_images or test_reject_levels or test_face_stream_frame", 600, 20)
