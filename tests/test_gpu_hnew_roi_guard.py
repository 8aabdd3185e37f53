"""tests/test_gpu_hnew_roi.py once more in a child process whose device buffers lie between unmapped guard ranges and end where their
mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py): a k_roi_hnew that reads past the job's image, the launch's
table blob or the cascade's records, or writes past the candidate list, faults at that access.  A fault here is a finding: read it
from the faulting address and the allocation log in the child's output, do not run it again to see it again."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_small_hnew_route_stays_inside_its_buffers():
    _guarded_child("test_gpu_hnew_roi.py", "test_", 900, 20)
