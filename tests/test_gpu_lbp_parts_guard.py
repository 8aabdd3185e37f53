"""tests/test_gpu_lbp_parts.py once more in a child process whose device buffers lie between unmapped guard ranges and end where their
mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py): part searches are sub-matrices of the part image, so a
k_roi_lbp that reads past a region's last row or past the launch's tables faults at that access.  A fault here is a finding: read it
from the faulting address and the allocation log in the child's output, do not run it again to see it again."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_lbp_part_streams_stay_inside_their_buffers():
    _guarded_child("test_gpu_lbp_parts.py", "all_roles_lbp or eight_streams or two_tickets or nv12", 900, 20)
