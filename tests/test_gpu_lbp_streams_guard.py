"""tests/test_gpu_lbp_streams.py once more in a child process whose device buffers lie between unmapped guard ranges and end where their
mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py): the pyramid now reads the LAST slot's gray image and LUT of a
lane, k_group the last level's rows of the position table and the last slot's threshold and box table, and the second ticket's lane has
buffers of its own -- a read or a store one slot, one level or one table row too far faults at that access.  A fault here is a finding:
read it from the faulting address and the allocation log in the child's output, do not run it again to see it again.  The time limit: the
unguarded file takes 18 s where tests/test_gpu_lbp.py takes 19 s, and gets that file's 900 s in the same proportion, as
tests/test_gpu_lbp_batch_guard.py states it."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_lbp_stream_kernels_stay_inside_their_buffers():
    _guarded_child("test_gpu_lbp_streams.py", "test_", 850, 20)
