"""tests/test_gpu_haar_tree.py once more in a child process whose device buffers lie between unmapped guard ranges and end where their
mappings end (NVCA_ALLOC_GUARD=2, the helper of tests/test_gpu_guard.py): a kernel of the general new-format HAAR evaluator that reads
past a level's sum, tilted or squared-integral planes, the node table, the stage-0 pass bits or a survivor list, or writes past the
candidate list, faults at that access.  A fault here is a finding: read it from the faulting address and the allocation log in the
child's output, do not run it again to see it again."""
import pytest

from test_gpu_guard import _guarded_child


@pytest.mark.gpu
def test_haar_tree_kernels_stay_inside_their_buffers():
    _guarded_child("test_gpu_haar_tree.py", "test_", 900, 20)
