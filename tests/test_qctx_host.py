"""CPU tests of the batch contexts' launch shape without a device (pt_selftest_fold_shape: qctx.cpp
fold_shape): the workgroup and the resident grid of a context with fold records (PathQuery,
PixelQuery) on a device of 256 compute units that hold 8 workgroups of 256 threads each.

Every expected figure is derived by hand from the rule: a resident lane's fold records take
16 B x RAY_DEPTH, a resident grid's at most 2^30 B.  A full grid is 256 x 8 = 2,048 workgroups of 256
lanes, 2^19 lanes: its records fit up to depth 2^30 / (2^19 x 16) = 128.  Beyond that the grid is
2^30 / (256 lanes x 16 B x depth) workgroups, rounded down, but never fewer than one per compute
unit; where 256 workgroups of 256 lanes are still too many, the workgroup halves down to one wave.
"""
import pytest

import _util as U

pt = U.ptrace()
CUS, PER_CU, BLOCK = 256, 8, 256


@pytest.mark.parametrize("depth,block,grid", [
    (6, 256, 2048),      # the bench job's depth: 2^19 lanes x 96 B = 48 MiB
    (128, 256, 2048),    # 2^19 lanes x 2,048 B = 2^30 exactly: not over
    (129, 256, 2032),    # 2^30 / (256 x 2,064) = 2,032.1
    (4096, 64, 256),     # 2^30 / (256 x 65,536) = 64 workgroups < 256 CUs: 256 of them, of 2^30 / (256 x 65,536) = 64 lanes
    (0, 256, 2048),      # as depth 1: a lane's area is never empty
    (1, 256, 2048),
])
def test_fold_shape(depth, block, grid):
    assert pt.selftest_fold_shape(CUS, PER_CU, BLOCK, depth) == (block, grid)


def test_fold_shape_refuses_a_depth_beyond_one_wave_per_cu():
    """depth 4,097: 256 workgroups x 64 lanes x 65,552 B > 2^30"""
    with pytest.raises(pt.PTError) as e:
        pt.selftest_fold_shape(CUS, PER_CU, BLOCK, 4097)
    assert e.value.code == pt.PT_E_OOM and "RAY_DEPTH too large" in pt.last_error()
