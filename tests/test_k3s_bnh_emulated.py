"""k_k3s_dgrad<1> / k_k3s_wgrad<0, 1> on the CPU SIMT emulator: the grouped 3x3 binary block's backward-data / backward-weight forming dy from (da, h),
bit for bit against mn_bnh_bwd_apply + the plain kernels and against fp64 (tests/k3s_bnh_cases.py).  The same checks run on the MI355X in test_gpu_k3s_bnh.py."""
import pytest

import abi_driver
import k3s_bnh_cases as B


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("case", range(len(B.CASES)))
def test_k3s_bnh_matches_two_step_path(be, case):
    B.check(be, seed=300 + case, **B.CASES[case])


def test_k3s_bnh_blocks_walk_several_stages(be):
    B.check(be, seed=310, **B.CASE_LONG)
