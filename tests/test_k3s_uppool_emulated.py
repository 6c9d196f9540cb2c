"""k_k3s_dgrad<1, 1> on the CPU SIMT emulator: the grouped 3x3 block's backward-data leaving the BatchNorm-backward sums of the pooled pointwise block in front
(tests/k3s_uppool_cases.py).  The same checks run on the MI355X in test_gpu_k3s_uppool.py."""
import pytest

import abi_driver
import k3s_uppool_cases as U


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("case", range(len(U.CASES)))
def test_k3s_uppool_sums_and_dx(be, case):
    U.check(be, seed=500 + case, **U.CASES[case])


def test_k3s_uppool_blocks_walk_several_stages(be):
    U.check(be, seed=510, **U.CASE_LONG)
