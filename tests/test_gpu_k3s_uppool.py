"""k_k3s_dgrad<1, 1> on the MI355X: the grouped 3x3 block's backward-data leaving the BatchNorm-backward sums of the pooled pointwise block in front
(tests/k3s_uppool_cases.py: the emulated run's cases + nin_gc's layers 4 and 7 at batch 8)."""
import pytest

import abi_driver
import k3s_uppool_cases as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


NIN_GC = [
    dict(x_shape=(8, 256, 16, 16), w_shape=(512, 16, 3, 3), groups=16, in_shuffle=2),        # layer 4
    dict(x_shape=(8, 512, 8, 8), w_shape=(1024, 16, 3, 3), groups=32, in_shuffle=16),        # layer 7
]


@pytest.mark.parametrize("case", range(len(U.CASES)))
def test_k3s_uppool_sums_and_dx(be, case):
    U.check(be, seed=500 + case, **U.CASES[case])


def test_k3s_uppool_blocks_walk_several_stages(be):
    U.check(be, seed=510, **U.CASE_LONG)


@pytest.mark.parametrize("case", range(len(NIN_GC)))
def test_k3s_uppool_nin_gc_layers(be, case):
    U.check(be, seed=520 + case, **NIN_GC[case])
