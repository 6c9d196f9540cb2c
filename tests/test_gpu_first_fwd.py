"""k_c1b_fwd<MT, EPI> on the MI355X: the first conv block's forward from bf16 term planes (tests/first_fwd_cases.py: the whole geometry sweep, every case with and
without bias)."""
import pytest

import abi_driver
import first_fwd_cases as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("case", range(len(U.CASES)))
def test_first_fwd_plain_within_bound(be, case, bias):
    U.check_plain(be, case, bias=bias, seed=700 + case)


def test_first_fwd_relu_and_minmax_partials(be):
    U.check_relu_mm(be, 6, seed=730)


def test_first_fwd_strip_independence_bitwise(be):
    U.check_strip_independence(be, seed=740)


@pytest.mark.parametrize("act,bits", [(1, 0), (2, 2), (2, 8)])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("case", range(len(U.CASES)))
def test_first_fwd_fused_codes_and_nibbles(be, case, bias, act, bits):
    U.check_fused(be, case, bias, act, bits, seed=750 + case)
