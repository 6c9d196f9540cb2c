"""k_c1b_fwd<MT, EPI> on the CPU SIMT emulator: the first conv block's forward from bf16 term planes (tests/first_fwd_cases.py).  A light selection; the whole
sweep, the N = 600 case and the strip-independence comparison built on it (600 emulated images: over a minute here) run on the MI355X in test_gpu_first_fwd.py."""
import pytest

import abi_driver
import first_fwd_cases as U


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("case", U.SMALL)
def test_first_fwd_plain_within_bound(be, case):
    U.check_plain(be, case, bias=case % 2 == 0, seed=700 + case)


def test_first_fwd_plain_without_and_with_bias_two_blocks(be):
    U.check_plain(be, 5, bias=True, seed=720)
    U.check_plain(be, 1, bias=False, seed=721)


def test_first_fwd_relu_and_minmax_partials(be):
    U.check_relu_mm(be, 6, seed=730)


@pytest.mark.parametrize("case,bias,act,bits", [(0, True, 1, 0), (1, False, 2, 2), (5, True, 2, 8), (6, False, 1, 0)])
def test_first_fwd_fused_codes_and_nibbles(be, case, bias, act, bits):
    U.check_fused(be, case, bias, act, bits, seed=750 + case)
