"""The two ends of the bit-packed plan (mn_conv2d_first_sign_bits, mn_bitsconv1x1_small_fwd) compiled for the CPU SIMT emulator, through the real C ABI; the same checks
run on the MI355X in tests/test_gpu_bits_ends.py.  All comparisons against the existing entry points are exact."""
import pytest

import abi_driver
import bits_ends_cases as E


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("case", range(len(E.FIRST_CASES)))
def test_first_conv_sign_bits(be, case):
    E.check_first_bits(be, *E.FIRST_CASES[case], seed=1100 + case)


def test_first_conv_sign_bits_zero_and_nan_rule(be):
    E.check_first_bits_zero_rule(be, seed=1110)


def test_first_conv_sign_bits_tail_is_zero(be):
    E.check_first_bits_tail_is_zero(be, seed=1111)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", range(len(E.CLASSIFIER_SHAPES)))
def test_bits_classifier(be, shape, bias):
    E.check_bits_classifier(be, *E.CLASSIFIER_SHAPES[shape], bias=bias, seed=1120 + shape)


def test_rejects_bad_arguments(be):
    E.check_rejects_bad_arguments(be)
