"""The two ends of the code-packed plan (mn_conv2d_first_codes, mn_planesconv1x1_small_fwd) compiled for the CPU SIMT emulator, through the real C ABI; the same checks
run on the MI355X in tests/test_gpu_codes_ends.py.  All comparisons against the existing entry points are exact."""
import pytest

import abi_driver
import codes_ends_cases as E


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("case", range(len(E.FIRST_CASES)))
def test_first_conv_codes(be, case):
    E.check_first_codes(be, *E.FIRST_CASES[case], seed=1500 + case)


def test_first_conv_codes_beyond_the_threshold_range_and_nan(be):
    E.check_first_codes_guard(be, seed=1510)


def test_first_conv_codes_tail_is_zero(be):
    E.check_first_codes_tail_is_zero(be, seed=1511)


def test_first_conv_codes_nonfinite_constants_are_counted(be):
    E.check_first_nonfinite_counted(be, seed=1512)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", range(len(E.CLASSIFIER_SHAPES)))
def test_planes_classifier(be, shape, bias):
    E.check_planes_classifier(be, *E.CLASSIFIER_SHAPES[shape], bias=bias, seed=1520 + shape)


@pytest.mark.parametrize("bias", [True, False])
def test_planes_classifier_partial_word_and_pixel_tail(be, bias):
    E.check_planes_classifier(be, *E.CLASSIFIER_ODD, bias=bias, N=3, Oc=3, seed=1530)


def test_rejects_bad_arguments(be):
    E.check_rejects_bad_arguments(be)
