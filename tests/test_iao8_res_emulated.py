"""The residual stages of the int8 ResNet deployment (csrc/qgemm_iao8_res.h: k_i8res_conv, k_i8res_add over k_i8conv_wpack's table) compiled for the CPU SIMT
emulator, through the real C ABI; the same checks run on the MI355X in tests/test_gpu_iao8_res.py.  All comparisons are exact (tests/iao8_res_cases.py)."""
import pytest

import abi_driver
import iao8_res_cases as RC


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("case", range(len(RC.CONVS)), ids=[c[0] for c in RC.CONVS])
def test_i8res_conv(be, case):
    RC.check_conv(be, case)


def test_i8res_conv_extreme_accumulator(be):
    RC.check_conv_extreme(be)


@pytest.mark.parametrize("nout", [1, 2])
@pytest.mark.parametrize("case", range(len(RC.ADDS)), ids=[c[0] for c in RC.ADDS])
def test_i8res_add(be, case, nout):
    RC.check_add(be, case, nout)


@pytest.mark.parametrize("case", range(len(RC.REFUSED)))
def test_i8res_refused_is_enotsup(be, case):
    RC.check_refused(be, case)


def test_i8res_widths_outside_2_to_8_are_refused(be):
    RC.check_widths_refused(be)


def test_i8res_add_refuses_stride_2(be):
    RC.check_add_stride2_refused(be)


def test_i8res_invalid_is_einval(be):
    RC.check_invalid(be)


def test_i8res_table_counters(be):
    RC.check_counters(be)
