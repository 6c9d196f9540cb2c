"""The dense 5x5 block on activation codes (csrc/qgemm_q5.h) compiled for the CPU SIMT emulator: the case table of tests/q5_cases.py."""
import pytest

import abi_driver
import q5_cases as Q


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("x_shape, Oc, kw", Q.CASES, ids=Q.IDS)
def test_q5(be, x_shape, Oc, kw):
    Q.check(be, x_shape, Oc, kw)


def test_q5_extremes(be):
    Q.check_extremes(be)


def test_q5_refused(be):
    Q.check_refused(be)
