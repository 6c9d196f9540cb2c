"""The byte form of the DoReFa W8A8 hidden block (csrc/qgemm_codes_w8.h) compiled for the CPU SIMT emulator, through the C ABI: the exact checks of tests/codes_w8_cases.py,
which tests/test_gpu_codes_w8.py runs on the MI355X."""
import pytest

import abi_driver
import codes_w8_cases as W


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("check, arg", [c[1:] for c in W.CHECKS], ids=[c[0] for c in W.CHECKS])
def test_code8(be, check, arg):
    check(be, arg)
