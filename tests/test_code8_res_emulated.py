"""The residual stages of the DoReFa W8A8 byte plan (csrc/qgemm_codes_w8_res.h) compiled for the CPU SIMT emulator, through the C ABI: the exact checks of
tests/code8_res_cases.py, which tests/test_gpu_code8_res.py runs on the MI355X."""
import pytest

import abi_driver
import code8_res_cases as R


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("check, arg", [c[1:] for c in R.CHECKS], ids=[c[0] for c in R.CHECKS])
def test_code8_res(be, check, arg):
    check(be, arg)
