"""The residual stages of the DoReFa W2A2 code plan (csrc/qgemm_codes_res.h) compiled for the CPU SIMT emulator, through the C ABI: the exact checks of
tests/coderes_cases.py, which tests/test_gpu_coderes.py runs on the MI355X."""
import pytest

import abi_driver
import coderes_cases as R


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("check, arg", [c[1:] for c in R.CHECKS], ids=[c[0] for c in R.CHECKS])
def test_coderes(be, check, arg):
    check(be, arg)
