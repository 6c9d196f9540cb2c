"""The 3x3 / stride-2 / padding-1 max-pool kernels (csrc/pool3s2.h) compiled for the CPU SIMT emulator, through the C ABI: the exact checks of
tests/pool3_cases.py, which tests/test_gpu_pool3.py runs on the MI355X."""
import pytest

import abi_driver
import pool3_cases as P


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("form, shape, kind, quant, off", P.CASES, ids=P.IDS)
def test_pool3(be, form, shape, kind, quant, off):
    P.check(be, form, shape, kind, quant, off)
