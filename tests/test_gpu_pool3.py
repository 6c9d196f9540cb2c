"""The 3x3 / stride-2 / padding-1 max-pool kernels (csrc/pool3s2.h) on the MI355X, through the C ABI: the exact checks of tests/pool3_cases.py, which
tests/test_pool3_emulated.py runs on the CPU emulation build."""
import pytest

import abi_driver
import pool3_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("form, shape, kind, quant, off", P.CASES, ids=P.IDS)
def test_pool3(be, form, shape, kind, quant, off):
    P.check(be, form, shape, kind, quant, off)
