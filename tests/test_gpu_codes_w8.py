"""The byte form of the DoReFa W8A8 hidden block (csrc/qgemm_codes_w8.h) on the MI355X, through the C ABI: the exact checks of tests/codes_w8_cases.py,
which tests/test_codes_w8_emulated.py runs on the CPU emulation build."""
import pytest

import abi_driver
import codes_w8_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("check, arg", [c[1:] for c in W.CHECKS], ids=[c[0] for c in W.CHECKS])
def test_code8(be, check, arg):
    check(be, arg)
