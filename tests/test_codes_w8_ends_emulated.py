"""The two ends of the W8A8 byte plan (mn_conv2d_first_bytes, mn_code8conv_fwd_f32) compiled for the CPU SIMT emulator, through the C ABI: the checks of
tests/codes_w8_ends_cases.py, which tests/test_gpu_codes_w8_ends.py runs on the MI355X."""
import pytest

import abi_driver
import codes_w8_ends_cases as E

be = pytest.fixture(scope="module")(lambda: abi_driver.Backend("emu"))


@pytest.mark.parametrize("check, arg", [c[1:] for c in E.CHECKS], ids=[c[0] for c in E.CHECKS])
def test_code8_ends(be, check, arg):
    check(be, arg)
