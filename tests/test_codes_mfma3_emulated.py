"""The int8-MFMA form of the 3x3 hidden code block (csrc/qgemm_codes_mfma3.h: k_codeconv_mfma3) compiled for the CPU SIMT emulator, through the real C ABI; the same
checks run on the MI355X in tests/test_gpu_codes_mfma3.py.  All comparisons are exact (tests/codes_mfma3_cases.py)."""
import pytest

import abi_driver
import codes_mfma3_cases as MC


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("case", range(len(MC.BLOCKS)), ids=[c[0] for c in MC.BLOCKS])
def test_codeconv_mfma3_block(be, case):
    MC.check_block(be, case)


@pytest.mark.parametrize("kcode", [3, 0])
def test_codeconv_mfma3_k_bound_fill(be, kcode):
    MC.check_fill(be, kcode)


@pytest.mark.parametrize("case", range(len(MC.REFUSED)))
def test_codeconv_mfma3_refused_is_enotsup(be, case):
    MC.check_refused(be, case)


def test_codeconv_mfma3_invalid_is_einval(be):
    MC.check_invalid(be)


def test_codeconv_mfma3_table_counters(be):
    MC.check_counters(be)
