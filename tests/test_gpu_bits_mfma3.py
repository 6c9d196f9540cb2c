"""The int8-MFMA form of the 3x3 hidden bit block (csrc/qgemm_bits_mfma3.h: k_bitconv_mfma3) on the MI355X, through the C ABI; the same
checks run on the CPU emulation build in tests/test_bits_mfma3_emulated.py.  All comparisons are exact (tests/bits_mfma3_cases.py)."""
import pytest

import abi_driver
import bits_mfma3_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("case", range(len(MC.BLOCKS)), ids=[c[0] for c in MC.BLOCKS])
def test_bitconv_mfma3_block(be, case):
    MC.check_block(be, case)


@pytest.mark.parametrize("sign", [1, -1])
def test_bitconv_mfma3_border_fill(be, sign):
    MC.check_fill(be, sign)


@pytest.mark.parametrize("case", range(len(MC.REFUSED)))
def test_bitconv_mfma3_refused_is_enotsup(be, case):
    MC.check_refused(be, case)


def test_bitconv_mfma3_invalid_is_einval(be):
    MC.check_invalid(be)


def test_bitconv_mfma3_table_counters(be):
    MC.check_counters(be)


@pytest.mark.parametrize("case", range(len(MC.LARGE_GRID)), ids=[c[0] for c in MC.LARGE_GRID])
def test_bitconv_mfma3_several_spans_per_block(be, case):
    """The launch shape of the measured batches: some block takes a second span, some does not (proved through mn_deploy_grid_rows and the table's span)."""
    MC.check_large(be, case)
