"""The int8-MFMA form of the 1x1 hidden bit block (csrc/qgemm_bits_mfma.h: k_bitconv_mfma) on the MI355X, through the C ABI; the same
checks run on the CPU emulation build in tests/test_bits_mfma_emulated.py.  All comparisons are exact (tests/bits_mfma_cases.py)."""
import pytest

import abi_driver
import bits_mfma_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("case", range(len(MC.BLOCKS)), ids=[c[0] for c in MC.BLOCKS])
def test_bitconv_mfma_block(be, case):
    MC.check_block(be, case)


@pytest.mark.parametrize("case", range(len(MC.REFUSED)))
def test_bitconv_mfma_refused_is_enotsup(be, case):
    MC.check_refused(be, case)


def test_bitconv_mfma_invalid_is_einval(be):
    MC.check_invalid(be)


def test_bitconv_mfma_table_counters(be):
    MC.check_counters(be)


@pytest.mark.parametrize("case", range(len(MC.LARGE_GRID)), ids=[c[0] for c in MC.LARGE_GRID])
def test_bitconv_mfma_several_sets_per_block(be, case):
    """The launch shape of the measured batches: a block walks more than one set, the last block fewer (proved through mn_deploy_grid_deal)."""
    MC.check_large(be, case)
