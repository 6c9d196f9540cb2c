"""The int8-MFMA form of the 1x1 hidden code block (csrc/qgemm_codes_mfma.h: k_codeconv_mfma) on the MI355X, through the C ABI: the checks of tests/codes_mfma_cases.py, which
tests/test_codes_mfma_emulated.py runs on the CPU emulation build.  All comparisons are exact."""
import pytest

import abi_driver
import codes_mfma_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("case", range(len(MC.BLOCKS)), ids=[c[0] for c in MC.BLOCKS])
def test_codeconv_mfma_block(be, case):
    MC.check_block(be, case)


@pytest.mark.parametrize("kcode", [3, 0])
def test_codeconv_mfma_k_bound_fill(be, kcode):
    MC.check_fill(be, kcode)


@pytest.mark.parametrize("case", range(len(MC.REFUSED)))
def test_codeconv_mfma_refused_is_enotsup(be, case):
    MC.check_refused(be, case)


def test_codeconv_mfma_invalid_is_einval(be):
    MC.check_invalid(be)


def test_codeconv_mfma_table_counters(be):
    MC.check_counters(be)


@pytest.mark.parametrize("case", range(len(MC.LARGE_GRID)), ids=[c[0] for c in MC.LARGE_GRID])
def test_codeconv_mfma_several_sets_per_block(be, case):
    """The launch shape of the measured batches: a block walks more than one set, the last block fewer (proved through mn_deploy_grid_deal)."""
    MC.check_large(be, case)
