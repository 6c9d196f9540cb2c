"""Code-packed kernels of plain nin (csrc/qgemm_codes.h: k_codeconv_tile, k_codes_maxpool) on the MI355X, through the C ABI: the checks of tests/codes_nin_cases.py,
which tests/test_codes_nin_emulated.py runs on the CPU emulation build.  All comparisons are exact."""
import pytest

import abi_driver
import codes_nin_cases as NC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("case", range(len(NC.BLOCKS)), ids=[c[0] for c in NC.BLOCKS])
def test_codeconv_tile_block(be, case):
    NC.check_block(be, case)


@pytest.mark.parametrize("kcode", [3, 0])
@pytest.mark.parametrize("case", range(len(NC.FILLS)), ids=["4x8", "5x8"])
def test_codeconv_tile_k_bound_fill(be, case, kcode):
    NC.check_fill(be, case, kcode)


@pytest.mark.parametrize("case", range(len(NC.REFUSED)))
def test_codeconv_tile_refused_is_enotsup(be, case):
    NC.check_refused(be, case)


def test_codeconv_tile_and_pool_invalid_is_einval(be):
    NC.check_invalid(be)


def test_codeconv_tile_table_counters(be):
    NC.check_counters(be)


@pytest.mark.parametrize("case", range(len(NC.POOLS)))
def test_codes_maxpool(be, case):
    NC.check_pool(be, case)


def test_codes_maxpool_refused_is_enotsup(be):
    NC.check_pool_refused(be)


@pytest.mark.parametrize("case", range(len(NC.LARGE_GRID)), ids=[c[0] for c in NC.LARGE_GRID])
def test_codeconv_tile_several_word_groups_per_block(be, case):
    """The launch shape of the measured batches: a block walks more than one output word group, the last block fewer (proved through mn_deploy_grid_deal)."""
    NC.check_large(be, case)
