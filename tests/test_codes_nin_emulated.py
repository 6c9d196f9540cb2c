"""Code-packed kernels of plain nin (csrc/qgemm_codes.h: k_codeconv_tile, k_codes_maxpool) compiled for the CPU SIMT emulator, through the real C ABI; the same checks
run on the MI355X in tests/test_gpu_codes_nin.py.  All comparisons are exact (tests/codes_nin_cases.py)."""
import pytest

import abi_driver
import codes_nin_cases as NC


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


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
