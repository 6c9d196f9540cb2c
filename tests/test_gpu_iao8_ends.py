"""The two ends of the int8 deployment of the BN-folded IAO graph (csrc/qgemm_iao8_ends.h: k_i8first, k_i8first_wpack, k_i8conv_f32) on the MI355X, through the C
ABI: the checks of tests/iao8_ends_cases.py, which tests/test_iao8_ends_emulated.py runs on the CPU emulation build.  All comparisons are exact."""
import pytest

import abi_driver
import iao8_ends_cases as EC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("case", range(len(EC.FIRST)), ids=[c[0] for c in EC.FIRST])
def test_i8first_block(be, case):
    EC.check_first(be, case)


@pytest.mark.parametrize("case", range(len(EC.FIRST_CHAINS)), ids=[c[0] for c in EC.FIRST_CHAINS])
def test_i8first_chain(be, case):
    EC.check_first_chain(be, case)


def test_i8first_extreme_accumulator(be):
    EC.check_first_extreme(be)


@pytest.mark.parametrize("case", range(len(EC.LAST)), ids=[c[0] for c in EC.LAST])
def test_i8conv_f32_block(be, case):
    EC.check_last(be, case)


@pytest.mark.parametrize("case", range(len(EC.LAST_CHAINS)), ids=[c[0] for c in EC.LAST_CHAINS])
def test_i8conv_f32_chain(be, case):
    EC.check_last_chain(be, case)


@pytest.mark.parametrize("case", range(len(EC.FIRST_REFUSED)))
def test_i8first_refused_is_enotsup(be, case):
    EC.check_first_refused(be, case)


def test_ends_invalid_is_einval(be):
    EC.check_invalid(be)


def test_i8first_table_counters(be):
    EC.check_first_counters(be)


@pytest.mark.parametrize("case", range(len(EC.LARGE_FIRST)), ids=[c[0] for c in EC.LARGE_FIRST])
def test_i8first_several_sets_per_block(be, case):
    """The launch shape of the measured batches: a block walks more than one set, the last block fewer (proved through mn_deploy_grid_deal)."""
    EC.check_large_first(be, case)


@pytest.mark.parametrize("case", range(len(EC.LARGE_LAST)), ids=[c[0] for c in EC.LARGE_LAST])
def test_i8conv_f32_several_sets_per_block(be, case):
    """The launch shape of the measured batches: a block walks more than one set, the last block fewer (proved through mn_deploy_grid_deal)."""
    EC.check_large_last(be, case)
