"""The int8 deployment kernels of the BN-folded IAO hidden blocks (csrc/qgemm_iao8.h: k_i8conv, k_i8conv_wpack, k_i8_pack, k_i8_unpack) on the MI355X, through the C
ABI: the checks of tests/iao8_cases.py, which tests/test_iao8_emulated.py runs on the CPU emulation build.  All comparisons are exact."""
import pytest

import abi_driver
import iao8_cases as IC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("case", range(len(IC.BLOCKS)), ids=[c[0] for c in IC.BLOCKS])
def test_i8conv_block(be, case):
    IC.check_block(be, case)


def test_i8conv_extreme_accumulator(be):
    IC.check_extreme(be)


@pytest.mark.parametrize("case", range(len(IC.CHAINS)), ids=[c[0] for c in IC.CHAINS])
def test_i8conv_chain(be, case):
    IC.check_chain(be, case)


@pytest.mark.parametrize("channels,a_bits,shuffle", [(40, 8, 0), (64, 8, 4), (33, 4, 0), (16, 8, 2)])
def test_i8_pack_unpack_codes(be, channels, a_bits, shuffle):
    IC.check_pack_unpack(be, channels, a_bits, shuffle)


@pytest.mark.parametrize("case", range(len(IC.REFUSED)))
def test_i8conv_refused_is_enotsup(be, case):
    IC.check_refused(be, case)


def test_i8conv_invalid_is_einval(be):
    IC.check_invalid(be)


def test_i8conv_table_counters(be):
    IC.check_counters(be)


@pytest.mark.parametrize("case", range(len(IC.LARGE_GRID)), ids=[c[0] for c in IC.LARGE_GRID])
def test_i8conv_several_sets_per_block(be, case):
    """The launch shape of the measured batches: a block walks more than one set, the last block fewer (proved through mn_deploy_grid_deal)."""
    IC.check_large(be, case)
