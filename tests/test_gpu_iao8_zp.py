"""The int8 deployment kernels with zero points (csrc/qgemm_iao8_zp.h: k_i8zconv, k_i8zconv_wpack, k_i8z_pack, k_i8z_unpack) on the MI355X, through the C ABI: the
checks of tests/iao8_zp_cases.py, which tests/test_iao8_zp_emulated.py runs on the CPU emulation build.  All comparisons are exact."""
import pytest

import abi_driver
import iao8_zp_cases as ZC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("case", range(len(ZC.BLOCKS)), ids=[c[0] for c in ZC.BLOCKS])
def test_i8zconv_block(be, case):
    ZC.check_block(be, case)


def test_i8zconv_extreme_sum(be):
    ZC.check_extreme(be)


@pytest.mark.parametrize("case", range(len(ZC.MIXES)), ids=[c[0] for c in ZC.MIXES])
def test_i8zconv_mix(be, case):
    ZC.check_mix(be, case)


def test_i8zconv_symmetric_is_the_present_chain(be):
    ZC.check_symmetric_is_the_present_chain(be)


@pytest.mark.parametrize("channels,a_bits,z,shuffle", [(40, 8, 0, 0), (64, 8, -130, 4), (33, 4, -3, 0), (16, 8, 65535, 2), (20, 8, -65535, 0)])
def test_i8z_pack_unpack_codes(be, channels, a_bits, z, shuffle):
    ZC.check_pack_unpack(be, channels, a_bits, z, shuffle)


@pytest.mark.parametrize("z,asym", [(0, 1), (-130, 1), (65535, 1), (-65535, 1), (65535, 0)])
def test_i8z_round_trip_of_every_code(be, z, asym):
    ZC.check_round_trip_all_codes(be, z, asym)


@pytest.mark.parametrize("case", range(len(ZC.REFUSED)))
def test_i8zconv_refused_is_enotsup(be, case):
    ZC.check_refused(be, case)


def test_i8zconv_invalid_is_einval(be):
    ZC.check_invalid(be)


def test_i8zconv_table_counters(be):
    ZC.check_counters(be)


@pytest.mark.parametrize("case", range(len(ZC.LARGE_GRID)), ids=[c[0] for c in ZC.LARGE_GRID])
def test_i8zconv_several_sets_per_block(be, case):
    """The launch shape of the measured batches: a block walks more than one set, the last block fewer (proved through mn_deploy_grid_deal)."""
    ZC.check_large(be, case)
