"""The int8 deployment kernels with zero points (csrc/qgemm_iao8_zp.h: k_i8zconv, k_i8zconv_wpack, k_i8z_pack, k_i8z_unpack) compiled for the CPU SIMT emulator,
through the real C ABI; the same checks run on the MI355X in tests/test_gpu_iao8_zp.py.  All comparisons are exact (tests/iao8_zp_cases.py)."""
import pytest

import abi_driver
import iao8_zp_cases as ZC


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


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


@pytest.mark.parametrize("case", range(len(ZC.BLOCKS)), ids=[c[0] for c in ZC.BLOCKS])
def test_judge_within_the_cap_of_the_fp32_path(case):
    ZC.check_vs_torch(case)
