"""The two ends of the int8 deployment of BN-folded IAO ResNets (csrc/qgemm_iao8_e2e.h: k_i8first2, k_i8poolfc, k_i8poolfc_wpack) compiled for the CPU SIMT emulator,
through the real C ABI; the same checks run on the MI355X in tests/test_gpu_iao8_e2e.py.  All comparisons are exact (tests/iao8_e2e_cases.py)."""
import pytest

import abi_driver
import iao8_e2e_cases as XC


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("case", range(len(XC.FIRST2)), ids=[c[0] for c in XC.FIRST2])
def test_i8first2_block(be, case):
    XC.check_first2(be, case)


@pytest.mark.parametrize("case", range(len(XC.FIRST2_CHAINS)), ids=[c[0] for c in XC.FIRST2_CHAINS])
def test_i8first2_chain(be, case):
    XC.check_first2_chain(be, case)


def test_i8first2_extreme_accumulator(be):
    XC.check_first2_extreme(be)


def test_i8first2_invalid_is_einval_and_uncovered_is_enotsup(be):
    XC.check_first2_invalid(be)


@pytest.mark.parametrize("case", range(len(XC.POOLFC)), ids=[c[0] for c in XC.POOLFC])
def test_i8poolfc(be, case):
    XC.check_poolfc(be, case)


@pytest.mark.parametrize("case", range(len(XC.POOLFC_CHAINS)), ids=[c[0] for c in XC.POOLFC_CHAINS])
def test_i8poolfc_chain(be, case):
    XC.check_poolfc_chain(be, case)


def test_i8poolfc_extreme_accumulator(be):
    XC.check_poolfc_extreme(be)


def test_i8poolfc_exact_ties_round_away_from_zero(be):
    XC.check_poolfc_ties(be)


def test_i8poolfc_codes_through_identity_rows(be):
    XC.check_poolfc_identity_rows(be)


def test_i8poolfc_table_counters(be):
    XC.check_poolfc_counters(be)


@pytest.mark.parametrize("case", range(len(XC.POOLFC_REFUSED)))
def test_i8poolfc_refused_is_enotsup(be, case):
    XC.check_poolfc_refused(be, case)


def test_i8poolfc_invalid_is_einval(be):
    XC.check_poolfc_invalid(be)
