"""The two ends of the int8 deployment of the BN-folded IAO graph (csrc/qgemm_iao8_ends.h: k_i8first, k_i8first_wpack, k_i8conv_f32) compiled for the CPU SIMT
emulator, through the real C ABI; the same checks run on the MI355X in tests/test_gpu_iao8_ends.py.  All comparisons are exact (tests/iao8_ends_cases.py)."""
import pytest

import abi_driver
import iao8_ends_cases as EC


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


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


@pytest.mark.parametrize("widths", [(8, 8), (4, 4)], ids=["w8a8", "w4a4"])
@pytest.mark.parametrize("kind,case", [("first", i) for i in range(len(EC.FIRST))] + [("last", i) for i in range(len(EC.LAST))],
                         ids=[c[0] for c in EC.FIRST] + [c[0] for c in EC.LAST])
def test_judge_within_the_cap_of_the_fp32_path(kind, case, widths):
    EC.check_vs_torch(kind, case, widths)
