"""The 4-bit instantiation of the two int8-MFMA code blocks (csrc/qgemm_codes_mfma.h, csrc/qgemm_codes_mfma3.h at (4, 4, 4)) on the MI355X, through the C ABI: the checks of
tests/codes_w4_cases.py, which tests/test_codes_w4_emulated.py runs on the CPU emulation build.  All comparisons are exact."""
import pytest

import abi_driver
import codes_w4_cases as W4

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("case", range(len(W4.BLOCKS1)), ids=[c[0] for c in W4.BLOCKS1])
def test_codeconv_mfma_w4_block(be, case):
    W4.check_block1(be, case)


@pytest.mark.parametrize("case", range(len(W4.BLOCKS3)), ids=[c[0] for c in W4.BLOCKS3])
def test_codeconv_mfma3_w4_block(be, case):
    W4.check_block3(be, case)


@pytest.mark.parametrize("form", ["mfma", "mfma3"])
@pytest.mark.parametrize("kcode", [15, 0])
def test_codeconv_w4_k_bound_fill(be, form, kcode):
    W4.check_fill(be, form, kcode)


@pytest.mark.parametrize("case", range(len(W4.REFUSED)))
def test_codeconv_w4_refused_is_enotsup(be, case):
    W4.check_refused(be, case)


def test_codeconv_w4_popcount_forms_refuse(be):
    W4.check_popcount_forms_refuse(be)


@pytest.mark.parametrize("form", ["mfma", "mfma3"])
def test_codeconv_w4_invalid_is_einval(be, form):
    W4.check_invalid(be, form)


@pytest.mark.parametrize("form", ["mfma", "mfma3"])
def test_codeconv_w4_table_counters(be, form):
    W4.check_counters(be, form)


@pytest.mark.parametrize("case", range(len(W4.LARGE1)), ids=[c[0] for c in W4.LARGE1])
def test_codeconv_mfma_w4_several_sets_per_block(be, case):
    """The launch shape of the measured batches: a block walks more than one set, the last block fewer (proved through mn_deploy_grid_deal)."""
    W4.check_large1(be, case)


@pytest.mark.parametrize("case", range(len(W4.LARGE3)), ids=[c[0] for c in W4.LARGE3])
def test_codeconv_mfma3_w4_several_spans_per_block(be, case):
    """The launch shape of the measured batches: some block takes a second span, some does not (proved through mn_deploy_grid_rows and the table's span)."""
    W4.check_large3(be, case)
