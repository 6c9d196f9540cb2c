"""Code-packed deployment kernels of the DoReFa W2A2 blocks (csrc/qgemm_codes.h) on the MI355X: the checks of tests/codes_cases.py, the nin_gc layers with N = 2 at the
net's own map size.  All comparisons are exact; the judge is an int64 numpy convolution plus the library's own mn_qa_fwd, and the numpy fp32 chain."""
import pytest

import abi_driver
import codes_cases as CC

pytestmark = pytest.mark.gpu

CASES = CC.block_cases(full=True)


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("Cc", [32, 80, 130, 256])
def test_codes_pack_unpack_roundtrip(be, Cc):
    CC.check_pack_roundtrip(be, Cc, seed=Cc)


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_codeconv_block(be, name, kw):
    CC.check_codeconv(be, **kw)


def test_codeconv_nonfinite_constants_counted(be):
    CC.check_nonfinite_counted(be)


@pytest.mark.parametrize("case", range(len(CC.UNSUPPORTED)))
def test_codeconv_unsupported_is_enotsup(be, case):
    CC.check_unsupported(be, case)


@pytest.mark.parametrize("case", range(len(CC.LARGE_GRID)), ids=[c[0] for c in CC.LARGE_GRID])
def test_codeconv_several_word_groups_per_block(be, case):
    """The launch shape of the measured batches: a block walks more than one output word group, the last block fewer (proved through mn_deploy_grid_deal)."""
    CC.check_large(be, case)
