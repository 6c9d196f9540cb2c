"""Code-packed deployment kernels of the DoReFa W2A2 blocks (csrc/qgemm_codes.h) compiled for the CPU SIMT emulator, through the real C ABI; the same checks run on the
MI355X in tests/test_gpu_codes.py.  All comparisons are exact; the judge is an int64 numpy convolution plus the library's own mn_qa_fwd, and the numpy fp32 chain."""
import pytest

import abi_driver
import codes_cases as CC

CASES = CC.block_cases(full=False)


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


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
    """The "several word groups per block" cases (9 and 17 s here; the emulator runs its blocks in order, so it shows a wrong loop, not a race between two groups --
    that is what the GPU run of the same table is for)."""
    CC.check_large(be, case)
