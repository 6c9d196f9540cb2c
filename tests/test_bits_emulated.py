"""Bit-packed inference kernels (csrc/qgemm_bits.hip) compiled for the CPU SIMT emulator, through the real C ABI; the same checks run on the MI355X in
tests/test_gpu_bits.py.  All comparisons are exact."""
import pytest

import abi_driver
import bits_cases as B
import kernel_cases as K


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("Cc", [32, 80, 130, 256])
def test_pack_unpack_roundtrip(be, Cc):
    B.check_pack_roundtrip(be, Cc, seed=Cc)


@pytest.mark.parametrize("W", [3, 2])
@pytest.mark.parametrize("case", range(len(K.DEPLOYED_CASES)))
def test_bitconv_deployed_cases(be, case, W):
    B.check_bitconv(be, seed=700 + case, W=W, **K.DEPLOYED_CASES[case])


@pytest.mark.parametrize("W", [3, 2])
@pytest.mark.parametrize("layer", range(len(B.NIN_GC_LAYERS)))
def test_bitconv_nin_gc_geometries(be, layer, W):
    B.check_bitconv(be, seed=800 + layer, W=W, **B.nin_gc_case(layer, full=False))


@pytest.mark.parametrize("W", [3, 2])
def test_bitconv_two_channels_per_group(be, W):
    B.check_bitconv(be, seed=900, W=W, **B.TWO_PER_GROUP)


@pytest.mark.parametrize("case", [1, 3])
def test_consumer_order_and_pool(be, case):
    B.check_order_and_pool(be, seed=950 + case, **K.DEPLOYED_CASES[case])
