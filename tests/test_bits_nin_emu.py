"""The bit kernels of the plain nin net (LDS-tiled 5x5, 3x3 / stride 2 max-pool folded and standalone) compiled for the CPU SIMT emulator, through the real C ABI;
the same table runs on the MI355X in tests/test_gpu_bits_nin.py.  All comparisons are exact."""
import pytest

import abi_driver
import bits_nin_cases as BN

SEEN = set()


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("W", [3, 2])
@pytest.mark.parametrize("case", range(len(BN.SMALL)))
def test_small_cases(be, case, W):
    SEEN.add(BN.check_case(be, seed=1100 + case, W=W, **BN.SMALL[case]))


@pytest.mark.parametrize("layer", [2, 5])
def test_nin_dense_blocks_one_image(be, layer):
    """nin's 5x5 (96 -> 192 on 16 x 16) and 3x3 (192 -> 192 on 8 x 8) blocks at full width, one image (the emulator runs one fiber per GPU thread)."""
    SEEN.add(BN.check_case(be, seed=1200 + layer, W=3, **BN.nin_case(layer, n=1)))


def test_tiled_block_honours_the_consumer_order(be):
    BN.check_consumer_order(be, seed=1300)


@pytest.mark.parametrize("hw", BN.POOL_MAPS)
@pytest.mark.parametrize("ksp", BN.POOLS)
def test_standalone_pool(be, ksp, hw):
    SEEN.add(BN.check_standalone_pool(be, *ksp, *hw, seed=1400 + hw[1]))


@pytest.mark.parametrize("hw", BN.POOL_MAPS)
@pytest.mark.parametrize("ksp", BN.POOLS)
def test_folded_pool(be, ksp, hw):
    SEEN.add(BN.check_folded_pool(be, *ksp, *hw, seed=1500 + hw[1]))


@pytest.mark.parametrize("case", range(len(BN.LARGE_GRID)), ids=[c[0] for c in BN.LARGE_GRID])
def test_several_output_words_per_block(be, case):
    """The "several output words per block" cases (7 to 18 s each here; the emulator runs its blocks in order, so it shows a wrong loop, not a race between two
    words -- that is what the GPU run of the same table is for)."""
    BN.check_large(be, case)


def test_refusals_keep_refusing(be):
    BN.check_refusals(be)


def test_every_new_instantiation_ran(be):
    """(runs last in this file) the cases above launched every new template instantiation at least once."""
    assert BN.INSTANTIATIONS <= SEEN, sorted(BN.INSTANTIATIONS - SEEN)
