"""csrc/qgemm_iao8_tile.h on the CPU SIMT emulator through the C ABI: the checks of tests/iao8_tile_cases.py (on the MI355X: tests/test_gpu_iao8_tile.py)."""
import pytest

import abi_driver
import iao8_tile_cases as T


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("emu")


@pytest.mark.parametrize("check, arg", [c[1:] for c in T.CHECKS], ids=[c[0] for c in T.CHECKS])
def test_iao8_tile(be, check, arg):
    check(be, arg)
