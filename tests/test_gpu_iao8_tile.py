"""csrc/qgemm_iao8_tile.h on the MI355X through the C ABI: the checks of tests/iao8_tile_cases.py (on the CPU emulator: tests/test_iao8_tile_emulated.py)."""
import pytest

import abi_driver
import iao8_tile_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("check, arg", [c[1:] for c in T.CHECKS], ids=[c[0] for c in T.CHECKS])
def test_iao8_tile(be, check, arg):
    check(be, arg)
