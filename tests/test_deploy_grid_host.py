"""The launch rule of the bit / code / byte deployment forwards (csrc/qgemm_mfma_sets.h: grid_rows, grid_deal) as the library states it through mn_deploy_grid_rows /
mn_deploy_grid_deal, exhaustively over bx in 1..4200 and units in 1..64, on the product library and on the CPU emulation build.  Host only: nothing is launched.

The "several units per block" cases of the kernel tables (tests/deploy_grid.py) prove through these two entries that they reach the kernels' inner loops; the
properties below are what those loops rely on: every unit is dealt, no block of grid.y is empty, and the grid is not cut below what fills the chip."""
import ctypes as C

import numpy as np
import pytest

import abi_driver
from micronet_amd import _lib

BX, UNITS = 4200, 64


@pytest.fixture(scope="module", params=["product", "emu"])
def lib(request):
    return _lib.get_lib() if request.param == "product" else abi_driver.Backend("emu").lib


@pytest.fixture(scope="module")
def table(lib):
    """(rows, gy, per) as int arrays [BX + 1, UNITS + 1] (row / column 0 unused), every pair asked once."""
    rows, gy, per = (np.zeros((BX + 1, UNITS + 1), dtype=np.int64) for _ in range(3))
    p = C.c_int(0)
    for bx in range(1, BX + 1):
        for u in range(1, UNITS + 1):
            rows[bx, u] = lib.mn_deploy_grid_rows(bx, u)
            p.value = -1
            gy[bx, u] = lib.mn_deploy_grid_deal(bx, u, C.byref(p))
            per[bx, u] = p.value
    return rows[1:, 1:], gy[1:, 1:], per[1:, 1:]


def _axes():
    return np.arange(1, BX + 1).reshape(-1, 1), np.arange(1, UNITS + 1).reshape(1, -1)


def test_every_unit_is_dealt_and_no_block_is_empty(table):
    rows, gy, per = table
    bx, u = _axes()
    assert (gy >= 1).all() and (gy <= u).all() and (per >= 1).all()
    assert (gy * per >= u).all(), "every unit is dealt"
    assert ((gy - 1) * per < u).all(), "the last block of grid.y has a unit"
    assert (gy <= rows).all(), "the deal never launches more rows than the round-robin rule"
    assert (rows >= 1).all() and (rows <= u).all()


def test_one_unit_per_block_until_the_pixels_fill_the_chip(table):
    rows, gy, per = table
    bx, u = _axes()
    # the cap as the library holds it: the smallest bx from which a single row is launched whatever the units
    first = int(np.flatnonzero((rows == 1).all(axis=1))[0]) + 1
    assert (rows[first - 1:] == 1).all() and first == 2048, first
    small = bx * u <= first
    assert (gy[small] == u.repeat(BX, 0)[small]).all() and (per[small] == 1).all() and (rows[small] == u.repeat(BX, 0)[small]).all()
    assert (rows * bx >= np.minimum(first, bx * u)).all(), "grid.y is not cut below what fills the chip"
    assert (per[first - 1:] == u).all() and (gy[first - 1:] == 1).all(), "from there one block takes every unit"


def test_the_shapes_the_kernel_tables_lean_on(lib):
    """bx = 344, 7 units: four blocks of two, the last with one; bx = 688, 4 spans: three rows, block 0 takes spans 0 and 3."""
    p = C.c_int(0)
    assert lib.mn_deploy_grid_deal(344, 7, C.byref(p)) == 4 and p.value == 2
    assert lib.mn_deploy_grid_deal(300, 9, C.byref(p)) == 5 and p.value == 2
    assert lib.mn_deploy_grid_rows(688, 4) == 3
    assert lib.mn_deploy_grid_deal(128, 16, C.byref(p)) == 16 and p.value == 1          # batch 32 of a 32 x 32 layer: what the plan tests ran at before


def test_invalid_arguments_are_einval(lib):
    p = C.c_int(7)
    for bx, u in ((0, 4), (-1, 4), (4, 0), (4, -3), (0, 0)):
        assert lib.mn_deploy_grid_rows(bx, u) == _lib.MN_EINVAL
        assert lib.mn_deploy_grid_deal(bx, u, C.byref(p)) == _lib.MN_EINVAL and p.value == 7
    assert lib.mn_deploy_grid_deal(4, 4, None) == _lib.MN_EINVAL
    assert "mn_deploy_grid_deal" in lib.mn_last_error().decode()
