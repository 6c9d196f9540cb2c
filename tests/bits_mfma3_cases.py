"""The int8-MFMA form of the 3x3 hidden bit block (csrc/qgemm_bits_mfma3.h: mn_bitconv_mfma3_*) through the C ABI: one case table for the CPU emulation build and the
GPU.  Every comparison is exact.

The two judges of tests/bits_mfma_cases.py: ``a_ref`` of ``bits_cases.make_inputs`` (the numpy fp32 expression) and mn_bitconv_fwd's output words on the same inputs and
order.  The input is packed by ``bits_cases.np_pack`` (mn_bits_pack_sign8 wants H * W % 4 == 0).  Buffers are poisoned and every case runs twice."""
import ctypes as C

import numpy as np

import bits_mfma_cases as BM
from bits_cases import make_inputs
from codes_cases import shuffle_order

F = np.float32
QUARTET, KERNEL = "mn_bitconv_mfma3", "k_bitconv_mfma3<0>"

# (id, x shape, w shape, groups, out_order shuffle, W, header word 5 (dead rows): 0, or None for "> 0", seed)
BLOCKS = [
    ("nin_gc_l4", (2, 256, 4, 8), (512, 16, 3, 3), 16, 16, 3, 0, 4300),          # span of 8 words, high / low half-words, interior and border pixels
    ("nin_gc_l7", (1, 512, 4, 4), (1024, 16, 3, 3), 32, 32, 3, 0, 4301),         # span of 16 words, fewer pixels than one wave
    ("padded_last_step", (3, 48, 5, 7), (40, 48, 3, 3), 1, 0, 3, None, 4302),    # 27 slots: a padded last k-step; partial input / output word; 105 pixels; dead rows
    ("upper_half_start", (1, 96, 4, 8), (64, 48, 3, 3), 2, 2, 3, 0, 4303),       # the second group starts on the upper half of word 1
    ("nin_dense", (1, 192, 4, 4), (192, 192, 3, 3), 1, 0, 3, 0, 4304),           # 27 full k-steps, 12 M tiles
    ("dead_rows", (1, 32, 8, 8), (48, 16, 3, 3), 2, 0, 3, None, 4305),           # 24 rows per group
    ("one_row", (2, 32, 1, 8), (32, 32, 3, 3), 1, 0, 3, 0, 4306),                # a whole tap row outside everywhere
    ("one_column", (1, 32, 8, 1), (32, 32, 3, 3), 1, 0, 3, 0, 4307),             # a whole tap column outside everywhere
    ("binary_weights", (1, 64, 4, 4), (64, 32, 3, 3), 2, 0, 2, 0, 4308),         # W = 2: no zero weight
    ("span_of_four", (1, 256, 4, 4), (512, 16, 3, 3), 16, 8, 3, 0, 4309),        # span of 4 words (shuffle 8 over 16 groups: 8 groups x 16 rows in 128 positions)
]
# Several spans per block (tests/deploy_grid.py): the smallest shapes at which a block of k_bitconv_mfma3 takes a second span (sp += gridDim.y).  Seven words in spans
# of two: four spans over grid.y = 3 at bx = 688 -- block 0 takes spans 0 and 3.  GPU only (tests/test_gpu_bits_mfma3.py): about 120 s each on the CPU emulation build (8 cores).
LARGE_GRID = [
    ("four_spans", (43, 16, 64, 64), (224, 16, 3, 3), 1, 0, 3, 0, 4310),
    ("four_spans_shuffled_partial", (43, 16, 64, 64), (200, 16, 3, 3), 1, 4, 3, None, 4311),          # O % 32 = 8
]
SPANS = {"nin_gc_l4": 8, "nin_gc_l7": 16, "nin_dense": 2, "span_of_four": 4}          # header word 2 where the span is known
FILL_X, FILL_W = (1, 400, 3, 3), (32, 400, 3, 3)          # all nine taps inside at the centre pixel only: acc = +-3600 there, +-1600 / +-2400 elsewhere

# (geometry keywords, in_shuffle, pool)
REFUSED = [
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1), 0, 1),                # the pooled 3x3 block stays on k_bitconv
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1), 0, 2),                # no 3x3 / 2 fold at all
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), 0, 0),                           # a 1x1: k_bitconv / k_bitconv_mfma keep it
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), 0, 0),                # a 5x5: the tile kernel keeps it
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=0), 0, 0),                # padding 0
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1, stride=2), 0, 0),      # stride 2
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 8, 3, 3), padding=1, groups=4), 0, 0),       # 8 channels per group
    (dict(x_shape=(1, 48, 8, 8), w_shape=(32, 24, 3, 3), padding=1, groups=2), 0, 0),      # 24 channels per group
]


def check_block(be, case, table=None):
    cid, x_shape, w_shape, groups, s, Wb, dead, seed = (BLOCKS if table is None else table)[case]
    _, x_log, w, b, a_ref = make_inputs(x_shape, w_shape, groups, 0, 1, seed, Wb)
    assert (a_ref == 1).any() and (a_ref == -1).any()
    order = shuffle_order(w_shape[0], s) if s else None
    hdr = BM.against_both(be, QUARTET, KERNEL, x_log, w, b, a_ref, groups, 1, order, 0, "%s %s groups %d shuffle %d W %d" % (x_shape, w_shape, groups, s, Wb))
    print("span", int(hdr[2]), "dead rows", int(hdr[5]))
    assert (int(hdr[5]) == 0) if dead == 0 else (int(hdr[5]) > 0), ("dead rows", int(hdr[5]))
    assert int(hdr[1]) == (9 * (x_shape[1] // groups // 16) + 3) // 4 and int(hdr[4]) == 32 * ((w_shape[0] + 31) // 32)
    if cid in SPANS:
        assert int(hdr[2]) == SPANS[cid], ("span", int(hdr[2]))
    return hdr


def check_large(be, case):
    """One LARGE_GRID case: check_block -- both judges --, and through the library's own launch rule and the span the packer wrote into the table (header word 2) that
    some block of grid.y took a second span and some block did not."""
    import deploy_grid as DG
    _, (N, _, H, Wd), w_shape, _, _, _, _, _ = LARGE_GRID[case]
    hdr = check_block(be, case, LARGE_GRID)
    OW = (w_shape[0] + 31) // 32
    span = int(hdr[2])
    DG.assert_uneven_rows(be, DG.pixel_blocks(N * H * Wd, 256), (OW + 1) >> 1, (OW + span - 1) // span)


def check_fill(be, sign):
    """x all +1, w all ``sign``: the bias puts the decision boundary on the extreme acc, which only the centre pixel (all nine taps inside) attains.  A -1 (or +1)
    read from outside the image instead of 0 would move the border pixels' acc across it.  400 channels are beyond what mn_bitconv_fwd covers: judge 1 alone."""
    x = np.ones(FILL_X, dtype=np.int8)
    w = np.full(FILL_W, sign, dtype=F)
    b = np.full(FILL_W[0], -3600 if sign > 0 else 3599, dtype=F)
    ref = np.full((1, FILL_W[0], 3, 3), -sign, dtype=np.int8)
    ref[:, :, 1, 1] = sign
    g = be.geom(FILL_X, FILL_W, padding=1)
    assert be.lib.mn_bitconv_supported(C.byref(g)) == 0
    BM.against_both(be, QUARTET, KERNEL, x, w, b, ref, 1, 1, None, 0, "%s fill w = %d" % (FILL_X, sign), popc=False)
    # and with the border pixels' own extreme on the boundary: a corner has 4 taps inside (acc = +-1600), an edge 6 (+-2400)
    b2 = np.full(FILL_W[0], -2400 if sign > 0 else 2399, dtype=F)
    ref2 = np.full((1, FILL_W[0], 3, 3), sign, dtype=np.int8)
    ref2[:, :, ::2, ::2] = -sign
    BM.against_both(be, QUARTET, KERNEL, x, w, b2, ref2, 1, 1, None, 0, "%s fill w = %d, edge boundary" % (FILL_X, sign), popc=False)


def check_refused(be, case):
    BM.check_refused(be, case, QUARTET, REFUSED)


def check_invalid(be):
    BM.check_invalid(be, QUARTET, 3)


def check_counters(be):
    BM.check_counters(be, QUARTET, 3)
