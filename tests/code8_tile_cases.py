"""csrc/qgemm_codes_w8_tile.h (mn_code8conv5_*, mn_code8_maxpool) through the C ABI: one case table for the CPU emulation build and the GPU.  The judge is numpy: the
5x5 accumulators in int64 (asserted within int32), then codes_w8_cases.chain_codes; the pools by a window maximum over the uint8 codes.  Bytes must be equal, tail
positions the code 0; output maps are poisoned before the launch, with a guard region behind them."""
import ctypes as C

import numpy as np

from bits_cases import _dev_i32, _empty_i32, _host_u32
from code8_res_cases import guarded_map, read_map
from codes_cases import make_chan, shuffle_order
from codes_nin_cases import np_codes_maxpool
from codes_w8_cases import W8, chain_codes, make_inputs, to_map
from micronet_amd._lib import MN_EINVAL, MN_ENOTSUP

# (id, x shape, O, consumer shuffle, seed, every input code / every weight code or None)
CONVS = [
    ("odd_narrow_map", (1, 16, 5, 7), 24, 0, 8700, None),                 # every border class, narrower than its halo tile, a partial output block; 25 slots: 3 padding slots
    ("images_share_a_block", (3, 48, 6, 6), 80, 2, 8701, None),           # 75 slots: one padding slot; two sets; three images in one tile: the halo between images
    ("two_row_bands", (1, 16, 20, 16), 16, 0, 8702, None),                # 320 pixels: a band of 16 rows and one of 4, the halo rows of each from the other
    ("saturated_255_against_0", (1, 16, 5, 7), 24, 0, 8700, (255, 0)),
    ("saturated_all_0", (1, 16, 5, 7), 24, 0, 8700, (0, 77)),
]
# (x shape, (kernel, stride, padding))
POOLS = [((1, 20, 5, 7), (3, 2, 1)), ((2, 32, 8, 8), (3, 2, 1)), ((2, 32, 8, 8), (2, 2, 0))]
# geometries refused: (x shape, w shape, stride, padding, groups, widths)
REFUSED = [
    ((1, 32, 8, 8), (32, 16, 5, 5), 1, 2, 2, W8), ((1, 32, 8, 8), (32, 32, 5, 5), 2, 2, 1, W8), ((1, 32, 8, 8), (32, 32, 5, 5), 1, 1, 1, W8),
    ((1, 20, 8, 8), (32, 20, 5, 5), 1, 2, 1, W8), ((1, 32, 8, 8), (32, 32, 5, 5), 1, 2, 1, (4, 4, 4)),
    ((1, 48, 2, 256), (16, 48, 5, 5), 1, 2, 1, W8),          # 3 * 5 * 260 = 3900 blocks: one output row with its halo is beyond 48 KB
]


def check_conv(be, idx):
    cid, x_shape, Oc, shuffle, seed, fill = CONVS[idx]
    codes, w, acc = make_inputs(x_shape, Oc, 5, 1, seed, fill)
    chan, order, g = make_chan(acc, seed), (shuffle_order(Oc, shuffle) if shuffle else None), be.geom(x_shape, w.shape, padding=2)
    ref = chain_codes(acc, chan, 0)
    nb = int(be.lib.mn_code8conv5_table_bytes(C.byref(g), *W8))
    assert be.lib.mn_code8conv5_supported(C.byref(g), *W8) == 1 and nb > 0 and nb % 16 == 0
    table, dO, dW, dC = _empty_i32(be, (nb // 4,)), (_dev_i32(be, order.astype(np.int32)) if shuffle else None), be.to_dev(w), be.to_dev(chan)
    be.call("mn_code8conv5_pack", C.byref(g), be.ptr(dW), be.ptr(dC), 8, 8, 8, be.ptr(dO), be.ptr(table), be.stream)
    hdr = _host_u32(be, table)
    assert (int(hdr[0]), int(hdr[7]), int(hdr[1])) == (0, 0, (25 * x_shape[1] // 16 + 3) // 4), "finite constants, weights on the grid, a valid order"
    N, _, H, Wd = x_shape
    (buf, size), dX = guarded_map(be, N, Oc, H * Wd), be.to_dev_u8(to_map(codes))
    be.call("mn_code8conv5_fwd", C.byref(g), be.ptr(table), be.ptr(dX), be.ptr(buf), be.stream)
    name, got = be.lib.mn_last_kernel().decode(), read_map(be, buf, size, N, Oc, H, Wd)
    want = ref[:, order] if shuffle else ref
    print(name, cid, "mismatches against the judge", int((got[:, :Oc] != want).sum()), "of", want.size, "distinct codes", len(np.unique(ref)))
    assert name == "k_code8conv5<5>" and np.array_equal(got[:, :Oc], want) and (got[:, Oc:] == 0).all()
    if fill is None:
        assert len(np.unique(ref)) > 16 and (acc[:, 4] == int(chan[2, 4])).any() and (acc[:, 5] == int(chan[2, 5])).any() and chan[4, 3] < 0
    else:          # a 5 x 7 map: the pixels of row 2, columns 2 .. 4 see all 25 x 16 positions, a corner 9 x 16
        assert (int(acc.min()), int(acc[0, 0, 2, 3]), int(acc.max())) == ((-255 * 255 * 16 * 25,) * 2 + (-255 * 255 * 16 * 9,) if fill[0] else (0, 0, 0))


def check_pool(be, idx):
    x_shape, (k, s, p) = POOLS[idx]
    codes = np.random.default_rng(8750 + idx).integers(0, 256, size=x_shape).astype(np.uint8)
    codes[:, :, 0, 0], codes[0, :, -1, -1] = 0, 255                      # a whole-zero pixel and a saturated one
    ref = np_codes_maxpool(codes, k, s, p)
    N, Cc, H, Wd = x_shape
    (buf, size), dX = guarded_map(be, N, Cc, ref.shape[2] * ref.shape[3]), be.to_dev_u8(to_map(codes))
    be.call("mn_code8_maxpool", be.ptr(dX), N, Cc, H, Wd, k, s, p, be.ptr(buf), be.stream)
    got = read_map(be, buf, size, N, Cc, *ref.shape[2:])
    assert be.lib.mn_last_kernel().decode() == "k_code8_maxpool"
    assert np.array_equal(got[:, :Cc], ref) and (got[:, Cc:] == 0).all(), "the window maximum of the codes; tail channels the code 0"


def check_refused(be, idx):
    """MN_ENOTSUP from every entry of a geometry (past the table: a pool kind) that is not covered; the poisoned buffer stays as it was."""
    buf, f = _empty_i32(be, (64,)), be.to_dev(np.zeros(64, dtype=np.float32))
    if idx < len(REFUSED):
        x_shape, w_shape, stride, padding, groups, (ai, wb, ao) = REFUSED[idx]
        g = be.geom(x_shape, w_shape, stride=stride, padding=padding, groups=groups)
        assert be.lib.mn_code8conv5_supported(C.byref(g), ai, wb, ao) == 0 and int(be.lib.mn_code8conv5_table_bytes(C.byref(g), ai, wb, ao)) == 0
        assert be.lib.mn_code8conv5_pack(C.byref(g), be.ptr(f), be.ptr(f), ai, wb, ao, None, be.ptr(buf), be.stream) == MN_ENOTSUP
        assert (ai, wb, ao) != W8 or be.lib.mn_code8conv5_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), be.stream) == MN_ENOTSUP          # (the forward takes no widths)
    else:
        assert be.lib.mn_code8_maxpool(be.ptr(f), 1, 16, 2, 2, 3, 1, 1, be.ptr(buf), be.stream) == MN_ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_invalid(be, _=None):
    """MN_EINVAL: a null table, a misaligned map, an output that overlaps the input, a pool in place."""
    g = be.geom((1, 16, 4, 4), (16, 16, 5, 5), padding=2)
    buf, out = _empty_i32(be, (4096,)), _empty_i32(be, (4096,))
    p, o, odd = be.ptr(buf), be.ptr(out), be.ptr_at(out, 1)
    fwd, pool = be.lib.mn_code8conv5_fwd, be.lib.mn_code8_maxpool
    assert fwd(C.byref(g), None, p, o, be.stream) == MN_EINVAL and fwd(C.byref(g), p, p, odd, be.stream) == MN_EINVAL and fwd(C.byref(g), p, o, o, be.stream) == MN_EINVAL
    assert pool(None, 1, 16, 4, 4, 2, 2, 0, o, be.stream) == MN_EINVAL and pool(p, 1, 16, 4, 4, 2, 2, 0, odd, be.stream) == MN_EINVAL
    assert pool(o, 1, 16, 4, 4, 2, 2, 0, o, be.stream) == MN_EINVAL, "no in-place pool"
    assert (_host_u32(be, out) == 0x5a5a5a5a).all(), "an invalid call writes nothing"


# (id, check, argument) for the two drivers: tests/test_code8_tile_emulated.py, tests/test_gpu_code8_tile.py
CHECKS = ([(c[0], check_conv, i) for i, c in enumerate(CONVS)] + [("pool%d_k%d" % (i, c[1][0]), check_pool, i) for i, c in enumerate(POOLS)]
          + [("refused%d" % i, check_refused, i) for i in range(len(REFUSED) + 1)] + [("invalid", check_invalid, None)])
