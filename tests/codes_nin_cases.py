"""Code-packed kernels the plain nin net needs (csrc/qgemm_codes.h: the LDS-tiled dense 5x5 block mn_codeconv_tile_*, the max-pool on code planes mn_codes_maxpool)
through the C ABI: one case table for the CPU emulation build and the GPU.  Every comparison is exact.

The judge of a block is that of tests/codes_cases.py -- an int64 numpy convolution gives acc, the library's mn_qa_fwd(stash = acc) gives codes, the numpy fp32 chain is
replayed step by step, the two must agree and the kernel must equal both -- with the constants of ``make_chan`` (gamma < 0, gamma = 0, thresholds out of reach both
ways, a rounding boundary on an attained acc).  The judge of a pool is a numpy maximum over the window of the unpacked codes with 0 padding."""
import ctypes as C

import numpy as np

import codes_cases as CC
from bits_cases import _dev_i32, _empty_i32, _host_u32
from bits_nin_cases import pooled_size
from codes_cases import judge, make_chan, make_inputs, np_pack_planes, np_unpack_planes, shuffle_order

F = np.float32
A_BITS = W_BITS = 2
K_BOUND_C = 145          # C * 25 * 9 <= 32767

# (id, x shape, w shape, out_order shuffle, kernel)
BLOCKS = [
    ("three_words_partial_out", (2, 96, 8, 8), (40, 96, 5, 5), 0, "k_codeconv_tile<5,3>"),      # three words unrolled, a partial output word, 48 of 64 pixels lose taps
    ("partial_in_two_tiles", (3, 40, 12, 20), (33, 40, 5, 5), 0, "k_codeconv_tile<5,0>"),       # a partial input word, tile remainders in both directions
    ("k_bound_short_map", (1, K_BOUND_C, 4, 8), (32, K_BOUND_C, 5, 5), 0, "k_codeconv_tile<5,0>"),          # the K bound, five words rolled, a map shorter than the kernel
    ("shuffled_order", (2, 32, 16, 16), (64, 32, 5, 5), 4, "k_codeconv_tile<5,0>"),
]
# Several output word groups per block (tests/deploy_grid.py): the smallest shape at which a block of k_codeconv_tile walks more than one group.  4 * 86 tiles of
# 16 x 16, seven groups: four blocks of two, the last takes one; O % 32 = 8, the consumer's shuffle.  GPU only (tests/test_gpu_codes_nin.py): 24 s on the
# CPU emulation build (8 cores).
LARGE_GRID = [
    ("seven_groups", (86, 8, 32, 32), (200, 8, 5, 5), 4, "k_codeconv_tile<5,0>"),
]
# the K-bound fills: every code 3 against every weight code 3 / 0.  On the 4 x 8 map of the case above a window holds at most 4 x 5 taps (acc = +-26100); the 5 x 8
# map holds a whole window, so that acc = +-32625 = +-(145 * 25 * 9), the ends of the range, is attained
FILLS = [((1, K_BOUND_C, 4, 8), 26100), ((1, K_BOUND_C, 5, 8), 32625)]

REFUSED = [
    (dict(x_shape=(1, 146, 8, 8), w_shape=(32, 146, 5, 5), padding=2), (2, 2, 2)),                # C = 146: beyond the K bound
    (dict(x_shape=(1, 64, 8, 8), w_shape=(32, 32, 5, 5), padding=2, groups=2), (2, 2, 2)),        # grouped
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=1), (2, 2, 2)),                  # padding 1
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1), (2, 2, 2)),                  # a 3x3: mn_codeconv_* covers it
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1), padding=0), (2, 2, 2)),                  # a 1x1: mn_codeconv_* covers it
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2, stride=2), (2, 2, 2)),        # stride 2
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), (3, 2, 2)),                  # 3-bit input codes
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), (2, 4, 2)),                  # 4-bit weights
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), (2, 2, 3)),                  # 3-bit output codes
]

# (x shape, (k, stride, pad), a_bits)
POOLS = [
    ((2, 40, 7, 9), (3, 2, 1), 2),          # odd sizes, a last window that is half padding
    ((1, 32, 8, 8), (2, 2, 0), 2),
    ((1, 70, 6, 4), (3, 2, 1), 3),          # three planes: a wrong plane order shows
]
POOLS_REFUSED = [(3, 1, 1, 2), (4, 2, 1, 2), (3, 2, 2, 2), (2, 1, 0, 2), (2, 2, 1, 2), (3, 2, 0, 2), (3, 3, 1, 2), (3, 2, 1, 0), (3, 2, 1, 9), (2, 2, 0, 9)]


def _enotsup():
    from micronet_amd import _lib
    return _lib.MN_ENOTSUP


def pack_tile_table(be, g, w, chan, order=None):
    nb = int(be.lib.mn_codeconv_tile_table_bytes(C.byref(g), A_BITS, W_BITS, A_BITS))
    assert nb > 0 and nb % 4 == 0
    table = _empty_i32(be, (nb // 4,))
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    dW, dC = be.to_dev(w), be.to_dev(chan)
    be.call("mn_codeconv_tile_pack", C.byref(g), be.ptr(dW), be.ptr(dC), A_BITS, W_BITS, A_BITS, be.ptr(dO), be.ptr(table), be.stream)
    return table


def tile_planes(be, codes, w, chan, order=None):
    """Pack the table and the planes, run mn_codeconv_tile_fwd TWICE into poisoned buffers; returns (output planes as host uint32, kernel name)."""
    g = be.geom(codes.shape, w.shape, padding=2)
    assert be.lib.mn_codeconv_tile_supported(C.byref(g), A_BITS, W_BITS, A_BITS) == 1, "geometry must be covered by the tiled code kernel"
    assert be.lib.mn_codeconv_supported(C.byref(g), A_BITS, W_BITS, A_BITS) == 0, "mn_codeconv_* keeps refusing 5x5"
    table = pack_tile_table(be, g, w, chan, order)
    hdr = _host_u32(be, table)
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0, "finite constants, weights on the grid, a valid order"
    xp = _dev_i32(be, np_pack_planes(codes).view(np.int32))
    N, _, H, Wd = codes.shape
    outs = []
    for _ in range(2):
        yp = _empty_i32(be, (N, (w.shape[0] + 31) // 32, A_BITS, H, Wd))          # poisoned
        be.call("mn_codeconv_tile_fwd", C.byref(g), be.ptr(table), be.ptr(xp), be.ptr(yp), be.stream)
        outs.append(_host_u32(be, yp))
    name = be.lib.mn_last_kernel().decode()
    assert np.array_equal(outs[0], outs[1]), "two runs give identical planes"
    Oc = w.shape[0]
    if Oc % 32:
        assert not (outs[0][:, -1] >> np.uint32(Oc % 32)).any(), "unused bits of the last output group are 0"
    return outs[0], name


def check_large(be, case):
    """One LARGE_GRID case: the library's own launch rule says that a block takes at least two word groups and the last block fewer; then check_block, whose exact
    accumulator comes from deploy_grid.exact_conv at this size."""
    import deploy_grid as DG
    _, (N, _, H, Wd), w_shape, _, _ = LARGE_GRID[case]
    DG.assert_uneven_deal(be, DG.tile_blocks(N, H, Wd), (w_shape[0] + 31) // 32)
    check_block(be, case, LARGE_GRID, 2150, DG.exact_conv)


def check_block(be, case, table=None, seed0=2100, conv=None):
    _, x_shape, w_shape, s, kernel = (BLOCKS if table is None else table)[case]
    seed = seed0 + case
    codes, w, acc = make_inputs(x_shape, w_shape, 1, 2, seed, conv=conv)
    chan = make_chan(acc, seed)
    ref = judge(be, acc, chan, 0)
    assert len(np.unique(ref)) == 4, "the case must produce all four codes"
    full = CC.chain_codes(acc, chan, 0)
    assert (full[:, 1] == 0).all() and (full[:, 2] == CC.N_LEVELS).all() and len(np.unique(full[:, 0])) == 1
    assert (acc[:, 4] == int(chan[2, 4])).any() and (acc[:, 5] == int(chan[2, 5])).any(), "a code boundary sits on an attained accumulator value"
    Oc = w_shape[0]
    order = shuffle_order(Oc, s) if s else None
    planes, name = tile_planes(be, codes, w, chan, order)
    got = np_unpack_planes(planes, Oc)
    want = ref[:, order] if s else ref
    print(name, x_shape, w_shape, "shuffle", s, "mismatches", int((got != want).sum()), "of", got.size)
    assert name == kernel, name
    assert np.array_equal(got, want), (int((got != want).sum()), got.size)


def check_fill(be, case, kcode):
    """All codes 3 against all weight codes ``kcode`` (3: acc = +9 per tap and channel, 0: -9) at the K bound."""
    x_shape, extreme = FILLS[case]
    w_shape = (32, K_BOUND_C, 5, 5)
    codes = np.full(x_shape, 3, dtype=np.uint8)
    k = np.full(w_shape, kcode, dtype=np.int64)
    w = (F(2) * (k.astype(F) / F(3)) - F(1)).astype(F)
    acc = CC.O.conv2d_fwd(codes.astype(np.int64), 2 * k - 3, None, padding=2, groups=1, acc=np.int64)
    sign = 1 if kcode == 3 else -1
    assert int(acc.max() if sign > 0 else acc.min()) == sign * extreme and np.abs(acc).max() <= 32767
    chan = make_chan(acc, 2200 + case)
    ref = judge(be, acc, chan, 0)
    planes, name = tile_planes(be, codes, w, chan)
    got = np_unpack_planes(planes, w_shape[0])
    print(name, x_shape, "fill", kcode, "extreme acc", sign * extreme, "mismatches", int((got != ref).sum()), "of", got.size)
    assert name == "k_codeconv_tile<5,0>" and np.array_equal(got, ref)


def check_refused(be, case):
    kw, (ai, wb, ao) = REFUSED[case]
    g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), groups=kw.get("groups", 1))
    assert be.lib.mn_codeconv_tile_supported(C.byref(g), ai, wb, ao) == 0
    assert int(be.lib.mn_codeconv_tile_table_bytes(C.byref(g), ai, wb, ao)) == 0
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    rc = be.lib.mn_codeconv_tile_pack(C.byref(g), be.ptr(f), be.ptr(f), ai, wb, ao, None, be.ptr(buf), be.stream)
    assert rc == _enotsup(), rc
    if (ai, wb, ao) == (2, 2, 2):
        assert be.lib.mn_codeconv_tile_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), be.stream) == _enotsup()
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_invalid(be):
    """Null, misaligned and an invalid geometry are MN_EINVAL and write nothing."""
    from micronet_amd import _lib
    g = be.geom((1, 32, 8, 8), (32, 32, 5, 5), padding=2)
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    odd = C.c_void_p(be.ptr(buf).value + 2)
    assert be.lib.mn_codeconv_tile_pack(C.byref(g), None, be.ptr(f), 2, 2, 2, None, be.ptr(buf), be.stream) == _lib.MN_EINVAL
    assert be.lib.mn_codeconv_tile_pack(C.byref(g), be.ptr(f), be.ptr(f), 2, 2, 2, None, odd, be.stream) == _lib.MN_EINVAL
    assert be.lib.mn_codeconv_tile_fwd(C.byref(g), be.ptr(buf), None, be.ptr(buf), be.stream) == _lib.MN_EINVAL
    assert be.lib.mn_codeconv_tile_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), odd, be.stream) == _lib.MN_EINVAL
    g0 = be.geom((0, 32, 8, 8), (32, 32, 5, 5), padding=2)
    assert be.lib.mn_codeconv_tile_supported(C.byref(g0), 2, 2, 2) == 0
    assert be.lib.mn_codeconv_tile_fwd(C.byref(g0), be.ptr(buf), be.ptr(buf), be.ptr(buf), be.stream) == _lib.MN_EINVAL
    assert be.lib.mn_codes_maxpool(None, 1, 1, 2, 8, 8, 3, 2, 1, be.ptr(buf), be.stream) == _lib.MN_EINVAL
    assert be.lib.mn_codes_maxpool(be.ptr(buf), 1, 1, 2, 8, 8, 3, 2, 1, odd, be.stream) == _lib.MN_EINVAL
    assert be.lib.mn_codes_maxpool(be.ptr(buf), 0, 1, 2, 8, 8, 3, 2, 1, be.ptr(buf), be.stream) == _lib.MN_EINVAL
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all()


def check_counters(be, seed=5):
    """Non-finite channel constants are counted into word 0 of the table, a weight off the grid (and a bad out_order entry) into word 7."""
    x_shape, w_shape = (1, 32, 4, 4), (32, 32, 5, 5)
    codes, w, acc = make_inputs(x_shape, w_shape, 1, 2, seed)
    chan = make_chan(acc, seed)
    g = be.geom(x_shape, w_shape, padding=2)
    hdr = _host_u32(be, pack_tile_table(be, g, w, chan))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0
    assert (int(hdr[1]), int(hdr[2]), int(hdr[4]), int(hdr[5])) == (1, 25, 32, 1) and int(hdr[6]) == (2 | 2 << 8 | 2 << 16)
    bad = chan.copy()
    bad[0, 7], bad[4, 9], bad[3, 11] = F(np.inf), F(np.nan), F(2e9)
    hdr = _host_u32(be, pack_tile_table(be, g, w, bad))
    assert int(hdr[0]) == 3 and int(hdr[7]) == 0
    w2 = w.copy()
    w2[5, 0, 0, 0] = F(0.5)
    hdr = _host_u32(be, pack_tile_table(be, g, w2, chan))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 1
    order = np.arange(w_shape[0])
    order[3] = w_shape[0]
    assert int(_host_u32(be, pack_tile_table(be, g, w, chan, order))[7]) == 1


def np_codes_maxpool(codes, k, s, p):
    """max over the window with 0 padding (codes are >= 0: a padded tap never wins against one inside the image)"""
    N, Cc, H, W = codes.shape
    Ho, Wo = pooled_size(H, k, s, p), pooled_size(W, k, s, p)
    big = np.zeros((N, Cc, H + 2 * p + k, W + 2 * p + k), dtype=np.int32)
    big[:, :, p:p + H, p:p + W] = codes
    out = np.zeros((N, Cc, Ho, Wo), dtype=np.int32)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, big[:, :, dy:dy + s * Ho:s, dx:dx + s * Wo:s])
    return out.astype(np.uint8)


def check_pool(be, case):
    import torch
    x_shape, (k, s, p), a_bits = POOLS[case]
    r = np.random.default_rng(2300 + case)
    codes = (r.integers(0, 1 << a_bits, size=x_shape) * (r.random(x_shape) < 0.3)).astype(np.uint8)          # mostly 0, so that every code is some window's maximum
    N, Cc, H, Wd = x_shape
    Cw, Ho, Wo = (Cc + 31) // 32, pooled_size(H, k, s, p), pooled_size(Wd, k, s, p)
    xp = _dev_i32(be, np_pack_planes(codes, a_bits).view(np.int32))
    yp = _empty_i32(be, (N, Cw, a_bits, Ho, Wo))          # poisoned
    be.call("mn_codes_maxpool", be.ptr(xp), N, Cw, a_bits, H, Wd, k, s, p, be.ptr(yp), be.stream)
    assert be.lib.mn_last_kernel().decode() == "k_codes_maxpool"
    got = _host_u32(be, yp)
    if Cc % 32:
        assert not (got[:, -1] >> np.uint32(Cc % 32)).any(), "unused bits of the last group stay 0"
    ref = np_codes_maxpool(codes, k, s, p)
    assert np.array_equal(ref, torch.nn.functional.max_pool2d(torch.from_numpy(codes.astype(F)), k, s, p).numpy().astype(np.uint8))
    out = np_unpack_planes(got, Cc)
    print("k_codes_maxpool", x_shape, (k, s, p), a_bits, "bits: mismatches", int((out != ref).sum()), "of", out.size)
    assert out.shape == ref.shape and np.array_equal(out, ref)
    assert len(np.unique(out)) == 1 << a_bits


def check_pool_refused(be):
    buf = _empty_i32(be, (4096,))
    for k, s, p, a_bits in POOLS_REFUSED:
        rc = be.lib.mn_codes_maxpool(be.ptr(buf), 1, 1, a_bits, 8, 8, k, s, p, be.ptr(buf), be.stream)
        assert rc == _enotsup(), (k, s, p, a_bits, rc)
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"
