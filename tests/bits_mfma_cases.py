"""The int8-MFMA form of the 1x1 hidden bit block (csrc/qgemm_bits_mfma.h: mn_bitconv_mfma_*) through the C ABI: one case table for the CPU emulation build and the GPU.
Every comparison is exact.

Inputs are those of ``bits_cases.make_inputs`` (exact zeros of acc * alpha + b, an alpha = 0 channel, two constant-decision channels: its own assertions).  Judge 1 is
its ``a_ref``, the numpy fp32 expression ``+1 iff not (fl(fl(acc * alpha) + b) < 0)`` (pooled: max_pool2d of the un-pooled ``a_ref``); judge 2 is mn_bitconv_fwd's output
words on the same inputs, order and pool.  Buffers are poisoned and every case runs twice."""
import ctypes as C

import numpy as np

from bits_cases import _dev_i32, _empty_i32, _host_u32, make_inputs, np_pack, np_unpack
from codes_cases import shuffle_order

F = np.float32

# (id, x shape, w shape, groups, out_order shuffle, pool, W, seed)
BLOCKS = [
    ("nin_gc_l2", (2, 256, 8, 8), (256, 128, 1, 1), 2, 2, 0, 3, 4100),             # two k-steps, 16 + 16 rows per word
    ("eight_per_group_pool", (1, 512, 4, 8), (512, 128, 1, 1), 4, 4, 1, 3, 4101),   # 8 rows per group per word, fewer pooled pixels than one tile
    ("partial_words", (3, 40, 6, 10), (33, 40, 1, 1), 1, 0, 0, 3, 4102),            # partial input word, K padded to 64, partial output word, pixel remainder
    ("two_and_a_half_steps", (1, 320, 4, 4), (64, 160, 1, 1), 2, 0, 1, 3, 4103),    # 2.5 k-steps, the second group starts at word 5
    ("half_a_step", (1, 128, 8, 8), (64, 32, 1, 1), 4, 0, 0, 3, 4104),              # half a k-step, two groups per output word
    ("dead_rows", (1, 64, 4, 8), (48, 32, 1, 1), 2, 0, 0, 3, 4105),                 # 24 rows per group: dead rows
    ("binary_weights", (1, 128, 4, 8), (64, 64, 1, 1), 2, 2, 0, 2, 4106),           # W = 2: no zero weight
]

# Several sets per block (tests/deploy_grid.py): the smallest shapes at which a block of k_bitconv_mfma walks set0 .. set1 over more than one set.  Seven sets over
# bx = 344 (pooled: 22016 pooled pixels / 64): four blocks of two, the last takes one.  GPU only (tests/test_gpu_bits_mfma.py): 56 s and 45 s on the CPU emulation build (8 cores).
LARGE_GRID = [
    ("seven_sets", (86, 64, 32, 32), (448, 32, 1, 1), 2, 2, 0, 3, 4110),
    ("seven_sets_pool_partial", (86, 64, 32, 32), (400, 32, 1, 1), 2, 4, 1, 3, 4111),          # 13 words: the last set is half a set, its last word half a word
]

# (geometry keywords, in_shuffle, pool)
REFUSED = [
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1), 0, 0),                # a 3x3: k_bitconv / k_bitconv_mfma3 keep it
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), 0, 0),                # a 5x5: the tile kernel keeps it
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1), stride=2), 0, 0),                 # stride 2
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1), padding=1), 0, 0),                # padding 1
    (dict(x_shape=(1, 64, 8, 8), w_shape=(64, 16, 1, 1), groups=4), 0, 0),                 # 16 channels per group: stays on k_bitconv
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), 2, 0),                           # an input shuffle is folded into the producer, never gathered
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), 0, 2),                           # the 3x3 / 2 fold stays on k_bitconv1_pool3
]


def _lib():
    from micronet_amd import _lib as L
    return L


def pooled_ref(a, pool):
    """max_pool2d (2x2 / 2) of the un-pooled decisions."""
    if not pool:
        return a
    import torch
    return torch.nn.functional.max_pool2d(torch.from_numpy(a.astype(F)), 2, 2).numpy().astype(np.int8)


def popcount_words(be, x_log, w, b, groups, padding, order, pool):
    """mn_bitconv_fwd's output words (judge 2): the table of mn_bitconv_pack, the input packed by numpy."""
    g = be.geom(x_log.shape, w.shape, padding=padding, groups=groups)
    assert be.lib.mn_bitconv_supported(C.byref(g)) == 1
    table = _empty_i32(be, (int(be.lib.mn_bitconv_table_bytes(C.byref(g))) // 4,))
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    dW, dB = be.to_dev(w), be.to_dev(b)
    be.call("mn_bitconv_pack", C.byref(g), be.ptr(dW), be.ptr(dB), be.ptr(dO), be.ptr(table), be.stream)
    assert int(_host_u32(be, table)[0]) == 0
    xb = _dev_i32(be, np_pack(x_log).view(np.int32))
    N, _, H, Wd = x_log.shape
    Ho, Wo = (H // 2, Wd // 2) if pool else (H, Wd)
    yb = _empty_i32(be, (N, (w.shape[0] + 31) // 32, Ho, Wo))
    be.call("mn_bitconv_fwd", C.byref(g), be.ptr(table), be.ptr(xb), be.ptr(yb), int(pool), be.stream)
    return _host_u32(be, yb)


def pack_table(be, quartet, g, w, b, order=None):
    nb = int(getattr(be.lib, quartet + "_table_bytes")(C.byref(g)))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    dW, dB = be.to_dev(w), be.to_dev(b)
    be.call(quartet + "_pack", C.byref(g), be.ptr(dW), be.ptr(dB), be.ptr(dO), be.ptr(table), be.stream)
    return table


def mfma_words(be, quartet, x_log, w, b, groups, padding, order=None, pool=0):
    """Pack the table and the bits, run ``quartet``_fwd TWICE into poisoned buffers; returns (output words as host uint32, kernel name, table header)."""
    g = be.geom(x_log.shape, w.shape, padding=padding, groups=groups)
    assert getattr(be.lib, quartet + "_supported")(C.byref(g)) == 1, "geometry must be covered by the MFMA bit kernel"
    table = pack_table(be, quartet, g, w, b, order)
    hdr = _host_u32(be, table)[:8].copy()
    assert int(hdr[0]) == 0, "every row's decision is monotone in acc, a valid order"
    xb = _dev_i32(be, np_pack(x_log).view(np.int32))
    N, _, H, Wd = x_log.shape
    Ho, Wo = (H // 2, Wd // 2) if pool else (H, Wd)
    outs = []
    for _ in range(2):
        yb = _empty_i32(be, (N, (w.shape[0] + 31) // 32, Ho, Wo))          # poisoned
        be.call(quartet + "_fwd", C.byref(g), be.ptr(table), be.ptr(xb), be.ptr(yb), int(pool), be.stream)
        outs.append(_host_u32(be, yb))
    name = be.lib.mn_last_kernel().decode()
    assert np.array_equal(outs[0], outs[1]), "two runs give identical words"
    Oc = w.shape[0]
    if Oc % 32:
        assert not (outs[0][:, -1] >> np.uint32(Oc % 32)).any(), "unused bits of the last output word are 0"
    return outs[0], name, hdr


def against_both(be, quartet, kernel, x_log, w, b, a_ref, groups, padding, order, pool, what, popc=True):
    Oc = w.shape[0]
    words, name, hdr = mfma_words(be, quartet, x_log, w, b, groups, padding, order, pool)
    got = np_unpack(words, Oc)
    want = pooled_ref(a_ref[:, order] if order is not None else a_ref, pool)
    print(name, what, "mismatches against a_ref", int((got != want).sum()), "of", got.size)
    assert name == kernel, name
    assert got.shape == want.shape and np.array_equal(got, want), (int((got != want).sum()), got.size)
    if popc:
        ref = popcount_words(be, x_log, w, b, groups, padding, order, pool)
        print(name, what, "words unlike mn_bitconv_fwd's", int((words != ref).sum()))
        assert words.shape == ref.shape and np.array_equal(words, ref), "the words of mn_bitconv_fwd, word for word"
    return hdr


def check_block(be, case, table=None):
    _, x_shape, w_shape, groups, s, pool, Wb, seed = (BLOCKS if table is None else table)[case]
    _, x_log, w, b, a_ref = make_inputs(x_shape, w_shape, groups, 0, 0, seed, Wb)
    assert (a_ref == 1).any() and (a_ref == -1).any()
    order = shuffle_order(w_shape[0], s) if s else None
    hdr = against_both(be, "mn_bitconv_mfma", "k_bitconv_mfma<%d>" % pool, x_log, w, b, a_ref, groups, 0, order, pool,
                       "%s %s groups %d shuffle %d pool %d W %d" % (x_shape, w_shape, groups, s, pool, Wb))
    assert (int(hdr[1]), int(hdr[4]), int(hdr[5])) == ((x_shape[1] // groups + 63) // 64, 32 * ((w_shape[0] + 31) // 32), (x_shape[1] + 31) // 32)
    return hdr


def check_large(be, case):
    """One LARGE_GRID case: the library's own launch rule says that a block takes at least two sets and the last block fewer; then check_block -- both judges."""
    import deploy_grid as DG
    _, (N, _, H, Wd), w_shape, _, _, pool, _, _ = LARGE_GRID[case]
    bx = DG.pixel_blocks(N * (H // 2) * (Wd // 2), 64) if pool else DG.pixel_blocks(N * H * Wd, 256)
    DG.assert_uneven_deal(be, bx, ((w_shape[0] + 31) // 32 + 1) // 2)          # a set: the rows of two consecutive output words
    hdr = check_block(be, case, LARGE_GRID)
    assert (int(hdr[4]) // 32 + 1) // 2 == ((w_shape[0] + 31) // 32 + 1) // 2


def check_refused(be, case, quartet="mn_bitconv_mfma", table=REFUSED):
    kw, shuf, pool = table[case]
    g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), groups=kw.get("groups", 1))
    g.in_shuffle = shuf
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    lib, ENOTSUP = be.lib, _lib().MN_ENOTSUP
    if pool:
        assert getattr(lib, quartet + "_supported")(C.byref(g)) == 1
        assert getattr(lib, quartet + "_fwd")(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), pool, be.stream) == ENOTSUP
    else:
        assert getattr(lib, quartet + "_supported")(C.byref(g)) == 0
        assert int(getattr(lib, quartet + "_table_bytes")(C.byref(g))) == 0
        assert getattr(lib, quartet + "_pack")(C.byref(g), be.ptr(f), be.ptr(f), None, be.ptr(buf), be.stream) == ENOTSUP
        for p in (0, 1):
            assert getattr(lib, quartet + "_fwd")(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), p, be.stream) == ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_invalid(be, quartet="mn_bitconv_mfma", k=1):
    """Null, misaligned (the table at 4-byte but not 16-byte alignment) and an invalid geometry are MN_EINVAL and write nothing."""
    EINVAL = _lib().MN_EINVAL
    pad = (k - 1) // 2
    g = be.geom((1, 32, 8, 8), (32, 32, k, k), padding=pad)
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    odd = C.c_void_p(be.ptr(buf).value + 2)
    off4 = C.c_void_p(be.ptr(buf).value + 4)
    assert be.ptr(buf).value % 16 == 0
    lib = be.lib
    pack, fwd = getattr(lib, quartet + "_pack"), getattr(lib, quartet + "_fwd")
    assert pack(C.byref(g), None, be.ptr(f), None, be.ptr(buf), be.stream) == EINVAL
    assert pack(C.byref(g), be.ptr(f), be.ptr(f), None, None, be.stream) == EINVAL
    assert pack(C.byref(g), be.ptr(f), be.ptr(f), None, off4, be.stream) == EINVAL
    assert fwd(C.byref(g), None, be.ptr(buf), be.ptr(buf), 0, be.stream) == EINVAL
    assert fwd(C.byref(g), off4, be.ptr(buf), be.ptr(buf), 0, be.stream) == EINVAL
    assert fwd(C.byref(g), be.ptr(buf), None, be.ptr(buf), 0, be.stream) == EINVAL
    assert fwd(C.byref(g), be.ptr(buf), be.ptr(buf), None, 0, be.stream) == EINVAL
    assert fwd(C.byref(g), be.ptr(buf), odd, be.ptr(buf), 0, be.stream) == EINVAL
    assert fwd(C.byref(g), be.ptr(buf), be.ptr(buf), odd, 0, be.stream) == EINVAL
    g0 = be.geom((0, 32, 8, 8), (32, 32, k, k), padding=pad)
    assert getattr(lib, quartet + "_supported")(C.byref(g0)) == 0 and int(getattr(lib, quartet + "_table_bytes")(C.byref(g0))) == 0
    assert pack(C.byref(g0), be.ptr(f), be.ptr(f), None, be.ptr(buf), be.stream) == EINVAL
    assert fwd(C.byref(g0), be.ptr(buf), be.ptr(buf), be.ptr(buf), 0, be.stream) == EINVAL
    if k == 1:
        godd = be.geom((1, 32, 7, 8), (32, 32, 1, 1))
        assert lib.mn_bitconv_mfma_supported(C.byref(godd)) == 1
        assert fwd(C.byref(godd), be.ptr(buf), be.ptr(buf), be.ptr(buf), 1, be.stream) == EINVAL          # the folded 2x2 pool needs even H and W
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all()


def check_counters(be, quartet="mn_bitconv_mfma", k=1, seed=5):
    """A bad out_order entry is counted into word 0 of the table and its bit stays 0; every other position carries its channel's decision."""
    pad = (k - 1) // 2
    x_shape, w_shape = (1, 32, 4, 4), (32, 32, k, k)
    _, x_log, w, b, a_ref = make_inputs(x_shape, w_shape, 1, 0, pad, seed, 3)
    g = be.geom(x_shape, w_shape, padding=pad)
    hdr = _host_u32(be, pack_table(be, quartet, g, w, b))
    assert int(hdr[0]) == 0 and int(hdr[4]) == 32
    order = np.arange(w_shape[0])
    order[3] = w_shape[0]
    table = pack_table(be, quartet, g, w, b, order)
    assert int(_host_u32(be, table)[0]) == 1
    xb = _dev_i32(be, np_pack(x_log).view(np.int32))
    yb = _empty_i32(be, (1, 1, 4, 4))
    be.call(quartet + "_fwd", C.byref(g), be.ptr(table), be.ptr(xb), be.ptr(yb), 0, be.stream)
    words = _host_u32(be, yb)
    assert not ((words >> np.uint32(3)) & 1).any(), "the bit of the bad entry stays 0"
    got = np_unpack(words, 32)
    ref = a_ref.copy()
    ref[:, 3] = -1
    assert np.array_equal(got, ref)
