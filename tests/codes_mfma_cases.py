"""The int8-MFMA form of the 1x1 hidden code block (csrc/qgemm_codes_mfma.h: mn_codeconv_mfma_*) through the C ABI: one case table for the CPU emulation build and the
GPU.  Every comparison is exact.

The judge of a block is that of tests/codes_cases.py -- an int64 numpy convolution gives acc, the library's mn_qa_fwd(stash = acc) gives codes, the numpy fp32 chain is
replayed step by step, the two must agree and the kernel must equal both -- with the constants of ``make_chan``.  Beside that the planes must equal mn_codeconv_fwd's
word for word on the same inputs and order.  mn_qa_fwd wants H * W % 8 == 0 (pooled: W % 8 == 0); on a smaller map the same accumulator values are handed to it
re-arranged (``judge_any``): the chain is element-wise and the pool acts on 2x2 windows, which the re-arrangement keeps whole."""
import ctypes as C
import math

import numpy as np

import codes_cases as CC
from bits_cases import _dev_i32, _empty_i32, _host_u32
from codes_cases import make_chan, make_inputs, np_pack_planes, np_unpack_planes, shuffle_order

F = np.float32
A_BITS = W_BITS = 2
K_BOUND_C = 3640          # C * 9 <= 32767

# (id, x shape, w shape, groups, out_order shuffle, pool, seed)
BLOCKS = [
    ("nin_gc_l2", (2, 256, 8, 8), (256, 128, 1, 1), 2, 2, 0, 3100),             # two k-steps, 16 + 16 rows per word
    ("eight_per_group_pool", (1, 512, 4, 8), (512, 128, 1, 1), 4, 4, 1, 3101),   # 8 rows per group per word, fewer pooled pixels than one tile
    ("partial_words", (3, 40, 6, 10), (33, 40, 1, 1), 1, 0, 0, 3102),            # partial input word, K padded to 64, partial output word, pixel remainder
    ("two_and_a_half_steps", (1, 320, 4, 4), (64, 160, 1, 1), 2, 0, 1, 3103),    # 2.5 k-steps, the second group starts at word 5
    ("half_a_step", (1, 128, 8, 8), (64, 32, 1, 1), 4, 0, 0, 3104),              # half a k-step, two groups per output word
    ("dead_rows", (1, 64, 4, 8), (48, 32, 1, 1), 2, 0, 0, 3105),                 # 24 rows per group: dead rows
]
# Several sets per block (tests/deploy_grid.py): the smallest shapes at which a block of k_codeconv_mfma walks set0 .. set1 over more than one set.  Seven sets over
# bx = 344 (pooled: 22016 pooled pixels / 64): four blocks of two, the last takes one.  GPU only (tests/test_gpu_codes_mfma.py): 70 s and 52 s on the CPU
# emulation build (8 cores).
LARGE_GRID = [
    ("seven_sets", (86, 64, 32, 32), (448, 32, 1, 1), 2, 2, 0, 3110),
    ("seven_sets_pool_partial", (86, 64, 32, 32), (400, 32, 1, 1), 2, 4, 1, 3111),          # 13 words: the last set is half a set, its last word half a word
]
FILL_X, FILL_W, FILL_EXTREME = (1, K_BOUND_C, 2, 2), (32, K_BOUND_C, 1, 1), 32760          # the K bound: every code 3 against every weight code 3 / 0

# (geometry keywords, (a_bits_in, w_bits, a_bits_out), pool)
REFUSED = [
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1), (2, 2, 2), 0),                # a 3x3: k_codeconv keeps it
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), (2, 2, 2), 0),                # a 5x5: the tile kernel keeps it
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1), stride=2), (2, 2, 2), 0),                 # stride 2
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1), padding=1), (2, 2, 2), 0),                # padding 1
    (dict(x_shape=(1, 64, 8, 8), w_shape=(64, 16, 1, 1), groups=4), (2, 2, 2), 0),                 # 16 channels per group: stays on k_codeconv
    (dict(x_shape=(1, 3641, 2, 2), w_shape=(32, 3641, 1, 1)), (2, 2, 2), 0),                       # beyond the K bound
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (3, 2, 2), 0),                           # 3-bit input codes
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (2, 4, 2), 0),                           # 4-bit weights
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (2, 2, 3), 0),                           # 3-bit output codes
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (2, 2, 2), 2),                           # the 3x3 / 2 pool is not folded
]


def _lib():
    from micronet_amd import _lib as L
    return L


def judge_any(be, acc, chan, pool):
    """``codes_cases.judge`` on any map size (see the module docstring); the numpy chain on the accumulator as it is must agree."""
    N, Oc, H, W = acc.shape
    if pool and W % 8:
        nwin = (H // 2) * (W // 2)
        a = acc.reshape(N, Oc, H // 2, 2, W // 2, 2).transpose(0, 1, 3, 2, 4, 5).reshape(N, Oc, 2, 2 * nwin)          # window i = columns 2 i, 2 i + 1 of two rows
        reps = 8 // math.gcd(2 * nwin, 8)
        ref = CC.judge(be, np.ascontiguousarray(np.tile(a, (1, 1, 1, reps))), chan, 1)[:, :, 0, :nwin].reshape(N, Oc, H // 2, W // 2)
    elif not pool and (H * W) % 8:
        reps = 8 // math.gcd(H * W, 8)
        ref = CC.judge(be, np.ascontiguousarray(np.tile(acc.reshape(N, Oc, 1, H * W), (1, 1, 1, reps))), chan, 0)[:, :, 0, :H * W].reshape(N, Oc, H, W)
    else:
        ref = CC.judge(be, acc, chan, pool)
    assert np.array_equal(ref, CC.chain_codes(acc, chan, pool)), "the numpy chain on the accumulator itself"
    return ref


def pack_mfma_table(be, g, w, chan, order=None):
    nb = int(be.lib.mn_codeconv_mfma_table_bytes(C.byref(g), A_BITS, W_BITS, A_BITS))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    dW, dC = be.to_dev(w), be.to_dev(chan)
    be.call("mn_codeconv_mfma_pack", C.byref(g), be.ptr(dW), be.ptr(dC), A_BITS, W_BITS, A_BITS, be.ptr(dO), be.ptr(table), be.stream)
    return table


def mfma_planes(be, codes, w, chan, groups, order=None, pool=0):
    """Pack the table and the planes, run mn_codeconv_mfma_fwd TWICE into poisoned buffers; returns (output planes as host uint32, kernel name)."""
    g = be.geom(codes.shape, w.shape, groups=groups)
    assert be.lib.mn_codeconv_mfma_supported(C.byref(g), A_BITS, W_BITS, A_BITS) == 1, "geometry must be covered by the MFMA code kernel"
    table = pack_mfma_table(be, g, w, chan, order)
    hdr = _host_u32(be, table)
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0, "finite constants, weights on the grid, a valid order"
    assert int(hdr[6]) == (2 | 2 << 8 | 2 << 16)
    xp = _dev_i32(be, np_pack_planes(codes).view(np.int32))
    N, _, H, Wd = codes.shape
    Ho, Wo = (H // 2, Wd // 2) if pool else (H, Wd)
    outs = []
    for _ in range(2):
        yp = _empty_i32(be, (N, (w.shape[0] + 31) // 32, A_BITS, Ho, Wo))          # poisoned
        be.call("mn_codeconv_mfma_fwd", C.byref(g), be.ptr(table), be.ptr(xp), be.ptr(yp), int(pool), be.stream)
        outs.append(_host_u32(be, yp))
    name = be.lib.mn_last_kernel().decode()
    assert np.array_equal(outs[0], outs[1]), "two runs give identical planes"
    Oc = w.shape[0]
    if Oc % 32:
        assert not (outs[0][:, -1] >> np.uint32(Oc % 32)).any(), "unused bits of the last output group are 0"
    return outs[0], name


def _against_both(be, codes, w, chan, groups, order, pool, ref, what):
    Oc = w.shape[0]
    planes, name = mfma_planes(be, codes, w, chan, groups, order, pool)
    got = np_unpack_planes(planes, Oc)
    want = ref[:, order] if order is not None else ref
    popc = _host_u32(be, CC.codeconv_planes(be, codes, w, chan, groups, 0, order, pool))          # mn_codeconv_fwd on the same inputs and order
    print(name, what, "mismatches against the judge", int((got != want).sum()), "of", got.size, "; words unlike mn_codeconv_fwd's", int((planes != popc).sum()))
    assert name == "k_codeconv_mfma<%d>" % pool, name
    assert got.shape == want.shape and np.array_equal(got, want), (int((got != want).sum()), got.size)
    assert planes.shape == popc.shape and np.array_equal(planes, popc), "the planes of mn_codeconv_fwd, word for word"


def check_large(be, case):
    """One LARGE_GRID case: the library's own launch rule says that a block takes at least two sets and the last block fewer; then check_block -- the judge and
    mn_codeconv_fwd's planes."""
    import deploy_grid as DG
    _, (N, _, H, Wd), w_shape, _, _, pool, _ = LARGE_GRID[case]
    bx = DG.pixel_blocks(N * (H // 2) * (Wd // 2), 64) if pool else DG.pixel_blocks(N * H * Wd, 256)
    DG.assert_uneven_deal(be, bx, ((w_shape[0] + 31) // 32 + 1) // 2)          # a set: the rows of two consecutive output words
    check_block(be, case, LARGE_GRID)


def check_block(be, case, table=None):
    _, x_shape, w_shape, groups, s, pool, seed = (BLOCKS if table is None else table)[case]
    codes, w, acc = make_inputs(x_shape, w_shape, groups, 0, seed)
    chan = make_chan(acc, seed)
    ref = judge_any(be, acc, chan, pool)
    assert len(np.unique(ref)) == 4, "the case must produce all four codes"
    full = CC.chain_codes(acc, chan, 0)
    assert (full[:, 1] == 0).all() and (full[:, 2] == CC.N_LEVELS).all() and len(np.unique(full[:, 0])) == 1
    assert (acc[:, 4] == int(chan[2, 4])).any() and (acc[:, 5] == int(chan[2, 5])).any(), "a code boundary sits on an attained accumulator value"
    order = shuffle_order(w_shape[0], s) if s else None
    _against_both(be, codes, w, chan, groups, order, pool, ref, "%s %s groups %d shuffle %d pool %d" % (x_shape, w_shape, groups, s, pool))


def check_fill(be, kcode):
    """All codes 3 against all weight codes ``kcode`` (3: acc = +9 per channel, 0: -9) at the K bound: acc = +-32760 is attained."""
    codes = np.full(FILL_X, 3, dtype=np.uint8)
    k = np.full(FILL_W, kcode, dtype=np.int64)
    w = (F(2) * (k.astype(F) / F(3)) - F(1)).astype(F)
    acc = CC.O.conv2d_fwd(codes.astype(np.int64), 2 * k - 3, None, padding=0, groups=1, acc=np.int64)
    sign = 1 if kcode == 3 else -1
    assert int(acc.max() if sign > 0 else acc.min()) == sign * FILL_EXTREME and np.abs(acc).max() <= 32767
    chan = make_chan(acc, 3200)
    ref = judge_any(be, acc, chan, 0)
    _against_both(be, codes, w, chan, 1, None, 0, ref, "%s fill %d extreme acc %d" % (FILL_X, kcode, sign * FILL_EXTREME))


def check_refused(be, case):
    kw, (ai, wb, ao), pool = REFUSED[case]
    g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), groups=kw.get("groups", 1))
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    if pool > 1:
        assert be.lib.mn_codeconv_mfma_supported(C.byref(g), ai, wb, ao) == 1
        assert be.lib.mn_codeconv_mfma_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), pool, be.stream) == _lib().MN_ENOTSUP
    else:
        assert be.lib.mn_codeconv_mfma_supported(C.byref(g), ai, wb, ao) == 0
        assert int(be.lib.mn_codeconv_mfma_table_bytes(C.byref(g), ai, wb, ao)) == 0
        rc = be.lib.mn_codeconv_mfma_pack(C.byref(g), be.ptr(f), be.ptr(f), ai, wb, ao, None, be.ptr(buf), be.stream)
        assert rc == _lib().MN_ENOTSUP, rc
        if (ai, wb, ao) == (2, 2, 2):
            for p in (0, 1):
                assert be.lib.mn_codeconv_mfma_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), p, be.stream) == _lib().MN_ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_invalid(be):
    """Null, misaligned, an invalid geometry and odd H with pool are MN_EINVAL and write nothing."""
    EINVAL = _lib().MN_EINVAL
    g = be.geom((1, 32, 8, 8), (32, 32, 1, 1))
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    odd = C.c_void_p(be.ptr(buf).value + 2)
    lib = be.lib
    assert lib.mn_codeconv_mfma_pack(C.byref(g), None, be.ptr(f), 2, 2, 2, None, be.ptr(buf), be.stream) == EINVAL
    assert lib.mn_codeconv_mfma_pack(C.byref(g), be.ptr(f), None, 2, 2, 2, None, be.ptr(buf), be.stream) == EINVAL
    assert lib.mn_codeconv_mfma_pack(C.byref(g), be.ptr(f), be.ptr(f), 2, 2, 2, None, None, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma_pack(C.byref(g), be.ptr(f), be.ptr(f), 2, 2, 2, None, odd, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma_fwd(C.byref(g), None, be.ptr(buf), be.ptr(buf), 0, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma_fwd(C.byref(g), be.ptr(buf), None, be.ptr(buf), 0, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), None, 0, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma_fwd(C.byref(g), be.ptr(buf), odd, be.ptr(buf), 0, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), odd, 0, be.stream) == EINVAL
    g0 = be.geom((0, 32, 8, 8), (32, 32, 1, 1))
    assert lib.mn_codeconv_mfma_supported(C.byref(g0), 2, 2, 2) == 0 and int(lib.mn_codeconv_mfma_table_bytes(C.byref(g0), 2, 2, 2)) == 0
    assert lib.mn_codeconv_mfma_pack(C.byref(g0), be.ptr(f), be.ptr(f), 2, 2, 2, None, be.ptr(buf), be.stream) == EINVAL
    assert lib.mn_codeconv_mfma_fwd(C.byref(g0), be.ptr(buf), be.ptr(buf), be.ptr(buf), 0, be.stream) == EINVAL
    godd = be.geom((1, 32, 7, 8), (32, 32, 1, 1))
    assert lib.mn_codeconv_mfma_supported(C.byref(godd), 2, 2, 2) == 1
    assert lib.mn_codeconv_mfma_fwd(C.byref(godd), be.ptr(buf), be.ptr(buf), be.ptr(buf), 1, be.stream) == EINVAL
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all()


def check_counters(be, seed=5):
    """Non-finite channel constants are counted into word 0 of the table, a weight off the grid (and a bad out_order entry) into word 7; word 6 carries the widths."""
    x_shape, w_shape = (1, 32, 4, 4), (32, 32, 1, 1)
    codes, w, acc = make_inputs(x_shape, w_shape, 1, 0, seed)
    chan = make_chan(acc, seed)
    g = be.geom(x_shape, w_shape)
    hdr = _host_u32(be, pack_mfma_table(be, g, w, chan))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0
    assert (int(hdr[1]), int(hdr[4]), int(hdr[5])) == (1, 32, 1) and int(hdr[6]) == (2 | 2 << 8 | 2 << 16)
    bad = chan.copy()
    bad[0, 7], bad[4, 9], bad[3, 11] = F(np.inf), F(np.nan), F(2e9)
    hdr = _host_u32(be, pack_mfma_table(be, g, w, bad))
    assert int(hdr[0]) == 3 and int(hdr[7]) == 0
    w2 = w.copy()
    w2[5, 0, 0, 0] = F(0.5)
    hdr = _host_u32(be, pack_mfma_table(be, g, w2, chan))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 1
    order = np.arange(w_shape[0])
    order[3] = w_shape[0]
    table = pack_mfma_table(be, g, w, chan, order)
    assert int(_host_u32(be, table)[7]) == 1
    # the position of the bad entry yields 0 bits, every other position its channel's code
    xp = _dev_i32(be, np_pack_planes(codes).view(np.int32))
    yp = _empty_i32(be, (1, 1, A_BITS, 4, 4))
    be.call("mn_codeconv_mfma_fwd", C.byref(g), be.ptr(table), be.ptr(xp), be.ptr(yp), 0, be.stream)
    got = np_unpack_planes(_host_u32(be, yp), 32)
    ref = judge_any(be, acc, chan, 0)
    ref[:, 3] = 0
    assert np.array_equal(got, ref)
