"""The int8-MFMA form of the 3x3 hidden code block (csrc/qgemm_codes_mfma3.h: mn_codeconv_mfma3_*) through the C ABI: one case table for the CPU emulation build and the
GPU.  Every comparison is exact.

The judge of a block is that of tests/codes_cases.py via ``codes_mfma_cases.judge_any`` -- an int64 numpy convolution gives acc, the library's mn_qa_fwd(stash = acc)
gives codes, the numpy fp32 chain is replayed step by step, the two must agree and the kernel must equal both -- with the constants of ``make_chan``.  Beside that the
planes must equal mn_codeconv_fwd's word for word on the same inputs and order.  Buffers are poisoned and every case runs twice."""
import ctypes as C

import numpy as np

import codes_cases as CC
from bits_cases import _dev_i32, _empty_i32, _host_u32
from codes_cases import make_chan, make_inputs, np_pack_planes, np_unpack_planes, shuffle_order
from codes_mfma_cases import judge_any

F = np.float32
A_BITS = W_BITS = 2
KERNEL = "k_codeconv_mfma3<0>"

# (id, x shape, w shape, groups, out_order shuffle, header word 5 (dead rows): 0, or None for "> 0", seed)
BLOCKS = [
    ("nin_gc_l4", (2, 256, 4, 8), (512, 16, 3, 3), 16, 16, 0, 3300),          # span of 8 words, high / low half-words, interior and border pixels
    ("nin_gc_l7", (1, 512, 4, 4), (1024, 16, 3, 3), 32, 32, 0, 3301),         # span of 16 words, fewer pixels than one wave
    ("padded_last_step", (3, 48, 5, 7), (40, 48, 3, 3), 1, 0, None, 3302),    # 27 slots: a padded last k-step; partial input / output word; 105 pixels; dead rows
    ("upper_half_start", (1, 96, 4, 8), (64, 48, 3, 3), 2, 2, 0, 3303),       # the second group starts on the upper half of word 1
    ("nin_dense", (1, 192, 4, 4), (192, 192, 3, 3), 1, 0, 0, 3304),           # 27 full k-steps, 12 M tiles
    ("dead_rows", (1, 32, 8, 8), (48, 16, 3, 3), 2, 0, None, 3305),           # 24 rows per group
    ("one_row", (2, 32, 1, 8), (32, 32, 3, 3), 1, 0, 0, 3306),                # a whole tap row outside everywhere
    ("one_column", (1, 32, 8, 1), (32, 32, 3, 3), 1, 0, 0, 3307),             # a whole tap column outside everywhere
]
# Several spans per block (tests/deploy_grid.py): the smallest shapes at which a block of k_codeconv_mfma3 takes a second span (sp += gridDim.y).  Seven word groups
# in spans of two: four spans over grid.y = 3 at bx = 688 -- block 0 takes spans 0 and 3.  GPU only (tests/test_gpu_codes_mfma3.py): 134 s and 110 s on the CPU emulation build.
LARGE_GRID = [
    ("four_spans", (43, 16, 64, 64), (224, 16, 3, 3), 1, 0, 0, 3310),
    ("four_spans_shuffled_partial", (43, 16, 64, 64), (200, 16, 3, 3), 1, 4, None, 3311),          # O % 32 = 8
]
SPANS = {"nin_gc_l4": 8, "nin_gc_l7": 16, "nin_dense": 2}          # header word 2 where the issue names the span
FILL_X, FILL_W, FILL_EXTREME = (1, 400, 3, 3), (32, 400, 3, 3), 32400          # the K bound: every code 3 against every weight code 3 / 0, all nine taps at the centre

# (geometry keywords, (a_bits_in, w_bits, a_bits_out), pool)
REFUSED = [
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1), (2, 2, 2), 1),                # the pooled 3x3 block stays on k_codeconv
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (2, 2, 2), 0),                           # a 1x1: k_codeconv / k_codeconv_mfma keep it
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), (2, 2, 2), 0),                # a 5x5: the tile kernel keeps it
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=0), (2, 2, 2), 0),                # padding 0
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1, stride=2), (2, 2, 2), 0),      # stride 2
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 8, 3, 3), padding=1, groups=4), (2, 2, 2), 0),       # 8 channels per group
    (dict(x_shape=(1, 48, 8, 8), w_shape=(32, 24, 3, 3), padding=1, groups=2), (2, 2, 2), 0),      # 24 channels per group
    (dict(x_shape=(1, 401, 3, 3), w_shape=(32, 401, 3, 3), padding=1), (2, 2, 2), 0),              # 401 channels
    (dict(x_shape=(1, 416, 3, 3), w_shape=(32, 416, 3, 3), padding=1), (2, 2, 2), 0),              # on a half-word boundary, beyond the K bound
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1), (3, 2, 2), 0),                # 3-bit input codes
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1), (2, 3, 2), 0),                # 3-bit weights
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1), (2, 2, 3), 0),                # 3-bit output codes
]


def _lib():
    from micronet_amd import _lib as L
    return L


def pack_mfma3_table(be, g, w, chan, order=None):
    nb = int(be.lib.mn_codeconv_mfma3_table_bytes(C.byref(g), A_BITS, W_BITS, A_BITS))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    dW, dC = be.to_dev(w), be.to_dev(chan)
    be.call("mn_codeconv_mfma3_pack", C.byref(g), be.ptr(dW), be.ptr(dC), A_BITS, W_BITS, A_BITS, be.ptr(dO), be.ptr(table), be.stream)
    return table


def mfma3_planes(be, codes, w, chan, groups, order=None):
    """Pack the table and the planes, run mn_codeconv_mfma3_fwd TWICE into poisoned buffers; returns (output planes as host uint32, kernel name, table header)."""
    g = be.geom(codes.shape, w.shape, padding=1, groups=groups)
    assert be.lib.mn_codeconv_mfma3_supported(C.byref(g), A_BITS, W_BITS, A_BITS) == 1, "geometry must be covered by the 3x3 MFMA code kernel"
    table = pack_mfma3_table(be, g, w, chan, order)
    hdr = _host_u32(be, table)[:8].copy()
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0, "finite constants, weights on the grid, a valid order"
    assert int(hdr[6]) == (2 | 2 << 8 | 2 << 16)
    xp = _dev_i32(be, np_pack_planes(codes).view(np.int32))
    N, _, H, Wd = codes.shape
    outs = []
    for _ in range(2):
        yp = _empty_i32(be, (N, (w.shape[0] + 31) // 32, A_BITS, H, Wd))          # poisoned
        be.call("mn_codeconv_mfma3_fwd", C.byref(g), be.ptr(table), be.ptr(xp), be.ptr(yp), 0, be.stream)
        outs.append(_host_u32(be, yp))
    name = be.lib.mn_last_kernel().decode()
    assert np.array_equal(outs[0], outs[1]), "two runs give identical planes"
    Oc = w.shape[0]
    if Oc % 32:
        assert not (outs[0][:, -1] >> np.uint32(Oc % 32)).any(), "unused bits of the last output group are 0"
    return outs[0], name, hdr


def _against_both(be, codes, w, chan, groups, order, ref, what):
    Oc = w.shape[0]
    planes, name, hdr = mfma3_planes(be, codes, w, chan, groups, order)
    got = np_unpack_planes(planes, Oc)
    want = ref[:, order] if order is not None else ref
    xp = _dev_i32(be, np_pack_planes(codes).view(np.int32))          # (packed here: mn_codes_pack_planes wants H * W % 4 == 0)
    popc = _host_u32(be, CC.codeconv_planes(be, codes, w, chan, groups, 1, order, 0, planes_in=xp))          # mn_codeconv_fwd on the same inputs and order
    print(name, what, "span", int(hdr[2]), "dead rows", int(hdr[5]), "mismatches against the judge", int((got != want).sum()), "of", got.size,
          "; words unlike mn_codeconv_fwd's", int((planes != popc).sum()))
    assert name == KERNEL, name
    assert got.shape == want.shape and np.array_equal(got, want), (int((got != want).sum()), got.size)
    assert planes.shape == popc.shape and np.array_equal(planes, popc), "the planes of mn_codeconv_fwd, word for word"
    return hdr


def check_large(be, case):
    """One LARGE_GRID case: check_block -- the judge and mn_codeconv_fwd's planes; the exact accumulator comes from deploy_grid.exact_conv at this size --, and through
    the library's own launch rule and the span the packer wrote into the table (header word 2) that some block of grid.y took a second span and some block did not."""
    import deploy_grid as DG
    _, (N, _, H, Wd), w_shape, _, _, _, _ = LARGE_GRID[case]
    hdr = check_block(be, case, LARGE_GRID, DG.exact_conv)
    OW = (w_shape[0] + 31) // 32
    span = int(hdr[2])
    DG.assert_uneven_rows(be, DG.pixel_blocks(N * H * Wd, 256), (OW + 1) >> 1, (OW + span - 1) // span)


def check_block(be, case, table=None, conv=None):
    cid, x_shape, w_shape, groups, s, dead, seed = (BLOCKS if table is None else table)[case]
    codes, w, acc = make_inputs(x_shape, w_shape, groups, 1, seed, conv=conv)
    chan = make_chan(acc, seed)
    ref = judge_any(be, acc, chan, 0)
    assert len(np.unique(ref)) == 4, "the case must produce all four codes"
    full = CC.chain_codes(acc, chan, 0)
    assert (full[:, 1] == 0).all() and (full[:, 2] == CC.N_LEVELS).all() and len(np.unique(full[:, 0])) == 1
    assert (acc[:, 4] == int(chan[2, 4])).any() and (acc[:, 5] == int(chan[2, 5])).any(), "a code boundary sits on an attained accumulator value"
    order = shuffle_order(w_shape[0], s) if s else None
    hdr = _against_both(be, codes, w, chan, groups, order, ref, "%s %s groups %d shuffle %d" % (x_shape, w_shape, groups, s))
    assert (int(hdr[5]) == 0) if dead == 0 else (int(hdr[5]) > 0), ("dead rows", int(hdr[5]))
    assert int(hdr[1]) == (9 * (x_shape[1] // groups // 16) + 3) // 4 and int(hdr[4]) == 32 * ((w_shape[0] + 31) // 32)
    if cid in SPANS:
        assert int(hdr[2]) == SPANS[cid], ("span", int(hdr[2]))
    return hdr


def check_fill(be, kcode):
    """All codes 3 against all weight codes ``kcode`` (3: acc = +9 per tap and channel, 0: -9) at the K bound: the centre pixel attains acc = +-32400."""
    codes = np.full(FILL_X, 3, dtype=np.uint8)
    k = np.full(FILL_W, kcode, dtype=np.int64)
    w = (F(2) * (k.astype(F) / F(3)) - F(1)).astype(F)
    acc = CC.O.conv2d_fwd(codes.astype(np.int64), 2 * k - 3, None, padding=1, groups=1, acc=np.int64)
    sign = 1 if kcode == 3 else -1
    assert (acc[:, :, 1, 1] == sign * FILL_EXTREME).all() and np.abs(acc).max() == FILL_EXTREME
    chan = make_chan(acc, 3400)
    ref = judge_any(be, acc, chan, 0)
    _against_both(be, codes, w, chan, 1, None, ref, "%s fill %d extreme acc %d" % (FILL_X, kcode, sign * FILL_EXTREME))


def check_refused(be, case):
    kw, (ai, wb, ao), pool = REFUSED[case]
    g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), groups=kw.get("groups", 1))
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    if pool:
        assert be.lib.mn_codeconv_mfma3_supported(C.byref(g), ai, wb, ao) == 1
        assert be.lib.mn_codeconv_mfma3_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), pool, be.stream) == _lib().MN_ENOTSUP
    else:
        assert be.lib.mn_codeconv_mfma3_supported(C.byref(g), ai, wb, ao) == 0
        assert int(be.lib.mn_codeconv_mfma3_table_bytes(C.byref(g), ai, wb, ao)) == 0
        rc = be.lib.mn_codeconv_mfma3_pack(C.byref(g), be.ptr(f), be.ptr(f), ai, wb, ao, None, be.ptr(buf), be.stream)
        assert rc == _lib().MN_ENOTSUP, rc
        if (ai, wb, ao) == (2, 2, 2):
            assert be.lib.mn_codeconv_mfma3_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), 0, be.stream) == _lib().MN_ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_invalid(be):
    """Null, misaligned and an invalid geometry are MN_EINVAL and write nothing."""
    EINVAL = _lib().MN_EINVAL
    g = be.geom((1, 32, 8, 8), (32, 32, 3, 3), padding=1)
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    odd = C.c_void_p(be.ptr(buf).value + 2)
    odd8 = C.c_void_p(be.ptr(buf).value + 8)
    lib = be.lib
    assert lib.mn_codeconv_mfma3_pack(C.byref(g), None, be.ptr(f), 2, 2, 2, None, be.ptr(buf), be.stream) == EINVAL
    assert lib.mn_codeconv_mfma3_pack(C.byref(g), be.ptr(f), None, 2, 2, 2, None, be.ptr(buf), be.stream) == EINVAL
    assert lib.mn_codeconv_mfma3_pack(C.byref(g), be.ptr(f), be.ptr(f), 2, 2, 2, None, None, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma3_pack(C.byref(g), be.ptr(f), be.ptr(f), 2, 2, 2, None, odd8, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma3_fwd(C.byref(g), None, be.ptr(buf), be.ptr(buf), 0, be.stream) == EINVAL          # the null table
    assert lib.mn_codeconv_mfma3_fwd(C.byref(g), odd8, be.ptr(buf), be.ptr(buf), 0, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma3_fwd(C.byref(g), be.ptr(buf), None, be.ptr(buf), 0, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma3_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), None, 0, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma3_fwd(C.byref(g), be.ptr(buf), odd, be.ptr(buf), 0, be.stream) == EINVAL
    assert lib.mn_codeconv_mfma3_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), odd, 0, be.stream) == EINVAL
    g0 = be.geom((0, 32, 8, 8), (32, 32, 3, 3), padding=1)
    assert lib.mn_codeconv_mfma3_supported(C.byref(g0), 2, 2, 2) == 0 and int(lib.mn_codeconv_mfma3_table_bytes(C.byref(g0), 2, 2, 2)) == 0
    assert lib.mn_codeconv_mfma3_pack(C.byref(g0), be.ptr(f), be.ptr(f), 2, 2, 2, None, be.ptr(buf), be.stream) == EINVAL
    assert lib.mn_codeconv_mfma3_fwd(C.byref(g0), be.ptr(buf), be.ptr(buf), be.ptr(buf), 0, be.stream) == EINVAL
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all()


def check_counters(be, seed=5):
    """Non-finite channel constants are counted into word 0 of the table, a weight off the grid and a bad out_order entry into word 7; word 6 carries the widths."""
    x_shape, w_shape = (1, 32, 4, 4), (32, 32, 3, 3)
    codes, w, acc = make_inputs(x_shape, w_shape, 1, 1, seed)
    chan = make_chan(acc, seed)
    g = be.geom(x_shape, w_shape, padding=1)
    hdr = _host_u32(be, pack_mfma3_table(be, g, w, chan))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0
    assert (int(hdr[1]), int(hdr[2]), int(hdr[4]), int(hdr[5])) == (5, 2, 32, 0) and int(hdr[6]) == (2 | 2 << 8 | 2 << 16)
    bad = chan.copy()
    bad[0, 7], bad[4, 9], bad[3, 11] = F(np.inf), F(np.nan), F(2e9)
    hdr = _host_u32(be, pack_mfma3_table(be, g, w, bad))
    assert int(hdr[0]) == 3 and int(hdr[7]) == 0
    w2 = w.copy()
    w2[5, 17, 2, 1] = F(0.5)
    hdr = _host_u32(be, pack_mfma3_table(be, g, w2, chan))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 1
    order = np.arange(w_shape[0])
    order[3] = w_shape[0]
    table = pack_mfma3_table(be, g, w, chan, order)
    hdr = _host_u32(be, table)
    assert int(hdr[7]) == 1 and int(hdr[5]) == 1, "31 rows: the second tile is a row short"
    # the position of the bad entry yields 0 bits, every other position its channel's code
    xp = _dev_i32(be, np_pack_planes(codes).view(np.int32))
    yp = _empty_i32(be, (1, 1, A_BITS, 4, 4))
    be.call("mn_codeconv_mfma3_fwd", C.byref(g), be.ptr(table), be.ptr(xp), be.ptr(yp), 0, be.stream)
    got = np_unpack_planes(_host_u32(be, yp), 32)
    ref = judge_any(be, acc, chan, 0)
    ref[:, 3] = 0
    assert np.array_equal(got, ref)
