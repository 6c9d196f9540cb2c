"""Code-packed deployment kernels of the k-bit (DoReFa W2A2) blocks (csrc/qgemm_codes.h: mn_codes_* / mn_codeconv_*) through the C ABI: the same checks on the CPU
emulation build and on the GPU.  Every comparison is exact -- accumulators and codes are integers.

The judge of a block is not the code under test: (1) an exact integer convolution in numpy (int64) gives acc, (2) the library's streaming forward
``mn_qa_fwd(in_f32 = 0, stash = acc as int16, chan, pool)`` turns acc into codes; beside that the qa_eval -> relu -> DoReFa code chain is replayed step by step in numpy
float32 (as kernel_cases.check_qa_thresholds does).  The new kernel's unpacked output must equal both."""
import ctypes as C

import numpy as np

from oracle import np_oracle as O
from bits_cases import _dev_i32, _empty_i32, _host_u32

F = np.float32
A_BITS = W_BITS = 2
N_LEVELS = 3          # 2^2 - 1: largest activation code, and n of the weight grid (2k - n) / n


# ---------------------------------------------------------------------------------------------- planes
def np_pack_planes(codes, a_bits=A_BITS):
    """[N, C, H, W] codes -> uint32 [N, ceil(C/32), a_bits, H, W]: bit c & 31 of plane p in word group c >> 5 is bit p of the code; unused bits 0."""
    N, Cc, H, W = codes.shape
    out = np.zeros((N, (Cc + 31) // 32, a_bits, H, W), dtype=np.uint32)
    for c in range(Cc):
        for p in range(a_bits):
            out[:, c >> 5, p] |= ((codes[:, c].astype(np.uint32) >> np.uint32(p)) & np.uint32(1)) << np.uint32(c & 31)
    return out


def np_unpack_planes(planes, Cc):
    a_bits = planes.shape[2]
    out = np.zeros((planes.shape[0], Cc) + planes.shape[3:], dtype=np.uint8)
    for c in range(Cc):
        for p in range(a_bits):
            out[:, c] |= (((planes[:, c >> 5, p] >> np.uint32(c & 31)) & np.uint32(1)) << np.uint32(p)).astype(np.uint8)
    return out


def pack(be, codes, a_bits=A_BITS):
    N, Cc, H, W = codes.shape
    planes = _empty_i32(be, (N, (Cc + 31) // 32, a_bits, H, W))          # poisoned
    be.call("mn_codes_pack_planes", be.ptr(be.to_dev_u8(codes)), N, Cc, H * W, a_bits, be.ptr(planes), be.stream)
    return planes


def unpack(be, planes, Cc):
    N, _, a_bits, H, W = planes.shape
    out = be.to_dev_u8(np.full((N, Cc, H, W), 0xee, dtype=np.uint8))          # poisoned
    be.call("mn_codes_unpack_planes", be.ptr(planes), N, Cc, H * W, a_bits, be.ptr(out), be.stream)
    return be.to_host(out).view(np.uint8)


def check_pack_roundtrip(be, Cc, seed=0):
    r = np.random.default_rng(seed)
    codes = r.integers(0, 4, size=(3, Cc, 4, 12)).astype(np.uint8)
    planes = pack(be, codes)
    got = _host_u32(be, planes)
    assert np.array_equal(got, np_pack_planes(codes)), "plane layout (every word of the poisoned buffer overwritten, zero tail bits of the last group)"
    if Cc % 32:
        assert not (got[:, -1] >> np.uint32(Cc % 32)).any()
    back = unpack(be, planes, Cc)
    assert np.array_equal(back, codes), "every byte of the poisoned buffer overwritten with the code"
    # a code above 2^a - 1 in the input is masked, not propagated
    wild = codes | (r.integers(0, 64, size=codes.shape).astype(np.uint8) << 2).astype(np.uint8)
    assert np.array_equal(_host_u32(be, pack(be, wild)), np_pack_planes(codes))


# ---------------------------------------------------------------------------------------------- one block
def make_inputs(x_shape, w_shape, groups=1, padding=0, seed=0, conv=None, **_):
    """(codes uint8 [N, C, H, W] in 0..3, stored weights fp32 on the grid (2k - 3) / 3, exact accumulator int64 [N, O, H, W]).  conv: another exact integer
    convolution (x, k, padding, groups) for the sizes at which np_oracle's int64 one is too slow (deploy_grid.exact_conv)."""
    r = np.random.default_rng(seed)
    codes = r.integers(0, 4, size=x_shape).astype(np.uint8)
    codes[:, :, 0, 0] = 0                                            # whole-zero pixels and a saturated one
    codes[0, :, -1, -1] = N_LEVELS
    k = r.integers(0, 4, size=w_shape).astype(np.int64)
    w = (F(2) * (k.astype(F) / F(N_LEVELS)) - F(1)).astype(F)       # what the DoReFa weight quantizer stores
    if conv is None:
        acc = O.conv2d_fwd(codes.astype(np.int64), 2 * k - N_LEVELS, None, padding=padding, groups=groups, acc=np.int64)
    else:
        acc = conv(codes.astype(np.int64), 2 * k - N_LEVELS, padding, groups)
    assert np.abs(acc).max() <= 32767
    return codes, w, acc


def make_chan(acc, seed=0, special=True):
    """[9][O] block constants (qact_kernels.hip: alpha, bias, mean, invstd, gamma, beta, A, B, gi) around the accumulator's own spread, so that all four codes
    occur; both signs of gamma.  special: channel 0 gamma = 0, channel 1 never reaches code 1, channel 2 always code 3, channel 3 gamma < 0 for certain, channel 4 a
    code boundary exactly on an attained accumulator value, channel 5 decreasing AND its boundary on an attained value."""
    r = np.random.default_rng(seed + 77)
    Oc = acc.shape[1]
    alpha = np.full(Oc, F(1) / F(3) * (F(1) / F(3)), dtype=F)        # weight scale x activation scale of a W2A2 block
    bias = (r.standard_normal(Oc) * 0.1).astype(F)
    y = acc.astype(np.float64) * float(alpha[0])
    mean = (y.mean(axis=(0, 2, 3)) + r.standard_normal(Oc) * 0.3).astype(F)
    invstd = (1.0 / (y.std(axis=(0, 2, 3)) + 0.5)).astype(F)
    ga = (r.standard_normal(Oc) * 4).astype(F)
    be = (r.standard_normal(Oc) * 2 + 4).astype(F)
    if special:
        assert Oc >= 6
        ga[0], be[0] = F(0), F(5)
        ga[1], be[1] = F(1e-6), F(-1e4)
        ga[2], be[2] = F(1e-6), F(1e4)
        ga[3] = -abs(ga[3]) - F(0.5)
        for c, sg in ((4, 1.0), (5, -1.0)):
            # z = +-5 (acc - v0) + 5: acc = v0 gives 0.1 z = 0.5, c / s = 1.5 -- the rounding boundary between codes 1 and 2 sits ON the attained value v0
            v0 = int(np.sort(acc[:, c].ravel())[acc[:, c].size // 2])          # an attained value near the middle
            alpha[c], bias[c], invstd[c], ga[c] = F(1), F(0), F(1), F(5 * sg)
            mean[c], be[c] = F(v0), F(5)
    return np.stack([alpha, bias, mean, invstd, ga, be, alpha * invstd, (bias - mean) * invstd, ga * invstd]).astype(F)


def chain_codes(acc, chan, pool):
    """The element-wise fp32 chain of k_qa_fwd in numpy, step by step."""
    alpha, bias, mean, invstd, ga, beb = (chan[i].reshape(1, -1, 1, 1) for i in range(6))
    v = acc.astype(F)
    y = (v * alpha).astype(F) + bias
    zh = ((y - mean).astype(F) * invstd).astype(F)
    z = ((zh * ga).astype(F) + beb).astype(F)
    a = np.where(z > 0, z, F(0)).astype(F)
    if pool:
        N, Cc, H, W = a.shape
        a = a.reshape(N, Cc, H // 2, 2, W // 2, 2).max(axis=(3, 5))
    c = np.minimum(np.maximum((a * F(0.1)).astype(F), F(0)), F(1)).astype(F)
    s32 = F(1.0) / F(N_LEVELS)
    return np.floor(((c / s32).astype(F) + F(0.5)).astype(F)).astype(np.uint8)


def qa_fwd_codes(be, acc, chan, pool):
    """The library's own streaming forward on the int16 stash."""
    N, Oc, H, W = acc.shape
    shape = (N, Oc, H // 2, W // 2) if pool else (N, Oc, H, W)
    dS, dC = be.to_dev_i16(acc.astype(np.int16)), be.to_dev(chan)
    out = be.to_dev_u8(np.full(shape, 0xee, dtype=np.uint8))
    be.call("mn_qa_fwd", 0, be.ptr(dS), be.ptr(dC), N, Oc, H, W, A_BITS, int(pool), be.ptr(out), None, be.stream)
    return be.to_host(out).view(np.uint8)


def judge(be, acc, chan, pool):
    ref = qa_fwd_codes(be, acc, chan, pool)
    chain = chain_codes(acc, chan, pool)
    assert np.array_equal(ref, chain), "the two judges disagree: mn_qa_fwd vs the numpy chain"
    return ref


def pack_table(be, g, w, chan, order=None):
    nb = int(be.lib.mn_codeconv_table_bytes(C.byref(g), A_BITS, W_BITS, A_BITS))
    assert nb > 0 and nb % 4 == 0
    table = _empty_i32(be, (nb // 4,))
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    dW, dC = be.to_dev(w), be.to_dev(chan)
    be.call("mn_codeconv_pack", C.byref(g), be.ptr(dW), be.ptr(dC), A_BITS, W_BITS, A_BITS, be.ptr(dO), be.ptr(table), be.stream)
    return table


def codeconv_planes(be, codes, w, chan, groups, padding, order=None, pool=0, planes_in=None):
    """pack the table, run mn_codeconv_fwd on the packed codes; returns the output planes (device buffer)."""
    g = be.geom(codes.shape, w.shape, padding=padding, groups=groups)
    assert be.lib.mn_codeconv_supported(C.byref(g), A_BITS, W_BITS, A_BITS) == 1, "geometry must be covered by the code kernels"
    table = pack_table(be, g, w, chan, order)
    hdr = _host_u32(be, table)
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0, "finite constants, weights on the grid, a valid order"
    xp = pack(be, codes) if planes_in is None else planes_in
    N, _, H, Wd = codes.shape
    Ho, Wo = (H // 2, Wd // 2) if pool else (H, Wd)
    yp = _empty_i32(be, (N, (w.shape[0] + 31) // 32, A_BITS, Ho, Wo))          # poisoned
    be.call("mn_codeconv_fwd", C.byref(g), be.ptr(table), be.ptr(xp), be.ptr(yp), int(pool), be.stream)
    return yp


def codeconv(be, codes, w, chan, groups, padding, order=None, pool=0):
    yp = codeconv_planes(be, codes, w, chan, groups, padding, order, pool)
    Oc = w.shape[0]
    if Oc % 32:
        assert not (_host_u32(be, yp)[:, -1] >> np.uint32(Oc % 32)).any(), "unused bits of the last output group are 0"
    return unpack(be, yp, Oc)


def shuffle_order(Oc, s):
    """what a consumer with in_shuffle_groups = s reads at position j (models/nin_gc.py:4-15)"""
    j = np.arange(Oc)
    return (j % s) * (Oc // s) + j // s


def check_codeconv(be, x_shape, w_shape, groups=1, padding=0, seed=0, pools=(0, 1), shuffles=(), **_):
    """The block on the case's geometry: not pooled and pooled, identity order and every consumer shuffle of ``shuffles``, against the judge."""
    codes, w, acc = make_inputs(x_shape, w_shape, groups, padding, seed)
    chan = make_chan(acc, seed)
    Oc = w_shape[0]
    for pool in pools:
        ref = judge(be, acc, chan, pool)
        assert len(np.unique(ref)) == 4, "the case must produce all four codes"
        for s in (0,) + tuple(shuffles):
            order = shuffle_order(Oc, s) if s else None
            got = codeconv(be, codes, w, chan, groups, padding, order=order, pool=pool)
            want = ref[:, order] if s else ref
            print("codeconv", x_shape, w_shape, "groups", groups, "pool", pool, "shuffle", s, "mismatches", int((got != want).sum()), "of", got.size)
            assert np.array_equal(got, want), (pool, s, int((got != want).sum()), got.size)
        # the special channels did what they are there for
        full = chain_codes(acc, chan, 0)
        assert (full[:, 1] == 0).all() and (full[:, 2] == N_LEVELS).all() and len(np.unique(full[:, 0])) == 1
    v0 = chan[2, 4]
    assert (acc[:, 4] == int(v0)).any() and (acc[:, 5] == int(chan[2, 5])).any(), "a code boundary sits on an attained accumulator value"


# Several output words per block (tests/deploy_grid.py): the smallest shapes at which a block of k_codeconv walks ow0 .. ow1 over more than one word group.  Seven
# groups over bx = 344: four blocks of two, the last takes one.  (id, check_codeconv keywords, out_order shuffle, kernel).  Wall time of the whole case on the CPU
# emulation build (8 cores, judge included) beside each: below 20 s, so tests/test_codes_emulated.py runs the table as well as tests/test_gpu_codes.py.
LARGE_GRID = [
    ("k1", dict(x_shape=(86, 32, 32, 32), w_shape=(224, 32, 1, 1), seed=1500), 4, "k_codeconv<1,1,0>"),          # emulated: 9 s
    ("k3_grouped_partial_word", dict(x_shape=(86, 32, 32, 32), w_shape=(200, 16, 3, 3), groups=2, padding=1, seed=1501), 4, "k_codeconv<3,1,0>"),          # O % 32 = 8.  17 s
]


def check_large(be, idx):
    """One LARGE_GRID case: the library's own launch rule says that a block takes at least two word groups and the last block fewer; then the un-pooled block in the
    consumer's order, twice into poisoned planes, against the judge."""
    import deploy_grid as DG
    cid, kw, s, kernel = LARGE_GRID[idx]
    x_shape, w_shape, groups, padding, seed = kw["x_shape"], kw["w_shape"], kw.get("groups", 1), kw.get("padding", 0), kw["seed"]
    N, _, H, Wd = x_shape
    Oc = w_shape[0]
    gy, per = DG.assert_uneven_deal(be, DG.pixel_blocks(N * H * Wd, 256), (Oc + 31) // 32)
    codes, w, acc = make_inputs(x_shape, w_shape, groups, padding, seed)
    chan = make_chan(acc, seed)
    ref = judge(be, acc, chan, 0)
    assert len(np.unique(ref)) == 4, "the case must produce all four codes"
    full = chain_codes(acc, chan, 0)
    assert (full[:, 1] == 0).all() and (full[:, 2] == N_LEVELS).all() and len(np.unique(full[:, 0])) == 1
    assert (acc[:, 4] == int(chan[2, 4])).any() and (acc[:, 5] == int(chan[2, 5])).any(), "a code boundary sits on an attained accumulator value"
    order = shuffle_order(Oc, s)
    outs = []
    for _ in range(2):
        yp = codeconv_planes(be, codes, w, chan, groups, padding, order, 0)          # poisoned planes
        name = be.lib.mn_last_kernel().decode()
        outs.append(_host_u32(be, yp))
    assert name == kernel, name
    assert np.array_equal(outs[0], outs[1]), "two runs give identical planes"
    if Oc % 32:
        assert not (outs[0][:, -1] >> np.uint32(Oc % 32)).any(), "unused bits of the last output group are 0"
    got, want = np_unpack_planes(outs[0], Oc), ref[:, order]
    bad = int((got != want).sum())
    print(name, cid, x_shape, w_shape, "groups", groups, "shuffle", s, "grid.y", gy, "per", per, "mismatches", bad, "of", got.size)
    assert got.shape == want.shape and bad == 0, (bad, got.size)


def check_nonfinite_counted(be, x_shape=(1, 32, 4, 4), w_shape=(32, 16, 1, 1), groups=2, seed=3):
    """A row whose channel constants fail qa_finite (mn_qa_fwd's element-wise path: no threshold form) is counted into word 0 of the table."""
    codes, w, acc = make_inputs(x_shape, w_shape, groups, 0, seed)
    chan = make_chan(acc, seed)
    g = be.geom(x_shape, w_shape, padding=0, groups=groups)
    assert int(_host_u32(be, pack_table(be, g, w, chan))[0]) == 0
    bad = chan.copy()
    bad[0, 7], bad[4, 9], bad[3, 11] = F(np.inf), F(np.nan), F(2e9)
    hdr = _host_u32(be, pack_table(be, g, w, bad))
    assert int(hdr[0]) == 3 and int(hdr[7]) == 0
    # a weight off the grid and an out-of-range order entry are counted into word 7
    w2 = w.copy()
    w2[5, 0, 0, 0] = F(0.5)
    assert int(_host_u32(be, pack_table(be, g, w2, chan))[7]) == 1
    order = np.arange(w_shape[0])
    order[3] = w_shape[0]
    assert int(_host_u32(be, pack_table(be, g, w, chan, order))[7]) == 1


UNSUPPORTED = [
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), (2, 2, 2)),                  # 5x5
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=0), (2, 2, 2)),                  # 3x3 without "same" padding
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1), stride=2), (2, 2, 2)),                   # stride 2
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (3, 2, 2)),                             # 3-bit input codes
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (2, 4, 2)),                             # 4-bit weights
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (2, 2, 3)),                             # 3-bit output codes
    (dict(x_shape=(1, 4096, 8, 8), w_shape=(32, 4096, 1, 1)), (2, 2, 2)),                         # K * 9 beyond the int16 stash
]


def check_unsupported(be, case):
    kw, (ai, wb, ao) = UNSUPPORTED[case]
    g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0))
    assert be.lib.mn_codeconv_supported(C.byref(g), ai, wb, ao) == 0
    assert int(be.lib.mn_codeconv_table_bytes(C.byref(g), ai, wb, ao)) == 0
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    rc = be.lib.mn_codeconv_pack(C.byref(g), be.ptr(f), be.ptr(f), ai, wb, ao, None, be.ptr(buf), be.stream)
    assert rc == MN_ENOTSUP(be), rc
    if (ai, wb, ao) == (2, 2, 2):
        assert be.lib.mn_codeconv_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), 0, be.stream) == MN_ENOTSUP(be)
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def MN_ENOTSUP(be):
    from micronet_amd import _lib
    return _lib.MN_ENOTSUP


# ---------------------------------------------------------------------------------------------- the case table (tests/test_codes_emulated.py, tests/test_gpu_codes.py)
FORTY_PER_GROUP = dict(x_shape=(2, 80, 8, 8), w_shape=(96, 40, 1, 1), groups=2)                  # C = 80: partial last word; group 1 spans two words at an odd offset
FORTY_PER_GROUP_3X3 = dict(x_shape=(1, 160, 4, 8), w_shape=(64, 40, 3, 3), groups=4, padding=1)   # the rolled 3x3 kernel
FORTY_EIGHT_PER_GROUP = dict(x_shape=(2, 96, 8, 8), w_shape=(96, 48, 1, 1), groups=2)
ALL_BORDER_3X3 = dict(x_shape=(2, 32, 4, 4), w_shape=(64, 16, 3, 3), groups=2, padding=1, pools=(0,))          # every pixel is a border pixel (4 x 4: not poolable by mn_qa_fwd)
ALL_BORDER_3X3_POOL = dict(x_shape=(2, 32, 2, 8), w_shape=(64, 16, 3, 3), groups=2, padding=1)    # ... pooled as well (W % 8 == 0 for the judge's pooled pass)


def block_cases(full):
    """(id, check_codeconv keywords) of every block case; ``full``: the nin_gc layers with N = 2 at the net's own map size (GPU), else N = 1 on the 8 x 8 / 8 x 16 cut (the
    emulator runs one fiber per GPU thread)."""
    import bits_cases as B
    import kernel_cases as K
    cases = []
    for i in range(len(B.NIN_GC_LAYERS)):
        # (the input shuffle of a layer is its PRODUCER's row order: exercised below through ``shuffles``, on the layers that feed a shuffling consumer in the net)
        kw = {k: v for k, v in B.nin_gc_case(i, full).items() if k != "in_shuffle"}
        nxt = B.NIN_GC_LAYERS[i + 1][4] if i + 1 < len(B.NIN_GC_LAYERS) else 0
        cases.append(("nin_gc%d" % i, dict(kw, seed=1100 + i, shuffles=(nxt,) if nxt > 1 else ())))
    cases.append(("two_per_group", dict(B.TWO_PER_GROUP, seed=1200, shuffles=(2,))))
    for i, c in enumerate(K.DEPLOYED_CASES):
        if c["w_shape"][2] in (1, 3):
            cases.append(("deployed%d" % i, dict({k: v for k, v in c.items() if k != "in_shuffle"}, seed=1300 + i)))
    cases.append(("forty_per_group", dict(FORTY_PER_GROUP, seed=1400, shuffles=(2, 16))))
    cases.append(("forty_per_group_3x3", dict(FORTY_PER_GROUP_3X3, seed=1401, shuffles=(16,))))
    cases.append(("forty_eight_per_group", dict(FORTY_EIGHT_PER_GROUP, seed=1402, shuffles=(2, 16))))
    cases.append(("all_border_3x3", dict(ALL_BORDER_3X3, seed=1403)))
    cases.append(("all_border_3x3_pool", dict(ALL_BORDER_3X3_POOL, seed=1404, shuffles=(2,))))
    return cases
