"""The 4-bit instantiation of the two int8-MFMA code blocks (csrc/qgemm_codes_mfma.h, csrc/qgemm_codes_mfma3.h: mn_codeconv_mfma_* / mn_codeconv_mfma3_* at
(a_bits_in, w_bits, a_bits_out) = (4, 4, 4), run through mn_codeconv_mfma_fwd_bits / mn_codeconv_mfma3_fwd_bits) through the C ABI: one case table for the CPU
emulation build and the GPU.  Every comparison is exact.

The judge is that of tests/codes_cases.py at width 4 -- an int64 numpy convolution gives acc, the library's mn_qa_fwd(a_bits = 4) on the int16 stash gives codes, the
numpy fp32 chain is replayed step by step with n = 15, the two must agree and the kernel must equal both.  There is no popcount kernel at 4 bits to compare words
against.  mn_qa_fwd wants H * W % 8 == 0 (pooled: W % 8 == 0); on a smaller map the same accumulator values are handed to it re-arranged, as
codes_mfma_cases.judge_any does.  Buffers are poisoned and every forward runs twice."""
import ctypes as C
import math

import numpy as np

from oracle import np_oracle as O
from bits_cases import _dev_i32, _empty_i32, _host_u32
from codes_cases import np_pack_planes, np_unpack_planes, shuffle_order

F = np.float32
BITS = 4
N_LEVELS = 15          # 2^4 - 1: largest activation code, and n of the weight grid (2k - n) / n
WIDTHS = (BITS, BITS, BITS)
WORD6 = 4 | 4 << 8 | 4 << 16
K_BOUND_C = 145          # C * 15 * 15 <= 32767

# (id, x shape, w shape, groups, out_order shuffle, pool, seed)
BLOCKS1 = [
    ("nin_gc_l2", (2, 256, 4, 8), (256, 128, 1, 1), 2, 2, 0, 4100),              # two k-steps
    ("eight_per_group_pool", (1, 512, 4, 8), (512, 128, 1, 1), 4, 4, 1, 4101),   # 8 rows per group per word; fewer pooled pixels than a tile
    ("partial_words", (3, 40, 6, 10), (33, 40, 1, 1), 1, 0, 0, 4102),            # partial input and output word; pixel remainder
    ("k_bound_pool", (1, 145, 4, 4), (64, 145, 1, 1), 1, 0, 1, 4103),            # the K bound: three k-steps, the last partial
    ("half_a_step", (1, 128, 8, 8), (64, 32, 1, 1), 4, 0, 0, 4104),              # half a step
    ("dead_rows", (1, 64, 4, 8), (48, 32, 1, 1), 2, 0, 0, 4105),                 # dead rows
]
# (id, x shape, w shape, groups, out_order shuffle, (span, dead rows) of the table header or None, seed); padding 1
BLOCKS3 = [
    ("nin_gc_l4", (2, 256, 4, 8), (512, 16, 3, 3), 16, 16, (8, 0), 4300),        # nin_gc's first 3x3 layer
    ("nin_gc_l7", (1, 512, 4, 4), (1024, 16, 3, 3), 32, 32, (8, 1024), 4301),    # the largest span / LDS image: 8 rows per group in 8 words, every tile half dead
    ("partial_words", (3, 16, 6, 10), (33, 16, 3, 3), 1, 0, (2, 15), 4302),      # partial output word; pixel remainder
    ("dead_rows", (1, 32, 8, 8), (48, 16, 3, 3), 2, 0, None, 4303),              # dead rows
    ("all_border", (1, 16, 2, 4), (32, 16, 3, 3), 1, 0, (2, 0), 4304),           # every pixel on the border
]
# Several units per block (tests/deploy_grid.py) at 4 bits, the shapes of codes_mfma_cases.LARGE_GRID / codes_mfma3_cases.LARGE_GRID: seven sets over bx = 344
# (four blocks of two, the last takes one); four spans of two word groups over grid.y = 3 at bx = 688 (block 0 takes spans 0 and 3).  GPU only (tests/test_gpu_codes_w4.py): 98 s,
# 52 s, 110 s and 106 s on the CPU emulation build (8 cores).
LARGE1 = [
    ("seven_sets", (86, 64, 32, 32), (448, 32, 1, 1), 2, 2, 0, 4110),
    ("seven_sets_pool_partial", (86, 64, 32, 32), (400, 32, 1, 1), 2, 4, 1, 4111),
]
LARGE3 = [
    ("four_spans", (43, 16, 64, 64), (224, 16, 3, 3), 1, 0, (2, 0), 4310),
    ("four_spans_shuffled_partial", (43, 16, 64, 64), (200, 16, 3, 3), 1, 4, None, 4311),
]
FILL1_X, FILL1_W, FILL1_EXTREME = (1, K_BOUND_C, 2, 2), (32, K_BOUND_C, 1, 1), 32625          # every code 15 against every weight code 15 / 0
FILL3_X, FILL3_W, FILL3_EXTREME = (1, 16, 4, 4), (32, 16, 3, 3), 32400                        # ... the interior pixels attain it

G1 = dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1))
G3 = dict(x_shape=(1, 16, 8, 8), w_shape=(32, 16, 3, 3), padding=1)
# (form, geometry keywords, widths, pool): refused -- supported == 0, table_bytes == 0, pack and fwd_bits MN_ENOTSUP -- except where pool != 0: supported, fwd_bits refuses
REFUSED = [
    ("mfma", dict(x_shape=(1, 146, 2, 2), w_shape=(32, 146, 1, 1)), WIDTHS, 0),                      # dense, beyond the K bound
    ("mfma", dict(x_shape=(1, 64, 8, 8), w_shape=(64, 16, 1, 1), groups=4), WIDTHS, 0),             # 16 channels per group
    ("mfma", dict(x_shape=(1, 320, 4, 4), w_shape=(64, 160, 1, 1), groups=2), WIDTHS, 0),           # whole words per group, beyond the K bound
    ("mfma3", dict(x_shape=(1, 64, 8, 8), w_shape=(32, 32, 3, 3), padding=1, groups=2), WIDTHS, 0),  # 32 channels per group: beyond the K bound
    ("mfma3", dict(x_shape=(1, 32, 8, 8), w_shape=(32, 8, 3, 3), padding=1, groups=4), WIDTHS, 0),   # 8 channels per group
    ("mfma", G1, WIDTHS, 2),                                                                         # the 3x3 / 2 pool is not folded
    ("mfma3", G3, WIDTHS, 1),                                                                        # no pool is folded into the 3x3 form
] + [(form, geo, wd, 0) for wd in ((4, 4, 2), (2, 2, 4), (4, 2, 4), (3, 3, 3), (8, 8, 8)) for form, geo in (("mfma", G1), ("mfma3", G3))]


def _lib():
    from micronet_amd import _lib as L
    return L


# ---------------------------------------------------------------------------------------------- inputs and the judge
def make_inputs(x_shape, w_shape, groups=1, padding=0, seed=0, conv=None):
    """(codes uint8 [N, C, H, W] in 0..15, stored weights fp32 on the grid (2k - 15) / 15, exact accumulator int64 [N, O, H, W]).  conv: another exact integer
    convolution (x, k, padding, groups) for the sizes at which np_oracle's int64 one is too slow (deploy_grid.exact_conv)."""
    r = np.random.default_rng(seed)
    codes = r.integers(0, N_LEVELS + 1, size=x_shape).astype(np.uint8)
    codes[:, :, 0, 0] = 0                                            # whole-zero pixels and a saturated one
    codes[0, :, -1, -1] = N_LEVELS
    k = r.integers(0, N_LEVELS + 1, size=w_shape).astype(np.int64)
    w = (F(2) * (k.astype(F) / F(N_LEVELS)) - F(1)).astype(F)       # what the DoReFa weight quantizer stores
    if conv is None:
        acc = O.conv2d_fwd(codes.astype(np.int64), 2 * k - N_LEVELS, None, padding=padding, groups=groups, acc=np.int64)
    else:
        acc = conv(codes.astype(np.int64), 2 * k - N_LEVELS, padding, groups)
    assert np.abs(acc).max() <= 32767
    return codes, w, acc


def make_chan(acc, seed=0):
    """codes_cases.make_chan for a W4A4 block: alpha = 1/15 * 1/15, the same six special channels -- channel 0 gamma = 0, channel 1 always code 0, channel 2 always code
    15, channel 3 gamma < 0 for certain, channel 4 a code boundary (7 | 8: 0.1 z = 0.5, c / s = 7.5) on an attained accumulator value, channel 5 decreasing and its
    boundary on an attained value."""
    r = np.random.default_rng(seed + 77)
    Oc = acc.shape[1]
    assert Oc >= 6
    alpha = np.full(Oc, F(1) / F(N_LEVELS) * (F(1) / F(N_LEVELS)), dtype=F)
    bias = (r.standard_normal(Oc) * 0.1).astype(F)
    y = acc.astype(np.float64) * float(alpha[0])
    mean = (y.mean(axis=(0, 2, 3)) + r.standard_normal(Oc) * 0.3).astype(F)
    invstd = (1.0 / (y.std(axis=(0, 2, 3)) + 0.5)).astype(F)
    ga = (r.standard_normal(Oc) * 4).astype(F)
    be = (r.standard_normal(Oc) * 2 + 4).astype(F)
    ga[0], be[0] = F(0), F(5)
    ga[1], be[1] = F(1e-6), F(-1e4)
    ga[2], be[2] = F(1e-6), F(1e4)
    ga[3] = -abs(ga[3]) - F(0.5)
    for c, sg in ((4, 1.0), (5, -1.0)):
        v0 = int(np.sort(acc[:, c].ravel())[acc[:, c].size // 2])          # an attained value near the middle
        alpha[c], bias[c], invstd[c], ga[c] = F(1), F(0), F(1), F(5 * sg)
        mean[c], be[c] = F(v0), F(5)
    return np.stack([alpha, bias, mean, invstd, ga, be, alpha * invstd, (bias - mean) * invstd, ga * invstd]).astype(F)


def chain_codes(acc, chan, pool, n=N_LEVELS):
    """The element-wise fp32 chain of k_qa_fwd in numpy, step by step, with n levels."""
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
    s32 = F(1.0) / F(n)
    return np.floor(((c / s32).astype(F) + F(0.5)).astype(F)).astype(np.uint8)


def qa_fwd_codes(be, acc, chan, pool):
    """The library's own streaming forward on the int16 stash, a_bits = 4."""
    N, Oc, H, W = acc.shape
    shape = (N, Oc, H // 2, W // 2) if pool else (N, Oc, H, W)
    dS, dC = be.to_dev_i16(acc.astype(np.int16)), be.to_dev(chan)
    out = be.to_dev_u8(np.full(shape, 0xee, dtype=np.uint8))
    be.call("mn_qa_fwd", 0, be.ptr(dS), be.ptr(dC), N, Oc, H, W, BITS, int(pool), be.ptr(out), None, be.stream)
    return be.to_host(out).view(np.uint8)


def judge(be, acc, chan, pool):
    """mn_qa_fwd(a_bits = 4) on any map size (the module docstring), and the numpy chain on the accumulator as it is: the two must agree."""
    N, Oc, H, W = acc.shape
    if pool and W % 8:
        nwin = (H // 2) * (W // 2)
        a = acc.reshape(N, Oc, H // 2, 2, W // 2, 2).transpose(0, 1, 3, 2, 4, 5).reshape(N, Oc, 2, 2 * nwin)          # window i = columns 2 i, 2 i + 1 of two rows
        reps = 8 // math.gcd(2 * nwin, 8)
        ref = qa_fwd_codes(be, np.ascontiguousarray(np.tile(a, (1, 1, 1, reps))), chan, 1)[:, :, 0, :nwin].reshape(N, Oc, H // 2, W // 2)
    elif not pool and (H * W) % 8:
        reps = 8 // math.gcd(H * W, 8)
        ref = qa_fwd_codes(be, np.ascontiguousarray(np.tile(acc.reshape(N, Oc, 1, H * W), (1, 1, 1, reps))), chan, 0)[:, :, 0, :H * W].reshape(N, Oc, H, W)
    else:
        ref = qa_fwd_codes(be, acc, chan, pool)
    assert np.array_equal(ref, chain_codes(acc, chan, pool)), "the two judges disagree: mn_qa_fwd vs the numpy chain"
    return ref


# ---------------------------------------------------------------------------------------------- the two quartets at (4, 4, 4)
def _geom(be, form, x_shape, w_shape, groups=1):
    return be.geom(x_shape, w_shape, padding=1 if form == "mfma3" else 0, groups=groups)


def pack_table(be, form, g, w, chan, order=None):
    q = "mn_codeconv_" + form
    nb = int(getattr(be.lib, q + "_table_bytes")(C.byref(g), *WIDTHS))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    dW, dC = be.to_dev(w), be.to_dev(chan)
    be.call(q + "_pack", C.byref(g), be.ptr(dW), be.ptr(dC), *WIDTHS, be.ptr(dO), be.ptr(table), be.stream)
    return table


def fwd_planes(be, form, codes, w, chan, groups, order=None, pool=0):
    """Pack the table and the planes, run the form's fwd_bits TWICE into poisoned buffers; returns (output planes as host uint32, kernel name, table header)."""
    q = "mn_codeconv_" + form
    g = _geom(be, form, codes.shape, w.shape, groups)
    assert getattr(be.lib, q + "_supported")(C.byref(g), *WIDTHS) == 1, "geometry must be covered at 4 bits"
    assert be.lib.mn_codeconv_supported(C.byref(g), *WIDTHS) == 0, "the popcount kernels have no 4-bit form"
    table = pack_table(be, form, g, w, chan, order)
    hdr = _host_u32(be, table)[:8].copy()
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0, "finite constants, weights on the grid, a valid order"
    assert int(hdr[6]) == WORD6
    xp = _dev_i32(be, np_pack_planes(codes, BITS).view(np.int32))
    N, _, H, Wd = codes.shape
    Ho, Wo = (H // 2, Wd // 2) if pool else (H, Wd)
    outs = []
    for _ in range(2):
        yp = _empty_i32(be, (N, (w.shape[0] + 31) // 32, BITS, Ho, Wo))          # poisoned
        be.call(q + "_fwd_bits", C.byref(g), *WIDTHS, be.ptr(table), be.ptr(xp), be.ptr(yp), int(pool), be.stream)
        outs.append(_host_u32(be, yp))
    name = be.lib.mn_last_kernel().decode()
    assert np.array_equal(outs[0], outs[1]), "two runs give identical planes"
    Oc = w.shape[0]
    if Oc % 32:
        assert not (outs[0][:, -1] >> np.uint32(Oc % 32)).any(), "unused bits of the last output group are 0"
    return outs[0], name, hdr


def _against_judge(be, form, codes, w, chan, groups, order, pool, ref, what):
    planes, name, hdr = fwd_planes(be, form, codes, w, chan, groups, order, pool)
    got = np_unpack_planes(planes, w.shape[0])
    want = ref[:, order] if order is not None else ref
    print(name, what, "span", int(hdr[2]) if form == "mfma3" else "-", "mismatches against the judge", int((got != want).sum()), "of", got.size)
    assert name == ("k_codeconv_mfma<%d>" % pool if form == "mfma" else "k_codeconv_mfma3<0>"), name
    assert got.shape == want.shape and np.array_equal(got, want), (int((got != want).sum()), got.size)
    return hdr


def _check_case_inputs(acc, chan, ref):
    """What every block case must hold: all sixteen codes in the judge's output, the special channels doing what they are there for, both boundary values attained."""
    assert len(np.unique(ref)) == N_LEVELS + 1, "the case must produce all sixteen codes"
    full = chain_codes(acc, chan, 0)
    assert (full[:, 1] == 0).all() and (full[:, 2] == N_LEVELS).all() and len(np.unique(full[:, 0])) == 1
    assert (acc[:, 4] == int(chan[2, 4])).any() and (acc[:, 5] == int(chan[2, 5])).any(), "a code boundary sits on an attained accumulator value"
    for c in (4, 5):          # c / s = 7.5 there: the rounding boundary between codes 7 and 8
        assert set(np.unique(full[:, c][acc[:, c] == int(chan[2, c])])) <= {7, 8}


def check_block1(be, case, table=None, conv=None):
    _, x_shape, w_shape, groups, s, pool, seed = (BLOCKS1 if table is None else table)[case]
    codes, w, acc = make_inputs(x_shape, w_shape, groups, 0, seed, conv=conv)
    chan = make_chan(acc, seed)
    ref = judge(be, acc, chan, pool)
    _check_case_inputs(acc, chan, ref)
    order = shuffle_order(w_shape[0], s) if s else None
    hdr = _against_judge(be, "mfma", codes, w, chan, groups, order, pool, ref, "%s %s groups %d shuffle %d pool %d" % (x_shape, w_shape, groups, s, pool))
    assert int(hdr[1]) == (x_shape[1] // groups + 63) // 64 and int(hdr[4]) == 32 * ((w_shape[0] + 31) // 32) and int(hdr[5]) == (x_shape[1] + 31) // 32


def check_block3(be, case, table=None, conv=None):
    _, x_shape, w_shape, groups, s, span_dead, seed = (BLOCKS3 if table is None else table)[case]
    codes, w, acc = make_inputs(x_shape, w_shape, groups, 1, seed, conv=conv)
    chan = make_chan(acc, seed)
    ref = judge(be, acc, chan, 0)
    _check_case_inputs(acc, chan, ref)
    order = shuffle_order(w_shape[0], s) if s else None
    hdr = _against_judge(be, "mfma3", codes, w, chan, groups, order, 0, ref, "%s %s groups %d shuffle %d" % (x_shape, w_shape, groups, s))
    assert int(hdr[1]) == 3 and int(hdr[4]) == 32 * ((w_shape[0] + 31) // 32)          # 9 slots of 16 channels: three k-steps, the last padded
    assert int(hdr[2]) in (2, 4, 8), ("span", int(hdr[2]))
    if span_dead is None:
        assert int(hdr[5]) > 0, ("dead rows", int(hdr[5]))
    else:
        assert (int(hdr[2]), int(hdr[5])) == span_dead, ("span, dead rows", int(hdr[2]), int(hdr[5]))
    return hdr


def check_large1(be, case):
    """One LARGE1 case: the library's own launch rule says that a block takes at least two sets and the last block fewer; then check_block1 against the judge."""
    import deploy_grid as DG
    _, (N, _, H, Wd), w_shape, _, _, pool, _ = LARGE1[case]
    bx = DG.pixel_blocks(N * (H // 2) * (Wd // 2), 64) if pool else DG.pixel_blocks(N * H * Wd, 256)
    DG.assert_uneven_deal(be, bx, ((w_shape[0] + 31) // 32 + 1) // 2)          # a set: the rows of two consecutive output words
    check_block1(be, case, LARGE1, DG.exact_conv)


def check_large3(be, case):
    """One LARGE3 case: check_block3 against the judge, and through the library's own launch rule and the span the packer wrote into the table (header word 2) that
    some block of grid.y took a second span and some block did not."""
    import deploy_grid as DG
    _, (N, _, H, Wd), w_shape, _, _, _, _ = LARGE3[case]
    hdr = check_block3(be, case, LARGE3, DG.exact_conv)
    OW = (w_shape[0] + 31) // 32
    span = int(hdr[2])
    DG.assert_uneven_rows(be, DG.pixel_blocks(N * H * Wd, 256), (OW + 1) >> 1, (OW + span - 1) // span)


def check_fill(be, form, kcode):
    """All codes 15 against all weight codes ``kcode`` (15: acc = +225 per channel and tap, 0: -225) at the K bound: acc = +-32625 (1x1) / +-32400 (3x3, interior)."""
    x_shape, w_shape, extreme = (FILL1_X, FILL1_W, FILL1_EXTREME) if form == "mfma" else (FILL3_X, FILL3_W, FILL3_EXTREME)
    codes = np.full(x_shape, N_LEVELS, dtype=np.uint8)
    k = np.full(w_shape, kcode, dtype=np.int64)
    w = (F(2) * (k.astype(F) / F(N_LEVELS)) - F(1)).astype(F)
    acc = O.conv2d_fwd(codes.astype(np.int64), 2 * k - N_LEVELS, None, padding=1 if form == "mfma3" else 0, groups=1, acc=np.int64)
    sign = 1 if kcode == N_LEVELS else -1
    if form == "mfma":
        assert (acc == sign * extreme).all()
    else:
        assert (acc[:, :, 1:-1, 1:-1] == sign * extreme).all() and np.abs(acc).max() == extreme
    chan = make_chan(acc, 4200)
    ref = judge(be, acc, chan, 0)
    _against_judge(be, form, codes, w, chan, 1, None, 0, ref, "%s fill %d extreme acc %d" % (x_shape, kcode, sign * extreme))


def check_refused(be, case):
    form, kw, widths, pool = REFUSED[case]
    q = "mn_codeconv_" + form
    g = be.geom(kw["x_shape"], kw["w_shape"], padding=kw.get("padding", 0), groups=kw.get("groups", 1))
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    ENOTSUP = _lib().MN_ENOTSUP
    if pool:
        assert getattr(be.lib, q + "_supported")(C.byref(g), *widths) == 1
    else:
        assert getattr(be.lib, q + "_supported")(C.byref(g), *widths) == 0
        assert int(getattr(be.lib, q + "_table_bytes")(C.byref(g), *widths)) == 0
        assert getattr(be.lib, q + "_pack")(C.byref(g), be.ptr(f), be.ptr(f), *widths, None, be.ptr(buf), be.stream) == ENOTSUP
    for p in ((pool,) if pool else (0, 1) if form == "mfma" else (0,)):
        assert getattr(be.lib, q + "_fwd_bits")(C.byref(g), *widths, be.ptr(buf), be.ptr(buf), be.ptr(buf), p, be.stream) == ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_popcount_forms_refuse(be):
    """The plane-serial kernels and the 5x5 tile kernel have no 4-bit instantiation."""
    for kw in (G1, G3, dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2)):
        g = be.geom(kw["x_shape"], kw["w_shape"], padding=kw.get("padding", 0))
        assert be.lib.mn_codeconv_supported(C.byref(g), *WIDTHS) == 0 and int(be.lib.mn_codeconv_table_bytes(C.byref(g), *WIDTHS)) == 0
        assert be.lib.mn_codeconv_tile_supported(C.byref(g), *WIDTHS) == 0 and int(be.lib.mn_codeconv_tile_table_bytes(C.byref(g), *WIDTHS)) == 0


def check_invalid(be, form):
    """Null, misaligned, an invalid geometry and (1x1) odd H with pool are MN_EINVAL and write nothing."""
    EINVAL = _lib().MN_EINVAL
    q = "mn_codeconv_" + form
    kw = G1 if form == "mfma" else G3
    g = be.geom(kw["x_shape"], kw["w_shape"], padding=kw.get("padding", 0))
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    odd = C.c_void_p(be.ptr(buf).value + 2)
    odd8 = C.c_void_p(be.ptr(buf).value + 8)
    pack, fwd = getattr(be.lib, q + "_pack"), getattr(be.lib, q + "_fwd_bits")
    assert pack(C.byref(g), None, be.ptr(f), *WIDTHS, None, be.ptr(buf), be.stream) == EINVAL
    assert pack(C.byref(g), be.ptr(f), None, *WIDTHS, None, be.ptr(buf), be.stream) == EINVAL
    assert pack(C.byref(g), be.ptr(f), be.ptr(f), *WIDTHS, None, None, be.stream) == EINVAL
    assert pack(C.byref(g), be.ptr(f), be.ptr(f), *WIDTHS, None, odd8, be.stream) == EINVAL
    assert fwd(C.byref(g), *WIDTHS, None, be.ptr(buf), be.ptr(buf), 0, be.stream) == EINVAL
    assert fwd(C.byref(g), *WIDTHS, odd8, be.ptr(buf), be.ptr(buf), 0, be.stream) == EINVAL
    assert fwd(C.byref(g), *WIDTHS, be.ptr(buf), None, be.ptr(buf), 0, be.stream) == EINVAL
    assert fwd(C.byref(g), *WIDTHS, be.ptr(buf), be.ptr(buf), None, 0, be.stream) == EINVAL
    assert fwd(C.byref(g), *WIDTHS, be.ptr(buf), odd, be.ptr(buf), 0, be.stream) == EINVAL
    assert fwd(C.byref(g), *WIDTHS, be.ptr(buf), be.ptr(buf), odd, 0, be.stream) == EINVAL
    x0 = (0,) + tuple(kw["x_shape"][1:])
    g0 = be.geom(x0, kw["w_shape"], padding=kw.get("padding", 0))
    assert getattr(be.lib, q + "_supported")(C.byref(g0), *WIDTHS) == 0 and int(getattr(be.lib, q + "_table_bytes")(C.byref(g0), *WIDTHS)) == 0
    assert pack(C.byref(g0), be.ptr(f), be.ptr(f), *WIDTHS, None, be.ptr(buf), be.stream) == EINVAL
    assert fwd(C.byref(g0), *WIDTHS, be.ptr(buf), be.ptr(buf), be.ptr(buf), 0, be.stream) == EINVAL
    if form == "mfma":
        godd = be.geom((1, 32, 7, 8), (32, 32, 1, 1))
        assert be.lib.mn_codeconv_mfma_supported(C.byref(godd), *WIDTHS) == 1
        assert fwd(C.byref(godd), *WIDTHS, be.ptr(buf), be.ptr(buf), be.ptr(buf), 1, be.stream) == EINVAL
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all()


def check_counters(be, form, seed=5):
    """Non-finite channel constants are counted into word 0 of the table, a weight off the grid and a bad out_order entry into word 7; word 6 carries the widths."""
    x_shape, w_shape = ((1, 32, 4, 4), (32, 32, 1, 1)) if form == "mfma" else ((1, 16, 4, 4), (32, 16, 3, 3))
    pad = 1 if form == "mfma3" else 0
    codes, w, acc = make_inputs(x_shape, w_shape, 1, pad, seed)
    chan = make_chan(acc, seed)
    g = _geom(be, form, x_shape, w_shape)
    hdr = _host_u32(be, pack_table(be, form, g, w, chan))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0 and int(hdr[6]) == WORD6
    if form == "mfma":
        assert (int(hdr[1]), int(hdr[4]), int(hdr[5])) == (1, 32, 1)
    else:
        assert (int(hdr[1]), int(hdr[2]), int(hdr[4]), int(hdr[5])) == (3, 2, 32, 0)
    bad = chan.copy()
    bad[0, 7], bad[4, 9], bad[3, 11] = F(np.inf), F(np.nan), F(2e9)
    hdr = _host_u32(be, pack_table(be, form, g, w, bad))
    assert int(hdr[0]) == 3 and int(hdr[7]) == 0
    w2 = w.copy()
    w2[(5, 0, 0, 0) if form == "mfma" else (5, 7, 2, 1)] = F(0.5)          # (0.5 * 15 + 15) / 2 = 11.25: off the grid
    hdr = _host_u32(be, pack_table(be, form, g, w2, chan))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 1
    order = np.arange(w_shape[0])
    order[3] = w_shape[0]
    table = pack_table(be, form, g, w, chan, order)
    hdr = _host_u32(be, table)
    assert int(hdr[7]) == 1
    if form == "mfma3":
        assert int(hdr[5]) == 1, "31 rows: the second tile is a row short"
    # the position of the bad entry yields 0 bits, every other position its channel's code
    xp = _dev_i32(be, np_pack_planes(codes, BITS).view(np.int32))
    yp = _empty_i32(be, (1, 1, BITS, 4, 4))
    be.call("mn_codeconv_%s_fwd_bits" % form, C.byref(g), *WIDTHS, be.ptr(table), be.ptr(xp), be.ptr(yp), 0, be.stream)
    got = np_unpack_planes(_host_u32(be, yp), 32)
    ref = judge(be, acc, chan, 0)
    ref[:, 3] = 0
    assert np.array_equal(got, ref)
