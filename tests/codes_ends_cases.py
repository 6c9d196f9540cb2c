"""The two ends of the code-packed plan through the C ABI (csrc/conv_first.hip: mn_conv2d_first_codes; csrc/qgemm_codes.h: mn_planesconv1x1_small_fwd): the same checks on
the CPU emulation build and on the GPU.  Every comparison against the existing entry points is exact -- integer words, or ``np.array_equal`` on fp32."""
import ctypes as C

import numpy as np

from oracle import np_oracle as O
from bits_cases import _empty_i32, _host_u32
import bits_ends_cases as BE
import codes_cases as CC

F = np.float32
MN_EINVAL, MN_ENOTSUP = -22, -95          # include/micronet_hip.h
A_BITS = 2

FIRST_CASES = BE.FIRST_CASES          # the smallest shapes that reach every MT, a partial last word, words straddling waves, half a chunk
CLASSIFIER_SHAPES = [(32, 16), (80, 16), (192, 64), (1024, 4), (1024, 64)]          # (C, HW) at N = 2, O = 10
CLASSIFIER_ODD = (40, 16)          # N = 3, O = 3: a partial word, a pixel tail block, OP rounded up


# ---------------------------------------------------------------------------------------------- the first conv
def make_chan_y(y, seed=0, special=True):
    """[9][O] block constants in the manner of codes_cases.make_chan, around the spread of the first conv's own y (alpha = 1, bias = 0: the rows of an fp32 input), so
    that all four codes occur; both signs of gamma.  special: channel 0 gamma = 0, channel 1 never reaches code 1, channel 2 always code 3, channel 3 gamma < 0 for
    certain, channels 4 and 5 a rounding boundary exactly on an attained y (mean = y0, invstd = 1, gamma = +-5, beta = 5: y = y0 gives 0.1 z = 0.5, c / s = 1.5)."""
    r = np.random.default_rng(seed + 77)
    Oc = y.shape[1]
    alpha, bias = np.ones(Oc, dtype=F), np.zeros(Oc, dtype=F)
    y64 = y.astype(np.float64)
    mean = (y64.mean(axis=(0, 2, 3)) + r.standard_normal(Oc) * 0.3).astype(F)
    invstd = (1.0 / (y64.std(axis=(0, 2, 3)) + 0.5)).astype(F)
    ga = (r.standard_normal(Oc) * 4).astype(F)
    be = (r.standard_normal(Oc) * 2 + 4).astype(F)
    y0 = {}
    if special:
        assert Oc >= 6
        ga[0], be[0] = F(0), F(5)
        ga[1], be[1] = F(1e-6), F(-1e4)
        ga[2], be[2] = F(1e-6), F(1e4)
        ga[3] = -abs(ga[3]) - F(0.5)
        for c, sg in ((4, 1.0), (5, -1.0)):
            y0[c] = np.sort(y[:, c].ravel())[y[:, c].size // 2]          # an attained value near the middle
            invstd[c], ga[c], mean[c], be[c] = F(1), F(5 * sg), y0[c], F(5)
    return np.stack([alpha, bias, mean, invstd, ga, be, alpha * invstd, (bias - mean) * invstd, ga * invstd]).astype(F), y0


def chain_codes_y(y, chan):
    """codes_cases.chain_codes without its acc -> y step: the element-wise fp32 chain of k_qa_fwd<1, 0, 0> in numpy, step by step, on fp32 y."""
    mean, invstd, ga, beb = (chan[i].reshape(1, -1, 1, 1) for i in range(2, 6))
    zh = ((y - mean).astype(F) * invstd).astype(F)
    z = ((zh * ga).astype(F) + beb).astype(F)
    a = np.where(z > 0, z, F(0)).astype(F)
    c = np.minimum(np.maximum((a * F(0.1)).astype(F), F(0)), F(1)).astype(F)
    s32 = F(1.0) / F(CC.N_LEVELS)
    return np.floor(((c / s32).astype(F) + F(0.5)).astype(F)).astype(np.uint8)


def first_y(be, g, dX, dW, dB):
    """today's first conv on the same backend: the fp32 map y (device buffer)"""
    return be.conv_fwd(g, be.actq(0), dX, dW, dB, 0)


def three_launch_planes(be, g, y, chan):
    """Today's first stage behind the conv: mn_qa_fwd(in_f32 = 1) -> one byte per code, mn_codes_pack_planes -> planes."""
    N, Oc, H, W = g.N, g.O, g.H, g.W
    codes = be.to_dev_u8(np.full((N, Oc, H, W), 0xee, dtype=np.uint8))
    be.call("mn_qa_fwd", 1, be.ptr(y), be.ptr(be.to_dev(chan)), N, Oc, H, W, A_BITS, 0, be.ptr(codes), None, be.stream)
    planes = _empty_i32(be, (N, (Oc + 31) // 32, A_BITS, H, W))
    be.call("mn_codes_pack_planes", be.ptr(codes), N, Oc, H * W, A_BITS, be.ptr(planes), be.stream)
    return _host_u32(be, planes)


def pack_first_table(be, chan):
    Oc = chan.shape[1]
    nb = int(be.lib.mn_conv2d_first_codes_table_bytes(Oc, A_BITS))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    be.call("mn_conv2d_first_codes_pack", be.ptr(be.to_dev(chan)), Oc, A_BITS, be.ptr(table), be.stream)
    return table


def first_codes(be, g, dX, dW, dB, table, fill=0x5a5a5a5a):
    planes = np.full((g.N, (g.O + 31) // 32, A_BITS, g.H, g.W), fill, dtype=np.uint32).view(np.int32)
    planes = planes if be.kind == "emu" else be.torch.from_numpy(planes).cuda()
    be.call("mn_conv2d_first_codes", C.byref(g), be.ptr(dX), be.ptr(dW), be.ptr(dB), be.ptr(table), be.ptr(planes), be.stream)
    return _host_u32(be, planes)


def _first_setup(be, N, Cc, H, W, Oc, k, seed):
    x, w, b = BE.first_inputs(N, Cc, H, W, Oc, k, seed)
    g = be.geom(x.shape, w.shape, padding=(k - 1) // 2)
    assert be.lib.mn_conv2d_first_sign_bits_supported(C.byref(g)) == 1 and be.lib.mn_conv2d_first_codes_supported(C.byref(g), A_BITS) == 1
    return x, w, b, g


def check_first_codes(be, N, Cc, H, W, Oc, k, seed=0):
    x, w, b, g = _first_setup(be, N, Cc, H, W, Oc, k, seed)
    dX, dW, dB = be.to_dev(x), be.to_dev(w), be.to_dev(b)
    dY = first_y(be, g, dX, dW, dB)
    y = be.to_host(dY)
    chan, y0 = make_chan_y(y, seed)
    want = three_launch_planes(be, g, dY, chan)                       # judge (a)
    chain = chain_codes_y(y, chan)                                    # judge (b)
    assert np.array_equal(want, CC.np_pack_planes(chain)), "the two judges disagree: mn_qa_fwd(in_f32 = 1) + pack vs the numpy chain on today's y"
    assert len(np.unique(chain)) == 4, "the case must produce all four codes"
    assert (chain[:, 1] == 0).all() and (chain[:, 2] == CC.N_LEVELS).all() and len(np.unique(chain[:, 0])) == 1 and chan[4, 3] < 0
    assert (y[:, 4] == y0[4]).any() and (y[:, 5] == y0[5]).any(), "a rounding boundary sits on an attained y"
    table = pack_first_table(be, chan)
    assert int(_host_u32(be, table)[0]) == 0, "finite constants"
    got = first_codes(be, g, dX, dW, dB, table)
    print("first codes", (N, Cc, H, W, Oc, k), "words differing from the three-launch path:", int((got != want).sum()), "of", got.size,
          "codes", np.bincount(chain.ravel(), minlength=4))
    assert np.array_equal(got, want)
    assert np.array_equal(got, CC.np_pack_planes(chain))


def check_first_codes_guard(be, seed=0):
    """|y| > 1e9 and NaN: channel 6 has bias 3e9, channel 7 bias NaN -- outside the thresholds' range, the kernel runs the chain itself; the planes are the three-launch path's."""
    N, Cc, H, W, Oc, k = 2, 3, 8, 8, 40, 5
    x, w, b, g = _first_setup(be, N, Cc, H, W, Oc, k, seed)
    dX, dW = be.to_dev(x), be.to_dev(w)
    chan, _ = make_chan_y(be.to_host(first_y(be, g, dX, dW, be.to_dev(b))), seed)          # constants on the spread of the unperturbed y
    b[6], b[7] = F(3e9), F(np.nan)
    dB = be.to_dev(b)
    dY = first_y(be, g, dX, dW, dB)
    y = be.to_host(dY)
    assert (np.abs(y[:, 6]) > 1e9).all() and np.isnan(y[:, 7]).all(), "the case must contain |y| > 1e9 and NaN"
    want = three_launch_planes(be, g, dY, chan)
    table = pack_first_table(be, chan)
    assert int(_host_u32(be, table)[0]) == 0
    got = first_codes(be, g, dX, dW, dB, table)
    print("first codes guard: words differing:", int((got != want).sum()), "of", got.size, "codes of the 3e9 channel", np.unique(CC.np_unpack_planes(got, Oc)[:, 6]),
          "of the NaN channel", np.unique(CC.np_unpack_planes(got, Oc)[:, 7]))
    assert np.array_equal(got, want)


def check_first_codes_tail_is_zero(be, seed=0):
    N, Cc, H, W, Oc, k = 2, 3, 8, 8, 40, 5
    x, w, b, g = _first_setup(be, N, Cc, H, W, Oc, k, seed)
    dX, dW, dB = be.to_dev(x), be.to_dev(w), be.to_dev(b)
    chan, _ = make_chan_y(be.to_host(first_y(be, g, dX, dW, dB)), seed)
    got = first_codes(be, g, dX, dW, dB, pack_first_table(be, chan), fill=0xFFFFFFFF)
    assert got.shape == (N, 2, 2, H, W)
    assert not (got[:, 1] >> np.uint32(8)).any(), "the high 24 bits of the last word group are 0 in both planes"
    assert (got[:, 0] != 0xFFFFFFFF).any() and (got[:, 1, 0] != 0).any() and (got[:, 1, 1] != 0).any()


def check_first_nonfinite_counted(be, seed=0):
    """A constant of 2e9 fails qa_chan_finite: counted into word 0 of the table."""
    x, w, b, g = _first_setup(be, 2, 3, 8, 8, 40, 5, seed)
    chan, _ = make_chan_y(be.to_host(first_y(be, g, be.to_dev(x), be.to_dev(w), be.to_dev(b))), seed)
    assert int(_host_u32(be, pack_first_table(be, chan))[0]) == 0
    bad = chan.copy()
    bad[4, 9] = F(2e9)
    assert int(_host_u32(be, pack_first_table(be, bad))[0]) == 1
    bad[3, 11], bad[5, 12] = F(np.inf), F(np.nan)
    assert int(_host_u32(be, pack_first_table(be, bad))[0]) == 3


# ---------------------------------------------------------------------------------------------- the classifier
def check_planes_classifier(be, Cc, HW, bias, N=2, Oc=10, seed=0):
    r = np.random.default_rng(seed)
    H, W = (HW // 8, 8) if HW % 8 == 0 else (HW // 4, 4)
    codes = r.integers(0, 4, size=(N, Cc, H, W)).astype(np.uint8)
    codes[:, :, 0, 0] = 0                                            # a whole-zero pixel and a saturated one
    codes[0, :, -1, -1] = CC.N_LEVELS
    w = (r.standard_normal((Oc, Cc, 1, 1)) * 0.1).astype(F)
    b = (r.standard_normal(Oc) * 0.2).astype(F) if bias else None
    assert be.lib.mn_planesconv1x1_small_supported(Cc, HW, Oc, A_BITS) == 1 and be.lib.mn_signconv1x1_small_supported(Cc, HW, Oc) == 1
    planes = CC.pack(be, codes)
    c8 = be.to_dev_u8(CC.unpack(be, planes, Cc))
    dW, dB = be.to_dev(w), (be.to_dev(b) if bias else None)
    y_planes, y_codes = be.empty((N, Oc, H, W)), be.empty((N, Oc, H, W))
    be.call("mn_planesconv1x1_small_fwd", be.ptr(planes), A_BITS, be.ptr(dW), be.ptr(dB), be.ptr(y_planes), N, Cc, HW, Oc, be.stream)
    be.call("mn_codeconv1x1_small_fwd", be.ptr(c8), A_BITS, be.ptr(dW), be.ptr(dB), be.ptr(y_codes), N, Cc, HW, Oc, be.stream)
    got, want = be.to_host(y_planes), be.to_host(y_codes)
    y64 = O.conv2d_fwd(codes.astype(np.float64) / CC.N_LEVELS, w.astype(np.float64), None if b is None else b.astype(np.float64))
    err = float(np.abs(got - y64).max() / np.abs(y64).max())
    print("planes classifier", (Cc, HW, N, Oc), "bias", bias, "differing from the code kernel:", int((got != want).sum()), "rel. error vs float64: %.2e" % err)
    assert np.array_equal(got, want)
    assert err <= 1e-5


# ---------------------------------------------------------------------------------------------- bad arguments
def _rc(be, name, *args):
    return getattr(be.lib, name)(*args)


def check_rejects_bad_arguments(be):
    POISON = 0x5a5a5a5a
    x, w, b = BE.first_inputs(2, 3, 8, 8, 40, 5, 0)
    dX, dW, dB = be.to_dev(x), be.to_dev(w), be.to_dev(b)
    g = be.geom(x.shape, w.shape, padding=2)
    chan, _ = make_chan_y(np.random.default_rng(0).standard_normal((2, 40, 8, 8)).astype(F), 0)
    table = pack_first_table(be, chan)
    t0 = _host_u32(be, table).copy()
    planes = _empty_i32(be, (2 * 2 * 2 * 64 + 4,))
    untouched = lambda: bool((_host_u32(be, planes) == POISON).all())
    call = lambda gg, px, pw, pt, pp: _rc(be, "mn_conv2d_first_codes", C.byref(gg), px, pw, be.ptr(dB), pt, pp, be.stream)
    args = (be.ptr(dX), be.ptr(dW), be.ptr(table), be.ptr(planes))
    # null pointers, misaligned planes / table, N = 0: MN_EINVAL
    for i in range(4):
        assert call(g, *[None if j == i else a for j, a in enumerate(args)]) == MN_EINVAL
    assert call(g, args[0], args[1], args[2], C.c_void_p(be.ptr(planes).value + 2)) == MN_EINVAL
    assert call(g, args[0], args[1], be.ptr_at(table, 1), args[3]) == MN_EINVAL
    assert _rc(be, "mn_conv2d_first_codes", None, args[0], args[1], be.ptr(dB), args[2], args[3], be.stream) == MN_EINVAL
    assert call(be.geom((0, 3, 8, 8), w.shape, padding=2), *args) == MN_EINVAL
    # geometries mn_conv2d_first_codes_supported refuses: valid but not covered -> MN_ENOTSUP
    refused = [be.geom((2, 4, 8, 8), (40, 2, 5, 5), padding=2, groups=2), be.geom(x.shape, w.shape, stride=2, padding=2), be.geom(x.shape, w.shape, padding=1),
               be.geom((2, 3, 8, 6), w.shape, padding=2)]
    for gg in refused:
        assert be.lib.mn_conv2d_first_codes_supported(C.byref(gg), A_BITS) == 0
        assert call(gg, *args) == MN_ENOTSUP
    assert be.lib.mn_conv2d_first_codes_supported(None, A_BITS) == 0
    assert untouched(), "a refused call writes nothing"
    # 3-bit output codes: not instantiated
    assert be.lib.mn_conv2d_first_codes_supported(C.byref(g), 3) == 0 and int(be.lib.mn_conv2d_first_codes_table_bytes(40, 3)) == 0
    dC = be.to_dev(chan)
    assert _rc(be, "mn_conv2d_first_codes_pack", be.ptr(dC), 40, 3, be.ptr(table), be.stream) == MN_ENOTSUP
    assert _rc(be, "mn_conv2d_first_codes_pack", None, 40, A_BITS, be.ptr(table), be.stream) == MN_EINVAL
    assert _rc(be, "mn_conv2d_first_codes_pack", be.ptr(dC), 40, A_BITS, None, be.stream) == MN_EINVAL
    assert _rc(be, "mn_conv2d_first_codes_pack", be.ptr(dC), 40, A_BITS, be.ptr_at(table, 1), be.stream) == MN_EINVAL
    assert _rc(be, "mn_conv2d_first_codes_pack", be.ptr(dC), 0, A_BITS, be.ptr(table), be.stream) == MN_EINVAL
    assert np.array_equal(_host_u32(be, table), t0), "a refused pack writes nothing"
    # the classifier
    Cc, HW, Oc, N = 32, 16, 10, 2
    wc, yb = be.to_dev(np.ones((Oc, Cc), dtype=F)), be.empty((N * Oc * HW + 4,))
    cpl = _empty_i32(be, (N * 2 * HW + 4,))
    y0 = be.to_host(yb).copy()
    ccall = lambda pb, pw, py, n=N, c=Cc, hw=HW, o=Oc, a=A_BITS: _rc(be, "mn_planesconv1x1_small_fwd", pb, a, pw, None, py, n, c, hw, o, be.stream)
    assert ccall(None, be.ptr(wc), be.ptr(yb)) == MN_EINVAL
    assert ccall(be.ptr(cpl), None, be.ptr(yb)) == MN_EINVAL
    assert ccall(be.ptr(cpl), be.ptr(wc), None) == MN_EINVAL
    assert ccall(be.ptr_at(cpl, 1), be.ptr(wc), be.ptr(yb)) == MN_EINVAL          # planes not 16-byte aligned
    assert ccall(be.ptr(cpl), be.ptr(wc), be.ptr_at(yb, 1)) == MN_EINVAL
    assert ccall(be.ptr(cpl), be.ptr(wc), be.ptr(yb), n=0) == MN_EINVAL
    for c_, hw_, o_, a_ in ((Cc, HW, Oc, 3), (Cc, HW, 17, A_BITS), (Cc, 6, Oc, A_BITS), (4096, HW, 16, A_BITS)):
        assert be.lib.mn_planesconv1x1_small_supported(c_, hw_, o_, a_) == 0
        assert ccall(be.ptr(cpl), be.ptr(wc), be.ptr(yb), c=c_, hw=hw_, o=o_, a=a_) == MN_ENOTSUP
    assert np.array_equal(be.to_host(yb), y0), "a refused call writes nothing"
