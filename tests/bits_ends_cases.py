"""The two ends of the bit-packed plan through the C ABI (csrc/conv_first.hip: mn_conv2d_first_sign_bits; csrc/qgemm_bits.hip: mn_bitsconv1x1_small_fwd): the same checks on
the CPU emulation build and on the GPU.  Every comparison against the existing entry points is exact -- integer words, or ``np.array_equal`` on fp32."""
import ctypes as C

import numpy as np

from oracle import np_oracle as O
import bits_cases as B

F = np.float32
MN_EINVAL, MN_ENOTSUP = -22, -95          # include/micronet_hip.h

# (N, C, H, W, O, k): 5x5 / padding 2 on 8 x 8 with one full word, a partial last word, several words (MT = 1, 1, 2); 3x3 / padding 1; one image of 4 x 8 (half a chunk);
# 48 and 64 channels per wave (MT = 3: words that straddle two waves, nin's 192-channel first conv is of this kind; MT = 4: two words per wave), O % 32 != 0
FIRST_CASES = [(2, 3, 8, 8, 32, 5), (2, 3, 8, 8, 40, 5), (2, 3, 8, 8, 96, 5), (2, 3, 8, 8, 40, 3), (1, 3, 4, 8, 40, 5), (1, 3, 8, 8, 170, 5), (1, 3, 4, 8, 230, 3)]
CLASSIFIER_SHAPES = [(32, 16), (80, 16), (192, 64), (1024, 4), (1024, 64)]          # (C, HW) at N = 2, O = 10


def first_inputs(N, Cc, H, W, Oc, k, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal((N, Cc, H, W)).astype(F)
    w = (r.standard_normal((Oc, Cc, k, k)) * 0.2).astype(F)
    b = (r.standard_normal(Oc) * 0.5).astype(F)
    return x, w, b


def three_launch_bits(be, g, dX, dW, dB):
    """Today's first stage on the same backend: first conv -> y, mn_bnsign_fwd_i8 with the identity statistics -> int8, mn_bits_pack_sign8 -> words.  Returns (words, y)."""
    N, Oc, H, W = g.N, g.O, g.H, g.W
    y = be.conv_fwd(g, be.actq(0), dX, dW, dB, 0)
    one, zero = np.ones(Oc, dtype=F), np.zeros(Oc, dtype=F)
    dG, dBe, dRM, dRV = be.to_dev(one), be.to_dev(zero), be.to_dev(zero), be.to_dev(one)
    save, a8 = be.empty((2, Oc)), be.empty_i8((N, Oc, H, W))
    ws = be.empty(int(be.lib.mn_bnsign_ws_floats(Oc)) + 8)
    be.call("mn_bnsign_fwd_i8", be.ptr(y), N, Oc, H * W, be.ptr(dG), be.ptr(dBe), 0.0, 0.0, 0, be.ptr(dRM), be.ptr(dRV), be.ptr(save), be.ptr(a8), be.ptr(ws), be.stream)
    bits = B._empty_i32(be, (N, (Oc + 31) // 32, H, W))
    be.call("mn_bits_pack_sign8", be.ptr(a8), N, Oc, H * W, be.ptr(bits), be.stream)
    return B._host_u32(be, bits), be.to_host(y)


def first_sign_bits(be, g, dX, dW, dB, fill=0x5a5a5a5a):
    bits = np.full((g.N, (g.O + 31) // 32, g.H, g.W), fill, dtype=np.uint32).view(np.int32)
    bits = bits if be.kind == "emu" else be.torch.from_numpy(bits).cuda()
    be.call("mn_conv2d_first_sign_bits", C.byref(g), be.ptr(dX), be.ptr(dW), be.ptr(dB), be.ptr(bits), be.stream)
    return B._host_u32(be, bits)


def np_sign_excluded(x, w, b, pad):
    """float64 convolution: (sign +-1, mask of the activations within 1e-4 max|y| of zero -- left out of the sign comparison)."""
    y = O.conv2d_fwd(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), padding=pad)
    return np.where(y < 0, -1, 1).astype(np.int8), np.abs(y) <= 1e-4 * np.abs(y).max()


def check_first_bits(be, N, Cc, H, W, Oc, k, seed=0):
    x, w, b = first_inputs(N, Cc, H, W, Oc, k, seed)
    g = be.geom(x.shape, w.shape, padding=(k - 1) // 2)
    assert be.lib.mn_conv2d_first_supported(C.byref(g), 0) == 1 and be.lib.mn_conv2d_first_sign_bits_supported(C.byref(g)) == 1
    dX, dW, dB = be.to_dev(x), be.to_dev(w), be.to_dev(b)
    want, _ = three_launch_bits(be, g, dX, dW, dB)
    got = first_sign_bits(be, g, dX, dW, dB)
    print("first bits", (N, Cc, H, W, Oc, k), "words differing from the three-launch path:", int((got != want).sum()), "of", got.size)
    assert np.array_equal(got, want)
    # independently: the signs of a float64 numpy convolution, but for activations too close to zero for fp32 to decide
    s64, near = np_sign_excluded(x, w, b, (k - 1) // 2)
    print("  left out of the float64 comparison: %d of %d" % (int(near.sum()), near.size))
    assert near.mean() <= 0.01
    assert np.array_equal(B.np_unpack(got, Oc)[~near], s64[~near])


def check_first_bits_zero_rule(be, seed=0):
    """y == +0, y == -0 and NaN: channel 1 has zero weights and bias +0, channel 2 zero weights and bias -0, channel 3 bias NaN; the bits are the three-launch path's."""
    N, Cc, H, W, Oc, k = 2, 3, 8, 8, 40, 5
    x, w, b = first_inputs(N, Cc, H, W, Oc, k, seed)
    w[1], w[2] = 0, 0
    b[1], b[2], b[3] = F(0.0), F(-0.0), F(np.nan)
    g = be.geom(x.shape, w.shape, padding=2)
    dX, dW, dB = be.to_dev(x), be.to_dev(w), be.to_dev(b)
    want, y = three_launch_bits(be, g, dX, dW, dB)
    assert (y[:, 1] == 0).all() and (y[:, 2] == 0).all() and np.isnan(y[:, 3]).all(), "the case must contain y == 0 and NaN"
    got = first_sign_bits(be, g, dX, dW, dB)
    assert np.array_equal(got, want)
    a = B.np_unpack(got, Oc)
    assert (a[:, 1] == 1).all() and (a[:, 2] == 1).all() and (a[:, 3] == 1).all(), "+0, -0 and NaN give +1 (mn_bnsign_fwd_i8 with the identity statistics)"


def check_first_bits_tail_is_zero(be, seed=0):
    N, Cc, H, W, Oc, k = 2, 3, 8, 8, 40, 5
    x, w, b = first_inputs(N, Cc, H, W, Oc, k, seed)
    g = be.geom(x.shape, w.shape, padding=2)
    got = first_sign_bits(be, g, be.to_dev(x), be.to_dev(w), be.to_dev(b), fill=0xFFFFFFFF)
    assert not (got[:, 1] >> np.uint32(8)).any(), "the high 24 bits of every second word are 0"
    assert (got[:, 0] != 0xFFFFFFFF).any() and (got[:, 1] != 0).any()


def check_bits_classifier(be, Cc, HW, bias, N=2, Oc=10, seed=0):
    r = np.random.default_rng(seed)
    H, W = (HW // 8, 8) if HW % 8 == 0 else (HW // 4, 4)
    a = np.where(r.standard_normal((N, Cc, H, W)) > 0, 1, -1).astype(np.int8)
    w = (r.standard_normal((Oc, Cc, 1, 1)) * 0.1).astype(F)
    b = (r.standard_normal(Oc) * 0.2).astype(F) if bias else None
    assert be.lib.mn_bitsconv1x1_small_supported(Cc, HW, Oc) == 1 and be.lib.mn_signconv1x1_small_supported(Cc, HW, Oc) == 1
    bits = B.pack(be, a)
    a8 = be.to_dev_i8(B.unpack(be, bits, Cc))
    dW, dB = be.to_dev(w), (be.to_dev(b) if bias else None)
    y_bits, y_codes = be.empty((N, Oc, H, W)), be.empty((N, Oc, H, W))
    be.call("mn_bitsconv1x1_small_fwd", be.ptr(bits), be.ptr(dW), be.ptr(dB), be.ptr(y_bits), N, Cc, HW, Oc, be.stream)
    be.call("mn_signconv1x1_small_fwd", be.ptr(a8), be.ptr(dW), be.ptr(dB), be.ptr(y_codes), N, Cc, HW, Oc, be.stream)
    got, want = be.to_host(y_bits), be.to_host(y_codes)
    y64 = O.conv2d_fwd(a.astype(np.float64), w.astype(np.float64), None if b is None else b.astype(np.float64))
    err = float(np.abs(got - y64).max() / np.abs(y64).max())
    print("bits classifier", (Cc, HW), "bias", bias, "differing from the code kernel:", int((got != want).sum()), "rel. error vs float64: %.2e" % err)
    assert np.array_equal(got, want)
    assert err <= 1e-5


def _rc(be, name, *args):
    return getattr(be.lib, name)(*args)


def check_rejects_bad_arguments(be):
    POISON = 0x5a5a5a5a
    x, w, b = first_inputs(2, 3, 8, 8, 40, 5, 0)
    dX, dW, dB = be.to_dev(x), be.to_dev(w), be.to_dev(b)
    g = be.geom(x.shape, w.shape, padding=2)
    bits = B._empty_i32(be, (2 * 2 * 64 + 4,))
    untouched = lambda: bool((B._host_u32(be, bits) == POISON).all())
    call = lambda gg, px, pw, pb: _rc(be, "mn_conv2d_first_sign_bits", C.byref(gg), px, pw, be.ptr(dB), pb, be.stream)
    # null pointers, misaligned bits: MN_EINVAL
    assert call(g, None, be.ptr(dW), be.ptr(bits)) == MN_EINVAL
    assert call(g, be.ptr(dX), None, be.ptr(bits)) == MN_EINVAL
    assert call(g, be.ptr(dX), be.ptr(dW), None) == MN_EINVAL
    assert call(g, be.ptr(dX), be.ptr(dW), C.c_void_p(be.ptr(bits).value + 2)) == MN_EINVAL
    assert _rc(be, "mn_conv2d_first_sign_bits", None, be.ptr(dX), be.ptr(dW), be.ptr(dB), be.ptr(bits), be.stream) == MN_EINVAL
    # geometries mn_conv2d_first_sign_bits_supported refuses: valid but not covered -> MN_ENOTSUP; not a geometry at all (O = 0) -> MN_EINVAL
    refused = [(be.geom((2, 4, 8, 8), (40, 2, 5, 5), padding=2, groups=2), MN_ENOTSUP), (be.geom(x.shape, w.shape, stride=2, padding=2), MN_ENOTSUP),
               (be.geom(x.shape, w.shape, padding=1), MN_ENOTSUP), (be.geom((2, 3, 8, 6), w.shape, padding=2), MN_ENOTSUP),
               (be.geom(x.shape, (0, 3, 5, 5), padding=2), MN_EINVAL)]
    for gg, code in refused:
        assert be.lib.mn_conv2d_first_sign_bits_supported(C.byref(gg)) == 0
        assert call(gg, be.ptr(dX), be.ptr(dW), be.ptr(bits)) == code
    assert be.lib.mn_conv2d_first_sign_bits_supported(None) == 0
    assert untouched(), "a refused call writes nothing"
    # the classifier
    Cc, HW, Oc, N = 32, 16, 10, 2
    wc, yb = be.to_dev(np.ones((Oc, Cc), dtype=F)), be.empty((N * Oc * HW + 4,))
    cbits = B._empty_i32(be, (N * HW + 4,))
    y0 = be.to_host(yb).copy()
    ccall = lambda pb, pw, py, n=N, c=Cc, hw=HW, o=Oc: _rc(be, "mn_bitsconv1x1_small_fwd", pb, pw, None, py, n, c, hw, o, be.stream)
    assert ccall(None, be.ptr(wc), be.ptr(yb)) == MN_EINVAL
    assert ccall(be.ptr(cbits), None, be.ptr(yb)) == MN_EINVAL
    assert ccall(be.ptr(cbits), be.ptr(wc), None) == MN_EINVAL
    assert ccall(be.ptr_at(cbits, 1), be.ptr(wc), be.ptr(yb)) == MN_EINVAL          # bits not 16-byte aligned
    assert ccall(be.ptr(cbits), be.ptr(wc), be.ptr_at(yb, 1)) == MN_EINVAL
    assert ccall(be.ptr(cbits), be.ptr(wc), be.ptr(yb), n=0) == MN_EINVAL
    for c_, hw_, o_ in ((Cc, HW, 0), (Cc, HW, 17), (Cc, 6, Oc), (2, HW, Oc), (4096, HW, 16)):
        assert be.lib.mn_bitsconv1x1_small_supported(c_, hw_, o_) == 0
        assert ccall(be.ptr(cbits), be.ptr(wc), be.ptr(yb), c=c_, hw=hw_, o=o_) == MN_ENOTSUP
    assert np.array_equal(be.to_host(yb), y0), "a refused call writes nothing"
