"""The first conv block's forward on the bf16 matrix cores (k_c1b_fwd<MT, EPI>, conv_first.hip): the image strip is staged once as three bf16 term planes and
the im2col tile is a gather of finished terms.  A geometry sweep of the plain forward against an fp64 convolution under a derived bound, strip independence bit
for bit, and the fused epilogues (codes + pass nibbles) against the host's evaluation of the plain forward's y.  Backend-agnostic (emulator / GPU)."""
import ctypes as C

import numpy as np

F = np.float32

# K = Cin k k: 75, 27, 25, 9; O: MT 1 .. 4, a partly filled last wave (72, 136, 200), two channel blocks (264); images: 8x8 (one 64-pixel chunk), 12x8 (a strip of
# 96 pixels: the second chunk half masked), 16x16 at N = 600 (R = H: one strip per image, four chunks), 16x8 (two strips per image: row0 > 0, the halo rows are
# the neighbouring strip's), 40x44 (one strip of 1760 pixels whose fp32 patch is 26 KB: the term planes take the block past 80 KB of LDS, one block per CU).  Every
# K, O and image once, not the cross product.
CASES = [
    dict(N=3, Cin=3, H=8, W=8, k=5, O=136),
    dict(N=2, Cin=3, H=12, W=8, k=3, O=72),
    dict(N=600, Cin=1, H=16, W=16, k=3, O=24),
    dict(N=3, Cin=1, H=8, W=8, k=5, O=200),
    dict(N=2, Cin=3, H=12, W=8, k=5, O=256),
    dict(N=3, Cin=3, H=8, W=8, k=3, O=264),
    dict(N=3, Cin=3, H=16, W=8, k=5, O=24),
    dict(N=1, Cin=3, H=40, W=44, k=5, O=24),
]
BIG = 2          # the N = 600 case
SMALL = [i for i in range(len(CASES)) if i != BIG]
MT_OF = lambda O: 4 if O > 192 else (3 if O > 128 else (2 if O > 64 else 1))


def make(case, bias, seed):
    r = np.random.default_rng(seed)
    c = CASES[case]
    x = r.standard_normal((c["N"], c["Cin"], c["H"], c["W"])).astype(F)
    w = (r.standard_normal((c["O"], c["Cin"], c["k"], c["k"])) * 0.2).astype(F)
    b = (r.standard_normal(c["O"]) * 0.3).astype(F) if bias else None
    return c, x, w, b


def conv64(x, w, b):
    """fp64 'same' convolution and, per output element, sum_k |w_k x_k|"""
    N, Cin, H, W = x.shape
    O, _, k, _ = w.shape
    p = k // 2
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (p, p), (p, p)))
    win = np.lib.stride_tricks.sliding_window_view(xp, (k, k), axis=(2, 3))          # [N][Cin][H][W][k][k]
    P = win.transpose(0, 2, 3, 1, 4, 5).reshape(N * H * W, Cin * k * k)
    Wm = w.astype(np.float64).reshape(O, -1)
    y = P @ Wm.T
    mag = np.abs(P) @ np.abs(Wm).T
    if b is not None:
        y = y + b.astype(np.float64)
    shape = lambda t: t.reshape(N, H, W, O).transpose(0, 3, 1, 2)
    return shape(y), shape(mag)


def forward(be, x, w, b, relu=None):
    """plain forward through mn_conv2d_fwd (relu None) or mn_conv2d_fwd_act with the (min, max) partials; returns y on the host [, the partials]"""
    N, Cin, H, W = x.shape
    O, _, k, _ = w.shape
    g = be.geom(x.shape, w.shape, padding=k // 2)
    assert be.lib.mn_conv2d_first_supported(C.byref(g), 0) == 1
    dX, dW, dB = be.to_dev(x), be.to_dev(w), (be.to_dev(b) if b is not None else None)
    none = be.actq(0)
    if relu is None:
        y = be.conv_fwd(g, none, dX, dW, dB, 0)
        assert be.lib.mn_last_kernel().decode() == "k_c1b_fwd<%d>" % MT_OF(O)
        return be.to_host(y)
    cnt = int(be.lib.mn_conv2d_fwd_act_mm_count(C.byref(g), C.byref(none), None))
    assert cnt > 0
    nb = int(be.lib.mn_conv2d_ws_bytes(C.byref(g), 0, 0))
    ws, y, mm = be.empty(nb // 4 + 4), be.empty((N, O, H, W)), be.empty(2 * cnt)
    be.call("mn_conv2d_fwd_act", C.byref(g), C.byref(none), None, be.ptr(dX), be.ptr(dW), be.ptr(dB), be.ptr(y), relu, be.ptr(mm), be.ptr(ws), nb, be.stream)
    assert be.lib.mn_last_kernel().decode() == "k_c1b_fwd<%d>" % MT_OF(O)
    return be.to_host(y), be.to_host(mm), cnt


def bound(w, b, mag):
    """|y - y64| <= (K + 4) 2^-24 sum_k |w_k x_k| + 2^-24 |bias|: fp32 accumulation of K products and the bias (K + 1 roundings of partial sums that sum_k |w_k x_k|
    + |bias| bounds) and the three term products of every w_k x_k that the six-product form drops."""
    K = w[0].size
    u = 2.0 ** -24
    bb = np.abs(b.astype(np.float64)).reshape(1, -1, 1, 1) if b is not None else 0.0
    return (K + 4) * u * mag + u * bb


def check_plain(be, case, bias, seed=0):
    c, x, w, b = make(case, bias, seed)
    y = forward(be, x, w, b).astype(np.float64)
    y64, mag = conv64(x, w, b)
    assert np.isfinite(y).all()
    err, bd = np.abs(y - y64), bound(w, b, mag)
    K = w[0].size
    print("first fwd case %d bias %d: max err in units of 2^-24 sum|w x| = %.3f (bound K + 4 = %d), max err / bound = %.4f"
          % (case, bias, float((err / (2.0 ** -24 * mag + 1e-300)).max()), K + 4, float((err / bd).max())))
    assert (err <= bd).all(), float((err / bd).max())
    return y


def check_relu_mm(be, case, seed=0):
    """relu and the (min, max) partials on: the plain forward rectified, bit for bit; the partials reduce to the extremes of what was stored"""
    c, x, w, b = make(case, True, seed)
    y0 = forward(be, x, w, b)
    y1, mm, cnt = forward(be, x, w, b, relu=1)
    assert np.array_equal(y1, np.maximum(y0, 0))
    assert mm[:cnt].min() == y1.min() and mm[cnt:].max() == y1.max()
    y64, mag = conv64(x, w, b)
    assert (np.abs(y1.astype(np.float64) - np.maximum(y64, 0)) <= bound(w, b, mag)).all()


def check_strip_independence(be, seed=0):
    """image 0 of the N = 600 case (R = H: one strip) computed alone (N = 1: the planner halves R twice, four strips of four rows): the same y bit for bit"""
    c, x, w, b = make(BIG, True, seed)
    y_all = forward(be, x, w, b)
    y_one = forward(be, x[:1], w, b)
    assert np.array_equal(y_all[0].view(np.uint32), y_one[0].view(np.uint32)), "a pixel's accumulation depends on the strip that staged its patch"
    return y_all


def fused_inputs(case, bias, act, seed):
    """the sweep's inputs with image 0 holding a constant channel and the last image a NaN pixel; BatchNorm constants of check_first_conv_fused"""
    c, x, w, b = make(case, bias, seed)
    r = np.random.default_rng(seed + 1000)
    x[0, c["Cin"] - 1] = F(0.75)
    x[-1, 0, c["H"] // 2, 3] = np.nan
    O = c["O"]
    if act == 1:
        gamma, beta = (r.standard_normal(O) * 0.5 + 1).astype(F), (r.standard_normal(O) * 0.3).astype(F)
    else:
        gamma, beta = (r.standard_normal(O) * 2.0 + 3.0).astype(F), (r.standard_normal(O) * 2.0 + 3.0).astype(F)
    return c, x, w, b, gamma, beta


def check_fused(be, case, bias, act, bits=2, seed=0):
    """mn_conv2d_first_bnact_fwd: codes and pass nibbles equal those formed on the host from the plain forward's y in the kernel's fp32 expression order
    (z = ((y - mean) * invstd) * gamma + beta; act 2: the library's own quantizer pass on y gives the reference codes, as in check_first_conv_fused)."""
    c, x, w, b, gamma, beta = fused_inputs(case, bias, act, seed)
    N, O, H, W = c["N"], c["O"], c["H"], c["W"]
    HW = H * W
    yh = forward(be, x, w, b)
    nan_y = np.isnan(yh)
    assert nan_y.any() and not nan_y.all(axis=(0, 2, 3)).any()
    # statistics of the finite part (the NaN pixel must not wipe out every channel)
    mean = np.nanmean(yh.astype(np.float64), axis=(0, 2, 3)).astype(F)
    invstd = (1.0 / np.sqrt(np.nanvar(yh.astype(np.float64), axis=(0, 2, 3)) + 1e-5)).astype(F)
    sv = np.stack([mean, invstd]).astype(F)
    c4 = lambda v: v.astype(F)[None, :, None, None]
    with np.errstate(invalid="ignore"):
        z = ((yh - c4(sv[0])) * c4(sv[1])) * c4(gamma) + c4(beta)
        assert z.dtype == F
        g = be.geom(x.shape, w.shape, padding=c["k"] // 2)
        dX, dW, dBi, dG, dB, dSV = be.to_dev(x), be.to_dev(w), (be.to_dev(b) if bias else None), be.to_dev(gamma), be.to_dev(beta), be.to_dev(sv)
        if act == 1:
            codes_ref = np.where(z < 0, -1, 1).astype(np.int8)
            lo_bits, hi_bits = (z > -1) & (z < 1), np.zeros_like(z, dtype=bool)
        else:
            dY, chan = be.to_dev(yh), be.empty((9, O))
            be.call("mn_qa_chan_from_save", be.ptr(dSV), be.ptr(dG), be.ptr(dB), O, be.ptr(chan), be.stream)
            cref = be.to_dev_u8(np.zeros((N, O, H, W), dtype=np.uint8))
            be.call("mn_qa_fwd", 1, be.ptr(dY), be.ptr(chan), N, O, H, W, bits, 0, be.ptr(cref), None, be.stream)
            codes_ref = be.to_host(cref)
            a = np.where(z > 0, z, 0).astype(F)
            t = a * F(0.1)
            lo_bits, hi_bits = z > 0, (z > 0) & (t >= 0) & (t <= 1)
    pack = lambda bts: (bts.reshape(N, O, HW // 4, 4) * np.array([1, 2, 4, 8])).sum(-1).astype(np.uint8)
    mask_ref = pack(lo_bits) | (pack(hi_bits) << 4)
    codes = be.to_dev_i8(np.full((N, O, H, W), 55, dtype=np.int8)) if act == 1 else be.to_dev_u8(np.full((N, O, H, W), 55, dtype=np.uint8))
    mask4 = be.to_dev_u8(np.full((N, O, HW // 4), 0xAA, dtype=np.uint8))
    be.call("mn_conv2d_first_bnact_fwd", C.byref(g), be.ptr(dX), be.ptr(dW), be.ptr(dBi), be.ptr(dSV), be.ptr(dG), be.ptr(dB), act, bits, be.ptr(codes), be.ptr(mask4),
            be.stream)
    assert be.lib.mn_last_kernel().decode() == "k_c1b_fwd<%d, %d>" % (MT_OF(O), act)
    ch, mh = be.to_host(codes), be.to_host(mask4)
    assert np.array_equal(ch, codes_ref), "codes: %d of %d differ" % (int((ch != codes_ref).sum()), ch.size)
    assert np.array_equal(mh, mask_ref), "pass nibbles: %d of %d bytes differ" % (int((mh != mask_ref).sum()), mh.size)
    # both code values / both nibble states occur: the comparison is not vacuous
    assert len(np.unique(ch)) >= 2 and len(np.unique(mh)) >= 2
