"""The residual stages of the DoReFa W8A8 byte plan (csrc/qgemm_codes_w8_res.h: mn_code8_quant_map, mn_code8res_conv_*, mn_code8res_add_*) through the C ABI: one case
table for the CPU emulation build and the GPU.  The judge is plain numpy: the accumulators in int64 (np_oracle.conv2d_fwd with stride, asserted within int32), then the
fp32 chain step by step (codes_w8_cases.chain_codes, extended by a = max(z + r, 0)).  Bytes must be equal, fp32 outputs equal as bit patterns; output buffers are
poisoned before the launch, with a guard region behind them."""
import ctypes as C

import numpy as np

from oracle import np_oracle as O
from bits_cases import _empty_i32, _host_u32
from codes_cases import make_chan          # (both signs of gamma, gamma = 0, saturating channels, a rounding boundary on an attained value)
from codes_w8_cases import W8, from_map, to_map
from micronet_amd._lib import MN_EINVAL, MN_ENOTSUP

F = np.float32
GUARD = 64
# (id, x shape, O, KS, stride, seed)
CONVS = [
    ("k3s2_odd_borders", (1, 32, 5, 7), 24, 3, 2, 8600),          # odd sizes, every border, a partial output block
    ("k1s2_tail_channels", (1, 20, 5, 4), 16, 1, 2, 8601),        # C % 16 = 4
    ("k3s2_45_slots", (2, 80, 4, 4), 80, 3, 2, 8602),             # the last k-step holds one slot; two sets, two images
    ("k3s1_as_code8conv", (1, 32, 5, 3), 32, 3, 1, 8603),         # ... and equal to mn_code8conv_fwd on the same table
]
# (id, branch x shape, O, KS, shortcut kind, block input shape, shortcut stride, seed, every input code / every weight code or None)
ADDS = [
    ("identity", (1, 32, 5, 3), 32, 3, 1, None, 1, 8610, None),
    ("identity_two_sets", (2, 80, 4, 4), 80, 3, 1, None, 1, 8611, None),
    ("conv_s2", (1, 32, 3, 4), 24, 3, 2, (1, 20, 5, 7), 2, 8612, None),
    ("conv_s1_long_k", (1, 16, 2, 3), 80, 3, 2, (1, 272, 2, 3), 1, 8613, None),          # 17 shortcut slots: 5 k-steps, 3 padding slots
    ("saturated_255_against_0", (1, 32, 3, 4), 24, 3, 2, (1, 20, 5, 7), 2, 8612, (255, 0)),
    ("saturated_all_0", (1, 32, 3, 4), 24, 3, 2, (1, 20, 5, 7), 2, 8612, (0, 77)),
]
OUTS = [("bytes", True, False), ("f32", False, True), ("both", True, True)]
# conv geometries refused: (geometry keywords, widths)
REFUSED = [
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (4, 4, 4)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 16, 1, 1), groups=2), W8),
    (dict(x_shape=(1, 32, 9, 9), w_shape=(32, 32, 1, 1), stride=3), W8),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), W8),
    (dict(x_shape=(1, 20, 8, 8), w_shape=(32, 20, 3, 3), padding=1), W8),
]
# add stages refused: (branch x shape, O, branch stride, shortcut kind, block input shape, shortcut stride)
REFUSED_ADD = [
    ((1, 32, 4, 4), 48, 1, 1, None, 1),                   # an identity shortcut with O != C
    ((1, 32, 4, 4), 32, 1, 2, (1, 16, 4, 4), 2),          # the shortcut's map is 2 x 2, the branch's 4 x 4
    ((1, 32, 4, 4), 32, 2, 1, None, 1),                   # a strided branch conv
]


def make_inputs(x_shape, Oc, KS, stride, seed, fill=None):
    """(codes uint8, stored weights fp32 on the grid (2k - 255) / 255, exact accumulator int64 of the strided conv)."""
    r = np.random.default_rng(seed)
    codes = r.integers(0, 256, size=x_shape).astype(np.uint8)
    codes[:, :, 0, 0], codes[0, :, -1, -1] = 0, 255                      # a whole-zero pixel and a saturated one
    k = r.integers(0, 256, size=(Oc, x_shape[1], KS, KS)).astype(np.int64)
    if fill is not None:
        codes[:], k[:] = fill
    w = (F(2) * (k.astype(F) / F(255)) - F(1)).astype(F)                 # what the DoReFa weight quantizer stores
    acc = O.conv2d_fwd(codes.astype(np.int64), 2 * k - 255, None, stride=stride, padding=KS // 2, acc=np.int64)
    assert np.abs(acc).max() < 2 ** 31
    return codes, w, acc


def chain_z(acc, chan):
    """The fp32 chain of k_qa_fwd up to and including the BatchNorm, step by step."""
    alpha, bias, mean, invstd, ga, beb = (chan[i].reshape(1, -1, 1, 1) for i in range(6))
    y = (acc.astype(F) * alpha).astype(F) + bias
    zh = ((y - mean).astype(F) * invstd).astype(F)
    return ((zh * ga).astype(F) + beb).astype(F)


relu = lambda z: np.where(z > 0, z, F(0)).astype(F)


def codes_of(a):
    """The 8-bit DoReFa activation code of fp32 a: rha(clamp(0.1 a, 0, 1) / s), s = fl(1 / 255)."""
    c = np.minimum(np.maximum((a * F(0.1)).astype(F), F(0)), F(1)).astype(F)
    return np.floor(((c / (F(1) / F(255))).astype(F) + F(0.5)).astype(F)).astype(np.uint8)


def pack_table(be, g, w, chan):
    nb = int(be.lib.mn_code8res_conv_table_bytes(C.byref(g), *W8))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    dW, dC = be.to_dev(w), be.to_dev(chan)
    be.call("mn_code8res_conv_pack", C.byref(g), be.ptr(dW), be.ptr(dC), 8, 8, 8, be.ptr(table), be.stream)
    hdr = _host_u32(be, table)
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0, "finite constants, weights on the grid"
    return table


def guarded_map(be, N, Cc, HW):
    size = N * ((Cc + 15) // 16) * HW * 16
    return be.empty_i8((size + GUARD,)), size


def read_map(be, buf, size, N, Cc, H, W):
    got = be.to_host(buf).view(np.uint8)
    assert (got[size:] == 77).all(), "the guard behind the map is intact"
    return from_map(got[:size].reshape(N, -1, H * W, 16), ((Cc + 15) // 16) * 16, H, W)


def check_quant(be, Cc=20):
    r = np.random.default_rng(8590)
    x = (r.standard_normal((3, Cc, 3, 5)) * 6).astype(F)          # negatives, values > 10
    x[0, :, 0, 0] = (F(10) * (np.arange(Cc, dtype=F) * 12 + F(0.5)) / F(255)).astype(F)          # on (or an ulp beside) the half-steps
    want = codes_of(x)
    assert (x < 0).any() and (x > 10).any() and len(np.unique(want)) > 32
    (buf, size), dX = guarded_map(be, 3, Cc, 15), be.to_dev(x)
    be.call("mn_code8_quant_map", be.ptr(dX), 3, Cc, 15, be.ptr(buf), be.stream)
    got = read_map(be, buf, size, 3, Cc, 3, 5)
    assert be.lib.mn_last_kernel().decode() == "k_code8_quant"
    assert np.array_equal(got[:, :Cc], want) and (got[:, Cc:] == 0).all(), "the codes of the judge; tail channels the code 0"


def check_conv(be, idx):
    cid, x_shape, Oc, KS, stride, seed = CONVS[idx]
    codes, w, acc = make_inputs(x_shape, Oc, KS, stride, seed)
    chan = make_chan(acc, seed)
    ref = codes_of(relu(chain_z(acc, chan)))
    g = be.geom(x_shape, w.shape, stride=stride, padding=KS // 2)
    assert be.lib.mn_code8res_conv_supported(C.byref(g), *W8) == 1
    table, dX = pack_table(be, g, w, chan), be.to_dev_u8(to_map(codes))
    N, (Ho, Wo) = x_shape[0], acc.shape[2:]
    buf, size = guarded_map(be, N, Oc, Ho * Wo)
    be.call("mn_code8res_conv_fwd", C.byref(g), be.ptr(table), be.ptr(dX), be.ptr(buf), be.stream)
    name, got = be.lib.mn_last_kernel().decode(), read_map(be, buf, size, N, Oc, Ho, Wo)
    bad = int((got[:, :Oc] != ref).sum())
    print(name, cid, "mismatches against the judge", bad, "of", ref.size, "distinct codes", len(np.unique(ref)))
    assert name == "k_code8res_conv<%d,%d>" % (KS, stride) and bad == 0 and (got[:, Oc:] == 0).all()
    assert len(np.unique(ref)) > 16 and (acc[:, 4] == int(chan[2, 4])).any() and (acc[:, 5] == int(chan[2, 5])).any() and chan[4, 3] < 0
    if stride == 1:          # the same table under the hidden blocks' kernel: byte for byte
        other = be.empty_i8((size,))
        be.call("mn_code8conv_fwd", C.byref(g), be.ptr(table), be.ptr(dX), be.ptr(other), 0, be.stream)
        assert np.array_equal(be.to_host(other).view(np.uint8), be.to_host(buf).view(np.uint8)[:size])


def check_add(be, arg):
    idx, (oid, want_b, want_f) = arg
    cid, x_shape, Oc, KS, sc, s_shape, s_stride, seed, fill = ADDS[idx]
    codes, w, acc = make_inputs(x_shape, Oc, KS, 1, seed, fill)
    chan = make_chan(acc, seed)
    N, _, H, Wd = x_shape
    g, gs, res, ts, dS = be.geom(x_shape, w.shape, padding=KS // 2), None, None, None, None
    if sc == 1:
        r = (np.random.default_rng(seed + 1).standard_normal((N, Oc, H, Wd)) * 3).astype(F)
        res = be.to_dev(r)
    else:
        codes_s, w_s, acc_s = make_inputs(s_shape, Oc, 1, s_stride, seed + 1, fill)
        chan_s = make_chan(acc_s, seed + 1)
        assert acc_s.shape == acc.shape
        r = chain_z(acc_s, chan_s)
        gs = be.geom(s_shape, w_s.shape, stride=s_stride)
        ts, dS = pack_table(be, gs, w_s, chan_s), be.to_dev_u8(to_map(codes_s))
    a = relu((chain_z(acc, chan) + r).astype(F))
    assert be.lib.mn_code8res_add_supported(C.byref(g), sc, C.byref(gs) if gs is not None else None, *W8) == 1
    table, dX = pack_table(be, g, w, chan), be.to_dev_u8(to_map(codes))
    (bbuf, size), fbuf = guarded_map(be, N, Oc, H * Wd), be.empty((a.size + GUARD,))
    be.call("mn_code8res_add_fwd", C.byref(g), be.ptr(table), be.ptr(dX), sc, be.ptr(res), C.byref(gs) if gs is not None else None, be.ptr(ts),
            be.ptr(dS), be.ptr(bbuf) if want_b else None, be.ptr(fbuf) if want_f else None, be.stream)
    name, gb, gf = be.lib.mn_last_kernel().decode(), be.to_host(bbuf).view(np.uint8), be.to_host(fbuf)
    assert name == "k_code8res_add<%d,%d>" % (KS, sc)
    ref = codes_of(a)
    if want_b:
        got = read_map(be, bbuf, size, N, Oc, H, Wd)
        print(name, cid, oid, "byte mismatches", int((got[:, :Oc] != ref).sum()), "of", ref.size, "distinct codes", len(np.unique(ref)))
        assert np.array_equal(got[:, :Oc], ref) and (got[:, Oc:] == 0).all()
    else:
        assert (gb == 77).all(), "an output that was not requested is not written"
    if want_f:
        print(name, cid, oid, "fp32 bit mismatches", int((gf[:a.size].view(np.uint32) != a.ravel().view(np.uint32)).sum()), "of", a.size)
        assert np.array_equal(gf[:a.size].view(np.uint32), a.ravel().view(np.uint32)) and (gf[a.size:] == F(-1234.5)).all()
    else:
        assert (gf == F(-1234.5)).all(), "an output that was not requested is not written"
    if fill is None:
        assert len(np.unique(ref)) > 16 and (a == 0).any() and (a > 10).any()
    else:          # a 3 x 4 map: an interior pixel sees 9 x 32 positions, a corner 4 x 32; the shortcut 20 channels at every pixel
        ext = (int(acc.min()), int(acc.max()), int(acc_s.min()), int(acc_s.max()))
        assert ext == ((-255 * 255 * 288, -255 * 255 * 128, -255 * 255 * 20, -255 * 255 * 20) if fill[0] else (0, 0, 0, 0))


def check_refused(be, idx):
    """MN_ENOTSUP from every entry of a geometry that is not covered; the poisoned buffer stays as it was."""
    buf, f = _empty_i32(be, (64,)), be.to_dev(np.zeros(64, dtype=F))
    if idx < len(REFUSED):
        kw, (ai, wb, ao) = REFUSED[idx]
        g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), groups=kw.get("groups", 1))
        assert be.lib.mn_code8res_conv_supported(C.byref(g), ai, wb, ao) == 0 and int(be.lib.mn_code8res_conv_table_bytes(C.byref(g), ai, wb, ao)) == 0
        assert be.lib.mn_code8res_conv_pack(C.byref(g), be.ptr(f), be.ptr(f), ai, wb, ao, be.ptr(buf), be.stream) == MN_ENOTSUP
        assert be.lib.mn_code8res_add_supported(C.byref(g), 0, None, ai, wb, ao) == 0
        if (ai, wb, ao) == W8:          # (the forwards take no widths)
            assert be.lib.mn_code8res_conv_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), be.stream) == MN_ENOTSUP
            assert be.lib.mn_code8res_add_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), 0, None, None, None, None, be.ptr(buf), None, be.stream) == MN_ENOTSUP
    else:
        x_shape, Oc, stride, sc, s_shape, s_stride = REFUSED_ADD[idx - len(REFUSED)]
        g = be.geom(x_shape, (Oc, x_shape[1], 3, 3), stride=stride, padding=1)
        gs = be.geom(s_shape, (Oc, s_shape[1], 1, 1), stride=s_stride) if s_shape else None
        pgs = C.byref(gs) if gs is not None else None
        assert be.lib.mn_code8res_conv_supported(C.byref(g), *W8) == 1 and be.lib.mn_code8res_add_supported(C.byref(g), sc, pgs, *W8) == 0
        assert be.lib.mn_code8res_add_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), sc, be.ptr(f), pgs, be.ptr(buf), be.ptr(buf), be.ptr(buf), None, be.stream) == MN_ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_invalid(be, _=None):
    """MN_EINVAL: a null table, a misaligned map, no output requested, a null residual."""
    g = be.geom((1, 32, 4, 4), (32, 32, 3, 3), padding=1)
    buf, out, f = _empty_i32(be, (4096,)), _empty_i32(be, (4096,)), be.to_dev(np.zeros(1024, dtype=F))
    p, o, odd = be.ptr(buf), be.ptr(out), be.ptr_at(out, 1)
    add = be.lib.mn_code8res_add_fwd
    assert be.lib.mn_code8_quant_map(be.ptr(f), 1, 32, 16, odd, be.stream) == MN_EINVAL and be.lib.mn_code8_quant_map(None, 1, 32, 16, o, be.stream) == MN_EINVAL
    assert be.lib.mn_code8res_conv_fwd(C.byref(g), None, p, o, be.stream) == MN_EINVAL and be.lib.mn_code8res_conv_fwd(C.byref(g), p, p, odd, be.stream) == MN_EINVAL
    assert add(C.byref(g), None, p, 0, None, None, None, None, o, None, be.stream) == MN_EINVAL
    assert add(C.byref(g), p, p, 0, None, None, None, None, odd, None, be.stream) == MN_EINVAL
    assert add(C.byref(g), p, p, 0, None, None, None, None, None, None, be.stream) == MN_EINVAL, "no output requested"
    assert add(C.byref(g), p, p, 1, None, None, None, None, o, None, be.stream) == MN_EINVAL, "an identity shortcut without its residual"
    assert add(C.byref(g), p, p, 2, None, None, None, None, o, None, be.stream) == MN_EINVAL, "a conv shortcut without its table"
    assert (_host_u32(be, out) == 0x5a5a5a5a).all(), "an invalid call writes nothing"


# (id, check, argument) for the two drivers: tests/test_code8_res_emulated.py, tests/test_gpu_code8_res.py
CHECKS = ([("quant_map", check_quant, 20)] + [(c[0], check_conv, i) for i, c in enumerate(CONVS)]
          + [("add_%s_%s" % (c[0], o[0]), check_add, (i, o)) for i, c in enumerate(ADDS) for o in OUTS]
          + [("refused%d" % i, check_refused, i) for i in range(len(REFUSED) + len(REFUSED_ADD))] + [("invalid", check_invalid, None)])
