"""The residual stages of the DoReFa W2A2 code plan (csrc/qgemm_codes_res.h: mn_coderes_quant_map, mn_coderes_conv_*, mn_coderes_add_*) through the C ABI: one case
table for the CPU emulation build and the GPU.  The judge is plain numpy: the accumulators in int64 (np_oracle.conv2d_fwd with stride, asserted within int32), then the
fp32 chain step by step (code8_res_cases.chain_z), a = max(z + r, 0), then the 2-bit code.  Planes must be equal word for word, tail bits included, fp32 outputs equal as
bit patterns; output buffers are poisoned before the launch, with a guard region behind them."""
import ctypes as C

import numpy as np

from oracle import np_oracle as O
from bits_cases import _dev_i32, _empty_i32, _host_u32
from codes_cases import make_chan, np_pack_planes          # (both signs of gamma, gamma = 0, saturating channels, a rounding boundary on an attained value)
from code8_res_cases import GUARD, OUTS, REFUSED, REFUSED_ADD, chain_z, relu
from micronet_amd._lib import MN_EINVAL, MN_ENOTSUP

F = np.float32
W2 = (2, 2, 2)
POISON = 0x5a5a5a5a
# (id, x shape, O, KS, stride, seed)
CONVS = [
    ("k3s2_odd_borders", (1, 32, 5, 7), 24, 3, 2, 8700),          # odd sizes, every border, a partial output word
    ("k1s2_tail_channels", (1, 20, 5, 4), 16, 1, 2, 8701),        # C % 16 = 4
    ("k3s2_45_slots", (2, 80, 4, 4), 80, 3, 2, 8702),             # the last k-step holds one slot; two and a half output words (two spans); two images
    ("k3s1", (1, 32, 5, 3), 32, 3, 1, 8703),
    ("k3s1_k41472", (1, 512, 2, 2), 16, 3, 1, 8704),              # K * 9 = 41472: beyond the 32767 of the threshold kernels
]
# (id, branch x shape, O, KS, shortcut kind, block input shape, shortcut stride, seed, every input code / every weight code or None)
ADDS = [
    ("identity", (1, 32, 5, 3), 32, 3, 1, None, 1, 8710, None),
    ("identity_two_spans", (2, 80, 4, 4), 80, 3, 1, None, 1, 8711, None),
    ("conv_s2", (1, 32, 3, 4), 24, 3, 2, (1, 20, 5, 7), 2, 8712, None),
    ("conv_s1_long_k", (1, 16, 2, 3), 80, 3, 2, (1, 272, 2, 3), 1, 8713, None),          # 17 shortcut slots: 5 k-steps, 3 padding slots
    ("saturated_3_against_0", (1, 32, 3, 4), 24, 3, 2, (1, 20, 5, 7), 2, 8712, (3, 0)),
    ("saturated_all_0", (1, 32, 3, 4), 24, 3, 2, (1, 20, 5, 7), 2, 8712, (0, 2)),
]
# the byte cases' refused geometries at widths (2, 2, 2) -- the one they refuse for its width alone is covered here -- and two covered geometries at other widths
REFUSED2 = [(kw, W2) for kw, w in REFUSED if w != (4, 4, 4)] + [(REFUSED[0][0], (4, 4, 4)), (REFUSED[0][0], (8, 8, 8))]


def make_inputs(x_shape, Oc, KS, stride, seed, fill=None):
    """(codes uint8 in 0 .. 3, stored weights fp32 on the grid (2k - 3) / 3, exact accumulator int64 of the strided conv)."""
    r = np.random.default_rng(seed)
    codes = r.integers(0, 4, size=x_shape).astype(np.uint8)
    codes[:, :, 0, 0], codes[0, :, -1, -1] = 0, 3                        # a whole-zero pixel and a saturated one
    k = r.integers(0, 4, size=(Oc, x_shape[1], KS, KS)).astype(np.int64)
    if fill is not None:
        codes[:], k[:] = fill
    w = (F(2) * (k.astype(F) / F(3)) - F(1)).astype(F)                   # what the DoReFa weight quantizer stores
    acc = O.conv2d_fwd(codes.astype(np.int64), 2 * k - 3, None, stride=stride, padding=KS // 2, acc=np.int64)
    assert np.abs(acc).max() < 2 ** 31
    return codes, w, acc


def codes_of(a):
    """The 2-bit DoReFa activation code of fp32 a: rha(clamp(0.1 a, 0, 1) / s), s = fl(1 / 3)."""
    c = np.minimum(np.maximum((a * F(0.1)).astype(F), F(0)), F(1)).astype(F)
    return np.floor(((c / (F(1) / F(3))).astype(F) + F(0.5)).astype(F)).astype(np.uint8)


def pack_table(be, g, w, chan):
    nb = int(be.lib.mn_coderes_conv_table_bytes(C.byref(g), *W2))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    dW, dC = be.to_dev(w), be.to_dev(chan)
    be.call("mn_coderes_conv_pack", C.byref(g), be.ptr(dW), be.ptr(dC), 2, 2, 2, be.ptr(table), be.stream)
    hdr = _host_u32(be, table)
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0, "finite constants, weights on the grid"
    return table


def guarded_planes(be, N, Cc, HW):
    size = N * ((Cc + 31) // 32) * 2 * HW
    return _empty_i32(be, (size + GUARD,)), size


def read_planes(be, buf, size, shape):
    got = _host_u32(be, buf)
    assert (got[size:] == POISON).all(), "the guard behind the map is intact"
    return got[:size].reshape(shape)


def check_quant(be, Cc=20):
    r = np.random.default_rng(8690)
    x = (r.standard_normal((3, Cc, 3, 5)) * 6).astype(F)          # negatives, values > 10
    x[0, :, 0, 0] = (F(10) * (np.arange(Cc, dtype=F) % 3 + F(0.5)) / F(3)).astype(F)          # on (or an ulp beside) the half-steps
    want = np_pack_planes(codes_of(x))
    assert (x < 0).any() and (x > 10).any() and len(np.unique(codes_of(x))) == 4
    (buf, size), dX = guarded_planes(be, 3, Cc, 15), be.to_dev(x)
    be.call("mn_coderes_quant_map", be.ptr(dX), 3, Cc, 15, be.ptr(buf), be.stream)
    got = read_planes(be, buf, size, want.shape)
    assert be.lib.mn_last_kernel().decode() == "k_coderes_quant"
    assert np.array_equal(got, want), "the planes of the judge's codes; tail channels 0 bits"


def check_conv(be, idx):
    cid, x_shape, Oc, KS, stride, seed = CONVS[idx]
    codes, w, acc = make_inputs(x_shape, Oc, KS, stride, seed)
    chan = make_chan(acc, seed)
    ref = codes_of(relu(chain_z(acc, chan)))
    want = np_pack_planes(ref)
    g = be.geom(x_shape, w.shape, stride=stride, padding=KS // 2)
    assert be.lib.mn_coderes_conv_supported(C.byref(g), *W2) == 1
    table, dX = pack_table(be, g, w, chan), _dev_i32(be, np_pack_planes(codes))
    buf, size = guarded_planes(be, x_shape[0], Oc, acc.shape[2] * acc.shape[3])
    be.call("mn_coderes_conv_fwd", C.byref(g), be.ptr(table), be.ptr(dX), be.ptr(buf), be.stream)
    name, got = be.lib.mn_last_kernel().decode(), read_planes(be, buf, size, want.shape)
    print(name, cid, "word mismatches against the judge", int((got != want).sum()), "of", want.size, "distinct codes", len(np.unique(ref)))
    assert name == "k_coderes_conv<%d,%d>" % (KS, stride) and np.array_equal(got, want)
    assert len(np.unique(ref)) == 4 and (acc[:, 4] == int(chan[2, 4])).any() and (acc[:, 5] == int(chan[2, 5])).any() and chan[4, 3] < 0
    assert KS * KS * x_shape[1] * 9 <= 32767 or cid == "k3s1_k41472"


def check_add(be, arg):
    idx, (oid, want_p, want_f) = arg
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
        ts, dS = pack_table(be, gs, w_s, chan_s), _dev_i32(be, np_pack_planes(codes_s))
    a = relu((chain_z(acc, chan) + r).astype(F))
    pgs = C.byref(gs) if gs is not None else None
    assert be.lib.mn_coderes_add_supported(C.byref(g), sc, pgs, *W2) == 1
    table, dX = pack_table(be, g, w, chan), _dev_i32(be, np_pack_planes(codes))
    (pbuf, size), fbuf = guarded_planes(be, N, Oc, H * Wd), be.empty((a.size + GUARD,))
    be.call("mn_coderes_add_fwd", C.byref(g), be.ptr(table), be.ptr(dX), sc, be.ptr(res), pgs, be.ptr(ts), be.ptr(dS), be.ptr(pbuf) if want_p else None,
            be.ptr(fbuf) if want_f else None, be.stream)
    name, gf = be.lib.mn_last_kernel().decode(), be.to_host(fbuf)
    assert name == "k_coderes_add<%d,%d>" % (KS, sc)
    ref = codes_of(a)
    want = np_pack_planes(ref)
    got = read_planes(be, pbuf, size, want.shape)
    if want_p:
        print(name, cid, oid, "word mismatches", int((got != want).sum()), "of", want.size, "distinct codes", len(np.unique(ref)))
        assert np.array_equal(got, want)
    else:
        assert (got == POISON).all(), "an output that was not requested is not written"
    if want_f:
        print(name, cid, oid, "fp32 bit mismatches", int((gf[:a.size].view(np.uint32) != a.ravel().view(np.uint32)).sum()), "of", a.size)
        assert np.array_equal(gf[:a.size].view(np.uint32), a.ravel().view(np.uint32)) and (gf[a.size:] == F(-1234.5)).all()
    else:
        assert (gf == F(-1234.5)).all(), "an output that was not requested is not written"
    if fill is None:
        assert len(np.unique(ref)) == 4 and (a == 0).any() and (a > 10).any()
    else:          # a 3 x 4 map: an interior pixel sees 9 x 32 positions, a corner 4 x 32; the shortcut 20 channels at every pixel
        ext = (int(acc.min()), int(acc.max()), int(acc_s.min()), int(acc_s.max()))
        assert ext == ((-9 * 288, -9 * 128, -9 * 20, -9 * 20) if fill[0] else (0, 0, 0, 0))


def check_refused(be, idx):
    """MN_ENOTSUP from every entry of a geometry or width that is not covered; the poisoned buffer stays as it was."""
    buf, f = _empty_i32(be, (64,)), be.to_dev(np.zeros(64, dtype=F))
    p = be.ptr(buf)
    if idx < len(REFUSED2):
        kw, (ai, wb, ao) = REFUSED2[idx]
        g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), groups=kw.get("groups", 1))
        assert be.lib.mn_coderes_conv_supported(C.byref(g), ai, wb, ao) == 0 and int(be.lib.mn_coderes_conv_table_bytes(C.byref(g), ai, wb, ao)) == 0
        assert be.lib.mn_coderes_conv_pack(C.byref(g), be.ptr(f), be.ptr(f), ai, wb, ao, p, be.stream) == MN_ENOTSUP
        assert be.lib.mn_coderes_add_supported(C.byref(g), 1, None, ai, wb, ao) == 0
        if (ai, wb, ao) == W2:          # (the forwards take no widths)
            assert be.lib.mn_coderes_conv_fwd(C.byref(g), p, p, p, be.stream) == MN_ENOTSUP
            assert be.lib.mn_coderes_add_fwd(C.byref(g), p, p, 1, be.ptr(f), None, None, None, p, None, be.stream) == MN_ENOTSUP
    else:
        x_shape, Oc, stride, sc, s_shape, s_stride = REFUSED_ADD[idx - len(REFUSED2)]
        g = be.geom(x_shape, (Oc, x_shape[1], 3, 3), stride=stride, padding=1)
        gs = be.geom(s_shape, (Oc, s_shape[1], 1, 1), stride=s_stride) if s_shape else None
        pgs = C.byref(gs) if gs is not None else None
        assert be.lib.mn_coderes_conv_supported(C.byref(g), *W2) == 1 and be.lib.mn_coderes_add_supported(C.byref(g), sc, pgs, *W2) == 0
        assert be.lib.mn_coderes_add_fwd(C.byref(g), p, p, sc, be.ptr(f), pgs, p, p, p, None, be.stream) == MN_ENOTSUP
    assert (_host_u32(be, buf) == POISON).all(), "a refused call writes nothing"


def check_invalid(be, _=None):
    """MN_EINVAL: a null table, a misaligned map, no output requested, a null residual, a conv shortcut without its table."""
    g = be.geom((1, 32, 4, 4), (32, 32, 3, 3), padding=1)
    buf, out, f = _empty_i32(be, (4096,)), _empty_i32(be, (4096,)), be.to_dev(np.zeros(1024, dtype=F))
    p, o, r = be.ptr(buf), be.ptr(out), be.ptr(f)
    odd = C.c_void_p(o.value + 2)          # (plane maps are 4-byte aligned)
    add = be.lib.mn_coderes_add_fwd
    assert be.lib.mn_coderes_quant_map(r, 1, 32, 16, odd, be.stream) == MN_EINVAL and be.lib.mn_coderes_quant_map(None, 1, 32, 16, o, be.stream) == MN_EINVAL
    assert be.lib.mn_coderes_conv_fwd(C.byref(g), None, p, o, be.stream) == MN_EINVAL and be.lib.mn_coderes_conv_fwd(C.byref(g), p, p, odd, be.stream) == MN_EINVAL
    assert be.lib.mn_coderes_conv_fwd(C.byref(g), be.ptr_at(buf, 1), p, o, be.stream) == MN_EINVAL, "a table that is not 16-byte aligned"
    assert add(C.byref(g), None, p, 1, r, None, None, None, o, None, be.stream) == MN_EINVAL
    assert add(C.byref(g), p, p, 1, r, None, None, None, odd, None, be.stream) == MN_EINVAL
    assert add(C.byref(g), p, p, 1, r, None, None, None, None, None, be.stream) == MN_EINVAL, "no output requested"
    assert add(C.byref(g), p, p, 1, None, None, None, None, o, None, be.stream) == MN_EINVAL, "an identity shortcut without its residual"
    assert add(C.byref(g), p, p, 2, None, None, None, None, o, None, be.stream) == MN_EINVAL, "a conv shortcut without its table"
    assert (_host_u32(be, out) == POISON).all(), "an invalid call writes nothing"


# (id, check, argument) for the two drivers: tests/test_coderes_emulated.py, tests/test_gpu_coderes.py
CHECKS = ([("quant_map", check_quant, 20)] + [(c[0], check_conv, i) for i, c in enumerate(CONVS)]
          + [("add_%s_%s" % (c[0], o[0]), check_add, (i, o)) for i, c in enumerate(ADDS) for o in OUTS]
          + [("refused%d" % i, check_refused, i) for i in range(len(REFUSED2) + len(REFUSED_ADD))] + [("invalid", check_invalid, None)])
