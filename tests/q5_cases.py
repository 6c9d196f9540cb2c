"""The dense 5x5 / padding 2 block on DoReFa activation codes (k_q5_fwd, csrc/qgemm_q5.h; k_kk_wgrad<1, 25, MN_ACTQ_CODE8>) through the C ABI: one case table for the
CPU emulation build and the GPU.  Every case is judged by kernel_cases.check_qconv_bnq (an fp64 numpy / torch chain, nothing of the code under test): stash == the
integer conv bit for bit, statistics, mn_qa_* on the stash, dx / dw / dbias within 1e-5 of the fp64 maximum."""
import ctypes as C

import numpy as np

import kernel_cases as K

# (x shape, output channels, keyword settings)
CASES = [
    ((2, 16, 8, 8), 16, dict(a_bits=2, w_bits=2)),                                   # one chunk: 25 slots, the last k-step = 1 real + 3 zero slots; int16 stash
    ((5, 16, 8, 8), 16, dict(a_bits=2, w_bits=2)),                                   # 4 images per tile, the last tile partial, image boundaries inside a tile
    ((2, 96, 16, 16), 32, dict(a_bits=4, w_bits=4)),                                 # nin's layer: one image per tile, 6 chunks, 150 slots = 37.5 k-steps, int32
    ((1, 32, 32, 32), 16, dict(a_bits=2, w_bits=2)),                                 # bands of 8 rows with halos between them
    ((2, 96, 16, 16), 16, dict(a_bits=2, w_bits=2, training=False, bias=False)),     # eval mode, no bias; 96 * 25 * 9 = 21600: int16
    ((2, 16, 16, 16), 16, dict(a_bits=7, w_bits=7)),                                 # widest operands, acc beyond 2^22
    ((2, 32, 4, 8), 48, dict(a_bits=2, w_bits=2)),                                   # two channel sets per block, the second half empty
    ((3, 48, 8, 16), 32, dict(a_bits=3, w_bits=5, out_bits=2)),                      # mixed widths
]
IDS = ["%dx%dx%dx%d-o%d-%s" % (s + (o, "".join("%s%s" % (k[0], int(v)) for k, v in sorted(kw.items())))) for s, o, kw in CASES]


def check(be, x_shape, Oc, kw):
    names, call = [], be.call

    def spy(name, *args):          # the kernel behind mn_qconv_bnq_fwd_stash, read right after the call: a case cannot pass by another route
        call(name, *args)
        if name == "mn_qconv_bnq_fwd_stash":
            names.append(be.lib.mn_last_kernel().decode())
    be.call = spy
    try:
        K.check_qconv_bnq(be, x_shape, (Oc, x_shape[1], 5, 5), padding=2, seed=5500 + Oc + x_shape[1], **kw)
    finally:
        del be.call
    assert len(names) == 1 and names[0].startswith("k_q5_fwd"), names


def _launch(be, codes, w, a_bits, w_bits, padding=2, groups=1, stride=1):
    """mn_qconv_bnq_fwd_stash on (codes, w): (rc, stash as integers or None, name of the kernel)."""
    N, Cc, H, W = codes.shape
    Oc = w.shape[0]
    g, wq = be.geom(codes.shape, w.shape, stride=stride, padding=padding, groups=groups), be.wq(mode=2, bits=w_bits)
    ok = be.lib.mn_qconv_bnq_supported(C.byref(g), C.byref(wq), a_bits)
    sbits = int(be.lib.mn_qconv_bnq_stash_bits(C.byref(g), C.byref(wq), a_bits)) or 32
    nb = max(int(be.lib.mn_qconv_bnq_ws_bytes(C.byref(g))), 1 << 16)
    ws, save, chan, nbt = be.empty(nb // 4 + 8), be.empty((2, Oc)), be.empty((9, Oc)), be.to_dev_i64([0])
    one, zero = be.to_dev(np.ones(Oc, K.F)), be.to_dev(np.zeros(Oc, K.F))
    rm, rv = be.to_dev(np.zeros(Oc, K.F)), be.to_dev(np.ones(Oc, K.F))
    stash = be.empty_i8((N, Oc, H, (sbits // 8) * W))
    dX, dW = be.to_dev_u8(codes), be.to_dev(w)
    rc = be.lib.mn_qconv_bnq_fwd_stash(C.byref(g), C.byref(wq), be.ptr(dX), a_bits, be.ptr(dW), None, be.ptr(one), be.ptr(zero), 1e-5, 0.1, 1,
                                       be.ptr(rm), be.ptr(rv), be.ptr(nbt), be.ptr(save), be.ptr(stash), be.ptr(chan), be.ptr(ws), nb, be.stream)
    st = be.to_host(stash).view(np.int16 if sbits == 16 else np.int32).reshape(N, Oc, H, W) if rc == 0 else None
    return ok, rc, st, be.lib.mn_last_kernel().decode()


def check_extremes(be, Cc=32, a_bits=7, w_bits=7):
    """All codes n_a, all weights +1 (code n_w): interior = C 25 n_a n_w, corner = C 9 n_a n_w -- sign, offset and halo at the extremes."""
    na, nw = 2 ** a_bits - 1, 2 ** w_bits - 1
    ok, rc, st, name = _launch(be, np.full((1, Cc, 8, 8), na, np.uint8), np.ones((16, Cc, 5, 5), K.F), a_bits, w_bits)
    assert ok == 1 and rc == 0 and name.startswith("k_q5_fwd"), (ok, rc, name)
    assert st[0, :, 3, 4].tolist() == [Cc * 25 * na * nw] * 16 and st[0, :, 0, 0].tolist() == [Cc * 9 * na * nw] * 16 and st[0, :, 7, 7].tolist() == [Cc * 9 * na * nw] * 16


def check_refused(be):
    """8-bit operands, C no multiple of 16, groups, stride and another padding keep today's route: supported == 0, MN_ENOTSUP."""
    for Cc, kw in ((16, dict(a_bits=8)), (16, dict(w_bits=8)), (24, {}), (32, dict(groups=2)), (16, dict(stride=2)), (16, dict(padding=1))):
        a, wb, gr = kw.pop("a_bits", 4), kw.pop("w_bits", 4), kw.get("groups", 1)
        ok, rc, _, _ = _launch(be, np.zeros((2, Cc, 8, 8), np.uint8), np.ones((16, Cc // gr, 5, 5), K.F), a, wb, **kw)
        assert ok == 0 and rc == -95, (Cc, kw, ok, rc)          # MN_ENOTSUP
