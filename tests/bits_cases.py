"""Bit-packed inference kernels (csrc/qgemm_bits.hip) through the C ABI: the same checks on the CPU emulation build and on the GPU.  Everything here is exact --
accumulators are integers and the decision is defined bit for bit as ``+1 iff not (fl(fl(acc * alpha) + b) < 0)`` (tests/kernel_cases.py:check_deployed_sign_block)."""
import ctypes as C

import numpy as np

from oracle import np_oracle as O
import kernel_cases as K

F = np.float32

# the seven quantised layers of nin_gc (models/nin_gc.py:62-147, cfg 256-256-256-512-512-512-1024-1024): (Cin, Cout, k, groups, input shuffle, map)
NIN_GC_LAYERS = [
    (256, 256, 1, 2, 0, 32), (256, 256, 1, 2, 2, 32), (256, 512, 3, 16, 2, 16), (512, 512, 1, 4, 16, 16), (512, 512, 1, 4, 4, 16), (512, 1024, 3, 32, 4, 8),
    (1024, 1024, 1, 8, 32, 8),
]


def nin_gc_case(i, full):
    """Layer i as a case dict; ``full``: N = 2 at the net's own map size, else (the emulator runs one fiber per GPU thread) N = 1 on an 8 x 8 / 8 x 16 cut."""
    cin, cout, k, g, sh, hw = NIN_GC_LAYERS[i]
    shape = (2, cin, hw, hw) if full else (1, cin, 8, 16 if i % 2 else 8)
    return dict(x_shape=shape, w_shape=(cout, cin // g, k, k), groups=g, in_shuffle=sh, padding=(k - 1) // 2)


# the grouped 3x3 layers of the small golden net (tests/golden/inference_meta.json: cfg 32-32-32-64-...): 2 channels per group
TWO_PER_GROUP = dict(x_shape=(2, 32, 8, 8), w_shape=(64, 2, 3, 3), groups=16, padding=1)


def _dev_i32(be, a):
    a = np.ascontiguousarray(a).view(np.int32)
    return a.copy() if be.kind == "emu" else be.torch.from_numpy(a.copy()).cuda()


def _empty_i32(be, shape):
    a = np.full(shape, 0x5a5a5a5a, dtype=np.int32)          # poison
    return a if be.kind == "emu" else be.torch.from_numpy(a).cuda()


def _host_u32(be, b):
    return be.to_host(b).view(np.uint32)


def np_pack(a):
    """[N, C, H, W] +-1 -> uint32 [N, ceil(C/32), H, W]: bit c & 31 of word c >> 5 is 1 iff +1, unused bits 0."""
    N, Cc, H, W = a.shape
    out = np.zeros((N, (Cc + 31) // 32, H, W), dtype=np.uint32)
    for c in range(Cc):
        out[:, c >> 5] |= (a[:, c] > 0).astype(np.uint32) << np.uint32(c & 31)
    return out


def np_unpack(bits, Cc):
    return np.stack([np.where((bits[:, c >> 5] >> np.uint32(c & 31)) & 1, 1, -1) for c in range(Cc)], axis=1).astype(np.int8)


def pack(be, a8):
    N, Cc, H, W = a8.shape
    bits = _empty_i32(be, (N, (Cc + 31) // 32, H, W))
    be.call("mn_bits_pack_sign8", be.ptr(be.to_dev_i8(a8)), N, Cc, H * W, be.ptr(bits), be.stream)
    return bits


def unpack(be, bits, Cc):
    N, _, H, W = bits.shape
    out = be.empty_i8((N, Cc, H, W))
    be.call("mn_bits_unpack_sign8", be.ptr(bits), N, Cc, H * W, be.ptr(out), be.stream)
    return be.to_host(out).view(np.int8)


def check_pack_roundtrip(be, Cc, seed=0):
    r = np.random.default_rng(seed)
    a = np.where(r.standard_normal((3, Cc, 4, 12)) > 0, 1, -1).astype(np.int8)
    bits = pack(be, a)
    got = _host_u32(be, bits)
    assert np.array_equal(got, np_pack(a)), "bit layout (incl. zero tail bits of the last word)"
    if Cc % 32:
        assert not (got[:, -1] >> np.uint32(Cc % 32)).any()
    assert np.array_equal(unpack(be, bits, Cc), a)


def make_inputs(x_shape, w_shape, groups=1, in_shuffle=0, padding=0, seed=0, W=3):
    """Inputs as check_deployed_sign_block builds them (every fifth bias 0: exact zeros of acc * alpha + b occur), plus an all-zero-weight channel (alpha = 0) and two
    channels whose bias makes the decision constant.  Returns (a_in physical codes, x_log logical codes, w, b, a_ref)."""
    r = np.random.default_rng(seed)
    N, Cin, H, Wd = x_shape
    Oc = w_shape[0]
    a_in = np.where(r.standard_normal(x_shape) > 0, 1, -1).astype(np.int8)
    w, _, _ = K.make_coded_weights(r, w_shape, 1)
    if W == 2:
        alpha = np.abs(w).reshape(Oc, -1).max(axis=1).reshape(-1, 1, 1, 1)
        w = np.where(w == 0, alpha, w).astype(F)
        assert (w != 0).all()
    else:
        assert (w == 0).any()
    b = (r.standard_normal(Oc) * 3.0).astype(F)
    b[::5] = 0
    w[1] = 0                                   # alpha = 0: the decision is sign(b[1]) everywhere
    b[2], b[3] = F(1e6), F(-1e6)               # constant +1 / constant -1
    x_log = a_in
    if in_shuffle > 1:
        x_log = np.ascontiguousarray(a_in.reshape(N, in_shuffle, Cin // in_shuffle, H, Wd).transpose(0, 2, 1, 3, 4).reshape(x_shape))
    acc = O.conv2d_fwd(x_log.astype(F), np.sign(w).astype(F), None, padding=padding, groups=groups)
    alpha = np.abs(w).reshape(Oc, -1).max(axis=1).astype(F)
    y = (acc.astype(F) * alpha.reshape(1, -1, 1, 1)).astype(F) + b.reshape(1, -1, 1, 1)
    a_ref = np.where(y.astype(F) < 0, -1, 1).astype(np.int8)
    assert (y == 0).any(), "the case must contain exact zeros of acc * alpha + b"
    return a_in, x_log, w, b, a_ref


def bitconv(be, x_log, w, b, groups, padding, out_order=None, pool=0):
    """pack the table, run mn_bitconv_fwd on pack(x_log); returns the unpacked output codes [N, O, Ho, Wo]."""
    g = be.geom(x_log.shape, w.shape, padding=padding, groups=groups)
    assert be.lib.mn_bitconv_supported(C.byref(g)) == 1, "geometry must be covered by the bit kernels"
    nb = int(be.lib.mn_bitconv_table_bytes(C.byref(g)))
    assert nb > 0 and nb % 4 == 0
    table = _empty_i32(be, (nb // 4,))
    order = _dev_i32(be, np.asarray(out_order, dtype=np.int32)) if out_order is not None else None
    dW, dB = be.to_dev(w), be.to_dev(b)
    be.call("mn_bitconv_pack", C.byref(g), be.ptr(dW), be.ptr(dB), be.ptr(order), be.ptr(table), be.stream)
    assert int(_host_u32(be, table)[0]) == 0, "every row's decision is monotone in acc"
    xb = pack(be, x_log)
    N, _, H, Wd = x_log.shape
    Ho, Wo = (H // 2, Wd // 2) if pool else (H, Wd)
    yb = _empty_i32(be, (N, (w.shape[0] + 31) // 32, Ho, Wo))
    be.call("mn_bitconv_fwd", C.byref(g), be.ptr(table), be.ptr(xb), be.ptr(yb), int(pool), be.stream)
    if w.shape[0] % 32:
        assert not (_host_u32(be, yb)[:, -1] >> np.uint32(w.shape[0] % 32)).any(), "unused bits of the last output word are 0"
    return unpack(be, yb, w.shape[0])


def check_bitconv(be, x_shape, w_shape, groups=1, in_shuffle=0, padding=0, seed=0, W=3):
    _, x_log, w, b, a_ref = make_inputs(x_shape, w_shape, groups, in_shuffle, padding, seed, W)
    got = bitconv(be, x_log, w, b, groups, padding)
    print("bitconv", x_shape, w_shape, "groups", groups, "W", W, "mismatches", int((got != a_ref).sum()), "of", got.size)
    assert np.array_equal(got, a_ref), (int((got != a_ref).sum()), got.size)


def check_order_and_pool(be, x_shape, w_shape, groups=1, in_shuffle=0, padding=0, seed=0, consumer_shuffle=4):
    """Consumer order: packed with a non-trivial out_order, the output equals the identity-order output with its channels permuted.  Pooled: equals max_pool2d of the
    un-pooled output (both orders)."""
    import torch
    _, x_log, w, b, a_ref = make_inputs(x_shape, w_shape, groups, in_shuffle, padding, seed, 3)
    Oc = w_shape[0]
    j = np.arange(Oc)
    order = (j % consumer_shuffle) * (Oc // consumer_shuffle) + j // consumer_shuffle          # what a consumer with in_shuffle_groups = consumer_shuffle reads at j
    ident = bitconv(be, x_log, w, b, groups, padding)
    assert np.array_equal(ident, a_ref)
    perm = bitconv(be, x_log, w, b, groups, padding, out_order=order)
    assert np.array_equal(perm, ident[:, order])
    # == channel_shuffle(ident, consumer_shuffle) (models/nin_gc.py:4-15)
    N, _, H, Wd = ident.shape
    shuf = ident.reshape(N, consumer_shuffle, Oc // consumer_shuffle, H, Wd).transpose(0, 2, 1, 3, 4).reshape(ident.shape)
    assert np.array_equal(perm, shuf)
    for oo, full in ((None, ident), (order, perm)):
        pooled = bitconv(be, x_log, w, b, groups, padding, out_order=oo, pool=1)
        ref = torch.nn.functional.max_pool2d(torch.from_numpy(full.astype(F)), 2, 2).numpy().astype(np.int8)
        assert np.array_equal(pooled, ref)


def check_byte_vs_bit(be, x_shape, w_shape, groups=1, in_shuffle=0, padding=0, seed=0, W=3):
    """GPU: the byte path (mn_qconv_bnsign_fwd_stash with identity statistics, as check_deployed_sign_block calls it) and the bit path on the same inputs."""
    a_in, x_log, w, b, a_ref = make_inputs(x_shape, w_shape, groups, in_shuffle, padding, seed, W)
    N, _, H, Wd = x_shape
    Oc = w_shape[0]
    g = be.geom(x_shape, w_shape, padding=padding, groups=groups)
    g.in_shuffle = in_shuffle
    wq = be.wq(mode=1)
    assert int(be.lib.mn_qconv_bnsign_stash_supported(C.byref(g), C.byref(wq))), "byte path must cover the geometry"
    nb = max(int(be.lib.mn_qconv_bnsign_stash_ws_bytes(C.byref(g))), 4 * int(be.lib.mn_bnsign_ws_floats(Oc)))
    ws = be.empty(nb // 4 + 8)
    one, zero = np.ones(Oc, dtype=F), np.zeros(Oc, dtype=F)
    dA, dW, dB = be.to_dev_i8(a_in), be.to_dev(w), be.to_dev(b)
    dG, dBe, dRM, dRV = be.to_dev(one), be.to_dev(zero), be.to_dev(zero), be.to_dev(one)
    save, a8 = be.empty((2, Oc)), be.empty_i8((N, Oc, H, Wd))
    h8, chan = be.empty_i8((N, Oc, H, Wd)), be.empty((int(be.lib.mn_qconv_bnsign_stash_chan_rows(C.byref(g))), Oc))
    be.call("mn_qconv_bnsign_fwd_stash", C.byref(g), C.byref(wq), be.ptr(dA), be.ptr(dW), be.ptr(dB), be.ptr(dG), be.ptr(dBe), 0.0, 0.0, 0,
            be.ptr(dRM), be.ptr(dRV), None, be.ptr(save), be.ptr(a8), be.ptr(h8), be.ptr(chan), be.ptr(ws), nb, be.stream)
    byte = be.to_host(a8).view(np.int8)
    bit = bitconv(be, x_log, w, b, groups, padding)
    print("byte vs bit", x_shape, w_shape, "byte!=ref", int((byte != a_ref).sum()), "bit!=ref", int((bit != a_ref).sum()))
    assert np.array_equal(bit, a_ref)
    assert np.array_equal(byte, bit), int((byte != bit).sum())
