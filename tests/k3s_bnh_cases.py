"""Grouped 3 x 3 binary block: backward-data / backward-weight that form dy from (da, h) themselves (k_k3s_dgrad<1>, k_k3s_wgrad<0, 1>) against the two-step
path (mn_bnh_bwd_apply writing dy, then the plain kernels) -- bit for bit -- and against an fp64 evaluation.  Backend-agnostic (emulator / GPU)."""
import ctypes as C

import numpy as np

import kernel_cases as K
from oracle import np_oracle as O

F = np.float32

# nin_gc layers 4 / 7 scaled down (Cg 16, Mg 32; 16 x 16 and 8 x 8 maps), one ragged geometry (Mg = Cg = 24: padded rows, a half-empty channel tile)
CASES = [
    dict(x_shape=(5, 32, 8, 8), w_shape=(64, 16, 3, 3), groups=2),             # two images per stage, odd N: the last stage is half clamped; 10 steps over 2 splits
    dict(x_shape=(3, 32, 16, 16), w_shape=(64, 16, 3, 3), groups=2),           # one image per stage; 24 steps over 6 splits
    dict(x_shape=(5, 48, 8, 8), w_shape=(48, 24, 3, 3), groups=2),             # ragged
    dict(x_shape=(5, 32, 8, 8), w_shape=(64, 16, 3, 3), groups=2, training=False),      # k1 = k2 = 0
]
# enough images that a backward-data block walks more than one stage (its grid is capped at 512 blocks) and a backward-weight wave more than two steps
CASE_LONG = dict(x_shape=(132, 128, 8, 8), w_shape=(256, 16, 3, 3), groups=8)


def check(be, x_shape, w_shape, groups, training=True, seed=0):
    r = np.random.default_rng(seed)
    N, Cin, H, W = x_shape
    Oc = w_shape[0]
    a_in = np.where(r.standard_normal(x_shape) > 0, 1, -1).astype(np.int8)
    w, wkw, _ = K.make_coded_weights(r, w_shape, 1)
    b = (r.standard_normal(Oc) * 0.2).astype(F)
    gamma, beta = (r.standard_normal(Oc) * 0.5 + 1).astype(F), (r.standard_normal(Oc) * 0.3).astype(F)
    rm, rv = (r.standard_normal(Oc) * 0.1).astype(F), (np.abs(r.standard_normal(Oc)) * 20 + 5).astype(F)
    da = r.standard_normal((N, Oc, H, W)).astype(F)
    g = be.geom(x_shape, w_shape, padding=1, groups=groups)
    wq = be.wq(**wkw)
    assert be.lib.mn_qconv_bnsign_stash_supported(C.byref(g), C.byref(wq)) == 1
    assert be.lib.mn_conv2d_bnh_supported(C.byref(g), C.byref(wq)) == 1, "the 3x3 geometry is not routed to the folded kernels"
    assert be.lib.mn_conv2d_bnh_pool_supported(C.byref(g), C.byref(wq)) == 0
    nb = max(int(be.lib.mn_qconv_bnsign_stash_ws_bytes(C.byref(g))), 4 * int(be.lib.mn_bnsign_ws_floats(Oc)))
    ws = be.empty(nb // 4 + 8)
    dA, dW, dB = be.to_dev_i8(a_in), be.to_dev(w), be.to_dev(b)
    dG, dBe, dRM, dRV, dDA = be.to_dev(gamma), be.to_dev(beta), be.to_dev(rm), be.to_dev(rv), be.to_dev(da)
    save, a8, h8 = be.empty((2, Oc)), be.empty_i8((N, Oc, H, W)), be.empty_i8((N, Oc, H, W))
    rows = int(be.lib.mn_qconv_bnsign_stash_chan_rows(C.byref(g)))
    assert rows == 17
    chan0 = be.empty((rows, Oc))
    nbt = be.to_dev_i64([0])
    be.call("mn_qconv_bnsign_fwd_stash", C.byref(g), C.byref(wq), be.ptr(dA), be.ptr(dW), be.ptr(dB), be.ptr(dG), be.ptr(dBe), 1e-5, 0.1, int(training),
            be.ptr(dRM), be.ptr(dRV), be.ptr(nbt), be.ptr(save), be.ptr(a8), be.ptr(h8), be.ptr(chan0), be.ptr(ws), nb, be.stream)
    # channel 1: a mask that passes nothing (L > U)
    ch = be.to_host(chan0).copy()
    ch[2, 1], ch[3, 1] = F(1e30), F(-1e30)
    chan = be.to_dev(ch)
    hb = be.to_host(h8).view(np.uint8).astype(np.float64)

    # what the stash reaches: every border class holds elements below L, inside [L, U] and above U
    nz = np.empty((Oc, H, W))
    for rc, rs in ((0, slice(0, 1)), (1, slice(1, H - 1)), (2, slice(H - 1, H))):
        for cc, cs in ((0, slice(0, 1)), (1, slice(1, W - 1)), (2, slice(W - 1, W))):
            nz[:, rs, cs] = ch[8 + 3 * rc + cc].astype(np.float64).reshape(-1, 1, 1)
    acc = 2.0 * hb - nz[None]
    cv = lambda k: ch[k].astype(np.float64).reshape(1, -1, 1, 1)
    u = acc * cv(1)
    below, above = u < cv(2), u > cv(3)
    mask = ~below & ~above
    live = np.ones(Oc, bool); live[1] = False
    for rs in (slice(0, 1), slice(1, H - 1), slice(H - 1, H)):
        for cs in (slice(0, 1), slice(1, W - 1), slice(W - 1, W)):
            assert below[:, live, rs, cs].any() and above[:, live, rs, cs].any() and mask[:, live, rs, cs].any()
    assert not mask[:, 1].any()

    sums, dgam, dbet = be.empty((2, Oc)), be.empty(Oc), be.empty(Oc)
    be.call("mn_bnh_bwd_sums", be.ptr(dDA), be.ptr(h8), None, be.ptr(chan), N, Oc, H, W, be.ptr(dgam), be.ptr(dbet), be.ptr(sums), be.ptr(ws), be.stream)
    # ---- the two-step path
    dy = be.empty((N, Oc, H, W))
    be.call("mn_bnh_bwd_apply", be.ptr(dDA), be.ptr(h8), None, be.ptr(chan), be.ptr(sums), N, Oc, H, W, int(training), be.ptr(dy), be.stream)
    aq8 = be.actq(3)
    dx_ref = be.to_host(be.conv_bwd_data(g, aq8, dy, dW, None, 3, wq=wq))
    assert be.lib.mn_last_kernel().decode() == "k_k3s_dgrad"
    dw_ref, db_ref = be.conv_bwd_weight(g, aq8, dy, dA, 3, bias=True)
    assert be.lib.mn_last_kernel().decode() == "k_k3s_wgrad"
    dw_ref, db_ref = be.to_host(dw_ref), be.to_host(db_ref)
    # ---- dy formed inside the kernels
    nb1 = be.lib.mn_conv2d_ws_bytes(C.byref(g), 1, 0)
    ws1, dx = be.empty(max(4, nb1 // 4 + 4)), be.empty(x_shape)
    be.call("mn_conv2d_bwd_data_bnh", C.byref(g), C.byref(wq), be.ptr(dDA), be.ptr(h8), be.ptr(chan), be.ptr(sums), int(training), be.ptr(dW), be.ptr(dx), be.ptr(ws1),
            nb1, be.stream)
    assert be.lib.mn_last_kernel().decode() == "k_k3s_dgrad<1>"
    nb2 = be.lib.mn_conv2d_ws_bytes(C.byref(g), 2, 0)
    ws2, dw, db = be.empty(max(4, nb2 // 4 + 4)), be.empty(w.shape), be.empty(Oc)
    be.call("mn_conv2d_bwd_weight_bnh", C.byref(g), be.ptr(dDA), be.ptr(h8), be.ptr(chan), be.ptr(sums), int(training), be.ptr(dA), be.ptr(dw), be.ptr(db),
            be.ptr(ws2), nb2, be.stream)
    assert be.lib.mn_last_kernel().decode() == "k_k3s_wgrad<0, 1>"
    dx, dw, db = be.to_host(dx), be.to_host(dw), be.to_host(db)
    assert np.isfinite(dx).all() and np.isfinite(dw).all() and np.abs(dx).max() > 0 and np.abs(dw).max() > 0
    assert np.array_equal(dx, dx_ref), ("dx", np.max(np.abs(dx - dx_ref)) / np.max(np.abs(dx_ref)))
    assert np.array_equal(dw, dw_ref), ("dw", np.max(np.abs(dw - dw_ref)) / np.max(np.abs(dw_ref)))
    assert np.array_equal(db, db_ref), ("dbias", np.max(np.abs(db - db_ref)))
    # dbias without dw's bias output requested: same dw
    dw_nb = be.empty(w.shape)
    be.call("mn_conv2d_bwd_weight_bnh", C.byref(g), be.ptr(dDA), be.ptr(h8), be.ptr(chan), be.ptr(sums), int(training), be.ptr(dA), be.ptr(dw_nb), None,
            be.ptr(ws2), nb2, be.stream)
    assert np.array_equal(be.to_host(dw_nb), dw)

    # ---- not only a self-comparison: fp64 dy from the same constants, fp64 contraction, at the tolerance of the grouped 3x3 rows of kernel_cases (1e-5)
    sm = be.to_host(sums).astype(np.float64)
    n = float(N * H * W)
    k1, k2 = (sm[0] / n, sm[1] / n) if training else (np.zeros(Oc), np.zeros(Oc))
    dz = np.where(mask, da.astype(np.float64), 0.0)
    dy64 = cv(6) * (dz - k1.reshape(1, -1, 1, 1) - (acc * cv(4) + cv(5)) * k2.reshape(1, -1, 1, 1))
    assert K.close(be.to_host(dy), dy64, 1e-5)
    dx64, dw64, db64 = O.conv2d_bwd(dy64, a_in.astype(np.float64), w.astype(np.float64), padding=1, groups=groups)
    assert K.close(dx, dx64, 1e-5), ("dx vs fp64", np.max(np.abs(dx - dx64)) / np.max(np.abs(dx64)))
    assert K.close(dw, dw64, 1e-5), ("dw vs fp64", np.max(np.abs(dw - dw64)) / np.max(np.abs(dw64)))
    # dbias in front of a BatchNorm cancels to ~0: bound by fp32 round-off of the sum of magnitudes (partial sums in fp32 over <= a few hundred terms, fp64 above that)
    assert np.all(np.abs(db - db64) <= 1e-5 * np.abs(dy64).sum(axis=(0, 2, 3)) + 1e-30), np.max(np.abs(db - db64))
    # misaligned operands are refused, not misread
    if be.kind == "emu":
        off = np.zeros(da.size + 1, dtype=F)[1:].reshape(da.shape)
        off[...] = da
        rc = be.lib.mn_conv2d_bwd_data_bnh(C.byref(g), C.byref(wq), be.ptr(off), be.ptr(h8), be.ptr(chan), be.ptr(sums), int(training), be.ptr(dW), be.ptr(be.empty(x_shape)),
                                           be.ptr(ws1), nb1, be.stream)
        assert rc != 0
        rc = be.lib.mn_conv2d_bwd_weight_bnh(C.byref(g), be.ptr(off), be.ptr(h8), be.ptr(chan), be.ptr(sums), int(training), be.ptr(dA), be.ptr(be.empty(w.shape)), None,
                                             be.ptr(ws2), nb2, be.stream)
        assert rc != 0
