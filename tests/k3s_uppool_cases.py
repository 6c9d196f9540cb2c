"""Grouped 3 x 3 binary block behind a 2x2 max-pool behind a pointwise BatchNorm+sign block: the backward-data kernel that also leaves the BatchNorm-backward sums
of the pooled block in front (k_k3s_dgrad<1, 1>, mn_conv2d_bwd_data_bnh_uppool + mn_bnh_bwd_sums_finish_pool) against the plain kernel (dx bit for bit), an fp64
evaluation from the stored dx and the pass it replaces (mn_bnh_bwd_sums with the block's own codes).  Backend-agnostic (emulator / GPU)."""
import ctypes as C

import numpy as np

import kernel_cases as K

F = np.float32

# (consumer x_shape, w_shape, groups): the upstream pointwise block is built for real at (N, C, 2H, 2W)
CASES = [
    dict(x_shape=(5, 32, 8, 8), w_shape=(64, 16, 3, 3), groups=2),             # two images per stage, odd N: the clamped half stage must not contribute
    dict(x_shape=(3, 32, 16, 16), w_shape=(64, 16, 3, 3), groups=2),           # one image per stage
    dict(x_shape=(5, 48, 8, 8), w_shape=(48, 24, 3, 3), groups=2),             # ragged: Cg = 24 gives two channel tiles, the second half empty
    dict(x_shape=(5, 32, 8, 8), w_shape=(64, 16, 3, 3), groups=2, in_shuffle=2),        # physical channel != g * Cg + c
]
# the grid cap makes some blocks walk two stages
CASE_LONG = dict(x_shape=(132, 128, 8, 8), w_shape=(256, 16, 3, 3), groups=8)
# error over the sum of magnitudes, for both sums: the bound kernel_cases._check_pwb holds k_pwb's upstream sums to
SUM_TOL = 2e-6


def derive_codes(h, chan):
    """The upstream block's output codes from its stash bytes: the byte threshold of the sign pass (qgemm_sign.hip, h_sign_stream_pw)."""
    T, fl, nnz = chan[0].astype(F), chan[1].astype(F), chan[7].astype(F)
    tf = np.where(fl > 0, np.ceil((T + nnz) * F(0.5)), np.floor((nnz - T) * F(0.5)) + F(1))
    tf = np.clip(tf, 0, 256).reshape(1, -1, 1, 1)
    ge = h.astype(np.float32) >= tf
    return np.where(ge != (fl <= 0).reshape(1, -1, 1, 1), 1, -1).astype(np.int8)


def windows(t):
    """[N][C][2H][2W] -> [N][C][H][W][4], a window's elements in row-major order"""
    N, Cc, H2, W2 = t.shape
    return t.reshape(N, Cc, H2 // 2, 2, W2 // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, Cc, H2 // 2, W2 // 2, 4)


def check(be, x_shape, w_shape, groups, in_shuffle=0, seed=0):
    r = np.random.default_rng(seed)
    N, Cin, H, W = x_shape
    Oc = w_shape[0]
    # ---- the upstream block for real: a pointwise grouped conv on random codes, BatchNorm + sign, pooled codes from the sign pass
    CU, GU = 32, 2
    u_shape, uw_shape = (N, CU, 2 * H, 2 * W), (Cin, CU // GU, 1, 1)
    gu = be.geom(u_shape, uw_shape, groups=GU)
    uwt, ukw, _ = K.make_coded_weights(r, uw_shape, 1)
    uwq = be.wq(**ukw)
    assert be.lib.mn_qconv_bnsign_fwd_stash_pool_supported(C.byref(gu), C.byref(uwq)) == 1
    ua = np.where(r.standard_normal(u_shape) > 0, 1, -1).astype(np.int8)
    ub = (r.standard_normal(Cin) * 0.2).astype(F)
    # |gamma| in [0.8, 1.6], beta in [-0.7, -0.3]: z ~ N(beta, gamma^2) leaves every channel all -1 windows whose element 0 is below -1 as well as first maxima above +1
    ug = ((0.8 + 0.8 * r.random(Cin)) * np.where(r.random(Cin) < 0.5, -1, 1)).astype(F)
    ube = (-0.7 + 0.4 * r.random(Cin)).astype(F)
    nbu = int(be.lib.mn_qconv_bnsign_stash_ws_bytes(C.byref(gu)))
    assert int(be.lib.mn_qconv_bnsign_stash_chan_rows(C.byref(gu))) == 8
    d_uh, d_uown, d_uap, d_uchan0 = be.empty_i8((N, Cin, 2 * H, 2 * W)), be.empty_i8((N, Cin, 2 * H, 2 * W)), be.empty_i8(x_shape), be.empty((8, Cin))
    keep = [be.to_dev_i8(ua), be.to_dev(uwt), be.to_dev(ub), be.to_dev(ug), be.to_dev(ube), be.to_dev(np.zeros(Cin, F)), be.to_dev(np.ones(Cin, F)), be.to_dev_i64([0]),
            be.empty((2, Cin)), be.empty(nbu // 4 + 8)]          # (buffers stay referenced until their results are read back)
    be.call("mn_qconv_bnsign_fwd_stash_pool", C.byref(gu), C.byref(uwq), be.ptr(keep[0]), be.ptr(keep[1]), be.ptr(keep[2]), be.ptr(keep[3]), be.ptr(keep[4]), 1e-5, 0.1, 1,
            be.ptr(keep[5]), be.ptr(keep[6]), be.ptr(keep[7]), be.ptr(keep[8]), be.ptr(d_uown), be.ptr(d_uap), be.ptr(d_uh), be.ptr(d_uchan0), be.ptr(keep[9]), nbu, be.stream)
    uh, uown, a_in = be.to_host(d_uh).view(np.uint8), be.to_host(d_uown), be.to_host(d_uap)
    uch = be.to_host(d_uchan0).copy()
    # the codes derived from the stash are the stored ones, on every element (what lets the kernel read 4 B per pooled element instead of 8)
    assert np.array_equal(derive_codes(uh, uch), uown), "derived codes != stored codes"
    uch[2, 1], uch[3, 1] = F(1e30), F(-1e30)          # channel 1: a mask that passes nothing (L > U)
    d_uchan = be.to_dev(uch)

    # ---- planted data, present before judging
    ow, hw = windows(uown) > 0, windows(uh).astype(np.float64)
    pos = np.argmax(ow, axis=-1)                      # the first +1 in row-major order, else element 0
    none = ~ow.any(axis=-1)
    for k in range(4):
        assert ((pos == k) & ~none).any(), "no window whose first +1 is at position %d" % k
    assert none.any(), "no all -1 window"
    hv = np.take_along_axis(hw, pos[..., None], axis=-1)[..., 0]
    cv = lambda k: uch[k].astype(np.float64).reshape(1, -1, 1, 1)
    acc = 2.0 * hv - cv(7)
    u = acc * cv(1)
    below, above = u < cv(2), u > cv(3)
    mask = ~below & ~above
    live = np.ones(Cin, bool); live[1] = False
    assert not mask[:, 1].any()
    for what, m in (("below L", below), ("inside [L, U]", mask), ("above U", above)):
        assert m.transpose(1, 0, 2, 3).reshape(Cin, -1)[live].any(axis=1).all(), "a live channel without a receiving pixel " + what

    # ---- the 3x3 block: forward on the pooled codes, then backward-data with and without the upstream sums
    w, wkw, _ = K.make_coded_weights(r, w_shape, 1)
    b = (r.standard_normal(Oc) * 0.2).astype(F)
    gamma, beta = (r.standard_normal(Oc) * 0.5 + 1).astype(F), (r.standard_normal(Oc) * 0.3).astype(F)
    da = r.standard_normal((N, Oc, H, W)).astype(F)
    g = be.geom(x_shape, w_shape, padding=1, groups=groups)
    g.in_shuffle = in_shuffle
    wq = be.wq(**wkw)
    assert be.lib.mn_conv2d_bnh_supported(C.byref(g), C.byref(wq)) == 1
    nb = max(int(be.lib.mn_qconv_bnsign_stash_ws_bytes(C.byref(g))), 4 * int(be.lib.mn_bnsign_ws_floats(max(Oc, Cin))))
    ws = be.empty(nb // 4 + 8)
    dW, dDA = be.to_dev(w), be.to_dev(da)
    a8, h8, chan = be.empty_i8((N, Oc, H, W)), be.empty_i8((N, Oc, H, W)), be.empty((17, Oc))
    keep2 = [be.to_dev_i8(a_in), be.to_dev(b), be.to_dev(gamma), be.to_dev(beta), be.to_dev(np.zeros(Oc, F)), be.to_dev(np.ones(Oc, F)), be.to_dev_i64([0]), be.empty((2, Oc)),
             be.empty(Oc), be.empty(Oc)]
    be.call("mn_qconv_bnsign_fwd_stash", C.byref(g), C.byref(wq), be.ptr(keep2[0]), be.ptr(dW), be.ptr(keep2[1]), be.ptr(keep2[2]), be.ptr(keep2[3]), 1e-5, 0.1, 1,
            be.ptr(keep2[4]), be.ptr(keep2[5]), be.ptr(keep2[6]), be.ptr(keep2[7]), be.ptr(a8), be.ptr(h8), be.ptr(chan), be.ptr(ws), nb, be.stream)
    sums = be.empty((2, Oc))
    be.call("mn_bnh_bwd_sums", be.ptr(dDA), be.ptr(h8), None, be.ptr(chan), N, Oc, H, W, be.ptr(keep2[8]), be.ptr(keep2[9]), be.ptr(sums), be.ptr(ws), be.stream)
    nb1 = be.lib.mn_conv2d_ws_bytes(C.byref(g), 1, 0)
    ws1, dx0 = be.empty(max(4, nb1 // 4 + 4)), be.empty(x_shape)
    be.call("mn_conv2d_bwd_data_bnh", C.byref(g), C.byref(wq), be.ptr(dDA), be.ptr(h8), be.ptr(chan), be.ptr(sums), 1, be.ptr(dW), be.ptr(dx0), be.ptr(ws1), nb1, be.stream)
    assert be.lib.mn_last_kernel().decode() == "k_k3s_dgrad<1>"
    splits = int(be.lib.mn_conv2d_bwd_data_bnh_uppool_splits(C.byref(g), C.byref(wq)))
    assert splits > 0

    def run_up():
        dx, part = be.empty(x_shape), be.empty(Cin * splits * 4 + 4)          # part: [C][splits][2] doubles
        be.call("mn_conv2d_bwd_data_bnh_uppool", C.byref(g), C.byref(wq), be.ptr(dDA), be.ptr(h8), be.ptr(chan), be.ptr(sums), 1, be.ptr(dW), be.ptr(dx), be.ptr(ws1), nb1,
                be.ptr(d_uh), 2 * H, 2 * W, be.ptr(d_uchan), 8, be.ptr(part), be.stream)
        assert be.lib.mn_last_kernel().decode() == "k_k3s_dgrad<1, 1>"
        return dx, part
    dx, part = run_up()
    dxh = be.to_host(dx)
    assert np.isfinite(dxh).all() and np.abs(dxh).max() > 0
    assert np.array_equal(dxh, be.to_host(dx0)), "dx differs from mn_conv2d_bwd_data_bnh"
    _, part2 = run_up()
    p1, p2 = be.to_host(part)[:Cin * splits * 4].view(np.float64), be.to_host(part2)[:Cin * splits * 4].view(np.float64)
    assert np.isfinite(p1).all() and np.array_equal(p1, p2), "partials differ between two runs"
    s_up, dg_up, db_up = be.empty((2, Cin)), be.empty(Cin), be.empty(Cin)
    be.call("mn_bnh_bwd_sums_finish_pool", be.ptr(part), splits, N, Cin, 2 * H, 2 * W, be.ptr(dg_up), be.ptr(db_up), be.ptr(s_up), be.stream)
    # the pass being replaced, on the same dx
    s_ref = be.empty((2, Cin))
    dg_ref, db_ref = be.empty(Cin), be.empty(Cin)
    be.call("mn_bnh_bwd_sums", be.ptr(dx), be.ptr(d_uh), be.ptr(d_uown), be.ptr(d_uchan), N, Cin, 2 * H, 2 * W, be.ptr(dg_ref), be.ptr(db_ref), be.ptr(s_ref),
            be.ptr(ws), be.stream)
    assert be.lib.mn_last_kernel().decode() == "k_bnh_partial_pool"
    got, ref = be.to_host(s_up).astype(np.float64), be.to_host(s_ref).astype(np.float64)
    # fp64 from the stored dx: route to the window's first maximum, mask, sum; the sums cancel, so the error is judged against the sum of magnitudes
    dz = np.where(mask, dxh.astype(np.float64), 0.0)
    zh = acc * cv(4) + cv(5)
    e1, e2 = dz.sum(axis=(0, 2, 3)), (dz * zh).sum(axis=(0, 2, 3))
    m1, m2 = np.abs(dz).sum(axis=(0, 2, 3)) + 1e-30, np.abs(dz * zh).sum(axis=(0, 2, 3)) + 1e-30
    err = (np.max(np.abs(got[0] - e1) / m1), np.max(np.abs(got[1] - e2) / m2))
    err_ref = (np.max(np.abs(ref[0] - e1) / m1), np.max(np.abs(ref[1] - e2) / m2))
    print("k3s uppool sums: error / sum of magnitudes", err, "replaced pass", err_ref)
    assert err_ref[0] <= SUM_TOL and err_ref[1] <= SUM_TOL, ("mn_bnh_bwd_sums", err_ref)
    assert err[0] <= SUM_TOL and err[1] <= SUM_TOL, ("k_k3s_dgrad<1, 1> upstream sums", err)
    # the kernel forms k_bnh_partial_pool's fp32 partials (four neighbouring windows of a row, left to right) and only the fp64 order between them differs: the
    # finished fp32 sums are the replaced pass's to the bit, so a training step does not depend on which route a block took
    assert np.array_equal(be.to_host(s_up), be.to_host(s_ref)), "finished sums differ from mn_bnh_bwd_sums in some bit"
    assert np.all(got[:, 1] == 0), "the channel with L > U has non-zero sums"
    assert np.abs(got[0][live]).max() > 0 and np.abs(got[1][live]).max() > 0
    assert np.array_equal(be.to_host(dg_up), be.to_host(s_up)[1]) and np.array_equal(be.to_host(db_up), be.to_host(s_up)[0])

    # ---- operands the plan does not cover are refused, and nothing is written
    if be.kind == "emu":
        def refused(uh_ptr, uH, uW, rows):
            dxr, partr = be.empty(x_shape), be.empty(Cin * splits * 4 + 4)
            rc = be.lib.mn_conv2d_bwd_data_bnh_uppool(C.byref(g), C.byref(wq), be.ptr(dDA), be.ptr(h8), be.ptr(chan), be.ptr(sums), 1, be.ptr(dW), be.ptr(dxr), be.ptr(ws1),
                                                      nb1, uh_ptr, uH, uW, be.ptr(d_uchan), rows, be.ptr(partr), be.stream)
            return rc != 0 and np.all(dxr == F(-1234.5)) and np.all(partr == F(-1234.5))
        off = np.zeros(uh.size + 16, dtype=np.uint8)
        base = off.ctypes.data
        mis = C.c_void_p(base + (1 if base % 4 == 0 else 4 - base % 4 + 1))          # 1 past a 4-byte boundary
        assert refused(mis, 2 * H, 2 * W, 8), "a misaligned upstream stash"
        assert refused(be.ptr(d_uh), 2 * H - 1, 2 * W, 8), "an odd upstream height"
        assert refused(be.ptr(d_uh), 2 * H, 2 * W, 17), "upstream constants of a 3x3 block"
