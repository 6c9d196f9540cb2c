"""csrc/qgemm_iao8_tile.h (mn_i8conv5_*, mn_i8_maxpool) through the C ABI: one case table for the CPU emulation build and the GPU.  The judge is tests/iao8_cases.py's:
the 5x5 accumulators in int64 (asserted within int32), then ``chain_codes`` in numpy float32; the pools by a window maximum over the in-map taps, then
``code_of(m * s_p, s_out)``.  Bytes must be equal, tail positions 0; output maps are poisoned before the launch, with a guard region behind them."""
import ctypes as C

import numpy as np

import iao8_cases as IC
from bits_cases import _dev_i32, _empty_i32, _host_u32
from code8_res_cases import guarded_map
from codes_cases import shuffle_order
from micronet_amd._lib import MN_EINVAL, MN_ENOTSUP

F = np.float32
# (id, x shape, O, consumer shuffle, seed, make_case keywords)
CONVS = [
    ("odd_narrow_map", (1, 16, 5, 7), 24, 0, 8800, {}),                     # every border class, narrower than its halo tile, a partial output block; 25 slots: 3 padding slots
    ("images_share_a_block", (3, 48, 6, 6), 80, 2, 8801, {}),               # 75 slots: one padding slot; two sets; three images in one tile: the halo between images
    ("two_row_bands", (1, 16, 20, 16), 16, 0, 8802, {}),                    # 320 pixels: a band of 16 rows and one of 4, the halo rows of each from the other
    ("extreme", (1, 16, 5, 7), 24, 0, 8800, dict(extreme=True)),            # every code at qmin against weight codes at +-127
    ("w4a4", (1, 16, 5, 7), 24, 0, 8803, dict(widths=(4, 4))),
]
# (x shape, (kernel, stride, padding), s_out / s_p): 2.0 makes every odd maximum a rounding tie, 0.37 saturates
POOLS = [((1, 20, 5, 7), (3, 2, 1), 1.0), ((2, 32, 8, 8), (3, 2, 1), 0.37), ((2, 32, 8, 8), (2, 2, 0), 2.0)]
# geometries refused: (x shape, w shape, stride, padding, groups, (a_bits, w_bits))
REFUSED = [
    ((1, 32, 8, 8), (32, 16, 5, 5), 1, 2, 2, (8, 8)), ((1, 32, 8, 8), (32, 32, 5, 5), 2, 2, 1, (8, 8)), ((1, 32, 8, 8), (32, 32, 5, 5), 1, 1, 1, (8, 8)),
    ((1, 20, 8, 8), (32, 20, 5, 5), 1, 2, 1, (8, 8)), ((1, 32, 8, 8), (32, 32, 5, 5), 1, 2, 1, (9, 8)),
    ((1, 48, 2, 256), (16, 48, 5, 5), 1, 2, 1, (8, 8)),          # 3 * 5 * 260 = 3900 blocks: one output row with its halo is beyond 48 KB
]


def read_map(be, buf, size, N, Cc, H, W):
    got = be.to_host(buf)
    assert (got[size:] == 77).all(), "the guard behind the map is intact"
    return IC.np_unblock(got[:size].reshape(N, -1, H * W, 16), (Cc + 15) // 16 * 16, H, W)


def check_conv(be, idx):
    cid, x_shape, Oc, shuffle, seed, kw = CONVS[idx]
    case = IC.make_case(x_shape, Oc, 5, 1, seed, **kw)
    ref, (ab, wb) = IC.judge(case, 0), (case["a_bits"], case["w_bits"])
    if not kw:
        IC.assert_case_is_hard(case)
    elif "extreme" in kw:
        assert (int(case["acc"].min()), int(case["acc"].max())) == (-128 * 127 * 16 * 25, 128 * 127 * 16 * 25) and len(np.unique(ref)) >= 2
    else:
        assert len(np.unique(ref)) == 8, "all non-negative 4-bit codes"
    order, g = (shuffle_order(Oc, shuffle) if shuffle else None), IC.geom_of(be, case)
    nb = int(be.lib.mn_i8conv5_table_bytes(C.byref(g), ab, wb))
    assert be.lib.mn_i8conv5_supported(C.byref(g), ab, wb) == 1 and be.lib.mn_i8conv_supported(C.byref(g), ab, wb) == 0 and nb > 0 and nb % 16 == 0
    table, dO = _empty_i32(be, (nb // 4,)), (_dev_i32(be, order.astype(np.int32)) if shuffle else None)
    dW, dS, dB = be.to_dev(case["w"]), be.to_dev(case["s_w"]), be.to_dev(case["b"])
    be.call("mn_i8conv5_pack", C.byref(g), be.ptr(dW), be.ptr(dS), 1, be.ptr(dB), float(case["s_a"]), float(case["s_out"]), ab, wb, be.ptr(dO), be.ptr(table), be.stream)
    hdr = _host_u32(be, table)
    assert (int(hdr[0]), int(hdr[7]), int(hdr[1]), int(hdr[6])) == (0, 0, (25 * x_shape[1] // 16 + 3) // 4, ab | wb << 8), "finite constants, weights on the grid"
    assert hdr[8:13].view(F).tolist() == [case["s_out"], case["s_out"], *IC.qrange(ab), case["s_a"]]
    N, _, H, Wd = x_shape
    (buf, size), dX = guarded_map(be, N, Oc, H * Wd), be.to_dev_i8(IC.np_block(case["j"]))
    be.call("mn_i8conv5_fwd", C.byref(g), ab, wb, be.ptr(table), be.ptr(dX), be.ptr(buf), be.stream)
    name, got = be.lib.mn_last_kernel().decode(), read_map(be, buf, size, N, Oc, H, Wd)
    want = IC.expect_positions(ref, order, (Oc + 15) // 16)
    print(name, cid, "mismatches against the judge", int((got != want).sum()), "of", want.size, "distinct codes", len(np.unique(ref)))
    assert name == "k_i8conv5<5>" and np.array_equal(got, want)


def np_pool(codes, s_p, s_out, a_bits, ksp):
    """The window maximum over the in-map taps (a tap outside the map: -128, which no window's real pixel is below), requantised from s_p to s_out."""
    k, s, p = ksp
    x = np.pad(codes.astype(np.int64), ((0, 0), (0, 0), (p, p), (p, p)), constant_values=-128)
    Ho, Wo = (x.shape[2] - k) // s + 1, (x.shape[3] - k) // s + 1
    m = np.max([x[:, :, dy:dy + s * Ho:s, dx:dx + s * Wo:s] for dy in range(k) for dx in range(k)], axis=0)
    return IC.code_of((m.astype(F) * F(s_p)).astype(F), s_out, a_bits).astype(np.int8)


def check_pool(be, idx):
    x_shape, ksp, ratio = POOLS[idx]
    codes = np.random.default_rng(8850 + idx).integers(-128, 128, size=x_shape).astype(np.int8)
    codes[:, :, 0, 0], codes[0, :, -1, -1] = 0, 127                      # a whole-zero pixel and a saturated one
    s_p = F(0.05)
    s_out = F(s_p * F(ratio))
    ref = np_pool(codes, s_p, s_out, 8, ksp)
    if ratio != 1.0:
        assert not np.array_equal(ref, np_pool(codes, s_p, s_p, 8, ksp)), "s_p != s_out must change codes"
    N, Cc, H, Wd = x_shape
    (buf, size), dX = guarded_map(be, N, Cc, ref.shape[2] * ref.shape[3]), be.to_dev_i8(IC.np_block(codes))
    be.call("mn_i8_maxpool", be.ptr(dX), N, Cc, H, Wd, *ksp, float(s_p), float(s_out), 8, be.ptr(buf), be.stream)
    got = read_map(be, buf, size, N, Cc, *ref.shape[2:])
    assert be.lib.mn_last_kernel().decode() == "k_i8_maxpool"
    assert np.array_equal(got, IC.expect_positions(ref, None, (Cc + 15) // 16)), "the requantised window maximum; tail channels 0"


def check_refused(be, idx):
    """MN_ENOTSUP from every entry of a geometry (past the table: a pool kind) that is not covered; the poisoned buffer stays as it was."""
    buf, f = _empty_i32(be, (64,)), be.to_dev(np.ones(64, dtype=F))
    if idx < len(REFUSED):
        x_shape, w_shape, stride, padding, groups, (ab, wb) = REFUSED[idx]
        g = be.geom(x_shape, w_shape, stride=stride, padding=padding, groups=groups)
        assert be.lib.mn_i8conv5_supported(C.byref(g), ab, wb) == 0 and int(be.lib.mn_i8conv5_table_bytes(C.byref(g), ab, wb)) == 0
        assert be.lib.mn_i8conv5_pack(C.byref(g), be.ptr(f), be.ptr(f), 1, be.ptr(f), 1.0, 1.0, ab, wb, None, be.ptr(buf), be.stream) == MN_ENOTSUP
        assert be.lib.mn_i8conv5_fwd(C.byref(g), ab, wb, be.ptr(buf), be.ptr(buf), be.ptr(buf), be.stream) == MN_ENOTSUP
    else:
        assert be.lib.mn_i8_maxpool(be.ptr(f), 1, 16, 2, 2, 3, 1, 1, 1.0, 1.0, 8, be.ptr(buf), be.stream) == MN_ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_invalid(be, _=None):
    """MN_EINVAL: a null table, a misaligned map, an output that overlaps the input, a pool in place."""
    g = be.geom((1, 16, 4, 4), (16, 16, 5, 5), padding=2)
    buf, out = _empty_i32(be, (4096,)), _empty_i32(be, (4096,))
    p, o, odd = be.ptr(buf), be.ptr(out), be.ptr_at(out, 1)
    fwd, pool = be.lib.mn_i8conv5_fwd, be.lib.mn_i8_maxpool
    assert fwd(C.byref(g), 8, 8, None, p, o, be.stream) == MN_EINVAL and fwd(C.byref(g), 8, 8, p, p, odd, be.stream) == MN_EINVAL
    assert fwd(C.byref(g), 8, 8, p, o, o, be.stream) == MN_EINVAL
    assert pool(None, 1, 16, 4, 4, 2, 2, 0, 1.0, 1.0, 8, o, be.stream) == MN_EINVAL and pool(p, 1, 16, 4, 4, 2, 2, 0, 1.0, 1.0, 8, odd, be.stream) == MN_EINVAL
    assert pool(o, 1, 16, 4, 4, 2, 2, 0, 1.0, 1.0, 8, o, be.stream) == MN_EINVAL, "no in-place pool"
    assert (_host_u32(be, out) == 0x5a5a5a5a).all(), "an invalid call writes nothing"


# (id, check, argument) for the two drivers: tests/test_iao8_tile_emulated.py, tests/test_gpu_iao8_tile.py
CHECKS = ([(c[0], check_conv, i) for i, c in enumerate(CONVS)] + [("pool%d_k%d" % (i, c[1][0]), check_pool, i) for i, c in enumerate(POOLS)]
          + [("refused%d" % i, check_refused, i) for i in range(len(REFUSED) + 1)] + [("invalid", check_invalid, None)])
