"""The two ends of the int8 deployment of BN-folded IAO ResNets (csrc/qgemm_iao8_e2e.h: mn_i8first_fwd2, mn_i8poolfc_*) through the C ABI: one case table for the CPU
emulation build and the GPU.  Every kernel comparison is exact, in buffers poisoned before the launch with a guard region behind every output, over two identical
runs.

The first block's judge is tests/iao8_ends_cases.py's -- the image built from a case's codes with exact ties, values far outside the range and -0.0, the codes read
back from it with ``code_of``, ``oracle.np_oracle.conv2d_fwd(acc=np.int64)`` and the chain up to r in numpy float32 -- with one ``code_of`` per output quantizer
behind it.  The pooled classifier's judge is numpy: the fp64 pooled value of the de-quantised codes (an exact sum), the fp32 code of it, int64 sums of code products
and the fp32 chain; its pooled value and code are also held bit for bit to the library's own mn_iao_fq_avgpool_fwd + mn_iao_fq_fwd."""
import ctypes as C

import numpy as np

import iao8_ends_cases as EC
from iao8_cases import F, assert_case_is_hard, code_of, np_block, np_unblock, qrange
from bits_cases import _empty_i32, _host_u32

GUARD = 256          # poisoned bytes / words behind every output

# (id, x shape, O, KS): seed 6200 + index; NOUT = 2
FIRST2 = [
    ("f3_rgb", (2, 3, 8, 8), 64, 3),                  # the base case
    ("f3_odd_map", (1, 3, 5, 7), 40, 3),              # 35 pixels < one wave, a partial output block
    ("f3_one_pixel", (1, 3, 1, 1), 16, 3),            # a single pixel
    ("f3_strip_cut", (3, 3, 20, 20), 64, 3),          # 400 pixels: two blocks per image, the cut falls mid-row
    ("f3_two_sets", (1, 3, 6, 6), 80, 3),
    ("f3_14", (1, 14, 4, 4), 32, 3),                  # K = 126, two k-steps
    ("f5_rgb", (1, 3, 6, 6), 32, 5),                  # the 5x5 kernel
]
NOT_HARD = ("f3_one_pixel",)          # too small for the tie channel and for the builder's assertions
# chain variants on f3_rgb's geometry: (id, widths (w, a) of the case, bits_1, s_1 / s_0, per-channel s_w)
FIRST2_CHAINS = [
    ("s1_double", (8, 8), 8, 2.0, True),
    ("w8_out8_out4", (8, 8), 4, 16.0, True),
    ("w4_out4_out4", (4, 4), 4, 1.37, True),
    ("per_layer", (8, 8), 8, 0.61, False),
]
S1_RATIO = 0.61          # the second consumer's scale of the geometry cases
# one launch whose blocks walk several sets (GPU only: the pattern of iao8_ends_cases.LARGE_FIRST): seed 6300
LARGE_FIRST2 = ("f3_five_sets", (700, 3, 8, 8), 312, 3)

# (id, (N, C, H, W), O): seed 6400 + index
POOLFC = [
    ("base", (3, 64, 4, 4), 10),
    ("partial_odd", (2, 40, 3, 3), 7),                # a partial channel block, odd HW
    ("hw1", (1, 512, 1, 1), 10),
    ("wide", (2, 2048, 2, 2), 10),
    ("o64", (1, 16, 8, 8), 64),
    ("five_images", (5, 512, 4, 4), 10),
]
# chain variants on the base geometry: (id, (p_bits, a_bits, w_bits), per-channel s_w, bias)
POOLFC_CHAINS = [
    ("w4a4", (4, 4, 4), True, True),
    ("pool8_fc4", (8, 4, 4), True, True),
    ("per_tensor", (8, 8, 8), False, True),
    ("null_bias", (8, 8, 8), True, False),
]
POOLFC_REFUSED = [((1, 64, 16, 65), (8, 8, 8)), ((1, 64, 4097, 10), (8, 8, 8)), ((1, 140000, 4, 10), (8, 8, 8)), ((1, 64, 16, 10), (9, 8, 8)),
                  ((1, 64, 16, 10), (8, 1, 8)), ((1, 64, 16, 10), (8, 8, 9))]


def _lib():
    from micronet_amd import _lib as L
    return L


# ---------------------------------------------------------------------------------------------- first block: judge and runner
def outs_of(case, bits1, ratio):
    """[(s_k, bits_k)]: output 0 is the case's consumer, output 1 a second quantizer."""
    return [(F(case["s_out"]), case["a_bits"]), (F(case["s_out"] * F(ratio)), bits1)]


def first2_judge(case, jx, outs):
    """[codes per output], the case as the judge saw it: the chain once up to r, one code_of per consumer."""
    ref0, seen = EC.first_judge(case, jx)
    r = EC.chain_r(seen["acc"], case["al"], case["b"], 1)
    refs = [code_of(r, s, bits).astype(np.int8) for s, bits in outs]
    assert np.array_equal(refs[0], ref0), "output 0 is the one-output judge's"
    return refs, seen


def assert_outs_are_hard(refs, outs):
    for ref, (_, bits) in zip(refs, outs):
        qmax = int(qrange(bits)[1])
        assert (ref == 0).any() and (ref == qmax).any() and ref.min() == 0, "both maps saturate at both ends of the ReLU's range"
    differ = float((refs[0] != refs[1]).mean())
    assert differ >= 0.25, ("the two maps must differ on a quarter of the positions", differ)


def _outs_struct(outs):
    q = _lib().I8FirstOuts()
    q.nout, q.s_out0, q.bits0 = len(outs), float(outs[0][0]), outs[0][1]
    q.s_out1, q.bits1 = (float(outs[1][0]), outs[1][1]) if len(outs) == 2 else (0.0, 0)
    return q


def run_first2(be, case, x, outs, table=None):
    """mn_i8first_pack at output 0's quantizer, then mn_i8first_fwd2 TWICE into poisoned buffers with a guard behind each map; returns ([codes [N, OB * 16, H, W]],
    kernel name, table)."""
    g = EC.first_geom(be, case)
    assert be.lib.mn_i8first_supported(C.byref(g), case["in_bits"], case["a_bits"], case["w_bits"]) == 1
    if table is None:
        table = EC.pack_first(be, g, case)
        hdr = _host_u32(be, table)
        assert int(hdr[0]) == 0 and int(hdr[7]) == 0
    N, _, H, W = x.shape
    OB = (case["w"].shape[0] + 15) // 16
    nb = N * OB * H * W * 16
    dx, q = be.to_dev(x), _outs_struct(outs)
    runs = []
    for _ in range(2):
        bufs = [be.empty_i8((nb + GUARD,)) for _ in outs]          # poisoned
        be.call("mn_i8first_fwd2", C.byref(g), case["in_bits"], case["w_bits"], be.ptr(table), be.ptr(dx), C.byref(q), be.ptr(bufs[0]),
                be.ptr(bufs[1]) if len(outs) == 2 else None, be.stream)
        runs.append([be.to_host(b) for b in bufs])
    name = be.lib.mn_last_kernel().decode()
    for a, b in zip(*runs):
        assert np.array_equal(a, b), "two runs give identical bytes"
        assert (a[nb:] == 77).all(), "the guard region keeps its poison"
    return [np_unblock(a[:nb].reshape(N, OB, H * W, 16), OB * 16, H, W) for a in runs[0]], name, table


def tiny_image(case):
    """The image of a map too small for make_image's five overridden elements (three values): an exact tie, a value far below the range, -0.0."""
    assert case["j"].size == 3
    s_a = case["s_a"]
    qmin = int(qrange(case["in_bits"])[0])
    x = np.array([F(2.5) * s_a, F(-1e6) * s_a, F(-0.0)], dtype=F).reshape(case["j"].shape)
    jx = code_of(x, s_a, case["in_bits"]).astype(np.int64)
    assert jx.reshape(-1).tolist() == [3, qmin, 0] and np.signbit(x.reshape(-1)[2]), "the tie rounds away from zero, the value outside clamps, -0.0 is the code 0"
    return x, jx


def _check_first2(be, case, seed, outs, what, hard):
    x, jx = tiny_image(case) if case["j"].size == 3 else EC.make_image(case, seed)
    refs, seen = first2_judge(case, jx, outs)
    if hard:
        if case["a_bits"] == 8:
            assert_case_is_hard(seen)
        assert_outs_are_hard(refs, outs)
    Oc = case["w"].shape[0]
    OB = (Oc + 15) // 16
    got, name, table = run_first2(be, case, x, outs)
    assert name == "k_i8first2<%d,2>" % case["KS"], name
    for k, (ref, out) in enumerate(zip(refs, got)):
        want = EC.expect_positions(ref, None, OB)
        bad = int((out != want).sum())
        print(name, what, "output", k, "mismatches against the judge", bad, "of", out.size, "distinct codes", len(np.unique(ref)))
        assert out.shape == want.shape and bad == 0, (k, bad, out.size)
    # output 0 is mn_i8first_fwd's on the same table, and NOUT = 1 through the new entry is the old entry's
    old, oname = EC.run_first(be, case, x, None, table=table)
    assert oname == "k_i8first<%d>" % case["KS"] and np.array_equal(old, got[0])
    one, name1, _ = run_first2(be, case, x, outs[:1], table=table)
    assert name1 == "k_i8first2<%d,1>" % case["KS"] and np.array_equal(one[0], old)


def check_first2(be, idx):
    name, x_shape, Oc, KS = FIRST2[idx]
    hard = name not in NOT_HARD
    case = EC.first_case(x_shape, Oc, KS, 6200 + idx, special=hard)
    _check_first2(be, case, 6200 + idx, outs_of(case, 8, S1_RATIO), "%s %s -> %d k%d" % (name, x_shape, Oc, KS), hard)


def check_first2_chain(be, idx):
    name, widths, bits1, ratio, per_channel = FIRST2_CHAINS[idx]
    _, x_shape, Oc, KS = FIRST2[0]
    case = EC.first_case(x_shape, Oc, KS, 6250 + idx, widths=widths, per_channel=per_channel)
    _check_first2(be, case, 6250 + idx, [(s, b) for s, b in outs_of(case, bits1, ratio)], name, True)


def check_first2_extreme(be):
    """check_first_extreme's accumulator (+-128 * 127 * 75) on both outputs."""
    _, x_shape, Oc, KS, _ = EC.FIRST[0]
    case = EC.first_case(x_shape, Oc, KS, 5500, extreme=True)
    assert int(np.abs(case["acc"]).max()) == 128 * 127 * 75 and int(case["acc"].min()) == -128 * 127 * 75
    outs = outs_of(case, 8, S1_RATIO)
    x, jx = EC.make_image(case, 5500)
    refs, _ = first2_judge(case, jx, outs)
    got, name, _ = run_first2(be, case, x, outs)
    assert name == "k_i8first2<5,2>"
    for ref, out in zip(refs, got):
        assert len(np.unique(ref)) >= 2 and np.array_equal(out, EC.expect_positions(ref, None, (Oc + 15) // 16))


def check_large_first2(be):
    import deploy_grid as DG
    from iao8_cases import LARGE_HEAD, chain_codes
    name, x_shape, Oc, KS = LARGE_FIRST2
    seed = 6300
    N, Cc, H, W = x_shape
    head = EC.first_case((LARGE_HEAD, Cc, H, W), Oc, KS, seed)
    qmin, qmax = (int(v) for v in qrange(head["in_bits"]))
    more = np.random.default_rng(seed + 500).integers(qmin, qmax + 1, size=(N - LARGE_HEAD, Cc, H, W)).astype(np.int8)
    more[:, :, 0, 0] = 0
    case = dict(head, j=np.concatenate([head["j"], more]))
    x, jx = EC.make_image(case, seed)
    OB = (Oc + 15) // 16
    gy, per = DG.assert_uneven_deal(be, N * DG.pixel_blocks(H * W, 256), (OB + 3) // 4)
    outs = outs_of(head, 8, S1_RATIO)
    got, kname, _ = run_first2(be, case, x, outs)
    assert kname == "k_i8first2<%d,2>" % KS, kname
    bad = 0
    for n0 in range(0, N, LARGE_HEAD):
        acc = DG.exact_conv(jx[n0:n0 + LARGE_HEAD], head["k"], KS // 2, 1)
        assert np.abs(acc).max() < 2 ** 31
        r = EC.chain_r(acc, head["al"], head["b"], 1)
        for k, (s, bits) in enumerate(outs):
            ref = code_of(r, s, bits).astype(np.int8)
            if k == 0:
                assert np.array_equal(ref, chain_codes(acc, head["al"], head["b"], head["s_out"], head["s_out"], head["a_bits"], 0))
            bad += int((got[k][n0:n0 + ref.shape[0]] != EC.expect_positions(ref, None, OB)).sum())
    print(kname, name, x_shape, "->", Oc, "grid.y", gy, "per", per, "mismatches against the judge", bad, "of", 2 * got[0].size)
    assert bad == 0, bad


def check_first2_invalid(be):
    """Every MN_EINVAL of mn_i8first_fwd2 with nothing written, MN_ENOTSUP for a 7x7 and a stride-2 stem."""
    L = _lib()
    lib, s = be.lib, be.stream
    g = be.geom((1, 3, 8, 8), (16, 3, 3, 3), padding=1)
    nb = int(lib.mn_i8first_table_bytes(C.byref(g), 8, 8, 8))
    tab = _empty_i32(be, (nb // 4,))
    f = be.to_dev(np.ones(3 * 64, dtype=F))
    oa, ob = be.empty_i8((1024,)), be.empty_i8((1024,))
    t, x, a, b = be.ptr(tab), be.ptr(f), be.ptr(oa), be.ptr(ob)
    off = lambda p, n: C.c_void_p(p.value + n)

    def q(nout=2, s0=1.0, b0=8, s1=1.0, b1=8):
        v = L.I8FirstOuts()
        v.nout, v.s_out0, v.bits0, v.s_out1, v.bits1 = nout, s0, b0, s1, b1
        return C.byref(v)
    call = lambda *args: lib.mn_i8first_fwd2(C.byref(g), 8, 8, *args, s)
    for args in ((None, x, q(), a, b), (t, None, q(), a, b), (t, x, None, a, b), (t, x, q(), None, b), (off(t, 4), x, q(), a, b), (t, off(x, 2), q(), a, b),
                 (t, x, q(), off(a, 8), b), (t, x, q(), a, off(b, 8)),                                            # null, misaligned
                 (t, x, q(nout=0), a, b), (t, x, q(nout=3), a, b), (t, x, q(nout=2), a, None), (t, x, q(nout=1), a, b),      # nout
                 (t, x, q(s0=0.0), a, b), (t, x, q(s1=-1.0), a, b), (t, x, q(s0=float("nan")), a, b), (t, x, q(s1=float("inf")), a, b),      # scales
                 (t, x, q(b0=1), a, b), (t, x, q(b1=9), a, b),                                                    # widths
                 (t, x, q(), a, a), (t, x, q(), a, off(a, 512)), (t, x, q(), x, b), (t, x, q(), a, off(x, 256)), (t, x, q(), t, b), (t, x, q(), a, off(t, 64))):      # overlaps
        assert call(*args) == L.MN_EINVAL, args
    g0 = be.geom((0, 3, 8, 8), (16, 3, 3, 3), padding=1)
    assert lib.mn_i8first_fwd2(C.byref(g0), 8, 8, t, x, q(), a, b, s) == L.MN_EINVAL
    for gn in (be.geom((1, 3, 8, 8), (16, 3, 7, 7), padding=3), be.geom((1, 3, 8, 8), (16, 3, 3, 3), padding=1, stride=2)):
        assert lib.mn_i8first_supported(C.byref(gn), 8, 8, 8) == 0
        assert lib.mn_i8first_fwd2(C.byref(gn), 8, 8, t, x, q(), a, b, s) == L.MN_ENOTSUP
        assert "not covered" in lib.mn_last_error().decode()
    assert lib.mn_i8first_fwd2(C.byref(g), 9, 8, t, x, q(), a, b, s) == L.MN_ENOTSUP
    assert (_host_u32(be, tab) == 0x5a5a5a5a).all() and (be.to_host(f) == 1).all() and (be.to_host(oa) == 77).all() and (be.to_host(ob) == 77).all(), "nothing is written"


# ---------------------------------------------------------------------------------------------- pooled classifier: judge and runner
def poolfc_case(shape, Oc, seed, bits=(8, 8, 8), per_channel=True, bias=True, kind="random"):
    """Codes at avg_pool's quantizer, fc weights on the grid, scales and bias.  kind: "random"; "extreme" (every j at qmin against weight codes +-kmax);
    "ties" (s_p = 2^-6, s_fc = s_p / 2 on a 2 x 2 map: m / s_fc = S / 2, every odd code sum an exact tie)."""
    p_bits, a_bits, w_bits = bits
    r = np.random.default_rng(seed)
    N, Cc, H, W = shape
    pmin, pmax = (int(v) for v in qrange(p_bits))
    amin, amax = (int(v) for v in qrange(a_bits))
    kmax = (1 << (w_bits - 1)) - 1
    s_p = F(2.0 ** -6) if kind == "ties" else F(2.0 ** -6 * 1.2345)
    if kind == "extreme":
        c = np.full(shape, pmin, dtype=np.int64)
        k = np.full((Oc, Cc), kmax, dtype=np.int64)
        k[1::2] = -kmax
    else:
        c = r.integers(pmin, pmax + 1, size=shape).astype(np.int64)
        c[:, 0] = pmin                                                   # a channel at either end of the range, a channel of zeros
        c[:, 1] = pmax
        c[:, 2] = 0
        k = r.integers(-kmax, kmax + 1, size=(Oc, Cc)).astype(np.int64)
    m = pooled(c, s_p)
    if kind == "extreme":
        s_fc = F(s_p * F(1 << (p_bits - a_bits)))                        # m = pmin s_p is the code amin
    elif kind == "ties":
        assert H * W == 4
        s_fc = F(s_p / F(2))
    else:
        s_fc = F(F(1.0173) * np.abs(m).max() / F(amax) * F(0.9))         # the extreme channels clamp
    s_w = (F(2.0 ** -7) * r.uniform(1.0, 2.0, size=Oc if per_channel else 1)).astype(F)
    sw_full = np.broadcast_to(s_w, (Oc,))
    w = (k.astype(F) * sw_full.reshape(-1, 1)).astype(F)
    al = (s_fc * sw_full).astype(F)
    b = (r.standard_normal(Oc) * 3.0).astype(F) if bias else None
    return dict(c=c.astype(np.int8), k=k, w=w, s_w=s_w, per_channel=per_channel, al=al, b=b, s_p=s_p, s_fc=s_fc, bits=bits, kind=kind)


def pooled(c, s_p):
    """m = (float)(sum_p (double)fl(float(c) * s_p) / (double)HW): the sum of at most 4096 fp32 values of at most 2^7 ulps' spread is exact in fp64 in any order."""
    v = (c.astype(F) * F(s_p)).astype(F)
    N, Cc, H, W = c.shape
    return (v.astype(np.float64).reshape(N, Cc, H * W).sum(axis=2) / np.float64(H * W)).astype(F)


def poolfc_judge(case):
    """(m, j, acc, y): the fp64 pooled value, its fp32 code at s_fc, int64 sums of code products, the fp32 chain."""
    m = pooled(case["c"].astype(np.int64), case["s_p"])
    j = code_of(m, case["s_fc"], case["bits"][1]).astype(np.int64)
    acc = j @ case["k"].T
    assert np.abs(acc).max() < 2 ** 31
    b = case["b"] if case["b"] is not None else np.zeros(case["k"].shape[0], dtype=F)
    y = ((acc.astype(F) * case["al"].reshape(1, -1)).astype(F) + b.reshape(1, -1).astype(F)).astype(F)
    return m, j, acc, y


def pack_poolfc(be, case, w=None, b=None, s_p=None, s_fc=None, s_w=None):
    Oc, Cc = case["k"].shape
    nb = int(be.lib.mn_i8poolfc_table_bytes(Cc, Oc, *case["bits"]))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    bias = case["b"] if b is None else b
    dW, dS, dB = be.to_dev(case["w"] if w is None else w), be.to_dev(case["s_w"] if s_w is None else s_w), be.to_dev(bias) if bias is not None else None
    be.call("mn_i8poolfc_pack", Cc, Oc, be.ptr(dW), be.ptr(dS), 1 if case["per_channel"] else 0, be.ptr(dB), C.c_float(float(case["s_p"] if s_p is None else s_p)),
            C.c_float(float(case["s_fc"] if s_fc is None else s_fc)), *case["bits"], be.ptr(table), be.stream)
    return table


def run_poolfc(be, case):
    """Pack, then mn_i8poolfc_fwd TWICE into poisoned buffers with a guard behind [N][O]; returns (y, kernel name)."""
    N, Cc, H, W = case["c"].shape
    Oc = case["k"].shape[0]
    assert be.lib.mn_i8poolfc_supported(N, Cc, H * W, Oc, *case["bits"]) == 1
    table = pack_poolfc(be, case)
    hdr = _host_u32(be, table)
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0, (int(hdr[0]), int(hdr[7]))
    assert int(hdr[6]) == (case["bits"][1] | case["bits"][2] << 8 | case["bits"][0] << 16)
    xb = be.to_dev_i8(np_block(case["c"]))
    outs = []
    for _ in range(2):
        y = be.empty((N * Oc + GUARD,))          # poisoned
        be.call("mn_i8poolfc_fwd", N, Cc, H * W, Oc, *case["bits"], be.ptr(table), be.ptr(xb), be.ptr(y), be.stream)
        outs.append(be.to_host(y))
    name = be.lib.mn_last_kernel().decode()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "two runs give identical values"
    assert (outs[0][N * Oc:] == F(-1234.5)).all(), "the guard region keeps its poison"
    return outs[0][:N * Oc].reshape(N, Oc), name


def library_pooled_code(be, case):
    """(m, fl(j * s_fc)) from the library's own mn_iao_fq_avgpool_fwd (k = H = W) and mn_iao_fq_fwd on the de-quantised map: the exact yardstick (square maps)."""
    N, Cc, H, W = case["c"].shape
    assert H == W
    v = (case["c"].astype(F) * case["s_p"]).astype(F)
    qp_p = be.to_dev(np.array([case["s_p"], 0, -1e30, 1e30], dtype=F))
    qp_f = be.to_dev(np.array([case["s_fc"], 0, -1e30, 1e30], dtype=F))
    dv, dm, dq = be.to_dev(v), be.empty((N * Cc,)), be.empty((N * Cc,))
    be.call("mn_iao_fq_avgpool_fwd", be.ptr(dv), be.ptr(dm), N * Cc, H, W, H, be.ptr(qp_p), case["bits"][0], 0, be.stream)
    be.call("mn_iao_fq_fwd", be.ptr(dm), be.ptr(dq), 1, N * Cc, be.ptr(qp_f), case["bits"][1], 0, 1, be.stream)
    return be.to_host(dm).reshape(N, Cc), be.to_host(dq).reshape(N, Cc)


def _check_poolfc(be, case, what):
    m, j, acc, want = poolfc_judge(case)
    amin, amax = (int(v) for v in qrange(case["bits"][1]))
    if case["kind"] == "random":
        assert j.min() == amin and j.max() == amax and len(np.unique(j)) > min(32, amax, j.size // 4), "the codes fill the range and clamp at both ends"
    if case["c"].shape[2] == case["c"].shape[3]:
        lm, lq = library_pooled_code(be, case)
        assert np.array_equal(lm.view(np.uint32), m.view(np.uint32)), "the judge's pooled value is the library's, bit for bit"
        assert np.array_equal(lq.view(np.uint32), (j.astype(F) * case["s_fc"]).astype(F).view(np.uint32)), "the judge's code is the library's"
    got, name = run_poolfc(be, case)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(name, what, "words that differ from the judge", bad, "of", got.size, "largest |acc|", int(np.abs(acc).max()))
    assert name == "k_i8poolfc", name
    assert bad == 0, (bad, got.size)
    return j, acc


def check_poolfc(be, idx):
    name, shape, Oc = POOLFC[idx]
    _check_poolfc(be, poolfc_case(shape, Oc, 6400 + idx), "%s %s -> %d" % (name, shape, Oc))


def check_poolfc_chain(be, idx):
    name, bits, per_channel, bias = POOLFC_CHAINS[idx]
    _, shape, Oc = POOLFC[0]
    _check_poolfc(be, poolfc_case(shape, Oc, 6450 + idx, bits=bits, per_channel=per_channel, bias=bias), name)


def check_poolfc_extreme(be):
    j, acc = _check_poolfc(be, poolfc_case((2, 2048, 2, 2), 10, 6480, kind="extreme"), "extreme")
    assert (j == -128).all() and int(np.abs(acc).max()) == 128 * 127 * 2048 and int(acc.min()) == -128 * 127 * 2048


def check_poolfc_ties(be):
    case = poolfc_case((3, 64, 2, 2), 10, 6481, kind="ties")
    j, _ = _check_poolfc(be, case, "ties")
    S = case["c"].astype(np.int64).sum(axis=(2, 3))
    odd = (S % 2 != 0) & (np.abs(S) < 250)
    assert odd.sum() > 20, "odd code sums in range"
    assert np.array_equal(j[odd], np.sign(S[odd]) * ((np.abs(S[odd]) + 1) // 2)), "an exact tie rounds away from zero"


def check_poolfc_identity_rows(be):
    """The kernel's own j, read through identity rows at al = 1: y[n, o] = j[n, o]."""
    case = poolfc_case((2, 64, 4, 4), 64, 6482, bias=False)
    case["k"] = np.eye(64, dtype=np.int64)
    case["s_w"] = np.full(64, F(1) / case["s_fc"], dtype=F)
    case["al"] = (case["s_fc"] * case["s_w"]).astype(F)
    case["w"] = (case["k"].astype(F) * case["s_w"].reshape(-1, 1)).astype(F)
    assert (case["al"] == 1).all() or np.allclose(case["al"], 1, rtol=2e-7)
    _, j, _, want = poolfc_judge(case)
    got, _ = run_poolfc(be, case)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if (case["al"] == 1).all():
        assert np.array_equal(got, j.astype(F))


def check_poolfc_counters(be):
    case = poolfc_case((1, 40, 2, 2), 7, 6483)
    hdr = _host_u32(be, pack_poolfc(be, case))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0 and (int(hdr[1]), int(hdr[2])) == (40, 7)
    assert hdr[8:12].view(F).tolist() == [case["s_p"], case["s_fc"], F(-128), F(127)]
    b = case["b"].copy()
    b[3] = F(np.nan)
    hdr = _host_u32(be, pack_poolfc(be, case, b=b))
    assert int(hdr[0]) == 1 and int(hdr[7]) == 0
    for kw in (dict(s_p=0.0), dict(s_fc=-1.0), dict(s_p=np.inf), dict(s_fc=np.nan)):
        hdr = _host_u32(be, pack_poolfc(be, case, **kw))
        assert int(hdr[0]) >= 1 and int(hdr[7]) == 0, kw
    sw = case["s_w"].copy()
    sw[2] = F(0)
    assert int(_host_u32(be, pack_poolfc(be, case, s_w=sw))[0]) >= 1
    w2 = case["w"].copy()
    w2[5, 17] += F(0.5) * case["s_w"][5]          # half a step off the grid
    w2[1, 3] = F(200) * case["s_w"][1]            # on the grid, beyond 2^(w-1) - 1
    hdr = _host_u32(be, pack_poolfc(be, case, w=w2))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 2


def check_poolfc_refused(be, idx):
    (N, Cc, HW, Oc), bits = POOLFC_REFUSED[idx]
    L = _lib()
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.ones(64, dtype=F))
    assert be.lib.mn_i8poolfc_supported(N, Cc, HW, Oc, *bits) == 0
    assert be.lib.mn_i8poolfc_fwd(N, Cc, HW, Oc, *bits, be.ptr(buf), be.ptr(buf), be.ptr(f), be.stream) == L.MN_ENOTSUP
    assert "not covered" in be.lib.mn_last_error().decode()
    if HW <= 4096:
        assert int(be.lib.mn_i8poolfc_table_bytes(Cc, Oc, *bits)) == 0
        assert be.lib.mn_i8poolfc_pack(Cc, Oc, be.ptr(f), be.ptr(f), 1, be.ptr(f), C.c_float(1), C.c_float(1), *bits, be.ptr(buf), be.stream) == L.MN_ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all() and (be.to_host(f) == 1).all(), "a refused call writes nothing"


def check_poolfc_invalid(be):
    L = _lib()
    lib, s = be.lib, be.stream
    nb = int(lib.mn_i8poolfc_table_bytes(16, 4, 8, 8, 8))
    tab = _empty_i32(be, (nb // 4,))
    f = be.to_dev(np.ones(64, dtype=F))
    codes = be.empty_i8((64,))
    t, p, c = be.ptr(tab), be.ptr(f), be.ptr(codes)
    off = lambda q, n: C.c_void_p(q.value + n)
    one = C.c_float(1.0)
    for args in ((None, p, 1, p, one, one, 8, 8, 8, t), (p, None, 1, p, one, one, 8, 8, 8, t), (p, p, 1, p, one, one, 8, 8, 8, None), (p, p, 1, p, one, one, 8, 8, 8, off(t, 4)),
                 (p, p, 2, p, one, one, 8, 8, 8, t), (p, p, -1, p, one, one, 8, 8, 8, t), (off(p, 2), p, 1, p, one, one, 8, 8, 8, t), (p, p, 1, off(p, 2), one, one, 8, 8, 8, t)):
        assert lib.mn_i8poolfc_pack(16, 4, *args, s) == L.MN_EINVAL, args
    assert lib.mn_i8poolfc_pack(0, 4, p, p, 1, p, one, one, 8, 8, 8, t, s) == L.MN_EINVAL
    for args in ((None, c, p), (t, None, p), (t, c, None), (off(t, 4), c, p), (t, off(c, 8), p), (t, c, off(p, 2)), (t, c, t), (t, p, p)):
        assert lib.mn_i8poolfc_fwd(1, 16, 4, 4, 8, 8, 8, *args, s) == L.MN_EINVAL, args
    for dims in ((0, 16, 4, 4), (1, 0, 4, 4), (1, 16, 0, 4), (1, 16, 4, 0)):
        assert lib.mn_i8poolfc_fwd(*dims, 8, 8, 8, t, c, p, s) == L.MN_EINVAL, dims
    assert (_host_u32(be, tab) == 0x5a5a5a5a).all() and (be.to_host(f) == 1).all() and (be.to_host(codes) == 77).all(), "nothing is written"
