"""The int8 deployment kernels with zero points (csrc/qgemm_iao8_zp.h: mn_i8zconv_*, mn_i8z_pack_codes, mn_i8z_unpack_codes) through the C ABI: one case table for the
CPU emulation build and the GPU.  Every comparison is exact.

A quantizer is (s, z, asym, bits): code range [lo, hi], stored byte = code - h, e = z + h (``qrange``, ``qh``).  The judge of a block is not the code under test:
``oracle.np_oracle.conv2d_fwd(..., acc=np.int64)`` on the integers J = j + e_a = code + z_a and K = k + e_w = code + z_w, zero padding the VALUES, gives S, and
    y = fl(fl(float(S) * al) + b), r = max(y, 0), c = code(r; s_out, z_out)      (pool: c1 = code(r; s_p, z_p), window maximum m, v = fl(fl(m + z_p) * s_p), c at out)
with code(r; s, z) = clamp(rha(fl(fl(r / s) - z)), lo, hi) is replayed step by step in numpy float32 (``chain_codes``).  The kernel's bytes must equal c - h_out bit
for bit in buffers that were poisoned before the launch.  ``torch_codes`` is the fp32 path -- a convolution of the fake-quantised values on the CPU -- against which
the judge itself is held to the one-step / 1e-4 cap of the GPU cross-check."""
import ctypes as C

import numpy as np

from oracle import np_oracle as O
from bits_cases import _dev_i32, _empty_i32, _host_u32
from codes_cases import shuffle_order
from iao8_cases import np_block, np_unblock, expect_positions

F = np.float32


def _lib():
    from micronet_amd import _lib as L
    return L


class Q:
    """One quantizer as the judge sees it."""

    def __init__(self, s, z=0.0, asym=0, bits=8):
        self.s, self.z, self.asym, self.bits = F(s), F(z), int(asym), int(bits)

    def ct(self):
        return _lib().I8ZQuant(float(self.s), float(self.z), self.asym, self.bits)

    def but(self, **kw):
        d = dict(s=self.s, z=self.z, asym=self.asym, bits=self.bits)
        d.update(kw)
        return Q(**d)


def qrange(asym, bits, act=True):
    if asym:
        return 0, (1 << bits) - (1 if act else 2)
    return (-(1 << (bits - 1)) if act else -((1 << (bits - 1)) - 1)), (1 << (bits - 1)) - 1


def qh(asym, bits, act=True):
    return ((1 << (bits - 1)) if act else (1 << (bits - 1)) - 1) if asym else 0


# ---------------------------------------------------------------------------------------------- the judge
def code_of(r, q, act=True):
    """clamp(rha(fl(fl(r / s) - z)), lo, hi) as float32."""
    lo, hi = qrange(q.asym, q.bits, act)
    v = ((np.asarray(r, dtype=F) / q.s).astype(F) - q.z).astype(F)
    return np.minimum(np.maximum(O.rha(v), F(lo)), F(hi)).astype(F)


def value_of(c, q):
    """fl(fl(c + z) * s)."""
    return ((np.asarray(c, dtype=F) + q.z).astype(F) * q.s).astype(F)


def chain_codes(S, al, b, q_p, q_out, pool):
    """The contract's chain on the exact S, one fp32 operation per step: the consumer's codes (not yet bytes)."""
    v = S.astype(F)                                                     # int -> float, round to nearest even
    y = ((v * al.reshape(1, -1, 1, 1).astype(F)).astype(F) + b.reshape(1, -1, 1, 1).astype(F)).astype(F)
    r = np.where(y > 0, y, F(0)).astype(F)
    if not pool:
        return code_of(r, q_out).astype(np.int32)
    c1 = code_of(r, q_p)
    N, Cc, H, W = c1.shape
    m = c1.reshape(N, Cc, H // 2, 2, W // 2, 2).max(axis=(3, 5))
    return code_of(value_of(m, q_p), q_out).astype(np.int32)


def judge(case, pool):
    return chain_codes(case["S"], case["al"], case["b"], case["q_p"], case["q_out"], pool)


def out_bytes(codes, q_out):
    return (codes - qh(q_out.asym, q_out.bits)).astype(np.int8)


def torch_codes(case, pool):
    """The fp32 path on the CPU: conv of the fake-quantised values + bias -> ReLU -> [fake-quant at the pool's quantizer -> max-pool] -> the consumer's code."""
    import torch
    import torch.nn.functional as TF
    x = torch.from_numpy(value_of(case["ca"], case["q_a"]))
    y = TF.conv2d(x, torch.from_numpy(case["w"]), torch.from_numpy(case["b"]), padding=case["KS"] // 2, groups=case["groups"])
    r = torch.relu(y).numpy()
    if pool:
        q = value_of(code_of(r, case["q_p"]), case["q_p"])
        N, Cc, H, W = q.shape
        r = q.reshape(N, Cc, H // 2, 2, W // 2, 2).max(axis=(3, 5))
    return code_of(r, case["q_out"]).astype(np.int32)


# ---------------------------------------------------------------------------------------------- inputs
def make_case(x_shape, Oc, KS, groups, seed, widths=(8, 8), a_asym=1, w_asym=1, out_asym=1, p_asym=None, z_a=0, z_w=(-185, -65), z_out=0, z_p=None, sp_ratio=1.0,
              per_channel=True, special=True, extreme=False, in_bits=None):
    """Codes, stored weights, quantizers and bias of one block, and its exact S.

    s_a = 2^-5; with ``special`` s_w[0] = 2^-7 and s_out = 2 al[0] = 2^-11 exactly, channel 0 has K = +1, +1, -1 at three places and 0 elsewhere and b = 0, so that
    fl(r / s_out) = S / 2 and EVERY odd S is a rounding tie; channel 1 is negative everywhere (the ReLU sends it to the value 0), channel 2 saturates at hi.  The other
    channels' s_w and b put the mean of y at 0.4 of the consumer's value range above its low end and one standard deviation at a quarter of the range.
    z_w: (low, high) drawn per channel, or one number; a symmetric quantizer takes z = 0.  in_bits: the width of the input codes where it is not the consumer's."""
    w_bits, a_bits = widths
    in_bits = a_bits if in_bits is None else in_bits
    r = np.random.default_rng(seed)
    N, Cc, H, W = x_shape
    Cg = Cc // groups
    p_asym = out_asym if p_asym is None else p_asym
    z_a = z_a if a_asym else 0
    z_out = z_out if out_asym else 0
    z_p = (z_out if z_p is None else z_p) if p_asym else 0
    lo_a, hi_a = qrange(a_asym, in_bits)
    lo_w, hi_w = qrange(w_asym, w_bits, False)
    lo_o, hi_o = qrange(out_asym, a_bits)
    nz = Oc if per_channel else 1
    if not w_asym:
        zw = np.zeros(nz, dtype=np.int64)
    elif isinstance(z_w, tuple):
        zw = r.integers(z_w[0], z_w[1] + 1, size=nz).astype(np.int64)
    else:
        zw = np.full(nz, z_w, dtype=np.int64)
    zw_full = np.broadcast_to(zw, (Oc,))
    if extreme:
        ca = np.full(x_shape, hi_a, dtype=np.int64)
        cw = np.full((Oc, Cg, KS, KS), hi_w, dtype=np.int64)
        cw[1::2] = lo_w
    else:
        ca = r.integers(lo_a, hi_a + 1, size=x_shape).astype(np.int64)
        ca[:, :, 0, 0] = min(max(-z_a, lo_a), hi_a)                      # a pixel of the value 0 (where it is a code), a pixel at either end of the range
        ca[0, :, -1, -1] = hi_a
        ca[0, :, 0, -1] = lo_a
        cw = r.integers(lo_w, hi_w + 1, size=(Oc, Cg, KS, KS)).astype(np.int64)
    tie = special and per_channel and not extreme
    if tie:
        cw[0] = -zw[0]
        cw[0].reshape(-1)[r.choice(Cg * KS * KS, size=3, replace=False)] = (1 - zw[0], 1 - zw[0], -1 - zw[0])
        assert lo_w <= cw[0].min() and cw[0].max() <= hi_w
    J, K = ca + z_a, cw + zw_full.reshape(-1, 1, 1, 1)
    S = O.conv2d_fwd(J, K, None, padding=KS // 2, groups=groups, acc=np.int64)          # zero padding of the values
    assert np.abs(S).max() < 2 ** 31
    s_a = F(2.0 ** -5)
    s_out = F(2.0 ** -11) if a_bits == 8 else F(2.0 ** -11 * 17)
    span = hi_o - lo_o
    Sf = S.astype(np.float64)
    sd, mean = Sf.std(axis=(0, 2, 3)) + 1.0, Sf.mean(axis=(0, 2, 3))
    if per_channel:
        s_w = np.maximum(0.25 * span * float(s_out) / sd / float(s_a), 1e-12).astype(F)
        if tie:
            s_w[0] = F(2.0 ** -7)
            s_out = F(F(2) * F(s_a * s_w[0]))
    else:
        s_w = np.full(1, 0.25 * span * float(s_out) / np.median(sd) / float(s_a), dtype=F)
    sw_full = np.broadcast_to(s_w, (Oc,)).astype(F)
    w = ((K.astype(F)) * sw_full.reshape(-1, 1, 1, 1)).astype(F)          # what prequantize_weights stores: fl(fl(code + z) * scale)
    al = (s_a * sw_full).astype(F)                                        # one fp32 multiply
    centre = (lo_o + z_out + 0.4 * span) * float(s_out)
    b = (centre - mean * al.astype(np.float64) + r.standard_normal(Oc) * 0.05 * span * float(s_out)).astype(F)
    if extreme:
        b = np.zeros(Oc, dtype=F)
    if tie:
        b[0] = F(0)
        if Oc >= 3:
            ymax = np.abs(S[:, 1:3]).max() * float(al[1:3].max())
            b[1] = F(-(ymax + 1.0))
            b[2] = F(ymax + (hi_o + z_out + 2) * float(s_out))
    q_a, q_out = Q(s_a, z_a, a_asym, in_bits), Q(s_out, z_out, out_asym, a_bits)
    q_p = Q(F(s_out * F(sp_ratio)), z_p, p_asym, a_bits)
    return dict(ca=ca, cw=cw, J=J, K=K, S=S, w=w, s_w=s_w, z_w=zw.astype(F), per_channel=per_channel, al=al, b=b, q_a=q_a, q_p=q_p, q_out=q_out, w_asym=int(w_asym),
                a_bits=a_bits, w_bits=w_bits, groups=groups, KS=KS, tie=tie)


def in_bytes(case, ca=None):
    ca = case["ca"] if ca is None else ca
    return (ca - qh(case["q_a"].asym, case["q_a"].bits)).astype(np.int8)


def assert_case_is_hard(case):
    """The properties the inputs must have, on the judge itself."""
    ref = judge(case, 0)
    q = case["q_out"]
    lo, hi = qrange(q.asym, q.bits)
    z = int(q.z)
    assert len(np.unique(ref)) > min(32, (1 << (q.bits - 1)) - 1), "the case must produce many codes"
    if case["tie"]:
        s0 = case["S"][:, 0]
        odd = (s0 > 0) & (s0 > 2 * (lo + z)) & (s0 < 2 * (hi + z)) & (s0 % 2 == 1)
        assert odd.any(), "odd S in range on the tie channel"
        v2 = s0[odd] - 2 * z                                             # twice the value that is rounded: odd, so a tie
        want = np.where(v2 > 0, (v2 + 1) // 2, -((-v2 + 1) // 2))
        assert np.array_equal(ref[:, 0][odd], want), "a tie rounds away from zero"
        zero = int(min(max(-z, lo), hi))
        assert (ref[:, 1] == zero).all() and (ref[:, 2] == hi).all(), "a channel the ReLU zeroes, a channel that saturates"
        assert (case["S"][:, 1] != 0).any()


# ---------------------------------------------------------------------------------------------- through the ABI
def geom_of(be, case, x_shape=None):
    return be.geom(case["ca"].shape if x_shape is None else x_shape, case["w"].shape, padding=case["KS"] // 2, groups=case["groups"])


def pack_table(be, g, case, order=None, rc=False, **kw):
    """mn_i8zconv_pack of the case, any of w, b, s_w, z_w, q_a, q_p, q_out replaced through ``kw``; returns the table (``rc``: the return code instead)."""
    a_bits, w_bits = case["a_bits"], case["w_bits"]
    nb = int(be.lib.mn_i8zconv_table_bytes(C.byref(g), a_bits, w_bits))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    get = lambda k: kw[k] if k in kw else case[k]
    dW, dS, dZ, dB = be.to_dev(get("w")), be.to_dev(get("s_w")), be.to_dev(get("z_w")), be.to_dev(get("b"))
    qa, qp, qo = get("q_a").ct(), get("q_p").ct(), get("q_out").ct()
    args = (C.byref(g), be.ptr(dW), be.ptr(dS), be.ptr(dZ), 1 if case["per_channel"] else 0, be.ptr(dB), C.byref(qa), C.byref(qp), C.byref(qo), case["w_asym"], w_bits,
            be.ptr(dO), be.ptr(table), be.stream)
    if rc:
        return be.lib.mn_i8zconv_pack(*args)
    be.call("mn_i8zconv_pack", *args)
    return table


COUNTERS = (0, 7, 13, 14, 15)


def counters(be, table):
    h = _host_u32(be, table)
    return tuple(int(h[i]) for i in COUNTERS)


def run_block(be, case, order, pool, ca=None):
    """Pack the table, run mn_i8zconv_fwd TWICE into poisoned buffers; returns (bytes [N, OB * 16, Ho, Wo] as the positions hold them, kernel name)."""
    ca = case["ca"] if ca is None else ca
    g = geom_of(be, case, ca.shape)
    assert be.lib.mn_i8zconv_supported(C.byref(g), case["a_bits"], case["w_bits"]) == 1
    table = pack_table(be, g, case, order)
    assert counters(be, table) == (0, 0, 0, 0, 0), "a valid table: %r" % (counters(be, table),)
    hdr = _host_u32(be, table)
    assert int(hdr[6]) == (case["a_bits"] | case["w_bits"] << 8 | case["q_a"].bits << 16)
    xb = be.to_dev_i8(np_block(in_bytes(case, ca)))
    N, _, H, W = ca.shape
    Oc = case["w"].shape[0]
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    OB = (Oc + 15) // 16
    outs = []
    for _ in range(2):
        yb = be.empty_i8((N, OB, Ho * Wo, 16))          # poisoned
        be.call("mn_i8zconv_fwd", C.byref(g), case["a_bits"], case["w_bits"], be.ptr(table), be.ptr(xb), be.ptr(yb), int(pool), be.stream)
        outs.append(be.to_host(yb))
    name = be.lib.mn_last_kernel().decode()
    assert np.array_equal(outs[0], outs[1]), "two runs give identical bytes"
    return np_unblock(outs[0], OB * 16, Ho, Wo), name


def _check(be, case, shuffle, pools, what):
    Oc = case["w"].shape[0]
    order = shuffle_order(Oc, shuffle) if shuffle else None
    for pool in pools:
        ref = judge(case, pool)
        got, name = run_block(be, case, order, pool)
        want = expect_positions(out_bytes(ref, case["q_out"]), order, (Oc + 15) // 16)
        bad = int((got != want).sum())
        print(name, what, "pool", pool, "mismatches against the judge", bad, "of", got.size, "distinct codes", len(np.unique(ref)))
        assert name == "k_i8zconv<%d,%d>" % (case["KS"], pool), name
        assert got.shape == want.shape and bad == 0, (bad, got.size)


# (id, x shape, O, KS, groups, out_order shuffle, seed, make_case keywords)
BLOCKS = [
    ("k1_nin_gc_l2", (2, 256, 8, 8), 256, 1, 2, 2, 5100, {}),                           # z_a = 0, z_w per channel in -185 .. -65: what the prepared nin_gc showed
    ("k1_partial_blocks", (3, 40, 5, 5), 33, 1, 1, 0, 5102, dict(z_a=-37)),             # tail channels and the padding slots must not enter the box sum
    ("k1_dead_rows", (1, 64, 4, 8), 48, 1, 2, 0, 5104, {}),                             # 24 rows per group
    ("k3_all_border", (1, 64, 2, 2), 32, 3, 4, 0, 5106, dict(z_a=-37)),                 # every pixel on the border; the padding byte is neither 0 nor -128
    ("k3_two_groups", (2, 32, 8, 8), 64, 3, 2, 0, 5105, dict(z_a=-5)),
    ("k3_sixteen_groups", (1, 256, 4, 4), 512, 3, 16, 2, 5107, {}),
]


def check_block(be, idx):
    name, x_shape, Oc, KS, groups, shuffle, seed, kw = BLOCKS[idx]
    case = make_case(x_shape, Oc, KS, groups, seed, **kw)
    assert_case_is_hard(case)
    if "z_a" in kw:
        pad = -(int(case["q_a"].z) + 128)
        assert pad not in (0, -128) and -128 <= pad <= 127
    pools = (0, 1) if x_shape[2] % 2 == 0 and x_shape[3] % 2 == 0 else (0,)
    _check(be, case, shuffle, pools, "%s %s -> %d k%d groups %d shuffle %d" % (name, x_shape, Oc, KS, groups, shuffle))


# mixes on one geometry: (id, make_case keywords)
MIX_GEOM = ((2, 64, 6, 6), 48, 1, 2)          # x shape, O, KS, groups
MIXES = [
    ("sym_act_asym_weight", dict(a_asym=0, out_asym=0)),
    ("asym_act_sym_weight", dict(w_asym=0, z_a=-9)),
    ("sym_in_asym_consumer", dict(a_asym=0, out_asym=1)),
    ("asym_in_sym_consumer", dict(a_asym=1, out_asym=0, z_a=-3)),
    ("pool_of_its_own", dict(sp_ratio=0.37, z_p=-3, z_out=-11)),
    ("sym_pool_asym_consumer", dict(p_asym=0, sp_ratio=1.9)),
    ("per_layer_weight", dict(per_channel=False, z_w=-120, z_a=-2)),
    ("w4a4", dict(widths=(4, 4), z_w=(-11, -4), z_a=-1)),
    # the input codes of another width than the consumer's (the pool's width is the consumer's): the packer takes lo / hi / h of each quantizer from its own bits
    ("a4_in_a8_out", dict(in_bits=4, z_a=-2, sp_ratio=0.6, z_p=-2)),
    ("a8_in_a4_out", dict(widths=(8, 4), in_bits=8, z_a=-7)),
]


def check_mix(be, idx):
    name, kw = MIXES[idx]
    x_shape, Oc, KS, groups = MIX_GEOM
    case = make_case(x_shape, Oc, KS, groups, 5300 + idx, **kw)
    if case["a_bits"] == 8:
        assert_case_is_hard(case)
    else:
        assert len(np.unique(judge(case, 0))) == 16, "all 4-bit codes"
    q_p, q_out = case["q_p"], case["q_out"]
    if (q_p.s, q_p.z, q_p.asym) != (q_out.s, q_out.z, q_out.asym):
        same = dict(case, q_p=q_out)
        assert not np.array_equal(judge(case, 1), judge(same, 1)), "a pool quantizer of its own must change pooled codes"
    _check(be, case, 0, (0, 1), name)


EXTREME = ("k1_extreme", (1, 1024, 2, 2), 32)          # every code at hi = 255 (e_a = 128) against every weight code at hi (z_w = 0) / at lo (z_w = -254): 16 k-steps


def check_extreme(be):
    name, x_shape, Oc = EXTREME
    case = make_case(x_shape, Oc, 1, 1, 5200, z_w=0, extreme=True)
    zw = np.zeros(Oc, dtype=np.int64)
    zw[1::2] = -254
    K = case["cw"] + zw.reshape(-1, 1, 1, 1)
    S = O.conv2d_fwd(case["J"], K, None, groups=1, acc=np.int64)
    # al = s_out = 2^-11: a unit of S is a unit of the code.  Row o aims at the code 8 o + 4: b = (target -+ S0) * 2^-11 is exact in fp32 (S0 is a multiple of 1024 below
    # 2^26, the target a multiple of 4), as are fl(float(S) * al) and the sum, so the judge's code IS the target -- distinct per row, none saturated -- and S off by the
    # fp32 spacing of its magnitude (4) moves every code
    S0 = 255 * 254 * 1024
    s_out = F(2.0 ** -11)
    s_w = np.full(Oc, s_out / F(2.0 ** -5), dtype=F)
    al = (F(2.0 ** -5) * s_w).astype(F)
    target = 8 * np.arange(Oc) + 4
    b = ((target - S[0, :, 0, 0]).astype(np.float64) * float(s_out)).astype(F)
    q = case["q_out"].but(s=s_out, z=0.0)
    case.update(K=K, S=S, z_w=zw.astype(F), s_w=s_w, al=al, b=b, q_out=q, q_p=q, w=(K.astype(F) * s_w.reshape(-1, 1, 1, 1)).astype(F))
    assert int(case["q_a"].z) + 128 == 128 and (case["ca"] == 255).all() and (al == s_out).all()
    assert int(S.min()) == -S0 and int(S.max()) == S0 and (np.abs(S) == S0).all()
    assert np.array_equal(b.astype(np.float64) / float(s_out), target - S[0, :, 0, 0]), "the bias is exact"
    for pool in (0, 1):
        ref = judge(case, pool)
        assert (ref == target.reshape(1, -1, 1, 1)).all() and ref.min() > 0 and ref.max() < 255, "every row at its own unsaturated code"
        off = judge(dict(case, S=S - 4), pool)
        assert (off == ref - 4).all(), "an S off by the spacing of fp32 at its magnitude moves every code"
    _check(be, case, 0, (0, 1), name)


def check_vs_torch(idx):
    """The cap of the GPU cross-check holds for the judge itself: against the fp32 path at most one step, on at most 1e-4 of the elements."""
    name, x_shape, Oc, KS, groups, _, seed, kw = BLOCKS[idx]
    case = make_case(x_shape, Oc, KS, groups, seed, special=False, **kw)
    for pool in ((0, 1) if x_shape[2] % 2 == 0 and x_shape[3] % 2 == 0 else (0,)):
        ref, par = judge(case, pool), torch_codes(case, pool)
        d = np.abs(ref - par)
        print(name, "pool", pool, "flips against the fp32 path", int((d != 0).sum()), "of", d.size, "largest", int(d.max()))
        assert d.max() <= 1 and (d != 0).mean() <= 1e-4


# ---------------------------------------------------------------------------------------------- several sets per block (tests/deploy_grid.py), GPU only
# (id, x shape, O, KS, groups, out_order shuffle, pool, seed, make_case keywords)
LARGE_GRID = [
    ("k1_nine_sets", (75, 16, 32, 32), 576, 1, 1, 0, 0, 5400, dict(z_a=-4)),
    ("k3_nine_sets_pool", (75, 16, 32, 32), 568, 3, 1, 4, 1, 5401, dict(z_a=-4)),
]
LARGE_HEAD = 25


def check_large(be, idx):
    """One LARGE_GRID case against the judge in chunks of 25 images, after proving through the library's own launch rule that a block takes at least two sets and the
    last block fewer."""
    import deploy_grid as DG
    name, x_shape, Oc, KS, groups, shuffle, pool, seed, kw = LARGE_GRID[idx]
    case = make_case((LARGE_HEAD,) + tuple(x_shape[1:]), Oc, KS, groups, seed, **kw)
    assert_case_is_hard(case)
    lo, hi = qrange(case["q_a"].asym, case["q_a"].bits)
    more = np.random.default_rng(seed + 500).integers(lo, hi + 1, size=(x_shape[0] - LARGE_HEAD,) + tuple(x_shape[1:])).astype(np.int64)
    ca = np.concatenate([case["ca"], more])
    N, _, H, W = x_shape
    OB = (Oc + 15) // 16
    bx = DG.pixel_blocks(N * (H // 2) * (W // 2), 64) if pool else DG.pixel_blocks(N * H * W, 256)
    gy, per = DG.assert_uneven_deal(be, bx, (OB + 3) // 4)
    order = shuffle_order(Oc, shuffle) if shuffle else None
    got, kname = run_block(be, case, order, pool, ca=ca)
    assert kname == "k_i8zconv<%d,%d>" % (KS, pool), kname
    bad = 0
    for n0 in range(0, N, LARGE_HEAD):
        S = DG.exact_conv(ca[n0:n0 + LARGE_HEAD] + int(case["q_a"].z), case["K"], KS // 2, groups)
        if n0 == 0:
            assert np.array_equal(S, case["S"])
        assert np.abs(S).max() < 2 ** 31
        ref = chain_codes(S, case["al"], case["b"], case["q_p"], case["q_out"], pool)
        want = expect_positions(out_bytes(ref, case["q_out"]), order, OB)
        bad += int((got[n0:n0 + ref.shape[0]] != want).sum())
    print(kname, name, x_shape, "->", Oc, "grid.y", gy, "per", per, "mismatches against the judge", bad, "of", got.size)
    assert bad == 0, (bad, got.size)


# ---------------------------------------------------------------------------------------------- pack / unpack
def check_pack_unpack(be, Cc, a_bits, z, shuffle=0, seed=0):
    """mn_i8z_pack_codes / mn_i8z_unpack_codes at an asymmetric quantizer against the judge's code_of and against mn_iao_fq_fwd with q_type = 1 on the same tensor."""
    r = np.random.default_rng(seed)
    N, H, W = 3, 5, 7
    q = Q(0.0371, z, 1, a_bits)
    lo, hi = qrange(1, a_bits)
    h = qh(1, a_bits)
    x = ((r.uniform(lo - 3, hi + 3, size=(N, Cc, H, W)) + z) * float(q.s)).astype(F)
    x[0, :, 0, 0] = ((np.arange(Cc) % 7 + z + F(0.5)) * q.s).astype(F)                    # rounding ties
    x[0, :, 0, 1] = ((hi - np.arange(Cc) % 7 + z - F(0.5)) * q.s).astype(F)
    order = shuffle_order(Cc, shuffle) if shuffle else None
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    CB = (Cc + 15) // 16
    qc = q.ct()
    codes = be.empty_i8((N, CB, H * W, 16))
    be.call("mn_i8z_pack_codes", be.ptr(be.to_dev(x)), N, Cc, H * W, C.byref(qc), be.ptr(dO), be.ptr(codes), be.stream)
    assert be.lib.mn_last_kernel().decode() == "k_i8z_pack"
    got = be.to_host(codes)
    ref = code_of(x, q)
    want = expect_positions((ref - h).astype(np.int8), order, CB)
    assert np.array_equal(np_unblock(got, CB * 16, H, W), want), "the consumer quantizer's bytes, zero tail bytes, every byte of the poisoned buffer written"
    assert len(np.unique(ref)) > min(32, hi // 2)
    # the library's own fake-quantizer (q_type 1) on the same tensor
    qp = be.to_dev(np.array([q.s, q.z, 0, 0], dtype=F))
    y = be.empty((N, Cc, H, W))
    be.call("mn_iao_fq_fwd", be.ptr(be.to_dev(x)), be.ptr(y), 1, x.size, be.ptr(qp), a_bits, 1, 1, be.stream)
    fq = be.to_host(y)
    assert np.array_equal(fq, value_of(ref, q)), "mn_iao_fq_fwd: the value of the judge's code"
    # unpack: fl(fl(c + z) * s) of every channel, the poisoned buffer overwritten; and the round trip back to the same bytes
    plain = be.empty_i8((N, CB, H * W, 16))
    be.call("mn_i8z_pack_codes", be.ptr(be.to_dev(x)), N, Cc, H * W, C.byref(qc), None, be.ptr(plain), be.stream)
    back = be.empty((N, Cc, H, W))
    be.call("mn_i8z_unpack_codes", be.ptr(plain), N, Cc, H * W, C.byref(qc), be.ptr(back), be.stream)
    assert be.lib.mn_last_kernel().decode() == "k_i8z_unpack"
    assert np.array_equal(be.to_host(back), fq)
    again = be.empty_i8((N, CB, H * W, 16))
    be.call("mn_i8z_pack_codes", be.ptr(back), N, Cc, H * W, C.byref(qc), None, be.ptr(again), be.stream)
    assert np.array_equal(be.to_host(again), be.to_host(plain)), "the quantizer on the unpacked values returns the same code"


def check_round_trip_all_codes(be, z, asym=1, a_bits=8):
    """unpack -> pack of every code returns the same bytes, also at |z| = 65535."""
    q = Q(0.0123, z, asym, a_bits)
    lo, hi = qrange(asym, a_bits)
    h = qh(asym, a_bits)
    Cc = hi - lo + 1
    bytes_ = (np.arange(lo, hi + 1) - h).astype(np.int8).reshape(1, Cc, 1, 1)
    blocked = be.to_dev_i8(np_block(bytes_))
    qc = q.ct()
    vals = be.empty((1, Cc, 1, 1))
    be.call("mn_i8z_unpack_codes", be.ptr(blocked), 1, Cc, 1, C.byref(qc), be.ptr(vals), be.stream)
    assert np.array_equal(be.to_host(vals).reshape(-1), value_of(np.arange(lo, hi + 1), q))
    again = be.empty_i8((1, (Cc + 15) // 16, 1, 16))
    be.call("mn_i8z_pack_codes", be.ptr(vals), 1, Cc, 1, C.byref(qc), None, be.ptr(again), be.stream)
    assert np.array_equal(be.to_host(again), np_block(bytes_))


# ---------------------------------------------------------------------------------------------- refusals, counters
def check_counters(be, seed=7):
    """Header words 0, 7, 13, 14, 15 count what makes a table unusable; a 1x1 stage takes a z_a that has no code for the value 0 and equals the judge."""
    case = make_case((1, 32, 4, 4), 32, 1, 1, seed, z_a=-5)
    g = geom_of(be, case)
    tab = pack_table(be, g, case)
    hdr = _host_u32(be, tab)
    assert counters(be, tab) == (0, 0, 0, 0, 0)
    assert (int(hdr[1]), int(hdr[4]), int(hdr[5]), int(hdr[23])) == (1, 1, 2, 2) and int(hdr[6]) == (8 | 8 << 8 | 8 << 16)
    assert int(hdr[21]) == 123 and int(hdr[24]) == 15
    assert hdr[8:13].view(F).tolist() == [case["q_p"].s, case["q_out"].s, F(0), F(255), case["q_a"].s]
    # word 0: non-finite constants
    b = case["b"].copy()
    b[9] = F(np.nan)
    assert counters(be, pack_table(be, g, case, b=b)) == (1, 0, 0, 0, 0)
    assert counters(be, pack_table(be, g, case, q_out=case["q_out"].but(s=np.inf)))[0] >= 1
    assert counters(be, pack_table(be, g, case, q_a=case["q_a"].but(s=0.0)))[0] >= 1
    # word 13: a zero point that is no integer, or beyond 65535
    for kw in (dict(q_a=case["q_a"].but(z=-4.5)), dict(q_p=case["q_p"].but(z=0.25)), dict(q_out=case["q_out"].but(z=70000.0)), dict(q_out=case["q_out"].but(z=np.nan))):
        c = counters(be, pack_table(be, g, case, **kw))
        assert c[2] == 1 and c[0] == 0, (kw, c)
    zw = case["z_w"].copy()
    zw[3] += F(0.5)
    zw[4] = F(-65536)
    c = counters(be, pack_table(be, g, case, z_w=zw))
    assert c[2] == 2 and c[1] >= 1, c                                     # (their rows' weights are off the grid as well)
    assert counters(be, pack_table(be, g, case, q_out=case["q_out"].but(z=65535.0)))[2] == 0
    # word 7: a weight off the grid, a weight code outside lo .. hi, an out_order entry >= O
    w2 = case["w"].copy()
    w2[5, 3, 0, 0] += F(0.5) * case["s_w"][5]
    assert counters(be, pack_table(be, g, case, w=w2)) == (0, 1, 0, 0, 0)
    w3 = case["w"].copy()
    w3[6, 1, 0, 0] = (F(255) + case["z_w"][6]) * case["s_w"][6]          # on the grid, the code 255 beyond hi = 254
    assert counters(be, pack_table(be, g, case, w=w3)) == (0, 1, 0, 0, 0)
    w4 = case["w"].copy()
    w4[7, 1, 0, 0] = (F(-1) + case["z_w"][7]) * case["s_w"][7]           # the code -1 below lo = 0
    assert counters(be, pack_table(be, g, case, w=w4)) == (0, 1, 0, 0, 0)
    order = np.arange(32)
    order[3] = 32
    assert counters(be, pack_table(be, g, case, order)) == (0, 1, 0, 0, 0)
    # word 14: the int32 bound, 1x1 with 1024 channels per group and z_a = -60000
    big = make_case((1, 1024, 2, 2), 32, 1, 1, seed + 1, special=False)
    gb = geom_of(be, big)
    assert counters(be, pack_table(be, gb, big)) == (0, 0, 0, 0, 0)
    assert counters(be, pack_table(be, gb, big, q_a=big["q_a"].but(z=-60000.0))) == (0, 0, 0, 32, 0)
    # ... and the bound is written in the width of the INPUT codes: symmetric weights, z_a = 16260: 1024 * (8 + 16268) * 127 fits, 1024 * (128 + 16388) * 127 does not
    narrow = make_case((1, 1024, 2, 2), 32, 1, 1, seed + 4, w_asym=0, z_a=16260, in_bits=4, special=False)
    assert 1024 * (8 + 16268) * 127 <= 2 ** 31 - 1 < 1024 * (128 + 16388) * 127
    assert counters(be, pack_table(be, gb, narrow)) == (0, 0, 0, 0, 0)
    assert int(_host_u32(be, pack_table(be, gb, narrow))[6]) == (8 | 8 << 8 | 4 << 16)
    assert counters(be, pack_table(be, gb, narrow, q_a=narrow["q_a"].but(bits=8))) == (0, 0, 0, 32, 0)
    # word 15: a 3x3 stage whose input quantizer has no code for the value 0; the same z_a on a 1x1 stage runs
    k3 = make_case((1, 32, 4, 4), 32, 3, 2, seed + 2, z_a=3, special=False)
    assert counters(be, pack_table(be, geom_of(be, k3), k3)) == (0, 0, 0, 0, 1)
    assert counters(be, pack_table(be, geom_of(be, k3), k3, q_a=k3["q_a"].but(z=-255.0))) == (0, 0, 0, 0, 0)
    assert counters(be, pack_table(be, geom_of(be, k3), k3, q_a=k3["q_a"].but(z=-256.0))) == (0, 0, 0, 0, 1)
    k1 = make_case((2, 32, 4, 4), 48, 1, 2, seed + 3, z_a=3)
    assert_case_is_hard(k1)
    _check(be, k1, 0, (0, 1), "1x1 with z_a = +3")


REFUSED = [
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1), stride=2), (8, 8)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), (8, 8)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 8, 3, 3), padding=1, groups=4), (8, 8)),          # a 3x3 with 8 channels per group
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=0), (8, 8)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (1, 8)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (9, 8)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (8, 9)),
]


def check_refused(be, idx):
    """What mn_i8conv_supported refuses, mn_i8zconv_supported refuses: MN_ENOTSUP, nothing written."""
    kw, (ab, wb) = REFUSED[idx]
    g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), groups=kw.get("groups", 1))
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.ones(64, dtype=F))
    ENOTSUP = _lib().MN_ENOTSUP
    q = Q(1.0, 0, 1, ab).ct()
    assert be.lib.mn_i8zconv_supported(C.byref(g), ab, wb) == 0 == be.lib.mn_i8conv_supported(C.byref(g), ab, wb)
    assert int(be.lib.mn_i8zconv_table_bytes(C.byref(g), ab, wb)) == 0
    assert be.lib.mn_i8zconv_pack(C.byref(g), be.ptr(f), be.ptr(f), be.ptr(f), 1, be.ptr(f), C.byref(q), C.byref(q), C.byref(q), 1, wb, None, be.ptr(buf),
                                  be.stream) == ENOTSUP
    for pool in (0, 1):
        assert be.lib.mn_i8zconv_fwd(C.byref(g), ab, wb, be.ptr(buf), be.ptr(buf), be.ptr(buf), pool, be.stream) == ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_invalid(be):
    """Null, misaligned, an invalid geometry, a flag outside 0 / 1 and odd H with pool are MN_EINVAL and write nothing; a pool outside 0 / 1 and a width outside
    2 .. 8 are MN_ENOTSUP."""
    L = _lib()
    g = be.geom((1, 32, 8, 8), (32, 32, 1, 1))
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.ones(64, dtype=F))
    odd = C.c_void_p(be.ptr(buf).value + 4)
    lib, s = be.lib, be.stream
    q = Q(1.0, 0, 1, 8).ct()
    qr = C.byref(q)
    fp, bp = be.ptr(f), be.ptr(buf)
    pk = lambda **kw: lib.mn_i8zconv_pack(kw.get("g", C.byref(g)), kw.get("w", fp), kw.get("s_w", fp), kw.get("z_w", fp), kw.get("stride", 1), fp, kw.get("qa", qr),
                                          kw.get("qp", qr), kw.get("qo", qr), kw.get("w_asym", 1), 8, None, kw.get("table", bp), s)
    for kw in (dict(w=None), dict(s_w=None), dict(table=None), dict(table=odd), dict(stride=2), dict(qa=None), dict(qp=None), dict(qo=None), dict(w_asym=2),
               dict(qa=C.byref(Q(1.0, 0, 2, 8).ct()))):
        assert pk(**kw) == L.MN_EINVAL, kw
    real = _empty_i32(be, (int(lib.mn_i8zconv_table_bytes(C.byref(g), 8, 8)) // 4,))
    w_ok = be.to_dev(np.zeros(32 * 32, dtype=F))
    assert pk(w=be.ptr(w_ok), z_w=None, table=be.ptr(real)) == L.MN_OK          # (no weight zero points: all 0)
    assert counters(be, real) == (0, 0, 0, 0, 0)
    assert pk(qo=C.byref(Q(1.0, 0, 1, 9).ct()), table=bp) == L.MN_ENOTSUP
    assert pk(qp=C.byref(Q(1.0, 0, 1, 4).ct()), table=bp) == L.MN_ENOTSUP          # the pool's width is the consumer's
    fw = lambda t=bp, x=bp, y=bp, pool=0, gg=g: lib.mn_i8zconv_fwd(C.byref(gg), 8, 8, t, x, y, pool, s)
    assert fw(t=None) == fw(x=None) == fw(y=None) == fw(x=odd) == fw(y=odd) == fw(t=odd) == L.MN_EINVAL
    assert fw(pool=2) == L.MN_ENOTSUP
    g0 = be.geom((0, 32, 8, 8), (32, 32, 1, 1))
    assert lib.mn_i8zconv_supported(C.byref(g0), 8, 8) == 0 and int(lib.mn_i8zconv_table_bytes(C.byref(g0), 8, 8)) == 0
    assert pk(g=C.byref(g0), table=bp) == L.MN_EINVAL and fw(gg=g0) == L.MN_EINVAL
    godd = be.geom((1, 32, 7, 8), (32, 32, 1, 1))
    assert lib.mn_i8zconv_supported(C.byref(godd), 8, 8) == 1 and fw(pool=1, gg=godd) == L.MN_EINVAL
    pc = lambda x=fp, N=1, q_=qr, out=bp: lib.mn_i8z_pack_codes(x, N, 16, 4, q_, None, out, s)
    up = lambda c=bp, Cc=16, q_=qr, y=fp: lib.mn_i8z_unpack_codes(c, 1, Cc, 4, q_, y, s)
    bad_q = [Q(0.0, 0, 1, 8), Q(1.0, 0.5, 1, 8), Q(1.0, 65536, 1, 8), Q(1.0, 0, 3, 8)]
    assert pc(x=None) == pc(out=None) == pc(out=odd) == pc(N=0) == pc(q_=None) == L.MN_EINVAL
    assert up(c=None) == up(y=None) == up(c=odd) == up(Cc=0) == up(q_=None) == L.MN_EINVAL
    for bq in bad_q:
        assert pc(q_=C.byref(bq.ct())) == L.MN_EINVAL and up(q_=C.byref(bq.ct())) == L.MN_EINVAL
    assert pc(q_=C.byref(Q(1.0, 0, 1, 9).ct())) == L.MN_ENOTSUP and up(q_=C.byref(Q(1.0, 0, 1, 1).ct())) == L.MN_ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all() and (be.to_host(f) == 1).all()


def check_symmetric_is_the_present_chain(be, seed=11):
    """Every quantizer symmetric with z = 0: k_i8zconv gives the bytes of k_i8conv on the same inputs."""
    import iao8_cases as IC
    old = IC.make_case((2, 64, 6, 6), 48, 1, 2, seed)
    got_old, _ = IC.run_block(be, old, None, 1)
    case = dict(ca=old["j"].astype(np.int64), w=old["w"], s_w=old["s_w"], z_w=np.zeros_like(old["s_w"]), b=old["b"], per_channel=True, w_asym=0, a_bits=8, w_bits=8,
                groups=2, KS=1, q_a=Q(old["s_a"]), q_p=Q(old["s_p"]), q_out=Q(old["s_out"]))
    got, name = run_block(be, case, None, 1)
    assert name == "k_i8zconv<1,1>" and np.array_equal(got, got_old)
    assert np.array_equal(got[:, :48], IC.judge(old, 1))
