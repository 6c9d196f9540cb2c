"""The int8 deployment kernels of the BN-folded IAO hidden blocks (csrc/qgemm_iao8.h: mn_i8conv_*, mn_i8_pack_codes, mn_i8_unpack_codes) through the C ABI: one case
table for the CPU emulation build and the GPU.  Every comparison is exact.

The judge of a block is not the code under test: ``oracle.np_oracle.conv2d_fwd(..., acc=np.int64)`` on the integer codes gives acc, and the chain
    y = fl(fl(float(acc) * al) + b), r = max(y, 0), c = clamp(rha(fl(r / s_out)))            (pool: c1 at s_p, window maximum, v = fl(m * s_p), c at s_out)
is replayed step by step in numpy float32 (``chain_codes``).  The kernel's bytes must equal it bit for bit in buffers that were poisoned before the launch.
``torch_codes`` is the parent's arithmetic -- an fp32 convolution of the fake-quantised values on the CPU -- against which the judge itself is held to the
one-step / 1e-4 cap of the GPU cross-check."""
import ctypes as C

import numpy as np

from oracle import np_oracle as O
from bits_cases import _dev_i32, _empty_i32, _host_u32
from codes_cases import shuffle_order

F = np.float32

# (id, x shape, O, KS, groups, out_order shuffle, seed)
BLOCKS = [
    ("k1_nin_gc_l2", (2, 256, 8, 8), 256, 1, 2, 2, 4100),
    ("k1_eight_per_group_pool", (1, 512, 4, 8), 512, 1, 4, 4, 4101),          # pooled: fewer pooled pixels than one tile
    ("k1_partial_blocks", (3, 40, 5, 5), 33, 1, 1, 0, 4102),                  # partial channel block, K padded to 64, partial output block, pixel remainder
    ("k1_half_a_step", (1, 128, 8, 8), 64, 1, 4, 0, 4103),
    ("k1_dead_rows", (1, 64, 4, 8), 48, 1, 2, 0, 4104),                       # 24 rows per group
    ("k3_two_groups", (2, 32, 8, 8), 64, 3, 2, 0, 4105),
    ("k3_all_border", (1, 64, 2, 2), 32, 3, 4, 0, 4106),                      # every pixel is on the border
    ("k3_sixteen_groups", (1, 256, 4, 4), 512, 3, 16, 2, 4107),
]
EXTREME = ("k1_extreme", (1, 1024, 2, 2), 32)          # every code at qmin against every weight code at +-127: 16 k-steps, |acc| = 128 * 127 * 1024
# chain variants on one geometry: (id, widths (w, a), per-channel s_w, s_p / s_out)
CHAIN_GEOM = ((2, 64, 6, 6), 48, 1, 2)          # x shape, O, KS, groups
CHAINS = [
    ("w8a8_per_channel", (8, 8), True, 1.0),
    ("w8a8_per_layer", (8, 8), False, 1.0),
    ("w8a8_pool_scale", (8, 8), True, 0.37),
    ("w4a4_per_channel", (4, 4), True, 1.0),
    ("w4a4_pool_scale", (4, 4), False, 1.9),
]

# (geometry keywords, (a_bits, w_bits))
REFUSED = [
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1), stride=2), (8, 8)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), (8, 8)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 8, 3, 3), padding=1, groups=4), (8, 8)),          # a 3x3 with 8 channels per group
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=0), (8, 8)),                   # padding mismatch
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1), padding=1), (8, 8)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=2, dilation=2), (8, 8)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (1, 8)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (9, 8)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (8, 1)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (8, 9)),
]


def _lib():
    from micronet_amd import _lib as L
    return L


def qrange(a_bits):
    return F(-(1 << (a_bits - 1))), F((1 << (a_bits - 1)) - 1)


# ---------------------------------------------------------------------------------------------- layout
def np_block(codes):
    """int8 [N, C, H, W] -> [N, ceil(C/16), H*W, 16], tail channels 0."""
    N, Cc, H, W = codes.shape
    CB = (Cc + 15) // 16
    full = np.zeros((N, CB * 16, H * W), dtype=np.int8)
    full[:, :Cc] = codes.reshape(N, Cc, H * W)
    return np.ascontiguousarray(full.reshape(N, CB, 16, H * W).transpose(0, 1, 3, 2))


def np_unblock(blocked, Cc, H, W):
    N, CB = blocked.shape[:2]
    return np.ascontiguousarray(blocked.transpose(0, 1, 3, 2).reshape(N, CB * 16, H, W)[:, :Cc])


# ---------------------------------------------------------------------------------------------- the judge
def code_of(r, s, a_bits):
    qmin, qmax = qrange(a_bits)
    return np.minimum(np.maximum(O.rha((r.astype(F) / F(s)).astype(F)), qmin), qmax).astype(F)


def chain_codes(acc, al, b, s_p, s_out, a_bits, pool):
    """The contract's chain on the exact accumulator, one fp32 operation per step."""
    v = acc.astype(F)                                                   # int -> float, round to nearest even
    y = ((v * al.reshape(1, -1, 1, 1).astype(F)).astype(F) + b.reshape(1, -1, 1, 1).astype(F)).astype(F)
    r = np.where(y > 0, y, F(0)).astype(F)
    if not pool:
        return code_of(r, s_out, a_bits).astype(np.int8)
    c1 = code_of(r, s_p, a_bits)
    N, Cc, H, W = c1.shape
    m = c1.reshape(N, Cc, H // 2, 2, W // 2, 2).max(axis=(3, 5))
    return code_of((m * F(s_p)).astype(F), s_out, a_bits).astype(np.int8)


def torch_codes(case, pool):
    """The parent's arithmetic on the CPU: fp32 conv of the fake-quantised values + bias -> ReLU -> [fake-quant at s_p -> max-pool] -> the consumer's code at s_out."""
    import torch
    import torch.nn.functional as TF
    x = torch.from_numpy((case["j"].astype(F) * case["s_a"]).astype(F))
    y = TF.conv2d(x, torch.from_numpy(case["w"]), torch.from_numpy(case["b"]), padding=case["KS"] // 2, groups=case["groups"])
    r = torch.relu(y).numpy()
    if pool:
        q = (code_of(r, case["s_p"], case["a_bits"]) * case["s_p"]).astype(F)
        N, Cc, H, W = q.shape
        r = q.reshape(N, Cc, H // 2, 2, W // 2, 2).max(axis=(3, 5))
    return code_of(r, case["s_out"], case["a_bits"]).astype(np.int8)


# ---------------------------------------------------------------------------------------------- inputs
def make_case(x_shape, Oc, KS, groups, seed, widths=(8, 8), per_channel=True, sp_ratio=1.0, special=True, extreme=False):
    """Codes, weights on the grid, scales and bias of one block, and its exact accumulator.

    Scales: s_a = 2^-5; s_w per channel (or one value); s_w[0] = 2^-7 and s_out = 2 al[0] = 2^-11 exactly, so that on channel 0 (sparse +-1 weights, b = 0)
    fl(r / s_out) = acc / 2 and EVERY odd acc is a rounding tie.  special (per-channel only): channel 1 is negative everywhere (the ReLU sends it to 0), channel 2
    saturates at qmax everywhere.  The other channels' s_w put about one to two thirds of qmax at one standard deviation of their accumulator."""
    w_bits, a_bits = widths
    r = np.random.default_rng(seed)
    N, Cc, H, W = x_shape
    Cg = Cc // groups
    qmin, qmax = (int(v) for v in qrange(a_bits))
    kmax = (1 << (w_bits - 1)) - 1
    if extreme:
        j = np.full(x_shape, qmin, dtype=np.int64)
        k = np.full((Oc, Cg, KS, KS), kmax, dtype=np.int64)
        k[1::2] = -kmax
    else:
        j = r.integers(qmin, qmax + 1, size=x_shape).astype(np.int64)
        j[:, :, 0, 0] = 0                                                # a whole-zero pixel, a pixel at either end of the range
        j[0, :, -1, -1] = qmax
        j[0, :, 0, -1] = qmin
        k = r.integers(-kmax, kmax + 1, size=(Oc, Cg, KS, KS)).astype(np.int64)
    tie = special and per_channel and not extreme
    if tie:
        k[0] = 0
        k[0].reshape(-1)[r.choice(Cg * KS * KS, size=3, replace=False)] = (1, 1, -1)
    acc = O.conv2d_fwd(j, k, None, padding=KS // 2, groups=groups, acc=np.int64)
    assert np.abs(acc).max() < 2 ** 31
    s_a = F(2.0 ** -5)
    sd = acc.astype(np.float64).std(axis=(0, 2, 3)) + 1.0
    if per_channel:
        s_w = (F(2.0 ** -7) * r.uniform(1.0, 2.0, size=Oc)).astype(F)
        if tie:
            s_w[0] = F(2.0 ** -7)                                        # al[0] a power of two: fl(acc * al[0]) and the quotient by 2 al[0] are exact
        al0 = F(s_a * s_w[0])
        s_out = F(2) * al0 if tie else F(al0 * F(sd[0] / (0.5 * qmax)))
        # al[o] * sd[o] / s_out = frac * qmax
        frac = r.uniform(0.3, 0.7, size=Oc)
        want = (frac * qmax * float(s_out) / sd / float(s_a)).astype(F)
        if tie:
            want[0] = s_w[0]
        s_w = np.maximum(want, F(1e-12)).astype(F)
    else:
        s_w = np.full(1, F(2.0 ** -7) * F(r.uniform(1.0, 2.0)), dtype=F)
        al0 = F(s_a * s_w[0])
        s_out = F(al0 * F(np.median(sd) / (0.5 * qmax)))
    sw_full = np.broadcast_to(s_w, (Oc,)) if not per_channel else s_w
    w = (k.astype(F) * sw_full.reshape(-1, 1, 1, 1).astype(F)).astype(F)          # what prequantize_weights stores: code * scale
    al = (s_a * sw_full).astype(F)                                                 # one fp32 multiply
    b = (r.standard_normal(Oc) * 0.25 * qmax * float(s_out)).astype(F)
    if tie:
        b[0] = F(0)
        if Oc >= 3:
            ymax = np.abs(acc[:, 1:3]).max() * float(al[1:3].max())
            b[1] = F(-(ymax + 1.0))
            b[2] = F(ymax + (qmax + 2) * float(s_out))
    s_p = F(s_out * F(sp_ratio))
    return dict(j=j.astype(np.int8), k=k, w=w, acc=acc, s_a=s_a, s_w=s_w, per_channel=per_channel, al=al, b=b, s_p=s_p, s_out=s_out, a_bits=a_bits, w_bits=w_bits,
                groups=groups, KS=KS, tie=tie)


def judge(case, pool):
    return chain_codes(case["acc"], case["al"], case["b"], case["s_p"], case["s_out"], case["a_bits"], pool)


def assert_case_is_hard(case):
    """The properties the issue asks the inputs to have, on the judge itself."""
    ref = judge(case, 0)
    qmin, qmax = (int(v) for v in qrange(case["a_bits"]))
    assert len(np.unique(ref)) > min(32, qmax), "the case must produce many codes"
    if case["tie"]:
        a0 = case["acc"][:, 0]
        odd = (a0 > 0) & (a0 < 2 * qmax) & (a0 % 2 == 1)
        assert odd.any(), "odd accumulators in range on the tie channel"
        assert np.array_equal(ref[:, 0][odd], ((a0[odd] + 1) // 2).astype(np.int8)), "a tie rounds away from zero"
        assert (ref[:, 1] == 0).all() and (ref[:, 2] == qmax).all(), "a channel the ReLU zeroes, a channel that saturates"
        assert (case["acc"][:, 1] != 0).any()


# ---------------------------------------------------------------------------------------------- through the ABI
def pack_table(be, g, case, order=None, w=None, b=None, s_w=None, s_a=None, s_p=None, s_out=None):
    a_bits, w_bits = case["a_bits"], case["w_bits"]
    nb = int(be.lib.mn_i8conv_table_bytes(C.byref(g), a_bits, w_bits))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    dW, dS, dB = be.to_dev(case["w"] if w is None else w), be.to_dev(case["s_w"] if s_w is None else s_w), be.to_dev(case["b"] if b is None else b)
    sv = lambda v, d: C.c_float(float(d if v is None else v))
    be.call("mn_i8conv_pack", C.byref(g), be.ptr(dW), be.ptr(dS), 1 if case["per_channel"] else 0, be.ptr(dB), sv(s_a, case["s_a"]), sv(s_p, case["s_p"]),
            sv(s_out, case["s_out"]), a_bits, w_bits, be.ptr(dO), be.ptr(table), be.stream)
    return table


def geom_of(be, case):
    return be.geom(case["j"].shape, case["w"].shape, padding=case["KS"] // 2, groups=case["groups"])


def run_block(be, case, order, pool):
    """Pack the table, run mn_i8conv_fwd TWICE into poisoned buffers; returns (codes [N, OB * 16, Ho, Wo] as the positions hold them, kernel name)."""
    g = geom_of(be, case)
    assert be.lib.mn_i8conv_supported(C.byref(g), case["a_bits"], case["w_bits"]) == 1
    table = pack_table(be, g, case, order)
    hdr = _host_u32(be, table)
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0, "finite constants, weights on the grid, a valid order: %d %d" % (int(hdr[0]), int(hdr[7]))
    assert int(hdr[6]) == (case["a_bits"] | case["w_bits"] << 8)
    xb = be.to_dev_i8(np_block(case["j"]))
    N, _, H, W = case["j"].shape
    Oc = case["w"].shape[0]
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    OB = (Oc + 15) // 16
    outs = []
    for _ in range(2):
        yb = be.empty_i8((N, OB, Ho * Wo, 16))          # poisoned
        be.call("mn_i8conv_fwd", C.byref(g), case["a_bits"], case["w_bits"], be.ptr(table), be.ptr(xb), be.ptr(yb), int(pool), be.stream)
        outs.append(be.to_host(yb))
    name = be.lib.mn_last_kernel().decode()
    assert np.array_equal(outs[0], outs[1]), "two runs give identical bytes"
    return np_unblock(outs[0], OB * 16, Ho, Wo), name


def expect_positions(ref, order, OB):
    """What the positions of the output hold: channel order[j] at position j, 0 past O."""
    N, Oc, Ho, Wo = ref.shape
    out = np.zeros((N, OB * 16, Ho, Wo), dtype=np.int8)
    out[:, :Oc] = ref[:, order] if order is not None else ref
    return out


def _check(be, case, shuffle, pools, what):
    Oc = case["w"].shape[0]
    order = shuffle_order(Oc, shuffle) if shuffle else None
    for pool in pools:
        ref = judge(case, pool)
        got, name = run_block(be, case, order, pool)
        want = expect_positions(ref, order, (Oc + 15) // 16)
        bad = int((got != want).sum())
        print(name, what, "pool", pool, "mismatches against the judge", bad, "of", got.size, "distinct codes", len(np.unique(ref)))
        assert name == "k_i8conv<%d,%d>" % (case["KS"], pool), name
        assert got.shape == want.shape and bad == 0, (bad, got.size)


def check_block(be, idx):
    name, x_shape, Oc, KS, groups, shuffle, seed = BLOCKS[idx]
    case = make_case(x_shape, Oc, KS, groups, seed)
    assert_case_is_hard(case)
    pools = (0, 1) if x_shape[2] % 2 == 0 and x_shape[3] % 2 == 0 else (0,)
    _check(be, case, shuffle, pools, "%s %s -> %d k%d groups %d shuffle %d" % (name, x_shape, Oc, KS, groups, shuffle))


# ---------------------------------------------------------------------------------------------- several sets per block (tests/deploy_grid.py)
# The smallest shapes at which a block of k_i8conv takes more than one set: (id, x shape, O, KS, groups, out_order shuffle, pool, seed).  16 channels keep the judge
# cheap; the pixels cannot shrink (the loop is entered once the pixel blocks alone fill the chip).  GPU only (tests/test_gpu_iao8.py): on the CPU emulation build
# (8 cores) a case takes 44 to 114 s, against one to four seconds on the MI355X.
LARGE_GRID = [
    ("k1_nine_sets", (75, 16, 32, 32), 576, 1, 1, 0, 0, 4400),               # bx 300, 9 sets: 5 blocks of 2, the last takes 1.  Emulated: 46 s
    ("k1_nine_sets_pool", (75, 16, 32, 32), 568, 1, 1, 4, 1, 4401),          # pooled: 19200 / 64 = 300 blocks; shuffle 4; the last set's last block half empty.  44 s
    ("k3_nine_sets", (75, 16, 32, 32), 568, 3, 1, 4, 0, 4402),               # the 3x3 form, 16 channels per group.  114 s
    ("k3_nine_sets_pool", (75, 16, 32, 32), 576, 3, 1, 0, 1, 4403),
    # five sets dealt 3 + 2 over two rows: the last set, with positions past O that no row writes, is the SECOND of its block -- its bytes are whatever the read-back
    # of the set before left in the LDS image (in the cases above the last set is the first of its block, or every byte of a set is overwritten)
    ("k1_last_set_second", (256, 16, 32, 32), 312, 1, 1, 4, 0, 4404),        # bx 1024, 5 sets.  80 s
    ("k1_last_set_second_pool", (256, 16, 32, 32), 312, 1, 1, 0, 1, 4405),   # pooled: 65536 / 64 = 1024 blocks
]
LARGE_HEAD = 25          # images make_case builds the block from (scales, bias, special channels, hardness); the rest of the batch is drawn from the same range


def large_case(x_shape, Oc, KS, groups, seed):
    """(case of the first LARGE_HEAD images -- the family's make_case, held to assert_case_is_hard --, codes int8 of the whole batch)."""
    head = min(LARGE_HEAD, x_shape[0])
    case = make_case((head,) + tuple(x_shape[1:]), Oc, KS, groups, seed)
    assert_case_is_hard(case)
    qmin, qmax = (int(v) for v in qrange(case["a_bits"]))
    more = np.random.default_rng(seed + 500).integers(qmin, qmax + 1, size=(x_shape[0] - head,) + tuple(x_shape[1:])).astype(np.int8)
    more[:, :, 0, 0] = 0          # (make_case's whole-zero pixel)
    return case, np.concatenate([case["j"], more])


def judge_chunks(case, j, pool):
    """The judge on the whole batch, LARGE_HEAD images at a time: (first image, codes) per chunk.  The first chunk is the case's own accumulator."""
    import deploy_grid as DG
    for n0 in range(0, j.shape[0], LARGE_HEAD):
        acc = DG.exact_conv(j[n0:n0 + LARGE_HEAD], case["k"], case["KS"] // 2, case["groups"])
        if n0 == 0:
            assert np.array_equal(acc, case["acc"])
        assert np.abs(acc).max() < 2 ** 31
        yield n0, chain_codes(acc, case["al"], case["b"], case["s_p"], case["s_out"], case["a_bits"], pool)


def check_large(be, idx):
    """One LARGE_GRID case through run_block (poisoned buffers, two identical runs, the kernel's name) against the judge, after proving through the library's own
    launch rule that a block takes at least two sets and the last block fewer."""
    import deploy_grid as DG
    name, x_shape, Oc, KS, groups, shuffle, pool, seed = LARGE_GRID[idx]
    case, j = large_case(x_shape, Oc, KS, groups, seed)
    N, _, H, W = x_shape
    OB = (Oc + 15) // 16
    bx = DG.pixel_blocks(N * (H // 2) * (W // 2), 64) if pool else DG.pixel_blocks(N * H * W, 256)
    nsets = (OB + 3) // 4
    gy, per = DG.assert_uneven_deal(be, bx, nsets)
    if "last_set_second" in name:
        assert nsets - (gy - 1) * per >= 2 and Oc % 64, "the last block takes two sets at least, and the last of them has positions past O"
    order = shuffle_order(Oc, shuffle) if shuffle else None
    got, kname = run_block(be, dict(case, j=j), order, pool)
    assert kname == "k_i8conv<%d,%d>" % (KS, pool), kname
    bad = 0
    for n0, ref in judge_chunks(case, j, pool):
        want = expect_positions(ref, order, OB)
        bad += int((got[n0:n0 + ref.shape[0]] != want).sum())
    print(kname, name, x_shape, "->", Oc, "grid.y", gy, "per", per, "mismatches against the judge", bad, "of", got.size)
    assert bad == 0, (bad, got.size)


def check_extreme(be):
    name, x_shape, Oc = EXTREME
    case = make_case(x_shape, Oc, 1, 1, 4200, extreme=True)
    assert int(np.abs(case["acc"]).max()) == 128 * 127 * 1024 and int(case["acc"].min()) == -128 * 127 * 1024
    assert len(np.unique(judge(case, 0))) >= 2
    _check(be, case, 0, (0, 1), name)


def check_chain(be, idx):
    name, widths, per_channel, ratio = CHAINS[idx]
    x_shape, Oc, KS, groups = CHAIN_GEOM
    case = make_case(x_shape, Oc, KS, groups, 4300 + idx, widths=widths, per_channel=per_channel, sp_ratio=ratio)
    if widths[1] == 8:
        assert_case_is_hard(case)
    else:
        assert len(np.unique(judge(case, 0))) == 8, "all non-negative 4-bit codes"
    if ratio != 1.0:
        same = dict(case, s_p=case["s_out"])
        assert not np.array_equal(judge(case, 1), judge(same, 1)), "s_p != s_out must change pooled codes"
    _check(be, case, 0, (0, 1), name)


def check_vs_torch(idx):
    """The cap of the GPU cross-check holds for the judge itself: against the parent's fp32 arithmetic at most one step, on at most 1e-4 of the elements."""
    _, x_shape, Oc, KS, groups, _, seed = BLOCKS[idx]
    case = make_case(x_shape, Oc, KS, groups, seed, special=False)
    for pool in ((0, 1) if x_shape[2] % 2 == 0 and x_shape[3] % 2 == 0 else (0,)):
        ref, par = judge(case, pool).astype(np.int32), torch_codes(case, pool).astype(np.int32)
        d = np.abs(ref - par)
        print(BLOCKS[idx][0], "pool", pool, "flips against the fp32 path", int((d != 0).sum()), "of", d.size, "largest", int(d.max()))
        assert d.max() <= 1 and (d != 0).mean() <= 1e-4


# ---------------------------------------------------------------------------------------------- pack / unpack
def check_pack_unpack(be, Cc, a_bits, shuffle=0, seed=0):
    r = np.random.default_rng(seed)
    N, H, W = 3, 5, 7
    qmin, qmax = qrange(a_bits)
    s = F(0.0371)
    x = (r.standard_normal((N, Cc, H, W)) * float(s) * float(qmax) * 0.7).astype(F)
    x[0, :, 0, 0] = (np.arange(Cc) % 7 + F(0.5)) * s                    # rounding ties
    x[0, :, 0, 1] = -(np.arange(Cc) % 7 + F(0.5)) * s
    order = shuffle_order(Cc, shuffle) if shuffle else None
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    CB = (Cc + 15) // 16
    codes = be.empty_i8((N, CB, H * W, 16))
    be.call("mn_i8_pack_codes", be.ptr(be.to_dev(x)), N, Cc, H * W, C.c_float(float(s)), a_bits, be.ptr(dO), be.ptr(codes), be.stream)
    got = be.to_host(codes)
    ref = code_of(x, s, a_bits)
    want = expect_positions(ref.astype(np.int8), order, CB)
    assert np.array_equal(np_unblock(got, CB * 16, H, W), want), "the consumer quantizer's codes, zero tail channels, every byte of the poisoned buffer written"
    # the library's own fake-quantizer on the same tensor, divided back to codes
    qp = be.to_dev(np.array([s, 0, 0, 0], dtype=F))
    y = be.empty((N, Cc, H, W))
    be.call("mn_iao_fq_fwd", be.ptr(be.to_dev(x)), be.ptr(y), 1, x.size, be.ptr(qp), a_bits, 0, 1, be.stream)
    fq = be.to_host(y)
    assert np.array_equal(O.rha((fq / s).astype(F)), ref), "mn_iao_fq_fwd / s"
    assert len(np.unique(ref)) > min(32, int(qmax))
    # unpack: fl(c * s) of every channel, the poisoned buffer overwritten; and the round trip back to the same codes
    plain = be.empty_i8((N, CB, H * W, 16))
    be.call("mn_i8_pack_codes", be.ptr(be.to_dev(x)), N, Cc, H * W, C.c_float(float(s)), a_bits, None, be.ptr(plain), be.stream)
    back = be.empty((N, Cc, H, W))
    be.call("mn_i8_unpack_codes", be.ptr(plain), N, Cc, H * W, C.c_float(float(s)), be.ptr(back), be.stream)
    vals = be.to_host(back)
    assert np.array_equal(vals, (ref * s).astype(F)) and np.array_equal(vals, fq)
    again = be.empty_i8((N, CB, H * W, 16))
    be.call("mn_i8_pack_codes", be.ptr(back), N, Cc, H * W, C.c_float(float(s)), a_bits, None, be.ptr(again), be.stream)
    assert np.array_equal(be.to_host(again), be.to_host(plain)), "fl(fl(c s) / s) rounds back to c"


# ---------------------------------------------------------------------------------------------- refusals, counters
def check_refused(be, idx):
    kw, (ab, wb) = REFUSED[idx]
    g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), dilation=kw.get("dilation", 1), groups=kw.get("groups", 1))
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.ones(64, dtype=F))
    one = C.c_float(1.0)
    ENOTSUP = _lib().MN_ENOTSUP
    assert be.lib.mn_i8conv_supported(C.byref(g), ab, wb) == 0
    assert int(be.lib.mn_i8conv_table_bytes(C.byref(g), ab, wb)) == 0
    assert be.lib.mn_i8conv_pack(C.byref(g), be.ptr(f), be.ptr(f), 1, be.ptr(f), one, one, one, ab, wb, None, be.ptr(buf), be.stream) == ENOTSUP
    for pool in (0, 1):
        assert be.lib.mn_i8conv_fwd(C.byref(g), ab, wb, be.ptr(buf), be.ptr(buf), be.ptr(buf), pool, be.stream) == ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_invalid(be):
    """Null, misaligned, an invalid geometry and odd H with pool are MN_EINVAL and write nothing; a pool outside 0 / 1 is MN_ENOTSUP."""
    L = _lib()
    g = be.geom((1, 32, 8, 8), (32, 32, 1, 1))
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.ones(64, dtype=F))
    one = C.c_float(1.0)
    odd = C.c_void_p(be.ptr(buf).value + 4)
    lib, s = be.lib, be.stream
    assert lib.mn_i8conv_pack(C.byref(g), None, be.ptr(f), 1, be.ptr(f), one, one, one, 8, 8, None, be.ptr(buf), s) == L.MN_EINVAL
    assert lib.mn_i8conv_pack(C.byref(g), be.ptr(f), None, 1, be.ptr(f), one, one, one, 8, 8, None, be.ptr(buf), s) == L.MN_EINVAL
    assert lib.mn_i8conv_pack(C.byref(g), be.ptr(f), be.ptr(f), 1, be.ptr(f), one, one, one, 8, 8, None, None, s) == L.MN_EINVAL
    assert lib.mn_i8conv_pack(C.byref(g), be.ptr(f), be.ptr(f), 1, be.ptr(f), one, one, one, 8, 8, None, odd, s) == L.MN_EINVAL
    assert lib.mn_i8conv_pack(C.byref(g), be.ptr(f), be.ptr(f), 2, be.ptr(f), one, one, one, 8, 8, None, be.ptr(buf), s) == L.MN_EINVAL
    assert lib.mn_i8conv_fwd(C.byref(g), 8, 8, None, be.ptr(buf), be.ptr(buf), 0, s) == L.MN_EINVAL
    assert lib.mn_i8conv_fwd(C.byref(g), 8, 8, be.ptr(buf), None, be.ptr(buf), 0, s) == L.MN_EINVAL
    assert lib.mn_i8conv_fwd(C.byref(g), 8, 8, be.ptr(buf), be.ptr(buf), None, 0, s) == L.MN_EINVAL
    assert lib.mn_i8conv_fwd(C.byref(g), 8, 8, be.ptr(buf), odd, be.ptr(buf), 0, s) == L.MN_EINVAL
    assert lib.mn_i8conv_fwd(C.byref(g), 8, 8, be.ptr(buf), be.ptr(buf), odd, 0, s) == L.MN_EINVAL
    assert lib.mn_i8conv_fwd(C.byref(g), 8, 8, be.ptr(buf), be.ptr(buf), be.ptr(buf), 2, s) == L.MN_ENOTSUP
    g0 = be.geom((0, 32, 8, 8), (32, 32, 1, 1))
    assert lib.mn_i8conv_supported(C.byref(g0), 8, 8) == 0 and int(lib.mn_i8conv_table_bytes(C.byref(g0), 8, 8)) == 0
    assert lib.mn_i8conv_pack(C.byref(g0), be.ptr(f), be.ptr(f), 1, be.ptr(f), one, one, one, 8, 8, None, be.ptr(buf), s) == L.MN_EINVAL
    assert lib.mn_i8conv_fwd(C.byref(g0), 8, 8, be.ptr(buf), be.ptr(buf), be.ptr(buf), 0, s) == L.MN_EINVAL
    godd = be.geom((1, 32, 7, 8), (32, 32, 1, 1))
    assert lib.mn_i8conv_supported(C.byref(godd), 8, 8) == 1
    assert lib.mn_i8conv_fwd(C.byref(godd), 8, 8, be.ptr(buf), be.ptr(buf), be.ptr(buf), 1, s) == L.MN_EINVAL
    assert lib.mn_i8_pack_codes(None, 1, 16, 4, one, 8, None, be.ptr(buf), s) == L.MN_EINVAL
    assert lib.mn_i8_pack_codes(be.ptr(f), 1, 16, 4, one, 8, None, None, s) == L.MN_EINVAL
    assert lib.mn_i8_pack_codes(be.ptr(f), 1, 16, 4, one, 8, None, odd, s) == L.MN_EINVAL
    assert lib.mn_i8_pack_codes(be.ptr(f), 0, 16, 4, one, 8, None, be.ptr(buf), s) == L.MN_EINVAL
    assert lib.mn_i8_pack_codes(be.ptr(f), 1, 16, 4, C.c_float(0.0), 8, None, be.ptr(buf), s) == L.MN_EINVAL
    assert lib.mn_i8_pack_codes(be.ptr(f), 1, 16, 4, one, 9, None, be.ptr(buf), s) == L.MN_ENOTSUP
    assert lib.mn_i8_unpack_codes(None, 1, 16, 4, one, be.ptr(f), s) == L.MN_EINVAL
    assert lib.mn_i8_unpack_codes(be.ptr(buf), 1, 16, 4, one, None, s) == L.MN_EINVAL
    assert lib.mn_i8_unpack_codes(odd, 1, 16, 4, one, be.ptr(f), s) == L.MN_EINVAL
    assert lib.mn_i8_unpack_codes(be.ptr(buf), 1, 0, 4, one, be.ptr(f), s) == L.MN_EINVAL
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all() and (be.to_host(f) == 1).all()


def check_counters(be, seed=7):
    """Word 0 counts a NaN bias and an infinite scale, word 7 a weight off the grid and an out_order entry >= O; a bad entry's position yields 0 bytes."""
    case = make_case((1, 32, 4, 4), 32, 1, 1, seed)
    g = geom_of(be, case)
    hdr = _host_u32(be, pack_table(be, g, case))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0
    assert (int(hdr[1]), int(hdr[4]), int(hdr[5])) == (1, 1, 2) and int(hdr[6]) == (8 | 8 << 8)
    assert hdr[8:13].view(F).tolist() == [case["s_p"], case["s_out"], F(-128), F(127), case["s_a"]]
    b = case["b"].copy()
    b[9] = F(np.nan)
    hdr = _host_u32(be, pack_table(be, g, case, b=b))
    assert int(hdr[0]) == 1 and int(hdr[7]) == 0
    for kw in (dict(s_out=np.inf), dict(s_p=np.inf), dict(s_a=np.inf), dict(s_out=0.0), dict(s_out=-1.0)):
        hdr = _host_u32(be, pack_table(be, g, case, **kw))
        assert int(hdr[0]) >= 1 and int(hdr[7]) == 0, kw
    sw = case["s_w"].copy()
    sw[4] = F(np.inf)
    assert int(_host_u32(be, pack_table(be, g, case, s_w=sw))[0]) >= 1
    w2 = case["w"].copy()
    w2[5, 3, 0, 0] += F(0.5) * case["s_w"][5]
    hdr = _host_u32(be, pack_table(be, g, case, w=w2))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 1
    w3 = case["w"].copy()
    w3[6, 1, 0, 0] = F(128) * case["s_w"][6]                             # on the grid, beyond 2^(w-1) - 1
    assert int(_host_u32(be, pack_table(be, g, case, w=w3))[7]) == 1
    order = np.arange(32)
    order[3] = 32
    table = pack_table(be, g, case, order)
    assert int(_host_u32(be, table)[7]) == 1
    xb = be.to_dev_i8(np_block(case["j"]))
    yb = be.empty_i8((1, 2, 16, 16))
    be.call("mn_i8conv_fwd", C.byref(g), 8, 8, be.ptr(table), be.ptr(xb), be.ptr(yb), 0, be.stream)
    ref = judge(case, 0)
    ref[:, 3] = 0
    assert np.array_equal(np_unblock(be.to_host(yb), 32, 4, 4), ref)
