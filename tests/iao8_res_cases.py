"""The residual stages of the int8 deployment of BN-folded IAO ResNets (csrc/qgemm_iao8_res.h: mn_i8res_*) through the C ABI: one case table for the CPU emulation
build (tests/test_iao8_res_emulated.py) and the GPU (tests/test_gpu_iao8_res.py).  Every kernel comparison is exact, in buffers poisoned before the launch, with a
guard region behind every output.

The judge is not the code under test: ``oracle.np_oracle.conv2d_fwd(..., acc=np.int64, stride=...)`` on the integer codes gives acc, and the contract's chain
    conv stage : y = fl(fl(float(acc) * al) + b), r = relu ? max(y, 0) : y, c = Q(r; s_out, out_bits)
    add stage  : c_r = Q(y; s_add, add_bits), t = fl(fl(float(c_r) * s_add) + fl(float(c_s) * s_add)), v = max(t, 0), out_k = Q(v; s_k, bits_k)
is replayed step by step in numpy float32.  Inputs come from ``iao8_cases.make_case`` (a stride-2 accumulator of a padding-(KS - 1) / 2 conv is the stride-1 one at the
even pixels, so its tie channel, its ReLU-zeroed channel and its saturating channel carry over; asserted).  ``torch_conv`` / ``torch_add`` are the fp32 path's
arithmetic on the CPU, against which the judge itself is held to the one-step / 1e-4 cap."""
import ctypes as C

import numpy as np

import iao8_cases as IC
from iao8_cases import F, O
from bits_cases import _empty_i32, _host_u32

GUARD = 256          # poisoned bytes behind every output

# (id, x shape, O, KS, stride, relu, special, seed); a seed is moved on where make_case's draw leaves the four output pixels of the tie channel without an odd accumulator
CONVS = [
    ("k3s2_even", (2, 16, 8, 8), 32, 3, 2, 1, True, 6100),
    ("k3s2_odd_map", (2, 16, 7, 5), 48, 3, 2, 1, True, 6101),                 # 7 x 5 -> 4 x 3
    ("k3s2_one_pixel", (1, 32, 1, 1), 16, 3, 2, 1, False, 6102),              # output 1 x 1, every tap but the centre outside
    ("k3s2_two_by_two", (1, 32, 2, 2), 16, 3, 2, 1, False, 6103),             # output 1 x 1, the taps above and left outside
    ("k3s2_320_pixels", (5, 16, 16, 16), 16, 3, 2, 1, True, 6104),            # 320 output pixels: a block boundary inside an image, a partial last wave
    ("k1s2_no_relu", (2, 32, 6, 6), 64, 1, 2, 0, True, 6105),                 # negative codes must survive
    ("k1s1_no_relu_partial", (2, 24, 5, 5), 40, 1, 1, 0, True, 6106),         # C and O no multiple of 16
    ("k3s2_36_steps", (1, 256, 4, 4), 16, 3, 2, 1, True, 6110),
]
EXTREME = ("k3_extreme", (1, 512, 2, 2), 32)          # every code at qmin against +-127: |acc| = 128 * 127 * 512 * 4 (every pixel of a 2 x 2 map sees all four)

# (id, x shape, O, KS, options of make_add_case): seed 6200 + index; every one runs with one and with two output maps
ADDS = [
    ("a3_two_images", (2, 16, 6, 6), 32, 3, {}),
    ("a3_odd_map_80", (1, 64, 3, 5), 80, 3, {}),
    ("a3_320_pixels", (5, 16, 8, 8), 16, 3, {}),
    ("a1_64", (2, 32, 4, 4), 64, 1, {}),
    ("a3_ties", (2, 16, 6, 6), 32, 3, dict(tie=True)),                               # s_add a power of two, s_A = 2 s_add: every odd sum is an exact tie
    ("a3_w4a4", (2, 16, 6, 6), 32, 3, dict(widths=(4, 4))),
    ("a3_add8_consumer4", (2, 16, 6, 6), 32, 3, dict(out_bits=(4, 8))),              # an 8-bit add in front of a 4-bit consumer
    ("a1_per_layer", (2, 32, 4, 4), 64, 1, dict(per_channel=False)),
]

# (geometry keywords) mn_i8res_* refuses at widths 8
REFUSED = [
    dict(x_shape=(1, 32, 8, 8), w_shape=(32, 16, 3, 3), padding=1, groups=2),
    dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=2, dilation=2),
    dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1, stride=3),
    dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=1, stride=(2, 1)),
    dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2),
    dict(x_shape=(1, 24, 8, 8), w_shape=(32, 24, 3, 3), padding=1),
    dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 3, 3), padding=0),
]


def _lib():
    from micronet_amd import _lib as L
    return L


# ---------------------------------------------------------------------------------------------- the judge
def chain_y(acc, al, b):
    v = acc.astype(F)                                                   # int -> float, round to nearest even
    return ((v * al.reshape(1, -1, 1, 1).astype(F)).astype(F) + b.reshape(1, -1, 1, 1).astype(F)).astype(F)


def exact_acc(case, stride):
    acc = O.conv2d_fwd(case["j"].astype(np.int64), case["k"], None, stride=stride, padding=case["KS"] // 2, acc=np.int64)
    assert np.abs(acc).max() < 2 ** 31
    return acc


def judge_conv(case, stride, relu):
    y = chain_y(exact_acc(case, stride), case["al"], case["b"])
    r = np.where(y > 0, y, F(0)).astype(F) if relu else y
    return IC.code_of(r, case["s_out"], case["a_bits"]).astype(np.int8)


def judge_add(case, nout):
    """(c_r, sums c_r + c_s, [out_A, out_B][:nout]) of an add case."""
    s = F(case["s_add"])
    y = chain_y(exact_acc(case, 1), case["al"], case["b"])
    c_r = IC.code_of(y, s, case["add_bits"])
    fr, fs = (c_r * s).astype(F), (case["c_s"].astype(F) * s).astype(F)
    t = (fr + fs).astype(F)
    v = np.where(t > 0, t, F(0)).astype(F)
    outs = [IC.code_of(v, case["s_k"][k], case["bits_k"][k]).astype(np.int8) for k in range(nout)]
    return c_r.astype(np.int64), c_r.astype(np.int64) + case["c_s"].astype(np.int64), outs


def torch_conv(case, stride, relu):
    """The fp32 path on the CPU: F.conv2d of the fake-quantised values + bias -> [ReLU] -> the consumer's code."""
    import torch
    import torch.nn.functional as TF
    x = torch.from_numpy((case["j"].astype(F) * case["s_a"]).astype(F))
    y = TF.conv2d(x, torch.from_numpy(case["w"]), torch.from_numpy(case["b"]), stride=stride, padding=case["KS"] // 2)
    r = (torch.relu(y) if relu else y).numpy()
    return IC.code_of(r, case["s_out"], case["a_bits"]).astype(np.int8)


def torch_add(case, nout):
    """... F.conv2d -> Q(res) s + Q(sc) s (QuantAdd.forward on the two fake-quantised values) -> ReLU -> the consumers' codes."""
    import torch
    import torch.nn.functional as TF
    s = F(case["s_add"])
    x = torch.from_numpy((case["j"].astype(F) * case["s_a"]).astype(F))
    y = TF.conv2d(x, torch.from_numpy(case["w"]), torch.from_numpy(case["b"]), padding=case["KS"] // 2).numpy()
    res = torch.from_numpy((IC.code_of(y, s, case["add_bits"]) * s).astype(F))
    sc = torch.from_numpy((case["c_s"].astype(F) * s).astype(F))          # the shortcut is a code at s_add: its fake-quantised value
    v = torch.relu(res + sc).numpy()
    return [IC.code_of(v, case["s_k"][k], case["bits_k"][k]).astype(np.int8) for k in range(nout)]


# ---------------------------------------------------------------------------------------------- inputs
def make_conv_case(idx, special=None):
    name, x_shape, Oc, KS, stride, relu, sp, seed = CONVS[idx]
    case = IC.make_case(x_shape, Oc, KS, 1, seed, special=sp if special is None else special)
    assert np.array_equal(exact_acc(case, stride), case["acc"][:, :, ::stride, ::stride]), "a strided accumulator is the stride-1 one at the even pixels"
    if not sp:
        # one output pixel per channel: make_case's scales (from the accumulator's spread over pixels) would saturate every code, and its special channels need a
        # map.  Put the largest |y| of channels 3 .. at code 100; channel 1 gets a bias that keeps it negative (the ReLU zeroes it), channel 2 one that saturates
        # it -- both depend on the bias alone.  A tie channel needs an odd accumulator on the one pixel: not built for these two cases.
        qmax = float(IC.qrange(case["a_bits"])[1])
        ya = chain_y(exact_acc(case, stride), case["al"], np.zeros_like(case["b"]))
        y = chain_y(exact_acc(case, stride), case["al"], case["b"])
        case["s_out"] = case["s_p"] = F(np.abs(y[:, 3:]).max() / 100.0)
        case["b"] = case["b"].copy()
        case["b"][1] = F(-(float(np.abs(ya[:, 1]).max()) + float(case["s_out"])))
        case["b"][2] = F(float(np.abs(ya[:, 2]).max()) + (qmax + 2.0) * float(case["s_out"]))
    return case


def assert_conv_case_is_hard(case, stride, relu):
    """make_case's special channels, on the judge itself at this stride."""
    ref = judge_conv(case, stride, relu)
    qmin, qmax = (int(v) for v in IC.qrange(case["a_bits"]))
    assert len(np.unique(ref)) > min(32, ref.size // 4), "the case must produce many codes"
    assert case["tie"]
    a0 = exact_acc(case, stride)[:, 0]
    odd = (a0 > 0) & (a0 < 2 * qmax) & (a0 % 2 == 1)
    assert odd.any(), "odd accumulators in range on the tie channel"
    assert np.array_equal(ref[:, 0][odd], ((a0[odd] + 1) // 2).astype(np.int8)), "a tie rounds away from zero"
    assert (ref[:, 2] == qmax).all(), "a channel that saturates"
    if relu:
        assert (ref[:, 1] == 0).all(), "a channel the ReLU zeroes"
    else:
        assert (ref[:, 1] == qmin).all() and (ref < 0).mean() > 0.2, "without the ReLU negative codes survive"
        negodd = (a0 < 0) & (a0 > 2 * qmin) & (a0 % 2 == 1)
        assert negodd.any() and np.array_equal(ref[:, 0][negodd], ((a0[negodd] - 1) // 2).astype(np.int8)), "a negative tie rounds away from zero"


def make_add_case(x_shape, Oc, KS, seed, widths=(8, 8), per_channel=True, out_bits=None, tie=False, special=True):
    """An add stage on make_case's conv: the conv's output scale becomes s_add (tie: make_case's 2^-11, a power of two; else 0.93 of it, so that the saturating channel
    still saturates), the shortcut's codes cover the whole range of the add's width, and the two consumers quantise at 1.37 s_add and 2.21 s_add (tie: 2 s_add and
    s_add; a narrower consumer: 2^(add - bits) times that)."""
    base = IC.make_case(x_shape, Oc, KS, 1, seed, widths=widths, per_channel=per_channel, special=special)
    r = np.random.default_rng(seed + 77)
    add_bits = widths[1]
    bits_k = tuple(out_bits) if out_bits is not None else (add_bits, add_bits)
    s_add = F(base["s_out"]) if tie else F(base["s_out"] * F(0.93))
    if tie:
        assert base["tie"] and float(s_add) == 2.0 ** -11
    amin, amax = (int(v) for v in IC.qrange(add_bits))
    N, _, H, W = x_shape
    c_s = r.integers(amin, amax + 1, size=(N, Oc, H, W)).astype(np.int8)
    ratio = (2.0, 1.0) if tie else (1.37, 2.21)
    s_k = tuple(F(s_add * F(ratio[k]) * F(1 << (add_bits - bits_k[k]))) for k in range(2))
    return dict(base, s_add=s_add, add_bits=add_bits, c_s=c_s, s_k=s_k, bits_k=bits_k, is_tie=tie)


def assert_add_case_is_hard(case):
    """What the add stage's inputs must contain, on the judge's own data."""
    c_r, sums, (oa, ob) = judge_add(case, 2)
    amin, amax = (int(v) for v in IC.qrange(case["add_bits"]))
    assert (c_r == amax).any() and (c_r == amin).any(), "c_r saturated at both ends"
    assert (c_r == amax).mean() < 0.5 and (c_r == amin).mean() < 0.5 and len(np.unique(c_r)) > min(32, amax)
    assert (sums > amax).any() and (sums < amin).any(), "sums beyond either end of the code range"
    neg = sums < 0
    assert neg.mean() > 0.1 and (oa[neg] == 0).all() and (ob[neg] == 0).all(), "negative sums that the ReLU zeroes"
    assert (oa != ob).mean() >= 0.25, "the two consumers' maps differ on at least a quarter of the positions"
    if case["is_tie"]:
        qmax = int(IC.qrange(case["bits_k"][0])[1])
        odd = (sums > 0) & (sums < 2 * qmax) & (sums % 2 == 1)
        assert odd.mean() > 0.1 and np.array_equal(oa[odd], ((sums[odd] + 1) // 2).astype(np.int8)), "every odd sum is a tie and rounds away from zero"
        assert np.array_equal(ob, np.clip(sums, 0, int(IC.qrange(case["bits_k"][1])[1])).astype(np.int8)), "at s_B = s_add the code is the clamped sum"


# ---------------------------------------------------------------------------------------------- through the ABI
def geom_of(be, case, stride=1):
    return be.geom(case["j"].shape, case["w"].shape, stride=stride, padding=case["KS"] // 2)


def pack_table(be, g, case, in_bits, out_bits, s_out, **over):
    nb = int(be.lib.mn_i8res_table_bytes(C.byref(g), in_bits, out_bits, case["w_bits"]))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    dW, dS, dB = be.to_dev(over.get("w", case["w"])), be.to_dev(over.get("s_w", case["s_w"])), be.to_dev(over.get("b", case["b"]))
    be.call("mn_i8res_pack", C.byref(g), be.ptr(dW), be.ptr(dS), 1 if case["per_channel"] else 0, be.ptr(dB), C.c_float(float(over.get("s_a", case["s_a"]))),
            C.c_float(float(s_out)), in_bits, out_bits, case["w_bits"], be.ptr(table), be.stream)
    return table


def checked_table(be, g, case, in_bits, out_bits, s_out):
    table = pack_table(be, g, case, in_bits, out_bits, s_out)
    hdr = _host_u32(be, table)
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0, "finite constants, weights on the grid: %d %d" % (int(hdr[0]), int(hdr[7]))
    assert int(hdr[6]) == (out_bits | case["w_bits"] << 8)
    return table


def guarded(be, nbytes):
    return be.empty_i8((nbytes + GUARD,))          # poisoned


def split_guard(be, buf, shape):
    """(the output [N, OB, HW, 16], True iff the guard behind it still holds the poison)."""
    h = be.to_host(buf)
    n = int(np.prod(shape))
    return h[:n].reshape(shape), bool((h[n:] == 77).all()) and h.size == n + GUARD


def run_conv(be, case, stride, relu):
    """Pack, run mn_i8res_conv_fwd twice into poisoned, guarded buffers: (codes [N, OB * 16, Ho, Wo], kernel name)."""
    g = geom_of(be, case, stride)
    bits = case["a_bits"]
    assert be.lib.mn_i8res_supported(C.byref(g), bits, bits, case["w_bits"]) == 1
    table = checked_table(be, g, case, bits, bits, case["s_out"])
    xb = be.to_dev_i8(IC.np_block(case["j"]))
    N, _, H, W = case["j"].shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    OB = (case["w"].shape[0] + 15) // 16
    shape = (N, OB, Ho * Wo, 16)
    outs = []
    for _ in range(2):
        yb = guarded(be, int(np.prod(shape)))
        be.call("mn_i8res_conv_fwd", C.byref(g), bits, bits, case["w_bits"], be.ptr(table), be.ptr(xb), be.ptr(yb), int(relu), be.stream)
        got, whole = split_guard(be, yb, shape)
        assert whole, "nothing is written behind the output"
        outs.append(got)
    name = be.lib.mn_last_kernel().decode()
    assert np.array_equal(outs[0], outs[1]), "two runs give identical bytes"
    return IC.np_unblock(outs[0], OB * 16, Ho, Wo), name


def _check_conv(be, case, stride, relu, what):
    ref = judge_conv(case, stride, relu)
    got, name = run_conv(be, case, stride, relu)
    want = IC.expect_positions(ref, None, (ref.shape[1] + 15) // 16)
    bad = int((got != want).sum())
    print(name, what, "mismatches against the judge", bad, "of", got.size, "distinct codes", len(np.unique(ref)))
    assert name == "k_i8res_conv<%d,%d,%d>" % (case["KS"], stride, relu), name
    assert got.shape == want.shape and bad == 0, (bad, got.size)


def check_conv(be, idx):
    name, x_shape, Oc, KS, stride, relu, special, _ = CONVS[idx]
    case = make_conv_case(idx)
    if special:
        assert_conv_case_is_hard(case, stride, relu)
    else:
        ref = judge_conv(case, stride, relu)
        assert ref.shape[2:] == (1, 1) and len(np.unique(ref)) > 4
        assert relu and (ref[:, 1] == 0).all() and (exact_acc(case, stride)[:, 1] != 0).all(), "a channel the ReLU zeroes"
        assert (ref[:, 2] == int(IC.qrange(case["a_bits"])[1])).all(), "a channel that saturates"
    _check_conv(be, case, stride, relu, "%s %s -> %d k%d stride %d relu %d" % (name, x_shape, Oc, KS, stride, relu))


def check_conv_extreme(be):
    name, x_shape, Oc = EXTREME
    case = IC.make_case(x_shape, Oc, 3, 1, 6150, extreme=True)
    acc = exact_acc(case, 1)
    assert int(np.abs(acc).max()) == 128 * 127 * 512 * 4 and int(acc.min()) == -128 * 127 * 512 * 4
    for relu in (1, 0):
        assert len(np.unique(judge_conv(case, 1, relu))) >= 2
        _check_conv(be, case, 1, relu, name)


def add_params(case, nout, **over):
    q = _lib().I8ResAdd()
    q.s_add, q.add_bits, q.nout = float(over.get("s_add", case["s_add"])), int(over.get("add_bits", case["add_bits"])), nout
    q.s_out0, q.bits0 = float(over.get("s0", case["s_k"][0])), int(over.get("bits0", case["bits_k"][0]))
    q.s_out1, q.bits1 = float(over.get("s1", case["s_k"][1])), int(over.get("bits1", case["bits_k"][1]))
    return q


def run_add(be, case, nout):
    """Pack (s_out = s_add at the add's width), run mn_i8res_add_fwd twice into poisoned, guarded buffers: ([codes [N, OB * 16, H, W]] per output map, kernel name)."""
    g = geom_of(be, case)
    in_bits = case["a_bits"]
    assert be.lib.mn_i8res_supported(C.byref(g), in_bits, case["add_bits"], case["w_bits"]) == 1
    table = checked_table(be, g, case, in_bits, case["add_bits"], case["s_add"])
    xb, sb = be.to_dev_i8(IC.np_block(case["j"])), be.to_dev_i8(IC.np_block(case["c_s"]))
    N, _, H, W = case["j"].shape
    OB = (case["w"].shape[0] + 15) // 16
    shape = (N, OB, H * W, 16)
    q = add_params(case, nout)
    runs = []
    for _ in range(2):
        ys = [guarded(be, int(np.prod(shape))) for _ in range(nout)]
        be.call("mn_i8res_add_fwd", C.byref(g), in_bits, case["w_bits"], be.ptr(table), be.ptr(xb), be.ptr(sb), C.byref(q), be.ptr(ys[0]),
                be.ptr(ys[1]) if nout == 2 else None, be.stream)
        got = [split_guard(be, y, shape) for y in ys]
        assert all(whole for _, whole in got), "nothing is written behind an output"
        runs.append([a for a, _ in got])
    name = be.lib.mn_last_kernel().decode()
    assert all(np.array_equal(a, b) for a, b in zip(*runs)), "two runs give identical bytes"
    assert np.array_equal(be.to_host(sb), IC.np_block(case["c_s"])), "the shortcut is only read"
    return [IC.np_unblock(a, OB * 16, H, W) for a in runs[0]], name


def check_add(be, idx, nout):
    name, x_shape, Oc, KS, opts = ADDS[idx]
    case = make_add_case(x_shape, Oc, KS, 6200 + idx, **opts)
    assert_add_case_is_hard(case)
    _, _, refs = judge_add(case, nout)
    gots, kname = run_add(be, case, nout)
    assert kname == "k_i8res_add<%d,%d>" % (KS, nout), kname
    for k, (got, ref) in enumerate(zip(gots, refs)):
        want = IC.expect_positions(ref, None, (Oc + 15) // 16)
        bad = int((got != want).sum())
        print(kname, name, x_shape, "->", Oc, "map", k, "mismatches against the judge", bad, "of", got.size, "distinct codes", len(np.unique(ref)))
        assert got.shape == want.shape and bad == 0, (k, bad, got.size)


def _within_cap(what, ref, par):
    d = np.abs(ref.astype(np.int32) - par.astype(np.int32))
    print(what, "flips against the fp32 path", int((d != 0).sum()), "of", d.size, "largest", int(d.max()))
    assert d.max() <= 1 and (d != 0).mean() <= 1e-4


def check_conv_vs_torch(idx):
    """The cap of the GPU cross-check holds for the judge itself: against the fp32 arithmetic at most one step, on at most 1e-4 of the elements."""
    name, _, _, _, stride, relu, _, _ = CONVS[idx]
    case = make_conv_case(idx, special=False)
    _within_cap(name, judge_conv(case, stride, relu), torch_conv(case, stride, relu))


def check_extreme_geometry_vs_torch():
    """... at the geometry of EXTREME, on ordinary inputs (with every code at qmin against +-127 the fp32 path's sums are not the point of the case)."""
    name, x_shape, Oc = EXTREME
    case = IC.make_case(x_shape, Oc, 3, 1, 6151, special=False)
    for relu in (1, 0):
        _within_cap("%s relu %d" % (name, relu), judge_conv(case, 1, relu), torch_conv(case, 1, relu))


def check_add_vs_torch(idx):
    name, x_shape, Oc, KS, opts = ADDS[idx]
    case = make_add_case(x_shape, Oc, KS, 6200 + idx, special=False, **dict(opts, tie=False))
    for k, (ref, par) in enumerate(zip(judge_add(case, 2)[2], torch_add(case, 2))):
        _within_cap("%s map %d" % (name, k), ref, par)


# ---------------------------------------------------------------------------------------------- refusals, invalid arguments, counters
def _small_add(be):
    """A 1x1 add stage 16 -> 16 on a 4 x 4 map (every tensor 256 bytes) with poisoned outputs: (g, case, table, x, shortcut, out_a, out_b)."""
    case = make_add_case((1, 16, 4, 4), 16, 1, 6300, special=False)
    g = geom_of(be, case)
    table = checked_table(be, g, case, 8, 8, case["s_add"])
    return g, case, table, be.to_dev_i8(IC.np_block(case["j"])), be.to_dev_i8(IC.np_block(case["c_s"])), _empty_i32(be, (64,)), _empty_i32(be, (64,))


def check_refused(be, idx):
    kw = REFUSED[idx]
    g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), dilation=kw.get("dilation", 1), groups=kw.get("groups", 1))
    buf, other = _empty_i32(be, (64,)), _empty_i32(be, (64,))
    f = be.to_dev(np.ones(64, dtype=F))
    one = C.c_float(1.0)
    ENOTSUP = _lib().MN_ENOTSUP
    q = add_params(dict(s_add=1.0, add_bits=8, s_k=(1.0, 1.0), bits_k=(8, 8)), 1)
    assert be.lib.mn_i8res_supported(C.byref(g), 8, 8, 8) == 0
    assert int(be.lib.mn_i8res_table_bytes(C.byref(g), 8, 8, 8)) == 0
    assert be.lib.mn_i8res_pack(C.byref(g), be.ptr(f), be.ptr(f), 1, be.ptr(f), one, one, 8, 8, 8, be.ptr(buf), be.stream) == ENOTSUP
    for relu in (0, 1):
        assert be.lib.mn_i8res_conv_fwd(C.byref(g), 8, 8, 8, be.ptr(buf), be.ptr(buf), be.ptr(other), relu, be.stream) == ENOTSUP
    assert be.lib.mn_i8res_add_fwd(C.byref(g), 8, 8, be.ptr(buf), be.ptr(buf), be.ptr(buf), C.byref(q), be.ptr(other), None, be.stream) == ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all() and (_host_u32(be, other) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_widths_refused(be):
    g = be.geom((1, 32, 8, 8), (32, 32, 1, 1))
    for bits in ((1, 8, 8), (9, 8, 8), (8, 1, 8), (8, 9, 8), (8, 8, 1), (8, 8, 9)):
        assert be.lib.mn_i8res_supported(C.byref(g), *bits) == 0 and int(be.lib.mn_i8res_table_bytes(C.byref(g), *bits)) == 0
    assert be.lib.mn_i8res_supported(C.byref(g), 8, 4, 8) == 1


def check_add_stride2_refused(be):
    """The conv stage takes the geometry, the add stage refuses it: the residual and the shortcut share one map."""
    g2 = be.geom((1, 16, 4, 4), (16, 16, 1, 1), stride=2)
    assert be.lib.mn_i8res_supported(C.byref(g2), 8, 8, 8) == 1
    g, case, table, x, sc, oa, ob = _small_add(be)
    q = add_params(case, 2)
    assert be.lib.mn_i8res_add_fwd(C.byref(g2), 8, 8, be.ptr(table), be.ptr(x), be.ptr(sc), C.byref(q), be.ptr(oa), be.ptr(ob), be.stream) == _lib().MN_ENOTSUP
    assert (_host_u32(be, oa) == 0x5a5a5a5a).all() and (_host_u32(be, ob) == 0x5a5a5a5a).all()


def check_invalid(be):
    """A null or misaligned tensor, an output that aliases the shortcut (or the input, or the other output), and a scale or width of the add stage that is not valid
    are MN_EINVAL and write nothing; the same call with valid arguments then runs."""
    L = _lib()
    g, case, table, x, sc, oa, ob = _small_add(be)
    lib, s = be.lib, be.stream
    p = be.ptr
    odd = lambda b: C.c_void_p(p(b).value + 4)
    q1, q2 = add_params(case, 1), add_params(case, 2)
    add = lambda q, *a: lib.mn_i8res_add_fwd(C.byref(g), 8, 8, a[0], a[1], a[2], C.byref(q) if q is not None else None, a[3], a[4], s)
    ok = (p(table), p(x), p(sc), p(oa), p(ob))
    swap = lambda i, v: tuple(v if k == i else a for k, a in enumerate(ok))
    assert add(q2, *swap(2, None)) == L.MN_EINVAL, "a null shortcut"
    assert add(q2, *swap(0, None)) == L.MN_EINVAL and add(q2, *swap(1, None)) == L.MN_EINVAL and add(q2, *swap(3, None)) == L.MN_EINVAL
    assert add(None, *ok) == L.MN_EINVAL
    assert add(q2, *swap(4, None)) == L.MN_EINVAL and add(q1, *ok) == L.MN_EINVAL, "nout and out_b must agree"
    assert add(q2, *swap(3, p(sc))) == L.MN_EINVAL and add(q2, *swap(4, p(sc))) == L.MN_EINVAL, "an output aliasing the shortcut"
    assert add(q2, *swap(3, p(x))) == L.MN_EINVAL and add(q2, *swap(4, p(oa))) == L.MN_EINVAL, "... the input, the other output"
    for i in range(5):
        assert add(q2, *swap(i, odd((table, x, sc, oa, ob)[i]))) == L.MN_EINVAL, "a misaligned pointer"
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert add(add_params(case, 2, s_add=bad), *ok) == L.MN_EINVAL
        assert add(add_params(case, 2, s0=bad), *ok) == L.MN_EINVAL
        assert add(add_params(case, 2, s1=bad), *ok) == L.MN_EINVAL
    for bad in (1, 9):
        assert add(add_params(case, 2, add_bits=bad), *ok) == L.MN_EINVAL
        assert add(add_params(case, 2, bits0=bad), *ok) == L.MN_EINVAL
        assert add(add_params(case, 2, bits1=bad), *ok) == L.MN_EINVAL
    q3 = add_params(case, 2)
    q3.nout = 3
    assert add(q3, *ok) == L.MN_EINVAL
    # the conv stage and the packer
    conv = lambda *a: lib.mn_i8res_conv_fwd(C.byref(g), 8, 8, 8, a[0], a[1], a[2], a[3], s)
    assert conv(None, p(x), p(oa), 1) == L.MN_EINVAL and conv(p(table), None, p(oa), 1) == L.MN_EINVAL and conv(p(table), p(x), None, 1) == L.MN_EINVAL
    assert conv(odd(table), p(x), p(oa), 1) == L.MN_EINVAL and conv(p(table), odd(x), p(oa), 1) == L.MN_EINVAL and conv(p(table), p(x), odd(oa), 1) == L.MN_EINVAL
    assert conv(p(table), p(x), p(x), 1) == L.MN_EINVAL, "an output aliasing the input"
    assert conv(p(table), p(x), p(oa), 2) == L.MN_EINVAL
    g0 = be.geom((0, 16, 4, 4), (16, 16, 1, 1))
    assert lib.mn_i8res_supported(C.byref(g0), 8, 8, 8) == 0
    assert lib.mn_i8res_conv_fwd(C.byref(g0), 8, 8, 8, p(table), p(x), p(oa), 1, s) == L.MN_EINVAL
    f = be.to_dev(np.ones(256, dtype=F))
    one = C.c_float(1.0)
    pk = lambda *a: lib.mn_i8res_pack(C.byref(g), a[0], a[1], a[2], p(f), one, one, 8, 8, 8, a[3], s)
    assert pk(None, p(f), 1, p(oa)) == L.MN_EINVAL and pk(p(f), None, 1, p(oa)) == L.MN_EINVAL and pk(p(f), p(f), 1, None) == L.MN_EINVAL
    assert pk(p(f), p(f), 1, odd(oa)) == L.MN_EINVAL and pk(p(f), p(f), 2, p(oa)) == L.MN_EINVAL
    assert (_host_u32(be, oa) == 0x5a5a5a5a).all() and (_host_u32(be, ob) == 0x5a5a5a5a).all() and (be.to_host(f) == 1).all(), "nothing was written"
    assert np.array_equal(be.to_host(sc), IC.np_block(case["c_s"])) and np.array_equal(be.to_host(x), IC.np_block(case["j"]))
    assert add(q2, *ok) == L.MN_OK
    _, _, refs = judge_add(case, 2)
    for buf, ref in zip((oa, ob), refs):
        assert np.array_equal(IC.np_unblock(be.to_host(buf).view(np.int8).reshape(1, 1, 16, 16), 16, 4, 4), ref)


def check_counters(be):
    """Both table counters of mn_i8res_pack: word 0 a NaN bias and a scale that is not finite and positive, word 7 a weight off the grid or beyond 2^(w-1) - 1."""
    case = make_conv_case(0)
    g = geom_of(be, case, 2)
    hdr = _host_u32(be, pack_table(be, g, case, 8, 8, case["s_out"]))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0
    assert (int(hdr[1]), int(hdr[4]), int(hdr[5])) == (3, 1, 1) and int(hdr[6]) == (8 | 8 << 8)          # 9 slots of 16 channels: three k-steps
    assert hdr[8:13].view(F).tolist() == [case["s_out"], case["s_out"], F(-128), F(127), case["s_a"]]
    assert int(_host_u32(be, pack_table(be, g, case, 8, 4, case["s_out"]))[6]) == (4 | 8 << 8)
    assert _host_u32(be, pack_table(be, g, case, 8, 4, case["s_out"]))[10:12].view(F).tolist() == [F(-8), F(7)]
    b = case["b"].copy()
    b[9] = F(np.nan)
    hdr = _host_u32(be, pack_table(be, g, case, 8, 8, case["s_out"], b=b))
    assert int(hdr[0]) == 1 and int(hdr[7]) == 0
    for s_out in (np.inf, 0.0, -1.0):
        hdr = _host_u32(be, pack_table(be, g, case, 8, 8, s_out))
        assert int(hdr[0]) >= 1 and int(hdr[7]) == 0, s_out
    assert int(_host_u32(be, pack_table(be, g, case, 8, 8, case["s_out"], s_a=np.inf))[0]) >= 1
    sw = case["s_w"].copy()
    sw[4] = F(np.inf)
    assert int(_host_u32(be, pack_table(be, g, case, 8, 8, case["s_out"], s_w=sw))[0]) >= 1
    w2 = case["w"].copy()
    w2[5, 3, 0, 0] += F(0.5) * case["s_w"][5]
    hdr = _host_u32(be, pack_table(be, g, case, 8, 8, case["s_out"], w=w2))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 1
    w3 = case["w"].copy()
    w3[6, 1, 0, 0] = F(128) * case["s_w"][6]                             # on the grid, beyond 2^(w-1) - 1
    assert int(_host_u32(be, pack_table(be, g, case, 8, 8, case["s_out"], w=w3))[7]) == 1
