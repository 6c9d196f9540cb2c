"""The fused k-bit block through the 3x3 / stride 2 / padding 1 max-pool (mn_qa_* with pool = 2, csrc/qact_pool3.h) through the C ABI: one case table for the CPU
emulation build and the GPU.

The judge uses nothing of the code under test.  Forward: mn_qa_fwd(pool = 0) gives the un-pooled codes and fp32 a; torch's max_pool2d(., 3, 2, 1) of each in float64
on the CPU is what pool = 2 must give BIT FOR BIT (the quantizer is non-decreasing: the max of the codes is the code of the max).  Backward: routing from float64
max_pool2d autograd on that a (ATen's CPU rule: the first maximum), masks from the same fp32 a, the clip-STE, sums, dgamma, dbeta and dy in float64 from the stash and
chan; <= 1e-5 of max |reference| per tensor (the project's figure for this chain, check_qconv_bnq).  mn_qa_bwd == mn_qa_bwd_sums + mn_qa_bwd_apply bit for bit."""
import numpy as np
import torch

F = np.float32
# shape (N, C, H, W): one output row, every window clipped at the top | a tile wants 64 planes and gets 2 | 16 planes per tile, last tile partial | several tiles per
# block | one plane per tile | 3 tiles of one channel: the channel is split over 3 blocks (splits = min(2048 / C, tiles, 32))
SHAPES = [(3, 5, 2, 8), (2, 3, 8, 8), (5, 2, 16, 16), (9, 2, 32, 32), (2, 2, 64, 64), (130, 1, 8, 8)]
# (shape, in_kind 0 int16 stash / 1 fp32 y / 2 int32 stash, out bits (2: the integer-threshold forward on a stash), quant, training)
MIX = [(1, 2, 0, 1), (2, 8, 1, 0), (0, 2, 1, 0), (1, 8, 1, 1), (2, 4, 0, 1), (0, 8, 0, 0)]
CASES = [(s, 0, 4, 1, 1) for s in SHAPES] + [(s,) + m for s, m in zip(SHAPES, MIX)]
CASES += [(SHAPES[2], 0, 2, 0, 1), (SHAPES[3], 2, 2, 1, 1), (SHAPES[1], 1, 4, 1, 0), (SHAPES[4], 0, 2, 1, 1), (SHAPES[0], 2, 4, 1, 1), (SHAPES[5], 0, 2, 1, 1),
          (SHAPES[3], 1, 4, 1, 1), (SHAPES[2], 2, 8, 1, 1)]
IDS = ["%dx%dx%dx%d-in%d-b%d-q%d-t%d" % (s + (k, b, q, t)) for s, k, b, q, t in CASES]


def make_inputs(be, shape, kind, seed):
    """(device input, v float64 [N, C, H, W], chan [9, C]): z = ((v alpha + bias - mean) invstd) gamma + beta covers z < 0, (0, 10] and > 10 in every plane; gamma < 0
    on odd channels (the chain decreases: flip = -1 on the threshold path); few distinct values and the ReLU's zeros give many exact ties."""
    N, Cc, H, W = shape
    r = np.random.default_rng(seed)
    vi = r.integers(-20, 21, size=shape)
    far = r.random(shape) < 0.05          # (|v| = 40 takes z beyond 10: rare, or the clamp would mask most windows' winners)
    vi[far] = r.choice([-40, 40], size=int(far.sum()))
    vi[:, :, 0, :3] = (-40, 0, 40)
    c = np.arange(Cc)
    alpha, bias = (np.full(Cc, 1.0, F), np.zeros(Cc, F)) if kind == 1 else (np.full(Cc, 0.5, F), (0.25 * c).astype(F))
    mean, invstd, gamma, beta = np.full(Cc, 1.0, F), np.full(Cc, 0.8, F), ((0.9 + 0.05 * c) * (1 - 2 * (c % 2))).astype(F), np.full(Cc, 2.0, F)
    chan = np.stack([alpha, bias, mean, invstd, gamma, beta, alpha * invstd, (bias - mean) * invstd, gamma * invstd]).astype(F)
    if kind == 1:
        v = (vi * 0.5).astype(F)
        dev = be.to_dev(v)
    elif kind == 2:
        v, dev = vi, be.to_dev(vi.astype(np.int32).view(F))
    else:
        v, dev = vi, be.to_dev_i16(vi)
    return dev, v.astype(np.float64), chan


def check(be, shape, kind, bits, quant, training):
    N, Cc, H, W = shape
    Ho, Wo = H // 2, W // 2
    assert be.lib.mn_qa_supported(H, W, 2) == 1
    dIn, v, chan = make_inputs(be, shape, kind, 7100 + H * W + kind)
    dCh = be.to_dev(chan)
    s = F(1.0 / (2 ** bits - 1))
    # ---- the parent's un-pooled kernel, then float64 max_pool2d on the CPU
    c0, a0 = be.empty_i8(shape), be.empty(shape)
    be.call("mn_qa_fwd", kind, be.ptr(dIn), be.ptr(dCh), N, Cc, H, W, bits, 0, be.ptr(c0), be.ptr(a0), be.stream)
    a0 = be.to_host(a0)
    ta = torch.tensor(a0.astype(np.float64), requires_grad=True)
    tp = torch.nn.functional.max_pool2d(ta, 3, 2, 1)
    want_a = tp.detach().numpy().astype(F)
    want_c = torch.nn.functional.max_pool2d(torch.tensor(be.to_host(c0).view(np.uint8).astype(np.float64)), 3, 2, 1).numpy().astype(np.uint8)
    ch = chan.astype(np.float64).reshape(9, 1, Cc, 1, 1)
    zh = (v * ch[0] + ch[1] - ch[2]) * ch[3]
    for p in (zh * ch[4] + ch[5]).reshape(N * Cc, -1):
        assert (p < 0).any() and ((p > 0) & (p <= 10)).any() and (p > 10).any(), "both masks act on both sides in every plane"
    c2, a2 = be.empty_i8((N, Cc, Ho, Wo)), be.empty((N, Cc, Ho, Wo))
    be.call("mn_qa_fwd", kind, be.ptr(dIn), be.ptr(dCh), N, Cc, H, W, bits, 2, be.ptr(c2), be.ptr(a2), be.stream)
    got_c, got_a = be.to_host(c2).view(np.uint8), be.to_host(a2)
    print(shape, kind, bits, "codes differ at", int((got_c != want_c).sum()), "| act differs at", int((got_a.view(np.uint32) != want_a.view(np.uint32)).sum()), "of", want_a.size)
    assert np.array_equal(got_c, want_c), "codes"
    assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32)), "act_f32"
    # ---- backward in float64
    dq = np.random.default_rng(7200 + H * W).integers(-8, 9, size=(N, Cc, Ho, Wo)).astype(F)
    d = (dq.astype(np.float64) * float(s)) / float(s) * 0.1 if quant else dq.astype(np.float64)
    tp.backward(torch.tensor(d))
    keep = (a0 > 0) & ((a0 * F(0.1) <= 1) if quant else True)
    dz = np.where(keep, ta.grad.numpy(), 0.0)
    t1, t2 = dz.sum(axis=(0, 2, 3)), (dz * zh).sum(axis=(0, 2, 3))
    n = N * H * W
    want_dy = ch[8] * (dz - t1.reshape(1, -1, 1, 1) / n - zh * t2.reshape(1, -1, 1, 1) / n) if training else ch[8] * dz
    assert (dz != 0).any() and (not quant or (ta.grad.numpy()[~keep] != 0).any()), "gradient passes, and the clamp mask removes routed gradient"
    dDQ, ws = be.to_dev(dq), be.empty(int(be.lib.mn_qa_ws_floats(Cc)))
    outs = []
    for fused in (0, 1):
        dy, dgam, dbet, sums = be.empty(shape), be.empty(Cc), be.empty(Cc), be.empty((2, Cc))
        if fused:
            be.call("mn_qa_bwd", kind, be.ptr(dIn), be.ptr(dCh), be.ptr(dDQ), N, Cc, H, W, bits, 2, quant, training, be.ptr(dgam), be.ptr(dbet), be.ptr(sums), be.ptr(dy),
                    be.ptr(ws), be.stream)
        else:
            be.call("mn_qa_bwd_sums", kind, be.ptr(dIn), be.ptr(dCh), be.ptr(dDQ), N, Cc, H, W, bits, 2, quant, be.ptr(dgam), be.ptr(dbet), be.ptr(sums), be.ptr(ws), be.stream)
            be.call("mn_qa_bwd_apply", kind, be.ptr(dIn), be.ptr(dCh), be.ptr(sums), be.ptr(dDQ), N, Cc, H, W, bits, 2, quant, training, be.ptr(dy), be.stream)
        outs.append([be.to_host(t) for t in (dy, dgam, dbet, sums)])
    for (name, want), got in zip((("dy", want_dy), ("dgamma", t2), ("dbeta", t1), ("sums", np.stack([t1, t2]))), outs[0]):
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(" ", name, "rel err", err)
        assert err <= 1e-5, (name, err)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(*outs)), "mn_qa_bwd != mn_qa_bwd_sums + mn_qa_bwd_apply"


def check_refused(be):
    """66 x 64 = 4224 elements: beyond one tile.  Also an unknown pool value."""
    N, Cc, H, W = 1, 1, 66, 64
    assert be.lib.mn_qa_supported(H, W, 2) == 0 and be.lib.mn_qa_supported(H, W, 1) == 1 and be.lib.mn_qa_supported(8, 8, 3) == 0
    x, chan, dq = be.to_dev_i16(np.zeros((N, Cc, H, W))), be.to_dev(np.ones((9, Cc), F)), be.to_dev(np.zeros((N, Cc, H // 2, W // 2), F))
    codes, dy, v, ws = be.empty_i8((N, Cc, H, W)), be.empty((N, Cc, H, W)), be.empty((2, Cc)), be.empty(int(be.lib.mn_qa_ws_floats(Cc)))
    lib, p, st = be.lib, be.ptr, be.stream
    assert lib.mn_qa_fwd(0, p(x), p(chan), N, Cc, H, W, 4, 2, p(codes), None, st) != 0
    assert lib.mn_qa_bwd_sums(0, p(x), p(chan), p(dq), N, Cc, H, W, 4, 2, 1, None, None, p(v), p(ws), st) != 0
    assert lib.mn_qa_bwd_apply(0, p(x), p(chan), p(v), p(dq), N, Cc, H, W, 4, 2, 1, 1, p(dy), st) != 0
    assert lib.mn_qa_bwd(0, p(x), p(chan), p(dq), N, Cc, H, W, 4, 2, 1, 1, None, None, p(v), p(dy), p(ws), st) != 0
    assert lib.mn_qa_fwd(0, p(x), p(chan), N, Cc, 8, 8, 4, 3, p(codes), None, st) != 0
