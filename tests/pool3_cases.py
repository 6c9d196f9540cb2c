"""max_pool2d(3, 2, 1) forward and backward (csrc/pool3s2.h) through the C ABI: one case table for the CPU emulation build and the GPU.  Three forms: fp32
(mn_maxpool3x3s2_f32_*), int8 sign codes (mn_maxpool3x3s2_sign8_*), fused with the IAO activation quantizer (mn_iao_fq_maxpool3x3s2_*).

The judge is torch.nn.functional.max_pool2d on the CPU in float64 with autograd -- on x, on the +-1 codes, or on the oracle's fake-quant of x (np_oracle.iao_fq_fwd), its
gradient then masked by the oracle's clip-STE (np_oracle.iao_fq_bwd of ones).  Selection is exact and gy holds integers |g| <= 8, so a sum of at most four of them is exact
in fp32: y and dx must equal the judge bit for bit (NaNs as NaNs), no tolerance.  The quantizers use power-of-two scales, for which the kernel's (g * s) / s is g."""
import ctypes as C

import numpy as np
import torch

from oracle import np_oracle as O

F = np.float32
TILE = 4096          # P3_TILE of csrc/pool3s2.h: the largest plane staged whole; beyond it bands of (TILE / W - 3) / 2 output rows
SHAPES = [(6, 8, 8), (5, 7, 9), (3, 1, 3), (2, 5, 1), (7, 16, 12), (2, 65, 64)]          # (2, 65, 64): 4160 > TILE -> bands of 30 + 3 output rows, H odd
assert 65 * 64 > TILE and (TILE // 64 - 3) // 2 == 30
KINDS = {"f32": ["ties", "neg", "nan"], "sign": ["allneg", "pm1"], "fq": ["ties", "neg", "wide"]}
QUANTS = [(8, 0), (2, 0), (2, 1), (8, 1)]          # (bits, q_type) of the fused form
# (form, shape, kind, (bits, q_type), offset): every shape x kind [x quantizer on two shapes]; offset 1 = every float / code tensor starts 4 bytes behind a 16-byte boundary
CASES = [(f, s, k, QUANTS[0], 0) for f in KINDS for s in SHAPES for k in KINDS[f]]
CASES += [("fq", s, "wide", q, 0) for q in QUANTS[1:] for s in (SHAPES[1], SHAPES[5])]
CASES += [(f, s, KINDS[f][-1], QUANTS[0], 1) for f in KINDS for s in (SHAPES[1], SHAPES[4])]
IDS = ["%s-%dx%dx%d-%s-b%dq%d-off%d" % ((f,) + s + (k,) + q + (o,)) for f, s, k, q, o in CASES]


def make_x(shape, kind, seed):
    r = np.random.default_rng(seed)
    if kind in ("ties", "nan"):
        x = r.choice(np.array([0, 0, 0, 1, 2], dtype=F), size=shape)          # ReLU-like: most windows hold several maxima
        if kind == "nan":
            x.reshape(-1)[r.choice(x.size, size=max(2, x.size // 16), replace=False)] = np.nan
        return x
    if kind == "neg":
        return -r.integers(1, 6, size=shape).astype(F)          # a padded cell counted as 0 would win every border window
    if kind == "wide":
        return r.integers(-3, 4, size=shape).astype(F)
    return np.full(shape, -1, F) if kind == "allneg" else r.choice(np.array([-1, 1], dtype=F), size=shape)


def quantizer(bits, q_type):
    """(scale, zp, min_val, max_val, qp row): range [-2, ~2) on a power-of-two scale, so x = -3 and x = 3 clip on either side (clamp and clip-STE)."""
    sc = F(1.0 if bits == 2 else 1.0 / 64)
    qmin, qmax = O.iao_qrange(bits, q_type, True)
    zp = F(0 if q_type == 0 else -2 / sc)
    mn, mx = F(-2), F((qmax + zp) * sc)
    lo, hi = mn / sc - zp, mx / sc - zp
    if q_type == 0:
        hi = max(abs(lo), abs(hi)); lo = -hi
    return sc, zp, mn, mx, np.array([sc, zp, lo, hi], dtype=F)


def judge(xq, gy, mask=None):
    """(y, dx) as fp32 of max_pool2d(xq, 3, 2, 1) in float64 on the CPU for [N, C, H, W] arrays; dx only where mask != 0."""
    t = torch.tensor(xq.astype(np.float64), requires_grad=True)
    ty = torch.nn.functional.max_pool2d(t, 3, 2, 1)
    ty.backward(torch.tensor(gy.astype(np.float64)))
    dx = t.grad.numpy().astype(F)
    return ty.detach().numpy().astype(F), dx if mask is None else np.where(mask != 0, dx, F(0))


def same_bits(got, want):
    return bool((((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))).all())


class Buf:
    """A device buffer whose payload starts `off` 4-byte elements behind the allocation's (16-byte aligned) base."""

    def __init__(self, be, arr, off, dtype=F):
        arr = np.asarray(arr, dtype=dtype)
        self.be, self.shape, self.pad = be, arr.shape, off * 4 // arr.itemsize
        flat = np.concatenate([np.zeros(self.pad, dtype), arr.reshape(-1)])
        self.dev = {np.dtype(F): be.to_dev, np.dtype(np.int8): be.to_dev_i8, np.dtype(np.uint8): be.to_dev_u8}[np.dtype(dtype)](flat)
        self.ptr = C.c_void_p(be.ptr(self.dev).value + 4 * off)
        assert be.ptr(self.dev).value % 16 == 0

    def host(self):
        return self.be.to_host(self.dev)[self.pad:].reshape(self.shape)


def check(be, form, shape, kind, quant, off):
    P, H, W = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    bits, q_type = quant
    x = make_x(shape, kind, 9300 + H * W)
    gy = np.random.default_rng(9400 + H * W).integers(-8, 9, size=(P, Ho, Wo)).astype(F)
    xq, mask = x, None
    if form == "fq":
        sc, zp, mn, mx, qp = quantizer(bits, q_type)
        xq = O.iao_fq_fwd(x, sc, zp, bits, q_type, True)[0]
        mask = O.iao_fq_bwd(np.ones_like(x), x, sc, zp, mn, mx, bits, q_type, True)
        assert set(np.unique(mask)) <= {0.0, 1.0}
        if kind == "wide":
            assert (mask[x > 0] == 0).any() and (mask[x < 0] == 0).any() and (mask == 1).any(), "cells clip on each side"
    want_y, want_dx = (a[0] for a in judge(xq[None], gy[None], None if mask is None else mask[None]))
    assert want_y.shape == (P, Ho, Wo)

    dG, dDx = Buf(be, gy, off), Buf(be, np.full(shape, -1234.5, F), off)
    if form == "sign":
        assert be.lib.mn_maxpool3x3s2_sign8_supported(H, W) == 1
        dA, dOut = Buf(be, x, off, np.int8), Buf(be, np.full((P, Ho, Wo), 77), off, np.int8)
        be.call("mn_maxpool3x3s2_sign8_fwd", dA.ptr, P, H, W, dOut.ptr, be.stream)
        got_y = dOut.host().astype(F)
        be.call("mn_maxpool3x3s2_sign8_bwd", dG.ptr, dA.ptr, P, H, W, dDx.ptr, be.stream)
    else:
        dX, dY, dI = Buf(be, x, off), Buf(be, np.full((P, Ho, Wo), -1234.5, F), off), Buf(be, np.full((P, Ho, Wo), 0xEE), 0, np.uint8)
        if form == "f32":
            assert be.lib.mn_maxpool3x3s2_f32_supported(H, W) == 1
            be.call("mn_maxpool3x3s2_f32_fwd", dX.ptr, P, H, W, dY.ptr, dI.ptr, be.stream)
            be.call("mn_maxpool3x3s2_f32_bwd", dG.ptr, dI.ptr, P, H, W, dDx.ptr, be.stream)
        else:
            count = int(be.lib.mn_iao_fq_maxpool3x3s2_mm_count(P, H, W))
            dQ, dM = Buf(be, qp, 0), Buf(be, np.zeros(2 * count, F), 0)
            be.call("mn_iao_fq_maxpool3x3s2_fwd", dX.ptr, P, H, W, dQ.ptr, bits, q_type, dY.ptr, dI.ptr, dM.ptr, be.stream)
            be.call("mn_iao_fq_maxpool3x3s2_bwd", dG.ptr, dI.ptr, dX.ptr, P, H, W, dQ.ptr, bits, q_type, 0, dDx.ptr, be.stream)
            mm = dM.host()
            assert count >= 1 and mm[:count].min() == want_y.min() and mm[count:].max() == want_y.max(), "the partials' extrema are those of y"
            if kind == "wide":          # ... and with the mask of the ReLU in front
                dDr = Buf(be, np.full(shape, -1234.5, F), off)
                be.call("mn_iao_fq_maxpool3x3s2_bwd", dG.ptr, dI.ptr, dX.ptr, P, H, W, dQ.ptr, bits, q_type, 1, dDr.ptr, be.stream)
                assert same_bits(dDr.host(), np.where(x > 0, want_dx, F(0))), "dx behind a ReLU"
        got_y = dY.host()
    got_dx = dDx.host()
    print(form, shape, kind, quant, off, "y differs at", int((got_y.view(np.uint32) != want_y.view(np.uint32)).sum()), "of", want_y.size,
          "| dx differs at", int((got_dx.view(np.uint32) != want_dx.view(np.uint32)).sum()), "of", want_dx.size)
    assert same_bits(got_y, want_y), "y"
    assert same_bits(got_dx, want_dx), "dx"
