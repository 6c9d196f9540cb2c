"""The 3x3 / stride-2 / padding-1 max-pool kernels (csrc/pool3s2.h) against the stock path they replace, on the two pooled maps of plain nin at one batch size:
[batch * 96][32][32] and [batch * 192][16][16], per form (fp32, sign codes, fused with the IAO quantizer) and direction.

    python scripts/kbench_pool3.py [--batch 256] [--warmup 5] [--iters 30] [--out profiles/pool3_kernels.json]

Both sides of a pair are alternated in ONE process (the procedure of scripts/kbench_codes.py): warm-up, then HIP events around each call.  Stock paths: fp32 =
F.max_pool2d and its autograd backward; sign = ops.sign_to_float (the fp32 +-1 tensor) + F.max_pool2d; iao = the separate fake-quant launch + F.max_pool2d + the
observer's full pass over the output (forward), the stock backward + the quantizer's clip-STE launch (backward); the new iao forward includes the observer update from
the partials it left.  Per pair: median / quartiles of both, and the new kernel's designed bytes (each operand read or written once) over its median.  No time is
promised."""
import argparse
import json
import os
import statistics
import sys
import types

import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def q(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), p25=statistics.quantiles(v, n=4)[0], p75=statistics.quantiles(v, n=4)[2])


def pair(stock, new, nbytes, args):
    for _ in range(args.warmup):
        stock(), new()
    t0, t1 = [], []
    for _ in range(args.iters):          # alternated: both see the same clocks and the same neighbours
        t0.append(timed(stock))
        t1.append(timed(new))
    m0, m1 = statistics.median(t0), statistics.median(t1)
    return dict(stock_ms=q(t0), new_ms=q(t1), stock_over_new=m0 / m1, designed_bytes=nbytes, new_GB_s=nbytes / m1 * 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "pool3_kernels.json"))
    args = ap.parse_args()
    from micronet_amd import ops
    from micronet_amd.sign_tensor import SignTensor
    torch.manual_seed(0)
    res = dict(batch=args.batch, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), maps={})
    grad = lambda y, x, g: torch.autograd.grad(y, x, g, retain_graph=True)
    for Cc, hw in ((96, 32), (192, 16)):
        shape, ho = (args.batch, Cc, hw, hw), hw // 2
        n, no = args.batch * Cc * hw * hw, args.batch * Cc * ho * ho
        x = torch.relu(torch.randn(shape, device="cuda")).requires_grad_()
        g = torch.randn((args.batch, Cc, ho, ho), device="cuda")
        a = SignTensor(torch.where(torch.randn(shape, device="cuda") < 0, -1, 1).to(torch.int8)).requires_grad_()
        qp = torch.tensor([[x.detach().max().item() / 127.5, 0.0, -127.5, 127.5]], device="cuda")
        mn, mx, st = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"), types.SimpleNamespace()
        out = {}
        with torch.no_grad():
            out["f32_fwd"] = pair(lambda: Fn.max_pool2d(x, 3, 2, 1), lambda: ops.MaxPool3x3S2F32.apply(x), 4 * n + 5 * no, args)
            out["sign_fwd"] = pair(lambda: Fn.max_pool2d(ops.sign_to_float(a), 3, 2, 1), lambda: ops.SignMaxPool3x3S2.apply(a), n + no, args)

            def iao_stock():
                y = Fn.max_pool2d(ops.IaoFakeQuant.apply(x, qp, 8, 0, True), 3, 2, 1)
                ops.iao_observe(y, 1, 1, False, 0.1, mn, mx)

            def iao_new():
                ops.IaoFakeQuantMaxPool3x3S2.apply(x, qp, 8, 0, True, st)
                ops.iao_observe_partials(st._mn_fwd_out, 1, False, 0.1, mn, mx)
            out["iao_fwd"] = pair(iao_stock, iao_new, 4 * n + 5 * no, args)
        y0, y1 = Fn.max_pool2d(x, 3, 2, 1), ops.MaxPool3x3S2F32.apply(x)
        out["f32_bwd"] = pair(lambda: grad(y0, x, g), lambda: grad(y1, x, g), 4 * n + 5 * no, args)
        s0, s1 = Fn.max_pool2d(ops.sign_to_float(a), 3, 2, 1), ops.SignMaxPool3x3S2.apply(a)
        out["sign_bwd"] = pair(lambda: grad(s0, a, g), lambda: grad(s1, a, g), 5 * n + 4 * no, args)
        q0, q1 = Fn.max_pool2d(ops.IaoFakeQuant.apply(x, qp, 8, 0, True), 3, 2, 1), ops.IaoFakeQuantMaxPool3x3S2.apply(x, qp, 8, 0, False, st)
        out["iao_bwd"] = pair(lambda: grad(q0, x, g), lambda: grad(q1, x, g), 8 * n + 5 * no, args)
        res["maps"]["%dx%dx%dx%d" % shape] = out
        for k, v in out.items():
            print("%-22s %-9s stock %.3f ms  new %.3f ms (p25 %.3f p75 %.3f)  stock/new %.2fx  new %.0f GB/s of designed bytes" % (
                "%dx%dx%dx%d" % shape, k, v["stock_ms"]["median"], v["new_ms"]["median"], v["new_ms"]["p25"], v["new_ms"]["p75"], v["stock_over_new"], v["new_GB_s"]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
