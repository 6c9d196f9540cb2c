"""The fused k-bit block through the 3x3 / stride-2 / padding-1 max-pool (mn_qa_* with pool = 2, csrc/qact_pool3.h) against the path it replaces, on the two pooled
positions of plain nin at one batch size -- [batch][96][32][32] and [batch][192][16][16], a 16-bit stash, 4-bit codes -- and one W4A4 nin training step with
prepare(fuse_pool3=...) off and on.

    python scripts/kbench_qa_pool3.py [--batch 256] [--warmup 5] [--iters 30] [--out profiles/qa_pool3_kernels.json]

The method of scripts/kbench_pool3.py: both sides of a pair alternated in ONE process, warm-up, HIP events around each call, median and quartiles.  The old side is the
un-fused block + pool: forward mn_qa_fwd(pool = 0) to fp32, then mn_maxpool3x3s2_f32_fwd; backward mn_maxpool3x3s2_f32_bwd, then mn_qa_bwd(pool = 0, quant = 0) on the
scattered gradient.  The new side: mn_qa_fwd(pool = 2) to codes; mn_qa_bwd(pool = 2, quant = 1).  Designed bytes of the new side (each operand read or written once per
pass): forward 2 n + n / 4, backward (2 n + n) + (2 n + n + 4 n).  No time is promised."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kbench_pool3 import pair          # noqa: E402  (warm-up, alternated HIP-event timing, quartiles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "qa_pool3_kernels.json"))
    args = ap.parse_args()
    from micronet.compression.quantization.wqaq.dorefa import quantize as Q
    from micronet_amd import ops
    from micronet_amd.ops import _call, _p, _s
    from micronet_amd.train import build_model, make_optimizer, synth_batch, train_step
    torch.manual_seed(0)
    res = dict(batch=args.batch, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), maps={})
    new = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda")
    for Cc, hw in ((96, 32), (192, 16)):
        N, H, W, ho = args.batch, hw, hw, hw // 2
        n = N * Cc * H * W
        stash = (torch.randn((N, Cc, H, W), device="cuda") * 1150).round().clamp(-32767, 32767).to(torch.int16)
        one, zero = torch.ones(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
        alpha, beta = one / 600, zero + 0.3          # z = acc / 600 + 0.3: about 44 % of the ReLUs closed
        chan = torch.stack([alpha, zero, zero, one, one, beta, alpha, zero, one]).contiguous()
        dq, gq = torch.randn((N, Cc, ho, ho), device="cuda"), torch.randn((N, Cc, ho, ho), device="cuda")
        act, pooled, idx, codes = new((N, Cc, H, W)), new((N, Cc, ho, ho)), new((N, Cc, ho, ho), torch.uint8), new((N, Cc, ho, ho), torch.uint8)
        dx, dy, dgam, dbet, sums = new((N, Cc, H, W)), new((N, Cc, H, W)), new(Cc), new(Cc), new((2, Cc))
        ws = new(int(ops._lib_().mn_qa_ws_floats(Cc)))

        def old_fwd():
            _call("mn_qa_fwd", 0, _p(stash), _p(chan), N, Cc, H, W, 4, 0, None, _p(act), _s())
            _call("mn_maxpool3x3s2_f32_fwd", _p(act), N * Cc, H, W, _p(pooled), _p(idx), _s())

        def new_fwd():
            _call("mn_qa_fwd", 0, _p(stash), _p(chan), N, Cc, H, W, 4, 2, _p(codes), None, _s())

        def old_bwd():
            _call("mn_maxpool3x3s2_f32_bwd", _p(gq), _p(idx), N * Cc, H, W, _p(dx), _s())
            _call("mn_qa_bwd", 0, _p(stash), _p(chan), _p(dx), N, Cc, H, W, 4, 0, 0, 1, _p(dgam), _p(dbet), _p(sums), _p(dy), _p(ws), _s())

        def new_bwd():
            _call("mn_qa_bwd", 0, _p(stash), _p(chan), _p(dq), N, Cc, H, W, 4, 2, 1, 1, _p(dgam), _p(dbet), _p(sums), _p(dy), _p(ws), _s())
        out = dict(fwd=pair(old_fwd, new_fwd, 2 * n + n // 4, args), bwd=pair(old_bwd, new_bwd, 10 * n, args))
        res["maps"]["%dx%dx%dx%d" % (N, Cc, H, W)] = out
        for k, v in out.items():
            print("%-16s %-4s old %.3f ms  new %.3f ms (p25 %.3f p75 %.3f)  old/new %.2fx  new %.0f GB/s of designed bytes" % (
                "%dx%dx%dx%d" % (N, Cc, H, W), k, v["stock_ms"]["median"], v["new_ms"]["median"], v["new_ms"]["p25"], v["new_ms"]["p75"], v["stock_over_new"], v["new_GB_s"]),
                flush=True)
    # one W4A4 training step of plain nin, the pools un-fused (stock side of the pair) and folded
    base = build_model("nin")
    x, y = synth_batch(args.batch, device="cuda")
    steps = []
    for flag in (False, True):
        model = Q.prepare(base, a_bits=4, w_bits=4, fuse_pool3=flag).cuda().train()
        opt = make_optimizer(model, 0.01, 0.0)
        steps.append(lambda model=model, opt=opt: train_step(model, opt, x, y))
    res["nin_w4a4_step"] = pair(steps[0], steps[1], 0, args)
    v = res["nin_w4a4_step"]
    print("nin W4A4 step    fuse_pool3 off %.3f ms  on %.3f ms (p25 %.3f p75 %.3f)  off/on %.3fx" % (
        v["stock_ms"]["median"], v["new_ms"]["median"], v["new_ms"]["p25"], v["new_ms"]["p75"], v["stock_over_new"]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
