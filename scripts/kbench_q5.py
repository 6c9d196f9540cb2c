"""The dense 5x5 block on activation codes (k_q5_fwd, csrc/qgemm_q5.h; k_kk_wgrad<1, 25, MN_ACTQ_CODE8>) against the route it replaces, on plain nin's layer at one
batch size -- 96 -> 192 channels, 16 x 16 maps behind the first 3x3 / stride-2 max-pool -- at W4A4 and W2A2, and one nin training step with
prepare(fuse_pool3=True, code_conv5=...) off and on.

    python scripts/kbench_q5.py [--batch 256] [--warmup 5] [--iters 30] [--out profiles/q5_kernels.json]

The method of scripts/kbench_pool3.py: both sides of a pair alternated in ONE process, warm-up, HIP events around each call, median and quartiles.
  forward   old: mn_qa_fwd(pool = 2, act_f32) from the 32 x 32 stash in front + mn_conv2d_fwd with the DoReFa prologue (fp32 y) + mn_bn_save_stats over y;
            new: mn_qa_fwd(pool = 2, codes) + mn_qconv_bnq_fwd_stash (weight pack, k_q5_fwd, statistics finish).
  wgrad     old: mn_conv2d_bwd_weight on the fp32 activation (DoReFa prologue); new: on the code bytes.
No time is promised."""
import argparse
import ctypes as C
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
    ap.add_argument("--out", default=os.path.join("profiles", "q5_kernels.json"))
    args = ap.parse_args()
    from micronet.compression.quantization.wqaq.dorefa import quantize as Q
    from micronet_amd import _lib, ops
    from micronet_amd.ops import ACTQ_CODE8, ACTQ_DOREFA, WQ_DOREFA, ActQ, WQ, _call, _geom, _p, _s, _ws
    from micronet_amd.train import build_model, make_optimizer, synth_batch, train_step
    torch.manual_seed(0)
    lib = ops._lib_()
    res = dict(batch=args.batch, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), layer="96->192 5x5 on 16x16", bits={})
    new = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda")
    N, Ci, Co, H = args.batch, 96, 192, 16
    g = _geom((N, Ci, H, H), (Co, Ci, 5, 5), 1, 2, 1, 1, 0)
    for bits in (4, 2):
        n = 2 ** bits - 1
        stash0 = (torch.randn((N, Ci, 2 * H, 2 * H), device="cuda") * 1150).round().clamp(-32767, 32767).to(torch.int16)
        one, zero = torch.ones(Ci, device="cuda"), torch.zeros(Ci, device="cuda")
        chan0 = torch.stack([one / 600, zero, zero, one, one, zero + 0.3, one / 600, zero, one]).contiguous()
        w = (2 * torch.randint(0, n + 1, (Co, Ci, 5, 5), device="cuda").float() / n - 1).contiguous()
        bias, gamma, beta = torch.zeros(Co, device="cuda"), torch.ones(Co, device="cuda"), torch.zeros(Co, device="cuda")
        rm, rv, nbt = torch.zeros(Co, device="cuda"), torch.ones(Co, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        act, codes, y, gy = new((N, Ci, H, H)), new((N, Ci, H, H), torch.uint8), new((N, Co, H, H)), torch.randn((N, Co, H, H), device="cuda")
        wd, aq_f, aq_c = WQ(WQ_DOREFA, bits, 0, 0, None), ActQ(ACTQ_DOREFA, bits, 0, 0, None), ActQ(ACTQ_CODE8, bits, 0, 0, None)
        assert lib.mn_qconv_bnq_supported(C.byref(g), C.byref(wd), bits) == 1
        sbits = int(lib.mn_qconv_bnq_stash_bits(C.byref(g), C.byref(wd), bits))
        stash = new((N, Co, H, H), torch.int32 if sbits == 32 else torch.int16)
        save, chan, dw = new((2, Co)), new((_lib.MN_QA_NCH, Co)), new((Co, Ci, 5, 5))
        ws0, nb0 = _ws(g, 0, "cuda")
        ws2, nb2 = _ws(g, 2, "cuda")
        nbq = int(lib.mn_qconv_bnq_ws_bytes(C.byref(g)))
        wsq, wss = new(nbq // 4 + 4), new(int(lib.mn_bnsign_ws_floats(Co)))

        def old_fwd():
            _call("mn_qa_fwd", 0, _p(stash0), _p(chan0), N, Ci, 2 * H, 2 * H, bits, 2, None, _p(act), _s())
            _call("mn_conv2d_fwd", C.byref(g), C.byref(aq_f), C.byref(wd), _p(act), _p(w), _p(bias), _p(y), _p(ws0), nb0, _lib.MN_ALGO_AUTO, _s())
            _call("mn_bn_save_stats", _p(y), N, Co, H * H, 1e-5, 0.1, 1, _p(rm), _p(rv), _p(save), _p(wss), _s())

        def new_fwd():
            _call("mn_qa_fwd", 0, _p(stash0), _p(chan0), N, Ci, 2 * H, 2 * H, bits, 2, _p(codes), None, _s())
            _call("mn_qconv_bnq_fwd_stash", C.byref(g), C.byref(wd), _p(codes), bits, _p(w), _p(bias), _p(gamma), _p(beta), 1e-5, 0.1, 1, _p(rm), _p(rv), _p(nbt), _p(save),
                  _p(stash), _p(chan), _p(wsq), nbq, _s())

        def old_wgrad():
            _call("mn_conv2d_bwd_weight", C.byref(g), C.byref(aq_f), _p(gy), _p(act), _p(dw), None, _p(ws2), nb2, _lib.MN_ALGO_AUTO, _s())

        def new_wgrad():
            _call("mn_conv2d_bwd_weight", C.byref(g), C.byref(aq_c), _p(gy), _p(codes), _p(dw), None, _p(ws2), nb2, _lib.MN_ALGO_AUTO, _s())
        nx, ny = N * Ci * H * H, N * Co * H * H
        out = dict(stash_bits=sbits, fwd=pair(old_fwd, new_fwd, 2 * 4 * nx + nx // 4 + nx + (sbits // 8) * ny, args))
        out["fwd_kernel"] = lib.mn_last_kernel().decode()
        out["wgrad"] = pair(old_wgrad, new_wgrad, nx + 4 * ny, args)
        out["wgrad_kernel"] = lib.mn_last_kernel().decode()
        res["bits"]["W%dA%d" % (bits, bits)] = out
        for k in ("fwd", "wgrad"):
            v = out[k]
            print("W%dA%d %-6s old %.3f ms  new %.3f ms (p25 %.3f p75 %.3f)  old/new %.2fx  [%s]" % (
                bits, bits, k, v["stock_ms"]["median"], v["new_ms"]["median"], v["new_ms"]["p25"], v["new_ms"]["p75"], v["stock_over_new"], out[k + "_kernel"]), flush=True)
    # one training step of plain nin with the pools folded, the 5x5 on fp32 (stock side of the pair) and on codes
    base = build_model("nin")
    x, yb = synth_batch(args.batch, device="cuda")
    for bits in (4, 2):
        steps = []
        for flag in (False, True):
            model = Q.prepare(base, a_bits=bits, w_bits=bits, fuse_pool3=True, code_conv5=flag).cuda().train()
            opt = make_optimizer(model, 0.01, 0.0)
            steps.append(lambda model=model, opt=opt: train_step(model, opt, x, yb))
        v = res["nin_w%da%d_step" % (bits, bits)] = pair(steps[0], steps[1], 0, args)
        print("nin W%dA%d step  code_conv5 off %.3f ms  on %.3f ms (p25 %.3f p75 %.3f)  off/on %.3fx" % (
            bits, bits, v["stock_ms"]["median"], v["new_ms"]["median"], v["new_ms"]["p25"], v["new_ms"]["p75"], v["stock_over_new"]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
