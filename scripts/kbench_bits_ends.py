"""The deployed bit plan with its two ends on bytes (``P0 = inference.wbwtab_compile_bits(F)``, the yardstick) and on bits (``P1 = ...(F, bit_ends=True)``), alternated
in ONE process, HIP events; and the two new kernels beside the launches they replace, from the library's profile hooks.

    python scripts/kbench_bits_ends.py [--model nin_gc|nin] [--batch 256] [--warmup 5] [--iters 20] [--out profiles/bits_ends.json]

Writes per-kernel microseconds (mean of --iters profiled launches), the plan's milliseconds (median / min / quartiles of the timed forwards of each plan) and the
device's name.  The outputs of the two plans are compared first: they must be equal."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIRST_OLD = ("k_c1b_fwd<", "k_c1_fwd<", "k_bns_apply<0, 1>", "k_bits_pack")
LAST_OLD = ("k_bits_unpack", "k_sconv_fwd")


def timed(fn, x):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(x)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def profile_us(lib, _lib, fn, x, iters):
    buf = (_lib.ProfEntry * 192)()
    torch.cuda.synchronize()
    lib.mn_profile_collect(buf, 192)
    lib.mn_profile_enable(1)
    for _ in range(iters):
        fn(x)
    torch.cuda.synchronize()
    n = lib.mn_profile_collect(buf, 192)
    lib.mn_profile_enable(0)
    return {buf[i].name.decode(): dict(launches_per_forward=int(buf[i].launches) / iters, us=1e3 * float(buf[i].total_ms) / max(int(buf[i].launches), 1)) for i in range(n)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="nin_gc", choices=["nin_gc", "nin"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--W", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "bits_ends.json"))
    args = ap.parse_args()
    from micronet.compression.quantization.wbwtab import quantize as Q
    from micronet_amd import _lib, inference
    from micronet_amd.train import build_model, synth_batch
    torch.manual_seed(0)
    I = Q.prepare(build_model(args.model), inplace=True, A=2, W=args.W, quant_inference=True).cuda()
    inference.prequantize_weights(I)
    F = inference.wbwtab_model_bn_fuse(I, W=args.W).eval()
    P0, P1 = inference.wbwtab_compile_bits(F), inference.wbwtab_compile_bits(F, bit_ends=True)
    lib = _lib.get_lib()
    q = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v), p25=statistics.quantiles(v, n=4)[0], p75=statistics.quantiles(v, n=4)[2])
    with torch.no_grad():
        x, _ = synth_batch(args.batch, device="cuda")
        assert torch.equal(P0(x), P1(x)), "the two plans must agree bit for bit"
        for _ in range(args.warmup):
            P0(x), P1(x)
        t0, t1 = [], []
        for _ in range(args.iters):          # alternated: both see the same clocks and the same neighbours
            t0.append(timed(P0, x))
            t1.append(timed(P1, x))
        k0, k1 = profile_us(lib, _lib, P0, x, args.iters), profile_us(lib, _lib, P1, x, args.iters)
    pick = lambda k, pre: {n: v["us"] for n, v in k.items() if n.startswith(pre)}
    first_old, last_old = pick(k0, FIRST_OLD), pick(k0, LAST_OLD)
    first_new, last_new = pick(k1, ("k_c1b_fwd<",)), pick(k1, ("k_bitsconv1x1_small",))
    res = dict(model=args.model, W=args.W, batch=args.batch, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0),
               arch=torch.cuda.get_device_properties(0).gcnArchName,
               plan_ms=dict(bit_ends_false=q(t0), bit_ends_true=q(t1), speedup_median=statistics.median(t0) / statistics.median(t1)),
               first_stage_us=dict(bit_ends_false=first_old, bit_ends_true=first_new, sum_false=sum(first_old.values()), sum_true=sum(first_new.values())),
               last_stage_us=dict(bit_ends_false=last_old, bit_ends_true=last_new, sum_false=sum(last_old.values()), sum_true=sum(last_new.values())),
               kernels_us=dict(bit_ends_false=k0, bit_ends_true=k1),
               kernel_us_total=dict(bit_ends_false=sum(v["us"] * v["launches_per_forward"] for v in k0.values()),
                                    bit_ends_true=sum(v["us"] * v["launches_per_forward"] for v in k1.values())))
    print("batch %d: bit_ends=False %.3f ms (min %.3f)  bit_ends=True %.3f ms (min %.3f)  speed-up %.2fx" %
          (args.batch, statistics.median(t0), min(t0), statistics.median(t1), min(t1), res["plan_ms"]["speedup_median"]), flush=True)
    print("first stage: %s = %.1f us -> %s = %.1f us" % (first_old, sum(first_old.values()), first_new, sum(first_new.values())))
    print("last stage: %s = %.1f us -> %s = %.1f us" % (last_old, sum(last_old.values()), last_new, sum(last_new.values())))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
