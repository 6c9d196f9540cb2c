"""Byte path vs bit path of the deployed (BN-folded, pre-quantised) W-ternary / A-binary nin_gc: images/s of the folded graph ``F`` (one byte per activation, the
training kernels in eval mode) and of ``B = inference.wbwtab_compile_bits(F)`` (one bit per hidden activation), alternated in ONE process, HIP events.

    python scripts/kbench_bits.py [--batches 256,1024] [--warmup 5] [--iters 20] [--out profiles/bits_inference.json]

Per batch: median / min of the timed forwards of each, the spread of F's own runs, B's per-kernel time from the library's profile hooks, and the designed HBM
bytes per image per layer (each operand read or written once)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, x):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(x)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def profile(lib, _lib, fn, x):
    buf = (_lib.ProfEntry * 192)()
    torch.cuda.synchronize()
    lib.mn_profile_collect(buf, 192)
    lib.mn_profile_enable(1)
    fn(x)
    torch.cuda.synchronize()
    n = lib.mn_profile_collect(buf, 192)
    lib.mn_profile_enable(0)
    return {buf[i].name.decode(): dict(launches=int(buf[i].launches), ms=float(buf[i].total_ms), designed_bytes=float(buf[i].bytes)) for i in range(n)}


def designed_bytes_per_image(B, hw=32):
    """First block: image in, int8 signs out, bits out.  Bit blocks: input words + output words.  Last: bits in, int8 out and in, fp32 logit maps out."""
    rows, h = [], hw
    for r, L in zip(B.report[1:-1], B.layers):
        ho = h // 2 if L["pool"] else h
        rows.append(dict(name=r["name"], kernel=r["kernel"], bits_bytes=4 * ((L["cin"] + 31) // 32) * h * h + 4 * ((L["cout"] + 31) // 32) * ho * ho,
                         byte_path_bytes=L["cin"] * h * h + 2 * L["cout"] * h * h))          # byte path: codes in, codes + stash out
        h = ho
    c1 = B.layers[0]["cin"]
    first = dict(name=B.report[0]["name"], bits_bytes=3 * 4 * hw * hw + 2 * c1 * hw * hw + 4 * ((c1 + 31) // 32) * hw * hw, byte_path_bytes=3 * 4 * hw * hw + c1 * hw * hw)
    cl = B.layers[-1]["cout"]
    last = dict(name=B.report[-1]["name"], bits_bytes=4 * ((cl + 31) // 32) * h * h + 2 * cl * h * h + 4 * 10 * h * h, byte_path_bytes=cl * h * h + 4 * 10 * h * h)
    return [first] + rows + [last]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--W", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "bits_inference.json"))
    args = ap.parse_args()
    from micronet.compression.quantization.wbwtab import quantize as Q
    from micronet_amd import _lib, inference
    from micronet_amd.train import build_model, synth_batch
    torch.manual_seed(0)
    I = Q.prepare(build_model("nin_gc"), inplace=True, A=2, W=args.W, quant_inference=True).cuda()
    inference.prequantize_weights(I)
    F = inference.wbwtab_model_bn_fuse(I, W=args.W).eval()
    B = inference.wbwtab_compile_bits(F)
    lib = _lib.get_lib()
    res = dict(model="nin_gc", W=args.W, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), report=B.report,
               designed_bytes_per_image=designed_bytes_per_image(B), batches={})
    with torch.no_grad():
        for bs in [int(v) for v in args.batches.split(",")]:
            x, _ = synth_batch(bs, device="cuda")
            assert torch.equal(F(x), B(x))
            for _ in range(args.warmup):
                F(x), B(x)
            tf, tb = [], []
            for _ in range(args.iters):          # alternated: both see the same clocks and the same neighbours
                tf.append(timed(F, x))
                tb.append(timed(B, x))
            kb, kf = profile(lib, _lib, B, x), profile(lib, _lib, F, x)
            first_ms = sum(v["ms"] for k, v in kb.items() if not k.startswith(("k_bitconv", "k_bits_unpack", "k_sconv")))
            med_f, med_b = statistics.median(tf), statistics.median(tb)
            res["batches"][str(bs)] = dict(
                F_ms=dict(median=med_f, min=min(tf), max=max(tf), p25=statistics.quantiles(tf, n=4)[0], p75=statistics.quantiles(tf, n=4)[2]),
                B_ms=dict(median=med_b, min=min(tb), max=max(tb), p25=statistics.quantiles(tb, n=4)[0], p75=statistics.quantiles(tb, n=4)[2]),
                F_img_s=bs / med_f * 1e3, B_img_s=bs / med_b * 1e3, B_over_F=med_f / med_b,
                B_kernels=kb, F_kernels=kf, B_kernel_ms_total=sum(v["ms"] for v in kb.values()), F_kernel_ms_total=sum(v["ms"] for v in kf.values()),
                B_first_block_kernel_ms=first_ms)
            print("batch %d: F %.3f ms (min %.3f)  B %.3f ms (min %.3f)  B/F speed %.2fx" % (bs, med_f, min(tf), med_b, min(tb), med_f / med_b), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
