"""Byte path vs bit path of the deployed (BN-folded, pre-quantised) W-ternary / A-binary nin_gc (or, --model nin, the plain nin): images/s of the folded graph ``F`` (one byte per activation, the
training kernels in eval mode) and of ``B = inference.wbwtab_compile_bits(F)`` (one bit per hidden activation), alternated in ONE process, HIP events.

    python scripts/kbench_bits.py [--model nin_gc|nin] [--batches 256,1024] [--warmup 5] [--iters 20] [--out profiles/bits_inference[_nin].json]

Per batch: median / min of the timed forwards of each, the spread of F's own runs, B's per-kernel time from the library's profile hooks, and the designed HBM
bytes per image per layer (each operand read or written once).  --model nin adds the design comparison of its two dense blocks, kernel against kernel on the
same table: the LDS-tiled 5x5 against the global re-read loop at KS = 5, and the rolled 3x3 the plan uses against the LDS-tiled kernel (MN_BITCONV_ALT).

    python scripts/kbench_bits.py --mfma-blocks --mfma-k3 [--model nin_gc|nin] [--out profiles/bits_mfma[_nin].json]

With either flag the three graphs F (folded), B0 = wbwtab_compile_bits(F) (the default plan: the yardstick) and B1 = wbwtab_compile_bits(F, mfma_blocks=..., mfma_k3=...)
are alternated in one process instead: medians and quartiles of each, the logits bit-equal, and the per-kernel ms of the launches B1 replaces beside the new ones."""
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
        pk = L["pool_ksp"]
        ho = (h + 2 * pk[2] - pk[0]) // pk[1] + 1 if pk else h
        rows.append(dict(name=r["name"], kernel=r["kernel"], bits_bytes=4 * ((L["cin"] + 31) // 32) * h * h + 4 * ((L["cout"] + 31) // 32) * ho * ho,
                         byte_path_bytes=L["cin"] * h * h + 2 * L["cout"] * h * h))          # byte path: codes in, codes + stash out
        h = ho
    c1 = B.layers[0]["cin"]
    first = dict(name=B.report[0]["name"], bits_bytes=3 * 4 * hw * hw + 2 * c1 * hw * hw + 4 * ((c1 + 31) // 32) * hw * hw, byte_path_bytes=3 * 4 * hw * hw + c1 * hw * hw)
    cl = B.layers[-1]["cout"]
    last = dict(name=B.report[-1]["name"], bits_bytes=4 * ((cl + 31) // 32) * h * h + 2 * cl * h * h + 4 * 10 * h * h, byte_path_bytes=cl * h * h + 4 * 10 * h * h)
    return [first] + rows + [last]


def kernel_ab(lib, _lib, bs, cin, cout, k, hw, iters, warmup):
    """The two kernels that can run one dense block (plan's choice first, MN_BITCONV_ALT second), alternated: per-launch HIP-event times in ms."""
    import ctypes as C
    from micronet_amd import ops
    g = _lib.ConvGeom(bs, cin, hw, hw, cout, k, k, 1, 1, (k - 1) // 2, (k - 1) // 2, 1, 1, 1, 0)
    gen = torch.Generator(device="cuda").manual_seed(k)
    w = (torch.randint(-1, 2, (cout, cin, k, k), device="cuda", generator=gen).float() * 0.05).contiguous()
    b = torch.randn(cout, device="cuda", generator=gen)
    table = torch.empty(int(lib.mn_bitconv_table_bytes(C.byref(g))) // 4, dtype=torch.int32, device="cuda")
    ops._call("mn_bitconv_pack", C.byref(g), ops._p(w), ops._p(b), None, ops._p(table), ops._s())
    x = torch.randint(-2 ** 31, 2 ** 31 - 1, (bs, (cin + 31) // 32, hw, hw), device="cuda", generator=gen, dtype=torch.int64).to(torch.int32)
    ya, yb = (torch.empty((bs, (cout + 31) // 32, hw, hw), dtype=torch.int32, device="cuda") for _ in range(2))
    names, times = {}, {0: [], 0x100: []}
    run = lambda flag, y: ops._call("mn_bitconv_fwd", C.byref(g), ops._p(table), ops._p(x), ops._p(y), flag, ops._s())
    for flag, y in ((0, ya), (0x100, yb)):
        run(flag, y)
        names[flag] = lib.mn_last_kernel().decode()
    assert torch.equal(ya, yb), "the two kernels must agree bit for bit"
    for i in range(warmup + iters):
        for flag, y in ((0, ya), (0x100, yb)):
            t = timed(lambda _: run(flag, y), None)
            if i >= warmup:
                times[flag].append(t)
    q = lambda v: dict(median=statistics.median(v), min=min(v), p25=statistics.quantiles(v, n=4)[0], p75=statistics.quantiles(v, n=4)[2])
    return dict(geometry="%d -> %d, %dx%d on %d x %d, batch %d" % (cin, cout, k, k, hw, hw, bs), plan_kernel=names[0], plan_ms=q(times[0]), alt_kernel=names[0x100],
                alt_ms=q(times[0x100]), alt_over_plan=statistics.median(times[0x100]) / statistics.median(times[0]))


def quart(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), p25=statistics.quantiles(v, n=4)[0], p75=statistics.quantiles(v, n=4)[2])


def main_mfma(args):
    """F / B0 / B1 alternated; B0 is the default plan, B1 the plan with the MFMA forms asked for."""
    from micronet.compression.quantization.wbwtab import quantize as Q
    from micronet_amd import _lib, inference
    from micronet_amd.train import build_model, synth_batch
    torch.manual_seed(0)
    I = Q.prepare(build_model(args.model), inplace=True, A=2, W=args.W, quant_inference=True).cuda()
    inference.prequantize_weights(I)
    F = inference.wbwtab_model_bn_fuse(I, W=args.W).eval()
    B0 = inference.wbwtab_compile_bits(F)
    B1 = inference.wbwtab_compile_bits(F, mfma_blocks=args.mfma_blocks, mfma_k3=args.mfma_k3)
    lib = _lib.get_lib()
    moved = [(a["name"], a["kernel"], b["kernel"]) for a, b in zip(B0.report, B1.report) if a != b]
    res = dict(model=args.model, W=args.W, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), mfma_blocks=args.mfma_blocks, mfma_k3=args.mfma_k3,
               report_B0=B0.report, report_B1=B1.report, moved=[dict(name=n, B0=a, B1=b) for n, a, b in moved],
               spans=[dict(name=L["name"], span=int(L["table"][2]), dead_rows=int(L["table"][5])) for L in B1.layers if L.get("mfma3")], batches={})
    old = lambda k: k.startswith("k_bitconv<")
    new = lambda k: k.startswith("k_bitconv_mfma")
    with torch.no_grad():
        for bs in [int(v) for v in args.batches.split(",")]:
            x, _ = synth_batch(bs, device="cuda")
            f = F(x)
            assert torch.equal(f, B0(x)) and torch.equal(f, B1(x)), "logits must be bit-equal"
            for _ in range(args.warmup):
                F(x), B0(x), B1(x)
            tf, t0, t1 = [], [], []
            for _ in range(args.iters):          # alternated: all three see the same clocks and the same neighbours
                tf.append(timed(F, x))
                t0.append(timed(B0, x))
                t1.append(timed(B1, x))
            k0, k1, kf = profile(lib, _lib, B0, x), profile(lib, _lib, B1, x), profile(lib, _lib, F, x)
            replaced = {k: v for k, v in k0.items() if k not in k1 or k1[k]["launches"] != v["launches"]}
            added = {k: v for k, v in k1.items() if new(k)}
            mf, m0, m1 = statistics.median(tf), statistics.median(t0), statistics.median(t1)
            res["batches"][str(bs)] = dict(
                F_ms=quart(tf), B0_ms=quart(t0), B1_ms=quart(t1), F_img_s=bs / mf * 1e3, B0_img_s=bs / m0 * 1e3, B1_img_s=bs / m1 * 1e3,
                B0_over_F=mf / m0, B1_over_F=mf / m1, B1_over_B0=m0 / m1, logits_bit_equal=True,
                B0_kernels=k0, B1_kernels=k1, F_kernels=kf, replaced_kernels_B0=replaced, new_kernels_B1=added,
                replaced_ms=sum(v["ms"] for v in replaced.values()) - sum(k1[k]["ms"] for k in replaced if k in k1 and old(k)), new_ms=sum(v["ms"] for v in added.values()),
                B0_kernel_ms_total=sum(v["ms"] for v in k0.values()), B1_kernel_ms_total=sum(v["ms"] for v in k1.values()), F_kernel_ms_total=sum(v["ms"] for v in kf.values()))
            print("batch %d: F %.3f ms  B0 %.3f ms  B1 %.3f ms  B0/F %.2fx  B1/F %.2fx  B1/B0 %.2fx" % (bs, mf, m0, m1, mf / m0, mf / m1, m0 / m1), flush=True)
            for k, v in sorted(replaced.items()):
                print("  B0 %-28s x%d %.4f ms" % (k, v["launches"], v["ms"]) + ("   (B1 keeps x%d %.4f ms)" % (k1[k]["launches"], k1[k]["ms"]) if k in k1 else ""), flush=True)
            for k, v in sorted(added.items()):
                print("  B1 %-28s x%d %.4f ms" % (k, v["launches"], v["ms"]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="nin_gc", choices=["nin_gc", "nin"])
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--W", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mfma-blocks", action="store_true", help="B1: the 1x1 hidden blocks on mn_bitconv_mfma_*")
    ap.add_argument("--mfma-k3", action="store_true", help="B1: the un-pooled 3x3 hidden blocks on mn_bitconv_mfma3_*")
    args = ap.parse_args()
    if args.mfma_blocks or args.mfma_k3:
        if args.out is None:
            args.out = os.path.join("profiles", "bits_mfma.json" if args.model == "nin_gc" else "bits_mfma_%s.json" % args.model)
        return main_mfma(args)
    if args.out is None:
        args.out = os.path.join("profiles", "bits_inference.json" if args.model == "nin_gc" else "bits_inference_%s.json" % args.model)
    from micronet.compression.quantization.wbwtab import quantize as Q
    from micronet_amd import _lib, inference
    from micronet_amd.train import build_model, synth_batch
    torch.manual_seed(0)
    I = Q.prepare(build_model(args.model), inplace=True, A=2, W=args.W, quant_inference=True).cuda()
    inference.prequantize_weights(I)
    F = inference.wbwtab_model_bn_fuse(I, W=args.W).eval()
    B = inference.wbwtab_compile_bits(F)
    lib = _lib.get_lib()
    res = dict(model=args.model, W=args.W, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), report=B.report,
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
            if args.model == "nin":
                res["batches"][str(bs)]["dense_blocks"] = [kernel_ab(lib, _lib, bs, 96, 192, 5, 16, args.iters, args.warmup),
                                                           kernel_ab(lib, _lib, bs, 192, 192, 3, 8, args.iters, args.warmup)]
                for d in res["batches"][str(bs)]["dense_blocks"]:
                    print("  %s: %s %.3f ms, %s %.3f ms" % (d["geometry"], d["plan_kernel"], d["plan_ms"]["median"], d["alt_kernel"], d["alt_ms"]["median"]), flush=True)
            print("batch %d: F %.3f ms (min %.3f)  B %.3f ms (min %.3f)  B/F speed %.2fx" % (bs, med_f, min(tf), med_b, min(tb), med_f / med_b), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
