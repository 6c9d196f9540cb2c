"""Byte path vs code-packed path of a deployed (pre-quantised) DoReFa W2A2 nin_gc: images/s of the eval-mode ``quant_inference=True`` model ``I`` (one byte per hidden
activation plus a 16-bit stash per block: the training kernels in eval mode -- the yardstick) and of ``P = inference.dorefa_compile_codes(I)`` (two bits per hidden
activation, one kernel per hidden block), alternated in ONE process, HIP events.

    python scripts/kbench_codes.py [--batches 256,1024] [--warmup 5] [--iters 20] [--out profiles/codes_inference.json]

Per batch: median / min / quartiles of the timed forwards of each, per-kernel times of both from the library's profile hooks, and the designed HBM bytes per image
per hidden block (arithmetic from the shapes: each operand read or written once).

    python scripts/kbench_codes.py --code-ends [--batches 256,1024] [--warmup 5] [--iters 20] [--out profiles/codes_ends.json]

alternates the default plan (``code_ends=False``: the yardstick) and ``dorefa_compile_codes(I, code_ends=True)`` the same way and reports the per-kernel times of
the launches replaced (first conv, k_qa_fwd, k_codes_pack, k_codes_unpack, the classifier on byte codes) beside the two new ones.

    python scripts/kbench_codes.py --arch nin [--batches 256,1024] [--warmup 5] [--iters 20] [--out profiles/codes_nin.json]

is the first protocol on PLAIN nin: ``P = dorefa_compile_codes(I, tile_blocks=True)`` (the dense 5x5 block on an LDS tile, the two 3x3 / 2 max-pools on planes).

    python scripts/kbench_codes.py --mfma-blocks [--batches 256,1024] [--warmup 5] [--iters 20] [--out profiles/codes_mfma.json]

alternates ``I``, the default plan and ``dorefa_compile_codes(I, mfma_blocks=True)`` (the five 1x1 blocks of nin_gc on the int8-MFMA kernel) in one process and puts
the per-kernel time of ``k_codeconv_mfma`` beside that of the default plan's ``k_codeconv<1,4,*>`` and of the byte path's ``k_pws`` + ``k_qa_fwd`` on the same five
layers; the three logits must be bit-equal.

    python scripts/kbench_codes.py --mfma-k3 [--arch nin] [--batches 256,1024] [--warmup 5] [--iters 20] [--out profiles/codes_mfma3.json]

alternates ``I``, ``dorefa_compile_codes(I, mfma_blocks=True)`` and ``dorefa_compile_codes(I, mfma_blocks=True, mfma_k3=True)`` (the un-pooled 3x3 blocks on
``k_codeconv_mfma3`` as well) the same way and puts the per-kernel time of ``k_codeconv_mfma3`` beside that of ``k_codeconv<3,*>`` in the other plan and of the byte
path's 3x3 conv kernels; ``--arch nin`` adds ``tile_blocks=True`` to both plans (default output profiles/codes_mfma3_nin.json).

    python scripts/kbench_codes.py --bits 4 [--batches 256,1024] [--warmup 5] [--iters 20] [--out profiles/codes_w4a4.json] [--two-bit-check PARENT.json THIS.json]

builds nin_gc W4A4, its ``I`` and ``P = dorefa_compile_codes(I)`` (four bits per hidden activation, every hidden block on an int8-MFMA kernel), alternates the two and
writes medians, per-kernel times, the activation footprint and ``bit_equal``.  ``--two-bit-check``: two results of ``--mfma-k3`` (W2A2), one measured on the parent
commit and one on this tree in the same session, are compared -- P1's median against the parent's median plus its own p25-p75 width -- and recorded under
``two_bit_check``."""
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


def designed_bytes_per_image(P, hw=32):
    """Hidden blocks.  Byte path: codes in (1 B), 16-bit stash out and in again (2 + 2 B per un-pooled output), codes out (1 B per pooled output).  Code path: 2 bits per
    input element, 2 bits per (pooled) output element, in whole 32-channel words.  A max-pool that is not folded (plain nin's 3x3 / 2): on the byte path the block
    writes fp32 (4 B per output), the pool reads it and writes fp32 (4 B per pooled output), the consumer's quantizer reads that and writes codes (4 + 1 B per pooled
    output); on the code path the block writes planes at full size, the pool reads them and writes the pooled planes."""
    rows, h = [], hw
    for r, L in zip(P.report[1:-1], P.layers):
        ksp = L.get("pool_ksp")
        ho = h // 2 if L["pool"] else ((h + 2 * ksp[2] - ksp[0]) // ksp[1] + 1 if ksp else h)
        wi, wo = (L["cin"] + 31) // 32, (L["cout"] + 31) // 32
        if ksp:
            codes = 4 * 2 * wi * h * h + 2 * 4 * 2 * wo * h * h + 4 * 2 * wo * ho * ho
            byte = L["cin"] * h * h + 4 * L["cout"] * h * h + 2 * 4 * L["cout"] * h * h + (4 + 4 + 1) * L["cout"] * ho * ho
        else:
            codes = 4 * 2 * wi * h * h + 4 * 2 * wo * ho * ho
            byte = L["cin"] * h * h + 4 * L["cout"] * h * h + L["cout"] * ho * ho
        rows.append(dict(name=r["name"], kernel=r["kernel"], codes_bytes=codes, byte_path_bytes=byte))
        h = ho
    return rows


def q(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), p25=statistics.quantiles(v, n=4)[0], p75=statistics.quantiles(v, n=4)[2])


ENDS_REPLACED = ("k_c1b_fwd<", "k_c1_fwd<", "k_qa_fwd", "k_codes_pack", "k_codes_unpack", "k_sconv_fwd")          # the default plan's two ends
ENDS_NEW = ("k_c1b_fwd<", "k_planesconv1x1_small")


def main_code_ends(args):
    """The default plan P0 against the plan with both ends on planes P1, alternated in one process."""
    from micronet.compression.quantization.wqaq.dorefa import quantize as Q
    from micronet_amd import _lib, inference
    from micronet_amd.train import build_model, synth_batch
    torch.manual_seed(0)
    I = Q.prepare(build_model("nin_gc"), inplace=True, a_bits=2, w_bits=2, quant_inference=True).cuda()
    inference.prequantize_weights(I)
    I.eval()
    P0, P1 = inference.dorefa_compile_codes(I), inference.dorefa_compile_codes(I, code_ends=True)
    lib = _lib.get_lib()
    res = dict(model="nin_gc", a_bits=2, w_bits=2, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), report=P1.report, batches={})
    with torch.no_grad():
        for bs in [int(v) for v in args.batches.split(",")]:
            x, _ = synth_batch(bs, device="cuda")
            ref, got = P0(x), P1(x)
            for _ in range(args.warmup):
                P0(x), P1(x)
            t0, t1 = [], []
            for _ in range(args.iters):          # alternated: both see the same clocks and the same neighbours
                t0.append(timed(P0, x))
                t1.append(timed(P1, x))
            k0, k1 = profile(lib, _lib, P0, x), profile(lib, _lib, P1, x)
            us = lambda k, names: {n: round(1e3 * v["ms"] / max(1, v["launches"]), 2) for n, v in k.items() if n.startswith(names)}
            med0, med1 = statistics.median(t0), statistics.median(t1)
            res["batches"][str(bs)] = dict(P0_ms=q(t0), P1_ms=q(t1), P0_img_s=bs / med0 * 1e3, P1_img_s=bs / med1 * 1e3, P1_over_P0=med0 / med1,
                                           bit_equal=bool(torch.equal(ref, got)), replaced_us=us(k0, ENDS_REPLACED), new_us=us(k1, ENDS_NEW),
                                           P0_kernel_ms_total=sum(v["ms"] for v in k0.values()), P1_kernel_ms_total=sum(v["ms"] for v in k1.values()),
                                           P0_kernels=k0, P1_kernels=k1)
            print("batch %d: default plan %.3f ms (min %.3f)  code_ends %.3f ms (min %.3f)  speed %.2fx  bit-equal %s" % (bs, med0, min(t0), med1, min(t1), med0 / med1,
                                                                                                                  torch.equal(ref, got)), flush=True)
            print("  replaced (us):", res["batches"][str(bs)]["replaced_us"], " new (us):", res["batches"][str(bs)]["new_us"], flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


def main_mfma_blocks(args):
    """I, the default plan P0 and the plan with the 1x1 blocks on the MFMA kernel P1, alternated in one process."""
    from micronet.compression.quantization.wqaq.dorefa import quantize as Q
    from micronet_amd import _lib, inference
    from micronet_amd.train import build_model, synth_batch
    torch.manual_seed(0)
    I = Q.prepare(build_model("nin_gc"), inplace=True, a_bits=2, w_bits=2, quant_inference=True).cuda()
    inference.prequantize_weights(I)
    I.eval()
    P0, P1 = inference.dorefa_compile_codes(I), inference.dorefa_compile_codes(I, mfma_blocks=True)
    lib = _lib.get_lib()
    rows = designed_bytes_per_image(P1)
    # the 1x1 layers' share of the byte path's hidden k_qa_fwd launches (<0, 0> un-pooled, <0, 1> pooled; <1, *> is the first block's): its traffic is per conv output
    # element, so the share of each kind is taken by those
    el = {(p_, one): 0 for p_ in (0, 1) for one in (False, True)}
    for L, h in zip(P1.layers, _map_sizes(P1)):
        el[(L["pool"], L["k"] == 1)] += L["cout"] * h * h
    share = {p_: el[(p_, True)] / max(1, el[(p_, True)] + el[(p_, False)]) for p_ in (0, 1)}
    res = dict(model="nin_gc", a_bits=2, w_bits=2, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), report=P1.report,
               designed_bytes_per_image=rows, mfma_layers_codes_bytes_per_image=sum(r["codes_bytes"] for r, L in zip(rows, P1.layers) if L.get("mfma")),
               mfma_layers_macs_per_image=sum(L["cin"] // L["groups"] * L["cout"] * hh * hh for L, hh in zip(P1.layers, _map_sizes(P1)) if L.get("mfma")),
               qa_fwd_share_of_1x1_layers={"k_qa_fwd<0, 0>": share[0], "k_qa_fwd<0, 1>": share[1]}, batches={})
    with torch.no_grad():
        for bs in [int(v) for v in args.batches.split(",")]:
            x, _ = synth_batch(bs, device="cuda")
            ref, y0, y1 = I(x), P0(x), P1(x)
            equal = bool(torch.equal(ref, y0) and torch.equal(ref, y1))
            assert equal, "I, the default plan and the mfma_blocks plan must give bit-equal logits"
            for _ in range(args.warmup):
                I(x), P0(x), P1(x)
            ti, t0, t1 = [], [], []
            for _ in range(args.iters):          # alternated: all three see the same clocks and the same neighbours
                ti.append(timed(I, x))
                t0.append(timed(P0, x))
                t1.append(timed(P1, x))
            ki, k0, k1 = profile(lib, _lib, I, x), profile(lib, _lib, P0, x), profile(lib, _lib, P1, x)
            ms = lambda k, names: sum(v["ms"] for n, v in k.items() if n.startswith(names))
            mi, m0, m1 = statistics.median(ti), statistics.median(t0), statistics.median(t1)
            popc, mfma = ms(k0, ("k_codeconv<1,",)), ms(k1, ("k_codeconv_mfma<",))
            qa1 = ms(ki, ("k_qa_fwd<0, 0>",)) * share[0] + ms(ki, ("k_qa_fwd<0, 1>",)) * share[1]
            byte = ms(ki, ("k_pws",)) + qa1
            res["batches"][str(bs)] = dict(I_ms=q(ti), P0_ms=q(t0), P1_ms=q(t1), P0_over_I=mi / m0, P1_over_I=mi / m1, P1_over_P0=m0 / m1, bit_equal=equal,
                                           layers_1x1_ms=dict(popcount=popc, mfma=mfma, byte_path=byte, byte_path_k_pws=ms(ki, ("k_pws",)), byte_path_k_qa_fwd_share=qa1),
                                           I_kernels=ki, P0_kernels=k0, P1_kernels=k1)
            print("batch %d: I %.3f ms  default plan %.3f ms (%.2fx I)  mfma_blocks %.3f ms (%.2fx I, %.2fx default)  bit-equal %s" % (bs, mi, m0, mi / m0, m1, mi / m1, m0 / m1,
                                                                                                                              equal), flush=True)
            print("  five 1x1 layers: k_codeconv<1,*> %.3f ms  k_codeconv_mfma %.3f ms  byte path (k_pws + share of k_qa_fwd) %.3f ms" % (popc, mfma, byte), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


def main_mfma_k3(args):
    """I, the plan with the 1x1 blocks on MFMA P0 and the plan with the 3x3 blocks on MFMA as well P1, alternated in one process."""
    from micronet.compression.quantization.wqaq.dorefa import quantize as Q
    from micronet_amd import _lib, inference
    from micronet_amd.train import build_model, synth_batch
    torch.manual_seed(0)
    I = Q.prepare(build_model(args.arch), inplace=True, a_bits=2, w_bits=2, quant_inference=True).cuda()
    inference.prequantize_weights(I)
    I.eval()
    kw = dict(tile_blocks=True) if args.arch == "nin" else {}
    P0 = inference.dorefa_compile_codes(I, mfma_blocks=True, **kw)
    P1 = inference.dorefa_compile_codes(I, mfma_blocks=True, mfma_k3=True, **kw)
    lib = _lib.get_lib()
    k3 = [L for L in P1.layers if L.get("mfma3")]
    res = dict(model=args.arch, a_bits=2, w_bits=2, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), report=P1.report,
               mfma3_layers=[dict(name=L["name"], cin=L["cin"], cout=L["cout"], groups=L["groups"], span_words=int(L["table"][2]), dead_rows=int(L["table"][5])) for L in k3],
               batches={})
    with torch.no_grad():
        for bs in [int(v) for v in args.batches.split(",")]:
            x, _ = synth_batch(bs, device="cuda")
            ref, y0, y1 = I(x), P0(x), P1(x)
            equal = bool(torch.equal(ref, y0) and torch.equal(ref, y1))
            assert equal, "I, the mfma_blocks plan and the mfma_k3 plan must give bit-equal logits"
            for _ in range(args.warmup):
                I(x), P0(x), P1(x)
            ti, t0, t1 = [], [], []
            for _ in range(args.iters):          # alternated: all three see the same clocks and the same neighbours
                ti.append(timed(I, x))
                t0.append(timed(P0, x))
                t1.append(timed(P1, x))
            ki, k0, k1 = profile(lib, _lib, I, x), profile(lib, _lib, P0, x), profile(lib, _lib, P1, x)
            ms = lambda k, names: sum(v["ms"] for n, v in k.items() if n.startswith(names))
            mi, m0, m1 = statistics.median(ti), statistics.median(t0), statistics.median(t1)
            popc, mfma3 = ms(k0, ("k_codeconv<3,",)), ms(k1, ("k_codeconv_mfma3<",))
            byte = ms(ki, ("k_k3s_fwd", "k_kk<"))          # the byte path's 3x3 conv launches (its k_qa_fwd share comes on top: I_kernels holds every launch)
            res["batches"][str(bs)] = dict(I_ms=q(ti), P0_ms=q(t0), P1_ms=q(t1), P0_over_I=mi / m0, P1_over_I=mi / m1, P1_over_P0=m0 / m1, bit_equal=equal,
                                           layers_3x3_ms=dict(popcount=popc, mfma3=mfma3, popcount_left_in_P1=ms(k1, ("k_codeconv<3,",)), byte_path_conv=byte),
                                           I_kernels=ki, P0_kernels=k0, P1_kernels=k1)
            print("batch %d: I %.3f ms  mfma_blocks %.3f ms (%.2fx I)  mfma_blocks + mfma_k3 %.3f ms (%.2fx I, %.2fx mfma_blocks)  bit-equal %s"
                  % (bs, mi, m0, mi / m0, m1, mi / m1, m0 / m1, equal), flush=True)
            print("  3x3 layers: k_codeconv<3,*> %.3f ms  k_codeconv_mfma3 %.3f ms  byte path conv kernels %.3f ms" % (popc, mfma3, byte), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


def two_bit_check(parent_path, this_path):
    """P1 (mfma_blocks + mfma_k3, W2A2) of this tree against the parent commit's, both measured by --mfma-k3: per batch the two medians, the parent's p25-p75 width
    and whether this tree's median stays within the parent's median plus that width."""
    parent, this = json.load(open(parent_path)), json.load(open(this_path))
    out = dict(protocol="scripts/kbench_codes.py --mfma-k3 on the parent commit and on this tree, one after the other in one session", batches={})
    for bs, a in parent["batches"].items():
        b = this["batches"][bs]
        width = a["P1_ms"]["p75"] - a["P1_ms"]["p25"]
        out["batches"][bs] = dict(parent_P1_ms=a["P1_ms"], this_P1_ms=b["P1_ms"], parent_p25_p75_width_ms=width, parent_I_ms=a["I_ms"], this_I_ms=b["I_ms"],
                                  parent_P1_over_I=a["P1_over_I"], this_P1_over_I=b["P1_over_I"],
                                  within=bool(b["P1_ms"]["median"] <= a["P1_ms"]["median"] + width))
    out["within"] = all(v["within"] for v in out["batches"].values())
    return out


def main_w4(args):
    """nin_gc W4A4: I against its plan, alternated in one process."""
    from micronet.compression.quantization.wqaq.dorefa import quantize as Q
    from micronet_amd import _lib, inference
    from micronet_amd.train import build_model, synth_batch
    torch.manual_seed(0)
    I = Q.prepare(build_model("nin_gc"), inplace=True, a_bits=4, w_bits=4, quant_inference=True).cuda()
    inference.prequantize_weights(I)
    I.eval()
    P = inference.dorefa_compile_codes(I)
    lib = _lib.get_lib()
    # hidden activations per image, as the plan stores them (whole 32-channel words x 4 planes) and as the byte path does (one byte each)
    sizes = _map_sizes(P) + [_map_sizes(P)[-1] // 2 if P.layers[-1]["pool"] else _map_sizes(P)[-1]]
    chans = [P.layers[0]["cin"]] + [L["cout"] for L in P.layers]
    foot = dict(plan_bytes=sum(4 * P.bits * ((c + 31) // 32) * h * h for c, h in zip(chans, sizes)), byte_path_bytes=sum(c * h * h for c, h in zip(chans, sizes)))
    res = dict(model="nin_gc", a_bits=4, w_bits=4, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), report=P.report,
               mfma3_layers=[dict(name=L["name"], cin=L["cin"], cout=L["cout"], groups=L["groups"], span_words=int(L["table"][2]), dead_rows=int(L["table"][5]))
                             for L in P.layers if L.get("mfma3")],
               hidden_activation_bytes_per_image=foot, batches={})
    with torch.no_grad():
        for bs in [int(v) for v in args.batches.split(",")]:
            x, _ = synth_batch(bs, device="cuda")
            ref, got = I(x), P(x)
            equal = bool(torch.equal(ref, got))
            for _ in range(args.warmup):
                I(x), P(x)
            ti, tp = [], []
            for _ in range(args.iters):          # alternated: both see the same clocks and the same neighbours
                ti.append(timed(I, x))
                tp.append(timed(P, x))
            kp, ki = profile(lib, _lib, P, x), profile(lib, _lib, I, x)
            med_i, med_p = statistics.median(ti), statistics.median(tp)
            res["batches"][str(bs)] = dict(I_ms=q(ti), P_ms=q(tp), I_img_s=bs / med_i * 1e3, P_img_s=bs / med_p * 1e3, P_over_I=med_i / med_p, bit_equal=equal,
                                           P_kernels=kp, I_kernels=ki, P_kernel_ms_total=sum(v["ms"] for v in kp.values()),
                                           I_kernel_ms_total=sum(v["ms"] for v in ki.values()))
            print("batch %d: I %.3f ms (min %.3f)  P %.3f ms (min %.3f)  P/I speed %.2fx  bit-equal %s" % (bs, med_i, min(ti), med_p, min(tp), med_i / med_p, equal), flush=True)
    if args.two_bit_check:
        res["two_bit_check"] = two_bit_check(*args.two_bit_check)
        print("two_bit_check within:", res["two_bit_check"]["within"], flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


def _map_sizes(P, hw=32):
    """The input map size of every hidden block."""
    out, h = [], hw
    for L in P.layers:
        out.append(h)
        h = h // 2 if L["pool"] else h
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--code-ends", action="store_true", help="the default plan against dorefa_compile_codes(I, code_ends=True)")
    ap.add_argument("--mfma-blocks", action="store_true", help="I, the default plan and dorefa_compile_codes(I, mfma_blocks=True)")
    ap.add_argument("--mfma-k3", action="store_true", help="I, the mfma_blocks plan and dorefa_compile_codes(I, mfma_blocks=True, mfma_k3=True); works with --arch nin")
    ap.add_argument("--arch", default="nin_gc", choices=("nin_gc", "nin"), help="nin: plain nin, compiled with tile_blocks=True")
    ap.add_argument("--bits", type=int, default=2, choices=(2, 4), help="4: nin_gc W4A4, I against its plan (every other protocol is measured at 2 bits)")
    ap.add_argument("--two-bit-check", nargs=2, metavar=("PARENT_JSON", "THIS_JSON"), default=None,
                    help="with --bits 4: two --mfma-k3 results, of the parent commit and of this tree, recorded under two_bit_check")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.bits == 4:
        if args.code_ends or args.mfma_blocks or args.mfma_k3 or args.arch != "nin_gc":
            ap.error("--bits 4 is its own protocol, on nin_gc")
        if args.out is None:
            args.out = os.path.join("profiles", "codes_w4a4.json")
        return main_w4(args)
    if args.two_bit_check:
        ap.error("--two-bit-check goes with --bits 4")
    if (args.code_ends or args.mfma_blocks) and args.arch != "nin_gc":
        ap.error("--code-ends and --mfma-blocks are measured on nin_gc")
    if args.code_ends + args.mfma_blocks + args.mfma_k3 > 1:
        ap.error("--code-ends, --mfma-blocks and --mfma-k3 are three protocols: run them one at a time")
    if args.mfma_k3:
        if args.out is None:
            args.out = os.path.join("profiles", "codes_mfma3.json" if args.arch == "nin_gc" else "codes_mfma3_nin.json")
        return main_mfma_k3(args)
    if args.out is None:
        args.out = os.path.join("profiles", "codes_mfma.json" if args.mfma_blocks else "codes_ends.json" if args.code_ends else "codes_nin.json" if args.arch == "nin" else "codes_inference.json")
    if args.code_ends:
        return main_code_ends(args)
    if args.mfma_blocks:
        return main_mfma_blocks(args)
    from micronet.compression.quantization.wqaq.dorefa import quantize as Q
    from micronet_amd import _lib, inference
    from micronet_amd.train import build_model, synth_batch
    torch.manual_seed(0)
    I = Q.prepare(build_model(args.arch), inplace=True, a_bits=2, w_bits=2, quant_inference=True).cuda()
    inference.prequantize_weights(I)
    I.eval()
    P = inference.dorefa_compile_codes(I, tile_blocks=args.arch == "nin")
    lib = _lib.get_lib()
    rows = designed_bytes_per_image(P)
    res = dict(model=args.arch, a_bits=2, w_bits=2, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), report=P.report,
               designed_bytes_per_image=rows, designed_hidden_bytes_per_image=dict(codes=sum(r["codes_bytes"] for r in rows), byte_path=sum(r["byte_path_bytes"] for r in rows)),
               batches={})
    with torch.no_grad():
        for bs in [int(v) for v in args.batches.split(",")]:
            x, _ = synth_batch(bs, device="cuda")
            ref, got = I(x), P(x)
            err = float((ref - got).abs().max())
            for _ in range(args.warmup):
                I(x), P(x)
            ti, tp = [], []
            for _ in range(args.iters):          # alternated: both see the same clocks and the same neighbours
                ti.append(timed(I, x))
                tp.append(timed(P, x))
            kp, ki = profile(lib, _lib, P, x), profile(lib, _lib, I, x)
            med_i, med_p = statistics.median(ti), statistics.median(tp)
            res["batches"][str(bs)] = dict(I_ms=q(ti), P_ms=q(tp), I_img_s=bs / med_i * 1e3, P_img_s=bs / med_p * 1e3, P_over_I=med_i / med_p,
                                           max_abs_logit_diff=err, bit_equal=bool(torch.equal(ref, got)), P_kernels=kp, I_kernels=ki,
                                           P_kernel_ms_total=sum(v["ms"] for v in kp.values()), I_kernel_ms_total=sum(v["ms"] for v in ki.values()))
            print("batch %d: I %.3f ms (min %.3f)  P %.3f ms (min %.3f)  P/I speed %.2fx  max |dlogit| %.3g" % (bs, med_i, min(ti), med_p, min(tp), med_i / med_p, err), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
