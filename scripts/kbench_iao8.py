"""fp32-map path vs int8 path of a deployed (BN-folded, pre-quantised) IAO W8A8 nin_gc: the eval-mode folded model ``F`` (every hidden block re-quantises an fp32
map, contracts on the fp32-exact kernels and writes an fp32 map: the yardstick) and ``P = inference.iao_compile_int8(F)`` (one int8 code per hidden activation, one
i8-MFMA kernel per hidden block), alternated in ONE process, HIP events.

    python scripts/kbench_iao8.py [--batches 256,1024] [--warmup 5] [--iters 20] [--out profiles/iao8_inference.json]

Per batch: median / min / quartiles of the timed forwards of each, per-kernel times of both from the library's profile hooks, the largest |P - F| relative to
max|F| and the argmax agreement; and the designed HBM bytes per image per hidden block on both paths (arithmetic from the shapes).

    python scripts/kbench_iao8.py --byte-ends [...] [--out profiles/iao8_ends_inference.json]

adds ``E = inference.iao_compile_int8(F, byte_ends=True)`` (the first conv writes bytes, the classifier reads them) as a third path alternated with the two: its
yardstick is ``P`` in the same run (``E_over_P``), and its per-kernel times stand beside P's.

    python scripts/kbench_iao8.py --resnet18 [...] [--out profiles/iao8_resnet_inference.json]

runs the same comparison on a BN-folded IAO W8A8 resnet18: ``F`` writes and re-reads an fp32 map around every conv, ReLU and QuantAdd, ``P`` keeps byte codes from the
pack behind conv1 to the unpack in front of avg_pool (strided convs, shortcut convs and the QuantAdd on bytes: csrc/qgemm_iao8_res.h).

    python scripts/kbench_iao8.py --asym [...] [--out profiles/iao8_zp_inference.json]

prepares nin_gc with ``q_type=1`` (asymmetric quantizers) and compiles it with ``zero_points=True`` (csrc/qgemm_iao8_zp.h): ``F`` is that net's own eval-mode folded
model.  The symmetric net's plan is compiled in the same process as well and its kernels profiled once per batch (``S_kernels``), so that k_i8zconv stands beside
k_i8conv on the same geometry under the same clocks (``zconv_over_conv_us``).  That second net is trained and compiled for this comparison alone: neither its plan
nor its folded model is timed end to end (the symmetric P / F stands in profiles/iao8_inference.json).

    python scripts/kbench_iao8.py --resnet18 --end-to-end [...] [--out profiles/iao8_resnet_e2e_inference.json]

adds ``E = inference.iao_compile_int8(F, end_to_end=True)`` (csrc/qgemm_iao8_e2e.h: conv1 writes one code map per consumer, avg_pool + fc read the last codes) as a
third path alternated with F and the default plan P, which is its yardstick (``E_over_P``).  Per batch it also records, from the profile hooks in a forward of
each plan's own, ``k_i8first2<3,2>`` against conv1 + the two packs and the hidden stages inside both plans (``ends``: they are the same launches, so they must agree
within the run's spread), and -- avg_pool and fc have no profile hook -- the two heads and the two tails alone under HIP events, alternated (``ends_events``)."""
import argparse
import importlib
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
    return {buf[i].name.decode(): dict(launches=int(buf[i].launches), ms=float(buf[i].total_ms), us_per_launch=round(1e3 * float(buf[i].total_ms) / max(1, int(buf[i].launches)), 2),
                                       designed_bytes=float(buf[i].bytes)) for i in range(n)}


def designed_bytes_per_image(P):
    """Hidden blocks, per image.  fp32-map path (F): the conv reads an fp32 map (4 B per input element) and writes one (4 B per output element), the ReLU reads and
    writes it (8 B), a QuantMaxPool2d reads it and writes the pooled map (4 + 1 B per output element).  int8 path (P): one byte per input element, one per (pooled)
    output element, in whole 16-channel blocks (``act_bytes_in`` / ``act_bytes_out`` of the report)."""
    rows = []
    for r in P.report[1:-1]:
        n_in, n_out_pooled = r["act_bytes_in"], r["act_bytes_out"]
        n_out = n_out_pooled * (4 if r["pool"] else 1)
        fp32 = 4 * n_in + 4 * n_out + 8 * n_out + ((4 * n_out + 4 * n_out_pooled) if r["pool"] else 0)
        rows.append(dict(name=r["name"], kernel=r["kernel"], int8_bytes=n_in + n_out_pooled, fp32_path_bytes=fp32, table_bytes=r["table_bytes"]))
    return rows


def designed_bytes_per_image_resnet(P):
    """The stages of a ResNet plan, per image, arithmetic from the shapes.  fp32-map path (F): a conv reads an fp32 map and writes one (4 B per input and per output
    element), a ReLU reads and writes it (8 B per element); a QuantAdd reads the residual and the shortcut and writes the sum (12 B), the block's ReLU reads and
    writes it (8 B).  int8 path (P): ``act_bytes_in`` / ``act_bytes_out`` of the report (an add stage reads its input and the shortcut, and writes ``nout`` maps)."""
    rows = []
    for r in P.report[1:-1]:
        n_out = r["act_bytes_out"] // r["nout"]
        n_in = r["act_bytes_in"] - (n_out if r["kind"] == "int8_add" else 0)
        fp32 = 4 * n_in + 4 * n_out + (8 * n_out if r["relu"] else 0) + (20 * n_out if r["kind"] == "int8_add" else 0)
        rows.append(dict(name=r["name"], kernel=r["kernel"], int8_bytes=r["act_bytes_in"] + r["act_bytes_out"], fp32_path_bytes=fp32, table_bytes=r["table_bytes"]))
    return rows


def ends_from_profiles(kp, ke):
    """The two plans' profiled kernels split into the hidden stages (the same launches in both) and the rest: conv1 + the packs + the unpack of the default plan
    (its avg_pool and fc have no profile hook), k_i8first2 + k_i8poolfc of the end_to_end plan."""
    hidden = lambda k: sum(v["ms"] for n, v in k.items() if n.startswith(("k_i8conv<", "k_i8res_")))
    rest = lambda k: {n: v["ms"] for n, v in k.items() if not n.startswith(("k_i8conv<", "k_i8res_"))}
    first2 = sum(v for n, v in rest(ke).items() if n.startswith("k_i8first2"))
    return dict(P_hidden_ms=hidden(kp), E_hidden_ms=hidden(ke), P_ends_profiled=rest(kp), E_ends_profiled=rest(ke),
                P_conv1_and_packs_ms=sum(v for n, v in rest(kp).items() if "unpack" not in n), E_first2_ms=first2,
                P_unpack_ms=sum(v for n, v in rest(kp).items() if "unpack" in n), E_poolfc_ms=sum(v for n, v in rest(ke).items() if n.startswith("k_i8poolfc")))


def ends_events(P, E, x, warmup, iters):
    """The head (image -> the stem's code maps) and the tail (last codes -> logits) of both plans alone, alternated, under HIP events: the default plan's conv1 +
    packs and unpack + avg_pool + fc against mn_i8first_fwd2 and mn_i8poolfc_fwd.  Runs on the plans' own buffers, behind a forward of each."""
    from micronet_amd import ops
    N = x.shape[0]
    a = P.first(x).contiguous()
    pb, _, py = P._shape_buffers(a.shape, a.device)
    eb, _, (ey, hw) = E._shape_buffers(a.shape, a.device)
    st = ops._s()

    def p_head(xx):
        aa = P.first(xx).contiguous()
        for o in P.stem["outs"]:
            ops._call("mn_i8_pack_codes", ops._p(aa), N, aa.shape[1], aa.shape[2] * aa.shape[3], o["s"], o["bits"], None, ops._p(pb[o["buf"]]), st)

    def p_tail(_):
        n_, c_, h_, w_ = py.shape
        ops._call("mn_i8_unpack_codes", ops._p(pb[P.tail_q["buf"]]), n_, c_, h_ * w_, P.tail_q["s"], ops._p(py), st)
        y = P.tail[0](py)
        return P.tail[1](y.view(y.size(0), -1))

    e_head = lambda xx: E._first(xx, [eb[o["buf"]] for o in E.stem["outs"]], st)
    e_tail = lambda _: E._last(eb[E.tail_q["buf"]], N, hw, ey, st)
    fns = dict(P_head=p_head, E_head=e_head, P_tail=p_tail, E_tail=e_tail)
    for _ in range(warmup):
        for fn in fns.values():
            fn(x)
    t = {n: [] for n in fns}
    for _ in range(iters):
        for n, fn in fns.items():
            t[n].append(timed(fn, x))
    return {n: q(v) for n, v in t.items()}


def q(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), p25=statistics.quantiles(v, n=4)[0], p75=statistics.quantiles(v, n=4)[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--byte-ends", action="store_true", help="also time the byte_ends plan, against the default plan of the same run")
    ap.add_argument("--resnet18", action="store_true", help="the BN-folded IAO W8A8 resnet18 instead of nin_gc (no --byte-ends: not built for ResNets)")
    ap.add_argument("--out", default=None, help="default: profiles/iao8_inference.json, with --byte-ends profiles/iao8_ends_inference.json, with --resnet18 "
                                                "profiles/iao8_resnet_inference.json")
    ap.add_argument("--end-to-end", action="store_true", help="with --resnet18: also time the end_to_end plan, against the default plan of the same run")
    ap.add_argument("--asym", action="store_true", help="nin_gc prepared with q_type=1, compiled with zero_points=True (no --byte-ends, no --resnet18: not built)")
    args = ap.parse_args()
    if args.resnet18 and args.byte_ends:
        ap.error("--resnet18 and --byte-ends exclude each other")
    if args.asym and (args.resnet18 or args.byte_ends):
        ap.error("--asym excludes --resnet18 and --byte-ends")
    if args.end_to_end and not args.resnet18:
        ap.error("--end-to-end needs --resnet18 (nin_gc's form is --byte-ends)")
    args.out = args.out or os.path.join("profiles", "iao8_zp_inference.json" if args.asym else "iao8_resnet_e2e_inference.json" if args.end_to_end else
                                        "iao8_resnet_inference.json" if args.resnet18 else
                                        "iao8_ends_inference.json" if args.byte_ends else "iao8_inference.json")
    arch = "resnet18" if args.resnet18 else "nin_gc"
    from micronet_amd import _lib, inference
    from micronet_amd.train import build_model, make_optimizer, synth_batch, train_step
    Q = importlib.import_module("micronet.compression.quantization.wqaq.iao.quantize")

    def folded(q_type):
        # two training steps give the observers a range and the scales a meaning; then the fold and the pre-quantisation
        T = Q.prepare(build_model(arch), inplace=True, a_bits=8, w_bits=8, q_type=q_type, q_level=0, weight_observer=0, bn_fuse=True).cuda().train()
        opt = make_optimizer(T, 0.01, 1e-5)
        xt, yt = synth_batch(32, device="cuda")
        for _ in range(2):
            train_step(T, opt, xt, yt)
        T.eval()
        Fm = inference.iao_model_bn_fuse(T)
        if args.end_to_end:
            Fm.fc.quant_inference = True          # the classifier's stored weights go on the grid as well (k_i8poolfc contracts their codes)
        inference.prequantize_weights(Fm)
        return Fm.eval()

    F = folded(1 if args.asym else 0)
    P = inference.iao_compile_int8(F, zero_points=True) if args.asym else inference.iao_compile_int8(F)
    E = inference.iao_compile_int8(F, byte_ends=True) if args.byte_ends else inference.iao_compile_int8(F, end_to_end=True) if args.end_to_end else None
    S = inference.iao_compile_int8(folded(0)) if args.asym else None          # the symmetric plan: its kernels on the same geometries, under the same clocks
    lib = _lib.get_lib()
    res = dict(model=arch, a_bits=8, w_bits=8, warmup=args.warmup, iters=args.iters, device=torch.cuda.get_device_name(0), report=P.report,
               designed_bytes_per_image=(designed_bytes_per_image_resnet if args.resnet18 else designed_bytes_per_image)(P), batches={})
    if E is not None:
        res["ends_report"] = E.report
    if S is not None:
        res["q_type"] = 1
        res["zero_points"] = [dict(name=L["name"], z_a=L["z_a"], z_out=L["z_out"], z_p=L["z_p"], z_w_min=float(L["z_w"].min()), z_w_max=float(L["z_w"].max()))
                              for L in P.layers]
    with torch.no_grad():
        for bs in [int(v) for v in args.batches.split(",")]:
            x, _ = synth_batch(bs, device="cuda")
            f, p = F(x), P(x)
            e = E(x) if E is not None else None
            for _ in range(args.warmup):
                F(x), P(x)
                if E is not None:
                    E(x)
            tf, tp, te = [], [], []
            for _ in range(args.iters):          # alternated: both see the same clocks and the same neighbours
                tf.append(timed(F, x))
                tp.append(timed(P, x))
                if E is not None:
                    te.append(timed(E, x))
            kf, kp = profile(lib, _lib, F, x), profile(lib, _lib, P, x)
            mf, mp = statistics.median(tf), statistics.median(tp)
            res["batches"][str(bs)] = dict(F_ms=q(tf), P_ms=q(tp), F_img_s=bs / mf * 1e3, P_img_s=bs / mp * 1e3, P_over_F=mf / mp,
                                           max_abs_diff_over_max_F=float((p - f).abs().max() / f.abs().max()),
                                           argmax_agreement=float((p.argmax(1) == f.argmax(1)).float().mean()),
                                           F_kernel_ms_total=sum(v["ms"] for v in kf.values()), P_kernel_ms_total=sum(v["ms"] for v in kp.values()),
                                           F_kernels=kf, P_kernels=kp)
            print("batch %d: F %.3f ms (min %.3f)  P %.3f ms (min %.3f)  speed %.2fx  max|P-F|/max|F| %.2e" % (bs, mf, min(tf), mp, min(tp), mf / mp,
                                                                                                           res["batches"][str(bs)]["max_abs_diff_over_max_F"]), flush=True)
            print("  P kernels (us per launch):", {n: v["us_per_launch"] for n, v in kp.items()}, flush=True)
            if S is not None:
                for _ in range(args.warmup):
                    S(x)
                ks = profile(lib, _lib, S, x)
                pairs = {n: dict(zconv_us=v["us_per_launch"], conv_us=ks[n.replace("k_i8zconv", "k_i8conv")]["us_per_launch"],
                                 ratio=v["us_per_launch"] / ks[n.replace("k_i8zconv", "k_i8conv")]["us_per_launch"])
                         for n, v in kp.items() if n.startswith("k_i8zconv<") and n.replace("k_i8zconv", "k_i8conv") in ks}
                res["batches"][str(bs)].update(S_kernel_ms_total=sum(v["ms"] for v in ks.values()), S_kernels=ks, zconv_over_conv_us=pairs)
                print("  k_i8zconv against k_i8conv (us per launch, same geometry):", {n: (v["zconv_us"], v["conv_us"]) for n, v in pairs.items()}, flush=True)
            if E is not None:
                ke, me = profile(lib, _lib, E, x), statistics.median(te)
                res["batches"][str(bs)].update(E_ms=q(te), E_img_s=bs / me * 1e3, E_over_P=mp / me, E_over_F=mf / me,
                                               E_max_abs_diff_over_max_F=float((e - f).abs().max() / f.abs().max()),
                                               E_max_abs_diff_over_max_P=float((e - p).abs().max() / p.abs().max()),
                                               E_argmax_agreement=float((e.argmax(1) == f.argmax(1)).float().mean()),
                                               E_kernel_ms_total=sum(v["ms"] for v in ke.values()), E_kernels=ke)
                print("  %s: E %.3f ms (min %.3f, p25 %.3f, p75 %.3f)  against P %.2fx  max|E-F|/max|F| %.2e" % ("end_to_end" if args.end_to_end else "byte_ends", me, min(te), q(te)["p25"], q(te)["p75"], mp / me,
                                                                                                                    res["batches"][str(bs)]["E_max_abs_diff_over_max_F"]), flush=True)
                print("  E kernels (us per launch):", {n: v["us_per_launch"] for n, v in ke.items()}, flush=True)
                if args.end_to_end:
                    # the hidden stages are the same launches in both plans: five more profiled forwards of each, alternated, say how far one forward's sum moves
                    rounds = [(ends_from_profiles(profile(lib, _lib, P, x), profile(lib, _lib, E, x))) for _ in range(5)]
                    hidden = dict(P_hidden_ms=q([r_["P_hidden_ms"] for r_ in rounds]), E_hidden_ms=q([r_["E_hidden_ms"] for r_ in rounds]))
                    res["batches"][str(bs)].update(ends=ends_from_profiles(kp, ke), hidden_rounds=hidden, ends_events=ends_events(P, E, x, args.warmup, args.iters))
                    print("  hidden stages over five profiled forwards each (ms):", {n: (round(v["median"], 4), round(v["min"], 4), round(v["max"], 4)) for n, v in hidden.items()},
                          flush=True)
                    print("  ends (profile hooks, ms):", res["batches"][str(bs)]["ends"], flush=True)
                    print("  ends (HIP events, ms):", {n: round(v["median"], 4) for n, v in res["batches"][str(bs)]["ends_events"].items()}, flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump(res, f_, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
