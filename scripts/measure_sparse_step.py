#!/usr/bin/env python
"""Step time of sparse training: the float nin_gc step at batch 256 with ``sparse_s = 0`` against ``sparse_s = 1e-3``, alternated in one process
(5 warm-up + 20 timed steps each, HIP events around the whole step), and -- the baseline of the launch saving -- a stock ``torch.optim.Adam`` + ``updateBN()`` loop,
which is run on a checkout of the commit BEFORE the sparse step existed (``--tree``), in a process of its own.  Beside the times: the kernel launches of the
optimizer phase (from ``optimizer.zero_grad()``'s end to ``step()``'s end, updateBN included) of one extra, untimed step, counted by torch.profiler.

    python scripts/measure_sparse_step.py --variant fused --out profiles/prune_sparse_step.json
    python scripts/measure_sparse_step.py --variant stock --tree <checkout of the parent commit> --out profiles/prune_sparse_step.json

Each run merges its figures into ``--out``."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def update_bn(model, s):
    """pruning/main.py:65-69"""
    import torch
    import torch.nn as nn
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.weight.grad.data.add_(s * torch.sign(m.weight.data))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=("fused", "stock"), required=True)
    ap.add_argument("--tree", default=ROOT, help="the checkout micronet_amd is imported from")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--s", type=float, default=1e-3)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from micronet_amd import train
    x, y = train.synth_batch(args.batch, device="cuda")

    def setup(sparse_s, fused):
        model = train.build_model("nin_gc").cuda().train()
        if fused:
            return model, train.make_optimizer(model, 0.01, 1e-5, sparse_s=sparse_s), None
        return model, train.make_optimizer(model, 0.01, 1e-5, fused=False), sparse_s

    def step(model, opt, s, mark=None):
        """train.train_step with the reference's updateBN() between backward() and step() where the optimizer does not carry the term"""
        loss = train.cross_entropy(model(x), y)
        opt.zero_grad()
        loss.backward()
        if mark is not None:
            torch.cuda.synchronize()
            mark.__enter__()
        if s:
            update_bn(model, s)
        opt.step()
        if mark is not None:
            torch.cuda.synchronize()
            mark.__exit__(None, None, None)
        return loss

    runs = {"fused": [("plain_ms", setup(0.0, True)), ("sparse_ms", setup(args.s, True))], "stock": [("stock_updatebn_ms", setup(args.s, False))]}[args.variant]
    times = {k: [] for k, _ in runs}
    for i in range(args.warmup + args.steps):
        for k, (model, opt, s) in runs:                  # alternated: both variants see the same clocks and cache state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(model, opt, s)
            e1.record()
            e1.synchronize()
            if i >= args.warmup:
                times[k].append(e0.elapsed_time(e1))
    res = {}
    for k, (model, opt, s) in runs:
        t = times[k]
        res[k] = {"median": statistics.median(t), "min": min(t), "max": max(t), "steps": len(t)}
        try:
            prof = torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA])
            step(model, opt, s, mark=prof)
            kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
            res[k]["optimizer_phase_launches"] = len(kernels)
            res[k]["optimizer_phase_kernels"] = sorted({e.name.split("(")[0][:60] for e in kernels})[:12]
        except Exception as e:                          # the times above stand without the count
            res[k]["optimizer_phase_launches"] = None
            res[k]["optimizer_phase_error"] = repr(e)[:200]
        print(k, json.dumps(res[k]), flush=True)
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    out.setdefault("workload", "float nin_gc train step, batch %d, lr 0.01, weight_decay 1e-5, s %g; HIP events around the whole step, %d warm-up + %d timed, "
                               "plain / sparse alternated in one process, stock in its own" % (args.batch, args.s, args.warmup, args.steps))
    out["device"] = torch.cuda.get_device_name(0)
    out.update(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
