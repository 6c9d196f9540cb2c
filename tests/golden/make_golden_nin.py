"""Generate tests/golden/inference_nin.npz + inference_nin_meta.json: the plain ``nin`` net of the reference's WbWtAb scripts (wbwtab/main.py --model_type 0), trained
for a few steps, pre-quantised and BN-folded BY THE REFERENCE'S OWN CODE on the CPU.

    MICRONET_REFERENCE=<checkout of the reference> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nin.py

The reference is only imported and executed (its ``quantize.py``, ``models/nin.py`` and ``bn_fuse/bn_fuse.py``); the fixture holds arrays and names only:
  * ``<key>_fused_<name>``: the folded state_dict (weights = codes x alpha, BN gone; a few BN gammas were forced negative before the fold so that both of its
    branches occur),
  * ``x``: the input batch; ``<key>_logits``: the folded graph's logits,
  * per hidden stage ``<key>_stage<i>_bits`` (np.packbits of output == +1, shape in the meta), ``<key>_stage<i>_tie`` (np.packbits of |pre-activation| <= 1e-4 *
    max |pre-activation|: where a sign may legitimately differ by float rounding),
and the meta JSON records, per W, how many signs the byte-path folded graph of oracle/torch_oracle.py (CPU) gets different from the fixture, per stage.
"""
import argparse
import copy
import importlib.util
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = os.environ.get("MICRONET_REFERENCE")
if not REF:
    raise SystemExit("set MICRONET_REFERENCE to a checkout of the reference micronet package")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

import numpy as np
import torch
import torch.nn as nn

CFG = [32, 32, 32, 64, 64, 64, 64, 64]
BATCH, SEED, STEPS, TIE = 2, 1234, 3, 1e-4
torch.set_num_threads(8)


def _load_reference():
    """The reference's bn_fuse.py loaded the way it runs as a script (its `import quantize` / `from models import ...` resolve through its own directories)."""
    qdir = os.path.join(REF, "micronet", "compression", "quantization", "wbwtab")
    saved = list(sys.path)
    sys.path[:0] = [qdir, os.path.join(REF, "micronet")]
    try:
        spec = importlib.util.spec_from_file_location("ref_wbwtab_bn_fuse", os.path.join(qdir, "bn_fuse", "bn_fuse.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        import models.nin as ref_nin
    finally:
        sys.path[:] = saved
    return mod, ref_nin


def _init(model):
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.xavier_uniform_(m.weight)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
    return model


def _stages(model, x):
    """[(child name, pre-activation of a block or None, output)] of model.model, child by child."""
    out, t = [], x
    for name, st in model.model.named_children():
        pre = st.bn(st.conv(t)) if hasattr(st, "conv") else None
        t = st(t)
        out.append((name, pre, t))
    return out


def main():
    bnf, ref_nin = _load_reference()
    Q = bnf.quantize
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(BATCH, 3, 32, 32, generator=g)
    xt, yt = torch.randn(16, 3, 32, 32, generator=g), torch.randint(0, 10, (16,), generator=g)
    out, meta = {"x": x.numpy().copy()}, {"cfg": CFG, "batch": BATCH, "seed": SEED, "steps": STEPS, "tie": TIE}
    for W in (3, 2):
        key = "nin_w%d" % W
        torch.manual_seed(1)
        base = _init(ref_nin.Net(cfg=CFG))
        train = Q.prepare(copy.deepcopy(base), inplace=True, A=2, W=W)
        opt = torch.optim.Adam(train.parameters(), lr=0.01)
        train.train()
        for _ in range(STEPS):
            loss = nn.functional.cross_entropy(train(xt), yt)
            opt.zero_grad()
            loss.backward()
            opt.step()
        with torch.no_grad():          # gammas of both signs (the fold's second branch)
            for m in train.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.weight[1::5] *= -1
        inf = Q.prepare(copy.deepcopy(base), inplace=True, A=2, W=W, quant_inference=True)
        inf.load_state_dict(train.state_dict())
        with torch.no_grad():          # the stored weights of a quant_inference net ARE the quantised ones
            for m in inf.modules():
                if isinstance(m, Q.QuantConv2d):
                    m.weight.data = m.weight_quantizer(m.weight).detach().clone()
        bnf.args = argparse.Namespace(W=W, A=2)
        bnf.bn_counter = 0
        bnf.bin_bn_fuse_num = sum(isinstance(m, Q.ActivationQuantizer) for m in inf.modules())
        fused = bnf.model_bn_fuse(inf, inplace=False).eval()
        for k_, v in fused.state_dict().items():
            out["%s_fused_%s" % (key, k_)] = v.detach().numpy().copy()
        with torch.no_grad():
            st = _stages(fused, x)
            out[key + "_logits"] = fused(x).numpy().copy()
        stages = []
        for name, pre, t in st:
            vals = set(np.unique(t.numpy()).tolist())
            if not vals <= {-1.0, 1.0}:
                continue          # the last block (ReLU) and the average pool
            rec = dict(name=name, shape=list(t.shape), pooled=pre is None)
            out["%s_stage%s_bits" % (key, name)] = np.packbits(t.numpy().reshape(-1) > 0)
            if pre is not None:
                tie = pre.abs() <= TIE * pre.abs().max()
                out["%s_stage%s_tie" % (key, name)] = np.packbits(tie.numpy().reshape(-1))
                rec["ties"] = int(tie.sum())
            stages.append(rec)
        # ---- the byte-path folded graph of the CPU oracle against this fixture (recorded, and asserted to meet the cap the GPU test applies)
        sys.path.insert(0, ROOT)
        from oracle import torch_oracle as TO
        from micronet_amd.models import nin as our_nin
        orc = TO.prepare(our_nin.Net(cfg=CFG), "wbwtab", inplace=True, A=2, W=W)
        orc.load_state_dict(train.state_dict())
        with torch.no_grad():
            for m in orc.modules():
                if isinstance(m, TO.OConv2d) and m.scheme == "wbwtab":
                    m.weight.data = TO.wbwtab_weight(m.weight, W).detach().clone()
        of = TO.bn_fuse_wbwtab(orc, W).eval()
        with torch.no_grad():
            got = {name: t for name, _, t in _stages(of, x)}
            lg = of(x)
        for rec in stages:
            ref = np.unpackbits(out["%s_stage%s_bits" % (key, rec["name"])])[:int(np.prod(rec["shape"]))].reshape(rec["shape"])
            diff = (got[rec["name"]].numpy() > 0) != (ref > 0)
            rec["oracle_mismatches"] = int(diff.sum())
            assert diff.sum() <= 1e-4 * diff.size, (key, rec)
            if not rec["pooled"]:
                tie = np.unpackbits(out["%s_stage%s_tie" % (key, rec["name"])])[:diff.size].reshape(rec["shape"]).astype(bool)
                assert not (diff & ~tie).any(), (key, rec)
        ref_lg = out[key + "_logits"]
        meta[key] = dict(W=W, stages=stages, bin_bn_fuse_num=int(bnf.bin_bn_fuse_num),
                         negative_gammas=int(sum((m.weight < 0).sum() for m in train.modules() if isinstance(m, nn.BatchNorm2d))),
                         oracle_logits_rel=float(np.abs(lg.numpy() - ref_lg).max() / np.abs(ref_lg).max()),
                         convs=[(n_, type(m).__name__) for n_, m in fused.named_modules() if isinstance(m, nn.Conv2d)])
        print(key, [(r["name"], r["oracle_mismatches"], r.get("ties")) for r in stages], "logits rel", meta[key]["oracle_logits_rel"])
    np.savez_compressed(os.path.join(HERE, "inference_nin.npz"), **out)
    with open(os.path.join(HERE, "inference_nin_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote", os.path.getsize(os.path.join(HERE, "inference_nin.npz")), "bytes")


if __name__ == "__main__":
    main()
