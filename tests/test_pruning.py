"""micronet_amd.pruning on the CPU: the selection arithmetic of normal_regular_prune.py / gc_prune.py against an independent sort-based evaluation, the
compaction of a dense net (the pruned net computes the pre-pruned net's function), the checkpoint round trip, and the optimizer surface of sparse training
(which groups get ``l1``) as far as it needs no GPU."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import prune_cases as P
from micronet_amd import pruning
from micronet_amd._lib import MicronetHipError
from micronet_amd.models import nin, nin_gc


def _gammas(model, layers=9):
    return [m.weight.detach().clone().numpy() for m in model.modules() if isinstance(m, nn.BatchNorm2d)][:layers - 1]


def _expected(gammas, percent, bases, fill_small=False):
    """The rules of the pruning module's section of the design, evaluated with numpy: top-k by a sort of each layer instead of a second threshold."""
    allabs = np.sort(np.concatenate([np.abs(g) for g in gammas]))
    thre = allabs[min(int(allabs.size * percent), allabs.size - 1)]
    cfg, masks = [], []
    for g, base in zip(gammas, bases):
        a = np.abs(g)
        keep = a > thre
        cnt = int(keep.sum())
        if cnt == 0:
            cnt, keep = 1, np.arange(g.size) == int(np.argmax(g))
        if cnt % base != 0 and (cnt > base or fill_small):
            lo = cnt // base * base
            if cnt < base:          # gc_prune_cfg only: a grouped layer cannot be narrower than its base number
                cnt = base
            else:
                cnt = min(lo if cnt - lo < lo + base - cnt else lo + base, g.size)
            keep = np.zeros(g.size, dtype=bool)
            keep[np.argsort(-a, kind="stable")[:cnt]] = True
        cfg.append(cnt)
        masks.append(keep)
    return cfg, masks


def test_import_exports():
    import micronet_amd
    assert micronet_amd.regular_prune is pruning.regular_prune and micronet_amd.compact is pruning.compact
    assert micronet_amd.gc_prune_cfg is pruning.gc_prune_cfg and micronet_amd.bn_threshold is pruning.bn_threshold


@pytest.mark.parametrize("base", [1, 4, 8])
@pytest.mark.parametrize("percent", [0.0, 0.3, 0.5, 0.99])
def test_regular_prune_matches_sort_based_evaluation(percent, base):
    model = P.seeded_nin()
    gam = _gammas(model)
    flat = np.abs(np.concatenate(gam))
    assert np.unique(flat).size == flat.size          # pairwise-distinct |gamma|: no tie anywhere
    betas = [m.bias.detach().clone() for m in model.modules() if isinstance(m, nn.BatchNorm2d)]
    thre = pruning.bn_threshold(model, percent, 9)
    assert float(thre) == np.sort(flat)[min(int(flat.size * percent), flat.size - 1)]
    cfg, masks = pruning.regular_prune(model, percent, base_number=base, layers=9)
    ecfg, emasks = _expected(gam, percent, [base] * 8)
    assert cfg == ecfg and len(masks) == 8
    for m, e in zip(masks, emasks):
        assert m.dtype == torch.bool and np.array_equal(m.numpy(), e)
    assert all(c == int(m.sum()) and (c % base == 0 or c <= base or c == m.numel()) for c, m in zip(cfg, masks))
    # the model is now the pre-pruned one: gamma and beta of pruned channels are 0, kept ones untouched; the ninth BatchNorm is left alone
    bns = [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)]
    for bn, g0, b0, e in zip(bns, gam, betas, emasks):
        et = torch.from_numpy(e)
        assert torch.equal(bn.weight.detach(), torch.from_numpy(g0) * et) and torch.equal(bn.bias.detach(), b0 * et)
    assert torch.equal(bns[8].bias.detach(), betas[8]) and float(bns[8].weight.detach().abs().min()) > 0
    nin.Net(cfg=cfg)(torch.zeros(1, 3, 32, 32))


def test_emptied_layer_keeps_one_channel():
    model = P.seeded_nin()
    bns = [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        bns[2].weight.copy_(-(torch.arange(16).float() + 1.0) * 1e-6)          # every scale of layer 2 under the threshold; arg-max of gamma = channel 0
    gam = _gammas(model)
    cfg, masks = pruning.regular_prune(model, 0.3, base_number=4)
    ecfg, emasks = _expected(gam, 0.3, [4] * 8)
    assert cfg == ecfg and cfg[2] == 1
    assert masks[2].nonzero().reshape(-1).tolist() == [0]
    nin.Net(cfg=cfg)(torch.zeros(1, 3, 32, 32))


def test_tie_at_the_cut_raises_and_names_the_layer():
    model = P.seeded_nin()
    bns = [(n, m) for n, m in model.named_modules() if isinstance(m, nn.BatchNorm2d)]
    name, bn = bns[4]
    with torch.no_grad():                              # 32 channels: 13 clearly kept, then FIVE tied at 0.75, the rest pruned
        g = torch.full((32,), 1e-4) + torch.arange(32).float() * 1e-7
        g[:13] = 2.0 + torch.arange(13).float()
        g[13:18] = 0.75
        bn.weight.copy_(g)
    thre = float(pruning.bn_threshold(model, 0.5, 9))
    assert 1e-3 < thre < 0.75                          # 18 channels pass the global threshold; base 8 rounds them to 16: the cut falls inside the tie
    before = [m.weight.detach().clone() for _, m in bns]
    with pytest.raises(MicronetHipError) as ei:
        pruning.regular_prune(model, 0.5, base_number=8)
    assert name in str(ei.value) and "0.75" in str(ei.value)
    assert all(torch.equal(m.weight.detach(), b) for (_, m), b in zip(bns, before))          # nothing was pruned


def test_gc_prune_cfg_base_numbers_and_buildable_cfg():
    model = P.seeded_nin_gc()
    gam = _gammas(model)
    flat = np.abs(np.concatenate(gam))
    assert np.unique(flat).size == flat.size
    # groups seen from the conv shapes: [1, 2, 2, 16, 4, 4, 32, 8, 1] -> smallest count divisible by both neighbours
    bases = [2, 2, 16, 16, 4, 32, 32, 8]
    convs = [m for m in model.modules() if isinstance(m, nn.Conv2d)]
    assert [1] + [convs[j].out_channels // convs[j + 1].weight.shape[1] for j in range(8)] == [1, 2, 2, 16, 4, 4, 32, 8, 1]
    for percent in (0.0, 0.4, 0.7):
        model = P.seeded_nin_gc()
        cfg, masks = pruning.gc_prune_cfg(model, percent)
        ecfg, emasks = _expected(gam, percent, bases, fill_small=True)
        assert cfg == ecfg, (percent, cfg, ecfg)
        for m, e in zip(masks, emasks):
            assert np.array_equal(m.numpy(), e)
        for c, b, w in zip(cfg, bases, P.NIN_GC_CFG):
            assert c % b == 0 and 0 < c <= w, (percent, cfg)
        out = nin_gc.Net(cfg=cfg)(torch.randn(2, 3, 32, 32))
        assert out.shape == (2, 10) and torch.isfinite(out).all()
    assert cfg != P.NIN_GC_CFG


def test_compact_preserves_the_function_and_round_trips(tmp_path):
    from micronet_amd import data
    model = P.seeded_nin()
    g = torch.Generator().manual_seed(11)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    cfg, masks = pruning.regular_prune(model, 0.5)
    assert sum(cfg) < sum(P.NIN_CFG) and min(cfg) >= 1
    small = pruning.compact(model, masks, nin.Net(cfg=cfg))
    assert [tuple(m.weight.shape) for m in small.modules() if isinstance(m, nn.Conv2d)][:3] == [(cfg[0], 3, 5, 5), (cfg[1], cfg[0], 1, 1), (cfg[2], cfg[1], 1, 1)]
    x = torch.randn(4, 3, 32, 32, generator=g, dtype=torch.float64)
    model.double().eval(), small.double().eval()
    with torch.no_grad():
        ref, got = model(x), small(x)
    assert float(ref.abs().max()) > 0
    # pruned channels have gamma = beta = 0: exactly 0 behind the ReLU, so only the order of summation differs
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    path = str(tmp_path / "nin_prune.pth")
    data.save_state(small, 12.5, path, cfg=cfg)
    ckpt = torch.load(path, map_location="cpu")
    assert ckpt["cfg"] == cfg and ckpt["best_acc"] == 12.5
    again = nin.Net(cfg=ckpt["cfg"]).double().eval()
    again.load_state_dict(ckpt["state_dict"])
    with torch.no_grad():
        assert torch.equal(again(x), got)


def test_compact_rejects_grouped_convs_and_wrong_widths():
    model = P.seeded_nin_gc()
    cfg, masks = pruning.gc_prune_cfg(model, 0.4)
    with pytest.raises(MicronetHipError, match="grouped"):
        pruning.compact(model, masks, nin_gc.Net(cfg=cfg))
    model = P.seeded_nin()
    cfg, masks = pruning.regular_prune(model, 0.5)
    wrong = list(cfg)
    wrong[3] += 1
    with pytest.raises(MicronetHipError, match="model.4"):
        pruning.compact(model, masks, nin.Net(cfg=wrong))


def test_sparse_optimizer_surface_without_gpu():
    """make_optimizer(sparse_s=) puts l1 on EVERY BatchNorm2d.weight (updateBN touches all of them, not only the pruned range) and nowhere else."""
    from micronet_amd.optim import Adam
    from micronet_amd.train import make_optimizer
    model = nin.Net(cfg=P.NIN_CFG)
    opt = make_optimizer(model, 0.01, 1e-5, fused=True, sparse_s=1e-4)
    gammas = {id(m.weight) for m in model.modules() if isinstance(m, nn.BatchNorm2d)}
    assert len(gammas) == 9
    for g in opt.param_groups:
        assert g["l1"] == (1e-4 if id(g["params"][0]) in gammas else 0.0)
    assert all(g["l1"] == 0.0 for g in make_optimizer(model, 0.01, 1e-5, fused=True).param_groups)
    with pytest.raises(ValueError):
        make_optimizer(model, 0.01, 1e-5, fused=False, sparse_s=1e-4)          # torch.optim.Adam has no such key: keep updateBN() there
    with pytest.raises(ValueError):
        make_optimizer(model, 0.01, 1e-5, fused=True, sparse_s=-1e-4)
    with pytest.raises(ValueError):
        Adam([{"params": [torch.nn.Parameter(torch.zeros(3))], "l1": float("nan")}])
