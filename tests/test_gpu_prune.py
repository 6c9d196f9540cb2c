"""Channel pruning on the MI355X: the sparse-training Adam step (k_adam_l1) at kernel level (tests/prune_cases.py, the emulated run's cases), the optimizer's
device-side ``l1`` table under eager and captured steps, and the hand-over of pruned widths to QAT (prepare() on nin / nin_gc built from a pruned cfg)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import abi_driver
import prune_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


def test_adam_l1_matches_torch_with_updatebn(be):
    P.check_adam_l1(be)


def test_adam_l1_more_tensors_than_one_table(be):
    P.check_adam_l1_many(be)


def test_adam_l1_zero_is_the_plain_step_bit_for_bit(be):
    P.check_l1_zero_is_plain(be)


def test_adam_l1_rejects_bad_arguments(be):
    P.check_l1_rejects_bad_arguments(be)


# ------------------------------------------------------------------------------------------------ optimizer surface
def _run_schedule(capturable):
    """3 steps on raw tensors with per-group l1; one group's l1 is edited after step 2 -> (p, exp_avg, exp_avg_sq) of every tensor"""
    from micronet_amd.optim import Adam
    r = np.random.default_rng(5)
    sizes, l1s = (5, 2049, 33, 4099), (1e-3, 0.0, 1e-4, 1e-3)
    ps = [torch.nn.Parameter(torch.from_numpy(P.seeded_params(r, n)).cuda()) for n in sizes]
    opt = Adam([{"params": [p], "lr": 0.01 * (1 + i), "weight_decay": 1e-5 * (i % 2), "l1": l1s[i]} for i, p in enumerate(ps)], lr=0.01)
    opt.capturable = capturable
    for step in range(3):
        if step == 2:
            opt.param_groups[0]["l1"] = 5e-3
            opt.param_groups[1]["l1"] = 2e-4          # ... and one group leaves 0
            if capturable:
                opt.refresh_hyper()
        for p in ps:
            p.grad = torch.from_numpy((r.standard_normal(p.numel()) * 0.1).astype(np.float32)).cuda()
        opt.step()
    torch.cuda.synchronize()
    if capturable:
        opt.sync_steps()
    assert all(int(opt.state[p]["step"]) == 3 for p in ps)
    return [(p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy()) for p in ps], opt


def test_device_side_l1_follows_the_groups():
    """capturable Adam keeps l1 in device memory beside {lr, weight_decay}: the same schedule as the eager optimizer, bit for bit; a changed group count raises"""
    from micronet_amd._lib import MicronetHipError
    eager, _ = _run_schedule(False)
    dev, opt = _run_schedule(True)
    for e, d in zip(eager, dev):
        for a, b in zip(e, d):
            assert np.array_equal(a, b)
    assert [round(v, 7) for v in opt._l1_dev[next(iter(opt._l1_dev))].cpu().tolist()] == [5e-3, 2e-4, 1e-4, 1e-3]
    extra = torch.nn.Parameter(torch.zeros(4, device="cuda"))
    opt.add_param_group({"params": [extra]})
    with pytest.raises(MicronetHipError):
        opt.refresh_hyper()


def _float_nin(sparse_s):
    from micronet_amd.models import nin
    from micronet_amd.train import init_like_main, make_optimizer
    torch.manual_seed(3)
    m = init_like_main(nin.Net(cfg=[16] * 8)).cuda().train()
    return m, make_optimizer(m, 0.01, 1e-5, sparse_s=sparse_s)


def test_graphed_sparse_step_matches_eager():
    """GraphedTrainStep captures and replays the step with sparse_s > 0 (no new graph node: the L1 term is inside the Adam launch); every BatchNorm2d.weight
    follows the eager loop -- bounds of test_gpu_models.test_graphed_train_step_matches_eager for a net that is not chaotic"""
    from micronet_amd.train import GraphedTrainStep, synth_batch, train_step
    x, y = synth_batch(8, device="cuda")
    m1, o1 = _float_nin(1e-3)
    assert sum(g["l1"] == 1e-3 for g in o1.param_groups) == 9
    eager = [float(train_step(m1, o1, x, y)[0].detach()) for _ in range(4)]
    m2, o2 = _float_nin(1e-3)
    g = GraphedTrainStep(m2, o2, x, y, warmup=2)
    graphed = [float(g.step()[0]) for _ in range(2)]
    g.finish()
    print("eager", eager, "graphed", graphed)
    assert all(int(st["step"]) == 4 for st in o2.state.values())
    for a, b in zip(eager[2:], graphed):
        assert abs(a - b) <= 2e-2 * max(1.0, abs(a)), (eager, graphed)
    for (n_, a), (_, b) in zip(m1.named_modules(), m2.named_modules()):
        if isinstance(a, nn.BatchNorm2d):
            assert float((a.weight - b.weight).abs().max()) <= 0.3 * max(1.0, float(a.weight.abs().max())), n_


def test_sparse_step_issues_no_extra_optimizer_launch(monkeypatch):
    """one eager step with sparse_s > 0 goes through the library's optimizer entry points as often as with sparse_s = 0 (counted around lib.mn_adam_step*: the
    profiler hook does not cover the optimizer kernel), through the _l1 entry point only when asked for"""
    from micronet_amd import _lib
    from micronet_amd.train import synth_batch, train_step
    lib = _lib.get_lib()
    x, y = synth_batch(8, device="cuda")
    counts = {}
    for name in ("mn_adam_step", "mn_adam_step_dev", "mn_adam_step_l1", "mn_adam_step_l1_dev"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: (counts.__setitem__(_n, counts.get(_n, 0) + 1), _r(*a))[1])
    seen = {}
    for s in (0.0, 1e-3):
        m, o = _float_nin(s)
        counts.clear()
        train_step(m, o, x, y)
        seen[s] = dict(counts)
    torch.cuda.synchronize()
    assert seen[0.0] == {"mn_adam_step": 1} and seen[1e-3] == {"mn_adam_step_l1": 1}, seen


# ------------------------------------------------------------------------------------------------ prune -> QAT
def _pruned_nin_gc():
    from micronet_amd import pruning
    from micronet_amd.models import nin_gc
    # BatchNorms 2 and 5 feed the 3x3 convs of 16 and 32 groups and are 32 and 64 wide: cut to their base number (16, 32) they would leave ONE input channel
    # per group, and wbwtab centres every filter over its input channels -- all weights of such a conv are identically 0, in the reference as well, the loss is
    # ln 10, no gradient flows and there is nothing to compare (0 / 0).  A sparse-trained net keeps such layers; here their scales are the strong ones.
    cfg, _ = pruning.gc_prune_cfg(P.seeded_nin_gc(strong=(2, 5)), 0.4)
    assert cfg != P.NIN_GC_CFG and (cfg[2], cfg[5]) == (32, 64)
    net = nin_gc.Net(cfg=cfg)
    assert all(m.weight.shape[1] > 1 for m in net.modules() if isinstance(m, nn.Conv2d))
    return lambda: nin_gc.Net(cfg=cfg)


def _pruned_nin():
    from micronet_amd import pruning
    from micronet_amd.models import nin
    cfg, _ = pruning.regular_prune(P.seeded_nin(), 0.5, base_number=8)
    return lambda: nin.Net(cfg=cfg)


@pytest.mark.parametrize("arch", ["pruned_nin_gc", "pruned_nin"])
def test_pruned_widths_train_through_prepare(monkeypatch, arch):
    """prepare(Net(cfg=pruned), A=2, W=2): one forward + backward at batch 8 against oracle/torch_oracle.py -- whole net at the free-running wbwtab bounds of
    test_gpu_models.test_training_trajectory_smoke_vs_reference (loss 6e-2, logits 1.0: one sign flip cascades), then every layer teacher-forced by
    test_gpu_models.test_layerwise_teacher_forced itself (1e-5, its fp64 slack for the cancelling d weight)."""
    import test_gpu_models as M
    from micronet_amd import ops, train
    from micronet.compression.quantization.wbwtab import quantize
    from oracle import torch_oracle as TO
    ctor = {"pruned_nin_gc": _pruned_nin_gc, "pruned_nin": _pruned_nin}[arch]()
    real = train.build_model

    def build_model(a, seed=1):
        if a != arch:
            return real(a, seed)
        torch.manual_seed(seed)
        return train.init_like_main(ctor())
    monkeypatch.setattr(train, "build_model", build_model)
    print(arch, "cfg", [m.num_features for m in build_model(arch).modules() if isinstance(m, nn.BatchNorm2d)])
    prod = quantize.prepare(build_model(arch), inplace=True, A=2, W=2).cuda().train()
    orc = TO.prepare(build_model(arch), "wbwtab", inplace=True, A=2, W=2).train()
    x, y = train.synth_batch(8)
    ref_out = orc(x)
    ref_loss = torch.nn.functional.cross_entropy(ref_out, y)
    ops.fallback_counts(reset=True)
    opt = train.make_optimizer(prod, 0.01, 0.0)
    loss, out = train.train_step(prod, opt, x.cuda(), y.cuda())
    torch.cuda.synchronize()
    fb = ops.fallback_counts()
    print(arch, "fallback_counts", fb)
    assert isinstance(fb, dict)
    err = float((out.detach().cpu() - ref_out.detach()).abs().max() / ref_out.detach().abs().max().clamp_min(1e-6))
    print(arch, "loss", float(loss.detach()), "ref", float(ref_loss), "logits rel err", err)
    assert float(ref_out.detach().abs().max()) > 0.1                        # (the reference's net is alive: a dead one has logits ~ 1e-5 and zero gradients)
    assert abs(float(loss) - float(ref_loss)) <= 6e-2 and err <= 1.0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in prod.parameters())
    monkeypatch.setitem(M.CFG, arch, (arch, "wbwtab", dict(A=2, W=2), 8, 0.0))
    M.test_layerwise_teacher_forced(arch)
