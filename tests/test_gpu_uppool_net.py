"""Whole nin_gc step under wbwtab: the two pooled pointwise blocks (layers 3 and 6) get the sums of their BatchNorm backward from the grouped 3x3 block behind
the pool (ops.UpSums kind 4: mn_conv2d_bwd_data_bnh_uppool + mn_bnh_bwd_sums_finish_pool) instead of mn_bnh_bwd_sums' pass over (pooled gradient, own codes, stash)."""
import copy
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu


def _step(monkeypatch, base, x, y, on, hook=False):
    from micronet_amd import ops
    real = ops._call
    n = {"own": 0}

    def counted(name, *a):
        n[name] = n.get(name, 0) + 1
        if name == "mn_bnh_bwd_sums" and a[2] is not None:          # a pass with the block's own codes: the pooled form
            n["own"] += 1
        return real(name, *a)
    monkeypatch.setattr(ops, "UP_SUMS_FOLD", on)
    monkeypatch.setattr(ops, "_call", counted)
    m = copy.deepcopy(base)
    hooks = []
    if hook:          # a backward hook on the pooled activation: what reaches the pool's backward is no longer the 3x3 block's dx tensor itself
        for mod in m.modules():
            if isinstance(mod, torch.nn.MaxPool2d):
                hooks.append(mod.register_forward_hook(lambda mod_, inp, out: out.register_hook(lambda g_: g_ * 1.0) and None))
        assert len(hooks) == 2
    ops.fallback_counts(reset=True)
    try:
        ops.cross_entropy(m(x), y).backward()
    finally:
        for h_ in hooks:
            h_.remove()
        monkeypatch.setattr(ops, "_call", real)
    assert ops.fallback_counts() == {}, ops.fallback_counts()
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}, n


def _assert_close(res_on, res_off):
    gscale = max(float(g.abs().max()) for g in res_off.values())
    for k, g0 in res_off.items():
        g1 = res_on[k]
        assert torch.isfinite(g1).all()
        assert float((g1 - g0).abs().max()) <= 2e-5 * float(g0.abs().max()) + 1e-6 * gscale, (k, float((g1 - g0).abs().max()), float(g0.abs().max()))


@pytest.fixture(scope="module", params=[3, 2], ids=["W3", "W2"])
def net(request):
    from micronet_amd.train import build_model, synth_batch
    quantize = importlib.import_module("micronet.compression.quantization.wbwtab.quantize")
    torch.manual_seed(11)
    base = quantize.prepare(build_model("nin_gc"), inplace=True, A=2, W=request.param).cuda().train()
    x, y = synth_batch(32, device="cuda")
    return base, x, y


def test_pooled_blocks_sums_ride_on_the_3x3_backward(monkeypatch, net):
    base, x, y = net
    res_on, n_on = _step(monkeypatch, base, x, y, True)
    res_off, n_off = _step(monkeypatch, base, x, y, False)
    assert n_on.get("mn_conv2d_bwd_data_bnh_uppool", 0) == 2 and n_on.get("mn_bnh_bwd_sums_finish_pool", 0) == 2, n_on
    assert n_on["own"] == 0, n_on
    assert n_off.get("mn_conv2d_bwd_data_bnh_uppool", 0) == 0 and n_off.get("mn_bnh_bwd_sums_finish_pool", 0) == 0 and n_off["own"] == 2, n_off
    _assert_close(res_on, res_off)


def test_a_hook_on_the_pooled_activation_takes_the_ordinary_pass(monkeypatch, net):
    base, x, y = net
    res_hook, n_hook = _step(monkeypatch, base, x, y, True, hook=True)
    res_off, _ = _step(monkeypatch, base, x, y, False)
    # the 3x3 blocks still leave their partials, but the gradient that reaches the pooled blocks is another tensor: identity fails, mn_bnh_bwd_sums runs
    assert n_hook.get("mn_bnh_bwd_sums_finish_pool", 0) == 0 and n_hook["own"] == 2, n_hook
    _assert_close(res_hook, res_off)
