"""The compiled byte plan of PLAIN nin (``dorefa_compile_bytes(model, tile_blocks=True)``, with and without ``byte_ends``) on the MI355X: a narrow W8A8 nin after two
training steps, batch 6 at 32 x 32, held stage by stage to the judge of tests/codes_w8_cases.py and, in its logits, to a plain fp64 CPU forward."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

import codes_w8_cases as W
import deploy_grid as DG
from codes_nin_cases import np_codes_maxpool
from test_gpu_codes_w8_plan import _stage_codes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[False, True], ids=["default", "byte_ends"])
def net(request):
    """(the eval-mode quant_inference model, its plan, six images, the plan's logits, its kept stages)."""
    from micronet_amd import inference
    from micronet_amd.models import nin
    from micronet_amd.train import init_like_main, make_optimizer, synth_batch, train_step
    Q = importlib.import_module("micronet.compression.quantization.wqaq.dorefa.quantize")

    def make(**kw):
        torch.manual_seed(1)
        return Q.prepare(init_like_main(nin.Net(cfg=[32, 32, 16, 32, 32, 32, 32, 32])), inplace=True, a_bits=8, w_bits=8, **kw).cuda()
    T = make().train()
    opt = make_optimizer(T, 0.01, 1e-5)
    x, y = synth_batch(32, device="cuda")
    for _ in range(2):
        train_step(T, opt, x, y)
    I = make(quant_inference=True)
    I.load_state_dict(T.state_dict())
    assert inference.prequantize_weights(I) == 8
    plan = inference.dorefa_compile_bytes(I.eval(), byte_ends=request.param, tile_blocks=True)
    assert plan.report == inference.dorefa_bytes_report(I, byte_ends=request.param, tile_blocks=True)
    plan.keep_stages = True
    with torch.no_grad():
        logits = plan(x[:6]).clone()
    return I, plan, x[:6], logits, _stage_codes(plan)


def test_stages_equal_the_judge(net):
    I, plan, _, _, stages = net
    convs = dict(I.named_modules())
    assert [L["name"] for L in plan.layers if L["tile"]] == ["model.4"] and [L["pool_ksp"] for L in plan.layers if L["pool_ksp"]] == [(3, 2, 1)] * 2
    assert [s.shape[2] for s in stages] == [32, 32, 16, 16, 16, 8, 8, 8], "a pooled stage keeps its post-pool map"
    for i, L in enumerate(plan.layers):
        k = torch.round((convs[L["name"]].conv.weight.detach() * 255 + 255) / 2).cpu().numpy().astype(np.int64)
        acc = DG.exact_conv(stages[i].astype(np.int64), 2 * k - 255, L["pad"], L["groups"])
        assert np.abs(acc).max() < 2 ** 31
        ref = W.chain_codes(acc, L["chan"].cpu().numpy(), 0)
        ref = np_codes_maxpool(ref, *L["pool_ksp"]) if L["pool_ksp"] else ref
        print(L["name"], "tile", L["tile"], "pool", L["pool_ksp"], "mismatches", int((stages[i + 1] != ref).sum()), "of", ref.size, "distinct codes", len(np.unique(ref)))
        assert np.array_equal(stages[i + 1], ref), L["name"]


def test_logits_and_chunks(net):
    """The model's own last block on the unpacked codes, bit for bit (``byte_ends``: an exact sum against its fp32 accumulation, within 1e-5 max|logits|); two chunks."""
    from micronet_amd.sign_tensor import QActTensor
    _, plan, x, logits, stages = net
    c8 = torch.from_numpy(stages[-1]).cuda()
    with torch.no_grad():
        want = plan._finish(plan.last(QActTensor(c8, 8, lambda: c8.float() * (10.0 / 255.0))))
        parts = [(plan(x[a:a + 3].contiguous()).clone(), _stage_codes(plan)) for a in (0, 3)]
    assert logits.shape == (6, 10) and float((logits - want).abs().max()) <= (1e-5 * float(want.abs().max()) if plan.byte_ends else 0.0)
    assert torch.equal(torch.cat([p[0] for p in parts]), logits)
    assert all(np.array_equal(np.concatenate([parts[0][1][i], parts[1][1][i]]), s) for i, s in enumerate(stages))


def test_plan_against_fp64_forward(net):
    """max|plan - ref| <= max(4 max|own - ref|, 1e-5 max|ref|); ref: the net in double on the host (stored weights, eval BatchNorm, the 8-bit quantizer in front of
    every quantised conv); own: the model's own GPU eval forward.  On the MI355X: 3.86e-9 (byte_ends 5.33e-9), 3.86e-9 and max|ref| = 0.0501."""
    I, _, x, logits, _ = net
    d = lambda t: t.detach().double().cpu()
    a = d(x)
    for i, m in enumerate(I.model.children()):
        if isinstance(m, (nn.MaxPool2d, nn.AvgPool2d)):
            a = (TF.max_pool2d if isinstance(m, nn.MaxPool2d) else TF.avg_pool2d)(a, m.kernel_size, m.stride, m.padding)
            continue
        conv, bn, v = m.conv, m.bn, lambda t: d(t).view(1, -1, 1, 1)
        a = torch.floor(torch.clamp(a * 0.1, 0, 1) * 255 + 0.5) / 255 if i else a
        a = TF.conv2d(a, d(conv.weight), d(conv.bias) if conv.bias is not None else None, padding=conv.padding)
        a = torch.relu((a - v(bn.running_mean)) / torch.sqrt(v(bn.running_var) + bn.eps) * v(bn.weight) + v(bn.bias))
    ref = a.reshape(6, -1).numpy()
    with torch.no_grad():
        own = I(x).cpu().numpy()
    d_plan, d_own, top = float(np.abs(logits.cpu().numpy() - ref).max()), float(np.abs(own - ref).max()), float(np.abs(ref).max())
    print("max|plan - ref| = %.3g, max|own - ref| = %.3g, max|ref| = %.3g" % (d_plan, d_own, top))
    assert ref.shape == (6, 10) and top > 0 and d_plan <= max(4 * d_own, 1e-5 * top)
