"""The compiled byte plan of a W8A8 net (micronet_amd.inference.dorefa_compile_bytes) on the MI355X: W8A8 nin_gc and one narrow pruned-style cfg after two training
steps, batch 6 at 32 x 32.  Every hidden stage equals the judge of tests/codes_w8_cases.py applied to the previous stage's bytes, the logits are the model's own last
block on the unpacked codes, batch 6 equals its two chunks; against the model's own 8-bit eval forward -- which does not promise the exact integer accumulate -- at
most one code step on at most twice the share measured on the CPU."""
import importlib

import numpy as np
import pytest
import torch

import codes_w8_cases as W
import deploy_grid as DG

pytestmark = pytest.mark.gpu
CFGS = {"nin_gc": None, "narrow": [160, 224, 256, 448, 384, 512, 896, 768]}
ORACLE_SHARE = 6 / 8404992          # 6 of the 8404992 hidden codes of the CPU oracle's eval forward on these two nets differ from the judge chain, each by 1


def _stage_codes(plan):
    """The plan's kept stages as uint8 codes [N, C, H, W] on the host (maps are square here)."""
    from micronet_amd import inference
    widths = [plan.first.conv.out_channels] + [L["cout"] for L in plan.layers]
    side = lambda s: int(round(s.shape[2] ** 0.5))
    return [inference.unpack_code_map(s, c, side(s), side(s)).cpu().numpy() for s, c in zip(plan.stage_codes, widths)]


@pytest.fixture(scope="module", params=list(CFGS))
def net(request):
    """(the eval-mode quant_inference model, its plan, six images, the plan's logits, its kept stages)."""
    from micronet_amd import inference
    from micronet_amd.models import nin_gc
    from micronet_amd.train import init_like_main, make_optimizer, synth_batch, train_step
    Q = importlib.import_module("micronet.compression.quantization.wqaq.dorefa.quantize")

    def make(**kw):
        torch.manual_seed(1)
        return Q.prepare(init_like_main(nin_gc.Net(cfg=CFGS[request.param])), inplace=True, a_bits=8, w_bits=8, **kw).cuda()
    T = make().train()
    opt = make_optimizer(T, 0.01, 1e-5)
    x, y = synth_batch(32, device="cuda")
    for _ in range(2):
        train_step(T, opt, x, y)
    I = make(quant_inference=True)
    I.load_state_dict(T.state_dict())
    assert inference.prequantize_weights(I) == 8
    plan = inference.dorefa_compile_bytes(I.eval())
    plan.keep_stages = True
    with torch.no_grad():
        logits = plan(x[:6]).clone()
    return I, plan, x[:6], logits, _stage_codes(plan)


def test_stages_equal_the_judge(net):
    I, plan, _, _, stages = net
    convs = dict(I.named_modules())
    for i, L in enumerate(plan.layers):
        k = torch.round((convs[L["name"]].conv.weight.detach() * 255 + 255) / 2).cpu().numpy().astype(np.int64)
        # the stage's input is already in the consumer's (shuffled) channel order: the producer's rows were packed in that order
        acc = DG.exact_conv(stages[i].astype(np.int64), 2 * k - 255, L["pad"], L["groups"])
        assert np.abs(acc).max() < 2 ** 31
        ref = W.chain_codes(acc, L["chan"].cpu().numpy(), L["pool"])
        ref = ref[:, L["out_order"].cpu().numpy()] if L["out_order"] is not None else ref
        print(L["name"], "pool", L["pool"], "mismatches", int((stages[i + 1] != ref).sum()), "of", ref.size, "distinct codes", len(np.unique(ref)))
        assert np.array_equal(stages[i + 1], ref), L["name"]


def test_logits_and_chunks(net):
    """The logits are the model's own last block and tail on the unpacked codes; batch 6 equals its two chunks, logits and every stage."""
    from micronet_amd.sign_tensor import QActTensor
    _, plan, x, logits, stages = net
    c8 = torch.from_numpy(stages[-1]).cuda()
    with torch.no_grad():
        want = plan._finish(plan.last(QActTensor(c8, 8, lambda: c8.float() * (10.0 / 255.0))))
        parts = [(plan(x[a:a + 3]).clone(), _stage_codes(plan)) for a in (0, 3)]
    assert logits.shape == (6, 10) and torch.equal(logits, want)
    assert torch.equal(torch.cat([p[0] for p in parts]), logits)
    assert all(np.array_equal(np.concatenate([parts[0][1][i], parts[1][1][i]]), s) for i, s in enumerate(stages))


def test_plan_against_the_model_s_own_eval_forward(net):
    I, plan, x, _, stages = net
    mods, kept = dict(I.named_modules()), {}
    hooks = [mods[L["name"]].register_forward_hook(lambda m, a, out, n=L["name"]: kept.__setitem__(n, out.codes.clone())) for L in plan.layers]
    with torch.no_grad():
        I(x)
    for h in hooks:
        h.remove()
    differ = total = 0
    for i, L in enumerate(plan.layers):
        own = kept[L["name"]].cpu().numpy()
        own = own[:, L["out_order"].cpu().numpy()] if L["out_order"] is not None else own
        d = np.abs(own.astype(np.int32) - stages[i + 1].astype(np.int32))
        print(L["name"], "codes unlike the model's own", int((d != 0).sum()), "of", d.size, "largest", int(d.max()))
        assert own.shape == stages[i + 1].shape and d.max() <= 1, (L["name"], int(d.max()))
        differ, total = differ + int((d != 0).sum()), total + d.size
    print("share", differ / total, "bound", 2 * ORACLE_SHARE)
    assert differ / total <= 2 * ORACLE_SHARE
