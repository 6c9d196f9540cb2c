"""The compiled byte plan of a W8A8 ResNet (micronet_amd.inference.dorefa_compile_bytes -> Byte8ResPlan) on the MI355X: ResNet(BasicBlock, [2, 1, 1, 1]) -- an identity
block fed by the stem, an identity block fed by a block (bytes + fp32 out), stride-2 conv-shortcut blocks (bytes only out), a last block (fp32 only out) -- weights
from init_like_main under torch.manual_seed(1) on the CPU, BatchNorm parameters and statistics from a seeded CPU generator, no training, batch 2 at 32 x 32.  Every
kept stage equals the numpy judge of tests/code8_res_cases.py applied to the plan's own previous stage, bytes and fp32 bits alike.  tests/golden/code8_res_ref_logits.npy
holds the logits of the reference's own CPU eval forward (its ResNet, prepare and pre-quantisation loop) on this state dict and these images: recorded results only."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import code8_res_cases as R
from conftest import GOLDEN
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu


def seeded_net_and_images():
    """(the fp32 net on the CPU, two images): the recipe the golden logits were recorded from."""
    from micronet_amd.models import resnet
    from micronet_amd.train import init_like_main
    torch.manual_seed(1)
    net = init_like_main(resnet.ResNet(resnet.BasicBlock, [2, 1, 1, 1]))
    g = torch.Generator().manual_seed(2)
    draw = lambda n: torch.randn(n, generator=g)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            n = m.num_features
            m.weight.data, m.bias.data = draw(n) * 0.5 + 0.8, draw(n) * 0.5 + 0.5          # (both signs of gamma)
            m.running_mean.data, m.running_var.data = draw(n), torch.rand(n, generator=g) * 6 + 2
    return net, draw((2, 3, 32, 32))


@pytest.fixture(scope="module")
def net():
    """(the eval-mode quant_inference model, its plan, the images, the plan's logits, its kept byte maps as uint8 codes, its kept fp32 maps)."""
    from micronet_amd import inference
    Q = importlib.import_module("micronet.compression.quantization.wqaq.dorefa.quantize")
    fp32, x = seeded_net_and_images()
    I = Q.prepare(fp32, inplace=True, a_bits=8, w_bits=8, quant_inference=True).cuda().eval()
    assert inference.prequantize_weights(I) == 14
    plan = inference.dorefa_compile_bytes(I)
    plan.keep_stages = True
    x = x.cuda()
    with torch.no_grad():
        logits = plan(x).clone()
    return I, plan, x, logits, _host_stages(plan)


def _host_stages(plan):
    widths = [plan.layers[0]["cin"]] + [L["cout"] for L in plan.layers]
    side = lambda s: int(round(s.shape[2] ** 0.5))          # (maps are square here)
    codes = [None if s is None else R.from_map(s.cpu().numpy().view(np.uint8), c, side(s), side(s)) for s, c in zip(plan.stage_codes, widths)]
    return codes, [None if f is None else f.cpu().numpy() for f in plan.stage_f32]


def _acc(codes, w, L, stride=None):
    k = np.rint((w.cpu().numpy().astype(np.float64) * 255 + 255) / 2).astype(np.int64)
    acc = O.conv2d_fwd(codes.astype(np.int64), 2 * k - 255, None, stride=L["stride"] if stride is None else stride, padding=k.shape[2] // 2, acc=np.int64)
    assert np.abs(acc).max() < 2 ** 31
    return acc


def test_stages_equal_the_judge(net):
    _, plan, _, _, (codes, f32) = net
    assert np.array_equal(codes[0], R.codes_of(f32[0])), "the stem's bytes are the 8-bit codes of its fp32 map"
    for j, L in enumerate(plan.layers):          # stage j reads entry j and writes entry j + 1; a block's input is the entry in front of its conv stage
        z = R.chain_z(_acc(codes[j], L["w"], L), L["chan"].cpu().numpy())
        if L["kind"] == "add":
            r = f32[j - 1] if L["shortcut"] == "identity" else R.chain_z(_acc(codes[j - 1], L["w_s"], L, L["s_stride"]), L["chan_s"].cpu().numpy())
            z = (z + r).astype(np.float32)
        a = R.relu(z)
        assert [codes[j + 1] is not None, f32[j + 1] is not None] == ["bytes" in L["outputs"], "f32" in L["outputs"]], L["name"]
        if codes[j + 1] is not None:
            ref = R.codes_of(a)
            print(L["name"], L["kernel"], "byte mismatches", int((codes[j + 1] != ref).sum()), "of", ref.size, "distinct codes", len(np.unique(ref)))
            assert np.array_equal(codes[j + 1], ref), L["name"]
        if f32[j + 1] is not None:
            print(L["name"], L["kernel"], "fp32 bit mismatches", int((f32[j + 1].view(np.uint32) != a.view(np.uint32)).sum()), "of", a.size)
            assert np.array_equal(f32[j + 1].view(np.uint32), a.view(np.uint32)), L["name"]
    assert [(L["shortcut"], L["outputs"]) for L in plan.layers if L["kind"] == "add"] == [
        ("identity", ["bytes", "f32"]), ("identity", ["bytes"]), ("conv", ["bytes"]), ("conv", ["bytes"]), ("conv", ["f32"])]


def test_logits_and_single_images(net):
    I, plan, x, logits, (_, f32) = net
    with torch.no_grad():
        last = torch.from_numpy(f32[-1]).cuda()
        want = I.fc(I.avg_pool(last).view(2, -1))
        parts = torch.cat([plan(x[i:i + 1]).clone() for i in (0, 1)])
    assert logits.shape == (2, 10) and torch.equal(logits, want) and torch.equal(parts, logits)


def test_plan_against_fp32_forwards(net):
    """Two fp32 evaluations of the same function that do not promise the exact integer sum -- the reference's CPU forward (recorded) and the model's own eval forward --
    bound the plan: max|plan - ref| <= max(4 max|own - ref|, 1e-5 max|ref|) (the one-step code flips of DESIGN.md 4h through four stages; the float contract)."""
    I, _, x, logits, _ = net
    ref = np.load(os.path.join(GOLDEN, "code8_res_ref_logits.npy"))
    with torch.no_grad():
        own = I(x).cpu().numpy()
    d_plan, d_own, top = float(np.abs(logits.cpu().numpy() - ref).max()), float(np.abs(own - ref).max()), float(np.abs(ref).max())
    print("max|plan - ref| = %.3g, max|own - ref| = %.3g, max|ref| = %.3g" % (d_plan, d_own, top))
    assert ref.shape == (2, 10) and top > 0 and d_plan <= max(4 * d_own, 1e-5 * top)
