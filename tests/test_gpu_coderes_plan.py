"""The compiled code plan of a W2A2 ResNet (micronet_amd.inference.dorefa_compile_codes -> CodeResPlan) on the MI355X: ResNet(BasicBlock, [2, 1, 1, 1]), the seeded
recipe, state dict and images of tests/test_gpu_code8_res_plan.py, prepared by default at a_bits = w_bits = 2 (fused blocks), batch 2 at 32 x 32.  Every kept stage equals
the numpy judge of tests/coderes_cases.py applied to the plan's own previous stage, plane words and fp32 bits alike.  tests/golden/coderes_ref_logits.npy holds the logits
of the reference's own CPU eval forward on this state dict and these images -- its ResNet, its prepare(a_bits=2, w_bits=2, quant_inference=True) and its
pre-quantisation loop (weight.data = weight_quantizer(weight)) over every quantised layer, the fc included, as prequantize_weights does: recorded results only."""
import importlib
import os

import numpy as np
import pytest
import torch

import coderes_cases as R
from codes_cases import np_unpack_planes
from conftest import GOLDEN
from oracle import np_oracle as O
from test_gpu_code8_res_plan import seeded_net_and_images

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net():
    """(the eval-mode quant_inference model, its plan, the images, the plan's logits, its kept plane maps as uint8 codes, its kept fp32 maps)."""
    from micronet_amd import inference
    Q = importlib.import_module("micronet.compression.quantization.wqaq.dorefa.quantize")
    fp32, x = seeded_net_and_images()
    I = Q.prepare(fp32, inplace=True, a_bits=2, w_bits=2, quant_inference=True).cuda().eval()
    assert inference.prequantize_weights(I) == 14 and type(I.conv2_x[0]).__name__ == "FusedBasicBlock"
    plan = inference.dorefa_compile_codes(I)
    plan.keep_stages = True
    x = x.cuda()
    with torch.no_grad():
        logits = plan(x).clone()
    widths = [plan.layers[0]["cin"]] + [L["cout"] for L in plan.layers]
    side = lambda s: int(round(s.shape[3] ** 0.5))          # (maps are square here)
    planes = lambda s: s.cpu().numpy().view(np.uint32).reshape(s.shape[:3] + (side(s), side(s)))
    codes = [None if s is None else np_unpack_planes(planes(s), c) for s, c in zip(plan.stage_codes, widths)]
    for s, c, w in zip(plan.stage_codes, codes, widths):          # word for word: the unused bits of the last word group are 0
        assert s is None or np.array_equal(planes(s), R.np_pack_planes(c)), w
    return I, plan, x, logits, (codes, [None if f is None else f.cpu().numpy() for f in plan.stage_f32])


def _acc(codes, w, stride):
    k = np.rint((w.cpu().numpy().astype(np.float64) * 3 + 3) / 2).astype(np.int64)
    acc = O.conv2d_fwd(codes.astype(np.int64), 2 * k - 3, None, stride=stride, padding=k.shape[2] // 2, acc=np.int64)
    assert np.abs(acc).max() < 2 ** 31
    return acc


def test_stages_equal_the_judge(net):
    _, plan, _, _, (codes, f32) = net
    assert type(plan).__name__ == "CodeResPlan"
    assert np.array_equal(codes[0], R.codes_of(f32[0])), "the stem's planes are the 2-bit codes of its fp32 map"
    for j, L in enumerate(plan.layers):          # stage j reads entry j and writes entry j + 1; a block's input is the entry in front of its conv stage
        z = R.chain_z(_acc(codes[j], L["w"], L["stride"]), L["chan"].cpu().numpy())
        if L["kind"] == "add":
            r = f32[j - 1] if L["shortcut"] == "identity" else R.chain_z(_acc(codes[j - 1], L["w_s"], L["s_stride"]), L["chan_s"].cpu().numpy())
            z = (z + r).astype(np.float32)
        a = R.relu(z)
        assert [codes[j + 1] is not None, f32[j + 1] is not None] == ["planes" in L["outputs"], "f32" in L["outputs"]], L["name"]
        if codes[j + 1] is not None:
            ref = R.codes_of(a)
            print(L["name"], L["kernel"], "code mismatches", int((codes[j + 1] != ref).sum()), "of", ref.size, "distinct codes", len(np.unique(ref)))
            assert np.array_equal(codes[j + 1], ref), L["name"]
        if f32[j + 1] is not None:
            print(L["name"], L["kernel"], "fp32 bit mismatches", int((f32[j + 1].view(np.uint32) != a.view(np.uint32)).sum()), "of", a.size)
            assert np.array_equal(f32[j + 1].view(np.uint32), a.view(np.uint32)), L["name"]
    assert [(L["shortcut"], L["outputs"]) for L in plan.layers if L["kind"] == "add"] == [
        ("identity", ["planes", "f32"]), ("identity", ["planes"]), ("conv", ["planes"]), ("conv", ["planes"]), ("conv", ["f32"])]


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
    ref = np.load(os.path.join(GOLDEN, "coderes_ref_logits.npy"))
    with torch.no_grad():
        own = I(x).cpu().numpy()
    d_plan, d_own, top = float(np.abs(logits.cpu().numpy() - ref).max()), float(np.abs(own - ref).max()), float(np.abs(ref).max())
    print("max|plan - ref| = %.3g, max|own - ref| = %.3g, max|ref| = %.3g" % (d_plan, d_own, top))
    assert ref.shape == (2, 10) and top > 0 and d_plan <= max(4 * d_own, 1e-5 * top)
