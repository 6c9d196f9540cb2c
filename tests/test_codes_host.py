"""Host-only behaviour of micronet_amd.inference.dorefa_codes_report / dorefa_compile_codes: the stage report of nin_gc, and what the walk refuses, without a GPU."""
import json
import os

import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN


def _prepared(arch="nin_gc", bits=2, net=None):
    from micronet.compression.quantization.wqaq.dorefa import quantize as Q
    from micronet_amd.train import build_model
    torch.manual_seed(0)
    return Q.prepare(net if net is not None else build_model(arch), inplace=True, a_bits=bits, w_bits=bits, quant_inference=True).eval()


def test_codes_report_nin_gc_is_pinned():
    from micronet_amd import inference
    rep = inference.dorefa_codes_report(_prepared())
    want = json.load(open(os.path.join(GOLDEN, "codes_report_nin_gc.json")))
    assert rep == want
    assert [r["kind"] for r in rep] == ["first"] + ["code"] * 7 + ["last"]
    assert all(set(r) == {"name", "kind", "K", "words", "planes", "kernel", "pooled", "out_order", "stage"} for r in rep)


def test_codes_report_refuses_8_bit_activations():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=r"model\.1\.conv has a_bits = 8"):
        inference.dorefa_codes_report(_prepared(bits=8))


def test_codes_report_refuses_plain_nin_5x5():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=r"model\.\d+\.conv: geometry not covered by mn_codeconv_supported \(5x5"):
        inference.dorefa_codes_report(_prepared("nin"))


def test_codes_report_refuses_an_unfolded_pool_position():
    """A 2x2 max-pool directly behind the first block has no code block in front of it to fold into."""
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    from micronet_amd.models import nin_gc
    net = nin_gc.Net(cfg=[32, 32, 32, 64, 64, 64, 128, 128])
    kids = list(net.model.children())
    net.model = nn.Sequential(kids[0], nn.MaxPool2d(2, 2), *kids[1:])
    with pytest.raises(MicronetHipError, match=r"model\.0: a 2x2 max-pool is folded only into a code block"):
        inference.dorefa_codes_report(_prepared(net=net))
    # ... and two pools in a row: prepare() cannot hand the block's codes through both, so the block in front is refused
    net = nin_gc.Net(cfg=[32, 32, 32, 64, 64, 64, 128, 128])
    kids = list(net.model.children())
    net.model = nn.Sequential(*kids[:4], nn.MaxPool2d(2, 2), *kids[4:])
    with pytest.raises(MicronetHipError, match=r"model\.2: its output is not handed over as 2-bit codes"):
        inference.dorefa_codes_report(_prepared(net=net))


def test_compile_codes_names_the_first_layer_whose_weights_are_off_the_grid():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=r"model\.1\.conv: the stored weights were not found on the 2-bit grid"):
        inference.dorefa_compile_codes(_prepared())          # never pre-quantised


def test_code_plan_is_eval_only():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    first, layers, last, tail, flatten, report = inference._walk_codes(_prepared())
    plan = inference.CodePlan(first, layers, last, tail, flatten, report)
    assert not plan.training
    assert plan.train(False) is plan and plan.eval() is plan
    with pytest.raises(MicronetHipError, match="eval-only"):
        plan.train()
    with pytest.raises(MicronetHipError, match="eval-only"):
        plan.train(True)


def test_code_entry_points_are_declared_and_bound():
    from micronet_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "micronet_hip.h")).read()
    for name in ("mn_codes_pack_planes", "mn_codes_unpack_planes", "mn_codeconv_supported", "mn_codeconv_table_bytes", "mn_codeconv_pack", "mn_codeconv_fwd"):
        assert name in _lib.PROTOTYPES and (name + "(") in header
