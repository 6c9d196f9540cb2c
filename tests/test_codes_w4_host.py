"""Host-only behaviour of ``dorefa_codes_report`` / the walk of ``dorefa_compile_codes`` on W4A4 nets: the stage report of nin_gc at 4 bits, what a 4-bit net refuses
(it runs on the two int8-MFMA blocks or not at all), and that nothing moves for a 2-bit net -- without a GPU."""
import inspect
import json
import os

import pytest
import torch.nn as nn

from conftest import GOLDEN
from test_codes_host import _prepared

NAMES = {"name", "kind", "K", "words", "planes", "kernel", "pooled", "out_order", "stage"}
FLAGS = [dict(), dict(mfma_blocks=True), dict(mfma_k3=True), dict(mfma_blocks=True, mfma_k3=True)]


def _golden(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def _refused(model, pattern, **kw):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=pattern):
        inference.dorefa_codes_report(model, **kw)


@pytest.mark.parametrize("flags", FLAGS, ids=["none", "mfma_blocks", "mfma_k3", "both"])
def test_codes_w4a4_report_nin_gc_is_pinned(flags):
    from micronet_amd import inference
    rep = inference.dorefa_codes_report(_prepared(bits=4), **flags)
    assert rep == _golden("codes_w4a4_report_nin_gc.json")
    assert [r["kind"] for r in rep] == ["first"] + ["code"] * 7 + ["last"] and all(set(r) == NAMES for r in rep)
    assert all(r["planes"] == 4 for r in rep[1:]) and rep[0]["planes"] == 0
    kernels = [r["kernel"] for r in rep[1:-1]]
    assert (kernels.count("k_codeconv_mfma<0>"), kernels.count("k_codeconv_mfma<1>"), kernels.count("k_codeconv_mfma3<0>")) == (3, 2, 2), kernels
    # the 2-bit report with both flags on differs in the planes alone
    two = _golden("codes_mfma3_report_nin_gc.json")
    assert [dict(r, planes=0) for r in rep] == [dict(r, planes=0) for r in two]


@pytest.mark.parametrize("flags", FLAGS, ids=["none", "mfma_blocks", "mfma_k3", "both"])
def test_w4a4_layers_carry_both_keys(flags):
    from micronet_amd import inference
    layers = inference._walk_codes(_prepared(bits=4), **flags)[1]
    assert [L["mfma"] for L in layers] == [L["k"] == 1 for L in layers] and [L["mfma3"] for L in layers] == [L["k"] == 3 for L in layers]


def test_w4a4_refuses_code_ends_and_tile_blocks():
    _refused(_prepared(bits=4), r"code_ends=True\): model\.0\.conv: the net has 4-bit codes; .* built for 2 bits only", code_ends=True)
    _refused(_prepared(bits=4), r"tile_blocks=True\): model\.1\.conv: the net has 4-bit codes; .* built for 2 bits only", tile_blocks=True)
    _refused(_prepared("nin", bits=4), r"tile_blocks=True\): model\.1\.conv: the net has 4-bit codes", tile_blocks=True)


def test_w4a4_refuses_plain_nin():
    """Its first hidden block already has 192 taps per output, beyond K * 225 <= 32767; a dense 5x5 block has no 4-bit form at any width."""
    from micronet_amd.models.nin_gc import ConvBNReLU
    _refused(_prepared("nin", bits=4), r"model\.1\.conv: not covered by the 4-bit int8-MFMA blocks .*192 taps per output: beyond K \* 15 \* 15 <= 32767")
    net = nn.Sequential(ConvBNReLU(3, 32, 5, padding=2), ConvBNReLU(32, 32, 5, padding=2), ConvBNReLU(32, 10, 1))
    _refused(_prepared(net=net, bits=4), r": 1\.conv: not covered by the 4-bit int8-MFMA blocks .*5x5, padding 2: only the 1x1 and the 3x3 / padding 1 block")


def test_w4a4_refuses_narrow_groups():
    from micronet_amd.models import nin_gc
    # 16 channels per group in the grouped 1x1 blocks (and 2 in the 3x3 blocks): the walk names the first
    _refused(_prepared(net=nin_gc.Net(cfg=[32, 32, 32, 64, 64, 64, 128, 128]), bits=4),
             r"model\.1\.conv: not covered by the 4-bit int8-MFMA blocks .*16 channels per group: a grouped 1x1 block needs whole input words per group")
    # 64 per group in the 1x1 blocks, 8 in the 3x3 blocks
    _refused(_prepared(net=nin_gc.Net(cfg=[128, 128, 128, 256, 256, 256, 512, 512]), bits=4),
             r"model\.4\.conv: not covered by the 4-bit int8-MFMA blocks .*8 channels per group: the 3x3 MFMA form covers C / groups == 16 at 4 bits")


def test_w4a4_refuses_a_pooled_3x3_block():
    from micronet_amd.models.nin_gc import ConvBNReLU
    net = nn.Sequential(ConvBNReLU(3, 32, 5, padding=2), ConvBNReLU(32, 32, 3, padding=1, groups=2), nn.MaxPool2d(2, 2), ConvBNReLU(32, 64, 1),
                        ConvBNReLU(64, 10, 1))
    _refused(_prepared(net=net, bits=4), r": 1\.conv: a 3x3 block with a folded 2x2 max-pool is not covered at 4 bits")


def test_mixed_and_other_widths_are_refused():
    m = _prepared(bits=4)
    m.model[4].conv.activation_quantizer.a_bits = m.model[4].conv.weight_quantizer.w_bits = 2
    _refused(m, r"model\.4\.conv has a_bits = 2, w_bits = 2; only W2A2 and W4A4 nets")
    m = _prepared(bits=4)
    m.model[5].conv.weight_quantizer.w_bits = 2
    _refused(m, r"model\.5\.conv has a_bits = 4, w_bits = 2")
    m = _prepared(bits=2)
    m.model[8].conv.activation_quantizer.a_bits = m.model[8].conv.weight_quantizer.w_bits = 4
    _refused(m, r"model\.8\.conv has a_bits = 4, w_bits = 4")
    _refused(_prepared(bits=3), r"model\.1\.conv has a_bits = 3, w_bits = 3")


def test_two_bit_reports_stay_their_goldens():
    from micronet_amd import inference
    assert inference.dorefa_codes_report(_prepared()) == _golden("codes_report_nin_gc.json")
    assert inference.dorefa_codes_report(_prepared(), code_ends=True) == _golden("codes_ends_report_nin_gc.json")
    assert inference.dorefa_codes_report(_prepared(), mfma_blocks=True) == _golden("codes_mfma_report_nin_gc.json")
    assert inference.dorefa_codes_report(_prepared(), mfma_blocks=True, mfma_k3=True) == _golden("codes_mfma3_report_nin_gc.json")
    assert inference.dorefa_codes_report(_prepared("nin"), tile_blocks=True) == _golden("codes_report_nin.json")
    assert inference.dorefa_codes_report(_prepared("nin"), code_ends=True, tile_blocks=True) == _golden("codes_ends_report_nin.json")
    assert not any("mfma" in L or "mfma3" in L for L in inference._walk_codes(_prepared())[1]), "a 2-bit net gains the keys under their flags only"


def test_code_plan_takes_the_width_last():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    p = inspect.signature(inference.CodePlan.__init__).parameters
    assert list(p)[-1] == "bits" and p["bits"].default == 2
    first, layers, last, tail, flatten, report = inference._walk_codes(_prepared(bits=4))
    plan = inference.CodePlan(first, layers, last, tail, flatten, report, bits=4)
    assert plan.bits == 4 and not plan.training
    assert inference.CodePlan(*inference._walk_codes(_prepared())).bits == 2
    with pytest.raises(MicronetHipError, match="a 4-bit plan is not covered"):
        inference.CodePlan(*inference._walk_codes(_prepared()), bits=4)          # popcount blocks
    with pytest.raises(MicronetHipError, match="a 4-bit plan is not covered"):
        inference.CodePlan(first, layers, last, tail, flatten, report, code_ends=True, bits=4)
    with pytest.raises(MicronetHipError, match="a 3-bit plan is not covered"):
        inference.CodePlan(first, layers, last, tail, flatten, report, bits=3)


def test_compile_names_the_first_layer_off_the_4_bit_grid():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=r"model\.1\.conv: the stored weights were not found on the 4-bit grid \(2k - 15\) / 15"):
        inference.dorefa_compile_codes(_prepared(bits=4))          # never pre-quantised


def test_w4_entry_points_are_declared_and_bound():
    from micronet_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "micronet_hip.h")).read()
    for name in ("mn_codeconv_mfma_fwd_bits", "mn_codeconv_mfma3_fwd_bits"):
        assert name in _lib.PROTOTYPES and (name + "(") in header
        assert len(_lib.PROTOTYPES[name][1]) == 9
