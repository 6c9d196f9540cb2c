"""Host-only behaviour of ``iao_int8_report(model)`` / the walk of ``iao_compile_int8(model)``: the stage report of the BN-folded nin_gc, and every refusal naming its
layer -- without a GPU.  (Weights off the grid are read from the packed tables: tests/test_gpu_iao8_plan.py.)"""
import json
import os

import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN

NAMES = {"name", "kind", "kernel", "k", "cin", "cout", "groups", "pool", "out_order", "table_bytes", "act_bytes_in", "act_bytes_out"}


def _folded(net=None, **kw):
    """The BN-folded IAO graph on the CPU (not pre-quantised: the walk does not read the weights)."""
    from micronet.compression.quantization.wqaq.iao import quantize as Q
    from micronet_amd import inference
    from micronet_amd.train import build_model
    torch.manual_seed(0)
    args = dict(a_bits=8, w_bits=8, q_type=0, q_level=0, weight_observer=0, bn_fuse=True)
    args.update(kw)
    T = Q.prepare(net if net is not None else build_model("nin_gc"), inplace=True, **args)
    return inference.iao_model_bn_fuse(T).eval()


def test_iao8_report_nin_gc_is_pinned():
    from micronet_amd import inference
    rep = inference.iao_int8_report(_folded())
    want = json.load(open(os.path.join(GOLDEN, "iao8_report_nin_gc.json")))
    assert rep == want
    assert [r["kind"] for r in rep] == ["first"] + ["int8"] * 7 + ["last"]
    assert all(set(r) == NAMES for r in rep)
    assert [r["kernel"] for r in rep[1:-1]] == ["k_i8conv<1,0>", "k_i8conv<1,1>", "k_i8conv<3,0>", "k_i8conv<1,0>", "k_i8conv<1,1>", "k_i8conv<3,0>", "k_i8conv<1,0>"]
    assert [r["out_order"] for r in rep] == ["identity", "shuffle 2", "shuffle 2", "shuffle 16", "shuffle 4", "shuffle 4", "shuffle 32", "identity", "identity"]
    for a, b in zip(rep[1:-1], rep[2:]):
        assert a["act_bytes_out"] == (b["act_bytes_in"] if b["kind"] == "int8" else b["act_bytes_in"] - 4 * b["cin"] * 8 * 8), "one byte per hidden activation"


def test_iao8_report_of_a_sequential_and_per_layer_weights():
    from micronet_amd import inference
    m = _folded(q_level=1)
    rep = inference.iao_int8_report(m.model)
    assert [r["name"] for r in rep] == ["0", "1", "2", "4", "5", "6", "8", "9", "10"]
    layers = inference._walk_iao8(m)[1]
    assert not any(L["per_channel"] for L in layers)
    assert all(L["per_channel"] for L in inference._walk_iao8(_folded())[1])


def _raises(match, model):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=match):
        inference.iao_int8_report(model)
    with pytest.raises(MicronetHipError, match=match):
        inference.iao_compile_int8(model)          # the same walk, before anything touches a GPU


def test_refuses_an_asymmetric_quantizer():
    m = _folded()
    m.model[4].conv.activation_quantizer.q_type = 1
    _raises(r"model\.4\.conv\.activation_quantizer is asymmetric", m)
    m = _folded()
    m.model[7].activation_quantizer.zero_point.fill_(3.0)
    _raises(r"model\.7\.activation_quantizer is asymmetric", m)
    _raises(r"model\.10\.conv\.activation_quantizer is asymmetric", _folded(q_type=1))


def test_refuses_a_32_bit_quantizer():
    m = _folded()
    m.model[5].conv.weight_quantizer.bits = 32
    _raises(r"model\.5\.conv\.weight_quantizer has 32 bits", m)
    m = _folded()
    m.model[2].conv.activation_quantizer.bits = 32
    _raises(r"model\.2\.conv\.activation_quantizer has 32 bits", m)


def test_refuses_a_per_tensor_scale_that_is_not_one_value():
    m = _folded()
    q = m.model[6].conv.activation_quantizer
    q.scale = torch.ones(3)
    q.zero_point = torch.zeros(3)
    _raises(r"model\.6\.conv\.activation_quantizer carries 3 scales", m)


def test_refuses_a_layer_that_is_not_quant_inference():
    m = _folded()
    m.model[2].conv.quant_inference = False
    _raises(r"model\.2\.conv is not quant_inference", m)


def test_refuses_a_geometry_the_kernel_does_not_cover():
    from micronet_amd.models import nin_gc
    _raises(r"model\.4\.conv: geometry not covered by mn_i8conv_supported \(3x3, stride 1, padding 1, dilation 1, groups 16, 2 channels per group",
            _folded(net=nin_gc.Net(cfg=[32, 32, 32, 64, 64, 64, 128, 128])))
    m = _folded()
    m.model[5].conv.stride = (2, 2)
    _raises(r"model\.5\.conv: geometry not covered by mn_i8conv_supported \(1x1, stride 2", m)


def test_refuses_another_pool():
    from micronet.compression.quantization.wqaq.iao import quantize as Q
    m = _folded()
    m.model[3] = nn.MaxPool2d(2, 2)
    _raises(r"model\.3 \(MaxPool2d, kernel 2, stride 2, padding 0\): only a 2x2 / stride 2 QuantMaxPool2d", m)
    m = _folded()
    m.model[7] = Q.QuantMaxPool2d(3, stride=2, padding=1)
    _raises(r"model\.7 \(QuantMaxPool2d, kernel 3, stride 2, padding 1\)", m)


def test_refuses_a_pool_directly_behind_the_first_block():
    m = _folded()
    kids = list(m.model.children())
    _raises(r"1: a max-pool directly behind the first block", nn.Sequential(kids[0], kids[3], *kids[1:3], *kids[4:]))


def test_a_cpu_model_is_refused_by_compile_only():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    assert inference.iao_int8_report(_folded())
    with pytest.raises(MicronetHipError, match="no CPU fallback"):
        inference.iao_compile_int8(_folded())


def test_the_plan_is_eval_only_and_the_entry_points_are_bound():
    from micronet_amd import _lib, inference
    assert issubclass(inference.Int8Plan, nn.Module)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "micronet_hip.h")).read()
    for name in ("mn_i8conv_supported", "mn_i8conv_table_bytes", "mn_i8conv_pack", "mn_i8conv_fwd", "mn_i8_pack_codes", "mn_i8_unpack_codes"):
        assert name in _lib.PROTOTYPES and (name + "(") in header
        assert _lib.PROTOTYPES[name][1][-1] is not None
    for name in ("mn_i8conv_pack", "mn_i8conv_fwd", "mn_i8_pack_codes", "mn_i8_unpack_codes"):          # the stream is the last argument
        import ctypes as C
        assert _lib.PROTOTYPES[name][1][-1] is C.c_void_p
