"""Host-only behaviour of ``iao_int8_report(model)`` / the walk of ``iao_compile_int8(model)`` on BN-folded IAO ResNets: stage order, kinds, strides, output maps and
their consumers; every refusal naming its layer; the old walk's report unchanged; and the judge of tests/iao8_res_cases.py held to the fp32 path's arithmetic in
torch on the CPU -- without a GPU.  (Weights off the grid are read from the packed tables: tests/test_gpu_iao8_res_plan.py.)"""
import json
import os

import pytest
import torch
import torch.nn as nn

import iao8_res_cases as RC
from conftest import GOLDEN

NAMES = {"name", "kind", "kernel", "k", "cin", "cout", "stride", "relu", "shortcut", "nout", "consumers", "table_bytes", "act_bytes_in", "act_bytes_out"}


def _folded(net, **kw):
    """The BN-folded IAO graph on the CPU (not pre-quantised: the walk does not read the weights)."""
    from micronet.compression.quantization.wqaq.iao import quantize as Q
    from micronet_amd import inference
    torch.manual_seed(0)
    args = dict(a_bits=8, w_bits=8, q_type=0, q_level=0, weight_observer=0, bn_fuse=True)
    args.update(kw)
    return inference.iao_model_bn_fuse(Q.prepare(net, inplace=True, **args)).eval()


def _basic(**kw):
    from micronet_amd.models import resnet
    return _folded(resnet.ResNet(resnet.BasicBlock, [1, 1, 1, 1]), **kw)


def _bottleneck(**kw):
    from micronet_amd.models import resnet
    return _folded(resnet.ResNet(resnet.BottleNeck, [1, 1, 1, 1]), **kw)


def _rows(rep):
    return [(r["name"], r["kind"], r["kernel"], r["stride"], r["nout"]) for r in rep]


def test_report_of_a_basic_block_net():
    from micronet_amd import inference
    rep = inference.iao_int8_report(_basic(), (16, 16))
    assert all(set(r) == NAMES for r in rep)
    assert _rows(rep) == [
        ("conv1", "first", "the model's own block (fp32), k_i8_pack x 2", 1, 2),
        ("conv2_x.0.residual_function.0", "int8", "k_i8conv<3,0>", 1, 1),
        ("conv2_x.0.residual_function.3", "int8_add", "k_i8res_add<3,2>", 1, 2),
        ("conv3_x.0.residual_function.0", "int8", "k_i8res_conv<3,2,1>", 2, 1),
        ("conv3_x.0.shortcut.0", "int8", "k_i8res_conv<1,2,0>", 2, 1),
        ("conv3_x.0.residual_function.3", "int8_add", "k_i8res_add<3,2>", 1, 2),
        ("conv4_x.0.residual_function.0", "int8", "k_i8res_conv<3,2,1>", 2, 1),
        ("conv4_x.0.shortcut.0", "int8", "k_i8res_conv<1,2,0>", 2, 1),
        ("conv4_x.0.residual_function.3", "int8_add", "k_i8res_add<3,2>", 1, 2),
        ("conv5_x.0.residual_function.0", "int8", "k_i8res_conv<3,2,1>", 2, 1),
        ("conv5_x.0.shortcut.0", "int8", "k_i8res_conv<1,2,0>", 2, 1),
        ("conv5_x.0.residual_function.3", "int8_add", "k_i8res_add<3,1>", 1, 1),
        ("avg_pool", "last", "k_i8_unpack, the model's own avg_pool and fc (fp32)", 1, 1),
    ]
    # who consumes what: conv1 feeds the first conv and -- the shortcut being the identity -- the block's own QuantAdd; a block in front of a down-sampling one feeds
    # that block's first conv and its shortcut conv; the shortcut conv writes at the QuantAdd's scale; the last block writes avg_pool's codes
    assert rep[0]["consumers"] == ["conv2_x.0.residual_function.0.activation_quantizer", "conv2_x.0.add.activation_quantizer"]
    assert rep[1]["consumers"] == ["conv2_x.0.residual_function.3.activation_quantizer"]
    assert rep[2]["consumers"] == ["conv3_x.0.residual_function.0.activation_quantizer", "conv3_x.0.shortcut.0.activation_quantizer"]
    assert rep[4]["consumers"] == ["conv3_x.0.add.activation_quantizer"] and rep[4]["relu"] == 0 and rep[3]["relu"] == 1
    assert rep[-2]["consumers"] == ["avg_pool.activation_quantizer"]
    assert [r["shortcut"] for r in rep if r["kind"] == "int8_add"] == ["identity", "conv", "conv", "conv"]
    # one byte per hidden activation: 16 x 16 images, maps 16, 8, 4, 2
    assert rep[0]["act_bytes_out"] == 4 * 64 * 256 + 2 * 64 * 256
    assert rep[2]["act_bytes_in"] == 2 * 64 * 256 and rep[2]["act_bytes_out"] == 2 * 64 * 256
    assert rep[3]["act_bytes_in"] == 64 * 256 and rep[3]["act_bytes_out"] == 128 * 64
    assert rep[-2]["act_bytes_out"] == 512 * 4 and rep[-1]["act_bytes_in"] == 512 * 4 + 4 * 512 * 4
    assert all(r["table_bytes"] > 0 for r in rep[1:-1]) and rep[0]["table_bytes"] == rep[-1]["table_bytes"] == 0


def test_report_of_a_bottleneck_net():
    from micronet_amd import inference
    rep = inference.iao_int8_report(_bottleneck(), (16, 16))
    assert _rows(rep)[:5] == [
        ("conv1", "first", "the model's own block (fp32), k_i8_pack x 2", 1, 2),
        ("conv2_x.0.residual_function.0", "int8", "k_i8conv<1,0>", 1, 1),
        ("conv2_x.0.residual_function.3", "int8", "k_i8conv<3,0>", 1, 1),
        ("conv2_x.0.shortcut.0", "int8", "k_i8res_conv<1,1,0>", 1, 1),          # 64 -> 256: a stride-1 shortcut conv, without ReLU
        ("conv2_x.0.residual_function.6", "int8_add", "k_i8res_add<1,2>", 1, 2),
    ]
    assert _rows(rep)[5:9] == [
        ("conv3_x.0.residual_function.0", "int8", "k_i8conv<1,0>", 1, 1),
        ("conv3_x.0.residual_function.3", "int8", "k_i8res_conv<3,2,1>", 2, 1),          # BottleNeck's strided 3x3
        ("conv3_x.0.shortcut.0", "int8", "k_i8res_conv<1,2,0>", 2, 1),
        ("conv3_x.0.residual_function.6", "int8_add", "k_i8res_add<1,2>", 1, 2),
    ]
    assert rep[0]["consumers"] == ["conv2_x.0.residual_function.0.activation_quantizer", "conv2_x.0.shortcut.0.activation_quantizer"]
    assert [r["kind"] for r in rep] == ["first"] + ["int8", "int8", "int8", "int8_add"] * 4 + ["last"]
    assert rep[-2]["kernel"] == "k_i8res_add<1,1>" and rep[-2]["cout"] == 2048 and rep[-1]["cin"] == 2048


def test_report_of_resnet18_has_no_fp32_map_between_the_pack_and_the_unpack():
    from micronet_amd import inference
    from micronet_amd.models import resnet
    rep = inference.iao_int8_report(_folded(resnet.resnet18()))
    kinds = [r["kind"] for r in rep]
    assert kinds[0] == "first" and kinds[-1] == "last" and set(kinds[1:-1]) == {"int8", "int8_add"}
    assert kinds.count("int8_add") == 8 and len(rep) == 2 + 16 + 3          # 16 block convs, three shortcut convs
    assert [r["shortcut"] for r in rep if r["kind"] == "int8_add"] == ["identity", "identity", "conv", "identity", "conv", "identity", "conv", "identity"]
    assert [r["nout"] for r in rep if r["kind"] == "int8_add"] == [2] * 7 + [1]
    # an identity block's second output is a code of its own QuantAdd
    assert rep[2]["consumers"] == ["conv2_x.1.residual_function.0.activation_quantizer", "conv2_x.1.add.activation_quantizer"]
    assert sum(r["stride"] == 2 for r in rep) == 6
    for r in rep[1:-1]:
        assert "fp32" not in r["kernel"]


def _raises(match, model, **kw):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=match):
        inference.iao_int8_report(model, **kw)
    with pytest.raises(MicronetHipError, match=match):
        inference.iao_compile_int8(model, **kw)          # the same walk, before anything touches a GPU


def test_refuses_an_asymmetric_quantadd():
    m = _basic()
    m.conv3_x[0].add.activation_quantizer.q_type = 1
    _raises(r"conv3_x\.0\.add\.activation_quantizer is asymmetric", m)
    m = _basic()
    m.conv2_x[0].add.activation_quantizer.zero_point.fill_(3.0)
    _raises(r"conv2_x\.0\.add\.activation_quantizer is asymmetric", m)
    _raises(r"conv2_x\.0\.add\.activation_quantizer is asymmetric", _basic(q_type=1))


def test_refuses_a_32_bit_quantizer():
    m = _basic()
    m.conv4_x[0].shortcut[0].weight_quantizer.bits = 32
    _raises(r"conv4_x\.0\.shortcut\.0\.weight_quantizer has 32 bits", m)
    m = _bottleneck()
    m.conv5_x[0].add.activation_quantizer.bits = 32
    _raises(r"conv5_x\.0\.add\.activation_quantizer has 32 bits", m)
    m = _basic()
    m.avg_pool.activation_quantizer.bits = 32
    _raises(r"avg_pool\.activation_quantizer has 32 bits", m)


def test_refuses_a_conv_that_is_not_quant_inference():
    m = _basic()
    m.conv3_x[0].residual_function[0].quant_inference = False
    _raises(r"conv3_x\.0\.residual_function\.0 is not quant_inference", m)


def test_refuses_a_net_that_was_not_folded():
    from micronet.compression.quantization.wqaq.iao import quantize as Q
    from micronet_amd.models import resnet
    torch.manual_seed(0)
    m = Q.prepare(resnet.ResNet(resnet.BasicBlock, [1, 1, 1, 1]), inplace=True, a_bits=8, w_bits=8, q_type=0, q_level=0, weight_observer=0, bn_fuse=True).eval()
    _raises(r"conv1\.0 \(QuantBNFuseConv2d\) is not a BN-folded IAO QuantConv2d", m)


def test_refuses_a_geometry_the_kernels_do_not_cover():
    m = _basic()
    m.conv3_x[0].residual_function[0].stride = (3, 3)
    _raises(r"conv3_x\.0\.residual_function\.0: geometry not covered by mn_i8res_supported \(3x3, stride \(3, 3\)", m)
    m = _basic()
    m.conv2_x[0].residual_function[0].dilation = (2, 2)
    _raises(r"conv2_x\.0\.residual_function\.0: geometry not covered by mn_i8conv_supported \(3x3, stride \(1, 1\), padding \(1, 1\), dilation \(2, 2\)", m)


def test_byte_ends_is_refused_naming_conv1():
    _raises(r"byte_ends=True\): conv1: .* the two-output form of k_i8first is not built", _basic(), byte_ends=True)


def test_a_cpu_model_is_refused_by_compile_only():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    assert inference.iao_int8_report(_basic())
    with pytest.raises(MicronetHipError, match="no CPU fallback"):
        inference.iao_compile_int8(_basic())


def test_the_old_walk_is_unchanged():
    """nin_gc's reports, row for row what they are at the parent commit (pinned there in tests/golden)."""
    from micronet_amd import inference
    from micronet_amd.train import build_model
    m = _folded(build_model("nin_gc"))
    assert not inference._is_ref_resnet(m)
    assert inference.iao_int8_report(m) == json.load(open(os.path.join(GOLDEN, "iao8_report_nin_gc.json")))
    assert inference.iao_int8_report(m, byte_ends=True) == json.load(open(os.path.join(GOLDEN, "iao8_ends_report_nin_gc.json")))
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=r"iao_compile_int8: module order not recognised \(Linear: expected an nn.Sequential of blocks"):
        inference.iao_int8_report(nn.Linear(4, 4))


def test_the_plan_is_a_module_and_the_entry_points_are_bound():
    import ctypes as C
    from micronet_amd import _lib, inference
    assert issubclass(inference.Int8ResPlan, nn.Module)
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "micronet_hip.h")).read()
    for name in ("mn_i8res_supported", "mn_i8res_table_bytes", "mn_i8res_pack", "mn_i8res_conv_fwd", "mn_i8res_add_fwd"):
        assert name in _lib.PROTOTYPES and (name + "(") in header
    for name in ("mn_i8res_pack", "mn_i8res_conv_fwd", "mn_i8res_add_fwd"):          # the stream is the last argument
        assert _lib.PROTOTYPES[name][1][-1] is C.c_void_p
    assert C.POINTER(_lib.I8ResAdd) in _lib.PROTOTYPES["mn_i8res_add_fwd"][1]
    assert [f[0] for f in _lib.I8ResAdd._fields_] == ["s_add", "add_bits", "nout", "s_out0", "bits0", "s_out1", "bits1"]


@pytest.mark.parametrize("case", range(len(RC.CONVS)), ids=[c[0] for c in RC.CONVS])
def test_conv_judge_within_the_cap_of_the_fp32_path(case):
    RC.check_conv_vs_torch(case)


def test_conv_judge_within_the_cap_at_the_extreme_geometry():
    RC.check_extreme_geometry_vs_torch()


@pytest.mark.parametrize("case", range(len(RC.ADDS)), ids=[c[0] for c in RC.ADDS])
def test_add_judge_within_the_cap_of_the_fp32_path(case):
    RC.check_add_vs_torch(case)
