"""Host-only behaviour of ``iao_int8_report(model, end_to_end=True)`` / the walk of ``iao_compile_int8(model, end_to_end=True)`` on BN-folded IAO ResNets: the two
end rows, the rows between them, the defaults untouched, every refusal naming its layer -- without a GPU.

The last three tests guard the JUDGE of tests/iao8_e2e_cases.py, not the feature: they hold its arithmetic to the fp32 path's in torch on the CPU (the first block
within one step on at most 1e-4 of the elements, the pooled code likewise over more than 10^6 pooled elements, the logits within the float accumulate's bound)."""
import json
import os

import numpy as np
import pytest
import torch

import iao8_cases as IC
import iao8_e2e_cases as XC
from conftest import GOLDEN
from test_iao8_res_host import NAMES, _folded

F = np.float32
E2E = r"iao_compile_int8\(end_to_end=True\): "


def _e2e(net, **kw):
    m = _folded(net, **kw)
    m.fc.quant_inference = True          # (iao_model_bn_fuse marks the convs; the classifier's stored weights go on the grid with prequantize_weights as well)
    return m


def _basic(**kw):
    from micronet_amd.models import resnet
    return _e2e(resnet.ResNet(resnet.BasicBlock, [1, 1, 1, 1]), **kw)


def _bottleneck(**kw):
    from micronet_amd.models import resnet
    return _e2e(resnet.ResNet(resnet.BottleNeck, [1, 1, 1, 1]), **kw)


def _resnet18(**kw):
    from micronet_amd.models import resnet
    return _e2e(resnet.resnet18(), **kw)


@pytest.mark.parametrize("make,hw,cl,hwl", [(_basic, (16, 16), 512, 4), (_bottleneck, (16, 16), 2048, 4), (_resnet18, (32, 32), 512, 16)], ids=["basic", "bottleneck", "resnet18"])
def test_end_to_end_report(make, hw, cl, hwl):
    from micronet_amd import inference
    m = make()
    rep, dflt = inference.iao_int8_report(m, hw, end_to_end=True), inference.iao_int8_report(m, hw)
    assert all(set(r) == NAMES for r in rep) and len(rep) == len(dflt)
    first, last = rep[0], rep[-1]
    assert (first["name"], first["kind"], first["kernel"], first["nout"]) == ("conv1", "int8_first", "k_i8first2<3,2>", 2)
    assert (last["name"], last["kind"], last["kernel"], last["nout"]) == ("avg_pool", "int8_last", "k_i8poolfc", 1)
    assert first["consumers"] == dflt[0]["consumers"] and first["table_bytes"] > 0 and last["table_bytes"] > 0
    # fp32 image in, nout byte maps out; bytes in, 4 O out
    assert first["act_bytes_in"] == 4 * 3 * hw[0] * hw[1] and first["act_bytes_out"] == 2 * 64 * hw[0] * hw[1]
    assert last["act_bytes_in"] == cl * hwl and last["act_bytes_out"] == 4 * 10 and (last["cin"], last["cout"]) == (cl, 10)
    assert rep[1:-1] == dflt[1:-1], "every row between the ends is the default report's"
    assert all("fp32" not in r["kernel"] for r in rep), "no fp32 stage is left"


def test_the_default_report_is_untouched():
    from micronet_amd import inference
    from micronet_amd.train import build_model
    for m in (_basic(), _bottleneck()):
        assert inference.iao_int8_report(m, (16, 16)) == inference.iao_int8_report(m, (16, 16), end_to_end=False)
        assert inference.iao_int8_report(m, (16, 16))[0]["kind"] == "first"
    g = _folded(build_model("nin_gc"))
    assert inference.iao_int8_report(g, end_to_end=False) == json.load(open(os.path.join(GOLDEN, "iao8_report_nin_gc.json")))
    assert inference.iao_int8_report(g, byte_ends=True, end_to_end=False) == json.load(open(os.path.join(GOLDEN, "iao8_ends_report_nin_gc.json")))


def _raises(match, model, **kw):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=match):
        inference.iao_int8_report(model, end_to_end=True, **kw)
    with pytest.raises(MicronetHipError, match=match):
        inference.iao_compile_int8(model, end_to_end=True, **kw)          # the same walk, before anything touches a GPU


def test_refuses_a_model_that_is_not_the_resnet_tree():
    from micronet_amd.train import build_model
    _raises(E2E + r"covered for the reference ResNet tree only \(nin_gc's form is byte_ends=True\)", _folded(build_model("nin_gc")))


def test_the_other_keywords_keep_their_messages():
    _raises(r"byte_ends=True\): conv1: .* the two-output form of k_i8first is not built", _basic(), byte_ends=True)
    _raises(r"zero_points=True\): the reference ResNet tree is not covered with zero points", _basic(), zero_points=True)


def test_refuses_a_conv1_that_is_not_quant_inference():
    m = _basic()
    m.conv1[0].quant_inference = False
    _raises(E2E + r"conv1\.0: conv1\.0 is not quant_inference", m)


def test_refuses_an_asymmetric_conv1_quantizer():
    m = _basic()
    m.conv1[0].activation_quantizer.q_type = 1
    _raises(E2E + r"conv1\.0: conv1\.0\.activation_quantizer is asymmetric", m)


def test_refuses_a_7x7_stem():
    m = _basic()
    m.conv1[0].kernel_size, m.conv1[0].padding = (7, 7), (3, 3)
    _raises(E2E + r"conv1\.0: geometry not covered by mn_i8first_supported \(7x7, stride \(1, 1\), padding \(3, 3\)", m)
    m = _basic()
    m.conv1[0].stride = (2, 2)
    _raises(E2E + r"conv1\.0: geometry not covered by mn_i8first_supported \(3x3, stride \(2, 2\)", m)


def test_refuses_an_avg_pool_that_is_not_adaptive_to_1x1():
    m = _basic()
    m.avg_pool.output_size = (2, 2)
    _raises(E2E + r"avg_pool: \(QuantAdaptiveAvgPool2d\) is not a QuantAdaptiveAvgPool2d to 1 x 1", m)


def test_refuses_an_fc_the_pooled_classifier_does_not_cover():
    m = _basic()
    m.fc = type(m.fc)(512, 65, a_bits=8, w_bits=8, q_type=0, q_level=0, quant_inference=True)
    _raises(E2E + r"fc: shape not covered by mn_i8poolfc_supported \(512 channels, a 4 x 4 map, 65 outputs", m)
    m = _basic()
    m.fc.activation_quantizer.q_type = 1
    _raises(E2E + r"fc: fc\.activation_quantizer is asymmetric", m)
    m = _basic()
    m.fc.in_features = 100
    _raises(E2E + r"fc: in_features is 100, the last block conv5_x\.0\.residual_function\.3 writes 512 channels", m)
    m = _basic()
    m.fc.quant_inference = False
    _raises(E2E + r"fc: is not quant_inference", m)
    m = _basic()
    m.fc = torch.nn.Linear(512, 10)
    _raises(E2E + r"fc: \(Linear\) is not an IAO QuantLinear", m)


def test_the_entry_points_are_bound():
    import ctypes as C
    from micronet_amd import _lib
    for name in ("mn_i8first_fwd2", "mn_i8poolfc_supported", "mn_i8poolfc_table_bytes", "mn_i8poolfc_pack", "mn_i8poolfc_fwd"):
        assert name in _lib.PROTOTYPES
    assert C.POINTER(_lib.I8FirstOuts) in _lib.PROTOTYPES["mn_i8first_fwd2"][1]
    assert [f[0] for f in _lib.I8FirstOuts._fields_] == ["nout", "s_out0", "bits0", "s_out1", "bits1"]


# ---------------------------------------------------------------------------------------------- the judge against torch on the CPU (guards the judge, not the feature)
def test_first_block_judge_within_the_cap_of_the_fp32_path():
    flips = total = 0
    for widths in ((8, 8), (4, 4)):
        for idx, (name, x_shape, Oc, KS) in enumerate(XC.FIRST2):
            case = IC.make_case(x_shape, Oc, KS, 1, 6200 + idx, widths=widths, special=False)
            outs = XC.outs_of(case, widths[1], XC.S1_RATIO)
            r = XC.EC.chain_r(case["acc"], case["al"], case["b"], 1)
            x = torch.from_numpy((case["j"].astype(F) * case["s_a"]).astype(F))
            rt = torch.relu(torch.nn.functional.conv2d(x, torch.from_numpy(case["w"]), torch.from_numpy(case["b"]), padding=KS // 2)).numpy()
            for s, bits in outs:
                d = np.abs(IC.code_of(r, s, bits).astype(np.int32) - IC.code_of(rt, s, bits).astype(np.int32))
                assert d.max() <= 1, (name, widths, int(d.max()))
                flips, total = flips + int((d != 0).sum()), total + d.size
    print("first block: flips against the fp32 path", flips, "of", total)
    assert total >= 300000 and flips <= 1e-4 * total


POOLED_SHAPES = [(64, 512, 4, 4), (64, 2048, 2, 2), (64, 64, 8, 8), (64, 40, 3, 3), (64, 64, 7, 5), (64, 512, 2, 2)]


def test_pooled_code_judge_within_the_cap_of_the_fp32_path():
    """torch.nn.functional.adaptive_avg_pool2d on the CPU does not sum like the contract (an fp32 sum in its own order, not the fp64 one), and its last-place
    differences decide exact ties: s_fc is drawn as 1.0173 max|m| / qmax, where no code boundary falls on a value the means take often."""
    r = np.random.default_rng(1)
    flips = total = 0
    for shape in POOLED_SHAPES:
        for s_p in (F(2.0 ** -6), F(2.0 ** -6 * 1.2345), F(0.0371)):
            for bits in (8, 4):
                lo, hi = (int(v) for v in IC.qrange(bits))
                c = r.integers(lo, hi + 1, size=shape).astype(np.int64)
                m = XC.pooled(c, s_p)
                s_fc = F(F(1.0173) * np.abs(m).max() / F(hi))
                v = torch.from_numpy((c.astype(F) * s_p).astype(F))
                mt = torch.nn.functional.adaptive_avg_pool2d(v, (1, 1)).numpy().reshape(m.shape)
                d = np.abs(IC.code_of(m, s_fc, bits).astype(np.int32) - IC.code_of(mt, s_fc, bits).astype(np.int32))
                assert d.max() <= 1, (shape, float(s_p), bits, int(d.max()))
                flips, total = flips + int((d != 0).sum()), total + d.size
    print("pooled code: flips against adaptive_avg_pool2d", flips, "of", total)
    assert total >= 10 ** 6 and flips <= 1e-4 * total


@pytest.mark.parametrize("case", range(len(XC.POOLFC)), ids=[c[0] for c in XC.POOLFC])
def test_logits_judge_within_the_bound_of_the_float_accumulate(case):
    name, shape, Oc = XC.POOLFC[case]
    cs = XC.poolfc_case(shape, Oc, 6400 + case)
    _, j, _, y = XC.poolfc_judge(cs)
    xq = torch.from_numpy((j.astype(F) * cs["s_fc"]).astype(F))
    yt = torch.nn.functional.linear(xq, torch.from_numpy(cs["w"]), torch.from_numpy(cs["b"])).numpy()
    bound = 1e-5 * ((np.abs(j) @ np.abs(cs["k"]).T).astype(np.float64) * cs["al"].reshape(1, -1).astype(np.float64) + np.abs(cs["b"]).reshape(1, -1))
    err = np.abs(y.astype(np.float64) - yt.astype(np.float64))
    print(name, "largest |judge - torch| / bound", float((err / bound).max()))
    assert (err <= bound).all()
