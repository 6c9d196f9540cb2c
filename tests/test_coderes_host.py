"""Host-only behaviour of ``dorefa_codes_report`` / ``dorefa_compile_codes`` on the reference's ResNets (csrc/qgemm_codes_res.h): the stage report of W2A2 resnet18 and
the named refusals -- without a GPU."""
import pytest
import torch.nn as nn

from test_codes_host import _prepared


def _refused(model, pattern, entry="dorefa_codes_report", **kw):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=pattern):
        getattr(inference, entry)(model, **kw)


def test_codes_report_resnet18():
    from micronet_amd import inference
    model = _prepared("resnet18")
    assert type(model.conv2_x[0]).__name__ == "FusedBasicBlock", "default prepare fuses the blocks; the walk accepts them"
    rep = inference.dorefa_codes_report(model)
    assert rep == inference.dorefa_codes_report(model, mfma_blocks=True, mfma_k3=True), "the plan is MFMA throughout"
    assert [r["kind"] for r in rep] == ["first", "quant"] + ["conv", "add"] * 8 + ["last"]
    assert all(sorted(r) == ["K", "blocks", "kernel", "kind", "name", "outputs", "shortcut", "stride"] for r in rep)
    assert rep[1]["kernel"] == "k_coderes_quant" and rep[1]["outputs"] == ["planes"] and rep[1]["blocks"] == 4
    conv, add = rep[2:-1:2], rep[3:-1:2]
    assert [r["name"] for r in conv[:3]] == ["conv2_x.0.residual_function.0", "conv2_x.1.residual_function.0", "conv3_x.0.residual_function.0"]
    assert [r["kernel"] for r in conv] == ["k_coderes_conv<3,%d>" % s for s in (1, 1, 2, 1, 2, 1, 2, 1)] and all(r["stride"] == 1 for r in add)
    assert [r["shortcut"] for r in add] == ["identity", "identity"] + ["conv", "identity"] * 3 and all(r["shortcut"] is None for r in conv)
    assert [r["kernel"] for r in add] == ["k_coderes_add<3,%d>" % s for s in (1, 1, 2, 1, 2, 1, 2, 1)]
    # planes while a block follows; fp32 only for a following identity shortcut, or avg_pool
    assert [r["outputs"] for r in add] == [["planes", "f32"], ["planes"]] * 3 + [["planes", "f32"], ["f32"]] and all(r["outputs"] == ["planes"] for r in conv)
    assert (rep[-2]["K"], rep[-2]["blocks"]) == (4608, 32), "conv5_x: K * 9 = 41472, beyond the threshold kernels"


def test_refusals_name_the_layer_and_the_rule():
    _refused(_prepared("resnet50"), r"conv2_x\.0: BottleNeck blocks are not built")
    _refused(_prepared("resnet18", bits=4), r"conv2_x\.0\.residual_function\.0 has a_bits = 4, w_bits = 4; only W2A2 ResNets are deployed on planes")
    m = _prepared("resnet18")
    m.conv3_x[0].shortcut[0].weight_quantizer.w_bits = 4
    _refused(m, r"conv3_x\.0\.shortcut\.0 has a_bits = 2, w_bits = 4")
    _refused(_prepared("resnet18"), r"code_ends=True\): conv1 / avg_pool: a ResNet's ends on planes .* are not built", code_ends=True)
    _refused(_prepared("resnet18"), r"tile_blocks=True\): a ResNet has neither", tile_blocks=True)
    m = _prepared("resnet18")
    m.conv3_x[0].shortcut[0].quant_inference = False
    _refused(m, r"conv3_x\.0\.shortcut\.0 is not a quant_inference=True layer")
    m = _prepared("resnet18")
    m.conv4_x[1].residual_function[4] = nn.BatchNorm2d(256, affine=False)
    _refused(m, r"conv4_x\.1\.residual_function\.4: needs a BatchNorm2d with affine parameters, running statistics")
    _refused(_prepared("resnet18"), r"conv2_x\.0\.residual_function\.0: the stored weights were not found on the 2-bit grid \(2k - 3\) / 3", "dorefa_compile_codes")
    _refused(_prepared("resnet18").train(), r"the model is in training mode", "dorefa_compile_codes")
