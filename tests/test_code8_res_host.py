"""Host-only behaviour of ``dorefa_bytes_report`` on the reference's ResNets (the walk of ``dorefa_compile_bytes``: csrc/qgemm_codes_w8_res.h): the stage report of W8A8
resnet18 and the named refusals -- without a GPU."""
import pytest

from test_codes_host import _prepared


def _refused(model, pattern, **kw):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=pattern):
        inference.dorefa_bytes_report(model, **kw)


def test_bytes_report_resnet18():
    from micronet_amd import inference
    rep = inference.dorefa_bytes_report(_prepared("resnet18", bits=8))
    assert [r["kind"] for r in rep] == ["first", "quant"] + ["conv", "add"] * 8 + ["last"]
    assert rep[1]["kernel"] == "k_code8_quant" and rep[1]["outputs"] == ["bytes"] and rep[1]["blocks"] == 4
    conv, add = rep[2:-1:2], rep[3:-1:2]
    assert [r["name"] for r in conv[:3]] == ["conv2_x.0.residual_function.0", "conv2_x.1.residual_function.0", "conv3_x.0.residual_function.0"]
    assert [r["stride"] for r in conv] == [1, 1, 2, 1, 2, 1, 2, 1] and all(r["stride"] == 1 for r in add)
    assert [r["kernel"] for r in conv] == ["k_code8res_conv<3,%d>" % s for s in (1, 1, 2, 1, 2, 1, 2, 1)]
    assert [r["shortcut"] for r in add] == ["identity", "identity"] + ["conv", "identity"] * 3 and all(r["shortcut"] is None for r in conv)
    assert [r["kernel"] for r in add] == ["k_code8res_add<3,%d>" % s for s in (1, 1, 2, 1, 2, 1, 2, 1)]
    # bytes while a block follows; fp32 only for a following identity shortcut, or avg_pool
    assert [r["outputs"] for r in add] == [["bytes", "f32"], ["bytes"]] * 3 + [["bytes", "f32"], ["f32"]]
    assert all(r["outputs"] == ["bytes"] for r in conv)
    assert [(r["K"], r["blocks"]) for r in rep[2:6]] == [(576, 4)] * 4 and (rep[-2]["K"], rep[-2]["blocks"]) == (4608, 32) and rep[-1]["K"] == 512


def test_refusals_name_the_layer_and_the_rule():
    _refused(_prepared("resnet50", bits=8), r"conv2_x\.0: BottleNeck blocks are not built")
    _refused(_prepared("resnet18", bits=4), r"conv2_x\.0\.residual_function\.0 has a_bits = 4, w_bits = 4; only W8A8 nets are deployed on bytes")
    m = _prepared("resnet18", bits=8)
    m.conv3_x[0].shortcut[0].quant_inference = False
    _refused(m, r"conv3_x\.0\.shortcut\.0 is not a quant_inference=True layer")
    _refused(_prepared("resnet18", bits=8), r"byte_ends=True\): conv1 / avg_pool: a ResNet's ends on bytes .* are not built", byte_ends=True)


def test_bytes_report_nin_gc_unchanged():
    from micronet_amd import inference
    rep = inference.dorefa_bytes_report(_prepared(bits=8))
    assert [r["kind"] for r in rep] == ["first"] + ["byte"] * 7 + ["last"]
    assert sorted(rep[1]) == ["K", "blocks", "kernel", "kind", "name", "out_order", "pooled", "stage"] and rep[1]["kernel"] == "k_code8conv<1,0>"
