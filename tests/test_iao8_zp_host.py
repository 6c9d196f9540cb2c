"""Host-only behaviour of ``iao_int8_report(model, zero_points=True)`` / the walk of ``iao_compile_int8(model, zero_points=True)``: the stage report of a BN-folded
nin_gc prepared with ``q_type=1``, what the keyword leaves unchanged, and every refusal naming its layer -- without a GPU."""
import ctypes as C
import os

import pytest
import torch

from conftest import GOLDEN
from test_iao8_host import NAMES, _folded


def _trained(m):
    """What a training step leaves behind on every quantizer: ``q_type`` set from the class (``update_qparams``)."""
    from micronet.compression.quantization.wqaq.iao import quantize as Q
    for q in m.modules():
        if isinstance(q, Q.Quantizer):
            q.q_type = q._q_type_static
    return m


def _raises(match, model, **kw):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=match):
        inference.iao_int8_report(model, zero_points=True, **kw)
    with pytest.raises(MicronetHipError, match=match):
        inference.iao_compile_int8(model, zero_points=True, **kw)          # the same walk, before anything touches a GPU


def test_report_of_an_asymmetric_nin_gc():
    from micronet_amd import inference
    m = _trained(_folded(q_type=1))
    rep = inference.iao_int8_report(m, zero_points=True)
    sym = inference.iao_int8_report(_folded())
    assert [r["kind"] for r in rep] == ["first"] + ["int8"] * 7 + ["last"]
    assert all(set(r) == NAMES for r in rep)
    assert [r["kernel"] for r in rep[1:-1]] == ["k_i8zconv<1,0>", "k_i8zconv<1,1>", "k_i8zconv<3,0>", "k_i8zconv<1,0>", "k_i8zconv<1,1>", "k_i8zconv<3,0>", "k_i8zconv<1,0>"]
    assert rep[0]["kernel"] == "the model's own block (fp32), k_i8z_pack" and rep[-1]["kernel"] == "k_i8z_unpack, the model's own block (fp32)"
    for a, b in zip(rep, sym):
        assert {k: v for k, v in a.items() if k not in ("kernel", "table_bytes")} == {k: v for k, v in b.items() if k not in ("kernel", "table_bytes")}
    # the tile header of the zero-point table holds two more words per row, and the table header 16 more words
    assert all(a["table_bytes"] > b["table_bytes"] for a, b in zip(rep[1:-1], sym[1:-1]))
    layers = inference._walk_iao8(m, zero_points=True)[1]
    assert all(L["zp"] and L["asym_a"] == L["asym_w"] == L["asym_p"] == L["asym_out"] == 1 for L in layers)
    # without the keyword the same model is refused as before
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=r"model\.10\.conv\.activation_quantizer is asymmetric; a zero byte must be the value 0 \(symmetric quantizers only\)"):
        inference.iao_int8_report(m)


def test_a_symmetric_net_reports_identically_with_the_keyword():
    from micronet_amd import inference
    m = _folded()
    assert inference.iao_int8_report(m, zero_points=True) == inference.iao_int8_report(m)
    a, b = inference._walk_iao8(m, zero_points=True)[1], inference._walk_iao8(m)[1]
    assert not any(L["zp"] for L in a) and [L["table_bytes"] for L in a] == [L["table_bytes"] for L in b]


def test_only_the_stages_next_to_an_asymmetric_quantizer_take_the_zero_point_kernel():
    """One asymmetric activation quantizer (model.5.conv): the stage that consumes it and the stage that produces it."""
    from micronet.compression.quantization.wqaq.iao import quantize as Q
    from micronet_amd import inference
    m = _folded()
    old = m.model[5].conv.activation_quantizer
    m.model[5].conv.activation_quantizer = _trained(Q.AsymmetricQuantizer(bits=8, observer=old.observer, activation_weight_flag=1))
    rep = inference.iao_int8_report(m, zero_points=True)
    assert [r["kernel"] for r in rep[1:-1]] == ["k_i8conv<1,0>", "k_i8conv<1,1>", "k_i8zconv<3,0>", "k_i8zconv<1,0>", "k_i8conv<1,1>", "k_i8conv<3,0>", "k_i8conv<1,0>"]
    assert "k_i8_pack" in rep[0]["kernel"] and "k_i8_unpack" in rep[-1]["kernel"]


def test_byte_ends_with_zero_points_raises():
    _raises(r"zero_points=True\): byte_ends=True is not covered together with zero points", _trained(_folded(q_type=1)), byte_ends=True)
    _raises(r"zero_points=True\): byte_ends=True is not covered together with zero points", _folded(), byte_ends=True)


def test_a_resnet_with_zero_points_raises():
    from micronet.compression.quantization.wqaq.iao import quantize as Q
    from micronet_amd import inference
    from micronet_amd.models import resnet
    torch.manual_seed(0)
    T = Q.prepare(resnet.ResNet(resnet.BasicBlock, [1, 1, 1, 1]), inplace=True, a_bits=8, w_bits=8, q_type=0, q_level=0, weight_observer=0, bn_fuse=True)
    m = inference.iao_model_bn_fuse(T).eval()
    assert inference.iao_int8_report(m)
    _raises(r"zero_points=True\): the reference ResNet tree is not covered with zero points", m)


def test_a_32_bit_quantizer_is_still_refused():
    m = _trained(_folded(q_type=1))
    m.model[5].conv.weight_quantizer.bits = 32
    _raises(r"model\.5\.conv\.weight_quantizer has 32 bits", m)
    m = _trained(_folded(q_type=1))
    m.model[3].activation_quantizer.bits = 32
    _raises(r"model\.3\.activation_quantizer has 32 bits", m)


def test_a_class_q_type_mismatch_is_refused():
    m = _trained(_folded(q_type=1))
    m.model[4].conv.activation_quantizer.q_type = 0
    _raises(r"model\.4\.conv\.activation_quantizer \(AsymmetricQuantizer\) carries q_type 0, its class q_type 1", m)
    m = _folded()
    m.model[6].conv.weight_quantizer.q_type = 1
    _raises(r"model\.6\.conv\.weight_quantizer \(SymmetricQuantizer\) carries q_type 1, its class q_type 0", m)
    # a net that never trained: every asymmetric quantizer still carries the default q_type 0
    _raises(r"model\.10\.conv\.activation_quantizer \(AsymmetricQuantizer\) carries q_type 0", _folded(q_type=1))


def test_a_multi_valued_activation_zero_point_is_refused():
    m = _trained(_folded(q_type=1))
    m.model[6].conv.activation_quantizer.zero_point = torch.zeros(3)
    _raises(r"model\.6\.conv\.activation_quantizer carries 3 zero points", m)
    m = _trained(_folded(q_type=1))
    m.model[7].activation_quantizer.zero_point = torch.zeros(2)
    _raises(r"model\.7\.activation_quantizer carries 2 zero points", m)
    m = _trained(_folded(q_type=1))
    m.model[2].conv.weight_quantizer.zero_point = torch.zeros(1)
    _raises(r"model\.2\.conv\.weight_quantizer carries 1 zero points for 256 scales", m)
    # a symmetric quantizer with a zero point stays what it was: refused
    m = _folded()
    m.model[7].activation_quantizer.zero_point.fill_(3.0)
    _raises(r"model\.7\.activation_quantizer is asymmetric", m)


def test_a_cpu_model_is_refused_by_compile_only():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    m = _trained(_folded(q_type=1))
    assert inference.iao_int8_report(m, zero_points=True)
    with pytest.raises(MicronetHipError, match="no CPU fallback"):
        inference.iao_compile_int8(m, zero_points=True)


def test_the_entry_points_are_bound():
    from micronet_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "micronet_hip.h")).read()
    names = ("mn_i8zconv_supported", "mn_i8zconv_table_bytes", "mn_i8zconv_pack", "mn_i8zconv_fwd", "mn_i8z_pack_codes", "mn_i8z_unpack_codes")
    for name in names:
        assert name in _lib.PROTOTYPES and (name + "(") in header
    for name in names[2:]:          # the stream is the last argument
        assert _lib.PROTOTYPES[name][1][-1] is C.c_void_p
    q = C.POINTER(_lib.I8ZQuant)
    assert _lib.PROTOTYPES["mn_i8zconv_pack"][1][6:9] == [q, q, q] and _lib.PROTOTYPES["mn_i8z_pack_codes"][1][4] is q and _lib.PROTOTYPES["mn_i8z_unpack_codes"][1][4] is q
    assert [f for f, _ in _lib.I8ZQuant._fields_] == ["s", "z", "asym", "bits"]
