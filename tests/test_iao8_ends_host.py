"""Host-only behaviour of ``iao_int8_report(model, byte_ends=True)`` / the walk of ``iao_compile_int8(model, byte_ends=True)``: the stage report of the BN-folded
nin_gc with both ends on the int8 kernels, and every refusal of the two ends naming its layer -- without a GPU.  (Weights off the grid are read from the packed
tables: tests/test_gpu_iao8_ends_plan.py.)"""
import ctypes as C
import json
import os

import pytest
import torch.nn as nn

from conftest import GOLDEN
from test_iao8_host import NAMES, _folded


def test_iao8_ends_report_nin_gc_is_pinned():
    from micronet_amd import inference
    F = _folded()
    rep = inference.iao_int8_report(F, byte_ends=True)
    assert rep == json.load(open(os.path.join(GOLDEN, "iao8_ends_report_nin_gc.json")))
    default = inference.iao_int8_report(F)
    assert default == json.load(open(os.path.join(GOLDEN, "iao8_report_nin_gc.json"))), "the default report stays equal to its own golden"
    assert inference.iao_int8_report(F, byte_ends=False) == default
    assert rep[1:-1] == default[1:-1], "the hidden rows are the default report's"
    assert [r["kind"] for r in rep] == ["int8_first"] + ["int8"] * 7 + ["int8_last"]
    assert all(set(r) == NAMES for r in rep)
    assert rep[0]["kernel"] == "k_i8first<5>" and rep[-1]["kernel"] == "k_i8conv_f32<1>"
    assert rep[0]["table_bytes"] > 0 and rep[-1]["table_bytes"] > 0
    assert rep[0]["act_bytes_in"] == 4 * 3 * 32 * 32 and rep[0]["act_bytes_out"] == 256 * 32 * 32
    assert rep[-1]["act_bytes_in"] == 1024 * 8 * 8 and rep[-1]["act_bytes_out"] == 4 * 10 * 8 * 8
    assert rep[0]["out_order"] == default[0]["out_order"] and rep[-1]["out_order"] == "identity"
    for a, b in zip(rep[:-1], rep[1:]):
        assert a["act_bytes_out"] == b["act_bytes_in"], "one byte per activation across every boundary"


def _raises(match, model):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    assert inference.iao_int8_report(model), "the default walk does not look at the first block"
    with pytest.raises(MicronetHipError, match=match):
        inference.iao_int8_report(model, byte_ends=True)
    with pytest.raises(MicronetHipError, match=match):
        inference.iao_compile_int8(model, byte_ends=True)          # the same walk, before anything touches a GPU


def test_refuses_a_7x7_first_conv():
    m = _folded()
    m.model[0].conv.kernel_size, m.model[0].conv.padding = (7, 7), (3, 3)
    _raises(r"iao_compile_int8\(byte_ends=True\): model\.0\.conv: geometry not covered by mn_i8first_supported \(7x7, stride \(1, 1\), padding \(3, 3\)", m)


def test_refuses_an_asymmetric_or_32_bit_image_quantizer():
    m = _folded()
    m.model[0].conv.activation_quantizer.q_type = 1
    _raises(r"iao_compile_int8\(byte_ends=True\): model\.0\.conv\.activation_quantizer is asymmetric", m)
    m = _folded()
    m.model[0].conv.activation_quantizer.bits = 32
    _raises(r"iao_compile_int8\(byte_ends=True\): model\.0\.conv\.activation_quantizer has 32 bits", m)


def test_refuses_a_first_block_that_is_not_quant_inference():
    m = _folded()
    m.model[0].conv.quant_inference = False
    _raises(r"iao_compile_int8\(byte_ends=True\): model\.0\.conv is not quant_inference", m)


def test_refuses_a_grouped_last_conv_the_kernel_does_not_cover():
    m = _folded()
    m.model[10].conv.groups = 128
    _raises(r"iao_compile_int8\(byte_ends=True\): model\.10\.conv: geometry not covered by mn_i8conv_supported, the rule of mn_i8conv_fwd_f32 \(1x1, .*groups 128, "
            r"8 channels per group", m)


def test_refuses_a_pool_directly_behind_the_first_block():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    m = _folded()
    kids = list(m.model.children())
    seq = nn.Sequential(kids[0], kids[3], *kids[1:3], *kids[4:])
    for call in (inference.iao_int8_report, inference.iao_compile_int8):
        with pytest.raises(MicronetHipError, match=r"iao_compile_int8\(byte_ends=True\): 1: a max-pool directly behind the first block is not covered \(the pooled form"):
            call(seq, byte_ends=True)


def test_the_entry_points_of_the_two_ends_are_bound():
    from micronet_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "micronet_hip.h")).read()
    for name in ("mn_i8first_supported", "mn_i8first_table_bytes", "mn_i8first_pack", "mn_i8first_fwd", "mn_i8conv_fwd_f32"):
        assert name in _lib.PROTOTYPES and (name + "(") in header
    for name in ("mn_i8first_pack", "mn_i8first_fwd", "mn_i8conv_fwd_f32"):          # the stream is the last argument
        assert _lib.PROTOTYPES[name][1][-1] is C.c_void_p
    assert len(_lib.PROTOTYPES["mn_i8first_pack"][1]) == 13 and len(_lib.PROTOTYPES["mn_i8first_fwd"][1]) == 8 and len(_lib.PROTOTYPES["mn_i8conv_fwd_f32"][1]) == 8
