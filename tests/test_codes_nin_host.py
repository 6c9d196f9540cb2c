"""Host-only behaviour of ``dorefa_codes_report(model, tile_blocks=True)`` / the walk of ``dorefa_compile_codes(model, tile_blocks=True)``: the stage report of plain
nin, what stays refused, and that the keyword changes nothing for nin_gc -- without a GPU."""
import json
import os

import pytest
import torch.nn as nn

from conftest import GOLDEN
from test_codes_host import _prepared

NAMES = {"name", "kind", "K", "words", "planes", "kernel", "pooled", "out_order", "stage"}


def _golden(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def _nin(cfg=None):
    from micronet_amd.models import nin
    return nin.Net(cfg=cfg)


def _refused(net, pattern, **kw):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=pattern):
        inference.dorefa_codes_report(_prepared(net=net), tile_blocks=True, **kw)


def test_codes_report_nin_is_pinned():
    from micronet_amd import inference
    rep = inference.dorefa_codes_report(_prepared("nin"), tile_blocks=True)
    assert rep == _golden("codes_report_nin.json")
    assert [r["kind"] for r in rep] == ["first"] + ["code"] * 7 + ["last"]
    assert all(set(r) == NAMES for r in rep)
    by = {r["name"]: r for r in rep}
    assert by["model.2"]["pooled"] == by["model.6"]["pooled"] == "standalone"
    assert by["model.2"]["kernel"] == by["model.6"]["kernel"] == "k_codeconv<1,0,0>, k_codes_maxpool"
    assert (by["model.2"]["stage"], by["model.6"]["stage"]) == ("3", "7"), "the stage of a pooled block is the pool's"
    assert by["model.4"]["kernel"] == "k_codeconv_tile<5,3>" and by["model.4"]["K"] == 96 * 25 and by["model.4"]["pooled"] is False
    assert [r["pooled"] for r in rep].count(False) == 7


def test_codes_ends_report_nin_is_pinned():
    from micronet_amd import inference
    rep = inference.dorefa_codes_report(_prepared("nin"), code_ends=True, tile_blocks=True)
    assert rep == _golden("codes_ends_report_nin.json")
    base = _golden("codes_report_nin.json")
    assert rep[1:-1] == base[1:-1], "every hidden row is the default report's"
    assert "k_c1b_fwd" in rep[0]["kernel"] and "k_planesconv1x1_small" in rep[-1]["kernel"]
    assert not any("pack" in r["kernel"] for r in rep)


def test_narrow_nin_takes_the_rolled_tile_kernel():
    from micronet_amd import inference
    rep = inference.dorefa_codes_report(_prepared(net=_nin([32, 32, 32, 64, 64, 64, 64, 64])), tile_blocks=True)
    assert {r["name"]: r["kernel"] for r in rep}["model.4"] == "k_codeconv_tile<5,0>"


@pytest.mark.parametrize("code_ends", [False, True])
def test_keyword_off_refuses_plain_nin_as_before(code_ends):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    for kw in ({}, {"tile_blocks": False}):
        with pytest.raises(MicronetHipError, match=r"model\.4\.conv: geometry not covered by mn_codeconv_supported \(5x5.*tile_blocks=True"):
            inference.dorefa_codes_report(_prepared("nin"), code_ends=code_ends, **kw)
    with pytest.raises(MicronetHipError, match=r"model\.4\.conv: geometry not covered by mn_codeconv_supported \(5x5"):
        inference.dorefa_compile_codes(_prepared("nin"), code_ends=code_ends)


def test_keyword_off_refuses_the_unfused_pool_as_before():
    """Without the 5x5 block in the way the walk reaches the block in front of the 3x3 / 2 pool and refuses it with today's words."""
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    net = _nin()
    kids = list(net.model.children())
    kids[4] = type(kids[4])(96, 192, kernel_size=3, stride=1, padding=1)
    net.model = nn.Sequential(*kids)
    with pytest.raises(MicronetHipError, match=r"model\.2: its output is not handed over as 2-bit codes"):
        inference.dorefa_codes_report(_prepared(net=net))
    rep = inference.dorefa_codes_report(_prepared(net=net), tile_blocks=True)
    assert {r["name"]: r["kernel"] for r in rep}["model.4"] == "k_codeconv<3,0,0>"


@pytest.mark.parametrize("code_ends", [False, True])
def test_nin_gc_reports_do_not_change_with_the_keyword(code_ends):
    from micronet_amd import inference
    want = _golden("codes_ends_report_nin_gc.json" if code_ends else "codes_report_nin_gc.json")
    assert inference.dorefa_codes_report(_prepared(), code_ends=code_ends, tile_blocks=True) == want
    first, layers, last, tail, flatten, report = inference._walk_codes(_prepared(), code_ends, True)
    assert not any(L["tile"] or L["pool_ksp"] for L in layers) and [L["pool"] for L in layers].count(1) == 2, "the 2x2 fold of nin_gc is untouched"


def test_refuses_a_pool_behind_the_first_block():
    net = _nin()
    kids = list(net.model.children())
    net.model = nn.Sequential(kids[0], nn.MaxPool2d(3, 2, 1), *kids[1:])
    _refused(net, r"model\.1: a max-pool directly behind the first block is not covered")
    _refused(net, r"model\.1: a max-pool directly behind the first block is not covered", code_ends=True)


def test_refuses_two_pools_in_a_row():
    net = _nin()
    kids = list(net.model.children())
    net.model = nn.Sequential(*kids[:4], nn.MaxPool2d(3, 2, 1), *kids[4:])
    _refused(net, r"model\.4: two max-pools in a row")
    from micronet_amd.models import nin_gc
    net = nin_gc.Net(cfg=[32, 32, 32, 64, 64, 64, 128, 128])
    kids = list(net.model.children())
    net.model = nn.Sequential(*kids[:4], nn.MaxPool2d(2, 2), *kids[4:])
    _refused(net, r"model\.4: two max-pools in a row")


def test_refuses_ceil_mode_and_other_pool_shapes():
    for pool in (nn.MaxPool2d(3, 2, 1, ceil_mode=True), nn.MaxPool2d(3, 1, 1), nn.MaxPool2d(2, 2, 1), nn.MaxPool2d(3, 2, 0), nn.MaxPool2d(3, 2, 1, dilation=2)):
        net = _nin()
        kids = list(net.model.children())
        kids[3] = pool
        net.model = nn.Sequential(*kids)
        _refused(net, r"model\.3: max-pool \(kernel .*\) is not covered by the code kernels")


def test_refuses_a_pool_without_a_quantised_block_behind_it():
    net = _nin()
    kids = list(net.model.children())
    net.model = nn.Sequential(*kids[:4], nn.Dropout(0.5), *kids[4:])
    _refused(net, r"model\.4 \(Dropout\): module order not recognised")


def test_refuses_a_5x5_block_beyond_the_k_bound():
    _refused(_nin([192, 160, 146, 192, 192, 192, 192, 192]), r"model\.4\.conv: a 5x5 block of 146 input channels is beyond the bound .*C \* 25 \* 9 <= 32767: at most 145 channels")
    from micronet_amd import inference
    rep = inference.dorefa_codes_report(_prepared(net=_nin([192, 160, 145, 192, 192, 192, 192, 192])), tile_blocks=True)
    assert {r["name"]: r for r in rep}["model.4"]["kernel"] == "k_codeconv_tile<5,0>"


def test_refuses_a_grouped_5x5_block():
    net = _nin()
    kids = list(net.model.children())
    kids[4] = type(kids[4])(96, 192, kernel_size=5, stride=1, padding=2, groups=2)
    net.model = nn.Sequential(*kids)
    _refused(net, r"model\.4\.conv: a grouped 5x5 block \(groups 2\) is not covered")


def test_refuses_a_5x5_block_without_same_padding():
    net = _nin()
    kids = list(net.model.children())
    kids[4] = type(kids[4])(96, 192, kernel_size=5, stride=1, padding=1)
    net.model = nn.Sequential(*kids)
    _refused(net, r"model\.4\.conv: geometry not covered by mn_codeconv_supported \(5x5, padding 1")


def test_consumer_behind_the_pool_must_read_2_bit_codes():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    m = _prepared("nin")
    m.model[4].conv.activation_quantizer.a_bits = 4
    with pytest.raises(MicronetHipError, match=r"model\.4\.conv has a_bits = 4"):
        inference.dorefa_codes_report(m, tile_blocks=True)


def test_plan_is_built_from_the_walk_and_eval_only():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    first, layers, last, tail, flatten, report = inference._walk_codes(_prepared("nin"), False, True)
    assert [L["name"] for L in layers if L["tile"]] == ["model.4"]
    assert {L["name"]: L["pool_ksp"] for L in layers if L["pool_ksp"]} == {"model.2": (3, 2, 1), "model.6": (3, 2, 1)}
    assert not any(L["pool"] for L in layers), "nothing is folded in plain nin"
    plan = inference.CodePlan(first, layers, last, tail, flatten, report)
    assert not plan.training and len(plan.tail) == 1
    with pytest.raises(MicronetHipError, match="eval-only"):
        plan.train()


def test_compile_names_the_first_layer_whose_weights_are_off_the_grid():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=r"model\.1\.conv: the stored weights were not found on the 2-bit grid"):
        inference.dorefa_compile_codes(_prepared("nin"), tile_blocks=True)          # never pre-quantised


def test_nin_entry_points_are_declared_and_bound():
    from micronet_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "micronet_hip.h")).read()
    for name in ("mn_codeconv_tile_supported", "mn_codeconv_tile_table_bytes", "mn_codeconv_tile_pack", "mn_codeconv_tile_fwd", "mn_codes_maxpool"):
        assert name in _lib.PROTOTYPES and (name + "(") in header
