"""Host-only behaviour of ``dorefa_codes_report(model, code_ends=True)`` / the walk of ``dorefa_compile_codes(model, code_ends=True)``: the stage report of nin_gc and
what the walk refuses for the two plane ends, without a GPU."""
import json
import os

import pytest
import torch.nn as nn

from conftest import GOLDEN
from test_codes_host import _prepared

SMALL_CFG = [32, 32, 32, 64, 64, 64, 128, 128]


def _golden(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def test_codes_ends_report_nin_gc_is_pinned():
    from micronet_amd import inference
    rep = inference.dorefa_codes_report(_prepared(), code_ends=True)
    assert rep == _golden("codes_ends_report_nin_gc.json")
    base = _golden("codes_report_nin_gc.json")
    assert rep[1:-1] == base[1:-1], "every hidden row is the default report's"
    for i in (0, -1):
        assert {k: v for k, v in rep[i].items() if k != "kernel"} == {k: v for k, v in base[i].items() if k != "kernel"}
    assert "k_c1b_fwd" in rep[0]["kernel"] and "k_planesconv1x1_small" in rep[-1]["kernel"]
    assert not any("pack" in r["kernel"] for r in rep)


def test_codes_report_without_code_ends_is_the_existing_golden():
    from micronet_amd import inference
    base = _golden("codes_report_nin_gc.json")
    assert inference.dorefa_codes_report(_prepared(), code_ends=False) == base
    assert inference.dorefa_codes_report(_prepared()) == base


def _small_net():
    from micronet_amd.models import nin_gc
    return nin_gc.Net(cfg=SMALL_CFG)


def _refused(net, pattern, bits=2):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=pattern):
        inference.dorefa_codes_report(_prepared(net=net, bits=bits), code_ends=True)


def test_code_ends_accepts_the_small_net():
    from micronet_amd import inference
    rep = inference.dorefa_codes_report(_prepared(net=_small_net()), code_ends=True)
    assert [r["kind"] for r in rep] == ["first"] + ["code"] * 7 + ["last"]


def test_code_ends_refuses_a_pool_behind_the_first_block():
    net = _small_net()
    kids = list(net.model.children())
    net.model = nn.Sequential(kids[0], nn.MaxPool2d(2, 2), *kids[1:])
    _refused(net, r"model\.0: a 2x2 max-pool is folded only into a code block")


def _last_block_index(net):
    return max(i for i, m in enumerate(net.model.children()) if isinstance(getattr(m, "conv", None), nn.Conv2d))


def _replace_conv(block, **kw):
    c = block.conv
    a = dict(in_channels=c.in_channels, out_channels=c.out_channels, kernel_size=c.kernel_size, stride=c.stride, padding=c.padding, groups=c.groups)
    a.update(kw)
    block.conv = nn.Conv2d(**a)
    if "out_channels" in kw:
        block.bn = nn.BatchNorm2d(kw["out_channels"])


def test_code_ends_refuses_a_last_conv_with_17_outputs():
    net = _small_net()
    i = _last_block_index(net)
    _replace_conv(net.model[i], out_channels=17)
    _refused(net, r"model\.%d\.conv: the last conv is not the small 1x1 classifier" % i)


def test_code_ends_refuses_a_3x3_last_conv():
    net = _small_net()
    i = _last_block_index(net)
    _replace_conv(net.model[i], kernel_size=3, padding=1)
    _refused(net, r"model\.%d\.conv: the last conv is not the small 1x1 classifier" % i)


def test_code_ends_refuses_a_shuffle_in_front_of_the_last_block():
    net = _small_net()
    i = _last_block_index(net)
    net.model[i].channel_shuffle_flag, net.model[i].shuffle_groups = 1, 2
    _refused(net, r"model\.%d: a channel shuffle in front of the last" % i)


def test_code_ends_refuses_a_first_block_handing_over_4_bit_codes():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    m = _prepared(net=_small_net())
    m.model[0].bn.q_out_bits = 4
    with pytest.raises(MicronetHipError, match=r"model\.0: the first block must hand over 2-bit activation codes"):
        inference.dorefa_codes_report(m, code_ends=True)


def test_code_ends_refuses_a_strided_first_conv():
    net = _small_net()
    _replace_conv(net.model[0], stride=2)
    _refused(net, r"model\.0\.conv: not covered by mn_conv2d_first_codes \(5x5, stride 2")


def test_code_end_entry_points_are_declared_and_bound():
    from micronet_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "micronet_hip.h")).read()
    for name in ("mn_conv2d_first_codes_supported", "mn_conv2d_first_codes_table_bytes", "mn_conv2d_first_codes_pack", "mn_conv2d_first_codes",
                 "mn_planesconv1x1_small_supported", "mn_planesconv1x1_small_fwd"):
        assert name in _lib.PROTOTYPES and (name + "(") in header
