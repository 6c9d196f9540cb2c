"""Host-only behaviour of ``dorefa_bytes_report(model, tile_blocks=True)``: the stage report of W8A8 plain nin, the new named refusals, and that the keyword changes
nothing for nin_gc -- without a GPU."""
import pytest
import torch.nn as nn

from test_codes_host import _prepared


def _nin(cfg=None, edit=None):
    """Plain nin, its children rearranged by ``edit(kids) -> kids``, prepared W8A8."""
    from micronet_amd.models import nin
    net = nin.Net(cfg=cfg)
    if edit:
        net.model = nn.Sequential(*edit(list(net.model.children())))
    return _prepared(net=net, bits=8)


def test_bytes_report_nin():
    from micronet_amd import inference
    rep = inference.dorefa_bytes_report(_nin(), tile_blocks=True)
    assert [r["kind"] for r in rep] == ["first"] + ["byte"] * 7 + ["last"]
    by = {r["name"]: r for r in rep}
    assert by["model.4"]["kernel"] == "k_code8conv5<5>" and by["model.4"]["K"] == 96 * 25 and by["model.4"]["pooled"] is False
    assert by["model.2"]["kernel"] == by["model.6"]["kernel"] == "k_code8conv<1,0>, k_code8_maxpool"
    assert by["model.2"]["pooled"] == by["model.6"]["pooled"] == "standalone" and (by["model.2"]["stage"], by["model.6"]["stage"]) == ("3", "7")
    ends = inference.dorefa_bytes_report(_nin(), byte_ends=True, tile_blocks=True)
    assert ends[1:-1] == rep[1:-1] and (ends[0]["kernel"], ends[-1]["kernel"]) == ("k_c1b_fwd<2,5>", "k_code8conv_f32")
    assert inference.dorefa_bytes_report(_prepared(bits=8), tile_blocks=True) == inference.dorefa_bytes_report(_prepared(bits=8)), "nin_gc: the keyword changes nothing"


@pytest.mark.parametrize("model, pattern", [
    (lambda: _nin(edit=lambda k: k[:4] + [type(k[4])(96, 192, kernel_size=5, stride=1, padding=2, groups=2)] + k[5:]),
     r"model\.4\.conv: a grouped 5x5 block \(groups 2\) is not covered by mn_code8conv5_supported"),
    (lambda: _nin([32, 32, 1328, 32, 32, 32, 32, 32]), r"model\.4\.conv: a 5x5 block of 1328 input channels is beyond the bounds of mn_code8conv5_supported .*C \* 25 <= 33025"),
    (lambda: _nin([32, 32, 1232, 32, 32, 32, 32, 32]), r"model\.4\.conv: a 5x5 block of 1232 input channels is beyond the bounds .*one output row with its halo in 48 KB of LDS"),
    (lambda: _nin(edit=lambda k: k[:4] + [nn.MaxPool2d(3, 2, 1)] + k[4:]), r"model\.4: two max-pools in a row are not covered \(one pool behind a byte block\)"),
    (lambda: _nin(edit=lambda k: [k[0], nn.MaxPool2d(3, 2, 1)] + k[1:]), r"model\.1: a max-pool directly behind the first block is not covered"),
    (lambda: _nin(edit=lambda k: k[:3] + [nn.MaxPool2d(3, 1, 1)] + k[4:]), r"model\.3: max-pool \(kernel .*\) is not covered by the byte kernels \(2x2 / 2 / 0 and 3x3 / 2 / 1"),
], ids=["grouped_5x5", "k_bound", "lds_bound", "two_pools", "pool_behind_first", "pool_kind"])
def test_new_refusals_name_the_layer_and_the_rule(model, pattern):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=r"dorefa_compile_bytes\(tile_blocks=True\): " + pattern):
        inference.dorefa_bytes_report(model(), tile_blocks=True)
