"""Host-only behaviour of ``dorefa_bytes_report(model, byte_ends=True)`` / the walk of ``dorefa_compile_bytes(model, byte_ends=True)``: the two end rows of W8A8 nin_gc,
the named refusals, and that the keyword is off by default -- without a GPU."""
import pytest

from micronet_amd.models import nin_gc
from test_codes_ends_host import _last_block_index, _replace_conv
from test_codes_host import _prepared

_narrow_net = lambda: nin_gc.Net(cfg=[160, 224, 256, 448, 384, 512, 896, 768])          # the narrow net of tests/test_gpu_codes_w8_plan.py: every group a multiple of 16 channels


def test_bytes_report_with_byte_ends_names_the_two_kernels():
    from micronet_amd import inference
    base, rep = inference.dorefa_bytes_report(_prepared(bits=8)), inference.dorefa_bytes_report(_prepared(bits=8), byte_ends=True)
    assert inference.dorefa_bytes_report(_prepared(bits=8), byte_ends=False) == base and base[0]["kernel"] == "first conv + k_qa_fwd, k_code8_pack"
    assert rep[1:-1] == base[1:-1] and len(rep) == len(base) == 9
    assert rep[0] == dict(base[0], kernel="k_c1b_fwd<2,5>") and rep[-1] == dict(base[-1], kernel="k_code8conv_f32")          # 256 first channels: two blocks of 128
    narrow = inference.dorefa_bytes_report(_prepared(net=_narrow_net(), bits=8), byte_ends=True)
    assert narrow[0]["kernel"] == "k_c1b_fwd<2,5>" and narrow[-1]["kernel"] == "k_code8conv_f32" and inference._first_bytes_kernel_name(64) == "k_c1b_fwd<1,5>"


@pytest.mark.parametrize("edit, pattern", [          # (what is done to the narrow net's blocks `first` and `last`, the message naming the layer)
    (lambda first, last: _replace_conv(first, stride=2), r"byte_ends=True\): model\.0\.conv: not covered by mn_conv2d_first_bytes \(5x5, stride 2"),
    (lambda first, last: _replace_conv(last, kernel_size=3, padding=1), r"byte_ends=True\): model\.%d\.conv: the last conv is not the small 1x1 classifier mn_code8conv_fwd_f32 covers \(3x3"),
    (lambda first, last: _replace_conv(last, stride=2), r"byte_ends=True\): model\.%d\.conv: the last conv is not the small 1x1 classifier mn_code8conv_fwd_f32 covers \(1x1, stride 2"),
    (lambda first, last: _replace_conv(last, groups=2), r"byte_ends=True\): model\.%d\.conv: the last conv is not the small 1x1 classifier mn_code8conv_fwd_f32 covers \(1x1, stride 1, padding \(0, 0\), groups 2"),
    (lambda first, last: setattr(last, "channel_shuffle_flag", 1) or setattr(last, "shuffle_groups", 2), r"model\.%d: a channel shuffle in front of the last block is not covered"),
], ids=["strided_first", "k3_last", "strided_last", "grouped_last", "shuffled_last"])
def test_byte_ends_refusals_name_the_layer(edit, pattern):
    from micronet_amd import _lib, inference
    net = _narrow_net()
    i = _last_block_index(net)
    edit(net.model[0], net.model[i])
    with pytest.raises(_lib.MicronetHipError, match=pattern % i if "%d" in pattern else pattern):
        inference.dorefa_bytes_report(_prepared(net=net, bits=8), byte_ends=True)
