"""Host-only behaviour of ``bit_ends=True`` (micronet_amd.inference.wbwtab_bits_report / wbwtab_compile_bits): which report rows change, what is refused -- without a GPU."""
import pytest
import torch.nn as nn

from test_bits_host import _folded as _folded_nin_gc
from test_bits_nin_host import SMALL, _folded, _nin


def _check_rows(F):
    from micronet_amd import inference
    r0, r1 = inference.wbwtab_bits_report(F), inference.wbwtab_bits_report(F, bit_ends=True)
    assert r0 == inference.wbwtab_bits_report(F, bit_ends=False), "the default is bit_ends=False"
    assert len(r1) == len(r0)
    diff = [(i, k) for i, (a, b) in enumerate(zip(r0, r1)) for k in set(a) | set(b) if a.get(k) != b.get(k)]
    assert sorted(diff) == [(0, "kernel"), (len(r0) - 1, "kernel")], diff
    assert r1[0]["kernel"] == "first conv -> bits (k_c1b_fwd)" and r1[-1]["kernel"] == "last conv on bits (k_bitsconv1x1_small)"
    assert r0[0]["kernel"] == "first conv + mn_bnsign_fwd_i8, k_bits_pack" and r0[-1]["kernel"] == "k_bits_unpack, last conv on sign codes"


@pytest.mark.parametrize("W", [3, 2])
def test_report_of_nin_gc_differs_in_the_two_end_rows_only(W):
    _check_rows(_folded_nin_gc(True, W=W))


@pytest.mark.parametrize("W", [3, 2])
def test_report_of_nin_differs_in_the_two_end_rows_only(W):
    _check_rows(_folded(_nin(), W=W))
    _check_rows(_folded(_nin(SMALL), W=W))


def _swap_conv(net, idx, **kw):
    c = net.model[idx].conv
    args = dict(kernel_size=c.kernel_size, stride=c.stride, padding=c.padding, groups=c.groups)
    args.update(kw)
    net.model[idx].conv = nn.Conv2d(c.in_channels, c.out_channels, **args)
    return net


def test_a_3x3_last_conv_is_refused_by_name_with_bit_ends_only():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    F = _folded(_swap_conv(_nin(SMALL), 10, kernel_size=3, padding=1))
    rep = inference.wbwtab_bits_report(F)
    assert rep[-1]["kind"] == "last" and rep[-1]["name"] == "model.10" and rep[-1]["K"] == 9 * 64
    with pytest.raises(MicronetHipError, match=r"bit_ends=True.*model\.10\.conv.*3x3"):
        inference.wbwtab_bits_report(F, bit_ends=True)
    with pytest.raises(MicronetHipError, match=r"model\.10\.conv"):
        inference.wbwtab_compile_bits(F, bit_ends=True)


def test_a_first_conv_the_kernel_refuses_is_refused_by_name_with_bit_ends_only():
    """7x7 over 3 channels: 147 taps per output, more than the first-layer kernels contract."""
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    F = _folded(_swap_conv(_nin(SMALL), 0, kernel_size=7, padding=3))
    assert inference.wbwtab_bits_report(F)[0]["K"] == 147
    with pytest.raises(MicronetHipError, match=r"bit_ends=True.*model\.0\.conv.*147 taps"):
        inference.wbwtab_bits_report(F, bit_ends=True)


def test_new_entry_points_are_declared_and_exported():
    from micronet_amd import _lib
    lib = _lib.get_lib()
    for name in ("mn_conv2d_first_sign_bits_supported", "mn_conv2d_first_sign_bits", "mn_bitsconv1x1_small_supported", "mn_bitsconv1x1_small_fwd"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
