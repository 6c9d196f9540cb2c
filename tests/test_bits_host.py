"""Host-only behaviour of micronet_amd.inference.wbwtab_compile_bits: what it refuses, without a GPU."""
import pytest
import torch


def _folded(prequantize, W=3):
    from micronet.compression.quantization.wbwtab import quantize as Q
    from micronet_amd import inference
    from micronet_amd.models import nin_gc
    torch.manual_seed(0)
    I = Q.prepare(nin_gc.Net(cfg=[32, 32, 32, 64, 64, 64, 128, 128]), inplace=True, A=2, W=W, quant_inference=True)
    if prequantize:
        # (CPU: the quantizer kernels need the GPU; store codes x alpha by hand, as the weight quantizer would, and record the verdict)
        for m in I.modules():
            if isinstance(m, Q.QuantConv2d):
                w = m.weight.detach()
                m.weight.data = torch.sign(w) * w.abs().flatten(1).mean(1).reshape(-1, 1, 1, 1)
                inference.mark_stored_codes(m)
    return inference.wbwtab_model_bn_fuse(I, W=W).eval()


def test_compile_bits_refuses_a_cpu_model():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    F = _folded(True)
    with pytest.raises(MicronetHipError, match="no CPU fallback"):
        inference.wbwtab_compile_bits(F)


def test_compile_bits_names_the_first_layer_that_is_not_prequantised():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    F = _folded(False)
    with pytest.raises(MicronetHipError, match=r"model\.1\.conv.*not codes x alpha"):
        inference.wbwtab_compile_bits(F)


def test_compile_bits_refuses_an_unknown_module_order():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match="not recognised"):
        inference.wbwtab_compile_bits(torch.nn.Sequential(torch.nn.Conv2d(3, 8, 1), torch.nn.ReLU()))


def test_bit_entry_points_are_declared_and_exported():
    from micronet_amd import _lib
    for name in ("mn_bits_pack_sign8", "mn_bits_unpack_sign8", "mn_bitconv_supported", "mn_bitconv_table_bytes", "mn_bitconv_pack", "mn_bitconv_fwd"):
        assert name in _lib.PROTOTYPES
