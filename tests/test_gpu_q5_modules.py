"""prepare(fuse_pool3=True, code_conv5=True) on W4A4 plain nin: the 96 -> 192 5x5 conv behind the first pool reads the pooled codes itself (k_q5_fwd) and leaves a
lazy output to its BatchNorm block; with the flag off it keeps the QActToFloat route, and both graphs are the same function."""
import pytest
import torch
import torch.nn as nn

from test_gpu_qa_pool3_modules import test_training_step_matches_unfused_pools as step_matches

pytestmark = pytest.mark.gpu


@pytest.fixture
def pair():
    from micronet.compression.quantization.wqaq.dorefa import quantize as Q
    from micronet_amd.train import build_model
    torch.manual_seed(0)
    base = build_model("nin")
    return (Q.prepare(base, a_bits=4, w_bits=4, fuse_pool3=True, code_conv5=True).cuda().train(),
            Q.prepare(base, a_bits=4, w_bits=4, fuse_pool3=True).cuda().train())


def test_conv5_route(pair):
    from micronet_amd import ops
    from micronet_amd.sign_tensor import LazyQConvOut, QActTensor
    from micronet_amd.train import synth_batch
    seen = {}
    for name, model in zip(("on", "off"), pair):
        assert isinstance(model.model[3], nn.MaxPool2d)
        conv = model.model[4].conv          # the block behind the first pool
        assert tuple(conv.kernel_size) == (5, 5) and conv.code_k5 is (name == "on")
        conv.register_forward_hook(lambda mod, args, out, name=name: seen.__setitem__(name, (type(args[0]), type(out))))
        ops.fallback_counts(reset=True)
        model(synth_batch(8, device="cuda")[0])
        assert not ops.fallback_counts(), ops.fallback_counts()
    assert seen["on"] == (QActTensor, LazyQConvOut), seen
    assert seen["off"][0] is QActTensor and seen["off"][1] is not LazyQConvOut, seen          # flag off: still the QActToFloat route


def test_training_step_matches_fp32_conv5(pair):
    """tolerances and exemptions of test_gpu_qa_pool3_modules, unchanged: 1e-6 logits, 2e-5 gradients, 2e-4 on the weight arg-max element, 2e-6 buffers; no fallback"""
    step_matches(pair)
