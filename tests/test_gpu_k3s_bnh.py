"""The grouped 3x3 binary block's backward on the MI355X: k_k3s_dgrad<1> / k_k3s_wgrad<0, 1> form dy from (da, h) -- kernel level (tests/k3s_bnh_cases.py, the
emulated run's cases + nin_gc's layers 4 and 7 at batch 8) and module level (ops.FOLD_BN_INTO_CONV_BWD on / off on one prepared block)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import abi_driver
import k3s_bnh_cases as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


NIN_GC = [
    dict(x_shape=(8, 256, 16, 16), w_shape=(512, 16, 3, 3), groups=16),        # layer 4
    dict(x_shape=(8, 512, 8, 8), w_shape=(1024, 16, 3, 3), groups=32),         # layer 7
]


@pytest.mark.parametrize("case", range(len(B.CASES)))
def test_k3s_bnh_matches_two_step_path(be, case):
    B.check(be, seed=300 + case, **B.CASES[case])


def test_k3s_bnh_blocks_walk_several_stages(be):
    B.check(be, seed=310, **B.CASE_LONG)


@pytest.mark.parametrize("case", range(len(NIN_GC)))
def test_k3s_bnh_nin_gc_layers(be, case):
    B.check(be, seed=320 + case, **NIN_GC[case])


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


def test_bn_backward_folded_into_3x3_conv_backward_matches():
    """One grouped 3x3 ConvBNReLU block of the wbwtab scheme (A=2, W=3), teacher-forced: with ops.FOLD_BN_INTO_CONV_BWD the block's dy is formed inside
    k_k3s_dgrad<1> / k_k3s_wgrad<0, 1>, without it mn_bnh_bwd_apply writes it.  The kernel-level results are bit-equal; the bound here is the one of
    test_gpu_modules.test_bn_backward_folded_into_conv_backward_matches."""
    import importlib
    from micronet_amd import ops
    from micronet_amd.models.nin_gc import ConvBNReLU
    from micronet_amd.sign_tensor import SignTensor
    w = importlib.import_module("micronet.compression.quantization.wbwtab.quantize")
    torch.manual_seed(23)
    net = nn.Sequential(ConvBNReLU(3, 64, 3, padding=1), ConvBNReLU(64, 128, 3, padding=1, groups=4, channel_shuffle=1, shuffle_groups=2),
                        ConvBNReLU(128, 10, 1), nn.AvgPool2d(8)).cuda().train()
    q = w.prepare(net, inplace=True, A=2, W=3)
    blk = q[1]
    codes = (torch.randint(0, 2, (8, 64, 8, 8), device="cuda", dtype=torch.int8) * 2 - 1)
    gout = torch.randn(8, 128, 8, 8, device="cuda")
    res, kern = {}, {}
    old, real = ops.FOLD_BN_INTO_CONV_BWD, ops._call
    for fold in (True, False):
        ops.FOLD_BN_INTO_CONV_BWD = fold
        seen_k = kern[fold] = {}
        ops._call = lambda name, *a, _k=seen_k: (real(name, *a), _k.__setitem__(name, ops.last_kernel()))[0]          # library call -> the kernel it launched
        try:
            for p_ in blk.parameters():
                p_.grad = None
            x = SignTensor(codes.clone()).requires_grad_(True)
            blk(x).backward(gout)
            res[fold] = [x.grad.clone()] + [p_.grad.clone() for n_, p_ in blk.named_parameters() if n_ != "conv.bias"]
        finally:
            ops.FOLD_BN_INTO_CONV_BWD, ops._call = old, real
    assert kern[True].get("mn_conv2d_bwd_data_bnh") == "k_k3s_dgrad<1>" and kern[True].get("mn_conv2d_bwd_weight_bnh") == "k_k3s_wgrad<0, 1>", kern[True]
    assert "mn_bnh_bwd_apply" not in kern[True] and "mn_bnh_bwd_apply" in kern[False] and "mn_conv2d_bwd_data_bnh" not in kern[False], kern
    for a_, b_ in zip(res[True], res[False]):
        assert torch.isfinite(a_).all() and a_.abs().max().item() > 0
        assert rel_err(a_.cpu(), b_.cpu()) <= 1e-5
    # a backward hook on the conv is a foreign consumer of dy: it sees the expanded tensor (mn_bnh_bwd_apply), and the gradients stay the same
    seen = {}
    hk = blk.conv.register_full_backward_hook(lambda m, gi, go: seen.__setitem__("go", (go[0] * 1.0).clone()))
    for p_ in blk.parameters():
        p_.grad = None
    x = SignTensor(codes.clone()).requires_grad_(True)
    blk(x).backward(gout)
    hk.remove()
    assert torch.isfinite(seen["go"]).all() and seen["go"].abs().sum().item() > 0
    assert rel_err(x.grad.cpu(), res[False][0].cpu()) <= 1e-5
