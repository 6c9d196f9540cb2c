"""nn.MaxPool2d(3, 2, 1) through the three pool modules prepare() installs (MaxPool2dSign, MaxPool2dF32, QuantMaxPool2d) and through one training step of plain nin:
the overlapping pools run on this library's kernels (csrc/pool3s2.h), never on the stock operator."""
import importlib

import numpy as np
import pytest
import torch

from oracle import np_oracle as O
from pool3_cases import F, judge, make_x, same_bits
from test_gpu_models import CFG

pytestmark = pytest.mark.gpu

SCHEMES = {"wbwtab": "c2_nin_gc_wbwtab_w3a2", "dorefa": "nin_dorefa_w4a4", "iao": "c3_nin_gc_iao_w8a8_bnfuse"}


@pytest.mark.parametrize("shape", [(2, 5, 16, 16), (2, 3, 7, 9)], ids=["16x16", "7x9"])
@pytest.mark.parametrize("scheme", list(SCHEMES))
def test_pool_module_3x3s2(scheme, shape):
    """Output and input gradient of each scheme's pool module equal the float64 judge of tests/pool3_cases.py bit for bit, and nothing is noted as a fall-through.
    iao: x lies on the grid k / 64 with max |x| = 127.5 / 64, so the observer's first scale is exactly 1 / 64 and (g * s) / s is g."""
    from micronet_amd import ops
    from micronet_amd.sign_tensor import SignTensor
    ops.fallback_counts(reset=True)
    Ho, Wo = (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1
    gy = np.random.default_rng(9500).integers(-8, 9, size=shape[:2] + (Ho, Wo)).astype(F)
    mask = None
    if scheme == "wbwtab":
        from micronet_amd.quantization.wbwtab.quantize import MaxPool2dSign
        x = xq = make_x(shape, "pm1", 9501)
        pool, inp = MaxPool2dSign(3, 2, 1), SignTensor(torch.from_numpy(x.astype(np.int8)).cuda()).requires_grad_()
    elif scheme == "dorefa":
        from micronet_amd.quantization.wqaq.dorefa.quantize import MaxPool2dF32
        x = xq = make_x(shape, "ties", 9502)
        pool, inp = MaxPool2dF32(3, 2, 1), torch.from_numpy(x).cuda().requires_grad_()
    else:
        from micronet_amd.quantization.wqaq.iao.quantize import QuantMaxPool2d
        x = (np.random.default_rng(9503).integers(-127, 128, size=shape) / 64).astype(F)
        x[0, 0, 0, 0] = F(127.5 / 64)
        sc, zp = O.iao_qparams(x.min(), x.max(), 8, 0, True)
        assert sc == F(1 / 64) and zp == 0
        xq = O.iao_fq_fwd(x, sc, zp, 8, 0, True)[0]
        mask = O.iao_fq_bwd(np.ones_like(x), x, sc, zp, x.min(), x.max(), 8, 0, True)
        pool, inp = QuantMaxPool2d(3, 2, 1, a_bits=8, q_type=0).cuda().train(), torch.from_numpy(x).cuda().requires_grad_()
    want_y, want_dx = judge(xq, gy, mask)
    out = pool(inp)
    (dx,) = torch.autograd.grad(out, inp, torch.from_numpy(gy).cuda())
    got_y = (out.codes if scheme == "wbwtab" else out).detach().float().cpu().numpy()
    assert same_bits(got_y, want_y) and same_bits(dx.cpu().numpy(), want_dx)
    assert not any("maxpool" in k.lower().replace("_", "") for k in ops.fallback_counts()), ops.fallback_counts()
    if scheme == "iao":
        mm, count = out._mn_minmax[:2]
        assert float(mm[:count].min()) == want_y.min() and float(mm[count:].max()) == want_y.max() and out._mn_qgrid[1:3] == (8, 0)


@pytest.mark.parametrize("scheme", list(SCHEMES))
def test_plain_nin_pools_stay_on_the_library(scheme):
    """One training step of plain nin (models/nin.py: two nn.MaxPool2d(3, 2, 1)) at batch 8 notes no max-pool fall-through in any scheme."""
    from micronet_amd import ops
    from micronet_amd.train import build_model, make_optimizer, synth_batch, train_step
    _, name, kw, _, wd = CFG[SCHEMES[scheme]]
    quantize = importlib.import_module("micronet.compression.quantization.%s.quantize" % name)
    model = quantize.prepare(build_model("nin"), inplace=True, **kw).cuda().train()
    opt = make_optimizer(model, 0.01, wd)
    x, y = synth_batch(8, device="cuda")
    ops.fallback_counts(reset=True)
    loss, _ = train_step(model, opt, x, y)
    print(scheme, "loss", float(loss.detach()), "fallbacks", ops.fallback_counts())
    assert torch.isfinite(loss)
    assert not any("maxpool" in k.lower().replace("_", "") for k in ops.fallback_counts()), ops.fallback_counts()
