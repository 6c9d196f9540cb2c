"""prepare(fuse_pool3=True) on W4A4 plain nin: both nn.MaxPool2d(3, 2, 1) are folded into the fused k-bit block in front (mn_qa_* with pool = 2); without the keyword
prepare() leaves them un-fused as before, and both graphs are the same function."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu


@pytest.fixture
def pair():          # (per test: a forward in training mode moves the BatchNorm buffers)
    from micronet.compression.quantization.wqaq.dorefa import quantize as Q
    from micronet_amd.train import build_model
    torch.manual_seed(0)
    base = build_model("nin")
    return Q.prepare(base, a_bits=4, w_bits=4, fuse_pool3=True).cuda().train(), Q.prepare(base, a_bits=4, w_bits=4).cuda().train()


def _pools(model):
    kids = list(model.model)
    return [(kids[i - 1], m, kids[i + 1]) for i, m in enumerate(kids) if isinstance(m, nn.MaxPool2d)]


def test_prepared_structure(pair):
    from micronet_amd.sign_tensor import QActTensor
    from micronet_amd.train import synth_batch
    on, off = pair
    assert len(_pools(on)) == len(_pools(off)) == 2
    for front, pool, _ in _pools(off):          # the default: what prepare() always produced for plain nin
        assert not getattr(pool, "_mn_fused_pool", False) and front.bn.q_out_bits == 0 and front.bn.q_pool is False
    seen = []
    for front, pool, behind in _pools(on):
        assert pool._mn_fused_pool is True and front.bn.q_pool == 2 and front.bn.q_out_bits == 4
        behind.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    on(synth_batch(8, device="cuda")[0])
    assert [type(t) for t in seen] == [QActTensor, QActTensor] and [tuple(t.shape[1:]) for t in seen] == [(96, 16, 16), (192, 8, 8)], seen


def test_training_step_matches_unfused_pools(pair):
    """One step at batch 8, flag on against off, to the tolerances (and exemptions) of test_gpu_modules.test_dorefa_fused_blocks_match_unfused at <= 4 bits:
    1e-6 logits, 2e-5 gradients (2e-4 on the weight quantizer's arg-max element), 2e-6 buffers."""
    from micronet_amd import ops
    from micronet_amd.train import synth_batch
    a, b = pair
    x, y = synth_batch(8, device="cuda")
    ops.fallback_counts(reset=True)
    oa = a(x)
    torch.nn.functional.cross_entropy(oa, y).backward()
    assert not ops.fallback_counts(), ops.fallback_counts()
    ob = b(x)
    torch.nn.functional.cross_entropy(ob, y).backward()
    assert float((oa - ob).detach().abs().max()) <= 1e-6 * float(ob.detach().abs().max()), "logits"
    gmax = max(float(p.grad.abs().max()) for p in b.parameters())
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if n.endswith("conv.bias") and float(pb.grad.abs().max()) < 1e-4 * gmax:
            continue          # (a conv bias in front of a BatchNorm: the true gradient is 0, both sides hold round-off)
        d, scale = (pa.grad - pb.grad).abs().flatten().clone(), pb.grad.abs().max().clamp_min(1e-30)
        if n.endswith("conv.weight") and pa.dim() == 4:
            k = int(pb.detach().abs().argmax())
            assert float(d[k] / scale) <= 2e-4, (n, "arg-max element", float(d[k] / scale))
            d[k] = 0
        assert float(d.max() / scale) <= 2e-5, (n, float(d.max() / scale))
    bufs_b = dict(b.named_buffers())
    for (n, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        scale = float(bb.abs().max().clamp_min(1e-6)) if ba.dtype.is_floating_point else 0.0
        if n.endswith("running_mean"):          # (a mean is accurate relative to the spread of the data)
            scale = max(scale, float(bufs_b[n[:-len("running_mean")] + "running_var"].max().sqrt()))
        assert float((ba - bb).abs().max()) <= 2e-6 * scale, n
