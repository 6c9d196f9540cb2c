"""The compiled bit-packed plans with ``mfma_blocks`` / ``mfma_k3`` (micronet_amd.inference.wbwtab_compile_bits) on the MI355X, batch 32: every stage's bits and the
logits are the default plan's to the bit -- whose stages tests/test_gpu_bits.py and tests/test_gpu_bits_nin.py hold against the folded graph -- and the logits are
the folded graph's."""
import pytest
import torch

pytestmark = pytest.mark.gpu

K1, K3 = "k_bitconv_mfma<", "k_bitconv_mfma3<0>"
FLAGS = [dict(mfma_blocks=True), dict(mfma_k3=True), dict(mfma_blocks=True, mfma_k3=True), dict(mfma_blocks=True, mfma_k3=True, bit_ends=True)]


def _stages(plan, x):
    plan.keep_stages = True
    with torch.no_grad():
        y = plan(x)
    plan.keep_stages = False
    return [b.clone() for b in plan.stage_bits], y.clone()


@pytest.fixture(scope="module")
def models():
    """(folded graph, batch, F(x), the default plan's stages and logits) per (net, W): built once, left unchanged."""
    from micronet_amd import inference
    from test_gpu_bits import _nin_gc_folded
    from test_gpu_bits_nin import _nin_folded
    out = {}
    for key, make, W in (("nin_gc_w3", _nin_gc_folded, 3), ("nin_gc_w2", _nin_gc_folded, 2), ("nin", _nin_folded, 3)):
        F, x = make(W)
        assert x.shape[0] == 32
        with torch.no_grad():
            f = F(x)
        stages, y = _stages(inference.wbwtab_compile_bits(F), x)
        assert torch.equal(y, f), "the default plan computes the folded graph"
        out[key] = (F, x, f, stages, y)
    return out


def _same_as_default(models, key, kw):
    from micronet_amd import inference
    F, x, f, a, ya = models[key]
    plan = inference.wbwtab_compile_bits(F, **kw)
    assert plan.report == inference.wbwtab_bits_report(F, **kw)
    assert all(("mfma" in L) == bool(kw.get("mfma_blocks")) and ("mfma3" in L) == bool(kw.get("mfma_k3")) for L in plan.layers)
    b, yb = _stages(plan, x)
    assert len(a) == len(b) == len(plan.layers) + 1
    for i, (p, q) in enumerate(zip(a, b)):
        print(key, kw, "stage", i, tuple(p.shape), "words unlike the default plan's:", int((p != q).sum()))
        assert p.shape == q.shape and torch.equal(p, q), ("stage", i, int((p != q).sum()))
    print(key, kw, "logits bit-equal to the default plan:", bool(torch.equal(ya, yb)), "to the folded graph:", bool(torch.equal(yb, f)))
    assert yb.shape == (32, 10) and torch.equal(ya, yb) and torch.equal(yb, f)
    ptrs = [t.data_ptr() for t in next(iter(plan._ws.values()))[0]]
    with torch.no_grad():
        y2 = plan(x)
    assert torch.equal(y2, yb) and len(plan._ws) == 1 and ptrs == [t.data_ptr() for t in next(iter(plan._ws.values()))[0]], "a second forward reuses the buffers"
    return plan


@pytest.mark.parametrize("kw", FLAGS, ids=["blocks", "k3", "both", "both_bit_ends"])
@pytest.mark.parametrize("key", ["nin_gc_w3", "nin_gc_w2"])
def test_mfma_plan_equals_the_default_plan_nin_gc(models, key, kw):
    plan = _same_as_default(models, key, kw)
    kernels = [r["kernel"] for r in plan.report[1:-1]]
    assert sum(k.startswith(K1) for k in kernels) == (5 if kw.get("mfma_blocks") else 0) and kernels.count(K3) == (2 if kw.get("mfma_k3") else 0), kernels
    if kw.get("mfma_k3"):
        assert [(int(L["table"][2]), int(L["table"][5])) for L in plan.layers if L["mfma3"]] == [(8, 0), (16, 0)], "the spans of shuffle 16 / shuffle 32, no dead rows"


@pytest.mark.parametrize("kw", FLAGS, ids=["blocks", "k3", "both", "both_bit_ends"])
def test_mfma_plan_equals_the_default_plan_plain_nin(models, kw):
    plan = _same_as_default(models, "nin", kw)
    kernels = [r["kernel"] for r in plan.report[1:-1]]
    assert kernels.count("k_bitconv_mfma<0>") == (3 if kw.get("mfma_blocks") else 0) and kernels.count(K3) == (1 if kw.get("mfma_k3") else 0), kernels
    assert kernels.count("k_bitconv1_pool3<8>") == 2 and kernels.count("k_bitconv_tile<5,3>") == 1, "the folded 3x3 / 2 blocks and the 5x5 keep their kernels"


def test_profile_of_one_forward(models):
    """One forward of nin_gc under both flags: seven MFMA launches, no popcount block."""
    from micronet_amd import _lib, inference
    F, x = models["nin_gc_w3"][:2]
    plan = inference.wbwtab_compile_bits(F, mfma_blocks=True, mfma_k3=True)
    lib = _lib.get_lib()
    with torch.no_grad():
        plan(x)
    torch.cuda.synchronize()
    buf = (_lib.ProfEntry * 192)()
    lib.mn_profile_collect(buf, 192)
    lib.mn_profile_enable(1)
    with torch.no_grad():
        plan(x)
    torch.cuda.synchronize()
    n = lib.mn_profile_collect(buf, 192)
    lib.mn_profile_enable(0)
    names = {buf[i].name.decode(): int(buf[i].launches) for i in range(n)}
    print(names)
    assert names.get(K3) == 2 and names.get("k_bitconv_mfma<0>") == 3 and names.get("k_bitconv_mfma<1>") == 2, names
    assert not [k for k in names if k.startswith("k_bitconv<")], names
    assert names.get("k_bits_pack") == 1 and names.get("k_bits_unpack") == 1, names


@pytest.mark.parametrize("kw", FLAGS, ids=["blocks", "k3", "both", "both_bit_ends"])
@pytest.mark.parametrize("key", ["nin_gc_w3", "nin"])
def test_mfma_plan_batch_256_equals_its_chunks(models, key, kw):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    from micronet_amd import inference
    DG.plan_whole_against_chunks(inference.wbwtab_compile_bits(models[key][0], **kw), "stage_bits")
