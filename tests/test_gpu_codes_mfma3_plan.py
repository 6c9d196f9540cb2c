"""The compiled code-packed plans with ``mfma_blocks=True, mfma_k3=True`` (micronet_amd.inference.dorefa_compile_codes) on the MI355X: every stage's planes and the
logits are the default plan's to the bit -- whose stages tests/test_gpu_codes_plan.py and tests/test_gpu_codes_nin_plan.py hold against the judge -- and the logits
are I(x)'s."""
import pytest
import torch

from test_gpu_codes_mfma_plan import _inference_model, _stages

pytestmark = pytest.mark.gpu

K3 = "k_codeconv_mfma3<0>"


@pytest.fixture(scope="module")
def gc_full():
    return _inference_model("nin_gc")


@pytest.fixture(scope="module")
def gc_spread():
    return _inference_model("nin_gc", spread=True)


@pytest.fixture(scope="module")
def nin_spread():
    return _inference_model("nin", spread=True)


def _same_as_default(I, x, **kw):
    """The plan with mfma_blocks=True, mfma_k3=True against the plan without either, same other keywords: stage planes, logits; the logits against I(x)."""
    from micronet_amd import inference
    base = inference.dorefa_compile_codes(I, **kw)
    plan = inference.dorefa_compile_codes(I, mfma_blocks=True, mfma_k3=True, **kw)
    assert all("mfma3" in L for L in plan.layers) and not any("mfma3" in L for L in base.layers)
    a, ya = _stages(base, x)
    b, yb = _stages(plan, x)
    assert len(a) == len(b) == len(plan.layers) + 1
    for i, (p, q) in enumerate(zip(a, b)):
        print("stage", i, tuple(p.shape), "words unlike the default plan's:", int((p != q).sum()))
        assert p.shape == q.shape and torch.equal(p, q), ("stage", i, int((p != q).sum()))
    with torch.no_grad():
        ref = I(x)
    print(kw, "logits bit-equal to the default plan:", bool(torch.equal(ya, yb)), "to I(x):", bool(torch.equal(yb, ref)))
    assert yb.shape == (32, 10) and torch.equal(ya, yb) and torch.equal(yb, ref)
    return plan


def _profile(plan, x):
    from micronet_amd import _lib
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
    return names


@pytest.mark.parametrize("which,code_ends", [("gc_full", False), ("gc_spread", False), ("gc_spread", True)])
def test_mfma3_plan_equals_the_default_plan_nin_gc(which, code_ends, request):
    I, x = request.getfixturevalue(which)
    plan = _same_as_default(I, x, code_ends=code_ends)
    kernels = [r["kernel"] for r in plan.report[1:-1]]
    assert kernels.count(K3) == 2 and kernels.count("k_codeconv_mfma<0>") == 3 and kernels.count("k_codeconv_mfma<1>") == 2, kernels
    assert [L["mfma3"] for L in plan.layers] == [L["k"] == 3 for L in plan.layers]
    assert [(int(L["table"][2]), int(L["table"][5])) for L in plan.layers if L["mfma3"]] == [(8, 0), (16, 0)], "the spans of shuffle 16 / shuffle 32, no dead rows"
    if which == "gc_spread":
        from micronet_amd import inference
        stages, _ = _stages(plan, x)
        for L, s in zip(plan.layers, stages[1:]):
            assert len(torch.unique(inference.unpack_codes(s, L["cout"]))) == 4, (L["name"], "the spread net must produce all four codes in every stage")


def test_mfma3_plan_equals_the_default_plan_plain_nin(nin_spread):
    I, x = nin_spread
    plan = _same_as_default(I, x, tile_blocks=True)
    k3 = [L for L in plan.layers if L["mfma3"]]
    assert len(k3) == 1 and (k3[0]["k"], k3[0]["cin"], k3[0]["cout"], k3[0]["groups"]) == (3, 192, 192, 1)
    assert (int(k3[0]["table"][2]), int(k3[0]["table"][5])) == (2, 0)
    assert [L["name"] for L in plan.layers if L["tile"]] == ["model.4"], "the 5x5 keeps the tile kernel"
    names = _profile(plan, x)
    assert names.get(K3) == 1 and not [k for k in names if k.startswith("k_codeconv<")], names


def test_profile_of_one_forward(gc_full):
    """One forward of nin_gc under both flags: seven MFMA launches, no popcount block."""
    from micronet_amd import inference
    I, x = gc_full
    names = _profile(inference.dorefa_compile_codes(I, mfma_blocks=True, mfma_k3=True), x)
    assert names.get(K3) == 2 and names.get("k_codeconv_mfma<0>") == 3 and names.get("k_codeconv_mfma<1>") == 2, names
    assert not [k for k in names if k.startswith("k_codeconv<")], names
    assert names.get("k_codes_pack") == 1 and names.get("k_codes_unpack") == 1, names


@pytest.mark.parametrize("which,kw", [("gc_spread", {}), ("gc_spread", dict(code_ends=True)), ("nin_spread", dict(tile_blocks=True))], ids=["nin_gc", "nin_gc_code_ends", "nin"])
def test_mfma3_plan_batch_256_equals_its_chunks(which, kw, request):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    from micronet_amd import inference
    I, _ = request.getfixturevalue(which)
    DG.plan_whole_against_chunks(inference.dorefa_compile_codes(I, mfma_blocks=True, mfma_k3=True, **kw), "stage_codes")
