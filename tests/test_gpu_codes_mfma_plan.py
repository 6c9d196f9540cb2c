"""The compiled code-packed plans with ``mfma_blocks=True`` (micronet_amd.inference.dorefa_compile_codes) on the MI355X: every stage's planes and the logits are the
default plan's to the bit -- whose stages tests/test_gpu_codes_plan.py and tests/test_gpu_codes_nin_plan.py hold against the judge -- and the logits are I(x)'s."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL_CFG = [32, 32, 32, 64, 64, 64, 128, 128]          # nin_gc with 16 channels per group in its grouped 1x1 blocks


def _inference_model(arch, cfg=None, spread=False):
    """The fixture of tests/test_gpu_codes_plan.py / test_gpu_codes_nin_plan.py: the W2A2 net trained for two steps, its quant_inference=True twin I with pre-quantised
    weights, the batch of 32.  spread: BatchNorm scales (both signs) and shifts drawn wide, so that all four codes occur in every stage."""
    from micronet_amd import inference
    from micronet_amd.train import build_model, init_like_main, make_optimizer, synth_batch, train_step
    Q = importlib.import_module("micronet.compression.quantization.wqaq.dorefa.quantize")
    net = importlib.import_module("micronet_amd.models." + arch)
    torch.manual_seed(1)
    make = (lambda: build_model(arch)) if cfg is None else (lambda: init_like_main(net.Net(cfg=cfg)))
    T = Q.prepare(make(), inplace=True, a_bits=2, w_bits=2).cuda().train()
    if spread:
        with torch.no_grad():
            for m in T.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.normal_(0.0, 3.0)
                    m.bias.normal_(4.0, 2.0)
                    m.momentum = 1.0
    opt = make_optimizer(T, 0.01, 1e-5)
    x, y = synth_batch(32, device="cuda")
    for _ in range(2):
        train_step(T, opt, x, y)
    I = Q.prepare(make(), inplace=True, a_bits=2, w_bits=2, quant_inference=True).cuda()
    I.load_state_dict(T.state_dict())
    assert inference.prequantize_weights(I) == 8
    I.eval()
    return I, x


@pytest.fixture(scope="module")
def gc_full():
    return _inference_model("nin_gc")


@pytest.fixture(scope="module")
def gc_spread():
    return _inference_model("nin_gc", spread=True)


@pytest.fixture(scope="module")
def gc_small():
    return _inference_model("nin_gc", SMALL_CFG, spread=True)


@pytest.fixture(scope="module")
def nin_spread():
    return _inference_model("nin", spread=True)


def _stages(plan, x):
    plan.keep_stages = True
    with torch.no_grad():
        y = plan(x)
    plan.keep_stages = False
    return plan.stage_codes, y


def _same_as_default(I, x, **kw):
    """The plan with mfma_blocks=True against the plan without, same other keywords: stage planes, logits; the logits against I(x).  Returns the MFMA plan."""
    from micronet_amd import inference
    base = inference.dorefa_compile_codes(I, **kw)
    plan = inference.dorefa_compile_codes(I, mfma_blocks=True, **kw)
    assert all("mfma" in L for L in plan.layers) and not any("mfma" in L for L in base.layers)
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


@pytest.mark.parametrize("code_ends", [False, True])
@pytest.mark.parametrize("which", ["gc_full", "gc_spread"])
def test_mfma_plan_equals_the_default_plan_nin_gc(which, code_ends, request):
    I, x = request.getfixturevalue(which)
    plan = _same_as_default(I, x, code_ends=code_ends)
    kernels = [r["kernel"] for r in plan.report[1:-1]]
    assert kernels.count("k_codeconv_mfma<0>") == 3 and kernels.count("k_codeconv_mfma<1>") == 2 and kernels.count("k_codeconv<3,1,0>") == 2, kernels
    assert [L["mfma"] for L in plan.layers] == [L["k"] == 1 for L in plan.layers]
    if which == "gc_spread":
        from micronet_amd import inference
        stages, _ = _stages(plan, x)
        for L, s in zip(plan.layers, stages[1:]):
            assert len(torch.unique(inference.unpack_codes(s, L["cout"]))) == 4, (L["name"], "the spread net must produce all four codes in every stage")


def test_mfma_plan_equals_the_default_plan_plain_nin(nin_spread):
    I, x = nin_spread
    plan = _same_as_default(I, x, tile_blocks=True)
    assert [L["mfma"] for L in plan.layers] == [L["k"] == 1 for L in plan.layers] and sum(L["mfma"] for L in plan.layers) == 5, "every dense 1x1 block is covered"
    assert [L["name"] for L in plan.layers if L["tile"]] == ["model.4"], "the 5x5 keeps the tile kernel"
    by = {r["name"]: r["kernel"] for r in plan.report}
    assert by["model.2"] == "k_codeconv_mfma<0>, k_codes_maxpool" and by["model.4"] == "k_codeconv_tile<5,3>"


def test_narrow_groups_stay_on_the_popcount_kernel(gc_small):
    I, x = gc_small
    plan = _same_as_default(I, x)
    narrow = [L for L in plan.layers if L["k"] == 1 and L["groups"] > 1 and (L["cin"] // L["groups"]) % 32]
    assert narrow and not any(L["mfma"] for L in narrow)
    by = {r["name"]: r["kernel"] for r in plan.report}
    assert all(by[L["name"]].startswith("k_codeconv<1,") for L in narrow), by
    assert all(by[L["name"]] == "k_codeconv_mfma<%d>" % L["pool"] for L in plan.layers if L["mfma"]), by


def test_profile_of_one_forward(gc_full):
    """One forward of nin_gc under the flag: the five 1x1 blocks on the MFMA kernel, the two 3x3 blocks on k_codeconv, no 1x1 popcount launch."""
    from micronet_amd import _lib, inference
    I, x = gc_full
    plan = inference.dorefa_compile_codes(I, mfma_blocks=True)
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
    assert names.get("k_codeconv_mfma<0>") == 3 and names.get("k_codeconv_mfma<1>") == 2, names
    assert not [k for k in names if k.startswith("k_codeconv<1,")], names
    assert names.get("k_codeconv<3,1,0>") == 2, names
    assert names.get("k_codes_pack") == 1 and names.get("k_codes_unpack") == 1, names


@pytest.mark.parametrize("which,kw", [("gc_spread", {}), ("gc_spread", dict(code_ends=True)), ("nin_spread", dict(tile_blocks=True))], ids=["nin_gc", "nin_gc_code_ends", "nin"])
def test_mfma_plan_batch_256_equals_its_chunks(which, kw, request):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    from micronet_amd import inference
    I, _ = request.getfixturevalue(which)
    DG.plan_whole_against_chunks(inference.dorefa_compile_codes(I, mfma_blocks=True, **kw), "stage_codes")
