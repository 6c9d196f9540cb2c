"""The compiled code-packed plan (micronet_amd.inference.dorefa_compile_codes) on the MI355X against the eval-mode quant_inference model it was compiled from: every
hidden stage exact against the judge of tests/codes_cases.py (int64 numpy convolution -> the library's mn_qa_fwd, and the numpy fp32 chain), the logits against I(x)."""
import importlib

import numpy as np
import pytest
import torch

import abi_driver
import codes_cases as CC

pytestmark = pytest.mark.gpu

SMALL_CFG = [32, 32, 32, 64, 64, 64, 128, 128]          # the small golden net of the inference tests (tests/golden/inference_meta.json)


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


def _deployed(cfg=None, spread=False):
    """nin_gc W2A2 trained for two steps (as test_gpu_inference._trained does), its quant_inference=True twin I with pre-quantised weights, the plan, the batch.
    spread: two steps from the default initialisation leave every hidden activation below the first code boundary (all codes 0); this variant draws the BatchNorm
    scales (both signs) and shifts wide before training and lets the running statistics follow the batch, so that all four codes occur in every stage."""
    from micronet_amd import inference
    from micronet_amd.models import nin_gc
    from micronet_amd.train import build_model, init_like_main, make_optimizer, synth_batch, train_step
    Q = importlib.import_module("micronet.compression.quantization.wqaq.dorefa.quantize")
    torch.manual_seed(1)
    make = (lambda: build_model("nin_gc")) if cfg is None else (lambda: init_like_main(nin_gc.Net(cfg=cfg)))
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
    return I, inference.dorefa_compile_codes(I), x


@pytest.fixture(scope="module")
def full():
    return _deployed()


@pytest.fixture(scope="module")
def small():
    return _deployed(SMALL_CFG)


@pytest.fixture(scope="module")
def spread():
    return _deployed(spread=True)


@pytest.fixture(scope="module")
def small_spread():
    return _deployed(SMALL_CFG, spread=True)


def _check_stages(be, I, plan, x, all_codes=False):
    """Every hidden stage, teacher-forced from the plan's own previous stage, equals the judge."""
    from micronet_amd import inference
    plan.keep_stages = True
    with torch.no_grad():
        plan(x)
    plan.keep_stages = False
    stages = plan.stage_codes
    assert len(stages) == len(plan.layers) + 1
    convs = {n_: m for n_, m in I.named_modules()}
    widths = [plan.first.conv.out_channels] + [L["cout"] for L in plan.layers]
    for i, L in enumerate(plan.layers):
        codes_in = inference.unpack_codes(stages[i], widths[i]).cpu().numpy()
        s = convs[L["name"]].conv.in_shuffle_groups or 0
        assert (L["out_order"] is None) == (i + 1 == len(plan.layers) or not (convs[plan.layers[i + 1]["name"]].conv.in_shuffle_groups or 0) > 1)
        conv = convs[L["name"]].conv
        n = CC.N_LEVELS
        k = torch.round((conv.weight.detach() * n + n) / 2).cpu().numpy().astype(np.int64)
        # the stage's input is already in the consumer's (shuffled) channel order: the producer's rows were packed in that order
        acc = CC.O.conv2d_fwd(codes_in.astype(np.int64), 2 * k - n, None, padding=L["pad"], groups=L["groups"], acc=np.int64)
        chan = L["chan"].cpu().numpy()
        ref = CC.judge(be, acc, chan, L["pool"])
        if L["out_order"] is not None:
            ref = ref[:, L["out_order"].cpu().numpy()]
        got = inference.unpack_codes(stages[i + 1], widths[i + 1]).cpu().numpy()
        print(L["name"], "shuffle in", s, "pool", L["pool"], "mismatches", int((got != ref).sum()), "of", got.size, "codes", np.bincount(got.ravel(), minlength=4))
        assert np.array_equal(got, ref), (L["name"], int((got != ref).sum()), got.size)
        assert not all_codes or len(np.unique(got)) == 4, (L["name"], "the spread nets must produce all four codes in every stage")
        if widths[i + 1] % 32:
            assert not (stages[i + 1][:, -1].cpu().numpy().view(np.uint32) >> np.uint32(widths[i + 1] % 32)).any()


def test_plan_stages_equal_the_judge_nin_gc(be, full):
    I, plan, x = full
    assert [r["kind"] for r in plan.report] == ["first"] + ["code"] * 7 + ["last"]
    _check_stages(be, I, plan, x[:4])


def test_plan_stages_equal_the_judge_small_net(be, small):
    I, plan, x = small
    _check_stages(be, I, plan, x[:4])


def test_plan_stages_equal_the_judge_nin_gc_all_codes(be, spread):
    I, plan, x = spread
    _check_stages(be, I, plan, x[:4], all_codes=True)


def test_plan_stages_equal_the_judge_small_net_all_codes(be, small_spread):
    I, plan, x = small_spread
    _check_stages(be, I, plan, x[:4], all_codes=True)


@pytest.mark.parametrize("which", ["full", "small", "spread", "small_spread"])
def test_plan_logits_against_the_inference_graph(which, request):
    """Batch 32.  The bound the plan was built to is that of test_dorefa_prequantized_inference_graph at 2 bits (1e-6 max|logits|, same argmax); the logits came out
    bit-equal on the MI355X -- the two ends are the model's own modules and every hidden code is the same -- so that is what is asserted."""
    I, plan, x = request.getfixturevalue(which)
    with torch.no_grad():
        ref, got = I(x), plan(x)
    assert got.shape == ref.shape == (32, 10)
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(which, "max |plan - I| =", err, "max |logits| =", scale, "bit-equal:", bool(torch.equal(got, ref)))
    assert err <= 1e-6 * scale, (err, scale)
    assert torch.equal(got.argmax(1), ref.argmax(1))
    assert torch.equal(got, ref), "bit-equal logits"


def test_plan_buffer_cache_and_run_to_run_identity(small_spread):
    I, plan, x = small_spread
    plan._ws.clear()
    with torch.no_grad():
        a = plan(x).clone()
        assert len(plan._ws) == 1
        ptrs = [b.data_ptr() for b in next(iter(plan._ws.values()))[0]]
        b = plan(x).clone()
        assert len(plan._ws) == 1 and ptrs == [t.data_ptr() for t in next(iter(plan._ws.values()))[0]], "the same shape reuses its buffers"
        c = plan(x[:8]).clone()
        assert len(plan._ws) == 2, "a second input shape extends the cache"
        d = plan(x).clone()
        assert len(plan._ws) == 2
    assert torch.equal(a, b) and torch.equal(a, d), "run-to-run bit identity"
    assert torch.equal(c, a[:8]), "a sample's logits do not depend on the batch it is in"


def test_plan_refuses_weights_off_the_grid_and_train(small):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    import copy
    I, plan, _ = small
    with pytest.raises(MicronetHipError, match="eval-only"):
        plan.train()
    J = copy.deepcopy(I)
    with torch.no_grad():
        J.model[4].conv.weight.data = J.model[4].conv.weight.data * 0.9
    with pytest.raises(MicronetHipError, match=r"model\.4\.conv: the stored weights were not found on the 2-bit grid"):
        inference.dorefa_compile_codes(J)


def test_pack_codes_unpack_codes_helpers():
    from micronet_amd import inference
    torch.manual_seed(3)
    codes = torch.randint(0, 4, (2, 80, 4, 8), dtype=torch.uint8, device="cuda")
    planes = inference.pack_codes(codes, 2)
    assert planes.shape == (2, 3, 2, 4, 8) and planes.dtype == torch.int32
    assert np.array_equal(planes.cpu().numpy().view(np.uint32), CC.np_pack_planes(codes.cpu().numpy()))
    assert torch.equal(inference.unpack_codes(planes, 80), codes)


@pytest.mark.parametrize("which", ["full", "spread"])
def test_plan_batch_256_equals_its_chunks(which, request):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    DG.plan_whole_against_chunks(request.getfixturevalue(which)[1], "stage_codes")
