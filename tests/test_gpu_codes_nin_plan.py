"""The compiled code-packed plan of PLAIN nin (micronet_amd.inference.dorefa_compile_codes(model, tile_blocks=True)) on the MI355X against the eval-mode
quant_inference model it was compiled from: every hidden stage exact against the judge of tests/codes_cases.py (int64 numpy convolution -> the library's mn_qa_fwd, and
the numpy fp32 chain; behind a standalone max-pool the judge's codes go through the numpy pool of tests/codes_nin_cases.py), the logits against I(x)."""
import importlib

import numpy as np
import pytest
import torch

import abi_driver
import codes_cases as CC
import codes_nin_cases as NC

pytestmark = pytest.mark.gpu

SMALL_CFG = [32, 32, 32, 64, 64, 64, 64, 64]


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


def _deployed(cfg=None, spread=False):
    """Plain nin W2A2 trained for two steps, its quant_inference=True twin I with pre-quantised weights, the plan and its code_ends twin, the batch.  spread: as in
    tests/test_gpu_codes_plan.py -- the BatchNorm scales (both signs) and shifts drawn wide before training, the running statistics following the batch, so that all
    four codes occur in every stage."""
    from micronet_amd import inference
    from micronet_amd.models import nin
    from micronet_amd.train import build_model, init_like_main, make_optimizer, synth_batch, train_step
    Q = importlib.import_module("micronet.compression.quantization.wqaq.dorefa.quantize")
    torch.manual_seed(1)
    make = (lambda: build_model("nin")) if cfg is None else (lambda: init_like_main(nin.Net(cfg=cfg)))
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
    return I, inference.dorefa_compile_codes(I, tile_blocks=True), inference.dorefa_compile_codes(I, code_ends=True, tile_blocks=True), x


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


def _stages(plan, x):
    plan.keep_stages = True
    with torch.no_grad():
        y = plan(x)
    plan.keep_stages = False
    return plan.stage_codes, y


def _check_stages(be, I, plan, x, all_codes=False):
    """Every hidden stage, teacher-forced from the plan's own previous stage, equals the judge (pooled stages: the judge, then the numpy pool)."""
    from micronet_amd import inference
    stages, _ = _stages(plan, x)
    assert len(stages) == len(plan.layers) + 1
    blocks = {n_: m for n_, m in I.named_modules()}
    widths = [plan.first.conv.out_channels] + [L["cout"] for L in plan.layers]
    for i, L in enumerate(plan.layers):
        codes_in = inference.unpack_codes(stages[i], widths[i]).cpu().numpy()
        conv = blocks[L["name"]].conv
        assert L["out_order"] is None and not L["pool"], "plain nin shuffles nothing and folds nothing"
        n = CC.N_LEVELS
        k = torch.round((conv.weight.detach() * n + n) / 2).cpu().numpy().astype(np.int64)
        acc = CC.O.conv2d_fwd(codes_in.astype(np.int64), 2 * k - n, None, padding=L["pad"], groups=L["groups"], acc=np.int64)
        ref = CC.judge(be, acc, L["chan"].cpu().numpy(), 0)
        if L["pool_ksp"]:
            ref = NC.np_codes_maxpool(ref, *L["pool_ksp"])
        got = inference.unpack_codes(stages[i + 1], widths[i + 1]).cpu().numpy()
        print(L["name"], "tile", L["tile"], "pool", L["pool_ksp"], "mismatches", int((got != ref).sum()), "of", got.size, "codes", np.bincount(got.ravel(), minlength=4))
        assert got.shape == ref.shape and np.array_equal(got, ref), (L["name"], int((got != ref).sum()), got.size)
        assert not all_codes or len(np.unique(got)) == 4, (L["name"], "the spread nets must produce all four codes in every stage")
        if widths[i + 1] % 32:
            assert not (stages[i + 1][:, -1].cpu().numpy().view(np.uint32) >> np.uint32(widths[i + 1] % 32)).any()


def test_plan_stages_equal_the_judge_nin(be, full):
    I, plan, _, x = full
    assert [r["kind"] for r in plan.report] == ["first"] + ["code"] * 7 + ["last"]
    assert [L["name"] for L in plan.layers if L["tile"]] == ["model.4"] and [L["name"] for L in plan.layers if L["pool_ksp"]] == ["model.2", "model.6"]
    _check_stages(be, I, plan, x[:2])


def test_plan_stages_equal_the_judge_small_net(be, small):
    I, plan, _, x = small
    assert {r["name"]: r["kernel"] for r in plan.report}["model.4"] == "k_codeconv_tile<5,0>"
    _check_stages(be, I, plan, x[:4])


def test_plan_stages_equal_the_judge_nin_all_codes(be, spread):
    I, plan, _, x = spread
    _check_stages(be, I, plan, x[:2], all_codes=True)


def test_plan_stages_equal_the_judge_small_net_all_codes(be, small_spread):
    I, plan, _, x = small_spread
    _check_stages(be, I, plan, x[:4], all_codes=True)


@pytest.mark.parametrize("which", ["full", "small", "spread", "small_spread"])
def test_plan_logits_against_the_inference_graph(which, request):
    """Batch 32.  The bound is the project's own for this path, that of test_dorefa_prequantized_inference_graph at 2 bits: 1e-6 max|logits| and the same argmax.
    The logits came out bit-equal on the MI355X for all four nets -- every hidden code is the same and the two ends are the model's own modules -- so
    that is what is asserted behind the bound."""
    I, plan, _, x = request.getfixturevalue(which)
    with torch.no_grad():
        ref, got = I(x), plan(x)
    assert got.shape == ref.shape == (32, 10)
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(which, "max |plan - I| =", err, "max |logits| =", scale, "bit-equal:", bool(torch.equal(got, ref)))
    assert err <= 1e-6 * scale, (err, scale)
    assert torch.equal(got.argmax(1), ref.argmax(1))
    assert torch.equal(got, ref), "bit-equal logits"


@pytest.mark.parametrize("which", ["full", "small", "spread", "small_spread"])
def test_code_ends_plan_equals_the_default_plan(which, request):
    """code_ends=True: every stage's planes and the logits are the default plan's to the bit."""
    _, plan, ends, x = request.getfixturevalue(which)
    assert "k_c1b_fwd" in ends.report[0]["kernel"] and "k_planesconv1x1_small" in ends.report[-1]["kernel"] and ends.report[1:-1] == plan.report[1:-1]
    a, ya = _stages(plan, x)
    b, yb = _stages(ends, x)
    assert len(a) == len(b) == 8
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q), ("stage", i, int((p != q).sum()))
    print(which, "code_ends logits bit-equal:", bool(torch.equal(ya, yb)), "max diff", float((ya - yb).abs().max()))
    assert torch.equal(ya, yb)


def test_plan_buffer_cache_and_run_to_run_identity(small_spread):
    _, plan, _, x = small_spread
    plan._ws.clear()
    with torch.no_grad():
        a = plan(x).clone()
        assert len(plan._ws) == 1
        ws = next(iter(plan._ws.values()))
        assert [m is not None for m in ws[4]] == [False, True, False, False, True, False, False], "one mid buffer per standalone pool"
        assert tuple(ws[4][1].shape) == (32, 1, 2, 32, 32) and tuple(ws[0][2].shape) == (32, 1, 2, 16, 16)
        ptrs = [b.data_ptr() for b in ws[0]]
        b = plan(x).clone()
        assert len(plan._ws) == 1 and ptrs == [t.data_ptr() for t in next(iter(plan._ws.values()))[0]], "the same shape reuses its buffers"
        c = plan(x[:8]).clone()
        assert len(plan._ws) == 2, "a second input shape extends the cache"
    assert torch.equal(a, b), "run-to-run bit identity"
    assert torch.equal(c, a[:8]), "a sample's logits do not depend on the batch it is in"


def test_profile_of_one_forward(full):
    """Between the first and the last conv only plane kernels run: one tiled 5x5 block, two plane max-pools, none of the byte-path hidden kernels."""
    from micronet_amd import _lib
    _, plan, ends, x = full
    lib = _lib.get_lib()
    for p_, ends_too in ((ends, True), (plan, False)):
        with torch.no_grad():
            p_(x)
        torch.cuda.synchronize()
        buf = (_lib.ProfEntry * 192)()
        lib.mn_profile_collect(buf, 192)
        lib.mn_profile_enable(1)
        with torch.no_grad():
            p_(x)
        torch.cuda.synchronize()
        n = lib.mn_profile_collect(buf, 192)
        lib.mn_profile_enable(0)
        names = {buf[i].name.decode(): int(buf[i].launches) for i in range(n)}
        print(names)
        assert names.get("k_codeconv_tile<5,3>") == 1 and names.get("k_codes_maxpool") == 2, names
        assert names.get("k_codeconv<1,0,0>") == 5 and names.get("k_codeconv<3,0,0>") == 1, names
        byte_path = [k for k in names if k.startswith(("k_pws", "k_k3s", "k_kk", "k_qa_fwd"))]
        if ends_too:          # code_ends: the two ends are plane kernels as well, so nothing of the byte path may show up at all
            assert not byte_path, names
            assert "k_codes_pack" not in names and "k_codes_unpack" not in names, names
        else:                 # the default plan: the model's own first and last block run on byte codes, one pack and one unpack between them and the planes
            assert names.get("k_codes_pack") == 1 and names.get("k_codes_unpack") == 1, names


@pytest.mark.parametrize("ends", [0, 1], ids=["default", "code_ends"])
def test_plan_batch_256_equals_its_chunks(spread, ends):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    DG.plan_whole_against_chunks(spread[1 + ends], "stage_codes")
