"""The compiled code-packed plan of a W4A4 nin_gc (micronet_amd.inference.dorefa_compile_codes: four bits per hidden activation, every hidden block on an int8-MFMA
kernel) on the MI355X against the eval-mode quant_inference model it was compiled from: every hidden stage exact against the judge of tests/codes_w4_cases.py (int64
numpy convolution -> the library's mn_qa_fwd(a_bits = 4), and the numpy fp32 chain with n = 15), the logits bit-equal to I(x)."""
import copy
import importlib

import numpy as np
import pytest
import torch

import abi_driver
import codes_w4_cases as W4

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


def _inference_model(spread=False):
    """The fixture of tests/test_gpu_codes_mfma_plan.py at a_bits = w_bits = 4: full nin_gc trained for two steps, its quant_inference=True twin I with pre-quantised
    weights, the plan, the batch of 32.  spread: BatchNorm scales (both signs) and shifts drawn wide, so that all sixteen codes occur in every stage."""
    from micronet_amd import inference
    from micronet_amd.train import build_model, make_optimizer, synth_batch, train_step
    Q = importlib.import_module("micronet.compression.quantization.wqaq.dorefa.quantize")
    torch.manual_seed(1)
    T = Q.prepare(build_model("nin_gc"), inplace=True, a_bits=4, w_bits=4).cuda().train()
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
    I = Q.prepare(build_model("nin_gc"), inplace=True, a_bits=4, w_bits=4, quant_inference=True).cuda()
    I.load_state_dict(T.state_dict())
    assert inference.prequantize_weights(I) == 8
    I.eval()
    return I, inference.dorefa_compile_codes(I), x


@pytest.fixture(scope="module")
def full():
    return _inference_model()


@pytest.fixture(scope="module")
def spread():
    return _inference_model(spread=True)


def _check_stages(be, I, plan, x, all_codes=False):
    """Every hidden stage, teacher-forced from the plan's own previous stage, equals the judge (test_gpu_codes_plan._check_stages at width 4)."""
    from micronet_amd import inference
    plan.keep_stages = True
    with torch.no_grad():
        plan(x)
    plan.keep_stages = False
    stages = plan.stage_codes
    assert len(stages) == len(plan.layers) + 1 and all(s.shape[2] == 4 for s in stages)
    convs = {n_: m for n_, m in I.named_modules()}
    widths = [plan.first.conv.out_channels] + [L["cout"] for L in plan.layers]
    n = W4.N_LEVELS
    for i, L in enumerate(plan.layers):
        codes_in = inference.unpack_codes(stages[i], widths[i]).cpu().numpy()
        assert (L["out_order"] is None) == (i + 1 == len(plan.layers) or not (convs[plan.layers[i + 1]["name"]].conv.in_shuffle_groups or 0) > 1)
        conv = convs[L["name"]].conv
        k = torch.round((conv.weight.detach() * n + n) / 2).cpu().numpy().astype(np.int64)
        # the stage's input is already in the consumer's (shuffled) channel order: the producer's rows were packed in that order
        acc = W4.O.conv2d_fwd(codes_in.astype(np.int64), 2 * k - n, None, padding=L["pad"], groups=L["groups"], acc=np.int64)
        ref = W4.judge(be, acc, L["chan"].cpu().numpy(), L["pool"])
        if L["out_order"] is not None:
            ref = ref[:, L["out_order"].cpu().numpy()]
        got = inference.unpack_codes(stages[i + 1], widths[i + 1]).cpu().numpy()
        print(L["name"], "pool", L["pool"], "mismatches", int((got != ref).sum()), "of", got.size, "codes", np.bincount(got.ravel(), minlength=16))
        assert np.array_equal(got, ref), (L["name"], int((got != ref).sum()), got.size)
        assert not all_codes or len(np.unique(got)) == 16, (L["name"], "the spread net must produce all sixteen codes in every stage")


def test_w4a4_plan_is_all_mfma(full):
    _, plan, _ = full
    assert plan.bits == 4 and [r["kind"] for r in plan.report] == ["first"] + ["code"] * 7 + ["last"]
    assert all(r["planes"] == 4 for r in plan.report[1:])
    assert [L["mfma"] for L in plan.layers] == [L["k"] == 1 for L in plan.layers] and [L["mfma3"] for L in plan.layers] == [L["k"] == 3 for L in plan.layers]
    for L in plan.layers:
        hdr = L["table"][:8].cpu().numpy().view(np.uint32)
        assert int(hdr[0]) == 0 and int(hdr[7]) == 0 and int(hdr[6]) == W4.WORD6, (L["name"], hdr)


def test_w4a4_plan_stages_equal_the_judge(be, full):
    I, plan, x = full
    _check_stages(be, I, plan, x[:4])


def test_w4a4_plan_stages_equal_the_judge_all_codes(be, spread):
    I, plan, x = spread
    _check_stages(be, I, plan, x[:4], all_codes=True)


@pytest.mark.parametrize("which", ["full", "spread"])
def test_w4a4_plan_logits_are_the_inference_graph_s(which, request):
    """The two ends are the model's own modules on the same byte codes and every hidden code is the same: bit-equal logits.  A sample's logits do not depend on the
    batch it is in, and two runs are identical."""
    I, plan, x = request.getfixturevalue(which)
    with torch.no_grad():
        ref, got = I(x), plan(x).clone()
        again = plan(x).clone()
        head = plan(x[:8]).clone()
    print(which, "max |plan - I| =", float((got - ref).abs().max()), "max |logits| =", float(ref.abs().max()), "bit-equal:", bool(torch.equal(got, ref)))
    assert got.shape == ref.shape == (32, 10)
    assert torch.equal(got, ref), "bit-equal logits"
    assert torch.equal(got, again), "run-to-run bit identity"
    assert torch.equal(head, got[:8])


def test_w4a4_profile_of_one_forward(full):
    """One forward: the five 1x1 blocks and the two 3x3 blocks on their MFMA kernels, one pack, one unpack, no popcount launch."""
    from micronet_amd import _lib
    _, plan, x = full
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
    assert names.get("k_codeconv_mfma<0>") == 3 and names.get("k_codeconv_mfma<1>") == 2 and names.get("k_codeconv_mfma3<0>") == 2, names
    assert names.get("k_codes_pack") == 1 and names.get("k_codes_unpack") == 1, names
    assert not [k for k in names if k.startswith("k_codeconv<")], names


def test_w4a4_plan_refuses_weights_off_the_grid(full):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    I, _, _ = full
    J = copy.deepcopy(I)
    with torch.no_grad():
        J.model[4].conv.weight.data = J.model[4].conv.weight.data * 0.9
    with pytest.raises(MicronetHipError, match=r"model\.4\.conv: the stored weights were not found on the 4-bit grid \(2k - 15\) / 15"):
        inference.dorefa_compile_codes(J)


def test_w4a4_refuses_code_ends_and_tile_blocks_on_the_gpu_model(full):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    I, _, _ = full
    with pytest.raises(MicronetHipError, match=r"model\.0\.conv: the net has 4-bit codes"):
        inference.dorefa_compile_codes(I, code_ends=True)
    with pytest.raises(MicronetHipError, match=r"model\.1\.conv: the net has 4-bit codes"):
        inference.dorefa_compile_codes(I, tile_blocks=True)


@pytest.mark.parametrize("which", ["full", "spread"])
def test_w4a4_plan_batch_256_equals_its_chunks(which, request):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    DG.plan_whole_against_chunks(request.getfixturevalue(which)[1], "stage_codes")
