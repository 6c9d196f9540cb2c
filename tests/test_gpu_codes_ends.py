"""The two ends of the code-packed plan on the MI355X: the kernel checks of tests/codes_ends_cases.py on the product library, and ``dorefa_compile_codes(I, code_ends=True)``
against the default plan compiled from the same model -- every stage's planes and the logits equal, no pack / unpack / byte-code launch, one launch of each new entry point."""
import importlib

import pytest
import torch

import abi_driver
import codes_ends_cases as E

pytestmark = pytest.mark.gpu

SMALL_CFG = [32, 32, 32, 64, 64, 64, 128, 128]          # the small golden net of the inference tests (tests/golden/inference_meta.json)


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("case", range(len(E.FIRST_CASES)))
def test_first_conv_codes(be, case):
    E.check_first_codes(be, *E.FIRST_CASES[case], seed=1500 + case)


def test_first_conv_codes_beyond_the_threshold_range_and_nan(be):
    E.check_first_codes_guard(be, seed=1510)


def test_first_conv_codes_tail_is_zero(be):
    E.check_first_codes_tail_is_zero(be, seed=1511)


def test_first_conv_codes_nonfinite_constants_are_counted(be):
    E.check_first_nonfinite_counted(be, seed=1512)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", range(len(E.CLASSIFIER_SHAPES)))
def test_planes_classifier(be, shape, bias):
    E.check_planes_classifier(be, *E.CLASSIFIER_SHAPES[shape], bias=bias, seed=1520 + shape)


@pytest.mark.parametrize("bias", [True, False])
def test_planes_classifier_partial_word_and_pixel_tail(be, bias):
    E.check_planes_classifier(be, *E.CLASSIFIER_ODD, bias=bias, N=3, Oc=3, seed=1530)


def test_rejects_bad_arguments(be):
    E.check_rejects_bad_arguments(be)


# ------------------------------------------------------------------------------------------------ the compiled plan
_DEPLOYED = {}


def _deployed(which):
    """The fixtures of tests/test_gpu_codes_plan.py (nin_gc and the small cfg, each plain and "spread": BatchNorm scales of both signs and wide shifts, so that all four
    codes occur in every stage), the model compiled twice: (I, default plan, code_ends plan, batch of 32).  Built once per kind."""
    if which not in _DEPLOYED:
        from micronet_amd import inference
        from micronet_amd.models import nin_gc
        from micronet_amd.train import build_model, init_like_main, make_optimizer, synth_batch, train_step
        Q = importlib.import_module("micronet.compression.quantization.wqaq.dorefa.quantize")
        cfg, spread = (SMALL_CFG if which.startswith("small") else None), which.endswith("spread")
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
        _DEPLOYED[which] = (I, inference.dorefa_compile_codes(I), inference.dorefa_compile_codes(I, code_ends=True), x)
    return _DEPLOYED[which]


def _count_calls(monkeypatch, fn):
    from micronet_amd import ops
    counts, real = {}, ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (counts.__setitem__(name, counts.get(name, 0) + 1), real(name, *a))[1])
    try:
        with torch.no_grad():
            out = fn()
    finally:
        monkeypatch.setattr(ops, "_call", real)
    return counts, out


BYTE_ENDS = ("mn_codes_pack_planes", "mn_codes_unpack_planes", "mn_qa_fwd", "mn_codeconv1x1_small_fwd")
CODE_ENDS = ("mn_conv2d_first_codes", "mn_planesconv1x1_small_fwd")
KINDS = ["full", "small", "spread", "small_spread"]


@pytest.mark.parametrize("which", KINDS)
def test_plan_with_code_ends_has_the_default_plans_stages(which, monkeypatch):
    """Batch 4: every stage's planes, what was launched, the buffers."""
    from micronet_amd import inference
    I, P0, P1, x = _deployed(which)
    x = x[:4].contiguous()
    assert P1.report == inference.dorefa_codes_report(I, code_ends=True) and P0.report == inference.dorefa_codes_report(I)
    assert P1.report[1:-1] == P0.report[1:-1]
    P0.keep_stages = P1.keep_stages = True
    c0, y0 = _count_calls(monkeypatch, lambda: P0(x))
    c1, y1 = _count_calls(monkeypatch, lambda: P1(x))
    P0.keep_stages = P1.keep_stages = False
    print(which, "P0", c0, "P1", c1)
    assert len(P1.stage_codes) == len(P0.stage_codes) == len(P0.layers) + 1
    for i, (b1, b0) in enumerate(zip(P1.stage_codes, P0.stage_codes)):
        assert torch.equal(b1, b0), (P0.report[i]["name"], int((b1 != b0).sum()), b0.numel())
    if which.endswith("spread"):
        codes = inference.unpack_codes(P1.stage_codes[0], P1.first.conv.out_channels)
        assert len(torch.unique(codes)) == 4, "the spread nets produce all four codes in the first stage"
    assert torch.equal(y1, y0), float((y1 - y0).abs().max())
    # what was launched: no byte ends in P1, one launch of each new entry point; P0 as before
    assert not [n for n in BYTE_ENDS if n in c1] and [c1.get(n) for n in CODE_ENDS] == [1, 1], c1
    assert c0.get("mn_codes_pack_planes") == 1 and c0.get("mn_codes_unpack_planes") == 1 and not [n for n in CODE_ENDS if n in c0], c0
    assert c1.get("mn_codeconv_fwd") == c0.get("mn_codeconv_fwd") == len(P0.layers)
    # buffers: no uint8 buffer in front of the last conv
    ws = P1._ws[next(k for k in P1._ws if k[0][0] == 4)]
    assert ws[2] is None and P0._ws[next(k for k in P0._ws if k[0][0] == 4)][2].dtype == torch.uint8
    assert all(t.dtype == torch.int32 for t in ws[0])


@pytest.mark.parametrize("which", KINDS)
def test_plan_with_code_ends_logits(which):
    """Batch 32: bit-equal to the default plan's, and so to I(x) (tests/test_gpu_codes_plan.py asserts that equality for the default plan)."""
    I, P0, P1, x = _deployed(which)
    with torch.no_grad():
        ref, y0, y1 = I(x), P0(x), P1(x)
    assert y1.shape == (32, 10)
    print(which, "max |P1 - P0| =", float((y1 - y0).abs().max()), "max |P1 - I| =", float((y1 - ref).abs().max()))
    assert torch.equal(y1, y0)
    assert torch.equal(y1, ref)


def test_code_ends_buffer_cache_and_run_to_run_identity():
    I, P0, P1, x = _deployed("small_spread")
    P1._ws.clear()
    with torch.no_grad():
        a = P1(x).clone()
        assert len(P1._ws) == 1
        ptrs = [b.data_ptr() for b in next(iter(P1._ws.values()))[0]]
        b = P1(x).clone()
        assert len(P1._ws) == 1 and ptrs == [t.data_ptr() for t in next(iter(P1._ws.values()))[0]], "the same shape reuses its buffers"
        c = P1(x[:8]).clone()
        assert len(P1._ws) == 2, "a second input shape extends the cache"
        d = P1(x).clone()
        assert len(P1._ws) == 2
    assert torch.equal(a, b) and torch.equal(a, d), "run-to-run bit identity"
    assert torch.equal(c, a[:8]), "a sample's logits do not depend on the batch it is in"


def test_code_ends_refuses_cpu_and_float64_inputs_and_uncovered_shapes():
    from micronet_amd._lib import MicronetHipError
    I, P0, P1, x = _deployed("small")
    with pytest.raises(MicronetHipError, match="float32 GPU tensor"):
        P1(x.cpu())
    with pytest.raises(MicronetHipError, match="float32 GPU tensor"):
        P1(x.double())
    with pytest.raises(MicronetHipError, match=r"model\.0\.conv"):
        P1(x[:, :, :, :30].contiguous())
    with pytest.raises(MicronetHipError, match="eval-only"):
        P1.train()


def test_plan_with_code_ends_batch_256_equals_its_chunks():
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    DG.plan_whole_against_chunks(_deployed("spread")[2], "stage_codes")
