"""The two ends of the bit-packed plan on the MI355X: the kernel checks of tests/bits_ends_cases.py on the product library, and ``wbwtab_compile_bits(F, bit_ends=True)``
against today's plan -- every stage's bits and the logits equal, no pack / unpack / byte-sign launch, one launch of each new entry point."""
import pytest
import torch

import abi_driver
import bits_ends_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("case", range(len(E.FIRST_CASES)))
def test_first_conv_sign_bits(be, case):
    E.check_first_bits(be, *E.FIRST_CASES[case], seed=1100 + case)


def test_first_conv_sign_bits_zero_and_nan_rule(be):
    E.check_first_bits_zero_rule(be, seed=1110)


def test_first_conv_sign_bits_tail_is_zero(be):
    E.check_first_bits_tail_is_zero(be, seed=1111)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", range(len(E.CLASSIFIER_SHAPES)))
def test_bits_classifier(be, shape, bias):
    E.check_bits_classifier(be, *E.CLASSIFIER_SHAPES[shape], bias=bias, seed=1120 + shape)


def test_rejects_bad_arguments(be):
    E.check_rejects_bad_arguments(be)


# ------------------------------------------------------------------------------------------------ the compiled plan
_FOLDED = {}


def _folded(arch, W):
    """nin_gc / nin built and folded as tests/test_gpu_bits.py / tests/test_gpu_bits_nin.py build theirs; once per (arch, W), batch 2 of the 32 x 32 inputs."""
    if (arch, W) not in _FOLDED:
        from test_gpu_bits import _nin_gc_folded
        from test_gpu_bits_nin import _nin_folded
        F, x = (_nin_gc_folded if arch == "nin_gc" else _nin_folded)(W)
        _FOLDED[(arch, W)] = (F, x[:2].contiguous())
    return _FOLDED[(arch, W)]


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


BYTE_ENDS = ("mn_bits_pack_sign8", "mn_bits_unpack_sign8", "mn_bnsign_fwd_i8")
BIT_ENDS = ("mn_conv2d_first_sign_bits", "mn_bitsconv1x1_small_fwd")


@pytest.mark.parametrize("W", [3, 2])
@pytest.mark.parametrize("arch", ["nin_gc", "nin"])
def test_plan_with_bit_ends_equals_todays_plan(arch, W, monkeypatch):
    from micronet_amd import inference
    F, x = _folded(arch, W)
    P0, P1 = inference.wbwtab_compile_bits(F), inference.wbwtab_compile_bits(F, bit_ends=True)
    assert P1.report == inference.wbwtab_bits_report(F, bit_ends=True) and P0.report == inference.wbwtab_bits_report(F)
    P0.keep_stages = P1.keep_stages = True
    c0, y0 = _count_calls(monkeypatch, lambda: P0(x))
    c1, y1 = _count_calls(monkeypatch, lambda: P1(x))
    print(arch, W, "P0", c0, "P1", c1)
    assert torch.equal(y1, y0), float((y1 - y0).abs().max())
    assert len(P1.stage_bits) == len(P0.stage_bits) == len(P0.report) - 1
    for i, (b1, b0) in enumerate(zip(P1.stage_bits, P0.stage_bits)):
        assert torch.equal(b1, b0), (P0.report[i]["name"], int((b1 != b0).sum()), b0.numel())
    # what was launched: no byte ends in P1, one launch of each new entry point; P0 as before
    assert not [n for n in BYTE_ENDS if n in c1] and [c1.get(n) for n in BIT_ENDS] == [1, 1], c1
    assert [c0.get(n) for n in BYTE_ENDS] == [1, 1, 1] and not [n for n in BIT_ENDS if n in c0], c0
    hidden = lambda c: {n: v for n, v in c.items() if n.startswith(("mn_bitconv", "mn_bits_maxpool"))}
    assert hidden(c1) == hidden(c0) and sum(hidden(c0).values()) >= 7
    # buffers: one set per input shape, reused by a second call; no int8 buffer in front of the last conv
    ws = next(iter(P1._ws.values()))
    ptrs = [t.data_ptr() for t in ws[0]]
    with torch.no_grad():
        y2 = P1(x)
    assert torch.equal(y2, y0)
    assert len(P1._ws) == 1 and ptrs == [t.data_ptr() for t in next(iter(P1._ws.values()))[0]]
    assert ws[2] is None and next(iter(P0._ws.values()))[2].dtype == torch.int8
    with pytest.raises(Exception, match="eval-only"):
        P1.train()


def test_bit_ends_names_an_input_the_first_kernel_does_not_cover():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    F, x = _folded("nin_gc", 3)
    P1 = inference.wbwtab_compile_bits(F, bit_ends=True)
    with pytest.raises(MicronetHipError, match=r"model\.0\.conv"):
        P1(x[:, :, :, :30].contiguous())


@pytest.mark.parametrize("arch", ["nin_gc", "nin"])
def test_plan_with_bit_ends_batch_256_equals_its_chunks(arch):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    from micronet_amd import inference
    F, _ = _folded(arch, 3)
    DG.plan_whole_against_chunks(inference.wbwtab_compile_bits(F, bit_ends=True), "stage_bits")
