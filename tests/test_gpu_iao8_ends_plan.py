"""``iao_compile_int8(model, byte_ends=True)`` on whole nets (micronet_amd/inference.py: Int8Plan over csrc/qgemm_iao8.h and csrc/qgemm_iao8_ends.h), on the MI355X.

The nets of tests/test_gpu_iao8_plan.py: nin_gc, and the narrow cfg 32, 32, 256, 64, 64, 512, 128, 128; each trained for two steps at batch 32, folded and
pre-quantised, run at batch 4.

The judge is never the code under test: the image's codes are ``code_of(x, s_a)`` in numpy, every contraction is ``oracle.np_oracle.conv2d_fwd(acc=np.int64)`` on the
judge's own codes, every chain is replayed in numpy float32 (tests/iao8_cases.py, tests/iao8_ends_cases.py); it is computed once per net.  Both ends and every hidden
stage must equal it bit for bit; the parent's path for the first block (the model's own block on x, then the consumer's quantizer) may differ from it by one step on at
most 1e-4 of the elements."""
import copy

import numpy as np
import pytest
import torch

import iao8_cases as IC
import iao8_ends_cases as EC
from test_gpu_iao8_plan import NARROW, _folded, _np, _order

pytestmark = pytest.mark.gpu

F = np.float32


def _acc(L, xin):
    """The exact accumulator of a layer dict on codes in the order the conv reads them, and its al and b."""
    s_w = np.broadcast_to(_np(L["s_w"]).astype(F), (L["cout"],)).astype(F)
    k = np.rint(_np(L["w"]).astype(np.float64) / s_w.reshape(-1, 1, 1, 1).astype(np.float64)).astype(np.int64)
    assert np.abs(k).max() <= 127
    acc = IC.O.conv2d_fwd(xin.astype(np.int64), k, None, padding=L["pad"], groups=L["groups"], acc=np.int64)
    b = _np(L["bias"]).astype(F) if L["bias"] is not None else np.zeros(L["cout"], dtype=F)
    return acc, (F(L["s_a"]) * s_w).astype(F), b


def _judge_chain(P, x):
    """(stages, orders, r): the judge's codes behind the first block and every hidden stage (natural channel order) with the shuffle each is read through, and the
    fp32 map behind the last block -- all started from the judge's own codes of the image."""
    Lf, Ll = P.ends
    acc, al, b = _acc(Lf, IC.code_of(_np(x), Lf["s_a"], Lf["in_bits"]))
    stages, orders = [IC.chain_codes(acc, al, b, F(Lf["s_out"]), F(Lf["s_out"]), Lf["a_bits"], 0)], [_order(Lf["cout"], Lf["shuffle"])]
    for L in P.layers:
        acc, al, b = _acc(L, stages[-1][:, orders[-1]] if orders[-1] is not None else stages[-1])
        stages.append(IC.chain_codes(acc, al, b, F(L["s_p"]), F(L["s_out"]), L["a_bits"], L["pool"]))
        orders.append(_order(L["cout"], L["shuffle"]))
    assert orders[-1] is None
    acc, al, b = _acc(Ll, stages[-1])
    return stages, orders, EC.chain_r(acc, al, b, Ll["relu"])


@pytest.fixture(scope="module", params=["nin_gc", "narrow"])
def compiled(request):
    from micronet_amd import inference
    Fm, x = _folded(None if request.param == "nin_gc" else NARROW)
    P = inference.iao_compile_int8(Fm, byte_ends=True)
    x = x[:4].contiguous()
    return Fm, P, x, _judge_chain(P, x)


def _blocked(codes, order):
    return torch.from_numpy(IC.np_block(codes[:, order] if order is not None else codes)).cuda()


def test_first_block_equals_the_judge(compiled):
    _, P, x, (stages, orders, _) = compiled
    ref = stages[0]
    assert len(np.unique(ref)) > 32, "the judge's codes take %d values: the test would be vacuous" % len(np.unique(ref))
    OB = (ref.shape[1] + 15) // 16
    got = IC.np_unblock(P.run_first(x).cpu().numpy(), OB * 16, ref.shape[2], ref.shape[3])
    bad = int((got != IC.expect_positions(ref, orders[0], OB)).sum())
    print(P.report[0]["kernel"], "mismatches against the judge", bad, "of", got.size, "distinct codes", len(np.unique(ref)))
    assert bad == 0, (bad, got.size)


def test_last_block_equals_the_judge(compiled):
    _, P, _, (stages, orders, r) = compiled
    N, _, H, W = stages[-1].shape
    got = P.run_last(_blocked(stages[-1], orders[-1]), N, H, W).cpu().numpy()
    bad = int((got.view(np.uint32) != r.view(np.uint32)).sum())
    print(P.report[-1]["kernel"], "words that differ from the judge", bad, "of", got.size, "largest |r|", float(np.abs(r).max()))
    assert got.shape == r.shape and bad == 0, (bad, got.size)
    assert (r > 0).any()


def test_plan_output(compiled):
    Fm, P, x, (stages, orders, r) = compiled
    P.keep_stages = True
    with torch.no_grad():
        p = P(x)
        p2 = P(x)
        f = Fm(x)
        y = torch.from_numpy(r).cuda()
        for m in P.tail:
            y = m(y)
        want = y.view(y.size(0), -1) if P.flatten else y
    P.keep_stages = False
    assert len(P._ws) == 1, "buffers are cached per input shape"
    assert torch.equal(p, p2)
    # free-running, the plan's stages are the judge's chain started from the judge's own first-block codes
    assert len(P.stage_codes) == len(stages)
    for got, ref, order, row in zip(P.stage_codes, stages, orders, P.report):
        CB = got.shape[1]
        assert np.array_equal(IC.np_unblock(got.cpu().numpy(), CB * 16, ref.shape[2], ref.shape[3]), IC.expect_positions(ref, order, CB)), row["name"]
    assert torch.equal(p, want), "the model's own tail on the judge's r"
    err, top = float((p - f).abs().max()), float(f.abs().max())
    agree = float((p.argmax(1) == f.argmax(1)).float().mean())
    print("max|P_ends - F| / max|F|", err / top, "argmax agreement", agree)
    assert err <= 2e-2 * top, err / top
    assert agree >= 0.9, agree


def test_parent_path_is_within_one_step_of_the_judge(compiled):
    """The model's own first block on x, then the consumer's quantizer: at most one step, on at most 1e-4 of the elements."""
    Fm, P, x, (stages, _, _) = compiled
    Lf = P.ends[0]
    with torch.no_grad():
        y = Fm.get_submodule(Lf["name"])(x)
    par = IC.code_of(_np(y), Lf["s_out"], Lf["a_bits"]).astype(np.int32)
    d = np.abs(par - stages[0].astype(np.int32))
    print(Lf["name"], "flips against the parent's path", int((d != 0).sum()), "of", d.size, "largest", int(d.max()))
    assert d.max() <= 1 and (d != 0).mean() <= 1e-4, (int(d.max()), float((d != 0).mean()))


def test_plan_is_eval_only_and_reports(compiled):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    Fm, P, _, _ = compiled
    with pytest.raises(MicronetHipError, match="eval-only"):
        P.train()
    assert P.report == inference.iao_int8_report(Fm, byte_ends=True)
    assert [r["kind"] for r in P.report] == ["int8_first"] + ["int8"] * 7 + ["int8_last"]


def test_weights_off_the_grid_are_refused_at_both_ends():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    Fm, _ = _folded(NARROW)
    for layer in (0, 10):
        bad = copy.deepcopy(Fm)
        conv = bad.model[layer].conv
        conv.weight.data[3, 0, 0, 0] += 0.5 * conv.weight_quantizer.scale.reshape(-1)[3]
        with pytest.raises(MicronetHipError, match=r"model\.%d\.conv: 1 rows whose stored weights are off the grid" % layer):
            inference.iao_compile_int8(bad, byte_ends=True)


def test_plan_batch_256_equals_its_chunks(compiled):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    DG.plan_whole_against_chunks(compiled[1], "stage_codes")
