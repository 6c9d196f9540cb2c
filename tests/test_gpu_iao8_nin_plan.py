"""``iao_compile_int8(model, tile_blocks=True)`` on a narrow plain nin (cfg 32, 32, 16, 32, 32, 32, 32, 32), with and without ``byte_ends``, on the MI355X: two training
steps at batch 32 as in tests/test_gpu_iao8_plan.py, folded and pre-quantised, run at batch 6.

The judge is never the code under test: every contraction is ``oracle.np_oracle.conv2d_fwd(acc=np.int64)`` on the judge's own previous codes (asserted within int32),
every chain is replayed in numpy float32 (tests/iao8_cases.py); a stage with an un-folded pool is the block's chain at the pool quantizer's scale, then the window
maximum and its requantisation (tests/iao8_tile_cases.py: np_pool).  Every stage must equal it bit for bit."""
import importlib

import numpy as np
import pytest
import torch

import iao8_cases as IC
import iao8_ends_cases as EC
import iao8_tile_cases as TC
from test_gpu_iao8_ends_plan import _acc
from test_gpu_iao8_plan import KW, _np
from test_iao8_tile_host import CFG

pytestmark = pytest.mark.gpu

F = np.float32


def _judge_chain(Fm, P, x):
    """(stages, logits): the judge's codes behind the first block and every hidden stage, and the model's own tail on the judge's last map."""
    if P.ends:
        Lf = P.ends[0]
        acc, al, b = _acc(Lf, IC.code_of(_np(x), Lf["s_a"], Lf["in_bits"]))
        stages = [IC.chain_codes(acc, al, b, F(Lf["s_out"]), F(Lf["s_out"]), Lf["a_bits"], 0)]
    else:
        stages = [IC.code_of(_np(Fm.get_submodule(P.report[0]["name"])(x)), P.pack["s"], P.pack["a_bits"]).astype(np.int8)]
    for L in P.layers:
        acc, al, b = _acc(L, stages[-1])
        assert np.abs(acc).max() < 2 ** 31 and not L["shuffle"] and not L["pool"]
        s_blk = F(L["s_p"] if L["pool_ksp"] else L["s_out"])
        c = IC.chain_codes(acc, al, b, s_blk, s_blk, L["a_bits"], 0)
        stages.append(TC.np_pool(c, F(L["s_p"]), F(L["s_out"]), L["a_bits"], L["pool_ksp"]) if L["pool_ksp"] else c)
    if P.ends:
        y = torch.from_numpy(EC.chain_r(*_acc(P.ends[1], stages[-1]), P.ends[1]["relu"])).cuda()
    else:
        y = Fm.get_submodule(P.report[-1]["name"])(torch.from_numpy((stages[-1].astype(F) * F(P.layers[-1]["s_out"])).astype(F)).cuda())
    for m in P.tail:
        y = m(y)
    return stages, y.view(y.size(0), -1)


@pytest.fixture(scope="module")
def folded():
    from micronet_amd import inference
    from micronet_amd.models import nin
    from micronet_amd.train import init_like_main, make_optimizer, synth_batch, train_step
    Q = importlib.import_module("micronet.compression.quantization.wqaq.iao.quantize")
    torch.manual_seed(1)
    m = Q.prepare(init_like_main(nin.Net(cfg=CFG)), inplace=True, **KW).cuda().train()
    opt = make_optimizer(m, 0.01, 1e-5)
    x, y = synth_batch(32, device="cuda")
    for _ in range(2):
        train_step(m, opt, x, y)
    I = inference.iao_model_bn_fuse(m.eval())
    assert inference.prequantize_weights(I) == 9
    return I.eval(), x[:6].contiguous()


@pytest.mark.parametrize("byte_ends", [False, True])
def test_nin_plan(folded, byte_ends):
    from micronet_amd import inference
    Fm, x = folded
    P = inference.iao_compile_int8(Fm, byte_ends=byte_ends, tile_blocks=True)
    assert P.report == inference.iao_int8_report(Fm, byte_ends=byte_ends, tile_blocks=True)
    assert [r["kernel"] for r in P.report[1:-1]].count("k_i8_maxpool") == 2 and P.report[4]["kernel"] == "k_i8conv5<5>"
    with torch.no_grad():
        stages, want = _judge_chain(Fm, P, x)
        # teacher-forced: every stage alone on the judge's own previous codes
        for i, L in enumerate(P.layers):
            j, ref = stages[i], stages[i + 1]
            N, _, H, W = j.shape
            got = IC.np_unblock(P.run_stage(i, torch.from_numpy(IC.np_block(j)).cuda(), N, H, W).cpu().numpy(), (L["cout"] + 15) // 16 * 16, *ref.shape[2:])
            bad = int((got != IC.expect_positions(ref, None, (L["cout"] + 15) // 16)).sum())
            print(L["name"], L["pool_ksp"], "mismatches against the judge", bad, "of", got.size, "distinct codes", len(np.unique(ref)))
            assert len(np.unique(ref)) > 32, "%s: the judge's codes take %d values: the test would be vacuous" % (L["name"], len(np.unique(ref)))
            assert bad == 0, (L["name"], bad, got.size)
        # free-running: the kept stages (a pooled stage's map is the post-pool map) and the logits
        P.keep_stages = True
        p, p2, f = P(x), P(x), Fm(x)
        P.keep_stages = False
    assert len(P._ws) == 1 and torch.equal(p, p2) and len(P.stage_codes) == len(stages)
    for got, ref in zip(P.stage_codes, stages):
        assert np.array_equal(IC.np_unblock(got.cpu().numpy(), got.shape[1] * 16, *ref.shape[2:]), IC.expect_positions(ref, None, got.shape[1]))
    assert torch.equal(p, want), "the model's own last block and tail on the judge's codes"
    err, top = float((p - f).abs().max()), float(f.abs().max())
    agree = float((p.argmax(1) == f.argmax(1)).float().mean())
    print("byte_ends", byte_ends, "max|P - F| / max|F|", err / top, "argmax agreement", agree)
    assert err <= 2e-2 * top, err / top
    assert agree >= 0.9, agree
