"""``iao_compile_int8`` on whole nets (micronet_amd/inference.py: Int8Plan over csrc/qgemm_iao8.h), on the MI355X.

Nets: nin_gc, and a narrow nin_gc whose every block the int8 kernels cover (cfg 32, 32, 256, 64, 64, 512, 128, 128); each trained for two steps at batch 32 as in
tests/test_gpu_inference.py, folded and pre-quantised, run at batch 4.  The small cfg of tests/golden/inference_meta.json (32, 32, 32, 64, 64, 64, 128, 128) has 3x3
blocks of TWO channels per group, which mn_i8conv_supported refuses by the same rule that refuses eight (C / groups % 16 == 0 for a 3x3): on that net the walk must
raise naming the layer, and that is what its case checks -- the stage-by-stage checks cannot run on a net the plan refuses.

The judge is tests/iao8_cases.py's: the exact integer convolution of numpy on the judge's own codes, the contract's chain replayed in numpy float32.  Every hidden
stage, teacher-forced on the judge's input codes, must equal it bit for bit; the parent's path (the stage's own module on x = j * s_a, then the consumer's
quantizer) may differ from it by one step on at most 1e-4 of the elements."""
import copy
import importlib
import json
import os

import numpy as np
import pytest
import torch

import iao8_cases as IC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F = np.float32
NARROW = [32, 32, 256, 64, 64, 512, 128, 128]
KW = dict(a_bits=8, w_bits=8, q_type=0, q_level=0, weight_observer=0, bn_fuse=True)


def _small_cfg():
    return json.load(open(os.path.join(GOLDEN, "inference_meta.json")))["cfg"]


def _folded(cfg):
    """Two training steps at batch 32, then BN fold and pre-quantisation; returns (folded eval-mode model, the batch)."""
    from micronet_amd import inference
    from micronet_amd.models import nin_gc
    from micronet_amd.train import build_model, init_like_main, make_optimizer, synth_batch, train_step
    Q = importlib.import_module("micronet.compression.quantization.wqaq.iao.quantize")
    if cfg is None:
        net = build_model("nin_gc")
    else:
        torch.manual_seed(1)
        net = init_like_main(nin_gc.Net(cfg=cfg))
    m = Q.prepare(net, inplace=True, **KW).cuda().train()
    opt = make_optimizer(m, 0.01, 1e-5)
    x, y = synth_batch(32, device="cuda")
    for _ in range(2):
        train_step(m, opt, x, y)
    m.eval()
    I = inference.iao_model_bn_fuse(m)
    assert inference.prequantize_weights(I) == 9
    return I.eval(), x


@pytest.fixture(scope="module", params=["nin_gc", "narrow"])
def compiled(request):
    from micronet_amd import inference
    Fm, x = _folded(None if request.param == "nin_gc" else NARROW)
    P = inference.iao_compile_int8(Fm)
    return Fm, P, x[:4].contiguous()


def _np(t):
    return t.detach().float().cpu().numpy()


def _order(Cc, s):
    return IC.shuffle_order(Cc, s) if s else None


def _judge_chain(Fm, P, x):
    """The judge's codes of every stage, free of the code under test: [(codes in natural channel order, H, W)] -- entry 0 behind the first block, entry i + 1 behind
    hidden stage i -- and per stage the accumulator-to-code constants it used."""
    with torch.no_grad():
        a0 = _np(Fm.get_submodule(P.report[0]["name"])(x))
    stages = [IC.code_of(a0, P.pack["s"], P.pack["a_bits"]).astype(np.int8)]
    orders = [None if P.pack["order"] is None else P.pack["order"].cpu().numpy()]
    for L in P.layers:
        j = stages[-1]
        xin = j[:, orders[-1]] if orders[-1] is not None else j          # what the conv reads: its input through the channel shuffle
        s_w = _np(L["s_w"]).astype(F)
        sw_full = np.broadcast_to(s_w, (L["cout"],)).astype(F)
        k = np.rint(_np(L["w"]).astype(np.float64) / sw_full.reshape(-1, 1, 1, 1).astype(np.float64)).astype(np.int64)
        assert np.abs(k).max() <= 127
        acc = IC.O.conv2d_fwd(xin.astype(np.int64), k, None, padding=L["pad"], groups=L["groups"], acc=np.int64)
        al = (F(L["s_a"]) * sw_full).astype(F)
        b = _np(L["bias"]).astype(F) if L["bias"] is not None else np.zeros(L["cout"], dtype=F)
        stages.append(IC.chain_codes(acc, al, b, F(L["s_p"]), F(L["s_out"]), L["a_bits"], L["pool"]))
        orders.append(_order(L["cout"], L["shuffle"]))
    return stages, orders


def test_every_hidden_stage_equals_the_judge(compiled):
    Fm, P, x = compiled
    stages, orders = _judge_chain(Fm, P, x)
    for i, L in enumerate(P.layers):
        j, ref = stages[i], stages[i + 1]
        N, _, H, W = j.shape
        assert len(np.unique(ref)) > 32, "%s: the judge's codes take %d values: the test would be vacuous" % (L["name"], len(np.unique(ref)))
        xin = j[:, orders[i]] if orders[i] is not None else j
        got = P.run_stage(i, torch.from_numpy(IC.np_block(xin)).cuda(), N, H, W)
        OB = (L["cout"] + 15) // 16
        got = IC.np_unblock(got.cpu().numpy(), OB * 16, ref.shape[2], ref.shape[3])
        want = IC.expect_positions(ref, orders[i + 1], OB)
        bad = int((got != want).sum())
        print(L["name"], P.report[i + 1]["kernel"], "mismatches against the judge", bad, "of", got.size, "distinct codes", len(np.unique(ref)))
        assert bad == 0, (L["name"], bad, got.size)


def test_parent_path_is_within_one_step_of_the_judge(compiled):
    """Each stage's own module of the folded model on x = j * s_a, then the consumer's quantizer: at most one step, on at most 1e-4 of the elements."""
    Fm, P, x = compiled
    stages, _ = _judge_chain(Fm, P, x)
    with torch.no_grad():
        for i, L in enumerate(P.layers):
            xf = torch.from_numpy((stages[i].astype(F) * F(L["s_a"])).astype(F)).cuda()
            y = Fm.get_submodule(L["name"])(xf)
            if L["pool"]:
                y = Fm.get_submodule(L["pool_name"])(y)
            par = IC.code_of(_np(y), L["s_out"], L["a_bits"]).astype(np.int32)
            d = np.abs(par - stages[i + 1].astype(np.int32))
            print(L["name"], "flips against the parent's path", int((d != 0).sum()), "of", d.size, "largest", int(d.max()))
            assert d.max() <= 1 and (d != 0).mean() <= 1e-4, (L["name"], int(d.max()), float((d != 0).mean()))


def test_plan_output(compiled):
    Fm, P, x = compiled
    stages, orders = _judge_chain(Fm, P, x)
    P.keep_stages = True
    with torch.no_grad():
        p = P(x)
        p2 = P(x)
        f = Fm(x)
        L = P.layers[-1]
        y = torch.from_numpy((stages[-1].astype(F) * F(L["s_out"])).astype(F)).cuda()
        y = Fm.get_submodule(P.report[-1]["name"])(y)
        for m in P.tail:
            y = m(y)
        want = y.view(y.size(0), -1) if P.flatten else y
    P.keep_stages = False
    assert len(P._ws) == 1, "buffers are cached per input shape"
    assert torch.equal(p, p2)
    # free-running, the plan's stages are the judge's
    for got, ref, order, row in zip(P.stage_codes, stages, orders, P.report):
        CB = got.shape[1]
        assert np.array_equal(IC.np_unblock(got.cpu().numpy(), CB * 16, ref.shape[2], ref.shape[3]), IC.expect_positions(ref, order, CB)), row["name"]
    assert torch.equal(p, want), "the model's own last block and tail on the unpacked judge codes"
    err, top = float((p - f).abs().max()), float(f.abs().max())
    agree = float((p.argmax(1) == f.argmax(1)).float().mean())
    print("max|P - F| / max|F|", err / top, "argmax agreement", agree)
    assert err <= 2e-2 * top, err / top
    assert agree >= 0.9, agree


def test_plan_is_eval_only_and_reports(compiled):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    Fm, P, _ = compiled
    with pytest.raises(MicronetHipError, match="eval-only"):
        P.train()
    assert P.report == inference.iao_int8_report(Fm)
    assert [r["kind"] for r in P.report] == ["first"] + ["int8"] * 7 + ["last"]


def test_weights_off_the_grid_are_refused():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    Fm, _ = _folded(NARROW)
    bad = copy.deepcopy(Fm)
    conv = bad.model[5].conv
    conv.weight.data[3, 0, 0, 0] += 0.5 * conv.weight_quantizer.scale.reshape(-1)[3]
    with pytest.raises(MicronetHipError, match=r"model\.5\.conv: 1 rows whose stored weights are off the grid"):
        inference.iao_compile_int8(bad)
    # folded but not pre-quantised: the stored weights are fp32
    raw = copy.deepcopy(Fm)
    raw.model[2].conv.weight.data.mul_(1.003)
    with pytest.raises(MicronetHipError, match=r"model\.2\.conv: \d+ rows whose stored weights are off the grid"):
        inference.iao_compile_int8(raw)


def test_small_cfg_is_refused_naming_the_layer():
    """The small cfg of tests/golden/inference_meta.json: its 3x3 blocks have two channels per group (see the module docstring)."""
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    Fm, x = _folded(_small_cfg())
    with pytest.raises(MicronetHipError, match=r"model\.4\.conv: geometry not covered by mn_i8conv_supported \(3x3, stride 1, padding 1, dilation 1, groups 16, 2 channels"):
        inference.iao_compile_int8(Fm)
    with torch.no_grad():
        assert Fm(x[:4]).shape == (4, 10)          # the caller still has the model


def test_plan_batch_256_equals_its_chunks(compiled):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    DG.plan_whole_against_chunks(compiled[1], "stage_codes")
