"""``iao_compile_int8(model, end_to_end=True)`` on BN-folded IAO ResNets (micronet_amd/inference.py: Int8ResPlan with the two ends of csrc/qgemm_iao8_e2e.h), on the
MI355X.

Nets: those of tests/test_gpu_iao8_res_plan.py -- ``ResNet(BasicBlock, [1, 1, 1, 1])`` and ``ResNet(BottleNeck, [1, 1, 1, 1])``, IAO W8A8 and W4A4 with
``bn_fuse=True``, two training steps at batch 32, folded and pre-quantised (the classifier's weights too: ``fc.quant_inference = True``) -- run at batch 3 on
16 x 16 images.

The judge starts from its OWN codes of the fp32 image (``code_of`` at conv1's activation scale), convolves them exactly, replays the chain up to r in numpy float32
and forms one code map per consumer quantizer; the stages are tests/test_gpu_iao8_res_plan.py's judge; the logits tests/iao8_e2e_cases.py's (the fp64 pooled value,
its fp32 code, int64 sums, the fp32 chain).  ``run_first``, every free-running code map and the logits (as uint32) must equal it bit for bit.  The folded model's own
modules may differ from the judge by one step on at most 1e-4 of each of conv1's maps (eight 32 x 32 images: 524 288 elements a map), and by the float
accumulate's bound 1e-5 (sum |j k| al + |b|) on the logits.  max|P - F| / max|F| is printed for this plan and the default one, not asserted."""
import copy
import importlib

import numpy as np
import pytest
import torch

import iao8_cases as IC
import iao8_e2e_cases as XC
import iao8_res_cases as RC
from test_gpu_iao8_res_plan import NETS, _blocked, _exact_conv, _judge_stage, _np

pytestmark = pytest.mark.gpu

F = np.float32


def _folded(kind, bits):
    """Two training steps at batch 32, then BN fold and pre-quantisation of every conv and of the classifier; returns (folded eval-mode model, the training batch)."""
    from micronet_amd import inference
    from micronet_amd.models import resnet
    from micronet_amd.train import init_like_main, make_optimizer, synth_batch, train_step
    Q = importlib.import_module("micronet.compression.quantization.wqaq.iao.quantize")
    torch.manual_seed(1)
    net = init_like_main(resnet.ResNet(resnet.BasicBlock if kind == "basic" else resnet.BottleNeck, [1, 1, 1, 1]))
    m = Q.prepare(net, inplace=True, a_bits=bits, w_bits=bits, q_type=0, q_level=0, weight_observer=0, bn_fuse=True).cuda().train()
    opt = make_optimizer(m, 0.01, 1e-5)
    x, y = synth_batch(32, device="cuda")
    for _ in range(2):
        train_step(m, opt, x, y)
    m.eval()
    I = inference.iao_model_bn_fuse(m)
    I.fc.quant_inference = True
    assert inference.prequantize_weights(I) >= (13 if kind == "basic" else 18)
    return I.eval(), x


def _codes_of_weights(L):
    sw_full = np.broadcast_to(_np(L["s_w"]).astype(F), (L["cout"],)).astype(F)
    shape = (-1,) + (1,) * (L["w"].dim() - 1)
    k = np.rint(_np(L["w"]).astype(np.float64) / sw_full.reshape(shape).astype(np.float64)).astype(np.int64)
    assert np.abs(k).max() <= 127
    return k, sw_full


def _judge_first(P, x):
    """[int8 codes [N, C, H, W] per output map of conv1] from the judge's own codes of the image."""
    Lf = P.ends[0]
    jx = IC.code_of(_np(x), Lf["s_a"], Lf["in_bits"]).astype(np.int64)
    k, sw_full = _codes_of_weights(Lf)
    acc = _exact_conv(jx, k, 1, Lf["pad"])
    assert np.abs(acc).max() < 2 ** 31
    b = _np(Lf["bias"]).astype(F) if Lf["bias"] is not None else np.zeros(Lf["cout"], dtype=F)
    y = RC.chain_y(acc, (F(Lf["s_a"]) * sw_full).astype(F), b)
    r = np.where(y > 0, y, F(0)).astype(F)
    return [IC.code_of(r, s, bits).astype(np.int8) for s, bits in zip(Lf["s_out"], Lf["out_bits"])]


def _fc_case(P, codes):
    Ll = P.ends[1]
    k, sw_full = _codes_of_weights(Ll)
    return dict(c=codes, k=k, al=(F(Ll["s_fc"]) * sw_full).astype(F), b=_np(Ll["bias"]).astype(F) if Ll["bias"] is not None else None, s_p=F(Ll["s_p"]),
                s_fc=F(Ll["s_fc"]), bits=(Ll["p_bits"], Ll["a_bits"], Ll["w_bits"]))


def _judge_chain(P, x):
    """({code map: int8 codes}, logits) of the whole plan, free of the code under test."""
    maps = {o["buf"]: ref for o, ref in zip(P.stem["outs"], _judge_first(P, x))}
    for L in P.layers:
        for o, ref in zip(L["outs"], _judge_stage(L, maps[L["src"]], maps[L["sc"]] if L["sc"] is not None else None)):
            maps[o["buf"]] = ref
    return maps, XC.poolfc_judge(_fc_case(P, maps[P.tail_q["buf"]]))


@pytest.fixture(scope="module", params=NETS, ids=["%s_w%da%d" % (k, b, b) for k, b in NETS])
def compiled(request):
    from micronet_amd import inference
    Fm, x32 = _folded(*request.param)
    P = inference.iao_compile_int8(Fm, end_to_end=True)
    x = x32[:3, :, :16, :16].contiguous()          # three 16 x 16 images: maps of 16, 8, 4, 2 pixels a side
    maps, (m, j, acc, logits) = _judge_chain(P, x)
    return Fm, P, x, maps, logits, x32


def _same_codes(got, ref):
    CB = got.shape[1]
    return np.array_equal(IC.np_unblock(got.cpu().numpy(), CB * 16, ref.shape[2], ref.shape[3]), IC.expect_positions(ref, None, CB))


def test_run_first_equals_the_judge_on_both_maps(compiled):
    Fm, P, x, maps, _, _ = compiled
    outs = P.run_first(x)
    assert len(outs) == len(P.stem["outs"]) == 2
    for o, got in zip(P.stem["outs"], outs):
        ref = maps[o["buf"]]
        print("conv1 ->", o["consumer"], ref.shape, "distinct codes", len(np.unique(ref)))
        assert _same_codes(got, ref), o["consumer"]
    # two quantizers, two maps -- unless both observed the same tensor (a BottleNeck's first conv and its shortcut conv both read conv1's output: one scale)
    s0, s1 = P.ends[0]["s_out"]
    assert np.array_equal(maps[P.stem["outs"][0]["buf"]], maps[P.stem["outs"][1]["buf"]]) == (s0 == s1), (s0, s1)
    assert max(len(np.unique(maps[o["buf"]])) for o in P.stem["outs"]) > (32 if P.ends[0]["out_bits"][0] == 8 else 4)


def test_plan_free_running_equals_the_judge_chain(compiled):
    from micronet_amd import inference
    Fm, P, x, maps, logits, _ = compiled
    P.keep_stages = True
    with torch.no_grad():
        p, p2 = P(x), P(x)
    P.keep_stages = False
    assert torch.equal(p, p2) and len(P.stage_codes) == len(maps) == len(P.buffers)
    for b, got in enumerate(P.stage_codes):
        assert _same_codes(got, maps[b]), "code map %d" % b
    assert p.shape == logits.shape and np.array_equal(p.cpu().numpy().view(np.uint32), logits.view(np.uint32)), "the logits, bit for bit"
    ref = maps[P.tail_q["buf"]]
    last = P.run_last(_blocked(ref), ref.shape[0], ref.shape[2], ref.shape[3])
    assert np.array_equal(last.cpu().numpy().view(np.uint32), logits.view(np.uint32)), "run_last on the judge's codes"
    assert P.report == inference.iao_int8_report(Fm, (16, 16), end_to_end=True)
    kinds = [r["kind"] for r in P.report]
    assert kinds[0] == "int8_first" and kinds[-1] == "int8_last" and set(kinds[1:-1]) == {"int8", "int8_add"}
    assert P.report[0]["kernel"] == "k_i8first2<3,2>" and P.report[-1]["kernel"] == "k_i8poolfc"


def test_batch_six_equals_its_two_chunks(compiled):
    Fm, P, x, _, _, x32 = compiled
    x6 = x32[:6, :, :16, :16].contiguous()
    with torch.no_grad():
        whole = P(x6)
        parts = torch.cat([P(x6[:3].contiguous()), P(x6[3:].contiguous())])
    assert torch.equal(whole, parts)
    assert np.array_equal(whole[:3].cpu().numpy().view(np.uint32), compiled[4].view(np.uint32))


def test_models_own_ends_are_within_the_cap_of_the_judge(compiled):
    """conv1 of the folded model on eight 32 x 32 training images: at most one step, on at most 1e-4 of each map of the judge (524 288 elements a map); the model's
    avg_pool and fc on the judge's de-quantised codes: within 1e-5 (sum |j k| al + |b|) of the judge's logits."""
    Fm, P, x, maps, logits, x32 = compiled
    Fm = copy.deepcopy(Fm)
    xbig = x32[:8].contiguous()
    with torch.no_grad():
        a0 = _np(Fm.conv1(xbig))
    Lf = P.ends[0]
    for ref, s, bits, o in zip(_judge_first(P, xbig), Lf["s_out"], Lf["out_bits"], P.stem["outs"]):
        d = np.abs(IC.code_of(a0, s, bits).astype(np.int32) - ref.astype(np.int32))
        print("conv1 ->", o["consumer"], "flips against the model's own conv1", int((d != 0).sum()), "of", d.size, "largest", int(d.max()))
        assert d.size == 524288 and d.max() <= 1 and (d != 0).mean() <= 1e-4
    ref = maps[P.tail_q["buf"]]
    case = _fc_case(P, ref)
    _, j, _, _ = XC.poolfc_judge(case)
    with torch.no_grad():
        y = Fm.avg_pool(torch.from_numpy((ref.astype(F) * case["s_p"]).astype(F)).cuda())
        own = _np(Fm.fc(y.view(y.size(0), -1)))
    b = np.abs(case["b"]).reshape(1, -1) if case["b"] is not None else 0.0
    bound = 1e-5 * ((np.abs(j) @ np.abs(case["k"]).T).astype(np.float64) * case["al"].reshape(1, -1).astype(np.float64) + b)
    err = np.abs(own.astype(np.float64) - logits.astype(np.float64))
    print("avg_pool + fc: largest |model - judge| / bound", float((err / bound).max()))
    assert (err <= bound).all()


def test_distance_to_the_fp32_model_is_printed(compiled):
    from micronet_amd import inference
    Fm, P, x, _, _, _ = compiled
    P0 = inference.iao_compile_int8(Fm)
    with torch.no_grad():
        f, p, p0 = Fm(x), P(x), P0(x)
    top = float(f.abs().max())
    print("max|P_e2e - F| / max|F|", float((p - f).abs().max()) / top, "max|P_default - F| / max|F|", float((p0 - f).abs().max()) / top,
          "argmax agreement", float((p.argmax(1) == f.argmax(1)).float().mean()))
    assert P0.report[0]["kind"] == "first" and P0.ends is None, "the default plan is the default plan"


def test_counters_refuse_naming_the_layer():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    Fm, _ = _folded("basic", 8)
    bad = copy.deepcopy(Fm)
    bad.fc.weight.data[3, 7] += 0.5 * bad.fc.weight_quantizer.scale.reshape(-1)[3 if bad.fc.weight_quantizer.scale.numel() > 1 else 0]
    with pytest.raises(MicronetHipError, match=r"end_to_end=True\): fc: 1 rows whose stored weights are off the grid"):
        inference.iao_compile_int8(bad, end_to_end=True)
    bad = copy.deepcopy(Fm)
    bad.conv1[0].activation_quantizer.scale.fill_(float("inf"))
    with pytest.raises(MicronetHipError, match=r"end_to_end=True\): conv1\.0: \d+ rows or scales with a non-finite or non-positive constant"):
        inference.iao_compile_int8(bad, end_to_end=True)
