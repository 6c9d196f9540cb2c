"""``iao_compile_int8(model, zero_points=True)`` on whole nets prepared with ``q_type=1`` (micronet_amd/inference.py: Int8Plan over csrc/qgemm_iao8_zp.h), on the
MI355X.

Nets: nin_gc, and the narrow nin_gc of tests/test_gpu_iao8_plan.py (cfg 32, 32, 256, 64, 64, 512, 128, 128); each trained for two steps at batch 32, folded and
pre-quantised, run at batch 4.

The judge is tests/iao8_zp_cases.py's: the exact integer convolution of numpy on the integers code + z of the judge's own codes, the contract's chain replayed in numpy
float32.  Every hidden stage, teacher-forced on the judge's input codes, must equal it bit for bit; the stage's own module on the values of those codes, then the
consumer's quantizer, may differ from it by one step on at most 1e-4 of the elements."""
import importlib

import numpy as np
import pytest
import torch

import iao8_zp_cases as ZC
from iao8_cases import np_block, np_unblock, expect_positions, shuffle_order

pytestmark = pytest.mark.gpu

F = np.float32
NARROW = [32, 32, 256, 64, 64, 512, 128, 128]
KW = dict(a_bits=8, w_bits=8, q_type=1, q_level=0, weight_observer=0, bn_fuse=True)


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
    P = inference.iao_compile_int8(Fm, zero_points=True)
    return Fm, P, x[:4].contiguous()


def _np(t):
    return t.detach().float().cpu().numpy()


def _order(Cc, s):
    return shuffle_order(Cc, s) if s else None


def _quants(L):
    return (ZC.Q(L["s_a"], L["z_a"], L["asym_a"], L["in_bits"]), ZC.Q(L["s_p"], L["z_p"], L["asym_p"], L["a_bits"]), ZC.Q(L["s_out"], L["z_out"], L["asym_out"], L["a_bits"]))


def _judge_chain(Fm, P, x):
    """The judge's CODES of every stage, free of the code under test: [codes int32 in natural channel order] -- entry 0 behind the first block, entry i + 1 behind hidden
    stage i -- the channel orders, and the quantizer each entry's codes belong to."""
    with torch.no_grad():
        a0 = _np(Fm.get_submodule(P.report[0]["name"])(x))
    q0 = _quants(P.layers[0])[0]
    stages, quants = [ZC.code_of(a0, q0).astype(np.int32)], [q0]
    orders = [None if P.pack["order"] is None else P.pack["order"].cpu().numpy()]
    for L in P.layers:
        q_a, q_p, q_out = _quants(L)
        assert (q_a.s, q_a.z, q_a.asym, q_a.bits) == (quants[-1].s, quants[-1].z, quants[-1].asym, quants[-1].bits), "a stage reads the codes its producer wrote"
        c = stages[-1]
        xin = c[:, orders[-1]] if orders[-1] is not None else c          # what the conv reads: its input through the channel shuffle
        sw_full = np.broadcast_to(_np(L["s_w"]).astype(F), (L["cout"],)).astype(F)
        zw_full = np.broadcast_to(_np(L["z_w"]).astype(F), (L["cout"],)).astype(np.float64)
        assert np.array_equal(zw_full, np.rint(zw_full)) and float(q_a.z) == round(float(q_a.z))
        cw = np.rint(_np(L["w"]).astype(np.float64) / sw_full.reshape(-1, 1, 1, 1).astype(np.float64) - zw_full.reshape(-1, 1, 1, 1)).astype(np.int64)
        lo_w, hi_w = ZC.qrange(L["asym_w"], L["w_bits"], False)
        assert lo_w <= cw.min() and cw.max() <= hi_w
        J, K = xin.astype(np.int64) + int(q_a.z), cw + zw_full.reshape(-1, 1, 1, 1).astype(np.int64)
        S = ZC.O.conv2d_fwd(J, K, None, padding=L["pad"], groups=L["groups"], acc=np.int64)
        assert np.abs(S).max() < 2 ** 31
        al = (F(L["s_a"]) * sw_full).astype(F)
        b = _np(L["bias"]).astype(F) if L["bias"] is not None else np.zeros(L["cout"], dtype=F)
        stages.append(ZC.chain_codes(S, al, b, q_p, q_out, L["pool"]))
        quants.append(q_out)
        orders.append(_order(L["cout"], L["shuffle"]))
    return stages, orders, quants


def _bytes(codes, q):
    return (codes - ZC.qh(q.asym, q.bits)).astype(np.int8)


def test_the_net_is_asymmetric_and_refused_without_the_keyword(compiled):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    Fm, P, _ = compiled
    assert all(L["zp"] and L["asym_a"] and L["asym_w"] and L["asym_out"] for L in P.layers)
    assert any(float(L["z_w"].abs().max()) > 0 for L in P.layers), "weight zero points that are not 0"
    assert [r["kernel"].startswith("k_i8zconv<") for r in P.report[1:-1]] == [True] * 7
    with pytest.raises(MicronetHipError, match=r"is asymmetric; a zero byte must be the value 0 \(symmetric quantizers only\)"):
        inference.iao_compile_int8(Fm)


def test_every_hidden_stage_equals_the_judge(compiled):
    from micronet_amd import ops
    Fm, P, x = compiled
    stages, orders, quants = _judge_chain(Fm, P, x)
    for i, L in enumerate(P.layers):
        c, ref = stages[i], stages[i + 1]
        N, _, H, W = c.shape
        assert len(np.unique(ref)) > 32, "%s: the judge's codes take %d values: the test would be vacuous" % (L["name"], len(np.unique(ref)))
        xin = c[:, orders[i]] if orders[i] is not None else c
        got = P.run_stage(i, torch.from_numpy(np_block(_bytes(xin, quants[i]))).cuda(), N, H, W)
        assert ops.last_kernel() == P.report[i + 1]["kernel"] == "k_i8zconv<%d,%d>" % (L["k"], L["pool"])
        OB = (L["cout"] + 15) // 16
        got = np_unblock(got.cpu().numpy(), OB * 16, ref.shape[2], ref.shape[3])
        want = expect_positions(_bytes(ref, quants[i + 1]), orders[i + 1], OB)
        bad = int((got != want).sum())
        print(L["name"], P.report[i + 1]["kernel"], "z_a", L["z_a"], "z_out", L["z_out"], "mismatches against the judge", bad, "of", got.size, "distinct codes",
              len(np.unique(ref)))
        assert bad == 0, (L["name"], bad, got.size)


def test_the_stages_own_module_is_within_one_step_of_the_judge(compiled):
    """Each stage's own module of the folded model on the values of the judge's input codes, then the consumer's quantizer: at most one step, on at most 1e-4 of the
    elements."""
    Fm, P, x = compiled
    stages, _, quants = _judge_chain(Fm, P, x)
    with torch.no_grad():
        for i, L in enumerate(P.layers):
            xf = torch.from_numpy(ZC.value_of(stages[i], quants[i])).cuda()
            y = Fm.get_submodule(L["name"])(xf)
            if L["pool"]:
                y = Fm.get_submodule(L["pool_name"])(y)
            par = ZC.code_of(_np(y), quants[i + 1]).astype(np.int32)
            d = np.abs(par - stages[i + 1])
            print(L["name"], "flips against the stage's own module", int((d != 0).sum()), "of", d.size, "largest", int(d.max()))
            assert d.max() <= 1 and (d != 0).mean() <= 1e-4, (L["name"], int(d.max()), float((d != 0).mean()))


def test_plan_output(compiled):
    Fm, P, x = compiled
    stages, orders, quants = _judge_chain(Fm, P, x)
    P.keep_stages = True
    with torch.no_grad():
        p = P(x)
        p2 = P(x)
        f = Fm(x)
        y = torch.from_numpy(ZC.value_of(stages[-1], quants[-1])).cuda()
        y = Fm.get_submodule(P.report[-1]["name"])(y)
        for m in P.tail:
            y = m(y)
        want = y.view(y.size(0), -1) if P.flatten else y
    P.keep_stages = False
    assert len(P._ws) == 1, "buffers are cached per input shape"
    assert torch.equal(p, p2)
    # free-running, the plan's stages are the judge's
    for got, ref, order, q, row in zip(P.stage_codes, stages, orders, quants, P.report):
        CB = got.shape[1]
        assert np.array_equal(np_unblock(got.cpu().numpy(), CB * 16, ref.shape[2], ref.shape[3]), expect_positions(_bytes(ref, q), order, CB)), row["name"]
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
    assert P.report == inference.iao_int8_report(Fm, zero_points=True)
    assert [r["kind"] for r in P.report] == ["first"] + ["int8"] * 7 + ["last"]
    assert "k_i8z_pack" in P.report[0]["kernel"] and "k_i8z_unpack" in P.report[-1]["kernel"]


def test_table_counters_are_refused_naming_the_layer(compiled):
    """What the packer counts in the header words 13, 14 and 15 of a zero-point table, read back by ``iao_compile_int8`` and raised naming the layer.  model.4 is the
    first 3x3 stage (16 channels per group, 144 products per output) of both nets."""
    import copy
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    Fm = compiled[0]

    def refused(match, change):
        bad = copy.deepcopy(Fm)
        change(bad.model[4].conv)
        with pytest.raises(MicronetHipError, match=match):
            inference.iao_compile_int8(bad, zero_points=True)

    # the value 0 is no code of the input quantizer: codes 0 .. 255 stand for 3 .. 258
    refused(r"model\.4\.conv: zero padding has no byte: the value 0 is not a code of the input quantizer \(zero point 3\)", lambda c: c.activation_quantizer.zero_point.fill_(3.0))
    # model.4's table (input zero point) and model.2's (its consumer's zero point) both count it: the first in the net's order is named
    refused(r"model\.2\.conv: 1 zero points \(of the input, pool and consumer quantizers and the rows' z_w\) that are not integers", lambda c: c.activation_quantizer.zero_point.fill_(0.5))

    def wide(c):
        # every weight zero point 300 lower with the codes kept (w = (code + z) s stays on the grid), the input zero point at its bound:
        # 144 * (128 + 65407) * (127 + ~300) > 2^31 - 1
        s = c.weight_quantizer.scale.reshape(-1, 1, 1, 1)
        c.weight.data.add_(-300.0 * s)
        c.weight_quantizer.zero_point.add_(-300.0)
        c.activation_quantizer.zero_point.fill_(-65535.0)
    refused(r"model\.4\.conv: %d rows whose sum over 16 channels x 9 taps does not fit int32 at these zero points" % Fm.model[4].conv.out_channels, wide)


def test_plan_batch_256_equals_its_chunks(compiled):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    DG.plan_whole_against_chunks(compiled[1], "stage_codes")
