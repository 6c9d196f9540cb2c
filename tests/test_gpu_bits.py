"""Bit-packed inference (micronet_amd.inference.wbwtab_compile_bits, csrc/qgemm_bits.hip) on the MI355X: the kernel checks of tests/bits_cases.py at full size, the
byte path against the bit path, and the compiled plan against the folded graph it was compiled from -- bit for bit."""
import importlib

import pytest
import torch

import abi_driver
import bits_cases as B
import kernel_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("Cc", [32, 80, 130, 256])
def test_pack_unpack_roundtrip(be, Cc):
    B.check_pack_roundtrip(be, Cc, seed=Cc)


@pytest.mark.parametrize("W", [3, 2])
@pytest.mark.parametrize("case", range(len(K.DEPLOYED_CASES)))
def test_bitconv_deployed_cases(be, case, W):
    B.check_bitconv(be, seed=700 + case, W=W, **K.DEPLOYED_CASES[case])


@pytest.mark.parametrize("W", [3, 2])
@pytest.mark.parametrize("layer", range(len(B.NIN_GC_LAYERS)))
def test_bitconv_nin_gc_geometries(be, layer, W):
    B.check_bitconv(be, seed=800 + layer, W=W, **B.nin_gc_case(layer, full=True))


@pytest.mark.parametrize("W", [3, 2])
def test_bitconv_two_channels_per_group(be, W):
    B.check_bitconv(be, seed=900, W=W, **B.TWO_PER_GROUP)


@pytest.mark.parametrize("case", [1, 3])
def test_consumer_order_and_pool(be, case):
    B.check_order_and_pool(be, seed=950 + case, **K.DEPLOYED_CASES[case])


@pytest.mark.parametrize("case", range(len(K.DEPLOYED_CASES)))
def test_byte_path_and_bit_path_agree(be, case):
    B.check_byte_vs_bit(be, seed=1000 + case, **K.DEPLOYED_CASES[case])


def _stage_codes(F, x):
    """The folded graph run child by child: {child name: int8 codes} for every +-1 stage output."""
    from micronet_amd.sign_tensor import SignTensor
    out, t = {}, x
    for name, m in F.model.named_children():
        t = m(t)
        if isinstance(t, SignTensor):
            out[name] = t.codes
    return out


def _check_stages(Bp, F, x):
    from micronet_amd import inference
    Bp.keep_stages = True
    with torch.no_grad():
        yb = Bp(x)
        ref = _stage_codes(F, x)
        yf = F(x)
    Bp.keep_stages = False
    hidden = [r for r in Bp.report if r["kind"] != "last"]
    assert len(hidden) == len(Bp.stage_bits)
    for i, (r, bits) in enumerate(zip(hidden, Bp.stage_bits)):
        want = ref[r["stage"]]
        got = inference.unpack_bits(bits, want.shape[1])
        order = Bp.layers[i - 1]["out_order"] if i > 0 else None
        if order is not None:          # bit j is channel order[j]: undo the consumer order
            phys = torch.empty_like(got)
            phys[:, order.long()] = got
            got = phys
        assert torch.equal(got, want), (r["name"], int((got != want).sum()), got.numel())
    assert torch.equal(yb, yf), float((yb - yf).abs().max())
    return yb


@pytest.mark.parametrize("W", [3, 2])
def test_compiled_plan_on_the_reference_trained_state(W):
    """The deployment flow of test_gpu_inference.py::test_wbwtab_bn_fused_graph_vs_reference_golden (state the reference trained, weights pre-quantised, then folded):
    every hidden stage's bits equal the folded graph's codes, the logits are bit-identical, and the classes agree with the oracle's folded graph."""
    from micronet_amd import inference
    from micronet_amd.train import synth_batch
    from oracle import torch_oracle as TO
    from test_gpu_inference import _inference_golden, _small_net
    Q = importlib.import_module("micronet.compression.quantization.wbwtab.quantize")
    g, meta = _inference_golden()
    key = "inf_wbwtab_w%d" % W
    orc2 = TO.prepare(_small_net(meta), "wbwtab", inplace=True, A=2, W=W)
    orc2.load_state_dict({k[len(key) + 9:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith(key + "_trained_")})
    with torch.no_grad():
        for m in orc2.modules():
            if isinstance(m, TO.OConv2d) and m.scheme == "wbwtab":
                m.weight.data = TO.wbwtab_weight(m.weight, W).detach().clone()
    OF2 = TO.bn_fuse_wbwtab(orc2, W).eval()
    I2 = Q.prepare(_small_net(meta), inplace=True, A=2, W=W, quant_inference=True)
    I2.load_state_dict(orc2.state_dict())
    F2 = inference.wbwtab_model_bn_fuse(I2.cuda(), W=W).eval()
    Bp = inference.wbwtab_compile_bits(F2)
    x, _ = synth_batch(4)
    lg = _check_stages(Bp, F2, x.cuda())
    with torch.no_grad():
        assert bool((lg.argmax(1).cpu() == OF2(x).argmax(1)).float().mean() >= 0.75)


def _nin_gc_folded(W):
    from micronet_amd import inference
    from micronet_amd.train import build_model
    from test_gpu_inference import _trained
    Q, T, x = _trained("wbwtab", "nin_gc", dict(A=2, W=W), wd=0.0)
    I = Q.prepare(build_model("nin_gc"), inplace=True, A=2, W=W, quant_inference=True).cuda()
    I.load_state_dict(T.state_dict())
    inference.prequantize_weights(I)
    return inference.wbwtab_model_bn_fuse(I, W=W).eval(), x


@pytest.mark.parametrize("W", [3, 2])
def test_compiled_plan_full_size_nin_gc(W):
    """Full-size nin_gc, two training steps, prequantise + fold, batch 32: the plan's logits equal the folded graph's, twice in a row (the second call reuses the
    plan's buffers); between the first and the last conv only the bit kernels run."""
    from micronet_amd import _lib, inference
    F, x = _nin_gc_folded(W)
    Bp = inference.wbwtab_compile_bits(F)
    with torch.no_grad():
        f = F(x)
        b1 = Bp(x)
        nbuf = len(Bp._ws)
        ptrs = [t.data_ptr() for t in next(iter(Bp._ws.values()))[0]]
        b2 = Bp(x)
    assert torch.equal(b1, f) and torch.equal(b2, f), (float((b1 - f).abs().max()), float((b2 - f).abs().max()))
    assert len(Bp._ws) == nbuf == 1 and ptrs == [t.data_ptr() for t in next(iter(Bp._ws.values()))[0]]
    _check_stages(Bp, F, x)
    # ---- what ran
    lib = _lib.get_lib()
    torch.cuda.synchronize()
    buf = (_lib.ProfEntry * 192)()
    lib.mn_profile_collect(buf, 192)          # (drop anything recorded before)
    lib.mn_profile_enable(1)
    with torch.no_grad():
        Bp(x)
    torch.cuda.synchronize()
    n = lib.mn_profile_collect(buf, 192)
    lib.mn_profile_enable(0)
    names = {buf[i].name.decode(): int(buf[i].launches) for i in range(n)}
    print(names)
    assert not [k for k in names if k.startswith(("k_pws", "k_h_sign", "k_k3s", "k_bnh"))], names
    assert sum(v for k, v in names.items() if k.startswith("k_bitconv<")) == 7 and names.get("k_bits_pack") == 1 and names.get("k_bits_unpack") == 1, names
    kinds = [r["kind"] for r in Bp.report]
    assert kinds == ["first"] + ["bit"] * 7 + ["last"], kinds
    assert [i for i, r in enumerate(Bp.report) if r["pooled"]] == [2, 5], Bp.report          # nin_gc's two pools, attributed to the blocks in front of them
    assert all(set(r) >= {"name", "kind", "K", "words", "kernel", "pooled", "out_order"} for r in Bp.report)
    assert [r["out_order"] for r in Bp.report[1:8]] == ["shuffle 2", "shuffle 2", "shuffle 16", "shuffle 4", "shuffle 4", "shuffle 32", "identity"]


def test_compile_bits_refuses_what_it_does_not_cover():
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    from micronet_amd.train import build_model
    Q = importlib.import_module("micronet.compression.quantization.wbwtab.quantize")
    I = Q.prepare(build_model("nin_gc"), inplace=True, A=2, W=3, quant_inference=True).cuda()
    F = inference.wbwtab_model_bn_fuse(I, W=3).eval()          # folded WITHOUT prequantize_weights
    with pytest.raises(MicronetHipError, match=r"model\.1\.conv"):
        inference.wbwtab_compile_bits(F)
    I32 = Q.prepare(build_model("nin_gc"), inplace=True, A=32, W=3, quant_inference=True).cuda()
    inference.prequantize_weights(I32)
    with pytest.raises(MicronetHipError):
        inference.wbwtab_compile_bits(inference.wbwtab_model_bn_fuse(I32, W=3).eval())


@pytest.mark.parametrize("W", [3, 2])
def test_compiled_plan_batch_256_equals_its_chunks(W):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    from micronet_amd import inference
    F, _ = _nin_gc_folded(W)
    DG.plan_whole_against_chunks(inference.wbwtab_compile_bits(F), "stage_bits")
