"""Bit-packed deployment of the plain nin net on the MI355X: the kernel table of tests/bits_nin_cases.py at full size, the pools against torch, and the compiled plan
against the folded graph it was compiled from (bit for bit) and against the reference's folded nin (tests/golden/inference_nin.npz)."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import abi_driver
import bits_nin_cases as BN

pytestmark = pytest.mark.gpu
SEEN = set()


@pytest.fixture(scope="module")
def be():
    return abi_driver.Backend("gpu")


@pytest.mark.parametrize("W", [3, 2])
@pytest.mark.parametrize("case", range(len(BN.SMALL)))
def test_small_cases(be, case, W):
    SEEN.add(BN.check_case(be, seed=1100 + case, W=W, **BN.SMALL[case]))


@pytest.mark.parametrize("W", [3, 2])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("layer", range(len(BN.NIN_LAYERS)))
def test_nin_layers_full_size(be, layer, n, W):
    SEEN.add(BN.check_case(be, seed=1200 + layer, W=W, **BN.nin_case(layer, n=n)))


def test_nin_3x3_block_on_the_tiled_kernel(be):
    """nin's 192 -> 192 3x3 block on the LDS-tiled kernel (measurement-only dispatch: the plan keeps k_bitconv<3,0,0> for it)."""
    case = BN.nin_case(5, n=5)
    assert BN.check_case(be, seed=1250, W=3, alt=True, **case) == "k_bitconv_tile<3,6>"
    case = BN.nin_case(2, n=5)
    assert BN.check_case(be, seed=1251, W=3, alt=True, **case) == "k_bitconv_direct<5>"


def test_tiled_block_honours_the_consumer_order(be):
    BN.check_consumer_order(be, seed=1300)


@pytest.mark.parametrize("hw", BN.POOL_MAPS)
@pytest.mark.parametrize("ksp", BN.POOLS)
def test_standalone_pool(be, ksp, hw):
    SEEN.add(BN.check_standalone_pool(be, *ksp, *hw, seed=1400 + hw[1]))


@pytest.mark.parametrize("hw", BN.POOL_MAPS)
@pytest.mark.parametrize("ksp", BN.POOLS)
def test_folded_pool(be, ksp, hw):
    SEEN.add(BN.check_folded_pool(be, *ksp, *hw, seed=1500 + hw[1]))


@pytest.mark.parametrize("case", range(len(BN.LARGE_GRID)), ids=[c[0] for c in BN.LARGE_GRID])
def test_several_output_words_per_block(be, case):
    """The launch shape of the measured batches: a block walks more than one output word, the last block fewer (proved through mn_deploy_grid_deal)."""
    BN.check_large(be, case)


def test_refusals_keep_refusing(be):
    BN.check_refusals(be)


def test_every_new_instantiation_ran(be):
    SEEN.add("k_bitconv_tile<3,6>"), SEEN.add("k_bitconv_direct<5>")          # (asserted by name in test_nin_3x3_block_on_the_tiled_kernel)
    assert BN.INSTANTIATIONS <= SEEN, sorted(BN.INSTANTIATIONS - SEEN)


# ------------------------------------------------------------------------------------------------ the compiled plan
def _stage_codes(F, x):
    """The folded graph run child by child: {child name: int8 codes} for every +-1 stage output (a SignTensor, or -- behind the stock 3x3 / 2 max-pool -- fp32 +-1)."""
    from micronet_amd.sign_tensor import SignTensor
    out, t = {}, x
    for name, m in F.model.named_children():
        t = m(t)
        if isinstance(t, SignTensor):
            out[name] = t.codes
        elif torch.is_tensor(t) and t.dim() == 4 and bool((t.float().abs() == 1).all()):
            out[name] = t.float().to(torch.int8)
    return out


def _check_stages(Bp, F, x):
    """tests/test_gpu_bits.py:_check_stages with the stage reader above: every hidden stage's signs and the logits equal the folded graph's."""
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
        if order is not None:
            phys = torch.empty_like(got)
            phys[:, order.long()] = got
            got = phys
        assert torch.equal(got, want), (r["name"], int((got != want).sum()), got.numel())
    assert torch.equal(yb, yf), float((yb - yf).abs().max())
    return yb


def _nin_folded(W):
    from micronet_amd import inference
    from micronet_amd.train import build_model
    from test_gpu_inference import _trained
    Q, T, x = _trained("wbwtab", "nin", dict(A=2, W=W), wd=0.0)
    I = Q.prepare(build_model("nin"), inplace=True, A=2, W=W, quant_inference=True).cuda()
    I.load_state_dict(T.state_dict())
    inference.prequantize_weights(I)
    return inference.wbwtab_model_bn_fuse(I, W=W).eval(), x


@pytest.mark.parametrize("W", [3, 2])
def test_compiled_plan_full_size_nin(W):
    """Fails without the feature (MicronetHipError: geometry not covered).  Full-size nin, two training steps, prequantise + fold: every hidden stage's signs and the
    logits equal the folded graph's -- the last block and the tail are the folded graph's own modules on identical +-1 inputs, so equality is the claim -- twice in a
    row (buffer reuse) and at a second batch size; between the first and the last conv only bit kernels run."""
    from micronet_amd import _lib, inference
    F, x = _nin_folded(W)
    Bp = inference.wbwtab_compile_bits(F)
    assert isinstance(Bp, inference.BitPlan) and Bp.report == inference.wbwtab_bits_report(F)
    with torch.no_grad():
        f = F(x)
        b1 = Bp(x)
        ptrs = [t.data_ptr() for t in next(iter(Bp._ws.values()))[0]]
        b2 = Bp(x)
    assert torch.equal(b1, f) and torch.equal(b2, f), (float((b1 - f).abs().max()), float((b2 - f).abs().max()))
    assert len(Bp._ws) == 1 and ptrs == [t.data_ptr() for t in next(iter(Bp._ws.values()))[0]]
    _check_stages(Bp, F, x)
    _check_stages(Bp, F, x[:5].contiguous())          # a second batch size: a second set of buffers
    assert len(Bp._ws) == 2
    lib = _lib.get_lib()
    torch.cuda.synchronize()
    buf = (_lib.ProfEntry * 192)()
    lib.mn_profile_collect(buf, 192)
    lib.mn_profile_enable(1)
    with torch.no_grad():
        Bp(x)
    torch.cuda.synchronize()
    n = lib.mn_profile_collect(buf, 192)
    lib.mn_profile_enable(0)
    names = {buf[i].name.decode(): int(buf[i].launches) for i in range(n)}
    print(names)
    assert not [k for k in names if k.startswith(("k_pws", "k_h_sign", "k_k3s", "k_bnh"))], names
    assert names.get("k_bitconv_tile<5,3>") == 1 and names.get("k_bitconv1_pool3<8>") == 2 and names.get("k_bitconv<3,0,0>") == 1 and names.get("k_bitconv<1,0,0>") == 3, names
    assert names.get("k_bits_pack") == 1 and names.get("k_bits_unpack") == 1 and "k_bits_maxpool" not in names, names


def test_compiled_plan_with_a_standalone_pool():
    """A 3x3 / 2 pool directly behind the 5x5 block cannot be folded: the plan runs mn_bits_maxpool and still equals the folded graph."""
    from micronet_amd import inference
    from micronet_amd.models import nin
    from micronet_amd.train import init_like_main, synth_batch
    Q = importlib.import_module("micronet.compression.quantization.wbwtab.quantize")
    torch.manual_seed(3)
    net = init_like_main(nin.Net(cfg=[32, 32, 32, 64, 64, 64, 64, 64]))
    seq = list(net.model)
    seq.insert(5, torch.nn.MaxPool2d(3, 2, 1))
    del seq[8]
    net.model = torch.nn.Sequential(*seq)
    I = Q.prepare(net, inplace=True, A=2, W=3, quant_inference=True).cuda()
    inference.prequantize_weights(I)
    F = inference.wbwtab_model_bn_fuse(I, W=3).eval()
    Bp = inference.wbwtab_compile_bits(F)
    assert [r["pooled"] for r in Bp.report if r["name"] == "model.4"] == ["standalone"]
    x, _ = synth_batch(4)
    _check_stages(Bp, F, x.cuda())


@pytest.mark.parametrize("W", [3, 2])
def test_compiled_plan_on_the_reference_folded_nin(W):
    """The reference's own fold of a small nin (tests/golden/make_golden_nin.py) loaded into the folded graph: plan == folded graph bit for bit; against the reference's
    stage outputs at most 1e-4 of a stage's signs may differ and none where |pre-activation| > 1e-4 * max |pre-activation| (float rounding of the fp32 first conv is the
    only source: every hidden block is integer); logits within the project's float bound (1e-5 relative) when no hidden sign differs, else compared to the folded graph
    alone (which the equality above already does)."""
    from micronet_amd import inference
    from micronet_amd.models import nin
    Q = importlib.import_module("micronet.compression.quantization.wbwtab.quantize")
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g, meta = np.load(os.path.join(here, "inference_nin.npz")), json.load(open(os.path.join(here, "inference_nin_meta.json")))
    key = "nin_w%d" % W
    I = Q.prepare(nin.Net(cfg=meta["cfg"]), inplace=True, A=2, W=W, quant_inference=True)
    F = inference.wbwtab_model_bn_fuse(I, W=W).eval()
    F.load_state_dict({k[len(key) + 7:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith(key + "_fused_")})
    F = F.cuda()
    for m in F.modules():
        if isinstance(m, Q.QuantConv2d):
            mag = m.weight.detach().abs().flatten(1)
            assert bool(((mag == 0) | (mag == mag.amax(1, keepdim=True))).all())          # the reference folded pre-quantised weights: codes x alpha
            inference.mark_stored_codes(m)
    Bp = inference.wbwtab_compile_bits(F)
    x = torch.from_numpy(g["x"].copy()).cuda()
    lg = _check_stages(Bp, F, x)
    Bp.keep_stages = True
    with torch.no_grad():
        Bp(x)
    Bp.keep_stages = False
    hidden = [r for r in Bp.report if r["kind"] != "last"]
    by_stage = {r["stage"]: inference.unpack_bits(b, b.shape[1] * 32)[:, :] for r, b in zip(hidden, Bp.stage_bits)}
    total = 0
    for rec in meta[key]["stages"]:
        if rec["name"] not in by_stage:
            continue          # (a block whose pool is folded in has no un-pooled stage in the plan)
        n_el = int(np.prod(rec["shape"]))
        ref = np.unpackbits(g["%s_stage%s_bits" % (key, rec["name"])])[:n_el].reshape(rec["shape"]).astype(bool)
        got = (by_stage[rec["name"]][:, :rec["shape"][1]] > 0).cpu().numpy()
        diff = got != ref
        print(key, "stage", rec["name"], "mismatches", int(diff.sum()), "of", n_el)
        total += int(diff.sum())
        assert diff.sum() <= 1e-4 * n_el, (rec["name"], int(diff.sum()))
        if not rec["pooled"]:
            tie = np.unpackbits(g["%s_stage%s_tie" % (key, rec["name"])])[:n_el].reshape(rec["shape"]).astype(bool)
            assert not (diff & ~tie).any(), rec["name"]
    ref_lg = g[key + "_logits"]
    rel = float(np.abs(lg.cpu().numpy().astype(np.float64) - ref_lg).max() / np.abs(ref_lg).max())
    print(key, "hidden sign mismatches", total, "logits rel", rel)
    if total == 0:
        assert rel <= 1e-5, rel


@pytest.mark.parametrize("W", [3, 2])
def test_compiled_plan_batch_256_equals_its_chunks(W):
    """Batch 256, the batch behind the measured numbers: a block of every hidden kernel takes several units (tests/deploy_grid.py).  Logits and every kept stage equal
    those of the same images in eight chunks of 32, the launch shape the tests above hold to the judge."""
    import deploy_grid as DG
    from micronet_amd import inference
    F, _ = _nin_folded(W)
    DG.plan_whole_against_chunks(inference.wbwtab_compile_bits(F), "stage_bits")
