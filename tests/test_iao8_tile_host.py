"""Host-only behaviour of ``iao_int8_report(model, tile_blocks=True)`` / the walk of ``iao_compile_int8(model, tile_blocks=True)`` on a narrow BN-folded IAO plain
nin: the stage report with the 5x5 tile block and the two un-folded max-pools, and the refusals -- without a GPU."""
import pytest
import torch

CFG = [32, 32, 16, 32, 32, 32, 32, 32]


def _folded(cfg=CFG):
    from micronet.compression.quantization.wqaq.iao import quantize as Q
    from micronet_amd import inference
    from micronet_amd.models import nin
    torch.manual_seed(0)
    T = Q.prepare(nin.Net(cfg=cfg), inplace=True, a_bits=8, w_bits=8, q_type=0, q_level=0, weight_observer=0, bn_fuse=True)
    return inference.iao_model_bn_fuse(T).eval()


def test_report_lists_the_tile_block_and_the_pools():
    from micronet_amd import inference
    Fm = _folded()
    for ends in (False, True):
        rep = inference.iao_int8_report(Fm, byte_ends=ends, tile_blocks=True)
        assert [r["name"] for r in rep] == ["model.%d" % i for i in range(11)]
        assert [r["kind"] for r in rep[1:-1]] == ["int8", "int8", "int8_pool", "int8", "int8", "int8", "int8_pool", "int8", "int8"]
        assert [r["kernel"] for r in rep[1:-1]] == ["k_i8conv<1,0>", "k_i8conv<1,0>", "k_i8_maxpool", "k_i8conv5<5>", "k_i8conv<1,0>", "k_i8conv<1,0>", "k_i8_maxpool",
                                                    "k_i8conv<3,0>", "k_i8conv<1,0>"]
        assert (rep[0]["kind"], rep[-1]["kind"]) == (("int8_first", "int8_last") if ends else ("first", "last"))
        # one byte per hidden activation: 32 x 32 up to model.3, 16 x 16 up to model.7, then 8 x 8
        assert [(r["act_bytes_in"], r["act_bytes_out"]) for r in (rep[3], rep[7])] == [(16 * 1024, 16 * 256), (32 * 256, 32 * 64)]
        assert (rep[4]["act_bytes_in"], rep[4]["act_bytes_out"], rep[8]["act_bytes_in"]) == (16 * 256, 32 * 256, 32 * 64)
        assert all(r["pool"] == 0 for r in rep) and rep[4]["table_bytes"] > 4 * 25 * 16 * 32 // 4
    layers = inference._walk_iao8(Fm, tile_blocks=True)[1]
    assert [(L["tile"], L["pool_ksp"]) for L in layers] == [(False, None), (False, (3, 2, 1)), (True, None), (False, None), (False, (3, 2, 1)), (False, None), (False, None)]


def _raises(match, model, **kw):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    for entry in (inference.iao_int8_report, inference.iao_compile_int8):          # the same walk, before anything touches a GPU
        with pytest.raises(MicronetHipError, match=match):
            entry(model, **kw)


def test_refusals_with_and_without_the_keyword():
    from micronet_amd.models import resnet
    Fm = _folded()
    _raises(r"model\.3 \(QuantMaxPool2d, kernel 3, stride 2, padding 1\): only a 2x2 / stride 2 QuantMaxPool2d is folded", Fm)
    _raises(r"tile_blocks=True\): zero_points=True is not covered together with tile_blocks", Fm, tile_blocks=True, zero_points=True)
    _raises(r"tile_blocks=True\): end_to_end=True is not covered together with tile_blocks", Fm, tile_blocks=True, end_to_end=True)
    _raises(r"tile_blocks=True\): the reference ResNet tree", resnet.resnet18(), tile_blocks=True)
    _raises(r"model\.4\.conv: geometry not covered by mn_i8conv5_supported \(5x5, stride 1, padding 2, dilation 1, groups 1, 24 channels: dense 5x5",
            _folded([32, 32, 24, 32, 32, 32, 32, 32]), tile_blocks=True)
    wide = _folded()
    with pytest.raises(Exception, match=r"model\.4\.conv: a 16-channel map 512 pixels wide is beyond the LDS bound of mn_i8conv5_supported"):
        from micronet_amd import inference
        inference.iao_int8_report(wide, input_hw=(8, 1024), tile_blocks=True)
