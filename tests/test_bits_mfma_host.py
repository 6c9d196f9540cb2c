"""Host-only behaviour of ``wbwtab_bits_report(model, mfma_blocks=..., mfma_k3=...)`` / the walk of ``wbwtab_compile_bits`` with the two keywords: which blocks take
the int8-MFMA forms (csrc/qgemm_bits_mfma.h, csrc/qgemm_bits_mfma3.h), that nothing else moves, and that the keywords are off by default -- without a GPU."""
import inspect
import json
import os

import torch.nn as nn

from conftest import GOLDEN
from test_bits_nin_host import _folded, _nin

NAMES = {"name", "kind", "K", "words", "kernel", "pooled", "out_order", "stage"}
K3 = "k_bitconv_mfma3<0>"
NIN_KERNELS = ["k_bitconv<1,0,0>", "k_bitconv1_pool3<8>", "k_bitconv_tile<5,3>", "k_bitconv<1,0,0>", "k_bitconv1_pool3<8>", "k_bitconv<3,0,0>", "k_bitconv<1,0,0>"]


def _golden(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def _gc():
    from micronet_amd.models import nin_gc
    return _folded(nin_gc.Net())


def test_keywords_default_to_off_and_go_last():
    from micronet_amd import inference
    for fn in (inference.wbwtab_compile_bits, inference.wbwtab_bits_report, inference._walk_bits):
        p = inspect.signature(fn).parameters
        assert list(p)[-3:] == ["bit_ends", "mfma_blocks", "mfma_k3"] and p["mfma_blocks"].default is False and p["mfma_k3"].default is False


def test_keywords_off_change_nothing():
    from micronet_amd import inference
    assert inference.wbwtab_bits_report(_gc()) == _golden("bits_report_nin_gc.json")
    assert inference.wbwtab_bits_report(_gc(), False, False, False) == _golden("bits_report_nin_gc.json")
    assert [r["kernel"] for r in inference.wbwtab_bits_report(_folded(_nin()), mfma_blocks=False, mfma_k3=False)[1:8]] == NIN_KERNELS
    for layers in (inference._walk_bits(_gc())[1], inference._walk_bits(_gc(), True)[1], inference._walk_bits(_folded(_nin()))[1]):
        assert not any("mfma" in L or "mfma3" in L for L in layers), "the layer dicts gain the keys under their flag only"
    assert all("mfma" in L and "mfma3" not in L for L in inference._walk_bits(_gc(), False, True)[1])
    assert all("mfma3" in L and "mfma" not in L for L in inference._walk_bits(_gc(), False, False, True)[1])


def test_bits_mfma_report_nin_gc_is_pinned():
    from micronet_amd import inference
    base = _golden("bits_report_nin_gc.json")
    rep = inference.wbwtab_bits_report(_gc(), mfma_blocks=True, mfma_k3=True)
    assert rep == _golden("bits_mfma_report_nin_gc.json")
    assert all(set(r) == NAMES for r in rep) and len(base) == len(rep)
    moved = [(a, b) for a, b in zip(base, rep) if a != b]
    assert len(moved) == 7
    for a, b in moved:
        assert a["kind"] == "bit" and {k for k in a if a[k] != b[k]} == {"kernel"}, "a moved row changes in its kernel only"
    assert [(a["K"], a["kernel"], b["kernel"]) for a, b in moved if a["K"] == 16 * 9] == [(144, "k_bitconv<3,1,0>", K3)] * 2, "the two K = 144 rows"
    ones = [(a, b) for a, b in moved if a["K"] != 16 * 9]
    assert len(ones) == 5 and all(a["kernel"].startswith("k_bitconv<1,4,") and b["kernel"] == "k_bitconv_mfma<%d>" % bool(a["pooled"]) for a, b in ones), "the five 1x1 rows"
    assert sum(bool(a["pooled"]) for a, _ in ones) == 2
    layers = inference._walk_bits(_gc(), False, True, True)[1]
    assert [L["mfma"] for L in layers] == [L["k"] == 1 for L in layers] and [L["mfma3"] for L in layers] == [L["k"] == 3 for L in layers]


def test_each_keyword_alone_and_with_bit_ends():
    from micronet_amd import inference
    for bit_ends in (False, True):
        base = inference.wbwtab_bits_report(_gc(), bit_ends=bit_ends)
        both = inference.wbwtab_bits_report(_gc(), bit_ends=bit_ends, mfma_blocks=True, mfma_k3=True)
        one = inference.wbwtab_bits_report(_gc(), bit_ends=bit_ends, mfma_blocks=True)
        k3 = inference.wbwtab_bits_report(_gc(), bit_ends=bit_ends, mfma_k3=True)
        assert [r for a, r in zip(base, one) if a != r] == [r for r in both if r["kernel"].startswith("k_bitconv_mfma<")]
        assert [r for a, r in zip(base, k3) if a != r] == [r for r in both if r["kernel"] == K3]
        assert [r["kernel"] for r in one].count(K3) == 0 and not [r for r in k3 if r["kernel"].startswith("k_bitconv_mfma<")]
        assert (base[0], base[-1]) == (both[0], both[-1]), "the ends are bit_ends' alone"


def test_plain_nin_the_dense_3x3_and_the_unpooled_1x1_rows_move():
    from micronet_amd import inference
    base = inference.wbwtab_bits_report(_folded(_nin()))
    rep = inference.wbwtab_bits_report(_folded(_nin()), mfma_blocks=True, mfma_k3=True)
    assert rep == _golden("bits_mfma_report_nin.json")
    assert [r["kernel"] for r in rep[1:8]] == ["k_bitconv_mfma<0>", "k_bitconv1_pool3<8>", "k_bitconv_tile<5,3>", "k_bitconv_mfma<0>", "k_bitconv1_pool3<8>", K3,
                                               "k_bitconv_mfma<0>"]
    for a, b in zip(base, rep):
        assert b == dict(a, kernel=b["kernel"])
        if a["pooled"] == "folded 3x3/2" or a["K"] == 2400:
            assert a == b, "the 5x5 row and the folded 3x3 / 2 rows do not move"
    layers = inference._walk_bits(_folded(_nin()), False, True, True)[1]
    assert [L["name"] for L in layers if L["mfma3"]] == ["model.8"] and [L["name"] for L in layers if L["mfma"]] == ["model.1", "model.5", "model.9"]
    assert [L["mfma"] for L in layers if L["pool"] == 2] == [False, False]


def test_a_pooled_3x3_and_a_thin_1x1_block_keep_their_kernels():
    """The 2x2 pool is folded into the 3x3 block in front of it and mn_bitconv_mfma3_fwd has no pooled form; a 1x1 block of 16 channels per group is not covered by
    mn_bitconv_mfma_supported.  Both keep k_bitconv; nothing is raised.  A 3x3 block whose pool runs as mn_bits_maxpool behind it still moves."""
    from micronet_amd import inference
    net = _nin([32, 32, 32, 64, 64, 64, 64, 64])
    seq = list(net.model)
    seq[9].conv = nn.Conv2d(64, 64, 1, groups=4)          # model.9: 16 channels per group
    seq.insert(9, nn.MaxPool2d(2, 2))                     # behind model.8 (the 3x3 block): folded
    net.model = nn.Sequential(*seq)
    base = inference.wbwtab_bits_report(_folded(net))
    flags = dict(mfma_blocks=True, mfma_k3=True)
    net2 = _nin([32, 32, 32, 64, 64, 64, 64, 64])
    seq = list(net2.model)
    seq[9].conv = nn.Conv2d(64, 64, 1, groups=4)
    seq.insert(9, nn.MaxPool2d(2, 2))
    net2.model = nn.Sequential(*seq)
    rep = inference.wbwtab_bits_report(_folded(net2), **flags)
    k3 = [(a, b) for a, b in zip(base, rep) if a["K"] == 64 * 9]
    thin = [(a, b) for a, b in zip(base, rep) if a["K"] == 16]
    assert len(k3) == 1 and k3[0][0] == k3[0][1] and k3[0][0]["kernel"] == "k_bitconv<3,0,1>" and k3[0][0]["pooled"] is True
    assert len(thin) == 1 and thin[0][0] == thin[0][1] and thin[0][0]["kernel"].startswith("k_bitconv<1,")
    # the same block with a 3x3 / 2 pool behind it: the pool is not folded (mn_bits_maxpool), the block runs un-pooled into the mid buffer -- on the MFMA form
    net3 = _nin([32, 32, 32, 64, 64, 64, 64, 64])
    seq = list(net3.model)
    seq.insert(9, nn.MaxPool2d(3, 2, 1))
    net3.model = nn.Sequential(*seq)
    row = [r for r in inference.wbwtab_bits_report(_folded(net3), **flags) if r["K"] == 64 * 9][0]
    assert row["kernel"] == K3 + ", k_bits_maxpool" and row["pooled"] == "standalone"


def test_mfma_entry_points_are_declared_and_bound():
    from micronet_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "micronet_hip.h")).read()
    for q in ("mn_bitconv_mfma", "mn_bitconv_mfma3"):
        for name in (q + "_supported", q + "_table_bytes", q + "_pack", q + "_fwd"):
            assert name in _lib.PROTOTYPES and (name + "(") in header and hasattr(_lib.get_lib(), name)
