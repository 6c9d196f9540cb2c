"""Host-only behaviour of ``dorefa_codes_report(model, mfma_k3=True)`` / the walk of ``dorefa_compile_codes(model, mfma_k3=True)``: which blocks take the 3x3 MFMA
form, that nothing else moves, and that the keyword is off by default -- without a GPU."""
import inspect
import json
import os

import torch.nn as nn

from conftest import GOLDEN
from test_codes_host import _prepared

NAMES = {"name", "kind", "K", "words", "planes", "kernel", "pooled", "out_order", "stage"}
K3 = "k_codeconv_mfma3<0>"


def _golden(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def test_keyword_defaults_to_off_and_goes_last():
    from micronet_amd import inference
    for fn in (inference.dorefa_compile_codes, inference.dorefa_codes_report, inference._walk_codes):
        p = inspect.signature(fn).parameters
        assert p["mfma_k3"].default is False and list(p)[-1] == "mfma_k3"


def test_keyword_off_changes_nothing():
    from micronet_amd import inference
    assert inference.dorefa_codes_report(_prepared()) == _golden("codes_report_nin_gc.json")
    assert inference.dorefa_codes_report(_prepared(), mfma_k3=False) == _golden("codes_report_nin_gc.json")
    assert inference.dorefa_codes_report(_prepared(), mfma_blocks=True) == _golden("codes_mfma_report_nin_gc.json")
    assert inference.dorefa_codes_report(_prepared("nin"), tile_blocks=True) == _golden("codes_report_nin.json")
    for layers in (inference._walk_codes(_prepared())[1], inference._walk_codes(_prepared(), False, False, True)[1], inference._walk_codes(_prepared("nin"), False, True)[1]):
        assert not any("mfma3" in L for L in layers), "the layer dict gains the key under the flag only"


def test_codes_mfma3_report_nin_gc_is_pinned():
    from micronet_amd import inference
    base = _golden("codes_mfma_report_nin_gc.json")
    rep = inference.dorefa_codes_report(_prepared(), mfma_blocks=True, mfma_k3=True)
    assert rep == _golden("codes_mfma3_report_nin_gc.json")
    assert all(set(r) == NAMES for r in rep)
    moved = [(a, b) for a, b in zip(base, rep) if a != b]
    assert len(moved) == 2 and len(base) == len(rep)
    for a, b in moved:
        assert a["K"] == 16 * 9 and a["kernel"] == "k_codeconv<3,1,0>" and b == dict(a, kernel=K3), "exactly the two K = 144 rows change, and only in their kernel"
    hidden = [r["kernel"] for r in rep[1:-1]]
    assert len(hidden) == 7 and all(k.startswith(("k_codeconv_mfma<", "k_codeconv_mfma3<")) for k in hidden), hidden
    layers = inference._walk_codes(_prepared(), False, False, True, True)[1]
    assert [L["mfma3"] for L in layers] == [L["k"] == 3 for L in layers] and sum(L["mfma3"] for L in layers) == 2
    assert not any(L["mfma"] and L["mfma3"] for L in layers)


def test_the_keyword_alone_and_with_code_ends():
    """Without mfma_blocks the 1x1 rows keep k_codeconv; code_ends changes the two ends only."""
    from micronet_amd import inference
    for code_ends in (False, True):
        base = inference.dorefa_codes_report(_prepared(), code_ends=code_ends)
        rep = inference.dorefa_codes_report(_prepared(), code_ends=code_ends, mfma_k3=True)
        assert [b for a, b in zip(base, rep) if a != b] == [dict(a, kernel=K3) for a in base if a["K"] == 16 * 9]
        assert [r["kernel"] for r in rep].count(K3) == 2


def test_plain_nin_only_the_3x3_row_changes():
    from micronet_amd import inference
    base = inference.dorefa_codes_report(_prepared("nin"), tile_blocks=True, mfma_blocks=True)
    rep = inference.dorefa_codes_report(_prepared("nin"), tile_blocks=True, mfma_blocks=True, mfma_k3=True)
    moved = [(a, b) for a, b in zip(base, rep) if a != b]
    assert len(moved) == 1
    a, b = moved[0]
    assert a["K"] == 192 * 9 and a["kernel"].startswith("k_codeconv<3,0,0>") and b == dict(a, kernel=a["kernel"].replace("k_codeconv<3,0,0>", K3))
    layers = inference._walk_codes(_prepared("nin"), False, True, True, True)[1]
    assert [L["name"] for L in layers if L["mfma3"]] == [a["name"]] and [L["name"] for L in layers if L["tile"]] == ["model.4"], "the 5x5 keeps the tile kernel"


def test_a_pooled_3x3_block_keeps_the_popcount_kernel():
    """The 2x2 pool is folded into the 3x3 block in front of it: mn_codeconv_mfma3_fwd has no pooled form, so the block stays on k_codeconv<3,*,1>; nothing is raised."""
    from micronet_amd import inference
    from micronet_amd.models.nin_gc import ConvBNReLU

    def net():
        return nn.Sequential(ConvBNReLU(3, 32, 5, padding=2), ConvBNReLU(32, 32, 3, padding=1), nn.MaxPool2d(2, 2), ConvBNReLU(32, 64, 3, padding=1),
                             ConvBNReLU(64, 10, 1))
    base = inference.dorefa_codes_report(_prepared(net=net()))
    rep = inference.dorefa_codes_report(_prepared(net=net()), mfma_k3=True)
    layers = inference._walk_codes(_prepared(net=net()), False, False, False, True)[1]
    assert [(L["k"], L["pool"], L["mfma3"]) for L in layers] == [(3, 1, False), (3, 0, True)]
    assert rep[1] == base[1] and base[1]["kernel"] == "k_codeconv<3,1,1>" and base[1]["pooled"] is True
    assert rep[2] == dict(base[2], kernel=K3) and rep[0] == base[0] and rep[3] == base[3]


def test_eight_channels_per_group_stay_on_the_popcount_kernel():
    from micronet_amd import inference
    from micronet_amd.models import nin_gc
    cfg = [128, 128, 128, 256, 256, 256, 512, 512]          # 128 / 16 and 256 / 32: 8 channels per group in both 3x3 blocks
    base = inference.dorefa_codes_report(_prepared(net=nin_gc.Net(cfg=cfg)))
    rep = inference.dorefa_codes_report(_prepared(net=nin_gc.Net(cfg=cfg)), mfma_k3=True)
    layers = inference._walk_codes(_prepared(net=nin_gc.Net(cfg=cfg)), False, False, False, True)[1]
    assert rep == base and not any(L["mfma3"] for L in layers)
    assert [L["cin"] // L["groups"] for L in layers if L["k"] == 3] == [8, 8]


def test_mfma3_entry_points_are_declared_and_bound():
    from micronet_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "micronet_hip.h")).read()
    for name in ("mn_codeconv_mfma3_supported", "mn_codeconv_mfma3_table_bytes", "mn_codeconv_mfma3_pack", "mn_codeconv_mfma3_fwd"):
        assert name in _lib.PROTOTYPES and (name + "(") in header
