"""Host-only behaviour of ``dorefa_codes_report(model, mfma_blocks=True)`` / the walk of ``dorefa_compile_codes(model, mfma_blocks=True)``: which blocks take the MFMA
form, that nothing else moves, and that the keyword is off by default -- without a GPU."""
import inspect
import json
import os

import pytest

from conftest import GOLDEN
from test_codes_host import _prepared

NAMES = {"name", "kind", "K", "words", "planes", "kernel", "pooled", "out_order", "stage"}


def _golden(name):
    return json.load(open(os.path.join(GOLDEN, name)))


@pytest.mark.parametrize("code_ends", [False, True])
def test_codes_mfma_report_nin_gc_is_pinned(code_ends):
    from micronet_amd import inference
    rep = inference.dorefa_codes_report(_prepared(), code_ends=code_ends, mfma_blocks=True)
    base = _golden("codes_ends_report_nin_gc.json" if code_ends else "codes_report_nin_gc.json")
    want = _golden("codes_mfma_report_nin_gc.json")
    assert rep == (want if not code_ends else [base[0]] + want[1:-1] + [base[-1]]), "the hidden rows do not depend on code_ends"
    assert rep[0] == base[0] and rep[-1] == base[-1], "both ends are unchanged"
    assert all(set(r) == NAMES for r in rep)
    moved = [(a, b) for a, b in zip(base, rep) if a != b]
    assert len(moved) == 5
    for a, b in moved:
        assert a["kernel"].startswith("k_codeconv<1,") and b["kernel"] == "k_codeconv_mfma<%d>" % int(bool(a["pooled"]))
        assert {k: v for k, v in a.items() if k != "kernel"} == {k: v for k, v in b.items() if k != "kernel"}, "only the kernel of a row changes"
    assert [r["kernel"] for r in rep].count("k_codeconv_mfma<0>") == 3 and [r["kernel"] for r in rep].count("k_codeconv_mfma<1>") == 2
    assert [r["kernel"] for r in rep if r["K"] == 16 * 9] == ["k_codeconv<3,1,0>"] * 2, "the two 3x3 rows keep their kernel"


@pytest.mark.parametrize("code_ends", [False, True])
def test_keyword_off_changes_nothing(code_ends):
    from micronet_amd import inference
    want = _golden("codes_ends_report_nin_gc.json" if code_ends else "codes_report_nin_gc.json")
    assert inference.dorefa_codes_report(_prepared(), code_ends=code_ends) == want
    assert inference.dorefa_codes_report(_prepared(), code_ends=code_ends, mfma_blocks=False) == want
    layers = inference._walk_codes(_prepared(), code_ends)[1]
    assert not any("mfma" in L for L in layers), "the layer dict gains the key under the flag only"


def test_keyword_defaults_to_off():
    from micronet_amd import inference
    for fn in (inference.dorefa_compile_codes, inference.dorefa_codes_report):
        p = inspect.signature(fn).parameters
        assert p["mfma_blocks"].default is False and p["code_ends"].default is False and p["tile_blocks"].default is False


def test_walk_marks_the_covered_blocks():
    from micronet_amd import inference
    layers = inference._walk_codes(_prepared(), False, False, True)[1]
    assert [L["mfma"] for L in layers] == [L["k"] == 1 for L in layers] and sum(L["mfma"] for L in layers) == 5
    assert [L["pool"] for L in layers if L["mfma"]].count(1) == 2, "the folded 2x2 pool goes with the block"


def test_plain_nin_dense_blocks_are_all_covered():
    """tile_blocks and mfma_blocks compose: the 5x5 block stays on the tile kernel and the 3x3 block on k_codeconv, every dense 1x1 block moves, a standalone pool
    stays behind its block."""
    from micronet_amd import inference
    base = inference.dorefa_codes_report(_prepared("nin"), tile_blocks=True)
    assert base == _golden("codes_report_nin.json")
    rep = inference.dorefa_codes_report(_prepared("nin"), tile_blocks=True, mfma_blocks=True)
    for a, b in zip(base, rep):
        if a["kernel"].startswith("k_codeconv<1,"):          # the dense 1x1 blocks
            assert b == dict(a, kernel=a["kernel"].replace("k_codeconv<1,0,0>", "k_codeconv_mfma<0>")), (a, b)
            assert b["kernel"].startswith("k_codeconv_mfma<0>")
        else:
            assert a == b
    assert sum(r["kernel"].startswith("k_codeconv_mfma") for r in rep) == 5
    assert {r["name"]: r["kernel"] for r in rep}["model.2"] == "k_codeconv_mfma<0>, k_codes_maxpool"


def test_narrow_groups_stay_on_the_popcount_kernel():
    """16 channels per group: the grouped 1x1 blocks are not covered and keep k_codeconv while the flag is on; nothing is refused."""
    from micronet_amd import inference
    from micronet_amd.models import nin_gc
    cfg = [32, 32, 32, 64, 64, 64, 128, 128]
    base = inference.dorefa_codes_report(_prepared(net=nin_gc.Net(cfg=cfg)))
    rep = inference.dorefa_codes_report(_prepared(net=nin_gc.Net(cfg=cfg)), mfma_blocks=True)
    layers = inference._walk_codes(_prepared(net=nin_gc.Net(cfg=cfg)), False, False, True)[1]
    for a, b, L in zip(base[1:-1], rep[1:-1], layers):
        covered = L["k"] == 1 and (L["groups"] == 1 or (L["cin"] // L["groups"]) % 32 == 0)
        assert L["mfma"] == covered
        assert b == (dict(a, kernel="k_codeconv_mfma<%d>" % L["pool"]) if covered else a)
    assert any(L["k"] == 1 and not L["mfma"] for L in layers), "the case must hold a narrow grouped 1x1 block"


def test_mfma_entry_points_are_declared_and_bound():
    from micronet_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "micronet_hip.h")).read()
    for name in ("mn_codeconv_mfma_supported", "mn_codeconv_mfma_table_bytes", "mn_codeconv_mfma_pack", "mn_codeconv_mfma_fwd"):
        assert name in _lib.PROTOTYPES and (name + "(") in header
