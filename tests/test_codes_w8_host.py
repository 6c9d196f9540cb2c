"""Host-only behaviour of ``dorefa_bytes_report`` / the walk of ``dorefa_compile_bytes``: the stage report of W8A8 nin_gc and the named refusals -- without a GPU."""
import json
import os

import pytest

from conftest import GOLDEN
from test_codes_host import _prepared


def _refused(model, pattern, fn="dorefa_bytes_report"):
    from micronet_amd import inference
    from micronet_amd._lib import MicronetHipError
    with pytest.raises(MicronetHipError, match=pattern):
        getattr(inference, fn)(model)


def test_bytes_report_nin_gc():
    from micronet_amd import inference
    rep = inference.dorefa_bytes_report(_prepared(bits=8))
    assert [r["kind"] for r in rep] == ["first"] + ["byte"] * 7 + ["last"]
    assert [r["kernel"] for r in rep[1:-1]] == ["k_code8conv<%d,%d>" % kp for kp in ((1, 0), (1, 1), (3, 0), (1, 0), (1, 1), (3, 0), (1, 0))]
    assert [r["blocks"] for r in rep] == [0, 16, 16, 16, 32, 32, 32, 64, 64]
    # names, K, pools, channel orders and stages are those of the 4-bit code plan of the same net
    four = json.load(open(os.path.join(GOLDEN, "codes_w4a4_report_nin_gc.json")))
    assert all(r[key] == f[key] for r, f in zip(rep, four) for key in ("name", "K", "pooled", "out_order", "stage"))


def test_refusals_name_the_layer_and_the_rule():
    _refused(_prepared(bits=2), r"model\.1\.conv has a_bits = 2, w_bits = 2; only W8A8 nets are deployed on bytes")
    m = _prepared(bits=8)
    m.model[4].conv.quant_inference = False
    _refused(m, r"model\.4\.conv is not a quant_inference=True layer")
    _refused(_prepared("nin", bits=8), r"model\.4\.conv: geometry not covered by mn_code8conv_supported \(5x5, padding 2, groups 1, 96 channels per group: needs 1x1")
    _refused(_prepared(bits=8), r"model\.1\.conv: the stored weights were not found on the 8-bit grid \(2k - 255\) / 255", "dorefa_compile_bytes")          # never pre-quantised
    # dorefa_compile_codes is as it was: it refuses the same W8A8 net by name
    _refused(_prepared(bits=8), r"model\.1\.conv has a_bits = 8, w_bits = 8; only W2A2 and W4A4 nets", "dorefa_compile_codes")
