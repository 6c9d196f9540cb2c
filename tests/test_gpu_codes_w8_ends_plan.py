"""``dorefa_compile_bytes(I, byte_ends=True)`` on the MI355X against the default plan compiled from the same model: the fixture of tests/test_gpu_codes_w8_plan.py (W8A8
nin_gc and the narrow cfg after two training steps, six images; imported, not copied).  Every stage's bytes equal the default plan's, the logits are held to an fp64 evaluation of the last
block and the tail on the plan's own last stage, batch 6 equals its two chunks; a classifier whose stored weights are off the grid is refused by name."""
import numpy as np
import pytest
import torch

import deploy_grid as DG
from test_gpu_codes_w8_plan import net          # noqa: F401 -- that file's fixture: (I, its default plan with the stages of the six images kept, the images, the logits, ...)

pytestmark = pytest.mark.gpu


def _run(plan, x):          # (logits, kept stages) of one forward
    with torch.no_grad():
        y = plan(x).clone()
    return y, [s.clone() for s in plan.stage_codes]


@pytest.fixture(scope="module")
def ends(net):
    """(I, the default plan, the byte_ends plan, six images, the default plan's (logits, stages), the byte_ends plan's)."""
    from micronet_amd import inference
    I, P0, x, y0, _ = net
    s0 = [s.clone() for s in P0.stage_codes]
    P1 = inference.dorefa_compile_bytes(I, byte_ends=True)
    assert P1.report == inference.dorefa_bytes_report(I, byte_ends=True) and P0.report == inference.dorefa_bytes_report(I) and P1.report[1:-1] == P0.report[1:-1]
    P1.keep_stages = True
    return I, P0, P1, x, (y0, s0), _run(P1, x)


def test_every_stage_equals_the_default_plans(ends):
    _, P0, _, _, (_, s0), (_, s1) = ends
    for i, (b1, b0) in enumerate(zip(s1, s0, strict=True)):
        assert torch.equal(b1, b0), (P0.report[i]["name"], int((b1 != b0).sum()), b0.numel())


def _fp64_logits(plan, stage):
    """The last block and the tail on a kept last stage, in double on the host: exact integer conv, alpha = 1 / 255^2 and bias, eval BatchNorm, ReLU, the tail."""
    from micronet_amd import inference
    conv, bn = plan.last.conv, plan.last.bn
    side = int(round(stage.shape[2] ** 0.5))
    codes = inference.unpack_code_map(stage, conv.in_channels, side, side).cpu().numpy().astype(np.int64)
    k = torch.round((conv.weight.detach() * 255 + 255) / 2).cpu().numpy().astype(np.int64)
    acc = DG.exact_conv(codes, 2 * k - 255, 0, 1)
    assert np.abs(acc).max() < 2 ** 31
    d = lambda t: t.detach().double().cpu().view(1, -1, 1, 1)
    y = torch.from_numpy(acc.astype(np.float64)) / (255.0 * 255.0) + (d(conv.bias) if conv.bias is not None else 0.0)
    z = torch.relu((y - d(bn.running_mean)) / torch.sqrt(d(bn.running_var) + bn.eps) * d(bn.weight) + d(bn.bias))
    for m in plan.tail:
        z = m(z)
    return z.reshape(z.shape[0], -1), int(np.abs(acc).max())


def test_logits_against_fp64_on_the_plans_own_last_stage(ends):
    """Within the float contract of DESIGN.md 7: 1e-5 max|ref|.  The default plan's distance (fp32 accumulation of sums beyond 2^24) is printed beside it, not asserted."""
    _, _, P1, _, (y0, _), (y1, s1) = ends
    ref, amax = _fp64_logits(P1, s1[-1])
    e1, e0 = (float((y.double().cpu() - ref).abs().max()) for y in (y1, y0))
    print("max |acc| %d, max|ref| %.6g: byte_ends %.3g, default plan %.3g (bound %.3g)" % (amax, float(ref.abs().max()), e1, e0, 1e-5 * float(ref.abs().max())))
    assert y1.shape == ref.shape == (6, 10) and e1 <= 1e-5 * float(ref.abs().max())


def test_batch_6_equals_its_two_chunks(ends):
    _, _, P1, x, _, (y1, s1) = ends
    parts = [_run(P1, x[a:a + 3].contiguous()) for a in (0, 3)]
    assert torch.equal(torch.cat([p[0] for p in parts]), y1)
    assert all(torch.equal(torch.cat([parts[0][1][i], parts[1][1][i]]), s) for i, s in enumerate(s1))


def test_a_classifier_off_the_grid_is_refused_by_name(ends):
    """Hidden convs on the 8-bit grid, the classifier's stored weights half a step off it: ``byte_ends`` names the classifier (the default plan never reads them as codes)."""
    from micronet_amd import _lib, inference
    I, P0 = ends[:2]
    conv, on_grid = P0.last.conv, P0.last.conv.weight.data
    conv.weight.data = on_grid + 1.0 / 255
    try:
        with pytest.raises(_lib.MicronetHipError, match=r"%s\.conv: the stored weights were not found on the 8-bit grid" % P0.report[-1]["name"].replace(".", r"\.")):
            inference.dorefa_compile_bytes(I, byte_ends=True)
    finally:
        conv.weight.data = on_grid
