"""Cases of the sparse-training Adam step (mn_adam_step_l1) shared by the CPU-emulation run (test_prune_emulated.py) and the MI355X run (test_gpu_prune.py),
and the seeded models the pruning tests start from.

Reference of the kernel: ``torch.optim.Adam`` on CPU with an explicit ``grad.add_(s * torch.sign(p))`` in front of ``step()`` -- the reference's updateBN()
(pruning/main.py:65-69).  Tolerance: the one of kernel_cases.check_adam for this kernel, 2e-6 * max(1, max|ref|)."""
import ctypes as C

import numpy as np

F = np.float32

SIZES = (1, 3, 5, 2048, 2049, 4099)             # scalar tail only, an exact chunk, a chunk plus one, an unaligned tail behind two chunks
L1S = (1e-3, 0.0, 1e-4, 0.0, 1e-3, 1e-4)
WDS = (1e-5, 1e-5, 0.0, 0.0, 2e-5, 0.0)         # weight decay on some tensors of each kind (s != 0 / s == 0)


def seeded_params(r, n):
    """standard-normal values of both signs with exact +0 and -0 planted (sign(+-0) = 0: no L1 term there)"""
    p = r.standard_normal(n).astype(F)
    p[0] = F(-0.0) if n == 1 else F(0.0)
    if n >= 3:
        p[1], p[2] = F(-0.0), F(-1.5)
    if n >= 2049:
        p[2047], p[2048] = F(-0.0), F(0.0)      # ... and on both sides of a chunk boundary
    return p


def _table(be, dp, dg, dm, dv, sizes, lrs, wds):
    from micronet_amd import _lib
    arr = (_lib.AdamTensor * len(sizes))()
    for i, n in enumerate(sizes):
        arr[i] = _lib.AdamTensor(be.ptr(dp[i]).value, be.ptr(dg[i]).value, be.ptr(dm[i]).value, be.ptr(dv[i]).value, n, lrs[i], wds[i])
    return arr


def check_adam_l1(be, sizes=SIZES, l1s=L1S, wds=WDS, steps=3, lr=0.01, seed=0):
    """mn_adam_step_l1 vs torch.optim.Adam (CPU, fp32) + grad.add_(s * sign(p)) on the same parameters / gradients for a few steps."""
    import torch
    r = np.random.default_rng(seed)
    ps = [seeded_params(r, n) for n in sizes]
    assert any(np.signbit(p[p == 0]).any() for p in ps) and any((~np.signbit(p[p == 0])).any() for p in ps)       # -0 and +0 are in
    lrs = [lr * (1 + i % 7) for i in range(len(sizes))]
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = torch.optim.Adam([{"params": [t], "lr": lrs[i], "weight_decay": wds[i]} for i, t in enumerate(tp)], lr=lr)
    dp = [be.to_dev(p) for p in ps]
    dm = [be.to_dev(np.zeros_like(p)) for p in ps]
    dv = [be.to_dev(np.zeros_like(p)) for p in ps]
    l1 = (C.c_float * len(sizes))(*l1s)
    for step in range(1, steps + 1):
        gs = [(r.standard_normal(n) * 0.1).astype(F) for n in sizes]
        for t, g, s in zip(tp, gs, l1s):
            t.grad = torch.from_numpy(g.copy())
            if s:
                t.grad.add_(s * torch.sign(t.detach()))          # updateBN()
        opt.step()
        dg = [be.to_dev(g) for g in gs]
        be.call("mn_adam_step_l1", _table(be, dp, dg, dm, dv, sizes, lrs, wds), l1, len(sizes), step, 0.9, 0.999, 1e-8, be.stream)
        for i, t in enumerate(tp):
            for got, ref, what in ((be.to_host(dp[i]), t.detach().numpy(), "p"), (be.to_host(dm[i]), opt.state[t]["exp_avg"].numpy(), "m"),
                                   (be.to_host(dv[i]), opt.state[t]["exp_avg_sq"].numpy(), "v")):
                err = np.max(np.abs(got - ref))
                assert err <= 2e-6 * max(1.0, np.max(np.abs(ref))), (what, step, i, sizes[i], err)


def check_adam_l1_many(be):
    """41 tensors with alternating s: more than one launch table holds, so the second table reads its slots at hyper_base + slot_src"""
    sizes = tuple(range(1, 42))
    check_adam_l1(be, sizes=sizes, l1s=tuple(1e-3 if i % 2 == 0 else 0.0 for i in range(41)), wds=tuple(1e-5 * (i % 3) for i in range(41)), steps=2, seed=1)


def check_l1_zero_is_plain(be, sizes=SIZES, wds=WDS, steps=2, seed=2):
    """all-zero l1 through mn_adam_step_l1 == mn_adam_step, bit for bit (p, m, v)"""
    r = np.random.default_rng(seed)
    ps = [seeded_params(r, n) for n in sizes]
    lrs = [0.01 * (1 + i) for i in range(len(sizes))]
    runs = []
    for _ in range(2):
        runs.append(([be.to_dev(p) for p in ps], [be.to_dev(np.zeros_like(p)) for p in ps], [be.to_dev(np.zeros_like(p)) for p in ps]))
    l1 = (C.c_float * len(sizes))(*([0.0] * len(sizes)))
    for step in range(1, steps + 1):
        gs = [(r.standard_normal(n) * 0.1).astype(F) for n in sizes]
        for k, (dp, dm, dv) in enumerate(runs):
            dg = [be.to_dev(g) for g in gs]
            arr = _table(be, dp, dg, dm, dv, sizes, lrs, wds)
            if k == 0:
                be.call("mn_adam_step", arr, len(sizes), step, 0.9, 0.999, 1e-8, be.stream)
            else:
                be.call("mn_adam_step_l1", arr, l1, len(sizes), step, 0.9, 0.999, 1e-8, be.stream)
    for a, b in zip(runs[0], runs[1]):
        for x, y in zip(a, b):
            x, y = be.to_host(x), be.to_host(y)
            assert np.array_equal(x, y) and np.array_equal(np.signbit(x), np.signbit(y))
    assert not np.array_equal(be.to_host(runs[0][0][3]), ps[3])          # (the steps did move the parameters)


def check_l1_rejects_bad_arguments(be):
    from micronet_amd import _lib
    p, g, m, v = (be.to_dev(np.zeros(4, F)) for _ in range(4))
    arr = (_lib.AdamTensor * 1)(_lib.AdamTensor(be.ptr(p).value, be.ptr(g).value, be.ptr(m).value, be.ptr(v).value, 4, 0.01, 0.0))
    assert be.lib.mn_adam_step_l1(arr, None, 1, 1, 0.9, 0.999, 1e-8, be.stream) != 0
    assert be.lib.mn_adam_step_l1(arr, (C.c_float * 1)(-1e-3), 1, 1, 0.9, 0.999, 1e-8, be.stream) != 0
    assert be.lib.mn_adam_step_l1(arr, (C.c_float * 1)(float("nan")), 1, 1, 0.9, 0.999, 1e-8, be.stream) != 0
    assert be.lib.mn_adam_step_l1_dev(arr, (C.c_float * 1)(1e-3), 1, None, None, None, 0.9, 0.999, 1e-8, be.stream) != 0
    assert np.array_equal(be.to_host(p), np.zeros(4, F))


# ----------------------------------------------------------------------------- seeded models for the selection / compaction / QAT tests
NIN_CFG = [16, 16, 16, 32, 32, 32, 32, 32]
NIN_GC_CFG = [32, 32, 32, 64, 64, 64, 128, 128]


def seed_gammas(model, seed, strong=()):
    """pairwise-distinct seeded BatchNorm scales of both signs (a random permutation of an arithmetic grid, so distinctness does not hang on a draw), random shifts;
    the BatchNorms whose index is in ``strong`` get |gamma| + 1 (still pairwise distinct: (1, 2] against (0, 1]), so a global threshold leaves them whole"""
    import torch
    import torch.nn as nn
    bns = [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)]
    total = sum(m.weight.numel() for m in bns)
    g = torch.Generator().manual_seed(seed)
    vals = (torch.randperm(total, generator=g).float() + 1.0) / total          # (0, 1], all different
    vals = vals * (torch.randint(0, 2, (total,), generator=g).float() * 2 - 1)
    off = 0
    with torch.no_grad():
        for k, m in enumerate(bns):
            n = m.weight.numel()
            m.weight.copy_(vals[off:off + n])
            if k in strong:
                m.weight.add_(torch.sign(m.weight))
            m.bias.copy_(torch.randn(n, generator=g) * 0.1)
            off += n
    return model


def seeded_nin(seed=7, cfg=NIN_CFG):
    import torch
    from micronet_amd.models import nin
    from micronet_amd.train import init_like_main
    torch.manual_seed(seed)
    return seed_gammas(init_like_main(nin.Net(cfg=cfg)), seed)


def seeded_nin_gc(seed=8, cfg=NIN_GC_CFG, strong=()):
    import torch
    from micronet_amd.models import nin_gc
    from micronet_amd.train import init_like_main
    torch.manual_seed(seed)
    return seed_gammas(init_like_main(nin_gc.Net(cfg=cfg)), seed, strong)
