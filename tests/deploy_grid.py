"""What the "several units per block" cases of the deployment kernel tables share (the LARGE_GRID tables of tests/bits_nin_cases.py, bits_mfma_cases.py,
bits_mfma3_cases.py, codes_cases.py, codes_nin_cases.py, codes_mfma_cases.py, codes_mfma3_cases.py, codes_w4_cases.py, iao8_cases.py, iao8_ends_cases.py).

Every bit / code / byte forward sizes grid.y with one rule (csrc/qgemm_mfma_sets.h).  Where the pixel blocks alone fill the chip a block no longer owns one unit (an
output word, a set of 64 rows, a span) but loops over several, carrying state -- an LDS image, a clamp of the last block -- from one to the next.  Those cases are the
smallest shapes at which that loop runs at all, so each one PROVES that it does: it computes grid.x from the pixel-block rule include/micronet_hip.h documents for the
kernel and asks the library itself (mn_deploy_grid_deal / mn_deploy_grid_rows) how the units are dealt.  No copy of the rule or of its cap lives in the tests: if the
rule changes, the assertions here fail instead of the cases turning vacuous."""
import ctypes as C

import numpy as np


def pixel_blocks(total, per_block=256):
    """grid.x of a forward that gives every block ``per_block`` (pooled) output pixels of the whole batch."""
    return (total + per_block - 1) // per_block


def tile_blocks(N, H, W):
    """grid.x of the LDS-tiled kernels (k_bitconv_tile, k_codeconv_tile): 8- or 16-wide tiles, ceil(N / ipb) * tx * ty blocks of ipb = 256 / (tw * th) images."""
    tw, th = (8 if W <= 8 else 16), (8 if H <= 8 else 16)
    ipb = 256 // (tw * th)
    return ((N + ipb - 1) // ipb) * ((W + tw - 1) // tw) * ((H + th - 1) // th)


def assert_uneven_deal(be, bx, units):
    """The consecutive deal (grid_deal): a block takes at least two units, and the last block fewer than the others (its clamp is exercised).  Returns (grid.y, per)."""
    per = C.c_int(0)
    gy = int(be.lib.mn_deploy_grid_deal(int(bx), int(units), C.byref(per)))
    print("grid: bx", bx, "units", units, "grid.y", gy, "per", per.value)
    assert gy >= 2 and per.value >= 2, ("a block must take several units", bx, units, gy, per.value)
    assert units % per.value != 0, ("the last block must take fewer units than the others", bx, units, gy, per.value)
    return gy, per.value


def assert_uneven_rows(be, bx, units, nspans):
    """The round-robin deal (grid_rows) of the 3x3 MFMA forms: grid.y is sized for ``units`` = ceil(OW / 2), the kernel walks the table's own ``nspans``; some block
    takes a second span and some block does not.  Returns grid.y."""
    gy = int(be.lib.mn_deploy_grid_rows(int(bx), int(units)))
    print("grid: bx", bx, "units", units, "grid.y", gy, "spans", nspans)
    assert 1 <= gy < nspans and nspans % gy != 0, ("a block must take several spans, unevenly", bx, units, gy, nspans)
    return gy


def plan_whole_against_chunks(plan, stages_attr, batch=256, chunk=32):
    """A compiled plan on ``batch`` images (the batch behind the measured numbers: a 32 x 32 layer then has 1024 pixel blocks, and a block of every hidden kernel takes
    several units -- asserted through the library) against the same images in chunks of 32, the launch shape the stage-by-stage tests hold to the judges (128 pixel
    blocks: one unit per block): the logits and every stage the plan keeps must be equal bit for bit.  Returns the logits of the whole batch."""
    import torch
    from micronet_amd import _lib
    from micronet_amd.train import synth_batch
    lib, per = _lib.get_lib(), C.c_int(0)
    assert lib.mn_deploy_grid_deal(pixel_blocks(batch * 32 * 32), 4, C.byref(per)) >= 1 and per.value >= 2, "the whole batch: several units per block"
    assert lib.mn_deploy_grid_deal(pixel_blocks(chunk * 32 * 32), 16, C.byref(per)) == 16 and per.value == 1, "a chunk: one unit per block"
    x, _ = synth_batch(batch, device="cuda")
    assert len(torch.unique(x.flatten(1), dim=0)) == batch, "distinct images"

    def run(xx):
        plan.keep_stages = True
        with torch.no_grad():
            y = plan(xx).clone()
        plan.keep_stages = False
        return y, [s.clone() for s in getattr(plan, stages_attr)]

    y, stages = run(x)
    parts = [run(x[i:i + chunk].contiguous()) for i in range(0, batch, chunk)]
    assert len(stages) >= 2 and all(len(p[1]) == len(stages) for p in parts)
    for i, s in enumerate(stages):
        c = torch.cat([p[1][i] for p in parts])
        bad = int((s != c).sum()) if s.shape == c.shape else -1
        print("stage", i, tuple(s.shape), "elements unlike the chunks':", bad)
        assert s.shape == c.shape and torch.equal(s, c), ("stage", i, bad)
    yc = torch.cat([p[0] for p in parts])
    print("logits bit-equal to the chunks':", bool(torch.equal(y, yc)))
    assert y.shape == (batch, 10) and torch.equal(y, yc), float((y - yc).abs().max())
    return y


def exact_conv(x, k, padding, groups):
    """The integer accumulator of a convolution of integer arrays where oracle.np_oracle.conv2d_fwd(acc=np.int64) is too slow: torch's float64 conv2d on the CPU.  Every
    partial sum is an integer below 2^53 (asserted on the worst case sum |x| max |k|), so float64 is exact whatever the order of summation; the first image is held to
    np_oracle's int64 result."""
    import torch
    from oracle import np_oracle as O
    x, k = np.asarray(x, dtype=np.int64), np.asarray(k, dtype=np.int64)
    bound = int(np.abs(x).max()) * int(np.abs(k).max()) * int(np.prod(k.shape[1:]))
    assert bound < 2 ** 53, bound
    with torch.no_grad():
        acc = torch.nn.functional.conv2d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(k.astype(np.float64)), padding=padding, groups=groups).numpy()
    out = acc.astype(np.int64)
    assert np.array_equal(out, acc), "integers"
    assert np.array_equal(out[:1], O.conv2d_fwd(x[:1], k, None, padding=padding, groups=groups, acc=np.int64)), "np_oracle's int64 convolution on the first image"
    return out
