"""Bit-packed kernels the plain nin net needs (csrc/qgemm_bits.hip: the LDS-tiled dense 5x5, the 3x3 / stride 2 max-pool folded into a 1x1 block or on its own)
through the C ABI: one case table for the CPU emulation build and the GPU.  Everything is exact: the reference is integer arithmetic on unpacked +-1 arrays
(bits_cases.make_inputs: oracle/np_oracle.py's convolution, then ``+1 iff not (fl(fl(acc * alpha) + b) < 0)``) and ``np_maxpool`` below."""
import ctypes as C

import numpy as np

import bits_cases as B

F = np.float32
ALT = 0x100          # MN_BITCONV_ALT: the measurement-only twin kernel of a tiled geometry

# nin's hidden layers at full size (models/nin.py _PLAN, DEFAULT_CFG): (Cin, Cout, k, pad, map, pool behind it)
NIN_LAYERS = [(192, 160, 1, 0, 32, 0), (160, 96, 1, 0, 32, 2), (96, 192, 5, 2, 16, 0), (192, 192, 1, 0, 16, 0), (192, 192, 1, 0, 16, 2), (192, 192, 3, 1, 8, 0),
              (192, 192, 1, 0, 8, 0)]


def nin_case(i, n=2):
    cin, cout, k, p, hw, pool = NIN_LAYERS[i]
    return dict(x_shape=(n, cin, hw, hw), w_shape=(cout, cin, k, k), padding=p, pool=pool)


# small / adversarial: channel counts that are not multiples of 32, batch 1 and 5, maps that do not fill a tile, every template instantiation
SMALL = [
    dict(x_shape=(5, 96, 8, 8), w_shape=(40, 96, 5, 5), padding=2),                      # k_bitconv_tile<5,3>, four images per block, the last block half empty
    dict(x_shape=(1, 96, 16, 16), w_shape=(33, 96, 5, 5), padding=2),                    # k_bitconv_tile<5,3>, one whole image per block
    dict(x_shape=(1, 40, 12, 20), w_shape=(33, 40, 5, 5), padding=2),                    # k_bitconv_tile<5,0>, two tiles per row, neither dimension a tile multiple
    dict(x_shape=(5, 33, 4, 6), w_shape=(40, 33, 5, 5), padding=2),                      # k_bitconv_tile<5,0>, map smaller than the window reach: every pixel a border
    dict(x_shape=(1, 160, 8, 16), w_shape=(96, 160, 5, 5), padding=2),                   # k_bitconv_tile<5,0>, five words, two images' worth of lanes on one
    dict(x_shape=(5, 20, 8, 8), w_shape=(40, 20, 5, 5), padding=2),                      # k_bitconv_tile<5,0>, a single word
    dict(x_shape=(5, 192, 8, 8), w_shape=(40, 192, 3, 3), padding=1, alt=True),          # k_bitconv_tile<3,6>
    dict(x_shape=(1, 40, 8, 12), w_shape=(33, 40, 3, 3), padding=1, alt=True),           # k_bitconv_tile<3,0>
    dict(x_shape=(1, 96, 8, 12), w_shape=(40, 96, 5, 5), padding=2, alt=True),           # k_bitconv_direct<5>
    dict(x_shape=(5, 40, 8, 8), w_shape=(40, 40, 1, 1), pool=2),                         # k_bitconv1_pool3<8>
    dict(x_shape=(1, 160, 6, 10), w_shape=(96, 160, 1, 1), pool=2),                      # k_bitconv1_pool3<8>, 6 x 10 -> 3 x 5
    dict(x_shape=(1, 96, 7, 9), w_shape=(33, 96, 1, 1), pool=2),                         # k_bitconv1_pool3<8>, odd map: 7 x 9 -> 4 x 5
    dict(x_shape=(1, 288, 8, 8), w_shape=(40, 288, 1, 1), pool=2),                       # k_bitconv1_pool3<0>, nine words
    dict(x_shape=(5, 64, 8, 8), w_shape=(64, 32, 1, 1), groups=2, pool=2),               # k_bitconv1_pool3<0>, grouped
]
INSTANTIATIONS = {"k_bitconv_tile<5,3>", "k_bitconv_tile<5,0>", "k_bitconv_tile<3,6>", "k_bitconv_tile<3,0>", "k_bitconv_direct<5>", "k_bitconv1_pool3<8>",
                  "k_bitconv1_pool3<0>", "k_bits_maxpool"}
POOLS = [(2, 2, 0), (3, 2, 1)]
POOL_MAPS = [(8, 8), (16, 16), (32, 32), (16, 32)]


def np_maxpool(a, k, s, p):
    """max-pool of an integer [N, C, H, W] array, floor mode; padding never wins (nn.MaxPool2d pads with -inf)."""
    N, Cc, H, W = a.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dt = np.int8 if a.dtype == np.int8 else np.int32          # (+-1 codes stay bytes: -128 is still below every cell)
    big = np.full((N, Cc, H + 2 * p + k, W + 2 * p + k), -128, dtype=dt)
    big[:, :, p:p + H, p:p + W] = a
    out = np.full((N, Cc, Ho, Wo), -128, dtype=dt)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, big[:, :, dy:dy + s * Ho:s, dx:dx + s * Wo:s])
    assert (out > -128).all()          # every window holds an in-image cell
    return out.astype(a.dtype)


def pooled_size(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def run_bitconv(be, x_log, w, b, groups=1, padding=0, pool=0, alt=False, out_order=None):
    """Pack the table and the input bits, run mn_bitconv_fwd; returns (unpacked +-1 output, kernel name)."""
    g = be.geom(x_log.shape, w.shape, padding=padding, groups=groups)
    assert be.lib.mn_bitconv_supported(C.byref(g)) == 1, "geometry must be covered by the bit kernels"
    nb = int(be.lib.mn_bitconv_table_bytes(C.byref(g)))
    assert nb > 0 and nb % 4 == 0
    table = B._empty_i32(be, (nb // 4,))
    order = B._dev_i32(be, np.asarray(out_order, dtype=np.int32)) if out_order is not None else None
    dW, dB = be.to_dev(w), be.to_dev(b)
    be.call("mn_bitconv_pack", C.byref(g), be.ptr(dW), be.ptr(dB), be.ptr(order), be.ptr(table), be.stream)
    assert int(B._host_u32(be, table)[0]) == 0, "every row's decision is monotone in acc"
    N, _, H, Wd = x_log.shape
    xb = B._dev_i32(be, B.np_pack(x_log).view(np.int32))
    Ho, Wo = {0: (H, Wd), 1: (H // 2, Wd // 2), 2: (pooled_size(H, 3, 2, 1), pooled_size(Wd, 3, 2, 1))}[pool]
    Oc = w.shape[0]
    yb = B._empty_i32(be, (N, (Oc + 31) // 32, Ho, Wo))
    be.call("mn_bitconv_fwd", C.byref(g), be.ptr(table), be.ptr(xb), be.ptr(yb), int(pool) | (ALT if alt else 0), be.stream)
    name = be.lib.mn_last_kernel().decode()
    got = B._host_u32(be, yb)
    if Oc % 32:
        assert not (got[:, -1] >> np.uint32(Oc % 32)).any(), "unused bits of the last output word are 0"
    return B.np_unpack(got, Oc), name


def check_case(be, x_shape, w_shape, groups=1, padding=0, pool=0, alt=False, seed=0, W=3):
    """Output bits == the integer model, bit for bit (pooled: its max-pool); returns the kernel that ran."""
    _, x_log, w, b, a_ref = B.make_inputs(x_shape, w_shape, groups, 0, padding, seed, W)
    got, name = run_bitconv(be, x_log, w, b, groups, padding, pool, alt)
    ref = a_ref if not pool else np_maxpool(a_ref, *(POOLS[pool - 1]))
    print(name, x_shape, w_shape, "pool", pool, "W", W, "mismatches", int((got != ref).sum()), "of", got.size)
    assert got.shape == ref.shape and np.array_equal(got, ref), (name, int((got != ref).sum()), got.size)
    return name


# Several output words per block (tests/deploy_grid.py): the smallest shapes at which a block of the popcount kernels walks ow0 .. ow1 over more than one word.
# (id, check_case keywords, out_order shuffle, kernel).  Seven words over bx = 344: four blocks of two, the last takes one.  Wall time of the whole case on the CPU
# emulation build (8 cores, judge included) beside each: all below 20 s, so tests/test_bits_nin_emu.py runs the table as well as tests/test_gpu_bits_nin.py.
LARGE_GRID = [
    ("k1", dict(x_shape=(86, 32, 32, 32), w_shape=(224, 32, 1, 1)), 4, "k_bitconv<1,1,0>"),                                        # emulated: 7 s
    ("k3_grouped_partial_word", dict(x_shape=(86, 32, 32, 32), w_shape=(200, 16, 3, 3), groups=2, padding=1), 4, "k_bitconv<3,1,0>"),          # O % 32 = 8.  12 s
    ("tile5", dict(x_shape=(86, 8, 32, 32), w_shape=(224, 8, 5, 5), padding=2), 0, "k_bitconv_tile<5,0>"),                         # 4 * 86 tiles of 16 x 16.  18 s
    ("k1_pool3", dict(x_shape=(344, 32, 32, 32), w_shape=(224, 32, 1, 1), pool=2), 0, "k_bitconv1_pool3<8>"),                      # 344 * 256 pooled pixels.  14 s
]


def check_large(be, idx, seed=1600):
    """One LARGE_GRID case: the library's own launch rule says that a block takes at least two output words and the last block fewer; then two runs into poisoned
    buffers, identical, equal to the integer model bit for bit (position j holds channel order[j])."""
    import deploy_grid as DG
    from codes_cases import shuffle_order
    cid, kw, s, kernel = LARGE_GRID[idx]
    x_shape, w_shape, groups, padding, pool = kw["x_shape"], kw["w_shape"], kw.get("groups", 1), kw.get("padding", 0), kw.get("pool", 0)
    N, _, H, Wd = x_shape
    Oc = w_shape[0]
    Ho, Wo = (pooled_size(H, 3, 2, 1), pooled_size(Wd, 3, 2, 1)) if pool == 2 else (H, Wd)
    bx = DG.tile_blocks(N, H, Wd) if kernel.startswith("k_bitconv_tile") else DG.pixel_blocks(N * Ho * Wo, 256)
    gy, per = DG.assert_uneven_deal(be, bx, (Oc + 31) // 32)
    _, x_log, w, b, a_ref = B.make_inputs(x_shape, w_shape, groups, 0, padding, seed + idx, 3)
    assert (a_ref == 1).any() and (a_ref == -1).any()
    order = shuffle_order(Oc, s) if s else None
    got, name = run_bitconv(be, x_log, w, b, groups, padding, pool, out_order=order)
    again, _ = run_bitconv(be, x_log, w, b, groups, padding, pool, out_order=order)
    assert name == kernel, name
    assert np.array_equal(got, again), "two runs give identical bits"
    ref = a_ref[:, order] if s else a_ref
    if pool:
        ref = np_maxpool(ref, *(POOLS[pool - 1]))
    bad = int((got != ref).sum())
    print(name, cid, x_shape, w_shape, "pool", pool, "shuffle", s, "grid.y", gy, "per", per, "mismatches", bad, "of", got.size)
    assert got.shape == ref.shape and bad == 0, (name, bad, got.size)


def check_consumer_order(be, seed=0):
    """The tiled 5x5 block honours out_order like every other bit block."""
    sh = dict(x_shape=(1, 96, 8, 8), w_shape=(64, 96, 5, 5), padding=2)
    _, x_log, w, b, a_ref = B.make_inputs(sh["x_shape"], sh["w_shape"], 1, 0, 2, seed, 3)
    j = np.arange(64)
    order = (j % 4) * 16 + j // 4
    got, _ = run_bitconv(be, x_log, w, b, 1, 2, out_order=order)
    assert np.array_equal(got, a_ref[:, order])


def check_standalone_pool(be, k, s, p, H, Wd, seed=0, Cc=40, N=2):
    import torch
    r = np.random.default_rng(seed)
    a = np.where(r.standard_normal((N, Cc, H, Wd)) > 0, 1, -1).astype(np.int8)
    xb = B._dev_i32(be, B.np_pack(a).view(np.int32))
    Ho, Wo = pooled_size(H, k, s, p), pooled_size(Wd, k, s, p)
    yb = B._empty_i32(be, (N, (Cc + 31) // 32, Ho, Wo))
    be.call("mn_bits_maxpool", be.ptr(xb), N, (Cc + 31) // 32, H, Wd, k, s, p, be.ptr(yb), be.stream)
    name = be.lib.mn_last_kernel().decode()
    got = B._host_u32(be, yb)
    assert not (got[:, -1] >> np.uint32(Cc % 32)).any()
    ref = torch.nn.functional.max_pool2d(torch.from_numpy(a.astype(F)), k, s, p).numpy().astype(np.int8)
    assert np.array_equal(B.np_unpack(got, Cc), ref) and np.array_equal(ref, np_maxpool(a, k, s, p))
    return name


def check_folded_pool(be, k, s, p, H, Wd, seed=0, W=3):
    """1x1 block with the pool folded in == torch's max_pool2d of the un-pooled block's output (itself checked against the integer model)."""
    import torch
    x_shape, w_shape = (2, 40, H, Wd), (40, 40, 1, 1)
    _, x_log, w, b, a_ref = B.make_inputs(x_shape, w_shape, 1, 0, 0, seed, W)
    full, _ = run_bitconv(be, x_log, w, b)
    assert np.array_equal(full, a_ref)
    got, name = run_bitconv(be, x_log, w, b, pool=POOLS.index((k, s, p)) + 1)
    ref = torch.nn.functional.max_pool2d(torch.from_numpy(full.astype(F)), k, s, p).numpy().astype(np.int8)
    assert np.array_equal(got, ref)
    return name


def check_refusals(be):
    """What the entry points do not cover keeps failing with MN_ENOTSUP (rc -2 is not assumed: any non-zero rc, and mn_bitconv_supported == 0)."""
    bad = [be.geom((1, 64, 8, 8), (64, 32, 5, 5), padding=2, groups=2), be.geom((1, 320, 8, 8), (32, 320, 5, 5), padding=2),
           be.geom((1, 64, 8, 8), (64, 64, 5, 5), padding=1), be.geom((1, 64, 8, 8), (64, 64, 5, 5), padding=2, stride=2),
           be.geom((1, 64, 8, 8), (64, 64, 7, 7), padding=3)]
    for g in bad:
        assert be.lib.mn_bitconv_supported(C.byref(g)) == 0 and be.lib.mn_bitconv_table_bytes(C.byref(g)) == 0
    dummy = B._empty_i32(be, (4096,))
    g5 = be.geom((1, 64, 8, 8), (64, 64, 5, 5), padding=2)
    g3 = be.geom((1, 64, 8, 8), (64, 64, 3, 3), padding=1)
    g1 = be.geom((1, 32, 8, 8), (64, 32, 1, 1))
    for g, pool in ((g5, 1), (g5, 2), (g3, 2), (g1, 3), (g1, ALT), (g1, 2 | ALT)):
        assert be.lib.mn_bitconv_fwd(C.byref(g), be.ptr(dummy), be.ptr(dummy), be.ptr(dummy), pool, be.stream) != 0, pool
    for k, s, p in ((3, 1, 1), (4, 2, 1), (3, 2, 2), (2, 1, 0)):
        assert be.lib.mn_bits_maxpool(be.ptr(dummy), 1, 1, 8, 8, k, s, p, be.ptr(dummy), be.stream) != 0, (k, s, p)
