"""The byte form of the DoReFa W8A8 hidden block (csrc/qgemm_codes_w8.h: mn_code8conv_*, mn_code8_*) through the C ABI: one case table for the CPU emulation build and
the GPU.  The judge is plain numpy: acc = sum j (2k - 255) in int64 (asserted within int32), then the element-wise fp32 chain of ``codes_cases.chain_codes`` with 255
levels.  The kernel's bytes must equal the judge's codes exactly, in buffers poisoned before the launch."""
import ctypes as C

import numpy as np

from oracle import np_oracle as O
from bits_cases import _dev_i32, _empty_i32, _host_u32
from codes_cases import make_chan, shuffle_order          # (constants around the accumulator's spread: both signs of gamma, gamma = 0, saturating channels, a boundary on an attained value)
from iao8_cases import np_block, np_unblock
from micronet_amd._lib import MN_ENOTSUP

F = np.float32
W8 = (8, 8, 8)
# (id, x shape, O, KS, groups, out_order shuffle, pool, seed, every input code / every weight code or None)
BLOCKS = [
    ("k1_tail_channels", (1, 20, 3, 5), 24, 1, 1, 0, 0, 8100, None),                # C % 16 = 4, 15 pixels, a partial output block
    ("k1_grouped_pool_shuffle", (2, 32, 4, 4), 32, 1, 2, 2, 1, 8101, None),
    ("k1_long_k", (1, 272, 2, 3), 80, 1, 1, 0, 0, 8102, None),                      # 17 slots: 5 k-steps, 3 padding slots; two sets
    ("k3_grouped", (1, 32, 5, 3), 32, 3, 2, 0, 0, 8103, None),                      # borders on every side
    ("k3_many_chunks_pool", (1, 80, 4, 4), 16, 3, 1, 0, 1, 8104, None),             # 45 slots: the last k-step holds one
    ("saturated_255_against_0", (1, 32, 5, 3), 32, 3, 2, 0, 0, 8103, (255, 0)),     # acc = -255 * 255 * 16 per in-bounds tap
    ("saturated_all_0", (1, 32, 5, 3), 32, 3, 2, 0, 0, 8103, (0, 77)),              # every byte 0x80: acc = 0
]
# (geometry keywords, widths)
REFUSED = [
    (dict(x_shape=(1, 33026, 1, 1), w_shape=(16, 33026, 1, 1)), W8),                # Cg * taps = 33026: beyond int32
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1), stride=2), W8),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 5, 5), padding=2), W8),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 8, 1, 1), groups=4), W8),             # grouped with 8 channels per group
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (4, 4, 4)),
    (dict(x_shape=(1, 32, 8, 8), w_shape=(32, 32, 1, 1)), (8, 8, 4)),
]


# uint8 codes [N, C, H, W] <-> the byte map [N, ceil(C/16), H*W, 16] as uint8: code ^ 0x80, tail channels 0x80
to_map = lambda codes: np_block(codes.view(np.int8)).view(np.uint8) ^ np.uint8(0x80)
from_map = lambda m, Cc, H, W: np_unblock(m.view(np.int8), Cc, H, W).view(np.uint8) ^ np.uint8(0x80)


def make_inputs(x_shape, Oc, KS, groups, seed, fill=None):
    """(codes uint8, stored weights fp32 on the grid (2k - 255) / 255, exact accumulator int64)."""
    r = np.random.default_rng(seed)
    codes = r.integers(0, 256, size=x_shape).astype(np.uint8)
    codes[:, :, 0, 0], codes[0, :, -1, -1] = 0, 255                      # a whole-zero pixel and a saturated one
    k = r.integers(0, 256, size=(Oc, x_shape[1] // groups, KS, KS)).astype(np.int64)
    if fill is not None:
        codes[:], k[:] = fill
    w = (F(2) * (k.astype(F) / F(255)) - F(1)).astype(F)                 # what the DoReFa weight quantizer stores
    acc = O.conv2d_fwd(codes.astype(np.int64), 2 * k - 255, None, padding=KS // 2, groups=groups, acc=np.int64)
    assert np.abs(acc).max() < 2 ** 31
    return codes, w, acc


def chain_codes(acc, chan, pool):
    """codes_cases.chain_codes with 255 levels: the element-wise fp32 chain of k_qa_fwd, step by step."""
    alpha, bias, mean, invstd, ga, beb = (chan[i].reshape(1, -1, 1, 1) for i in range(6))
    y = (acc.astype(F) * alpha).astype(F) + bias
    zh = ((y - mean).astype(F) * invstd).astype(F)
    z = ((zh * ga).astype(F) + beb).astype(F)
    a = np.where(z > 0, z, F(0)).astype(F)
    if pool:
        N, Cc, H, W = a.shape
        a = a.reshape(N, Cc, H // 2, 2, W // 2, 2).max(axis=(3, 5))
    c = np.minimum(np.maximum((a * F(0.1)).astype(F), F(0)), F(1)).astype(F)
    return np.floor(((c / (F(1) / F(255))).astype(F) + F(0.5)).astype(F)).astype(np.uint8)


def pack_table(be, g, w, chan, order=None):
    nb = int(be.lib.mn_code8conv_table_bytes(C.byref(g), *W8))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    dW, dC = be.to_dev(w), be.to_dev(chan)
    be.call("mn_code8conv_pack", C.byref(g), be.ptr(dW), be.ptr(dC), 8, 8, 8, be.ptr(dO), be.ptr(table), be.stream)
    return table


def check_block(be, idx):
    """Pack the table, run mn_code8conv_fwd into a poisoned map: the codes the positions hold equal the judge's (channel out_order[j] at position j, the code 0 past O)."""
    cid, x_shape, Oc, KS, groups, shuffle, pool, seed, fill = BLOCKS[idx]
    codes, w, acc = make_inputs(x_shape, Oc, KS, groups, seed, fill)
    chan = make_chan(acc, seed)
    ref = chain_codes(acc, chan, pool)
    order = shuffle_order(Oc, shuffle) if shuffle else None
    g = be.geom(x_shape, w.shape, padding=KS // 2, groups=groups)
    assert be.lib.mn_code8conv_supported(C.byref(g), *W8) == 1
    table = pack_table(be, g, w, chan, order)
    hdr = _host_u32(be, table)
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0 and int(hdr[6]) == (8 | 8 << 8 | 8 << 16), "finite constants, weights on the grid, a valid order"
    N, _, H, Wd = x_shape
    Ho, Wo, OB = (H // 2 if pool else H), (Wd // 2 if pool else Wd), (Oc + 15) // 16
    yb = be.empty_i8((N, OB, Ho * Wo, 16))          # poisoned
    be.call("mn_code8conv_fwd", C.byref(g), be.ptr(table), be.ptr(be.to_dev_u8(to_map(codes))), be.ptr(yb), int(pool), be.stream)
    got, name = from_map(be.to_host(yb), OB * 16, Ho, Wo), be.lib.mn_last_kernel().decode()
    want = np.zeros_like(got)
    want[:, :Oc] = ref[:, order] if shuffle else ref
    bad = int((got != want).sum())
    print(name, cid, "mismatches against the judge", bad, "of", got.size, "distinct codes", len(np.unique(ref)))
    assert name == "k_code8conv<%d,%d>" % (KS, pool) and got.shape == want.shape and bad == 0, (name, bad, got.size)
    if fill is None:
        assert len(np.unique(ref)) > 32 and len(np.unique(ref[:, 0])) == 1 and (ref[:, 1] == 0).all() and (ref[:, 2] == 255).all() and chan[4, 3] < 0
        assert (acc[:, 4] == int(chan[2, 4])).any() and (acc[:, 5] == int(chan[2, 5])).any(), "a rounding boundary sits on an attained accumulator value"
    else:
        assert (int(acc.min()), int(acc.max())) == ((-255 * 255 * 144, -255 * 255 * 64) if fill[0] else (0, 0)), "an interior pixel sees 9 x 16 positions, a corner 4 x 16"


def check_roundtrip(be, Cc=20):
    """NCHW codes -> map -> NCHW codes; tail channels 0x80, every byte of the poisoned buffers written, a guard region behind the map intact."""
    codes = np.random.default_rng(8200).integers(0, 256, size=(3, Cc, 3, 5)).astype(np.uint8)
    want = to_map(codes)
    buf = be.empty_i8((want.size + 64,))          # the map and a guard of 64 bytes behind it
    be.call("mn_code8_pack_codes", be.ptr(be.to_dev_u8(codes)), 3, Cc, 15, be.ptr(buf), be.stream)
    got = be.to_host(buf).view(np.uint8)
    assert np.array_equal(got[:want.size], want.ravel()) and (got[want.size:] == 77).all()
    back = be.to_dev_u8(np.full(codes.shape, 0xee, dtype=np.uint8))
    be.call("mn_code8_unpack_codes", be.ptr(buf), 3, Cc, 15, be.ptr(back), be.stream)
    assert np.array_equal(be.to_host(back).view(np.uint8), codes)


def check_refused(be, idx):
    kw, (ai, wb, ao) = REFUSED[idx]
    g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), groups=kw.get("groups", 1))
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.zeros(64, dtype=F))
    assert be.lib.mn_code8conv_supported(C.byref(g), ai, wb, ao) == 0 and int(be.lib.mn_code8conv_table_bytes(C.byref(g), ai, wb, ao)) == 0
    assert be.lib.mn_code8conv_pack(C.byref(g), be.ptr(f), be.ptr(f), ai, wb, ao, None, be.ptr(buf), be.stream) == MN_ENOTSUP
    if (ai, wb, ao) == W8:          # (the forward takes no widths)
        assert all(be.lib.mn_code8conv_fwd(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), pool, be.stream) == MN_ENOTSUP for pool in (0, 1))
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


def check_counters(be, seed=8300):
    """Word 0 counts the rows with non-finite constants, word 7 a weight off the grid and a bad out_order entry."""
    codes, w, acc = make_inputs((1, 32, 4, 4), 32, 1, 2, seed)
    chan = make_chan(acc, seed)
    g = be.geom(codes.shape, w.shape, groups=2)
    hdr = _host_u32(be, pack_table(be, g, w, chan))
    assert (int(hdr[0]), int(hdr[7]), int(hdr[1]), int(hdr[8])) == (0, 0, 1, 16)
    bad = chan.copy()
    bad[0, 7], bad[4, 9], bad[3, 11] = F(np.inf), F(np.nan), F(2e9)
    hdr = _host_u32(be, pack_table(be, g, w, bad))
    assert int(hdr[0]) == 3 and int(hdr[7]) == 0
    w2, order = w.copy(), np.arange(32)
    w2[5, 3, 0, 0] += F(1.0 / 255)          # half a grid step
    order[3] = 32
    assert int(_host_u32(be, pack_table(be, g, w2, chan, order))[7]) == 2 and int(_host_u32(be, pack_table(be, g, w2, chan))[0]) == 0


# (id, check, argument) for the two drivers: tests/test_codes_w8_emulated.py, tests/test_gpu_codes_w8.py
CHECKS = ([(b[0], check_block, i) for i, b in enumerate(BLOCKS)] + [("roundtrip_c20", check_roundtrip, 20), ("counters", check_counters, 8300)]
          + [("refused%d" % i, check_refused, i) for i in range(len(REFUSED))])
