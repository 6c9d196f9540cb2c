"""The two ends of the W8A8 byte plan through the C ABI (csrc/conv_first.hip: mn_conv2d_first_bytes; csrc/qgemm_codes_w8_ends.h: mn_code8conv_fwd_f32): one case table
for both builds.  The first conv's map equals, byte for byte, the numpy fp32 chain on today's y AND today's three launches; the classifier a numpy judge (acc in
int64, y in fp64) within three fp32 roundings.  Output buffers are poisoned."""
import ctypes as C

import numpy as np

from bits_cases import _empty_i32, _host_u32
from bits_ends_cases import FIRST_CASES, first_inputs
from codes_ends_cases import make_chan_y          # (codes_cases.make_chan on fp32 y: both signs of gamma, gamma = 0, saturating channels, a rounding boundary on an attained y)
from codes_w8_cases import chain_codes, make_inputs, pack_table, to_map
from micronet_amd._lib import MN_ENOTSUP

F = np.float32
FIRST = FIRST_CASES + [(1, 3, 24, 8, 40, 3)]          # the seven shapes of the bit ends, and one strip of 192 pixels: three chunks through the parked tile
ALPHA = F(1.0 / 255.0) * F(1.0 / 255.0)          # the stored fp32 product of the weight and the activation scale
# (id, N, C, H, W, O, seed, every input code / every weight code or None)
CLASSIFIER = [
    ("c16_one_slot", 1, 16, 4, 4, 10, 8400, None),                   # one k-step: three waves idle
    ("c80_uneven_split", 1, 80, 4, 4, 10, 8401, None),               # 5 slots: two k-steps, 3 padding slots, two waves idle
    ("c20_tails_hw15", 1, 20, 3, 5, 10, 8402, None),                 # 0x80 tail bytes against zero weight bytes; a partial pixel tile
    ("hw70_o16", 1, 32, 7, 10, 16, 8403, None),                      # a second pixel block; a full M tile
    ("n2_o24", 2, 48, 3, 5, 24, 8404, None),                         # two images in one pixel tile; two M tiles over the same B operands
    ("c1024_registers", 1, 1024, 2, 4, 10, 8405, None),              # 16 k-steps: the most the B operands stay in registers for
    ("c1040_streamed", 1, 1040, 2, 4, 24, 8406, None),               # 17 k-steps: B streamed per tile, uneven split
    ("c1040_saturated", 1, 1040, 2, 4, 10, 8407, (255, 255)),        # acc = 1040 * 255 * 255 > 2^24: the int -> float rounding, the combine's range
    ("o70_two_sets", 1, 32, 4, 4, 70, 8409, None),                   # more than 64 outputs: a second set, dealt over grid.y
    ("all_0x80", 1, 32, 4, 4, 10, 8408, (0, 77)),                    # acc = 0: y = bias exactly
]
# classifier geometries refused: 3x3, stride 2, groups 2, C * taps beyond int32
REFUSED = [dict(x_shape=(1, 32, 8, 8), w_shape=(10, 32, 3, 3), padding=1), dict(x_shape=(1, 32, 8, 8), w_shape=(10, 32, 1, 1), stride=2),
           dict(x_shape=(1, 32, 8, 8), w_shape=(10, 16, 1, 1), groups=2), dict(x_shape=(1, 33026, 1, 1), w_shape=(10, 33026, 1, 1))]


def three_launches(be, g, dY, chan):
    """Today's first stage behind the conv on the same backend: mn_qa_fwd(in_f32 = 1) -> uint8 codes, mn_code8_pack_codes -> the map."""
    codes = be.to_dev_u8(np.full((g.N, g.O, g.H, g.W), 0xee, dtype=np.uint8))
    be.call("mn_qa_fwd", 1, be.ptr(dY), be.ptr(be.to_dev(chan)), g.N, g.O, g.H, g.W, 8, 0, be.ptr(codes), None, be.stream)
    m = be.empty_i8((g.N, (g.O + 15) // 16, g.H * g.W, 16))
    be.call("mn_code8_pack_codes", be.ptr(codes), g.N, g.O, g.H * g.W, be.ptr(m), be.stream)
    return be.to_host(m).view(np.uint8)


def first_bytes(be, g, dX, dW, dB, chan):
    """mn_conv2d_first_bytes into a poisoned map with a guard of 64 bytes behind it: (map, kernel name)."""
    size = g.N * ((g.O + 15) // 16) * g.H * g.W * 16
    buf = be.empty_i8((size + 64,))
    be.call("mn_conv2d_first_bytes", C.byref(g), be.ptr(dX), be.ptr(dW), be.ptr(dB), be.ptr(be.to_dev(chan)), be.ptr(buf), be.stream)
    got = be.to_host(buf).view(np.uint8)
    assert (got[size:] == 77).all(), "the guard behind the map is intact"
    return got[:size].reshape(g.N, -1, g.H * g.W, 16), be.lib.mn_last_kernel().decode()


def _first_setup(be, N, Cc, H, W, Oc, k, seed):
    x, w, b = first_inputs(N, Cc, H, W, Oc, k, seed)
    g = be.geom(x.shape, w.shape, padding=(k - 1) // 2)
    assert be.lib.mn_conv2d_first_bytes_supported(C.byref(g)) == 1
    return x, w, b, g, be.to_dev(x), be.to_dev(w)


def check_first(be, idx):
    N, Cc, H, W, Oc, k = FIRST[idx]
    x, w, b, g, dX, dW = _first_setup(be, N, Cc, H, W, Oc, k, 8500 + idx)
    dB = be.to_dev(b)
    dY = be.conv_fwd(g, be.actq(0), dX, dW, dB, 0)
    y = be.to_host(dY)
    chan, y0 = make_chan_y(y, 8500 + idx)
    assert (chan[0] == 1).all() and not chan[1].any()          # alpha = 1, bias = 0: codes_w8_cases.chain_codes on y itself IS the in_f32 chain, step for step
    chain = chain_codes(y, chan, 0)
    want = three_launches(be, g, dY, chan)
    assert np.array_equal(want, to_map(chain)), "the two judges disagree: mn_qa_fwd(in_f32 = 1) + pack vs the numpy chain on today's y"
    assert len(np.unique(chain)) > 32 and (chain[:, 1] == 0).all() and (chain[:, 2] == 255).all() and len(np.unique(chain[:, 0])) == 1 and chan[4, 3] < 0
    assert (y[:, 4] == y0[4]).any() and (y[:, 5] == y0[5]).any(), "a rounding boundary sits on an attained y"
    got, name = first_bytes(be, g, dX, dW, dB, chan)
    print(name, FIRST[idx], "bytes differing from the three launches:", int((got != want).sum()), "of", got.size, "distinct codes", len(np.unique(chain)))
    assert name == "k_c1b_fwd<%d,5>" % (1 if Oc <= 64 else 2) and np.array_equal(got, want)
    if Oc % 16:
        assert (got[:, -1, :, Oc % 16:] == 0x80).all(), "tail channels of the last block are the code 0"


def check_first_wild(be, kind):
    """A NaN bias, a non-finite constant: no gate, the chain is evaluated as it is -- the bytes are the three launches'."""
    x, w, b, g, dX, dW = _first_setup(be, 2, 3, 8, 8, 40, 5, 8510)
    chan, _ = make_chan_y(be.to_host(be.conv_fwd(g, be.actq(0), dX, dW, be.to_dev(b), 0)), 8510)          # constants on the spread of the unperturbed y
    if kind == "nan_bias":
        b[7] = F(np.nan)
    else:
        chan[4, 9], chan[3, 11] = F(np.inf), F(np.nan)
    dB = be.to_dev(b)
    want = three_launches(be, g, be.conv_fwd(g, be.actq(0), dX, dW, dB, 0), chan)
    assert np.array_equal(first_bytes(be, g, dX, dW, dB, chan)[0], want)


def check_classifier(be, idx):
    cid, N, Cc, H, W, Oc, seed, fill = CLASSIFIER[idx]
    codes, w, acc = make_inputs((N, Cc, H, W), Oc, 1, 1, seed, fill)
    bias, one, zero = (np.random.default_rng(seed).standard_normal(Oc) * 0.2).astype(F), np.ones(Oc, dtype=F), np.zeros(Oc, dtype=F)
    chan = np.stack([one * ALPHA, bias, zero, one, one, zero, one * ALPHA, bias, one]).astype(F)          # identity BatchNorm rows
    g = be.geom(codes.shape, w.shape)
    assert be.lib.mn_code8conv_f32_supported(C.byref(g)) == 1
    table = pack_table(be, g, w, chan)
    assert not _host_u32(be, table)[[0, 7]].any(), "finite constants, weights on the grid"
    HW = H * W
    yb = be.empty((N * Oc * HW + 16 * HW + 64,))          # poisoned; behind y, where a row past O or a pixel past the batch would land
    be.call("mn_code8conv_fwd_f32", C.byref(g), be.ptr(table), be.ptr(be.to_dev_u8(to_map(codes))), be.ptr(yb), be.stream)
    got, name = be.to_host(yb), be.lib.mn_last_kernel().decode()
    y = got[:N * Oc * HW].reshape(N, Oc, H, W).astype(np.float64)
    mag = np.abs(acc) * float(ALPHA) + np.abs(bias.astype(np.float64)).reshape(1, -1, 1, 1)
    ref = acc * float(ALPHA) + bias.astype(np.float64).reshape(1, -1, 1, 1)
    # at most three fp32 roundings (int -> float, the product, the sum), each <= 2^-24 relative; one factor left for second-order terms
    worst = float((np.abs(y - ref) / np.maximum(mag, 1e-300)).max())
    print(name, cid, "max |y - ref| / (|acc| alpha + |bias|) = %.3g (bound %.3g)" % (worst, 2.0 ** -22), "max |acc|", int(np.abs(acc).max()))
    assert name == "k_code8conv_f32" and (np.abs(y - ref) <= 2.0 ** -22 * mag).all()
    assert (got[N * Oc * HW:] == F(-1234.5)).all(), "channels >= O and pixels >= N H W are never written"
    if fill == (255, 255):
        assert int(acc.min()) == Cc * 255 * 255 > 2 ** 24
    if fill == (0, 77):
        assert not acc.any() and np.array_equal(got[:N * Oc * HW].reshape(N, Oc, HW), np.broadcast_to(bias.reshape(1, -1, 1), (N, Oc, HW)))


def check_refused(be, idx):          # MN_ENOTSUP and nothing written: the classifier's geometries, and (idx == len(REFUSED)) a first conv whose strip is over the LDS cap
    buf, f = _empty_i32(be, (64,)), be.to_dev(np.zeros(64, dtype=F))
    if idx == len(REFUSED):
        g = be.geom((1, 3, 4, 1024), (40, 3, 5, 5), padding=2)
        assert be.lib.mn_conv2d_first_supported(C.byref(g), 0) == 1 and be.lib.mn_conv2d_first_bytes_supported(C.byref(g)) == 0
        assert be.lib.mn_conv2d_first_bytes(C.byref(g), be.ptr(f), be.ptr(f), be.ptr(f), be.ptr(f), be.ptr(buf), be.stream) == MN_ENOTSUP
    else:
        kw = REFUSED[idx]
        g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), groups=kw.get("groups", 1))
        assert be.lib.mn_code8conv_f32_supported(C.byref(g)) == 0
        assert be.lib.mn_code8conv_fwd_f32(C.byref(g), be.ptr(buf), be.ptr(buf), be.ptr(buf), be.stream) == MN_ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all(), "a refused call writes nothing"


# (id, check, argument) for the two drivers: tests/test_codes_w8_ends_emulated.py, tests/test_gpu_codes_w8_ends.py
CHECKS = ([("first%d" % i, check_first, i) for i in range(len(FIRST))] + [("first_" + k, check_first_wild, k) for k in ("nan_bias", "nonfinite_constant")]
          + [(c[0], check_classifier, i) for i, c in enumerate(CLASSIFIER)] + [("refused%d" % i, check_refused, i) for i in range(len(REFUSED) + 1)])
