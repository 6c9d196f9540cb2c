"""The two ends of the int8 deployment of the BN-folded IAO graph (csrc/qgemm_iao8_ends.h: mn_i8first_*, mn_i8conv_fwd_f32) through the C ABI: one case table for the
CPU emulation build and the GPU.  Every kernel comparison is exact, in buffers poisoned before the launch.

The judge is tests/iao8_cases.py's, never the code under test: ``oracle.np_oracle.conv2d_fwd(..., acc=np.int64)`` on integer codes and the contract's chain replayed
in numpy float32.  For the first block the fp32 image is BUILT from a case's codes -- x = (j + u) s_a with u in (-0.49, 0.49), a few elements per image overridden
with exact rounding ties, values far outside the range and -0.0 -- and the judge recomputes the codes from that image with ``code_of`` and convolves those."""
import ctypes as C

import numpy as np

from iao8_cases import (F, O, assert_case_is_hard, chain_codes, code_of, expect_positions, geom_of, judge, make_case, np_block, np_unblock, pack_table, qrange,
                        torch_codes)
from bits_cases import _dev_i32, _empty_i32, _host_u32
from codes_cases import shuffle_order

# (id, x shape, O, KS, out_order shuffle): seed 5200 + index
FIRST = [
    ("f5_rgb", (2, 3, 8, 8), 48, 5, 2),                    # K = 75: the second k-step is partly padding
    ("f5_all_border", (1, 3, 3, 3), 16, 5, 0),             # a map smaller than the kernel (special=False: too small for the tie channel)
    ("f5_odd_map", (3, 3, 5, 7), 33, 5, 0),                # 35 pixels < one wave, a partial output block
    ("f5_strip_cut", (1, 3, 20, 20), 16, 5, 0),            # 400 pixels: two blocks, the cut falls mid-row, halo rows on both sides
    ("f3_rgb", (2, 3, 6, 6), 64, 3, 0),                    # K = 27, one k-step
    ("f5_four_planes", (1, 4, 6, 6), 20, 5, 0),            # K = 100
    ("f5_one_plane", (1, 1, 9, 9), 16, 5, 0),              # K = 25
    ("f5_256", (1, 3, 8, 8), 256, 5, 2),                   # four sets, nin_gc's O
    ("f3_14", (1, 14, 5, 5), 16, 3, 0),                    # K = 126, the largest covered
]
NOT_SPECIAL = ("f5_all_border",)
# chain variants on f5_rgb's geometry: (id, widths (w, a), per-channel s_w, in_bits)
FIRST_CHAINS = [
    ("w4a4", (4, 4), True, 4),
    ("w8a8_per_layer", (8, 8), False, 8),
    ("in8_out4", (8, 8), True, 8),          # an 8-bit image quantizer in front of a 4-bit consumer (a_bits 4, s_out 16 times the case's)
]
# (id, x shape, O, KS, groups): seed 5300 + index
LAST = [
    ("l1_classifier", (2, 1024, 8, 8), 10, 1, 1),          # 16 k-steps, six dead rows
    ("l1_partial", (3, 40, 5, 5), 33, 1, 1),               # partial channel block, K padded, pixel remainder
    ("l1_one", (1, 16, 1, 1), 1, 1, 1),                    # one output element
    ("l3_two_groups", (1, 32, 4, 4), 20, 3, 2),            # the 3x3 form the template gives
]
# chain variants on l1_partial's geometry: (id, widths, per-channel s_w, out_order)
LAST_CHAINS = [
    ("w8a8_per_layer", (8, 8), False, False),
    ("w4a4", (4, 4), True, False),
    ("out_order", (8, 8), True, True),
]
# mn_i8first_* refuses: (geometry keywords, (in_bits, a_bits, w_bits))
FIRST_REFUSED = [
    (dict(x_shape=(1, 3, 8, 8), w_shape=(16, 3, 7, 7), padding=3), (8, 8, 8)),
    (dict(x_shape=(1, 6, 8, 8), w_shape=(16, 6, 5, 5), padding=2), (8, 8, 8)),               # K = 150
    (dict(x_shape=(1, 3, 8, 8), w_shape=(16, 3, 1, 1)), (8, 8, 8)),
    (dict(x_shape=(1, 3, 8, 8), w_shape=(16, 3, 5, 5), padding=2, stride=2), (8, 8, 8)),
    (dict(x_shape=(1, 3, 8, 8), w_shape=(16, 3, 5, 5), padding=0), (8, 8, 8)),
    (dict(x_shape=(1, 3, 8, 8), w_shape=(16, 3, 5, 5), padding=4, dilation=2), (8, 8, 8)),
    (dict(x_shape=(1, 3, 8, 8), w_shape=(48, 1, 5, 5), padding=2, groups=3), (8, 8, 8)),
    (dict(x_shape=(1, 3, 8, 8), w_shape=(16, 3, 5, 5), padding=2, in_shuffle=3), (8, 8, 8)),
] + [(dict(x_shape=(1, 3, 8, 8), w_shape=(16, 3, 5, 5), padding=2), tuple(bad if i == pos else 8 for i in range(3))) for pos in range(3) for bad in (1, 9)]


def _lib():
    from micronet_amd import _lib as L
    return L


# ---------------------------------------------------------------------------------------------- the judge
def chain_r(acc, al, b, relu):
    """The contract's chain up to r on the exact accumulator, one fp32 operation per step."""
    v = acc.astype(F)
    y = ((v * al.reshape(1, -1, 1, 1).astype(F)).astype(F) + b.reshape(1, -1, 1, 1).astype(F)).astype(F)
    return np.where(y > 0, y, F(0)).astype(F) if relu else y


def first_case(x_shape, Oc, KS, seed, widths=(8, 8), per_channel=True, special=True, extreme=False, out_bits=None):
    """make_case for a first block (groups 1), with the image quantizer's width ``in_bits``; out_bits: a narrower consumer (s_out scaled by 2^(in - out))."""
    case = make_case(x_shape, Oc, KS, 1, seed, widths=widths, per_channel=per_channel, special=special, extreme=extreme)
    case["in_bits"], case["extreme"] = case["a_bits"], extreme
    if out_bits is not None:
        case["s_out"] = F(case["s_out"] * F(1 << (case["a_bits"] - out_bits)))
        case["s_p"], case["a_bits"] = case["s_out"], out_bits
    return case


def make_image(case, seed):
    """The fp32 image of a case's codes and what the judge reads back from it: (x, codes int64).  Asserts the properties the overridden elements must have."""
    r = np.random.default_rng(seed + 1000)
    j = case["j"].astype(np.int64)
    s_a = case["s_a"]
    assert s_a == F(2.0 ** -5)
    qmin, qmax = (int(v) for v in qrange(case["in_bits"]))
    x = ((j + r.uniform(-0.49, 0.49, size=j.shape)) * float(s_a)).astype(F)
    N = j.shape[0]
    xf, jf = x.reshape(N, -1), j.reshape(N, -1)
    want = np.full(jf.shape, 1 << 20, dtype=np.int64)          # the code an overridden element must give
    for n in range(N):
        if case["extreme"]:
            xf[n, 0], want[n, 0] = F(-1e6), qmin
            continue
        free = np.ones(jf.shape[1], dtype=bool)

        def take(mask):
            i = int(np.flatnonzero(mask & free)[0])
            free[i] = False
            return i
        i = take(jf[n] == jf[n].max())
        xf[n, i], want[n, i] = F(1e6) * s_a, qmax                                   # far outside the range: clamps
        i = take(jf[n] == jf[n].min())
        xf[n, i], want[n, i] = F(-1e6) * s_a, qmin
        i = take(jf[n] == 0)
        xf[n, i], want[n, i] = F(-0.0), 0
        i = take((jf[n] >= 0) & (jf[n] < qmax))
        xf[n, i], want[n, i] = F((jf[n, i] + 0.5) * float(s_a)), jf[n, i] + 1      # exact ties round away from zero
        i = take((jf[n] <= 0) & (jf[n] > qmin))
        xf[n, i], want[n, i] = F((jf[n, i] - 0.5) * float(s_a)), jf[n, i] - 1
    jx = code_of(x, s_a, case["in_bits"]).astype(np.int64)
    over = want != 1 << 20
    assert np.array_equal(jx[~over.reshape(j.shape)], j[~over.reshape(j.shape)]), "away from the overridden elements the image gives the case's codes"
    assert np.array_equal(jx.reshape(N, -1)[over], want[over]), "ties round away from zero, values outside the range clamp, -0.0 is the code 0"
    assert over.sum() == (N if case["extreme"] else 5 * N)
    return x, jx


def first_judge(case, jx):
    """(codes, the case as the judge saw it): the exact convolution of the codes read back from the image, then the un-pooled chain."""
    acc = O.conv2d_fwd(jx, case["k"], None, padding=case["KS"] // 2, groups=1, acc=np.int64)
    assert np.abs(acc).max() < 2 ** 31
    seen = dict(case, j=jx.astype(np.int8), acc=acc)
    return chain_codes(acc, case["al"], case["b"], case["s_out"], case["s_out"], case["a_bits"], 0), seen


# ---------------------------------------------------------------------------------------------- through the ABI
def first_geom(be, case):
    return be.geom(case["j"].shape, case["w"].shape, padding=case["KS"] // 2)


def pack_first(be, g, case, order=None, w=None, b=None, s_out=None):
    bits = (case["in_bits"], case["a_bits"], case["w_bits"])
    nb = int(be.lib.mn_i8first_table_bytes(C.byref(g), *bits))
    assert nb > 0 and nb % 16 == 0
    table = _empty_i32(be, (nb // 4,))
    dO = _dev_i32(be, np.asarray(order, dtype=np.int32)) if order is not None else None
    dW, dS, dB = be.to_dev(case["w"] if w is None else w), be.to_dev(case["s_w"]), be.to_dev(case["b"] if b is None else b)
    be.call("mn_i8first_pack", C.byref(g), be.ptr(dW), be.ptr(dS), 1 if case["per_channel"] else 0, be.ptr(dB), C.c_float(float(case["s_a"])),
            C.c_float(float(case["s_out"] if s_out is None else s_out)), *bits, be.ptr(dO), be.ptr(table), be.stream)
    return table


def run_first(be, case, x, order, table=None):
    """Pack the table, run mn_i8first_fwd TWICE into poisoned buffers; returns (codes [N, OB * 16, H, W] as the positions hold them, kernel name)."""
    g = first_geom(be, case)
    bits = (case["in_bits"], case["a_bits"], case["w_bits"])
    assert be.lib.mn_i8first_supported(C.byref(g), *bits) == 1
    if table is None:
        table = pack_first(be, g, case, order)
        hdr = _host_u32(be, table)
        assert int(hdr[0]) == 0 and int(hdr[7]) == 0, "finite constants, weights on the grid, a valid order: %d %d" % (int(hdr[0]), int(hdr[7]))
        assert int(hdr[6]) == (case["a_bits"] | case["w_bits"] << 8 | case["in_bits"] << 16)
    N, _, H, W = x.shape
    OB = (case["w"].shape[0] + 15) // 16
    dx = be.to_dev(x)
    outs = []
    for _ in range(2):
        yb = be.empty_i8((N, OB, H * W, 16))          # poisoned
        be.call("mn_i8first_fwd", C.byref(g), *bits, be.ptr(table), be.ptr(dx), be.ptr(yb), be.stream)
        outs.append(be.to_host(yb))
    name = be.lib.mn_last_kernel().decode()
    assert np.array_equal(outs[0], outs[1]), "two runs give identical bytes"
    return np_unblock(outs[0], OB * 16, H, W), name


def _check_first(be, case, shuffle, seed, what, hard):
    x, jx = make_image(case, seed)
    ref, seen = first_judge(case, jx)
    if hard:
        assert_case_is_hard(seen)
    Oc = case["w"].shape[0]
    order = shuffle_order(Oc, shuffle) if shuffle else None
    got, name = run_first(be, case, x, order)
    want = expect_positions(ref, order, (Oc + 15) // 16)
    bad = int((got != want).sum())
    print(name, what, "mismatches against the judge", bad, "of", got.size, "distinct codes", len(np.unique(ref)))
    assert name == "k_i8first<%d>" % case["KS"], name
    assert got.shape == want.shape and bad == 0, (bad, got.size)
    return ref


def check_first(be, idx):
    name, x_shape, Oc, KS, shuffle = FIRST[idx]
    special = name not in NOT_SPECIAL
    case = first_case(x_shape, Oc, KS, 5200 + idx, special=special)
    _check_first(be, case, shuffle, 5200 + idx, "%s %s -> %d k%d shuffle %d" % (name, x_shape, Oc, KS, shuffle), special)


def check_first_chain(be, idx):
    name, widths, per_channel, in_bits = FIRST_CHAINS[idx]
    _, x_shape, Oc, KS, shuffle = FIRST[0]
    seed = 5400 + idx
    case = first_case(x_shape, Oc, KS, seed, widths=widths, per_channel=per_channel, out_bits=4 if name == "in8_out4" else None)
    assert case["in_bits"] == in_bits
    ref = _check_first(be, case, shuffle, seed, name, case["a_bits"] == 8)
    if case["a_bits"] == 4:
        assert len(np.unique(ref)) == 8, "all non-negative 4-bit codes"


def check_first_extreme(be):
    _, x_shape, Oc, KS, shuffle = FIRST[0]
    case = first_case(x_shape, Oc, KS, 5500, extreme=True)
    assert int(np.abs(case["acc"]).max()) == 128 * 127 * 75 and int(case["acc"].min()) == -128 * 127 * 75
    ref = _check_first(be, case, shuffle, 5500, "first_extreme", False)
    assert len(np.unique(ref)) >= 2


def run_last(be, case, order, relu, guard=64):
    """mn_i8conv_pack with s_p = s_out = 1, then mn_i8conv_fwd_f32 TWICE into poisoned buffers with a guard region behind [N][O][H*W]."""
    g = geom_of(be, case)
    assert be.lib.mn_i8conv_supported(C.byref(g), case["a_bits"], case["w_bits"]) == 1
    table = pack_table(be, g, case, order, s_p=1.0, s_out=1.0)
    hdr = _host_u32(be, table)
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0
    xb = be.to_dev_i8(np_block(case["j"]))
    N, _, H, W = case["j"].shape
    Oc = case["w"].shape[0]
    outs = []
    for _ in range(2):
        y = be.empty((N * Oc * H * W + guard,))          # poisoned
        be.call("mn_i8conv_fwd_f32", C.byref(g), case["a_bits"], case["w_bits"], be.ptr(table), be.ptr(xb), be.ptr(y), relu, be.stream)
        outs.append(be.to_host(y))
    name = be.lib.mn_last_kernel().decode()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "two runs give identical values"
    assert (outs[0][N * Oc * H * W:] == F(-1234.5)).all(), "the guard region keeps its poison"
    return outs[0][:N * Oc * H * W].reshape(N, Oc, H, W), name


def _check_last(be, case, order, what, hard):
    if hard:
        assert_case_is_hard(case)
    for relu in (0, 1):
        r = chain_r(case["acc"], case["al"], case["b"], relu)
        if case["tie"] and r.shape[1] >= 3:
            assert (r[:, 1] < 0).all() if relu == 0 else (r[:, 1] == 0).all(), "the channel the ReLU zeroes keeps its negative values without it"
        want = r[:, order] if order is not None else r
        got, name = run_last(be, case, order, relu)
        bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print(name, what, "relu", relu, "words that differ from the judge", bad, "of", got.size)
        assert name == "k_i8conv_f32<%d>" % case["KS"], name
        assert bad == 0, (bad, got.size)


def check_last(be, idx):
    name, x_shape, Oc, KS, groups = LAST[idx]
    case = make_case(x_shape, Oc, KS, groups, 5300 + idx)
    _check_last(be, case, None, "%s %s -> %d k%d" % (name, x_shape, Oc, KS), Oc >= 3 and case["acc"].size >= 640)


def check_last_chain(be, idx):
    name, widths, per_channel, ordered = LAST_CHAINS[idx]
    _, x_shape, Oc, KS, groups = LAST[1]
    case = make_case(x_shape, Oc, KS, groups, 5600 + idx, widths=widths, per_channel=per_channel)
    order = np.random.default_rng(5600 + idx).permutation(Oc) if ordered else None
    _check_last(be, case, order, name, widths[1] == 8)


# ---------------------------------------------------------------------------------------------- several sets per block (tests/deploy_grid.py, iao8_cases.LARGE_GRID)
# (id, x shape, O, KS, out_order shuffle): seed 5800 + index.  k_i8first gives every image ceil(H W / 256) blocks, so 8 x 8 images keep the judge cheap.  GPU only
# (tests/test_gpu_iao8_ends.py): 31 s, 40 s and 71 s on the CPU emulation build (8 cores).
LARGE_FIRST = [
    ("f5_five_sets", (700, 3, 8, 8), 312, 5, 4),               # bx 700, 5 sets: blocks of 2, 2, 1; the last output block half empty
    ("f5_last_set_second", (1024, 3, 8, 8), 312, 5, 0),        # bx 1024: blocks of 3 and 2 -- the last set, with positions past O, is the second of its block
    ("f5_four_waves", (512, 3, 16, 16), 320, 5, 2),            # bx 512: blocks of 2, 2, 1; 256 pixels per image, so all four waves of a block have pixels (one at 8 x 8)
]
# (id, x shape, O, KS, groups): seed 5900 + index; a random out_order.  GPU only: 78 s on the CPU emulation build.
LARGE_LAST = [
    ("l1_five_sets", (130, 16, 32, 32), 312, 1, 1),            # bx 520, 5 sets: blocks of 2, 2, 1; O % 16 != 0
]


def check_large_first(be, idx):
    import deploy_grid as DG
    from iao8_cases import LARGE_HEAD
    name, x_shape, Oc, KS, shuffle = LARGE_FIRST[idx]
    seed = 5800 + idx
    N, Cc, H, W = x_shape
    head = first_case((LARGE_HEAD, Cc, H, W), Oc, KS, seed)
    qmin, qmax = (int(v) for v in qrange(head["in_bits"]))
    more = np.random.default_rng(seed + 500).integers(qmin, qmax + 1, size=(N - LARGE_HEAD, Cc, H, W)).astype(np.int8)
    more[:, :, 0, 0] = 0          # (make_case's whole-zero pixel: make_image puts its -0.0 on a zero code)
    case = dict(head, j=np.concatenate([head["j"], more]))
    x, jx = make_image(case, seed)
    OB = (Oc + 15) // 16
    nsets = (OB + 3) // 4
    gy, per = DG.assert_uneven_deal(be, N * DG.pixel_blocks(H * W, 256), nsets)
    if "last_set_second" in name:
        assert nsets - (gy - 1) * per >= 2 and Oc % 64, "the last block takes two sets at least, and the last of them has positions past O"
    order = shuffle_order(Oc, shuffle) if shuffle else None
    got, kname = run_first(be, case, x, order)
    assert kname == "k_i8first<%d>" % KS, kname
    bad = 0
    for n0 in range(0, N, LARGE_HEAD):
        acc = DG.exact_conv(jx[n0:n0 + LARGE_HEAD], head["k"], KS // 2, 1)
        assert np.abs(acc).max() < 2 ** 31
        if n0 == 0:
            assert_case_is_hard(dict(head, j=jx[:LARGE_HEAD].astype(np.int8), acc=acc))
        ref = chain_codes(acc, head["al"], head["b"], head["s_out"], head["s_out"], head["a_bits"], 0)
        bad += int((got[n0:n0 + ref.shape[0]] != expect_positions(ref, order, OB)).sum())
    print(kname, name, x_shape, "->", Oc, "grid.y", gy, "per", per, "mismatches against the judge", bad, "of", got.size)
    assert bad == 0, (bad, got.size)


def check_large_last(be, idx):
    import deploy_grid as DG
    from iao8_cases import LARGE_HEAD, large_case
    name, x_shape, Oc, KS, groups = LARGE_LAST[idx]
    seed = 5900 + idx
    head, j = large_case(x_shape, Oc, KS, groups, seed)
    case = dict(head, j=j)
    N, _, H, W = x_shape
    gy, per = DG.assert_uneven_deal(be, DG.pixel_blocks(N * H * W, 256), ((Oc + 15) // 16 + 3) // 4)
    order = np.random.default_rng(seed).permutation(Oc)
    for relu in (0, 1):
        got, kname = run_last(be, case, order, relu)
        assert kname == "k_i8conv_f32<%d>" % KS, kname
        bad = 0
        for n0 in range(0, N, LARGE_HEAD):
            acc = DG.exact_conv(j[n0:n0 + LARGE_HEAD], head["k"], KS // 2, groups)
            assert np.abs(acc).max() < 2 ** 31
            want = chain_r(acc, head["al"], head["b"], relu)[:, order]
            bad += int((got[n0:n0 + want.shape[0]].view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).sum())
        print(kname, name, x_shape, "->", Oc, "relu", relu, "grid.y", gy, "per", per, "words that differ from the judge", bad, "of", got.size)
        assert bad == 0, (bad, got.size)


def check_vs_torch(kind, idx, widths):
    """The cap of the GPU cross-check holds for the judge itself at the geometries above: against the parent's fp32 arithmetic at most one step, on at most 1e-4 of
    the elements (CPU only)."""
    if kind == "first":
        name, x_shape, Oc, KS, _ = FIRST[idx]
        case = make_case(x_shape, Oc, KS, 1, 5200 + idx, widths=widths, special=False)
    else:
        name, x_shape, Oc, KS, groups = LAST[idx]
        case = make_case(x_shape, Oc, KS, groups, 5300 + idx, widths=widths, special=False)
    ref, par = judge(case, 0).astype(np.int32), torch_codes(case, 0).astype(np.int32)
    d = np.abs(ref - par)
    print(name, widths, "flips against the fp32 path", int((d != 0).sum()), "of", d.size, "largest", int(d.max()))
    assert d.max() <= 1 and (d != 0).mean() <= 1e-4


# ---------------------------------------------------------------------------------------------- refusals, counters
def check_first_refused(be, idx):
    kw, bits = FIRST_REFUSED[idx]
    g = be.geom(kw["x_shape"], kw["w_shape"], stride=kw.get("stride", 1), padding=kw.get("padding", 0), dilation=kw.get("dilation", 1), groups=kw.get("groups", 1))
    g.in_shuffle = kw.get("in_shuffle", 0)
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.ones(64, dtype=F))
    one = C.c_float(1.0)
    ENOTSUP = _lib().MN_ENOTSUP
    assert be.lib.mn_i8first_supported(C.byref(g), *bits) == 0
    assert int(be.lib.mn_i8first_table_bytes(C.byref(g), *bits)) == 0
    assert be.lib.mn_i8first_pack(C.byref(g), be.ptr(f), be.ptr(f), 1, be.ptr(f), one, one, *bits, None, be.ptr(buf), be.stream) == ENOTSUP
    assert "not covered" in be.lib.mn_last_error().decode()
    assert be.lib.mn_i8first_fwd(C.byref(g), *bits, be.ptr(buf), be.ptr(f), be.ptr(buf), be.stream) == ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all() and (be.to_host(f) == 1).all(), "a refused call writes nothing"


def check_invalid(be):
    """Null, misaligned, N <= 0 and relu = 2 are MN_EINVAL and write nothing."""
    L = _lib()
    lib, s = be.lib, be.stream
    buf = _empty_i32(be, (64,))
    f = be.to_dev(np.ones(64, dtype=F))
    one = C.c_float(1.0)
    odd = C.c_void_p(be.ptr(buf).value + 4)
    oddf = C.c_void_p(be.ptr(f).value + 2)
    g = be.geom((1, 3, 8, 8), (16, 3, 5, 5), padding=2)
    assert lib.mn_i8first_supported(C.byref(g), 8, 8, 8) == 1
    b, p = be.ptr(buf), be.ptr(f)
    for args in ((None, p, 1, p, one, one, 8, 8, 8, None, b), (p, None, 1, p, one, one, 8, 8, 8, None, b), (p, p, 1, p, one, one, 8, 8, 8, None, None),
                 (p, p, 1, p, one, one, 8, 8, 8, None, odd), (p, p, 2, p, one, one, 8, 8, 8, None, b), (oddf, p, 1, p, one, one, 8, 8, 8, None, b)):
        assert lib.mn_i8first_pack(C.byref(g), *args, s) == L.MN_EINVAL, args
    for args in ((None, p, b), (b, None, b), (b, p, None), (odd, p, b), (b, oddf, b), (b, p, odd)):
        assert lib.mn_i8first_fwd(C.byref(g), 8, 8, 8, *args, s) == L.MN_EINVAL, args
    g0 = be.geom((0, 3, 8, 8), (16, 3, 5, 5), padding=2)
    assert lib.mn_i8first_supported(C.byref(g0), 8, 8, 8) == 0 and int(lib.mn_i8first_table_bytes(C.byref(g0), 8, 8, 8)) == 0
    assert lib.mn_i8first_pack(C.byref(g0), p, p, 1, p, one, one, 8, 8, 8, None, b, s) == L.MN_EINVAL
    assert lib.mn_i8first_fwd(C.byref(g0), 8, 8, 8, b, p, b, s) == L.MN_EINVAL
    gl = be.geom((1, 32, 8, 8), (32, 32, 1, 1))
    for args in ((None, b, p, 1), (b, None, p, 1), (b, b, None, 1), (odd, b, p, 1), (b, odd, p, 1), (b, b, oddf, 1), (b, b, p, 2), (b, b, p, -1)):
        assert lib.mn_i8conv_fwd_f32(C.byref(gl), 8, 8, *args, s) == L.MN_EINVAL, args
    gl0 = be.geom((0, 32, 8, 8), (32, 32, 1, 1))
    assert lib.mn_i8conv_fwd_f32(C.byref(gl0), 8, 8, b, b, p, 1, s) == L.MN_EINVAL
    g5 = be.geom((1, 32, 8, 8), (32, 32, 5, 5), padding=2)
    assert lib.mn_i8conv_fwd_f32(C.byref(g5), 8, 8, b, b, p, 1, s) == L.MN_ENOTSUP
    assert lib.mn_i8conv_fwd_f32(C.byref(gl), 9, 8, b, b, p, 1, s) == L.MN_ENOTSUP
    assert (_host_u32(be, buf) == 0x5a5a5a5a).all() and (be.to_host(f) == 1).all()


def check_first_counters(be, seed=5700):
    """Word 0 counts a non-finite bias and s_out <= 0, word 7 a weight half a step off the grid and a bad out_order entry, whose position yields 0 bytes."""
    case = first_case((1, 3, 6, 6), 32, 5, seed)
    g = first_geom(be, case)
    hdr = _host_u32(be, pack_first(be, g, case))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 0
    assert (int(hdr[1]), int(hdr[4]), int(hdr[5])) == (2, 1, 75) and int(hdr[6]) == (8 | 8 << 8 | 8 << 16)
    assert hdr[9:15].view(F).tolist() == [case["s_out"], F(-128), F(127), case["s_a"], F(-128), F(127)]
    b = case["b"].copy()
    b[9] = F(np.inf)
    hdr = _host_u32(be, pack_first(be, g, case, b=b))
    assert int(hdr[0]) == 1 and int(hdr[7]) == 0
    for s_out in (0.0, -1.0, np.nan):
        hdr = _host_u32(be, pack_first(be, g, case, s_out=s_out))
        assert int(hdr[0]) >= 1 and int(hdr[7]) == 0, s_out
    w2 = case["w"].copy()
    w2[5, 1, 3, 4] += F(0.5) * case["s_w"][5]
    hdr = _host_u32(be, pack_first(be, g, case, w=w2))
    assert int(hdr[0]) == 0 and int(hdr[7]) == 1
    order = np.arange(32)
    order[3] = -1
    table = pack_first(be, g, case, order)
    assert int(_host_u32(be, table)[7]) == 1
    x, jx = make_image(case, seed)
    ref, _ = first_judge(case, jx)
    ref[:, 3] = 0
    got, _ = run_first(be, case, x, None, table=table)
    assert np.array_equal(got, ref)
