"""Direct oracle checks of the IAO streaming kernels at kernel-sized inputs, shared by the CPU-emulation run (tests/test_iao_stream_emulated.py) and the MI355X run
(tests/test_gpu_iao_stream.py): the observer (mn_iao_observe, mn_iao_qparams, mn_iao_union_range), the fake-quantizer (mn_iao_fq_fwd / _bwd), the fused activation
and average-pool kernels of csrc/iao_ops.hip, the generic map kernels (k_map1 / k_map2) and the histogram observer through the C ABI.

Every check drives the ABI through ``abi_driver.Backend`` and compares with ``oracle/np_oracle.py`` plus plain numpy evaluated in the kernels' fp32 step order.
Everything is generated from seeds.  Comparisons are exact (``eq``: equal values, NaN where the reference has NaN) except the two the kernels cannot make exact:
the sigmoid (device expf against fp64 exp: <= 1e-6 of max|ref|, the bound of tests/test_gpu_iao_ops.py) and the global average (fp64 accumulation rounded once:
<= 1 fp32 ulp of the fp64 mean rounded once).

Sizes come from the launch code:
  * k_map1 / k_map2 (launch_map1/2), k_iao_fq_* with rows == 1 (fq_grid) and k_fq_act_* cap the grid at EW_GRID_CAP = 2048 blocks of 256 lanes: one float4
    sweep covers 2048 * 256 * 4 elements, one sweep of the scalar path (a pointer that is not 16-byte aligned) 2048 * 256;
  * mn_iao_observe with rows == 1 gives a block 1024 float4 and caps at OBS_NB = 1024 blocks: above 1024 * 1024 * 4 elements the grid stops growing; one
    grid-stride step of that grid covers 1024 * 256 float4 (1024 * 256 elements on the scalar path);
  * k_fq_avgpool_fwd / _bwd cap at 4096 blocks of 256 lanes, one output (fwd) or input (bwd) element per lane.
"""
import ctypes as C

import numpy as np

from kernel_cases import eq
from oracle import np_oracle as O

F = np.float32
POISON = F(-1234.5)

EW_SWEEP_VEC = 2048 * 256 * 4          # EW_GRID_CAP blocks x 256 lanes x float4 = 2,097,152 elements
EW_SWEEP_SCALAR = 2048 * 256           # the same grid on the scalar path = 524,288 elements
OBS_CAP = 1024 * 1024 * 4              # OBS_NB blocks of 1024 float4 = 4,194,304 elements: the largest tensor that gets a block per 1024 float4
OBS_STEP_VEC = 1024 * 256 * 4          # one grid-stride step of OBS_NB blocks x 256 lanes x float4 = 1,048,576 elements
OBS_STEP_SCALAR = 1024 * 256           # ... on the scalar path = 262,144 elements
POOL_CAP = 4096 * 256                  # avgpool grid cap x 256 lanes = 1,048,576 outputs (fwd) / inputs (bwd)
TAIL = 4 * 256 * 3 + 3                 # three more blocks of float4 (a partial last sweep) and a 3-element tail
N_EW = EW_SWEEP_VEC + TAIL             # size (a) of the element-wise families: 2,100,227
N_OBS = OBS_CAP + TAIL                 # size (a) of the flat observer: 4,197,379
SMALL = (1, 3, 5, 255, 257, 1027)      # sizes (c): around the float4 width (4) and the block width (256); 1027 = one block of float4 + a 3-element tail

MOMENTUM = 0.1
RANGE = (F(-1.37), F(2.91))            # the observed range the fake-quant checks take their (scale, zero point) from
SLOPE = F(0.1)


# ----------------------------------------------------------------------------- buffers
class Buf:
    """n floats on the device with poisoned guard elements on both sides; ``mis``: the view starts 4 bytes past a 16-byte boundary (size (b): scalar path)."""

    def __init__(self, be, n, mis=False, data=None):
        self.be, self.n, self.off = be, int(n), 5 if mis else 4
        h = np.full(self.n + 12, POISON, dtype=F)
        if data is not None:
            h[self.off:self.off + self.n] = np.asarray(data, dtype=F).reshape(-1)
        self.dev = be.to_dev(h)
        self.ptr = be.ptr_at(self.dev, self.off)
        assert (self.ptr.value % 16 != 0) == bool(mis)

    def get(self):
        h = self.be.to_host(self.dev).reshape(-1)
        assert np.all(h[:self.off] == POISON) and np.all(h[self.off + self.n:] == POISON), "wrote outside the output"
        return h[self.off:self.off + self.n]


def _rng(*key):
    return np.random.default_rng(list(key))


def _grad(r, shape):
    """gradients bounded away from zero, so that a clip-STE that zeroes (or fails to zero) an element always shows"""
    return (r.uniform(0.5, 1.5, shape) * r.choice([-1.0, 1.0], shape)).astype(F)


def qp_host(mn, mx, bits, q_type, is_act, scale=None, zp=None):
    """(scale, zp, qp) as iao_qparams_row (csrc/common.h) defines them: O.iao_qparams, or the given (scale, zp) for update == 0, and the clip-STE bounds
    lo = min / scale - zp, hi = max / scale - zp (symmetric: hi = max(|lo|, |hi|), lo = -hi) -- the expressions of O.iao_fq_bwd."""
    mn, mx = np.asarray(mn, dtype=F).reshape(-1), np.asarray(mx, dtype=F).reshape(-1)
    with np.errstate(all="ignore"):
        if scale is None:
            scale, zp = O.iao_qparams(mn, mx, bits, q_type, is_act)
        scale, zp = np.asarray(scale, dtype=F).reshape(-1), np.asarray(zp, dtype=F).reshape(-1)
        lo, hi = (mn / scale - zp).astype(F), (mx / scale - zp).astype(F)
        if q_type == 0:
            hi = np.maximum(np.abs(lo), np.abs(hi))
            lo = -hi
    return scale, zp, np.stack([scale, zp, lo, hi], axis=1).astype(F)


# ----------------------------------------------------------------------------- 1. observer
OLD_RANGE = (F(-0.75), F(1.25))        # the observer's buffers before a first == 0 call
OBS_COMBOS = ((0, 1), (1, 1), (0, 0), (1, 0))      # (obs_kind, first)


def check_qparams(be, mn, mx):
    """mn_iao_qparams on an observed range against O.iao_qparams: update 1 / 0, symmetric / asymmetric, 2 / 4 / 8 / 16 bits, weight / activation ranges; scale,
    zero point and all four qp words exact."""
    rows = mn.size
    dmn, dmx = be.to_dev(mn), be.to_dev(mx)
    for bits in (2, 4, 8, 16):
        for q_type in (0, 1):
            for is_act in (0, 1):
                for update in (1, 0):
                    sc0, zp0 = np.full(rows, 0.037, dtype=F), np.full(rows, 3.0 if q_type else 0.0, dtype=F)
                    sc, zp, qp = be.to_dev(sc0), be.to_dev(zp0), be.empty((rows, 4))
                    be.call("mn_iao_qparams", be.ptr(dmn), be.ptr(dmx), rows, bits, q_type, is_act, update, be.ptr(sc), be.ptr(zp), be.ptr(qp), be.stream)
                    rsc, rzp, rqp = qp_host(mn, mx, bits, q_type, is_act) if update else qp_host(mn, mx, bits, q_type, is_act, sc0, zp0)
                    what = (bits, q_type, is_act, update)
                    assert eq(be.to_host(sc).reshape(-1), rsc), ("scale",) + what
                    assert eq(be.to_host(zp).reshape(-1), rzp), ("zero point",) + what
                    assert eq(be.to_host(qp).reshape(rows, 4), rqp), ("qp",) + what


def check_union(be, a, b):
    """mn_iao_union_range of two observed (min, max) pairs: NaN-propagating min / max, as torch.min / torch.max of the reference's QuantAdd"""
    d = [be.to_dev(np.asarray(v, dtype=F).reshape(1)) for v in (a[0], a[1], b[0], b[1])]
    lo, hi = be.empty(1), be.empty(1)
    be.call("mn_iao_union_range", be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), be.ptr(d[3]), be.ptr(lo), be.ptr(hi), be.stream)
    assert eq(be.to_host(lo), np.minimum(F(a[0]), F(b[0])).reshape(1)) and eq(be.to_host(hi), np.maximum(F(a[1]), F(b[1])).reshape(1)), (a, b)


def observe_run(be, x, rows, cols, mis, obs_kind, first):
    """One mn_iao_observe call on x viewed as [rows][cols] against O.observe + O.observer_update, then mn_iao_qparams on the result.  -> (min, max)"""
    xb = Buf(be, rows * cols, mis, x)
    mn, mx = be.to_dev(np.full(rows, OLD_RANGE[0], dtype=F)), be.to_dev(np.full(rows, OLD_RANGE[1], dtype=F))
    ws = be.empty(max(4, int(be.lib.mn_iao_observe_ws_floats(rows, cols))))
    be.call("mn_iao_observe", xb.ptr, rows, cols, obs_kind, first, MOMENTUM, be.ptr(mn), be.ptr(mx), be.ptr(ws), be.stream)
    x2 = np.asarray(x, dtype=F).reshape(rows, cols)
    with np.errstate(all="ignore"):
        cmin, cmax = O.observe(x2, "L" if rows == 1 else "FC")
        rmin, rmax = O.observer_update("minmax" if obs_kind == 0 else "ema", first, np.full(rows, OLD_RANGE[0], dtype=F), np.full(rows, OLD_RANGE[1], dtype=F),
                                       cmin.reshape(-1), cmax.reshape(-1), MOMENTUM)
    gmin, gmax = be.to_host(mn).reshape(-1), be.to_host(mx).reshape(-1)
    assert eq(gmin, rmin), ("min", rows, cols, mis, obs_kind, first, gmin[:4], rmin[:4])
    assert eq(gmax, rmax), ("max", rows, cols, mis, obs_kind, first, gmax[:4], rmax[:4])
    check_qparams(be, rmin, rmax)
    return rmin, rmax


_base = {}


def _base_data(n):
    if n not in _base:
        _base[n] = _rng(11, n).standard_normal(n).astype(F)        # |x| < 7: the planted -50 / +60 are the global extremes
    return _base[n]


def _planted(n, min_pos, max_pos):
    x = _base_data(n).copy()
    x[max_pos] = F(60.0)
    x[min_pos] = F(-50.0)                   # (n == 1: one element, minimum == maximum)
    return x


def _flat_positions(n, mis):
    """element 0, the last tail element, the last element of the first sweep and the first of the second -- the sweep being both the grid-stride step of the
    launched grid and, on the float4 path, the 1024 x 1024 float4 at which the grid stops growing"""
    step = OBS_STEP_SCALAR if mis else OBS_STEP_VEC
    p = [0, n - 1, step - 1, step] + ([] if mis else [OBS_CAP - 1, OBS_CAP])
    return [v for v in p if 0 <= v < n]


def _flat_runs(n, mis):
    """run i: the minimum at position i, the maximum at position i + 1 (cyclic) of the first four positions, so that each of them holds the minimum in one run and
    the maximum in another; the runs go through the four (obs_kind, first) combinations.  The float4 path adds one run for its second pair of positions."""
    p = _flat_positions(n, mis)
    pairs = [(p[i], p[(i + 1) % 4]) for i in range(4)] + ([(p[4], p[5])] if len(p) == 6 else [])
    return [dict(n=n, mis=mis, min_pos=a, max_pos=b, obs_kind=OBS_COMBOS[i % 4][0], first=OBS_COMBOS[i % 4][1]) for i, (a, b) in enumerate(pairs)]


# sizes (a) and (b) of the flat observer, one planted run per case (a run costs the emulator several seconds: 1024 blocks through two block reductions)
OBSERVE_FLAT_BIG = _flat_runs(N_OBS, False) + _flat_runs(N_OBS, True)


def check_observe_flat(be, n, mis, min_pos, max_pos, obs_kind, first):
    a = observe_run(be, _planted(n, min_pos, max_pos), 1, n, mis, obs_kind, first)
    check_union(be, (a[0][0], a[1][0]), (F(-3.5), F(77.0)))
    check_union(be, (F(-80.0), F(0.25)), (a[0][0], a[1][0]))


def check_observe_flat_small(be):
    """sizes (c), aligned and through the offset pointer, every (obs_kind, first), the extremes on the first and the last element in turn"""
    for n in SMALL:
        for mis in (False, True):
            for obs_kind, first in OBS_COMBOS:
                check_observe_flat(be, n, mis, 0, n - 1, obs_kind, first)
                check_observe_flat(be, n, mis, n - 1, 0, obs_kind, first)


OBSERVE_SPECIAL_N = (1027, 5 * 4096 + 3)   # one block + tail; six blocks (a second stage over several partials) + tail


def check_observe_special(be, n, mis):
    """NaN in the tail (the range becomes NaN, as torch.min / max give), +inf and -inf, and a constant-zero tensor, whose scale clamps to eps"""
    x = _base_data(n).copy()
    x[n - 2] = np.nan
    nan_range = observe_run(be, x, 1, n, mis, 0, 1)
    assert np.isnan(nan_range[0][0]) and np.isnan(nan_range[1][0])
    observe_run(be, x, 1, n, mis, 1, 0)
    x = _base_data(n).copy()
    x[1], x[n - 1] = np.inf, -np.inf
    inf_range = observe_run(be, x, 1, n, mis, 0, 0)
    assert inf_range[0][0] == -np.inf and inf_range[1][0] == np.inf
    observe_run(be, x, 1, n, mis, 1, 1)
    zero_range = observe_run(be, np.zeros(n, dtype=F), 1, n, mis, 1, 1)
    for q_type in (0, 1):
        assert qp_host(zero_range[0], zero_range[1], 8, q_type, 1)[0][0] == O.EPS32
    check_union(be, (nan_range[0][0], nan_range[1][0]), (inf_range[0][0], inf_range[1][0]))
    check_union(be, (inf_range[0][0], inf_range[1][0]), (zero_range[0][0], zero_range[1][0]))


# rows > 1 (k_minmax_rows, a block per row): the (obs_kind, first) combinations each shape runs.  The two shapes with a thousand blocks and more take one
# combination each (the update is the same device function for every shape); together the table holds all four.
OBSERVE_ROWS = [dict(rows=1024, cols=128, combos=((0, 0),)), dict(rows=10, cols=1024, combos=OBS_COMBOS), dict(rows=256, cols=75, combos=((1, 1), (0, 0))),
                dict(rows=2100, cols=4, combos=((1, 0),)), dict(rows=3, cols=1, combos=OBS_COMBOS)]


def check_observe_rows(be, rows, cols, combos):
    """per-row ranges; the extremes of the tensor in the last column of the last row, one NaN row and one row holding both infinities (rows permitting)"""
    x = (_rng(12, rows, cols).standard_normal((rows, cols)) * (1.0 + np.arange(rows)[:, None] % 5)).astype(F)
    for i, (obs_kind, first) in enumerate(combos):
        x[rows - 1, cols - 1] = F(60.0) if i % 2 == 0 else F(-50.0)
        if rows >= 10:
            x[4, cols - 1], x[7, 0], x[7, cols - 1] = np.nan, np.inf, -np.inf
        observe_run(be, x, rows, cols, False, obs_kind, first)


# ----------------------------------------------------------------------------- 2. fake-quant
def _flat_qp(bits, q_type, is_act=1):
    return qp_host([RANGE[0]], [RANGE[1]], bits, q_type, is_act)


def run_fq(be, x, g, rows, cols, qp, bits, q_type, is_act, mis):
    xb, gb, qpd = Buf(be, rows * cols, mis, x), Buf(be, rows * cols, mis, g), be.to_dev(qp)
    y, dx = Buf(be, rows * cols, mis), Buf(be, rows * cols, mis)
    be.call("mn_iao_fq_fwd", xb.ptr, y.ptr, rows, cols, be.ptr(qpd), bits, q_type, is_act, be.stream)
    be.call("mn_iao_fq_bwd", gb.ptr, xb.ptr, dx.ptr, rows, cols, be.ptr(qpd), bits, q_type, is_act, be.stream)
    return y.get(), dx.get()


def check_fq_flat(be, n, mis, bits, q_type):
    """rows == 1 at one size: data that overshoots the observed range on both sides"""
    r = _rng(21, n, bits, q_type)
    x, g = (r.standard_normal(n) * 2).astype(F), _grad(r, n)
    sc, zp, qp = _flat_qp(bits, q_type)
    y, dx = run_fq(be, x, g, 1, n, qp, bits, q_type, 1, mis)
    assert eq(y, O.iao_fq_fwd(x, sc[0], zp[0], bits, q_type, 1)[0]), ("fwd", n, mis)
    assert eq(dx, O.iao_fq_bwd(g, x, sc[0], zp[0], RANGE[0], RANGE[1], bits, q_type, 1)), ("bwd", n, mis)


def check_fq_flat_small(be):
    for i, n in enumerate(SMALL):
        for mis in (False, True):
            check_fq_flat(be, n, mis, (2, 4, 8, 16)[i % 4], i % 2)


# rows > 1: (1024, 128) float4, a block per row; (256, 75) cols % 4 != 0 -> scalar path; (2100, 4) more rows than EW_GRID_CAP = 2048 -> the gridDim.y row
# loop; (3, 2048 * 1024 + 4) a row wider than one float4 sweep -> per_row == EW_GRID_CAP, gridDim.y == 1, the row loop and the column stride loop together
FQ_ROWS = [dict(rows=1024, cols=128, bits=4, q_type=0), dict(rows=256, cols=75, bits=8, q_type=1), dict(rows=2100, cols=4, bits=8, q_type=0),
           dict(rows=3, cols=2048 * 1024 + 4, bits=4, q_type=1)]


def check_fq_rows(be, rows, cols, bits, q_type):
    """per-row (weight) quantizers whose ranges differ by a factor of 100 and more between neighbouring rows: a slip in the row index changes every value"""
    r = _rng(22, rows, cols)
    mag = (10.0 ** ((np.arange(rows) * 5) % 7 - 3)).astype(np.float64)
    mn, mx = (RANGE[0] * mag).astype(F), (RANGE[1] * mag).astype(F)
    sc, zp, qp = qp_host(mn, mx, bits, q_type, 0)
    x, g = (r.standard_normal((rows, cols)) * 2 * mag[:, None]).astype(F), _grad(r, (rows, cols))
    y, dx = run_fq(be, x, g, rows, cols, qp, bits, q_type, 0, False)
    col = lambda v: v.reshape(-1, 1)
    assert eq(y.reshape(rows, cols), O.iao_fq_fwd(x, col(sc), col(zp), bits, q_type, 0)[0]), "fwd"
    assert eq(dx.reshape(rows, cols), O.iao_fq_bwd(g, x, col(sc), col(zp), col(mn), col(mx), bits, q_type, 0)), "bwd"


BOUNDARY = [(bits, q_type) for bits in (2, 4, 8, 16) for q_type in (0, 1)]
# mn_iao_fq_* also with the weight code range: there alone does the symmetric quantizer keep v == hi inside the clamp (rha(hi) == qmax; with the activation
# range hi = qmax + 0.5 rounds past qmax and the clamp's own mask hides what the clip-STE decides at its bound)
FQ_BOUNDARY = [(bits, q_type, is_act) for bits, q_type in BOUNDARY for is_act in (1, 0)]


def boundary_set(bits, q_type, is_act=1):
    """Inputs on the decision boundaries of the quantizer made by O.iao_qparams from RANGE: every rounding boundary x = fl32((k + 0.5 + zp) * scale), k in
    [qmin - 2, qmax + 1] (past both clamp ends) with both fp32 neighbours; the clip-STE bounds (x = min_val and x = max_val give v == lo and v == hi exactly, the
    strict > / < of Round.backward; symmetric: +-max(|min|, |max|)) with their neighbours; +-0, +-inf, NaN."""
    sc, zp, qp = _flat_qp(bits, q_type, is_act)
    qmin, qmax = O.iao_qrange(bits, q_type, is_act)
    k = np.arange(int(qmin) - 2, int(qmax) + 2, dtype=np.float64)
    c = ((k + 0.5 + float(zp[0])) * float(sc[0])).astype(F)
    e = np.array([RANGE[0], RANGE[1], -RANGE[0], -RANGE[1]], dtype=F)
    pts = np.concatenate([c, e])
    x = np.concatenate([pts, np.nextafter(pts, F(-np.inf)), np.nextafter(pts, F(np.inf)), np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=F)]).astype(F)
    return x, _grad(_rng(23, bits, q_type), x.size), sc, zp, qp


def check_fq_boundary(be, bits, q_type, is_act):
    x, g, sc, zp, qp = boundary_set(bits, q_type, is_act)
    for mis in (False, True):
        y, dx = run_fq(be, x, g, 1, x.size, qp, bits, q_type, is_act, mis)
        with np.errstate(all="ignore"):
            assert eq(y, O.iao_fq_fwd(x, sc[0], zp[0], bits, q_type, is_act)[0]), ("fwd", mis)
            dx_ref = O.iao_fq_bwd(g, x, sc[0], zp[0], RANGE[0], RANGE[1], bits, q_type, is_act)
        assert eq(dx, dx_ref), ("bwd", mis)
        if q_type == 1 or is_act == 0:      # the gradient passes at both clip-STE bounds themselves (v == lo, v == hi)
            at_bound = np.isin(x, [RANGE[0], RANGE[1]] if q_type else [RANGE[1], -RANGE[1]])
            assert at_bound.sum() >= 2 and np.all(dx_ref[at_bound] != 0)


# ----------------------------------------------------------------------------- 3. fake-quant + activation
ACT_RELU, ACT_LEAKY, ACT_SIGMOID = 1, 2, 3
SIGMOID_BOUND = 1e-6                     # of max|ref|: device expf against fp64 exp (the bound of tests/test_gpu_iao_ops.py for this op)
worst = {"sigmoid": 0.0, "gap_ulp": 0.0}   # the largest errors measured in this process, printed by the runners


def _rel_err(got, ref):
    """max |got - ref| / max |ref| over the finite reference values; NaN exactly where the reference has NaN"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert eq(np.isnan(got), np.isnan(ref)), "NaN pattern"
    ok = np.isfinite(ref)
    return float(np.max(np.abs(got[ok] - ref[ok])) / max(np.max(np.abs(ref[ok])), 1e-30)) if ok.any() else 0.0


def check_fq_act(be, x, g, bits, q_type, act, mis):
    """y = act(Q(x)) and dx = Q'(x) * act'(Q(x)) * g.  ReLU / LeakyReLU exact: act on the oracle's Q(x), the oracle's clip-STE on g or fl32(g * slope).  Sigmoid:
    fp64 1 / (1 + exp(-q)) on the oracle's exact q, backward g * (1 - y) * y in fp64 where the oracle's STE passes the gradient; <= SIGMOID_BOUND of max|ref|."""
    n = x.size
    sc, zp, qp = _flat_qp(bits, q_type)
    xb, gb, qpd = Buf(be, n, mis, x), Buf(be, n, mis, g), be.to_dev(qp)
    y, dx = Buf(be, n, mis), Buf(be, n, mis)
    be.call("mn_iao_fq_act_fwd", xb.ptr, y.ptr, n, be.ptr(qpd), bits, q_type, act, C.c_float(float(SLOPE)), be.stream)
    be.call("mn_iao_fq_act_bwd", gb.ptr, xb.ptr, dx.ptr, n, be.ptr(qpd), bits, q_type, act, C.c_float(float(SLOPE)), be.stream)
    y, dx = y.get(), dx.get()
    ste = lambda d: O.iao_fq_bwd(d, x, sc[0], zp[0], RANGE[0], RANGE[1], bits, q_type, 1)
    with np.errstate(all="ignore"):
        q = O.iao_fq_fwd(x, sc[0], zp[0], bits, q_type, 1)[0]
        assert eq(np.isnan(y), np.isnan(x)), "NaN inputs stay NaN, nothing else becomes NaN"
        if act == ACT_SIGMOID:
            q64, g64 = q.astype(np.float64), g.astype(np.float64)
            y_ref = 1.0 / (1.0 + np.exp(-q64))
            dx_ref = np.where(ste(np.ones(n, dtype=F)) != 0, g64 * (1.0 - y_ref) * y_ref, 0.0)
            e_fwd, e_bwd = _rel_err(y, y_ref), _rel_err(dx, dx_ref)
            worst["sigmoid"] = max(worst["sigmoid"], e_fwd, e_bwd)
            assert e_fwd <= SIGMOID_BOUND and e_bwd <= SIGMOID_BOUND, (e_fwd, e_bwd)
            return
        neg = F(0) if act == ACT_RELU else SLOPE
        y_ref = np.where(q > 0, q, np.where(np.isnan(q), q, (q * neg).astype(F)))
        assert eq(y, y_ref), ("fwd", act, mis)
        assert eq(dx, ste(np.where(q > 0, g, (g * neg).astype(F)).astype(F))), ("bwd", act, mis)


def check_fq_act_size(be, n, mis, act, bits=8, q_type=1):
    r = _rng(31, n, act)
    check_fq_act(be, (r.standard_normal(n) * 2).astype(F), _grad(r, n), bits, q_type, act, mis)


def check_fq_act_small(be, act):
    for i, n in enumerate(SMALL):
        for mis in (False, True):
            check_fq_act_size(be, n, mis, act, (2, 4, 8, 16)[i % 4], i % 2)


def check_fq_act_boundary(be, bits, q_type, act):
    x, g = boundary_set(bits, q_type)[:2]
    for mis in (False, True):
        check_fq_act(be, x, g, bits, q_type, act, mis)


# ----------------------------------------------------------------------------- 4. fake-quant + average pool
# (planes, H, W, k): H != W; Ho == 1; the identity pool (y == Q(x)); a plain one; one whose 4100 * 16 * 16 outputs and 4100 * 32 * 32 inputs cross POOL_CAP
AVGPOOL = [dict(planes=5, H=9, W=6, k=3), dict(planes=3, H=7, W=14, k=7), dict(planes=4, H=5, W=5, k=1), dict(planes=24, H=12, W=12, k=2),
           dict(planes=4100, H=32, W=32, k=2)]
# the global average (k == H == W, k_fq_gap_fwd: one wave per plane) at H * W = k * k.  The entry point takes (H, W, k), so a plane of 7 elements cannot be
# asked for: 7 x 7 = 49 stands in for it (odd, and less than one wave, as 7 is).  1: a single lane; 64: exactly one wave; 100, 4096: the lane loop.
GAP_K = (1, 7, 8, 10, 64)
GAP_PLANES = 37
GAP_BOUND_ULP = 1.0                      # fp64 accumulation errs far below half an fp32 ulp, so the result is the correctly rounded mean or its neighbour


def check_avgpool(be, planes, H, W, k, bits=8, q_type=1):
    r = _rng(41, planes, H, W, k)
    x = (r.standard_normal((planes, H, W)) * 2).astype(F)
    Ho, Wo = H // k, W // k
    g = _grad(r, (planes, Ho, Wo))
    sc, zp, qp = _flat_qp(bits, q_type)
    assert be.lib.mn_iao_fq_avgpool_supported(H, W, k) == 1
    xb, gb, qpd = Buf(be, x.size, False, x), Buf(be, g.size, False, g), be.to_dev(qp)
    y, dx = Buf(be, g.size), Buf(be, x.size)
    be.call("mn_iao_fq_avgpool_fwd", xb.ptr, y.ptr, planes, H, W, k, be.ptr(qpd), bits, q_type, be.stream)
    be.call("mn_iao_fq_avgpool_bwd", gb.ptr, xb.ptr, dx.ptr, planes, H, W, k, be.ptr(qpd), bits, q_type, be.stream)
    y, dx = y.get().reshape(planes, Ho, Wo), dx.get().reshape(planes, H, W)
    q = O.iao_fq_fwd(x, sc[0], zp[0], bits, q_type, 1)[0]
    q5 = q.reshape(planes, Ho, k, Wo, k)
    mean64 = q5.astype(np.float64).mean(axis=(2, 4))
    if k == H and k == W:
        ref = mean64.astype(F)
        ulp = float(np.max(np.abs(y.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.maximum(np.abs(ref), np.finfo(F).tiny)).astype(np.float64)))
        worst["gap_ulp"] = max(worst["gap_ulp"], ulp)
        assert ulp <= GAP_BOUND_ULP, ulp
    else:
        s = np.zeros((planes, Ho, Wo), dtype=F)
        for rr in range(k):                         # the kernel's order: rows, then columns, fp32; then one fp32 divide
            for cc in range(k):
                s = (s + q5[:, :, rr, :, cc]).astype(F)
        assert eq(y, (s / F(k * k)).astype(F)), "fwd"
        assert np.max(np.abs(y - mean64)) <= 1e-6 * np.max(np.abs(mean64)), np.max(np.abs(y - mean64)) / np.max(np.abs(mean64))
        if k == 1:
            assert eq(y, q)
    gv = (g / F(k * k)).astype(F)
    g_up = np.repeat(np.repeat(gv, k, axis=1), k, axis=2)
    assert eq(dx, O.iao_fq_bwd(g_up, x, sc[0], zp[0], RANGE[0], RANGE[1], bits, q_type, 1)), "bwd"


def check_avgpool_refusals(be):
    """H % k != 0, k > 64 and k > H are refused by mn_iao_fq_avgpool_supported, and the forward entry then returns MN_EINVAL and writes nothing"""
    MN_EINVAL = -22
    qpd, xb = be.to_dev(_flat_qp(8, 1)[2]), Buf(be, 130 * 130, False, np.ones(130 * 130, dtype=F))
    for H, W, k in ((10, 10, 3), (12, 10, 4), (130, 130, 65), (4, 4, 8), (12, 12, 0)):
        assert be.lib.mn_iao_fq_avgpool_supported(H, W, k) == 0, (H, W, k)
        y = Buf(be, 130 * 130)
        assert be.lib.mn_iao_fq_avgpool_fwd(xb.ptr, y.ptr, 1, H, W, k, be.ptr(qpd), 8, 1, be.stream) == MN_EINVAL, (H, W, k)
        assert np.all(y.get() == POISON)
    for H, W, k in ((12, 12, 2), (64, 64, 64), (1, 1, 1), (128, 64, 64)):
        assert be.lib.mn_iao_fq_avgpool_supported(H, W, k) == 1, (H, W, k)


# ----------------------------------------------------------------------------- 5. map kernels
MAP_VARIANTS = ("aligned", "in0", "in1", "out")    # which operand goes through the offset pointer (in1: the two-input calls only)


def _map_data(n):
    """values around the decision points of all three maps: rounding ties k + 0.5 (and 0.49999997, which the fp32 add rounds up), the DoReFa clamp ends
    (0.1 x == 0 and == 1) and +-1 / +-0 of the binary activation's STE"""
    r = _rng(51, n)
    x = (r.standard_normal(n) * 4).astype(F)
    special = np.array([0.5, -0.5, 1.5, -2.5, 0.49999997, -0.49999997, 0.0, -0.0, 10.0, 1.0, -1.0, 8388607.5, 3.5, 9.999999, 10.000001, 0.99999994, -0.99999994],
                       dtype=F)
    m = min(n, special.size)
    x[n - m:] = special[:m]                 # in the tail
    x[:m] = special[:m][::-1]
    return x, _grad(r, n)


def check_maps(be, n, variant):
    x, g = _map_data(n)
    mis = dict(aligned=(0, 0, 0), in0=(1, 0, 0), in1=(0, 1, 0), out=(0, 0, 1))[variant]

    def map1(name, ref, *extra):
        a, y = Buf(be, n, mis[0], x), Buf(be, n, mis[2])
        be.call(name, a.ptr, y.ptr, n, *extra, be.stream)
        assert eq(y.get(), ref), (name, n, variant)

    def map2(name, ref, *extra):
        a, b, y = Buf(be, n, mis[0], g), Buf(be, n, mis[1], x), Buf(be, n, mis[2])
        be.call(name, a.ptr, b.ptr, y.ptr, n, *extra, be.stream)
        assert eq(y.get(), ref), (name, n, variant)
    if variant != "in1":
        map1("mn_round_half_away", O.rha(x))
        map1("mn_binact_fwd", O.binact_fwd(x))
    map2("mn_binact_bwd", O.binact_bwd(g, x))
    for bits in (2, 8):
        if variant != "in1":
            map1("mn_dorefa_act_fwd", O.dorefa_act_fwd(x, bits)[0], bits)
        map2("mn_dorefa_act_bwd", O.dorefa_act_bwd(g, x, bits), bits)


def check_maps_small(be):
    for n in SMALL:
        for variant in MAP_VARIANTS:
            check_maps(be, n, variant)


# ----------------------------------------------------------------------------- 6. histogram observer through the ABI
HIST_N = (1, 255, 257, 100003)


def _hist_ks(n):
    return sorted({1, max(1, n // 2), n})


def _hist_step(be, x, k, first, mv, ws):
    """one mn_hist_observe call with `out`; -> the expected max_val after it"""
    n = x.size
    xb, out = Buf(be, n, False, x), be.empty(1)
    be.call("mn_hist_observe", xb.ptr, n, k, first, MOMENTUM, be.ptr(mv), be.ptr(out), be.ptr(ws), be.stream)
    cur = np.sort(np.abs(x))[k - 1].reshape(1)              # np.sort puts NaN last, as torch.kthvalue does
    assert eq(be.to_host(out), cur), ("kth", n, k, be.to_host(out), cur)
    return cur


def check_hist(be, x, ks):
    n = x.size
    ws = be.empty(int(be.lib.mn_kth_abs_ws_bytes()) // 4 + 4)
    x2 = (x[::-1] * F(0.75)).astype(F)
    for k in ks:
        mv = be.empty(1)
        cur = _hist_step(be, x, k, 1, mv, ws)
        assert eq(be.to_host(mv), cur), ("first", n, k)
        cur2 = _hist_step(be, x2, k, 0, mv, ws)
        with np.errstate(all="ignore"):
            ref = O.observer_update("ema", False, cur, cur, cur2, cur2, MOMENTUM)[1]
        assert eq(be.to_host(mv), ref), ("ema", n, k, be.to_host(mv), ref)


def check_hist_sizes(be, n):
    check_hist(be, (_rng(61, n).standard_normal(n) * 3).astype(F), _hist_ks(n))


def check_hist_special(be):
    n = 257
    check_hist(be, np.full(n, 0.625, dtype=F), _hist_ks(n))                               # all equal: every rank is the same value
    x = (_rng(62).standard_normal(n)).astype(F)
    x[:12] = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-42, -7e-41, 1.1754942e-38, -1.1754944e-38, 1e-39, 0.0, -0.0, 2e-44], dtype=F)    # +-0, denormals, the smallest normal
    check_hist(be, x, [1, 2, 4, 5, 6, 9, 12, 13, n // 2, n])
    x = (_rng(63).standard_normal(n) * 2).astype(F)
    x[100] = np.nan                                                                      # NaN sorts last: rank n is NaN, rank n - 1 the largest finite |x|
    check_hist(be, x, [n - 1, n])
