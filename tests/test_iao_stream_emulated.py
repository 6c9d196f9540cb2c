"""The IAO streaming kernels (observer, fake-quant, fused activation / average pool, map kernels, histogram observer) compiled for the CPU SIMT emulator, through
the real C ABI, at the sizes where their launches change shape (tests/iao_stream_cases.py); the same table runs on the MI355X in tests/test_gpu_iao_stream.py.
No case of the table is GPU-only: the slowest (one flat-observer run above the grid cap, (2100, 4) per-row observer) take the emulator about ten seconds."""
import pytest

import abi_driver
import iao_stream_cases as S


@pytest.fixture(scope="module")
def be():
    b = abi_driver.Backend("emu")
    yield b
    print("\nemu worst errors: sigmoid %.3e of max|ref| (bound %.0e), global average %.3f fp32 ulp (bound %.0f)"
          % (S.worst["sigmoid"], S.SIGMOID_BOUND, S.worst["gap_ulp"], S.GAP_BOUND_ULP))


# ---- 1. observer + qparams + union
@pytest.mark.parametrize("case", range(len(S.OBSERVE_FLAT_BIG)))
def test_observe_flat_over_cap(be, case):
    S.check_observe_flat(be, **S.OBSERVE_FLAT_BIG[case])


def test_observe_flat_small(be):
    S.check_observe_flat_small(be)


@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("n", S.OBSERVE_SPECIAL_N)
def test_observe_nan_inf_zero(be, n, mis):
    S.check_observe_special(be, n, mis)


@pytest.mark.parametrize("case", range(len(S.OBSERVE_ROWS)))
def test_observe_rows(be, case):
    S.check_observe_rows(be, **S.OBSERVE_ROWS[case])


# ---- 2. fake-quant
@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("bits,q_type", [(8, 1), (4, 0)])
def test_fq_flat_over_cap(be, bits, q_type, mis):
    S.check_fq_flat(be, S.N_EW, mis, bits, q_type)


def test_fq_flat_small(be):
    S.check_fq_flat_small(be)


@pytest.mark.parametrize("case", range(len(S.FQ_ROWS)))
def test_fq_rows(be, case):
    S.check_fq_rows(be, **S.FQ_ROWS[case])


@pytest.mark.parametrize("bits,q_type,is_act", S.FQ_BOUNDARY)
def test_fq_boundaries(be, bits, q_type, is_act):
    S.check_fq_boundary(be, bits, q_type, is_act)


# ---- 3. fake-quant + activation
@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("act", [S.ACT_RELU, S.ACT_LEAKY, S.ACT_SIGMOID])
def test_fq_act_over_cap(be, act, mis):
    S.check_fq_act_size(be, S.N_EW, mis, act)


@pytest.mark.parametrize("act", [S.ACT_RELU, S.ACT_LEAKY, S.ACT_SIGMOID])
def test_fq_act_small(be, act):
    S.check_fq_act_small(be, act)


@pytest.mark.parametrize("act", [S.ACT_RELU, S.ACT_LEAKY, S.ACT_SIGMOID])
@pytest.mark.parametrize("bits,q_type", S.BOUNDARY)
def test_fq_act_boundaries(be, bits, q_type, act):
    S.check_fq_act_boundary(be, bits, q_type, act)


# ---- 4. fake-quant + average pool
@pytest.mark.parametrize("case", range(len(S.AVGPOOL)))
def test_fq_avgpool(be, case):
    S.check_avgpool(be, **S.AVGPOOL[case])


@pytest.mark.parametrize("k", S.GAP_K)
def test_fq_global_avgpool(be, k):
    S.check_avgpool(be, S.GAP_PLANES, k, k, k)


def test_fq_avgpool_refusals(be):
    S.check_avgpool_refusals(be)


# ---- 5. map kernels
@pytest.mark.parametrize("variant", S.MAP_VARIANTS)
def test_maps_over_cap(be, variant):
    S.check_maps(be, S.N_EW, variant)


def test_maps_small(be):
    S.check_maps_small(be)


# ---- 6. histogram observer
@pytest.mark.parametrize("n", S.HIST_N)
def test_hist_observe(be, n):
    S.check_hist_sizes(be, n)


def test_hist_observe_special(be):
    S.check_hist_special(be)
