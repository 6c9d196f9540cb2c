// The per-channel constants of a k-bit (DoReFa) block and its integer-threshold form, shared by the streaming forward (qact_kernels.hip: k_qa_fwd) and the table pack
// of the code-packed deployment (qgemm_bits.hip: k_codes_wpack) -- ONE copy of the chain and of the search, so both produce the same codes by construction.
//
// The code is a monotone step function of the integer accumulator -- every step of the chain acc -> y -> zhat -> z -> relu -> clamp(0.1 a) -> rha(./s) is monotone in
// fp32 as well -- so per channel there are n = 2^a - 1 integers T_k with code = #{k : u >= T_k}, u = flip * acc (flip = -1 when the chain decreases).  T_k = the
// smallest u whose EXACT chain value reaches k, found by a binary search over the int16 range with that chain.
#pragma once
#include "common.h"

#define QA_NCH 9          // chan rows: alpha, bias, mean, invstd, gamma, beta, A = alpha*invstd, B = (bias - mean)*invstd, gi = gamma*invstd
struct QaCh { float alpha, bias, mean, invstd, ga, be, A, B, gi; };
__device__ __forceinline__ QaCh qa_load_ch(const float* __restrict__ chan, int C, int c) {
    QaCh k;
    k.alpha = chan[c]; k.bias = chan[C + c]; k.mean = chan[2 * C + c]; k.invstd = chan[3 * C + c]; k.ga = chan[4 * C + c]; k.be = chan[5 * C + c];
    k.A = chan[6 * C + c]; k.B = chan[7 * C + c]; k.gi = chan[8 * C + c];
    return k;
}
template <int IN>
__device__ __forceinline__ void qa_eval(float v, const QaCh& k, float& zh, float& z) {
    const float y = IN == 1 ? v : v * k.alpha + k.bias;
    zh = (y - k.mean) * k.invstd;
    z = zh * k.ga + k.be;
}
template <int IN>
__device__ __forceinline__ uint32_t qa_code_of(float v, const QaCh& k, float s) { float zh, z; qa_eval<IN>(v, k, zh, z); return qa_code(qa_relu(z), s); }
// |constant| <= 1e9 for all six: no intermediate of the chain can overflow on an int16 input (|y| <= 3.3e13, |zhat| <= 3.3e22, |z| <= 3.3e31), so no
// inf * 0 = NaN can break the monotonicity the thresholds rely on; anything wilder (or NaN) takes the element-wise path
__device__ __forceinline__ bool qa_finite(float v) { return fabsf(v) <= 1.0e9f; }
__device__ __forceinline__ bool qa_chan_finite(const QaCh& k) {
    return qa_finite(k.alpha) && qa_finite(k.bias) && qa_finite(k.mean) && qa_finite(k.invstd) && qa_finite(k.ga) && qa_finite(k.be);
}
// -1 when the chain decreases in the accumulator
__device__ __forceinline__ float qa_flip_of(const QaCh& k, float s) { return (qa_code_of<0>(32767.f, k, s) < qa_code_of<0>(-32768.f, k, s)) ? -1.f : 1.f; }
// smallest u in [-32768, 32768] with code(flip * u) >= level, 32769 if none (u = 32768 only occurs as -(-32768))
__device__ __forceinline__ int qa_threshold_of(const QaCh& k, float s, float flip, uint32_t level) {
    int lo = -32768, hi = 32769;                       // invariant: code(lo - 1) < level (virtually), code(hi) >= level (virtually at 32769)
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (qa_code_of<0>(flip * (float)mid, k, s) >= level) hi = mid; else lo = mid + 1;
    }
    return lo;
}
