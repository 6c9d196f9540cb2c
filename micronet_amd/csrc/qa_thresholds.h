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

// ---- IN = 1: the chain on fp32 y (the block behind the un-quantised first conv; alpha and bias take no part).  It is monotone in y the same way, so per channel
// there are flip and three fp32 thresholds with code = #{k : u >= T_k}, u = flip * y, for every |y| <= 1e9: with the constants within qa_chan_finite no intermediate
// overflows (|y - mean| <= 2e9, |zhat| <= 2e18, |z| <= 2e27 + 1e9), so no inf * 0 breaks the monotonicity.  Beyond that range (and for NaN) the caller evaluates
// qa_code_of<1> itself.  T_k = the smallest u in [-1e9, 1e9] whose exact chain value reaches k: bisection over the ordered bit patterns of fp32.
// the order-preserving integer key of an fp32 (-0 and +0 are one point, key 0) and its inverse
__device__ __forceinline__ int64_t qa_f32_key(float v) { const uint32_t b = mn_f2u(v); return (b & 0x80000000u) ? -(int64_t)(b & 0x7fffffffu) : (int64_t)b; }
__device__ __forceinline__ float qa_f32_of_key(int64_t k) { return k >= 0 ? mn_u2f((uint32_t)k) : mn_u2f(0x80000000u | (uint32_t)(-k)); }
#define QA_F32_RANGE 1.0e9f
__device__ __forceinline__ float qa_flip_of_f32(const QaCh& k, float s) { return (qa_code_of<1>(QA_F32_RANGE, k, s) < qa_code_of<1>(-QA_F32_RANGE, k, s)) ? -1.f : 1.f; }
// smallest u in [-1e9, 1e9] with code(flip * u) >= level, +inf if none (32 steps: the range holds 2.6e9 keys)
__device__ __forceinline__ float qa_threshold_of_f32(const QaCh& k, float s, float flip, uint32_t level) {
    int64_t lo = qa_f32_key(-QA_F32_RANGE), hi = qa_f32_key(QA_F32_RANGE) + 1;          // invariant: code(lo - 1) < level (virtually), code(hi) >= level (virtually at the end)
    const int64_t none = hi;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (qa_code_of<1>(flip * qa_f32_of_key(mid), k, s) >= level) hi = mid; else lo = mid + 1;
    }
    return lo == none ? INFINITY : qa_f32_of_key(lo);
}
