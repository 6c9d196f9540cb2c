// Code-packed deployment of the k-bit (DoReFa) blocks conv -> bn -> relu -> [2x2 max-pool] -> next quantizer (qact_kernels.hip's block, eval mode): packed
// activation codes in, packed activation codes out, one kernel per hidden block.  Included by qgemm_bits.hip (whose route into both builds it shares).
//
//   activation planes : uint32 [N][ceil(C/32)][a_bits][H][W]; bit (c & 31) of plane p in word group (c >> 5) is bit p of channel c's code j in [0, 2^a - 1]; unused
//                       high bits of the last group are 0.  A zero word is 32 activations of CODE 0 = the value 0, so zero padding is a zero word: no border
//                       mask, no correction term.  Planar in (H, W): lanes = pixels read coalesced dwords.
//   accumulator       : weights (2k - n) / n, k in [0, n], n = 2^w - 1, as w_bits planes k_q.  Per output channel, over the channels c of its group and the taps:
//                         sum_c j_c k_c = sum_p sum_q 2^(p+q) popc(x_p & k_q)          sum_c j_c = sum_p 2^p popc(x_p & gmask)   (once per lane and group)
//                         acc = 2 sum j k - n sum j          -- the exact integer the byte path stashes (qgemm_sign.hip: mn_qconv_bnq_fwd_stash)
//   code              : u = flip * acc, code = #{k : u >= T_k}, T_k the integer thresholds of qa_thresholds.h (the search k_qa_fwd runs, on the same fp32 chain).
//                       2x2 max-pool: the code of the largest u of the window (the pool sits behind the ReLU and the quantizer is non-decreasing: exact).
//   weight table      : (private layout) 8 header words -- [0] rows whose channel constants fail qa_finite, [1] NW, [2] taps, [3] row stride, [4] rows, [5] Cw,
//                       [6] a_in | w_bits << 8 | a_out << 16, [7] bad out_order entries + rows with a weight off the grid -- then one row per output position, the
//                       32 rows of an output word SORTED BY GROUP (a lane keeps a group's input words and sum j in registers across all rows of the group):
//                         row[0] = w0 (first input word group the row reads), row[1] = flip (+-1), row[2] = bit position in the output word, row[3] = 1: another
//                         group than the row before, row[4..6] = T_1..T_3, row[7] = 0, then taps x NW x w_bits weight planes, then NW group-mask words.
//   consumer order    : the row at bit position j of an output word computes channel out_order[32 * word + j] (mn_bitconv_pack's convention).
// Covered: a_in = w_bits = a_out = 2; 1x1 and 3x3 / padding 1, stride 1, any groups, the 2x2 / stride 2 pool folded or not (mn_codeconv_*); the dense 5x5 / padding 2
// block of plain nin on an LDS-resident tile (mn_codeconv_tile_*) and the 2x2 / 2 and 3x3 / 2 / 1 max-pools on planes (mn_codes_maxpool).  The 1x1 block, dense or with
// whole input words per group, also has an int8-MFMA form with the same planes, thresholds and bits (mn_codeconv_mfma_*: qgemm_codes_mfma.h).
// The un-pooled 3x3 block with C / groups % 16 == 0 has one too, an implicit GEMM over (tap, channel) (mn_codeconv_mfma3_*: qgemm_codes_mfma3.h).
// The two MFMA forms, and only they, are also instantiated for a_in = w_bits = a_out = 4 (make_geom's `wide`); everything in this file is the 2-bit instantiation.
#pragma once
#include "qa_thresholds.h"

namespace mn_codes {

enum { HDR = 8, ROWHDR = 8, A = 2, WB = 2, NTHR = 3 };

struct Geom {
    int N, C, H, W, O, KS, groups;
    int Cg, Og, K, taps, Cw, OW, NW, stride;
    float s;          // the output quantizer's scale, dorefa_scale(a_bits_out): what mn_qa_fwd evaluates the chain with
};

// tile: the geometry of the LDS-tiled dense block (mn_codeconv_tile_*: 5x5 / padding 2, groups 1) instead of that of mn_codeconv_* (1x1, 3x3 / padding 1); the table
// layout, the K bound and everything k_codes_wpack reads are the same.  wide: the caller is one of the two int8-MFMA geometries (qgemm_codes_mfma.h, qgemm_codes_mfma3.h),
// whose kernels are also instantiated for 4-bit codes and weights: (4, 4, 4) is admitted beside (2, 2, 2); the popcount kernels never pass it.
static inline bool make_geom(const mn_conv_geom* g, int a_in, int w_bits, int a_out, Geom& q, bool tile = false, bool wide = false) {
    if (!g || g->N <= 0 || g->C <= 0 || g->H <= 0 || g->W <= 0 || g->O <= 0 || g->groups <= 0) return false;
    const bool four = wide && !tile && a_in == 4 && w_bits == 4 && a_out == 4;
    if (!four && (a_in != A || w_bits != WB || a_out != 2)) return false;          // (3-bit and mixed widths: not instantiated)
    if (g->KH != g->KW || (tile ? (g->KH != 5 || g->groups != 1) : (g->KH != 1 && g->KH != 3))) return false;
    const int pad = (g->KH - 1) / 2;
    if (g->stride_h != 1 || g->stride_w != 1 || g->dil_h != 1 || g->dil_w != 1 || g->pad_h != pad || g->pad_w != pad) return false;
    if (g->C % g->groups || g->O % g->groups || g->in_shuffle > 1) return false;      // a channel shuffle is folded into the PRODUCER's row order, never gathered here
    q.N = g->N; q.C = g->C; q.H = g->H; q.W = g->W; q.O = g->O; q.KS = g->KH; q.groups = g->groups;
    q.Cg = g->C / g->groups; q.Og = g->O / g->groups; q.taps = g->KH * g->KW;
    if ((int64_t)q.Cg * q.taps * ((1 << a_in) - 1) * ((1 << w_bits) - 1) > 32767) return false;          // the thresholds are searched over the int16 range of the stash
    q.K = q.Cg * q.taps;
    q.Cw = (g->C + 31) >> 5; q.OW = (g->O + 31) >> 5;
    q.NW = mn_bits::span_words(g->C, g->groups);
    q.stride = ROWHDR + q.taps * q.NW * WB + q.NW;
    q.s = dorefa_scale(a_out);
    const int64_t words = (int64_t)g->N * a_in * (q.Cw > q.OW ? q.Cw : q.OW) * g->H * g->W;
    if (words >= (1ll << 31) || (int64_t)q.OW * 32 * q.stride >= (1ll << 30)) return false;
    return true;
}

// ---------------------------------------------------------------- uint8 codes <-> planes
// one thread = 4 consecutive pixels of one channel word group: 32 aligned dword reads of 4 codes each per plane, 4 words out per plane.  Only planes p < a_bits are
// extracted: a code above 2^a - 1 is masked, not propagated.
__global__ __launch_bounds__(256) void k_codes_pack(const uint8_t* __restrict__ a, uint32_t* __restrict__ planes, int64_t total, int C, int Cw, int HW4, int abits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int p4 = (int)(i % HW4);
    const int64_t t = i / HW4;
    const int cw = (int)(t % Cw);
    const int64_t n = t / Cw;
    const int HW = HW4 * 4;
    const int cend = C - cw * 32 < 32 ? C - cw * 32 : 32;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a + (n * C + (int64_t)cw * 32) * HW) + p4;
    for (int p = 0; p < abits; ++p) {
        uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
        for (int b = 0; b < cend; ++b) {
            const uint32_t v = src[(int64_t)b * HW4] >> p;
            o0 |= (v & 1u) << b; o1 |= ((v >> 8) & 1u) << b; o2 |= ((v >> 16) & 1u) << b; o3 |= ((v >> 24) & 1u) << b;
        }
        uint32_t* dst = planes + ((n * Cw + cw) * abits + p) * HW + 4 * p4;
        dst[0] = o0; dst[1] = o1; dst[2] = o2; dst[3] = o3;
    }
}

// one thread = 4 consecutive pixels of one channel: 4 words in per plane, one dword of 4 codes out
__global__ __launch_bounds__(256) void k_codes_unpack(const uint32_t* __restrict__ planes, uint8_t* __restrict__ a, int64_t total, int C, int Cw, int HW4, int abits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int p4 = (int)(i % HW4);
    const int64_t t = i / HW4;
    const int c = (int)(t % C);
    const int64_t n = t / C;
    const int HW = HW4 * 4;
    uint32_t r = 0;
    for (int p = 0; p < abits; ++p) {
        const uint32_t* src = planes + ((n * Cw + (c >> 5)) * abits + p) * HW + 4 * p4;
#pragma unroll
        for (int e = 0; e < 4; ++e) r |= ((src[e] >> (c & 31)) & 1u) << (8 * e + p);
    }
    reinterpret_cast<uint32_t*>(a + (n * C + c) * HW)[p4] = r;
}

// ---------------------------------------------------------------- weight table: one block per output position
__global__ __launch_bounds__(256) void k_codes_wpack(Geom q, const float* __restrict__ w, const float* __restrict__ chan, const int32_t* __restrict__ order,
                                                     uint32_t* __restrict__ tab) {
    __shared__ int sh[256];
    const int j = blockIdx.x, tid = threadIdx.x, wd = j >> 5;
    if (j == 0 && tid == 0) {
        tab[1] = (uint32_t)q.NW; tab[2] = (uint32_t)q.taps; tab[3] = (uint32_t)q.stride; tab[4] = (uint32_t)(q.OW * 32); tab[5] = (uint32_t)q.Cw;
        tab[6] = (uint32_t)(A | (WB << 8) | (2 << 16));
    }
    // the channel and group of every position of this output word (a bad out_order entry or a position past O: no channel, sorted last, the row never fires)
    auto chan_of = [&](int jj) { const int o = jj < q.O ? (order ? order[jj] : jj) : -1; return (o >= 0 && o < q.O) ? o : -1; };
    const int o = chan_of(j);
    const int grp = o < 0 ? INT_MAX : o / q.Og;
    int rank = 0, same_before = 0;
    for (int jj = wd * 32; jj < wd * 32 + 32; ++jj) {
        const int oo = chan_of(jj);
        const int gg = oo < 0 ? INT_MAX : oo / q.Og;
        rank += (gg < grp) || (gg == grp && jj < j);
        same_before |= (gg == grp && jj < j);
    }
    uint32_t* row = tab + HDR + (int64_t)(wd * 32 + rank) * q.stride;
    if (j < q.O && o < 0 && tid == 0) atomicAdd(tab + 7, 1u);
    if (o < 0) {
        for (int i = tid; i < q.stride; i += 256) row[i] = i == 1 ? 1u : i == 2 ? (uint32_t)(j & 31) : i == 3 ? (uint32_t)!same_before : (i >= 4 && i < 4 + NTHR) ? 0x7fffffffu : 0u;
        return;
    }
    const int c0 = grp * q.Cg;
    int w0 = c0 >> 5;
    if (w0 > q.Cw - q.NW) w0 = q.Cw - q.NW;          // every row reads NW word groups per tap: keep the window inside the pixel's words
    const float* wr = w + (int64_t)o * q.K;          // [Cg][taps]
    const float nf = (float)((1 << WB) - 1);
    int off = 0;
    for (int idx = tid; idx < q.taps * q.NW; idx += 256) {
        const int t = idx / q.NW, k = idx - t * q.NW;
        uint32_t pl[WB] = {0u, 0u};
        for (int b = 0; b < 32; ++b) {
            const int ci = (w0 + k) * 32 + b - c0;
            if (ci >= 0 && ci < q.Cg) {
                const float kf = (wr[ci * q.taps + t] * nf + nf) * 0.5f;          // w = (2k - n) / n
                const float kr = rintf(kf);
                if (!(fabsf(kf - kr) <= 1e-3f) || kr < 0.f || kr > nf) off = 1;
                const uint32_t kc = (uint32_t)(kr < 0.f ? 0.f : kr > nf ? nf : kr == kr ? kr : 0.f);
#pragma unroll
                for (int qq = 0; qq < WB; ++qq) pl[qq] |= ((kc >> qq) & 1u) << b;
            }
        }
#pragma unroll
        for (int qq = 0; qq < WB; ++qq) row[ROWHDR + idx * WB + qq] = pl[qq];
    }
    for (int k = tid; k < q.NW; k += 256) {
        uint32_t m = 0;
        for (int b = 0; b < 32; ++b) {
            const int ci = (w0 + k) * 32 + b - c0;
            m |= (uint32_t)(ci >= 0 && ci < q.Cg) << b;
        }
        row[ROWHDR + q.taps * q.NW * WB + k] = m;
    }
    sh[tid] = off;
    __syncthreads();
    if (tid == 0) {
        int any = 0;
        for (int i = 0; i < 256; ++i) any |= sh[i];
        if (any) atomicAdd(tab + 7, 1u);
    }
    // thresholds: the search of k_qa_fwd on the block's eval-mode constants
    const QaCh k = qa_load_ch(chan, q.O, o);
    const float s = q.s;
    const bool fin = qa_chan_finite(k);
    const float flip = fin ? qa_flip_of(k, s) : 1.f;
    if (tid < NTHR) row[4 + tid] = fin ? (uint32_t)qa_threshold_of(k, s, flip, (uint32_t)tid + 1u) : 0x7fffffffu;
    if (tid == 0) {
        if (!fin) atomicAdd(tab + 0, 1u);
        row[0] = (uint32_t)w0;
        row[1] = (uint32_t)(flip < 0.f ? -1 : 1);
        row[2] = (uint32_t)(j & 31);
        row[3] = (uint32_t)!same_before;
        row[7] = 0u;
    }
}

// ---------------------------------------------------------------- plane-serial popcount convolution + thresholds -> output planes
struct Fwd {
    int total, Cw, H, W, Ho, Wo, OW, nw, stride, owpb;
};

// One lane owns one output pixel (POOL: one pooled pixel = the 2x2 window) and loops over the 32 rows of an output word; the row's words are wave-uniform (scalar
// loads).  NW > 0: the lane's input patch -- (KS + POOL)^2 cells x NW word groups x 2 planes -- lives in registers and is reloaded only when the row's group changes
// (rows are sorted by group).  NW == 0: any span, rolled loops, the words re-read per row (they stay in L1 / L2); registers stay flat.
template <int KS, int NW, bool POOL>
__global__ __launch_bounds__(256) void k_codeconv(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, uint32_t* __restrict__ y, Fwd q) {
    constexpr int SUB = POOL ? 4 : 1, PD = (POOL ? 2 : 1) + KS - 1, CELLS = PD * PD, P = (KS - 1) / 2, NWR = NW ? NW : 1;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= q.total) return;
    const int nw = NW ? NW : q.nw;
    const int HWo = q.Ho * q.Wo, HW = q.H * q.W;
    const int n = p / HWo, r = p - n * HWo;
    const int oh = r / q.Wo, ow = r - oh * q.Wo;
    const int ph0 = (POOL ? 2 * oh : oh) - P, pw0 = (POOL ? 2 * ow : ow) - P;
    const uint32_t* xn = x + (int64_t)n * q.Cw * A * HW;
    int off[CELLS];          // pixel offset of every cell of the patch, -1 outside the image (a zero word: code 0)
#pragma unroll
    for (int c = 0; c < CELLS; ++c) {
        const int ih = ph0 + c / PD, iw = pw0 + c % PD;
        off[c] = (ih >= 0 && ih < q.H && iw >= 0 && iw < q.W) ? ih * q.W + iw : -1;
    }
    uint32_t xr[CELLS * NWR * A];
#pragma unroll
    for (int i = 0; i < CELLS * NWR * A; ++i) xr[i] = 0u;
    int S[SUB];          // sum of the group's input codes over the taps of sub-pixel s
#pragma unroll
    for (int s = 0; s < SUB; ++s) S[s] = 0;
    const int ow0 = blockIdx.y * q.owpb;
    const int ow1 = ow0 + q.owpb < q.OW ? ow0 + q.owpb : q.OW;
    for (int owi = ow0; owi < ow1; ++owi) {
        const uint32_t* rowp = tab + HDR + (int64_t)owi * 32 * q.stride;
        uint32_t word0 = 0, word1 = 0;
        for (int j = 0; j < 32; ++j) {
            const uint32_t* row = rowp + j * q.stride;          // wave-uniform: every word of the row is a scalar operand
            const uint32_t* wp = row + ROWHDR;
            const uint32_t* xw = xn + (int64_t)row[0] * A * HW;
            if (row[3]) {          // (wave-uniform) a new group: its input words and the sum of its codes
                const uint32_t* gm = wp + KS * KS * nw * WB;
                if (NW) {
#pragma unroll
                    for (int c = 0; c < CELLS; ++c)
#pragma unroll
                        for (int k = 0; k < NWR; ++k)
#pragma unroll
                            for (int a = 0; a < A; ++a) xr[(c * NWR + k) * A + a] = off[c] >= 0 ? xw[(k * A + a) * HW + off[c]] : 0u;
                }
#pragma unroll
                for (int s = 0; s < SUB; ++s) {
                    int sum = 0;
#pragma unroll
                    for (int t = 0; t < KS * KS; ++t) {
                        const int c = ((s >> 1) + t / KS) * PD + (s & 1) + t % KS;
                        if (NW) {
#pragma unroll
                            for (int k = 0; k < NWR; ++k)
                                sum += mn_popc(xr[(c * NWR + k) * A] & gm[k]) + 2 * mn_popc(xr[(c * NWR + k) * A + 1] & gm[k]);
                        } else if (off[c] >= 0) {
#pragma unroll 1
                            for (int k = 0; k < nw; ++k)
                                sum += mn_popc(xw[(k * A) * HW + off[c]] & gm[k]) + 2 * mn_popc(xw[(k * A + 1) * HW + off[c]] & gm[k]);
                        }
                    }
                    S[s] = sum;
                }
            }
            const int flip = (int)row[1];
            int um = INT_MIN;
#pragma unroll
            for (int s = 0; s < SUB; ++s) {
                int d0 = 0, d1 = 0, d2 = 0;          // weights 1, 2, 4 of sum_p sum_q 2^(p+q) popc(x_p & k_q)
#pragma unroll
                for (int t = 0; t < KS * KS; ++t) {
                    const int c = ((s >> 1) + t / KS) * PD + (s & 1) + t % KS;
                    if (NW) {
#pragma unroll
                        for (int k = 0; k < NWR; ++k) {
                            const uint32_t x0 = xr[(c * NWR + k) * A], x1 = xr[(c * NWR + k) * A + 1];
                            const uint32_t k0 = wp[(t * NWR + k) * WB], k1 = wp[(t * NWR + k) * WB + 1];
                            d0 += mn_popc(x0 & k0); d1 += mn_popc(x0 & k1) + mn_popc(x1 & k0); d2 += mn_popc(x1 & k1);
                        }
                    } else if (off[c] >= 0) {
#pragma unroll 1
                        for (int k = 0; k < nw; ++k) {
                            const uint32_t x0 = xw[(k * A) * HW + off[c]], x1 = xw[(k * A + 1) * HW + off[c]];
                            const uint32_t k0 = wp[(t * nw + k) * WB], k1 = wp[(t * nw + k) * WB + 1];
                            d0 += mn_popc(x0 & k0); d1 += mn_popc(x0 & k1) + mn_popc(x1 & k0); d2 += mn_popc(x1 & k1);
                        }
                    }
                }
                const int acc = 2 * (d0 + 2 * d1 + 4 * d2) - 3 * S[s];
                const int u = flip * acc;
                um = u > um ? u : um;
            }
            const uint32_t code = (uint32_t)(um >= (int)row[4]) + (uint32_t)(um >= (int)row[5]) + (uint32_t)(um >= (int)row[6]);
            word0 |= (code & 1u) << row[2];
            word1 |= (code >> 1) << row[2];
        }
        uint32_t* yo = y + ((int64_t)n * q.OW + owi) * A * HWo + r;
        yo[0] = word0;
        yo[HWo] = word1;
    }
}

template <int KS, bool POOL>
static void launch_nw(int nwsel, dim3 grid, hipStream_t s, const uint32_t* tab, const uint32_t* x, uint32_t* y, const Fwd& f) {
    switch (nwsel) {
    case 1: hipLaunchKernelGGL((k_codeconv<KS, 1, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    case 2: if (KS == 1) { hipLaunchKernelGGL((k_codeconv<1, 2, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break; }
    case 4: if (KS == 1) { hipLaunchKernelGGL((k_codeconv<1, 4, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break; }
    default: hipLaunchKernelGGL((k_codeconv<KS, 0, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    }
}
static inline int nw_select(const Geom& q) { return (q.NW == 1 || (q.KS == 1 && (q.NW == 2 || q.NW == 4))) ? q.NW : 0; }

// ---------------------------------------------------------------- the classifier on planes: 1x1 conv, few outputs, fp32 weights, code planes in
// k_sconv_fwd<OP, 1> (norm_kernels.hip: the last conv of a DoReFa net on one-byte codes) with the byte read replaced by a plane extraction: j = b0 + 2 b1 as a float
// (exact).  Everything that decides the fp32 sums is that kernel's -- the 1024-thread block of 64 consecutive pixels, 16 waves splitting the channels into ranges of
// ceil(C / 16), lane (pq, cs) accumulating w * j over the channels c0 + cs + 4 i of its wave in increasing order, the two shuffles, the fixed-order LDS combine, the
// final * ascale + bias -- so the result equals mn_codeconv1x1_small_fwd on the unpacked planes to the bit (as k_bitsconv1x1_small relates to k_sconv_fwd<OP, 0>).
// A lane's channels of one 32-channel word group come out of one 16-byte load per plane; two word groups are in flight per trip.
enum { PC_WAVES = 16 };
template <int OP>
__global__ __launch_bounds__(1024) void k_planesconv1x1_small(const uint32_t* __restrict__ planes, const float* __restrict__ w, const float* __restrict__ bias,
                                                              float* __restrict__ y, int C, int Cw, int HW, int O, int64_t NP, float ascale) {
    HIP_DYNAMIC_SHARED(float, smem)
    float* wl = smem;                          // [C][OP]
    float* red = smem + (size_t)C * OP;        // [8][OP][64]
    const int tid = threadIdx.x, lane = tid & 63, wv = mn_uniform(tid >> 6), pq = lane & 15, cs = lane >> 4;
    for (int i = tid; i < C * OP; i += 1024) wl[i] = 0.f;
    __syncthreads();
    for (int i = tid; i < C * O; i += 1024) {       // coalesced read of w[o][c], transposed LDS write
        const int o = i / C, c = i - o * C;
        wl[c * OP + o] = w[i];
    }
    const int64_t P = (int64_t)blockIdx.x * 64 + 4 * pq;
    const int64_t Pc = P < NP ? P : 0;
    const int64_t n = Pc / HW;
    const int p = (int)(Pc - n * HW);
    float acc[4][OP];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int o = 0; o < OP; ++o) acc[e][o] = 0.f;
    const int per = (C + PC_WAVES - 1) / PC_WAVES;
    const int c0 = wv * per, c1 = (c0 + per) < C ? (c0 + per) : C;
    const uint32_t* src = planes + n * Cw * A * HW + p;          // plane 0 of word group 0 at the lane's four pixels (16-byte aligned: HW % 4 == 0)
    __syncthreads();
    auto add = [&](const u32x4& x0, const u32x4& x1, int sh, int c) {
        const float s0 = (float)(((x0[0] >> sh) & 1u) + 2u * ((x1[0] >> sh) & 1u)), s1 = (float)(((x0[1] >> sh) & 1u) + 2u * ((x1[1] >> sh) & 1u));
        const float s2 = (float)(((x0[2] >> sh) & 1u) + 2u * ((x1[2] >> sh) & 1u)), s3 = (float)(((x0[3] >> sh) & 1u) + 2u * ((x1[3] >> sh) & 1u));
#pragma unroll
        for (int o4 = 0; o4 < OP; o4 += 4) {
            const float4 w4 = *reinterpret_cast<const float4*>(wl + c * OP + o4);
            const float wv_[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[0][o4 + k] += wv_[k] * s0; acc[1][o4 + k] += wv_[k] * s1; acc[2][o4 + k] += wv_[k] * s2; acc[3][o4 + k] += wv_[k] * s3;
            }
        }
    };
    const int first = c0 + cs;                               // this lane's channels: first + 4 i < c1, in increasing order
    if (first < c1) {
        const int wlast = (c1 - 1) >> 5, r4 = first & 3;     // (wlast <= Cw - 1: every word read lies inside the pixel's Cw word groups)
        for (int wi = first >> 5; wi <= wlast; wi += 2) {
            const int wj = wi + 1 <= wlast ? wi + 1 : wlast;
            const uint32_t* pa = src + (int64_t)wi * A * HW;
            const uint32_t* pb = src + (int64_t)wj * A * HW;
            const u32x4 xa0 = *reinterpret_cast<const u32x4*>(pa), xa1 = *reinterpret_cast<const u32x4*>(pa + HW);
            const u32x4 xb0 = *reinterpret_cast<const u32x4*>(pb), xb1 = *reinterpret_cast<const u32x4*>(pb + HW);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int c = wi * 32 + r4 + 4 * b;
                if (c >= first && c < c1) add(xa0, xa1, r4 + 4 * b, c);
            }
            if (wi + 1 <= wlast) {
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const int c = wj * 32 + r4 + 4 * b;
                    if (c < c1) add(xb0, xb1, r4 + 4 * b, c);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int o = 0; o < OP; ++o) {
            float t = acc[e][o];
            t += __shfl_xor(t, 16, 64); t += __shfl_xor(t, 32, 64);
            acc[e][o] = t;
        }
    if (wv >= 8 && cs == 0) {
#pragma unroll
        for (int o = 0; o < OP; ++o)
            *reinterpret_cast<float4*>(red + ((wv - 8) * OP + o) * 64 + 4 * pq) = make_float4(acc[0][o], acc[1][o], acc[2][o], acc[3][o]);
    }
    __syncthreads();
    if (wv < 8 && cs == 0) {
#pragma unroll
        for (int o = 0; o < OP; ++o) {
            float4* r = reinterpret_cast<float4*>(red + (wv * OP + o) * 64 + 4 * pq);
            const float4 t = *r;
            *r = make_float4(acc[0][o] + t.x, acc[1][o] + t.y, acc[2][o] + t.z, acc[3][o] + t.w);
        }
    }
    __syncthreads();
    for (int i = tid; i < O * 16; i += 1024) {
        const int o = i >> 4, q = i & 15;                       // quad q of the block
        const int64_t Pq = (int64_t)blockIdx.x * 64 + 4 * q;
        if (Pq < NP) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < 8; ++k) {                        // fixed order
                const float4 t = *reinterpret_cast<const float4*>(red + (k * OP + o) * 64 + 4 * q);
                v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
            }
            const float bb = bias ? bias[o] : 0.f;
            const int64_t nq = Pq / HW;
            v.x *= ascale; v.y *= ascale; v.z *= ascale; v.w *= ascale;
            *reinterpret_cast<float4*>(y + (nq * O + o) * HW + (Pq - nq * HW)) = make_float4(v.x + bb, v.y + bb, v.z + bb, v.w + bb);
        }
    }
}

static inline bool planes_args_ok(const void* a, const void* b, int64_t N, int64_t C, int64_t HW, int a_bits) {
    return a && b && N > 0 && C > 0 && HW > 0 && HW % 4 == 0 && !(((uintptr_t)a) & 3) && !(((uintptr_t)b) & 3) && C <= (1 << 20) && HW <= (1 << 26) && a_bits >= 1 && a_bits <= 8;
}

// ---------------------------------------------------------------- dense 5x5 on an LDS-resident tile (k_bitconv_tile's launch shape on code planes)
// A 256-thread block owns a tile of output pixels (x images per block when the map is small) and stages the (th + 4) x (tw + 4) halo tile of all Cw word groups x 2
// planes into LDS once; halo cells and cells outside the batch are ZERO words = 32 activations of code 0 = the value 0, which is what zero padding is in this layout:
// no border mask, no `lost` correction.  The two planes of a cell are adjacent in LDS (one 8-byte read).  groups == 1: sum j is formed once per lane.
struct Tile {
    int N, Cw, H, W, OW, stride, owpb, tw, th, ipb, tx, ty;          // tile width / height (8 or 16), images per block (256 / (tw * th)), tiles per image row / column
};
enum { TILE_MAXW = 5, TILE_WORDS = 4 * 12 * 12 * TILE_MAXW * A };          // C <= 145: at most 5 word groups; 4 images of 8 x 8 + halo 2 is the largest LDS image

// NW > 0: Cw == NW, the loops over the word groups unrolled; NW == 0: any Cw <= TILE_MAXW, rolled.  Either way the window is read from LDS for every table row, one
// window row at a time (a 25 x NW x 2 register patch does not fit: fully unrolled, the hoisted window spills).
template <int KS, int NW>
__global__ __launch_bounds__(256) void k_codeconv_tile(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, uint32_t* __restrict__ y, Tile q) {
    __shared__ uint32_t sx[TILE_WORDS];
    constexpr int P = (KS - 1) / 2;
    const int nw = NW ? NW : q.Cw;
    const int tid = threadIdx.x;
    const int pw = q.tw + 2 * P, cells = (q.th + 2 * P) * pw;
    int b = blockIdx.x;
    const int bx = b % q.tx; b /= q.tx;
    const int by = b % q.ty;
    const int n0 = (b / q.ty) * q.ipb, h0 = by * q.th, w0 = bx * q.tw;
    const int HW = q.H * q.W;
    const int tot = q.ipb * nw * A * cells;          // <= TILE_WORDS (checked by the host)
    for (int i = tid; i < tot; i += 256) {
        const int c = i % cells, r = i / cells;          // r = (image, word group, plane): consecutive lanes read consecutive pixels of one plane
        const int pl = r % A, k = (r / A) % nw, im = r / (A * nw);
        const int n = n0 + im, ih = h0 + c / pw - P, iw = w0 + c % pw - P;
        uint32_t v = 0u;          // halo and everything outside the batch: zero words
        if (n < q.N && ih >= 0 && ih < q.H && iw >= 0 && iw < q.W) v = x[(((int64_t)n * q.Cw + k) * A + pl) * HW + ih * q.W + iw];
        sx[2 * ((im * nw + k) * cells + c) + pl] = v;
    }
    __syncthreads();
    const int per = q.tw * q.th;
    const int im = tid / per, r = tid - im * per;
    const int ly = r / q.tw, lx = r - ly * q.tw;
    const int n = n0 + im, oh = h0 + ly, ow = w0 + lx;
    if (n >= q.N || oh >= q.H || ow >= q.W) return;
    const uint32_t* xs = sx + 2 * (im * nw * cells + ly * pw + lx);          // the lane's window: cell (ty, tx) of word group k at xs[2 * (k * cells + ty * pw + tx) + plane]
    int S = 0;          // sum of the input codes over the window
#pragma unroll
    for (int t = 0; t < KS * KS; ++t) {
        const uint32_t* xp = xs + 2 * ((t / KS) * pw + t % KS);
        if (NW) {
#pragma unroll
            for (int k = 0; k < NW; ++k) S += mn_popc(xp[2 * k * cells]) + 2 * mn_popc(xp[2 * k * cells + 1]);
        } else {
#pragma unroll 1
            for (int k = 0; k < nw; ++k) S += mn_popc(xp[2 * k * cells]) + 2 * mn_popc(xp[2 * k * cells + 1]);
        }
    }
    const int ow0 = blockIdx.y * q.owpb;
    const int ow1 = ow0 + q.owpb < q.OW ? ow0 + q.owpb : q.OW;
    for (int owi = ow0; owi < ow1; ++owi) {
        const uint32_t* rowp = tab + HDR + (int64_t)owi * 32 * q.stride;
        uint32_t word0 = 0, word1 = 0;
        for (int j = 0; j < 32; ++j) {
            const uint32_t* row = rowp + j * q.stride;          // wave-uniform: every word of the row is a scalar operand
            const uint32_t* wp = row + ROWHDR;
            int d0 = 0, d1 = 0, d2 = 0;          // weights 1, 2, 4 of sum_p sum_q 2^(p+q) popc(x_p & k_q)
#pragma unroll 1
            for (int ty = 0; ty < KS; ++ty) {          // rolled: one window row (KS cells x nw word groups x 2 planes) is in registers at a time, the rest stays in LDS
                const uint32_t* xp = xs + 2 * ty * pw;
                const uint32_t* wt = wp + ty * KS * nw * WB;
                if (NW) {
#pragma unroll
                    for (int tx = 0; tx < KS; ++tx)
#pragma unroll
                        for (int k = 0; k < NW; ++k) {
                            const uint32_t x0 = xp[2 * (k * cells + tx)], x1 = xp[2 * (k * cells + tx) + 1];
                            const uint32_t k0 = wt[(tx * NW + k) * WB], k1 = wt[(tx * NW + k) * WB + 1];
                            d0 += mn_popc(x0 & k0); d1 += mn_popc(x0 & k1) + mn_popc(x1 & k0); d2 += mn_popc(x1 & k1);
                        }
                } else {
#pragma unroll
                    for (int tx = 0; tx < KS; ++tx)
#pragma unroll 1
                        for (int k = 0; k < nw; ++k) {
                            const uint32_t x0 = xp[2 * (k * cells + tx)], x1 = xp[2 * (k * cells + tx) + 1];
                            const uint32_t k0 = wt[(tx * nw + k) * WB], k1 = wt[(tx * nw + k) * WB + 1];
                            d0 += mn_popc(x0 & k0); d1 += mn_popc(x0 & k1) + mn_popc(x1 & k0); d2 += mn_popc(x1 & k1);
                        }
                }
            }
            const int acc = 2 * (d0 + 2 * d1 + 4 * d2) - 3 * S;
            const int u = (int)row[1] * acc;
            const uint32_t code = (uint32_t)(u >= (int)row[4]) + (uint32_t)(u >= (int)row[5]) + (uint32_t)(u >= (int)row[6]);
            word0 |= (code & 1u) << row[2];
            word1 |= (code >> 1) << row[2];
        }
        uint32_t* yo = y + ((int64_t)n * q.OW + owi) * A * HW + oh * q.W + ow;
        yo[0] = word0;
        yo[HW] = word1;
    }
}

// ---------------------------------------------------------------- max-pool on code planes: one lane per output word position, all planes
// Bit-sliced maximum of 32 codes at once, most significant plane first: gt / lt collect the channels where the running maximum / the tap is already decided to be
// larger, and the tap's bits are selected where lt.  Taps outside the image contribute code 0 (the pool sits behind a ReLU: no code is below it), i.e. are skipped.
// Planes at and above abits are zero registers (every index is a compile-time constant: nothing goes to scratch).
enum { POOL_MAXB = 8 };
__global__ __launch_bounds__(256) void k_codes_maxpool(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t total, int abits, int H, int W, int Ho, int Wo,
                                                       int k, int s, int pad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ow = (int)(i % Wo);
    const int64_t t = i / Wo;
    const int oh = (int)(t % Ho);
    const int64_t nc = t / Ho;          // (image, word group)
    const int HW = H * W, HWo = Ho * Wo;
    const uint32_t* src = in + nc * abits * HW;
    uint32_t m[POOL_MAXB];
#pragma unroll
    for (int p = 0; p < POOL_MAXB; ++p) m[p] = 0u;
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
            const int ih = oh * s - pad + dy, iw = ow * s - pad + dx;
            if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
            uint32_t v[POOL_MAXB];
#pragma unroll
            for (int p = 0; p < POOL_MAXB; ++p) v[p] = p < abits ? src[p * HW + ih * W + iw] : 0u;
            uint32_t gt = 0u, lt = 0u;
#pragma unroll
            for (int p = POOL_MAXB - 1; p >= 0; --p) {
                const uint32_t open = ~(gt | lt);
                gt |= open & m[p] & ~v[p];
                lt |= open & v[p] & ~m[p];
            }
#pragma unroll
            for (int p = 0; p < POOL_MAXB; ++p) m[p] = (m[p] & ~lt) | (v[p] & lt);
        }
    uint32_t* dst = out + nc * abits * HWo + oh * Wo + ow;
#pragma unroll
    for (int p = 0; p < POOL_MAXB; ++p)
        if (p < abits) dst[p * HWo] = m[p];
}

}  // namespace mn_codes

extern "C" int mn_codes_pack_planes(const uint8_t* codes, int64_t N, int64_t C, int64_t HW, int a_bits, uint32_t* planes, mn_stream_t stream) {
    if (!mn_codes::planes_args_ok(codes, planes, N, C, HW, a_bits)) MN_FAIL(MN_EINVAL, "mn_codes_pack_planes: needs H*W %% 4 == 0, 1 <= a_bits <= 8 and 4-byte aligned tensors");
    const int Cw = (int)((C + 31) >> 5);
    const int64_t total = N * Cw * (HW / 4);
    if (total > (int64_t)INT_MAX * 256 || N * Cw * a_bits * HW >= (1ll << 40)) MN_FAIL(MN_ENOTSUP, "mn_codes_pack_planes: tensor too large");
    mn_set_last_kernel("k_codes_pack"); mn_prof_bytes((double)N * C * HW + 4.0 * N * Cw * a_bits * HW); mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_codes::k_codes_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codes, planes, total, (int)C, Cw, (int)(HW / 4), a_bits);
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_codes_pack_planes");
    return MN_OK;
}

extern "C" int mn_codes_unpack_planes(const uint32_t* planes, int64_t N, int64_t C, int64_t HW, int a_bits, uint8_t* codes, mn_stream_t stream) {
    if (!mn_codes::planes_args_ok(codes, planes, N, C, HW, a_bits)) MN_FAIL(MN_EINVAL, "mn_codes_unpack_planes: needs H*W %% 4 == 0, 1 <= a_bits <= 8 and 4-byte aligned tensors");
    const int Cw = (int)((C + 31) >> 5);
    const int64_t total = N * C * (HW / 4);
    if (total > (int64_t)INT_MAX * 256 || N * Cw * a_bits * HW >= (1ll << 40)) MN_FAIL(MN_ENOTSUP, "mn_codes_unpack_planes: tensor too large");
    mn_set_last_kernel("k_codes_unpack"); mn_prof_bytes((double)N * C * HW + 4.0 * N * Cw * a_bits * HW); mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_codes::k_codes_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, planes, codes, total, (int)C, Cw, (int)(HW / 4), a_bits);
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_codes_unpack_planes");
    return MN_OK;
}

extern "C" int mn_codeconv_supported(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_codes::Geom q;
    return mn_codes::make_geom(g, a_bits_in, w_bits, a_bits_out, q) ? 1 : 0;
}

extern "C" int64_t mn_codeconv_table_bytes(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_codes::Geom q;
    if (!mn_codes::make_geom(g, a_bits_in, w_bits, a_bits_out, q)) return 0;
    return 4 * ((int64_t)mn_codes::HDR + (int64_t)q.OW * 32 * q.stride);
}

extern "C" int mn_planesconv1x1_small_supported(int64_t C, int64_t HW, int64_t O, int a_bits) {
    return a_bits == mn_codes::A && mn_bitsconv1x1_small_supported(C, HW, O);          // (mn_signconv1x1_small_supported's LDS bound)
}
extern "C" int mn_planesconv1x1_small_fwd(const uint32_t* planes, int a_bits, const float* w, const float* bias, float* y, int64_t N, int64_t C, int64_t HW, int64_t O,
                                          mn_stream_t stream) {
    if (!planes || !w || !y || N <= 0 || !aligned16(planes) || !aligned16(y)) MN_FAIL(MN_EINVAL, "mn_planesconv1x1_small_fwd: null argument / planes and y must be 16-byte aligned");
    if (!mn_planesconv1x1_small_supported(C, HW, O, a_bits))
        MN_FAIL(MN_ENOTSUP, "mn_planesconv1x1_small_fwd: needs 2-bit codes, O <= 16, C >= 4, HW %% 4 == 0 and the weights in LDS (mn_planesconv1x1_small_supported)");
    hipStream_t s = (hipStream_t)stream;
    const int64_t NP = N * HW, nb = (NP + 63) / 64;
    const int Cw = (int)((C + 31) >> 5);
    if (nb > 0x7fffffff || N * Cw * a_bits * HW >= (1ll << 40)) MN_FAIL(MN_ENOTSUP, "mn_planesconv1x1_small_fwd: tensor too large");
    const int OP = (int)((O + 3) / 4 * 4);
    const size_t lds = ((size_t)C * OP + (size_t)8 * OP * 64) * 4;
    const float ascale = dorefa_scale(a_bits);
    mn_set_last_kernel("k_planesconv1x1_small"); mn_prof_bytes(4.0 * N * Cw * a_bits * HW + 4.0 * N * O * HW + 4.0 * O * C); mn_prof_begin(s);
#define PC_LAUNCH(OPV) { raise_lds_limit((const void*)mn_codes::k_planesconv1x1_small<OPV>, lds); \
        hipLaunchKernelGGL((mn_codes::k_planesconv1x1_small<OPV>), dim3((unsigned)nb), dim3(1024), lds, s, planes, w, bias, y, (int)C, Cw, (int)HW, (int)O, NP, ascale); }
    if (OP == 4) PC_LAUNCH(4) else if (OP == 8) PC_LAUNCH(8) else if (OP == 12) PC_LAUNCH(12) else PC_LAUNCH(16)
#undef PC_LAUNCH
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_planesconv1x1_small_fwd");
    return MN_OK;
}

#define MN_CODECONV_COVER "geometry not covered (2-bit codes and weights; 1x1 or 3x3 / padding 1, stride 1, no input shuffle, K * 9 <= 32767)"
extern "C" int mn_codeconv_pack(const mn_conv_geom* g, const float* w, const float* chan, int a_bits_in, int w_bits, int a_bits_out, const int32_t* out_order,
                                uint32_t* table, mn_stream_t stream) {
    mn_codes::Geom q;
    if (!w || !chan || !table || (((uintptr_t)table) & 3)) MN_FAIL(MN_EINVAL, "mn_codeconv_pack: null / unaligned argument");
    if (!mn_codes::make_geom(g, a_bits_in, w_bits, a_bits_out, q)) MN_FAIL(MN_ENOTSUP, "mn_codeconv_pack: " MN_CODECONV_COVER);
    if (hipMemsetAsync(table, 0, 4 * mn_codes::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_codeconv_pack: header reset failed");          // the two counters
    mn_set_last_kernel("k_codes_wpack");
    hipLaunchKernelGGL(mn_codes::k_codes_wpack, dim3(q.OW * 32), dim3(256), 0, (hipStream_t)stream, q, w, chan, out_order, table);
    MN_CHECK_LAUNCH("mn_codeconv_pack");
    return MN_OK;
}

extern "C" int mn_codeconv_fwd(const mn_conv_geom* g, const uint32_t* table, const uint32_t* in_planes, uint32_t* out_planes, int pool, mn_stream_t stream) {
    mn_codes::Geom q;
    if (!table || !in_planes || !out_planes) MN_FAIL(MN_EINVAL, "mn_codeconv_fwd: null argument");
    if (!mn_codes::make_geom(g, mn_codes::A, mn_codes::WB, 2, q)) MN_FAIL(MN_ENOTSUP, "mn_codeconv_fwd: " MN_CODECONV_COVER);
    if (pool < 0 || pool > 1) MN_FAIL(MN_ENOTSUP, "mn_codeconv_fwd: pool must be 0 or 1 (2x2 / stride 2); the 3x3 / stride 2 pool is not folded");
    if (pool && ((q.H & 1) || (q.W & 1))) MN_FAIL(MN_EINVAL, "mn_codeconv_fwd: the folded 2x2 max-pool needs even H and W");
    mn_codes::Fwd f;
    f.Cw = q.Cw; f.H = q.H; f.W = q.W; f.OW = q.OW; f.nw = q.NW; f.stride = q.stride;
    f.Ho = pool ? q.H / 2 : q.H; f.Wo = pool ? q.W / 2 : q.W;
    f.total = q.N * f.Ho * f.Wo;
    const int bx = (f.total + 255) / 256;
    const dim3 grid(bx, mn_sets::grid_deal(bx, q.OW, f.owpb));          // the output words over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const int nwsel = mn_codes::nw_select(q);
    mn_set_last_kernel("k_codeconv<%d,%d,%d>", q.KS, nwsel, pool);
    mn_prof_bytes(4.0 * mn_codes::A * q.N * q.Cw * q.H * q.W + 4.0 * mn_codes::A * q.N * q.OW * f.Ho * f.Wo + 4.0 * (mn_codes::HDR + (double)q.OW * 32 * q.stride));
    mn_prof_begin(s);
    if (q.KS == 1) {
        if (pool) mn_codes::launch_nw<1, true>(nwsel, grid, s, table, in_planes, out_planes, f);
        else mn_codes::launch_nw<1, false>(nwsel, grid, s, table, in_planes, out_planes, f);
    } else {
        if (pool) mn_codes::launch_nw<3, true>(nwsel, grid, s, table, in_planes, out_planes, f);
        else mn_codes::launch_nw<3, false>(nwsel, grid, s, table, in_planes, out_planes, f);
    }
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_codeconv_fwd");
    return MN_OK;
}
#undef MN_CODECONV_COVER

// ---------------------------------------------------------------- the dense 5x5 block of plain nin, and the max-pool behind a block that cannot fold it
static inline bool tile_geom_valid(const mn_conv_geom* g) {
    return g && g->N > 0 && g->C > 0 && g->H > 0 && g->W > 0 && g->O > 0 && g->groups > 0 && g->KH > 0 && g->KW > 0 && g->stride_h > 0 && g->stride_w > 0 && g->dil_h > 0 &&
           g->dil_w > 0 && g->pad_h >= 0 && g->pad_w >= 0;
}
#define MN_CODETILE_COVER "geometry not covered (2-bit codes and weights; dense 5x5 / padding 2, stride 1, groups 1, C * 25 * 9 <= 32767: at most 145 channels)"

extern "C" int mn_codeconv_tile_supported(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_codes::Geom q;
    return mn_codes::make_geom(g, a_bits_in, w_bits, a_bits_out, q, true) ? 1 : 0;
}

extern "C" int64_t mn_codeconv_tile_table_bytes(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_codes::Geom q;
    if (!mn_codes::make_geom(g, a_bits_in, w_bits, a_bits_out, q, true)) return 0;
    return 4 * ((int64_t)mn_codes::HDR + (int64_t)q.OW * 32 * q.stride);
}

extern "C" int mn_codeconv_tile_pack(const mn_conv_geom* g, const float* w, const float* chan, int a_bits_in, int w_bits, int a_bits_out, const int32_t* out_order,
                                     uint32_t* table, mn_stream_t stream) {
    mn_codes::Geom q;
    if (!w || !chan || !table || (((uintptr_t)table) & 3) || !tile_geom_valid(g)) MN_FAIL(MN_EINVAL, "mn_codeconv_tile_pack: null / unaligned argument or invalid geometry");
    if (!mn_codes::make_geom(g, a_bits_in, w_bits, a_bits_out, q, true)) MN_FAIL(MN_ENOTSUP, "mn_codeconv_tile_pack: " MN_CODETILE_COVER);
    if (hipMemsetAsync(table, 0, 4 * mn_codes::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_codeconv_tile_pack: header reset failed");          // the two counters
    mn_set_last_kernel("k_codes_wpack");
    hipLaunchKernelGGL(mn_codes::k_codes_wpack, dim3(q.OW * 32), dim3(256), 0, (hipStream_t)stream, q, w, chan, out_order, table);
    MN_CHECK_LAUNCH("mn_codeconv_tile_pack");
    return MN_OK;
}

extern "C" int mn_codeconv_tile_fwd(const mn_conv_geom* g, const uint32_t* table, const uint32_t* in_planes, uint32_t* out_planes, mn_stream_t stream) {
    mn_codes::Geom q;
    if (!table || !in_planes || !out_planes || ((((uintptr_t)table) | ((uintptr_t)in_planes) | ((uintptr_t)out_planes)) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_codeconv_tile_fwd: null / unaligned argument or invalid geometry");
    if (!mn_codes::make_geom(g, mn_codes::A, mn_codes::WB, 2, q, true)) MN_FAIL(MN_ENOTSUP, "mn_codeconv_tile_fwd: " MN_CODETILE_COVER);
    mn_codes::Tile t;
    t.N = q.N; t.Cw = q.Cw; t.H = q.H; t.W = q.W; t.OW = q.OW; t.stride = q.stride;
    t.tw = q.W <= 8 ? 8 : 16; t.th = q.H <= 8 ? 8 : 16; t.ipb = 256 / (t.tw * t.th);
    t.tx = (q.W + t.tw - 1) / t.tw; t.ty = (q.H + t.th - 1) / t.th;
    const int64_t blocks = (int64_t)((q.N + t.ipb - 1) / t.ipb) * t.tx * t.ty;
    if (blocks > INT_MAX || q.Cw > mn_codes::TILE_MAXW || t.ipb * q.Cw * mn_codes::A * (t.tw + q.KS - 1) * (t.th + q.KS - 1) > mn_codes::TILE_WORDS)
        MN_FAIL(MN_ENOTSUP, "mn_codeconv_tile_fwd: tile does not fit");
    const int bx = (int)blocks;
    const dim3 grid(bx, mn_sets::grid_deal(bx, q.OW, t.owpb));          // the output words over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const int tsel = q.Cw == 3 ? 3 : 0;
    mn_set_last_kernel("k_codeconv_tile<%d,%d>", q.KS, tsel);
    mn_prof_bytes(4.0 * mn_codes::A * q.N * q.Cw * q.H * q.W + 4.0 * mn_codes::A * q.N * q.OW * q.H * q.W + 4.0 * (mn_codes::HDR + (double)q.OW * 32 * q.stride));
    mn_prof_begin(s);
    if (tsel) hipLaunchKernelGGL((mn_codes::k_codeconv_tile<5, 3>), grid, dim3(256), 0, s, table, in_planes, out_planes, t);
    else hipLaunchKernelGGL((mn_codes::k_codeconv_tile<5, 0>), grid, dim3(256), 0, s, table, in_planes, out_planes, t);
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_codeconv_tile_fwd");
    return MN_OK;
}
#undef MN_CODETILE_COVER

extern "C" int mn_codes_maxpool(const uint32_t* planes_in, int64_t N, int64_t Cw, int a_bits, int64_t H, int64_t W, int k, int stride, int pad, uint32_t* planes_out,
                                mn_stream_t stream) {
    if (!planes_in || !planes_out || ((((uintptr_t)planes_in) | ((uintptr_t)planes_out)) & 3) || N <= 0 || Cw <= 0 || H <= 0 || W <= 0)
        MN_FAIL(MN_EINVAL, "mn_codes_maxpool: null / unaligned / empty argument");
    if (!((k == 2 && stride == 2 && pad == 0) || (k == 3 && stride == 2 && pad == 1)) || a_bits < 1 || a_bits > mn_codes::POOL_MAXB)
        MN_FAIL(MN_ENOTSUP, "mn_codes_maxpool: window not covered (2x2 / stride 2 / padding 0 or 3x3 / stride 2 / padding 1, floor mode; 1 <= a_bits <= 8)");
    if (H > (1 << 15) || W > (1 << 15) || N * Cw * a_bits * H * W >= (1ll << 31)) MN_FAIL(MN_ENOTSUP, "mn_codes_maxpool: tensor too large");
    if (H + 2 * pad < k || W + 2 * pad < k) MN_FAIL(MN_EINVAL, "mn_codes_maxpool: image smaller than the window");
    const int Ho = (int)((H + 2 * pad - k) / stride + 1), Wo = (int)((W + 2 * pad - k) / stride + 1);
    const int64_t total = N * Cw * Ho * Wo;
    mn_set_last_kernel("k_codes_maxpool"); mn_prof_bytes(4.0 * N * Cw * a_bits * H * W + 4.0 * total * a_bits); mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_codes::k_codes_maxpool, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, planes_in, planes_out, total, a_bits, (int)H, (int)W,
                       Ho, Wo, k, stride, pad);
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_codes_maxpool");
    return MN_OK;
}
