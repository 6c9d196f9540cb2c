// Bit-packed inference of the BN-folded W-ternary / W-binary, A-binary graph (wbwtab/bn_fuse/bn_fuse.py:36-55: sign(conv(a, t * alpha) + b), a in +-1): one BIT per
// activation, XNOR / AND / popcount instead of multiply-accumulate, the bias and alpha folded into one integer threshold per output channel.
//
//   activation bits : uint32 [N][ceil(C/32)][H][W]; bit (c & 31) of word (c >> 5) at a pixel is 1 iff the activation is +1; unused high bits of the last word are 0.
//                     Channel-word planar: lanes = pixels read coalesced dwords.
//   weight table    : (private layout) 8 header words, then one row per output POSITION j (rows padded to a multiple of 32):
//                       row[0] = T (int32), row[1] = w0 (first input word the row reads), row[2] = nnz, row[3] = 0, then taps x NW pairs (s, m):
//                       s = sign plane (1 = +1), m = non-zero plane, of input words w0 .. w0 + NW - 1 at each tap; bits outside the row's group are 0 in both.
//                     acc = 2 * popc(~(x ^ s) & m & valid) - popc(m & valid)  -- zero padding is 0, not -1: a tap outside the image drops out of both terms.
//                     decision: +1 iff acc >= T, T = the first acc in [-K, K] for which !(fl(fl(acc * alpha) + b) < 0) holds in fp32 (K + 1: never).  The pack kernel
//                     EVALUATES that expression for every acc, so the threshold is exact by construction (alpha = 0 and NaN: constant decisions), and it counts
//                     the rows whose decision is not monotone in acc into header word 0 (0 for every alpha >= 0).
//   consumer order  : row j computes output channel out_order[j] (the channel the consumer reads at position j -- its channel shuffle folded into the producer);
//                     the row carries its own group's word offset, so no kernel gathers bits.
// One lane owns one output pixel (pool: one POOLED pixel, OR of the four decisions), loops over the 32 rows of an output word with the row's s / m / T wave-uniform
// (scalar loads), assembles the word in a register and stores one coalesced dword.
//
// Dense k x k blocks (groups == 1, at most 8 input words: the 5x5 / padding 2 block of nin, and the layout of a dense 3x3 with more than one word) are TILED: a block
// stages the words of its image tile plus the halo into LDS once, halo cells as ZERO words, and the inner loop carries no border mask.  A zero word reads as 32
// activations of -1, so a tap outside the image adds -d_t (d_t = the sum of the row's weight signs at tap t) instead of 0; the row carries the 2-D prefix sums of d_t
// ((KS + 1)^2 words behind its planes) and a lane adds back the d_t of the taps its border class loses: four lane-indexed loads per row, 0 for an interior pixel.
//   tiled row       : row[0..3] as above, taps x NW pairs (s, m), then S[(KS + 1)][(KS + 1)], S[a][b] = sum of d_t over taps (ty < a, tx < b).
// The 3x3 / stride 2 / padding 1 max-pool (models/nin.py) is an OR over the in-image cells of the window: folded into a 1x1 block (one lane = one pooled pixel, up to
// nine decisions) or a word-wise kernel of its own behind any other producer.
//
// The k-bit (DoReFa W2A2) counterpart -- activation CODES as bit planes, plane-serial popcounts, the block's BatchNorm + ReLU + quantizer as integer thresholds -- is
// qgemm_codes.h, included at the end of this file.  Behind it: the int8-MFMA forms of the 1x1 and the un-pooled 3x3 bit block (mn_bitconv_mfma_*, mn_bitconv_mfma3_*:
// qgemm_bits_mfma.h, qgemm_bits_mfma3.h) -- same bits, order, decision and header word 0, only the contraction differs.
#include "qgemm_dev.h"
#include "qgemm_mfma_sets.h"          // (the grid rule)

namespace mn_bits {

enum { HDR = 8, ROWHDR = 4 };

struct Geom {
    int N, C, H, W, O, KS, groups;
    int Cg, Og, K, taps, Cw, OW, NW, stride;      // channels per group in / out, taps per output, input / output words per pixel, words a row spans per tap, row stride
    int tiled;                                    // 1: the row carries the tap-sum prefix table of the LDS-tiled kernel behind its planes
};

enum { TILE_MAXW = 8, TILE_WORDS = 4 * 12 * 12 * TILE_MAXW };          // words per pixel the tiled kernel stages; its LDS image (4 images of 8 x 8 + halo 2 is the largest)

static inline int span_words(int C, int groups) {
    const int Cg = C / groups;
    int nw = 1;
    for (int g = 0; g < groups; ++g) {
        const int a = (g * Cg) >> 5, b = (g * Cg + Cg - 1) >> 5;
        if (b - a + 1 > nw) nw = b - a + 1;
    }
    return nw;
}

// popc == false: the geometry alone, for the MFMA forms (qgemm_bits_mfma.h, qgemm_bits_mfma3.h) -- without the bounds that belong to the popcount rows (the words a
// row spans, the tiled layout, the row stride), which those forms do not have.
static inline bool make_geom(const mn_conv_geom* g, Geom& q, bool popc = true) {
    if (!g || g->N <= 0 || g->C <= 0 || g->H <= 0 || g->W <= 0 || g->O <= 0 || g->groups <= 0) return false;
    if (g->KH != g->KW || (g->KH != 1 && g->KH != 3 && g->KH != 5)) return false;
    const int pad = (g->KH - 1) / 2;
    if (g->stride_h != 1 || g->stride_w != 1 || g->dil_h != 1 || g->dil_w != 1 || g->pad_h != pad || g->pad_w != pad) return false;
    if (g->C % g->groups || g->O % g->groups || g->in_shuffle > 1) return false;      // a channel shuffle is folded into the PRODUCER's row order, never gathered here
    q.N = g->N; q.C = g->C; q.H = g->H; q.W = g->W; q.O = g->O; q.KS = g->KH; q.groups = g->groups;
    q.Cg = g->C / g->groups; q.Og = g->O / g->groups; q.taps = g->KH * g->KW;
    if ((int64_t)q.Cg * q.taps > 65536) return false;
    q.K = q.Cg * q.taps;
    q.Cw = (g->C + 31) >> 5; q.OW = (g->O + 31) >> 5;
    q.NW = span_words(g->C, g->groups);
    if (!popc) {
        q.tiled = 0; q.stride = 0;
        return (int64_t)g->N * (q.Cw > q.OW ? q.Cw : q.OW) * g->H * g->W < (1ll << 31);
    }
    if (q.NW > (g->KH == 1 ? 64 : 8)) return false;
    q.tiled = g->KH > 1 && g->groups == 1 && q.Cw > 1 && q.Cw <= TILE_MAXW;
    if (g->KH == 5 && !(g->groups == 1 && q.Cw <= TILE_MAXW)) return false;          // 5x5: the tiled kernel only (dense, C <= 256)
    if (g->KH == 5) q.tiled = 1;
    q.stride = ROWHDR + 2 * q.taps * q.NW + (q.tiled ? (g->KH + 1) * (g->KH + 1) : 0);
    const int64_t words = (int64_t)g->N * (q.Cw > q.OW ? q.Cw : q.OW) * g->H * g->W;
    if (words >= (1ll << 31) || (int64_t)q.OW * 32 * q.stride >= (1ll << 30)) return false;
    return true;
}

// ---------------------------------------------------------------- int8 +-1 <-> bits
// one thread = 4 consecutive pixels of one channel word: 32 aligned dword reads of 4 codes each, 4 words out
__global__ __launch_bounds__(256) void k_bits_pack(const int8_t* __restrict__ a, uint32_t* __restrict__ bits, int64_t total, int C, int Cw, int HW4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int p4 = (int)(i % HW4);
    const int64_t t = i / HW4;
    const int cw = (int)(t % Cw);
    const int64_t n = t / Cw;
    const int HW = HW4 * 4;
    uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
    const int cend = C - cw * 32 < 32 ? C - cw * 32 : 32;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a + (n * C + (int64_t)cw * 32) * HW) + p4;
    for (int b = 0; b < cend; ++b) {
        const uint32_t v = ~src[(int64_t)b * HW4];          // +1 = 0x01, -1 = 0xff: the byte's top bit is the sign
        o0 |= ((v >> 7) & 1u) << b; o1 |= ((v >> 15) & 1u) << b; o2 |= ((v >> 23) & 1u) << b; o3 |= ((v >> 31) & 1u) << b;
    }
    uint32_t* dst = bits + (n * Cw + cw) * HW + 4 * p4;
    dst[0] = o0; dst[1] = o1; dst[2] = o2; dst[3] = o3;
}

// one thread = 4 consecutive pixels of one channel: 4 words in, one dword of 4 codes out
__global__ __launch_bounds__(256) void k_bits_unpack(const uint32_t* __restrict__ bits, int8_t* __restrict__ a, int64_t total, int C, int Cw, int HW4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int p4 = (int)(i % HW4);
    const int64_t t = i / HW4;
    const int c = (int)(t % C);
    const int64_t n = t / C;
    const int HW = HW4 * 4;
    const uint32_t* src = bits + (n * Cw + (c >> 5)) * HW + 4 * p4;
    uint32_t r = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) r |= (((src[e] >> (c & 31)) & 1u) ? 0x01u : 0xffu) << (8 * e);
    reinterpret_cast<uint32_t*>(a + (n * C + c) * HW)[p4] = r;
}

// ---------------------------------------------------------------- weight table
__device__ __forceinline__ int block_reduce(int v, int op, int* sh) {      // op 0: sum, 1: min, 2: max; every thread of the 256-thread block calls it
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const int a = sh[tid], b = sh[tid + s];
            sh[tid] = op == 0 ? a + b : op == 1 ? (a < b ? a : b) : (a > b ? a : b);
        }
        __syncthreads();
    }
    return sh[0];
}

// The decision of the byte kernels, !(fl(fl(acc * alpha) + b) < 0), EVALUATED for every accumulator value acc in [-K, K] a row can produce -- the one copy of the
// search (k_bits_wpack, and the packs of the MFMA forms in qgemm_bits_mfma.h / qgemm_bits_mfma3.h).  Thread `tid` of `nt` takes acc = -K + tid, -K + tid + nt, ...;
// the caller combines tmin (min) and cnt (sum) over its threads and reads the threshold off the pair.
__device__ __forceinline__ void decision_scan(int K, float alpha, float b, int tid, int nt, int& tmin, int& cnt) {
    tmin = INT_MAX; cnt = 0;
    for (int acc = -K + tid; acc <= K; acc += nt) {
        const float p = (float)acc * alpha;
        const float yv = p + b;
        if (!(yv < 0.f)) { cnt++; if (acc < tmin) tmin = acc; }
    }
}
__device__ __forceinline__ bool decision_monotone(int K, int tmin, int cnt) { return cnt == 0 || cnt == K - tmin + 1; }          // (alpha < 0 cannot come out of max|w|)
__device__ __forceinline__ int decision_threshold(int K, int tmin, int cnt) { return cnt == 0 ? K + 1 : tmin; }                 // K + 1: never

// one block per table row
__global__ __launch_bounds__(256) void k_bits_wpack(Geom q, const float* __restrict__ w, const float* __restrict__ bias, const int32_t* __restrict__ order,
                                                    uint32_t* __restrict__ tab) {
    __shared__ int sh[256];
    const int j = blockIdx.x, tid = threadIdx.x;
    uint32_t* row = tab + HDR + (int64_t)j * q.stride;
    if (j == 0 && tid == 0) { tab[1] = (uint32_t)q.NW; tab[2] = (uint32_t)q.taps; tab[3] = (uint32_t)q.stride; tab[4] = (uint32_t)(q.OW * 32); tab[5] = (uint32_t)q.Cw; tab[6] = (uint32_t)q.tiled; }
    int o = j < q.O ? (order ? order[j] : j) : -1;
    if (j < q.O && (o < 0 || o >= q.O)) {          // a bad out_order entry: counted, the row never fires, nothing is read out of bounds
        if (tid == 0) atomicAdd(tab + 0, 1u);
        o = -1;
    }
    if (o < 0) {
        for (int i = tid; i < q.stride; i += 256) row[i] = i == 0 ? 0x7fffffffu : 0u;
        return;
    }
    const int grp = o / q.Og, c0 = grp * q.Cg;
    int w0 = c0 >> 5;
    if (w0 > q.Cw - q.NW) w0 = q.Cw - q.NW;          // every row reads NW words per tap: keep the window inside the pixel's words
    const float* wr = w + (int64_t)o * q.K;          // [Cg][taps]
    float mx = 0.f;
    int nz = 0, nan = 0;
    for (int i = tid; i < q.K; i += 256) {
        const float v = wr[i];
        mx = fmaxf(mx, fabsf(v));
        nz += v != 0.f;
        nan |= v != v;
    }
    mx = mn_u2f((unsigned)block_reduce((int)mn_f2u(mx), 2, sh));          // non-negative floats order like their bit patterns
    nz = block_reduce(nz, 0, sh);
    nan = block_reduce(nan, 2, sh);
    const float alpha = nan ? mn_u2f(0x7fc00000u) : mx;
    for (int idx = tid; idx < q.taps * q.NW; idx += 256) {
        const int t = idx / q.NW, k = idx - t * q.NW;
        uint32_t s = 0, m = 0;
        for (int b = 0; b < 32; ++b) {
            const int ci = (w0 + k) * 32 + b - c0;
            if (ci >= 0 && ci < q.Cg) {
                const float v = wr[ci * q.taps + t];
                m |= (uint32_t)(v != 0.f) << b;
                s |= (uint32_t)(v > 0.f) << b;
            }
        }
        row[ROWHDR + 2 * idx] = s;
        row[ROWHDR + 2 * idx + 1] = m;
    }
    if (q.tiled) {          // S[a][b] = sum over taps (ty < a, tx < b) of d_t, d_t = sum of the row's weight signs at tap t (what a zero halo word wrongly subtracts)
        __shared__ int dt[32];
        if (tid < q.taps) {
            int d = 0;
            for (int ci = 0; ci < q.Cg; ++ci) {
                const float v = wr[ci * q.taps + tid];
                d += (v > 0.f) - (v < 0.f);
            }
            dt[tid] = d;
        }
        __syncthreads();
        const int S1 = q.KS + 1;
        if (tid < S1 * S1) {
            const int a = tid / S1, c = tid - a * S1;
            int v = 0;
            for (int ty = 0; ty < a; ++ty)
                for (int tx = 0; tx < c; ++tx) v += dt[ty * q.KS + tx];
            row[ROWHDR + 2 * q.taps * q.NW + tid] = (uint32_t)v;
        }
    }
    // the decision of the byte kernels, evaluated for every accumulator value the row can produce
    const float b = bias ? bias[o] : 0.f;
    int tmin, cnt;
    decision_scan(q.K, alpha, b, tid, 256, tmin, cnt);
    tmin = block_reduce(tmin, 1, sh);
    cnt = block_reduce(cnt, 0, sh);
    if (tid == 0) {
        if (!decision_monotone(q.K, tmin, cnt)) atomicAdd(tab + 0, 1u);          // not monotone in acc
        row[0] = (uint32_t)decision_threshold(q.K, tmin, cnt);
        row[1] = (uint32_t)w0;
        row[2] = (uint32_t)nz;
        row[3] = 0u;
    }
}

// ---------------------------------------------------------------- XNOR-popcount convolution + threshold -> output bits
struct Fwd {
    int total, Cw, H, W, Ho, Wo, OW, nw, stride, owpb;
};

template <int KS, int NW, bool POOL>
__global__ __launch_bounds__(256) void k_bitconv(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, uint32_t* __restrict__ y, Fwd q) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= q.total) return;
    const int nw = NW ? NW : q.nw;
    const int HWo = q.Ho * q.Wo, HW = q.H * q.W;
    const int n = p / HWo, r = p - n * HWo;
    const int oh = r / q.Wo, ow = r - oh * q.Wo;
    const uint32_t* xn = x + (int64_t)n * q.Cw * HW;
    const int ow0 = blockIdx.y * q.owpb;
    const int ow1 = ow0 + q.owpb < q.OW ? ow0 + q.owpb : q.OW;
    for (int owi = ow0; owi < ow1; ++owi) {
        const uint32_t* rowp = tab + HDR + (int64_t)owi * 32 * q.stride;
        uint32_t word = 0;
#pragma unroll 2
        for (int j = 0; j < 32; ++j) {
            const uint32_t* row = rowp + j * q.stride;          // wave-uniform: T, w0, nnz, s and m are scalar operands
            const int T = (int)row[0];
            const uint32_t* xw = xn + (int64_t)row[1] * HW;
            uint32_t bit = 0;
#pragma unroll(KS == 1 ? 4 : 1)
            for (int sub = 0; sub < (POOL ? 4 : 1); ++sub) {
                const int ph = POOL ? 2 * oh + (sub >> 1) : oh, pw = POOL ? 2 * ow + (sub & 1) : ow;
                int acc;
                if (KS == 1) {
                    const uint32_t* xp = xw + ph * q.W + pw;
                    int P = 0;
#pragma unroll
                    for (int k = 0; k < nw; ++k) P += mn_popc(~(xp[k * HW] ^ row[ROWHDR + 2 * k]) & row[ROWHDR + 2 * k + 1]);
                    acc = 2 * P - (int)row[2];
                } else {
                    int P = 0, Z = 0;
#pragma unroll
                    for (int t = 0; t < 9; ++t) {
                        const int ih = ph + t / 3 - 1, iw = pw + t % 3 - 1;
                        const bool ok = ih >= 0 && ih < q.H && iw >= 0 && iw < q.W;
                        const uint32_t* xp = xw + ih * q.W + iw;
#pragma unroll
                        for (int k = 0; k < nw; ++k) {
                            const uint32_t xv = ok ? xp[k * HW] : 0u;
                            const uint32_t mv = ok ? row[ROWHDR + 2 * (t * nw + k) + 1] : 0u;
                            P += mn_popc(~(xv ^ row[ROWHDR + 2 * (t * nw + k)]) & mv);
                            Z += mn_popc(mv);
                        }
                    }
                    acc = 2 * P - Z;
                }
                bit |= (uint32_t)(acc >= T);
            }
            word |= bit << j;
        }
        y[((int64_t)n * q.OW + owi) * HWo + r] = word;
    }
}

template <int KS, bool POOL>
static void launch_nw(int nwsel, dim3 grid, hipStream_t s, const uint32_t* tab, const uint32_t* x, uint32_t* y, const Fwd& f) {
    switch (nwsel) {          // (3x3: one word per tap -- every grouped 3x3 layer of the nets -- is unrolled; wider spans take the rolled loop, whose registers stay flat)
    case 1: hipLaunchKernelGGL((k_bitconv<KS, 1, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    case 2: if (KS == 1) { hipLaunchKernelGGL((k_bitconv<1, 2, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break; }
    case 4: if (KS == 1) { hipLaunchKernelGGL((k_bitconv<1, 4, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break; }
    default: hipLaunchKernelGGL((k_bitconv<KS, 0, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    }
}


// ---------------------------------------------------------------- dense k x k on an LDS-resident tile
struct Tile {
    int N, Cw, H, W, OW, stride, owpb, tw, th, ipb, tx, ty;          // tile width / height (8 or 16), images per block (256 / (tw * th)), tiles per image row / column
};

// NW > 0: Cw == NW, the lane's KS x KS x NW window is read from LDS into registers once; NW == 0: any Cw <= TILE_MAXW, the window is read from LDS for every row.
template <int KS, int NW>
__global__ __launch_bounds__(256) void k_bitconv_tile(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, uint32_t* __restrict__ y, Tile q) {
    __shared__ uint32_t sx[TILE_WORDS];
    constexpr int P = (KS - 1) / 2, S1 = KS + 1;
    const int nw = NW ? NW : q.Cw;
    const int tid = threadIdx.x;
    const int pw = q.tw + 2 * P, cells = (q.th + 2 * P) * pw;
    int b = blockIdx.x;
    const int bx = b % q.tx; b /= q.tx;
    const int by = b % q.ty;
    const int n0 = (b / q.ty) * q.ipb, h0 = by * q.th, w0 = bx * q.tw;
    const int HW = q.H * q.W;
    const int tot = q.ipb * nw * cells;          // <= TILE_WORDS (checked by the host)
    for (int i = tid; i < tot; i += 256) {
        const int c = i % cells, r = i / cells;
        const int k = r % nw, n = n0 + r / nw;
        const int ih = h0 + c / pw - P, iw = w0 + c % pw - P;
        uint32_t v = 0u;          // halo and everything outside the batch: zero words
        if (n < q.N && ih >= 0 && ih < q.H && iw >= 0 && iw < q.W) v = x[((int64_t)n * q.Cw + k) * HW + ih * q.W + iw];
        sx[i] = v;
    }
    __syncthreads();
    const int per = q.tw * q.th;
    const int im = tid / per, r = tid - im * per;
    const int ly = r / q.tw, lx = r - ly * q.tw;
    const int n = n0 + im, oh = h0 + ly, ow = w0 + lx;
    if (n >= q.N || oh >= q.H || ow >= q.W) return;
    // the taps inside the image are ty in [y0, y1), tx in [x0, x1): the lane's border class, as four offsets into the row's prefix table
    const int y0 = P - oh > 0 ? P - oh : 0, y1 = q.H + P - oh < KS ? q.H + P - oh : KS;
    const int x0 = P - ow > 0 ? P - ow : 0, x1 = q.W + P - ow < KS ? q.W + P - ow : KS;
    const int i11 = y1 * S1 + x1, i01 = y0 * S1 + x1, i10 = y1 * S1 + x0, i00 = y0 * S1 + x0;
    const uint32_t* xs = sx + im * nw * cells + ly * pw + lx;
    uint32_t xr[NW ? KS * KS * NW : 1];
    if (NW) {
#pragma unroll
        for (int t = 0; t < KS * KS; ++t)
#pragma unroll
            for (int k = 0; k < NW; ++k) xr[t * NW + k] = xs[k * cells + (t / KS) * pw + t % KS];
    }
    const int ow0 = blockIdx.y * q.owpb;
    const int ow1 = ow0 + q.owpb < q.OW ? ow0 + q.owpb : q.OW;
    for (int owi = ow0; owi < ow1; ++owi) {
        const uint32_t* rowp = tab + HDR + (int64_t)owi * 32 * q.stride;
        uint32_t word = 0;
        for (int j = 0; j < 32; ++j) {
            const uint32_t* row = rowp + j * q.stride;          // wave-uniform
            const uint32_t* sp = row + ROWHDR + 2 * KS * KS * nw;
            const int lost = (int)sp[S1 * S1 - 1] - ((int)sp[i11] - (int)sp[i01] - (int)sp[i10] + (int)sp[i00]);          // sum of d_t over the taps outside the image
            int Pc = 0;
            if (NW) {
#pragma unroll
                for (int t = 0; t < KS * KS * NW; ++t) Pc += mn_popc(~(xr[t] ^ row[ROWHDR + 2 * t]) & row[ROWHDR + 2 * t + 1]);
            } else {
#pragma unroll
                for (int t = 0; t < KS * KS; ++t) {
                    const uint32_t* xp = xs + (t / KS) * pw + t % KS;
                    for (int k = 0; k < nw; ++k) Pc += mn_popc(~(xp[k * cells] ^ row[ROWHDR + 2 * (t * nw + k)]) & row[ROWHDR + 2 * (t * nw + k) + 1]);
                }
            }
            const int acc = 2 * Pc - (int)row[2] + lost;
            word |= (uint32_t)(acc >= (int)row[0]) << j;
        }
        y[((int64_t)n * q.OW + owi) * HW + oh * q.W + ow] = word;
    }
}

// MEASUREMENT ONLY (never dispatched by a plan): the global re-read loop of k_bitconv at any odd KS, on the same table -- what the tiled kernel is compared against.
template <int KS>
__global__ __launch_bounds__(256) void k_bitconv_direct(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, uint32_t* __restrict__ y, Fwd q) {
    constexpr int P = (KS - 1) / 2;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= q.total) return;
    const int HW = q.H * q.W;
    const int n = p / HW, r = p - n * HW;
    const int oh = r / q.W, ow = r - oh * q.W;
    const uint32_t* xn = x + (int64_t)n * q.Cw * HW;
    const int ow0 = blockIdx.y * q.owpb;
    const int ow1 = ow0 + q.owpb < q.OW ? ow0 + q.owpb : q.OW;
    for (int owi = ow0; owi < ow1; ++owi) {
        const uint32_t* rowp = tab + HDR + (int64_t)owi * 32 * q.stride;
        uint32_t word = 0;
        for (int j = 0; j < 32; ++j) {
            const uint32_t* row = rowp + j * q.stride;
            int Pc = 0, Z = 0;
#pragma unroll
            for (int t = 0; t < KS * KS; ++t) {
                const int ih = oh + t / KS - P, iw = ow + t % KS - P;
                const bool ok = ih >= 0 && ih < q.H && iw >= 0 && iw < q.W;
                const uint32_t* xp = xn + ih * q.W + iw;
                for (int k = 0; k < q.nw; ++k) {
                    const uint32_t xv = ok ? xp[k * HW] : 0u;
                    const uint32_t mv = ok ? row[ROWHDR + 2 * (t * q.nw + k) + 1] : 0u;
                    Pc += mn_popc(~(xv ^ row[ROWHDR + 2 * (t * q.nw + k)]) & mv);
                    Z += mn_popc(mv);
                }
            }
            word |= (uint32_t)(2 * Pc - Z >= (int)row[0]) << j;
        }
        y[((int64_t)n * q.OW + owi) * HW + r] = word;
    }
}

// ---------------------------------------------------------------- 1x1 block + the 3x3 / stride 2 / padding 1 max-pool behind it
// One lane owns one POOLED pixel: OR of the decisions of the (up to nine) in-image cells of its window.  NWMAX > 0: dense (every row reads words 0 .. Cw - 1, Cw <=
// NWMAX), the window's words are held in registers; NWMAX == 0: any 1x1 geometry, the words are re-read per row.
template <int NWMAX>
__global__ __launch_bounds__(256) void k_bitconv1_pool3(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, uint32_t* __restrict__ y, Fwd q) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= q.total) return;
    const int HWo = q.Ho * q.Wo, HW = q.H * q.W;
    const int n = p / HWo, r = p - n * HWo;
    const int oh = r / q.Wo, ow = r - oh * q.Wo;
    const uint32_t* xn = x + (int64_t)n * q.Cw * HW;
    uint32_t okm = 0;
    int off[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        const int ih = 2 * oh - 1 + c / 3, iw = 2 * ow - 1 + c % 3;
        const bool ok = ih >= 0 && ih < q.H && iw >= 0 && iw < q.W;
        okm |= (uint32_t)ok << c;
        off[c] = ok ? ih * q.W + iw : 0;          // (a cell outside the image is never read)
    }
    uint32_t xr[NWMAX ? 9 * NWMAX : 1];
    if (NWMAX) {
#pragma unroll
        for (int c = 0; c < 9; ++c)
#pragma unroll
            for (int k = 0; k < NWMAX; ++k) xr[c * NWMAX + k] = (k < q.nw && ((okm >> c) & 1u)) ? xn[k * HW + off[c]] : 0u;
    }
    const int ow0 = blockIdx.y * q.owpb;
    const int ow1 = ow0 + q.owpb < q.OW ? ow0 + q.owpb : q.OW;
    for (int owi = ow0; owi < ow1; ++owi) {
        const uint32_t* rowp = tab + HDR + (int64_t)owi * 32 * q.stride;
        uint32_t word = 0;
        for (int j = 0; j < 32; ++j) {
            const uint32_t* row = rowp + j * q.stride;          // wave-uniform
            const int T = (int)row[0] + (int)row[2];          // 2 * P - nnz >= T
            uint32_t hit = 0;
            if (NWMAX) {
#pragma unroll
                for (int c = 0; c < 9; ++c) {
                    int Pc = 0;
#pragma unroll
                    for (int k = 0; k < NWMAX; ++k)
                        if (k < q.nw) Pc += mn_popc(~(xr[c * NWMAX + k] ^ row[ROWHDR + 2 * k]) & row[ROWHDR + 2 * k + 1]);
                    hit |= (uint32_t)(2 * Pc >= T) << c;
                }
            } else {
                const uint32_t* xw = xn + (int64_t)row[1] * HW;
#pragma unroll
                for (int c = 0; c < 9; ++c) {
                    int Pc = 0;
                    if ((okm >> c) & 1u)
                        for (int k = 0; k < q.nw; ++k) Pc += mn_popc(~(xw[k * HW + off[c]] ^ row[ROWHDR + 2 * k]) & row[ROWHDR + 2 * k + 1]);
                    hit |= (uint32_t)(2 * Pc >= T) << c;
                }
            }
            word |= (uint32_t)((hit & okm) != 0u) << j;
        }
        y[((int64_t)n * q.OW + owi) * HWo + r] = word;
    }
}

// ---------------------------------------------------------------- max-pool on bits: OR over the in-image cells of the window, one thread per output word
__global__ __launch_bounds__(256) void k_bits_maxpool(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int64_t total, int H, int W, int Ho, int Wo, int k, int s,
                                                      int pad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ow = (int)(i % Wo);
    const int64_t t = i / Wo;
    const int oh = (int)(t % Ho);
    const uint32_t* src = in + (t / Ho) * H * W;
    uint32_t v = 0;
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
            const int ih = oh * s - pad + dy, iw = ow * s - pad + dx;
            if (ih >= 0 && ih < H && iw >= 0 && iw < W) v |= src[ih * W + iw];
        }
    out[i] = v;
}

// ---------------------------------------------------------------- the classifier on bits: 1x1 conv, few outputs, fp32 weights, activation bits in
// k_sconv_fwd (norm_kernels.hip: the last conv of a binary net on int8 sign codes) with the code read replaced by a bit extraction: +w where the bit is 1, -w where
// it is 0 (w * +-1.f: exact).  Everything that decides the fp32 sums is that kernel's: block = 64 consecutive pixels of the [N][HW] pixel axis, 16 waves split the
// channels into ranges of ceil(C / 16), lane (pq, cs) accumulates 4 pixels x OP outputs over the channels c0 + cs + 4 i of its wave in increasing order, the four
// cs groups are combined by the same two shuffles and the 16 waves through LDS in the same fixed order -- the logits equal mn_signconv1x1_small_fwd on the unpacked
// bits to the bit.  What changes is the traffic: a lane's channels of one 32-channel word (every fourth: 8 of them) come out of ONE 16-byte load of the word's four
// pixels instead of 8 dword loads of codes; two words are in flight per trip.
enum { BC_MAXO = 16, BC_WAVES = 16 };
template <int OP>
__global__ __launch_bounds__(1024) void k_bitsconv1x1_small(const uint32_t* __restrict__ bits, const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ y, int C, int Cw, int HW, int O, int64_t NP) {
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
    const int per = (C + BC_WAVES - 1) / BC_WAVES;
    const int c0 = wv * per, c1 = (c0 + per) < C ? (c0 + per) : C;
    const uint32_t* src = bits + n * Cw * HW + p;          // word 0 of the lane's four pixels (16-byte aligned: HW % 4 == 0)
    __syncthreads();
    auto add = [&](const u32x4& x, int sh, int c) {
        const float s0 = ((x[0] >> sh) & 1u) ? 1.f : -1.f, s1 = ((x[1] >> sh) & 1u) ? 1.f : -1.f, s2 = ((x[2] >> sh) & 1u) ? 1.f : -1.f, s3 = ((x[3] >> sh) & 1u) ? 1.f : -1.f;
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
        const int wlast = (c1 - 1) >> 5, r4 = first & 3;     // (wlast <= Cw - 1: every word read lies inside the pixel's Cw words)
        for (int wi = first >> 5; wi <= wlast; wi += 2) {
            const int wj = wi + 1 <= wlast ? wi + 1 : wlast;
            const u32x4 xa = *reinterpret_cast<const u32x4*>(src + (int64_t)wi * HW), xb = *reinterpret_cast<const u32x4*>(src + (int64_t)wj * HW);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int c = wi * 32 + r4 + 4 * b;
                if (c >= first && c < c1) add(xa, r4 + 4 * b, c);
            }
            if (wi + 1 <= wlast) {
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const int c = wj * 32 + r4 + 4 * b;
                    if (c < c1) add(xb, r4 + 4 * b, c);
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
            *reinterpret_cast<float4*>(y + (nq * O + o) * HW + (Pq - nq * HW)) = make_float4(v.x + bb, v.y + bb, v.z + bb, v.w + bb);
        }
    }
}

}  // namespace mn_bits

extern "C" int mn_bitsconv1x1_small_supported(int64_t C, int64_t HW, int64_t O) {
    if (!(O >= 1 && O <= mn_bits::BC_MAXO && C >= 4 && C <= (1 << 20) && HW >= 4 && HW % 4 == 0 && HW <= (1 << 26))) return 0;
    const int64_t OP = (O + 3) / 4 * 4;
    return (C * OP + 8 * OP * 64) * 4 <= 128 * 1024;          // the weight image and the partial sums live in LDS (mn_signconv1x1_small_supported's bound)
}
extern "C" int mn_bitsconv1x1_small_fwd(const uint32_t* bits, const float* w, const float* bias, float* y, int64_t N, int64_t C, int64_t HW, int64_t O, mn_stream_t stream) {
    if (!bits || !w || !y || N <= 0 || !aligned16(bits) || !aligned16(y)) MN_FAIL(MN_EINVAL, "mn_bitsconv1x1_small_fwd: null argument / bits and y must be 16-byte aligned");
    if (!mn_bitsconv1x1_small_supported(C, HW, O)) MN_FAIL(MN_ENOTSUP, "mn_bitsconv1x1_small_fwd: needs O <= 16, C >= 4, HW %% 4 == 0 and the weights in LDS (mn_bitsconv1x1_small_supported)");
    hipStream_t s = (hipStream_t)stream;
    const int64_t NP = N * HW, nb = (NP + 63) / 64;
    const int Cw = (int)((C + 31) >> 5);
    if (nb > 0x7fffffff || N * Cw * HW >= (1ll << 40)) MN_FAIL(MN_ENOTSUP, "mn_bitsconv1x1_small_fwd: tensor too large");
    const int OP = (int)((O + 3) / 4 * 4);
    const size_t lds = ((size_t)C * OP + (size_t)8 * OP * 64) * 4;
    mn_set_last_kernel("k_bitsconv1x1_small"); mn_prof_bytes(4.0 * N * Cw * HW + 4.0 * N * O * HW + 4.0 * O * C); mn_prof_begin(s);
#define BC_LAUNCH(OPV) { raise_lds_limit((const void*)mn_bits::k_bitsconv1x1_small<OPV>, lds); \
        hipLaunchKernelGGL((mn_bits::k_bitsconv1x1_small<OPV>), dim3((unsigned)nb), dim3(1024), lds, s, bits, w, bias, y, (int)C, Cw, (int)HW, (int)O, NP); }
    if (OP == 4) BC_LAUNCH(4) else if (OP == 8) BC_LAUNCH(8) else if (OP == 12) BC_LAUNCH(12) else BC_LAUNCH(16)
#undef BC_LAUNCH
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_bitsconv1x1_small_fwd");
    return MN_OK;
}

extern "C" int mn_bits_pack_sign8(const int8_t* a, int64_t N, int64_t C, int64_t HW, uint32_t* bits, mn_stream_t stream) {
    if (!a || !bits || N <= 0 || C <= 0 || HW <= 0 || HW % 4 || (((uintptr_t)a) & 3) || (((uintptr_t)bits) & 3) || C > (1 << 20) || HW > (1 << 26))
        MN_FAIL(MN_EINVAL, "mn_bits_pack_sign8: needs H*W %% 4 == 0 and 4-byte aligned tensors");
    const int Cw = (int)((C + 31) >> 5);
    const int64_t total = N * Cw * (HW / 4);
    if (total > (int64_t)INT_MAX * 256) MN_FAIL(MN_ENOTSUP, "mn_bits_pack_sign8: tensor too large");
    mn_set_last_kernel("k_bits_pack"); mn_prof_bytes((double)N * C * HW + 4.0 * N * Cw * HW); mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_bits::k_bits_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, bits, total, (int)C, Cw, (int)(HW / 4));
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_bits_pack_sign8");
    return MN_OK;
}

extern "C" int mn_bits_unpack_sign8(const uint32_t* bits, int64_t N, int64_t C, int64_t HW, int8_t* a, mn_stream_t stream) {
    if (!a || !bits || N <= 0 || C <= 0 || HW <= 0 || HW % 4 || (((uintptr_t)a) & 3) || (((uintptr_t)bits) & 3) || C > (1 << 20) || HW > (1 << 26))
        MN_FAIL(MN_EINVAL, "mn_bits_unpack_sign8: needs H*W %% 4 == 0 and 4-byte aligned tensors");
    const int Cw = (int)((C + 31) >> 5);
    const int64_t total = N * C * (HW / 4);
    if (total > (int64_t)INT_MAX * 256) MN_FAIL(MN_ENOTSUP, "mn_bits_unpack_sign8: tensor too large");
    mn_set_last_kernel("k_bits_unpack"); mn_prof_bytes((double)N * C * HW + 4.0 * N * Cw * HW); mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_bits::k_bits_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bits, a, total, (int)C, Cw, (int)(HW / 4));
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_bits_unpack_sign8");
    return MN_OK;
}

extern "C" int mn_bitconv_supported(const mn_conv_geom* g) {
    mn_bits::Geom q;
    return mn_bits::make_geom(g, q) ? 1 : 0;
}

extern "C" int64_t mn_bitconv_table_bytes(const mn_conv_geom* g) {
    mn_bits::Geom q;
    if (!mn_bits::make_geom(g, q)) return 0;
    return 4 * ((int64_t)mn_bits::HDR + (int64_t)q.OW * 32 * q.stride);
}

extern "C" int mn_bitconv_pack(const mn_conv_geom* g, const float* w, const float* bias, const int32_t* out_order, uint32_t* table, mn_stream_t stream) {
    mn_bits::Geom q;
    if (!w || !table || (((uintptr_t)table) & 3)) MN_FAIL(MN_EINVAL, "mn_bitconv_pack: null / unaligned argument");
    if (!mn_bits::make_geom(g, q)) MN_FAIL(MN_ENOTSUP, "mn_bitconv_pack: geometry not covered (1x1, 3x3 / padding 1 or dense 5x5 / padding 2 of at most 256 channels; stride 1, no input shuffle)");
    if (hipMemsetAsync(table, 0, 4 * mn_bits::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_bitconv_pack: header reset failed");          // word 0: bad-row count
    mn_set_last_kernel("k_bits_wpack");
    hipLaunchKernelGGL(mn_bits::k_bits_wpack, dim3(q.OW * 32), dim3(256), 0, (hipStream_t)stream, q, w, bias, out_order, table);
    MN_CHECK_LAUNCH("mn_bitconv_pack");
    return MN_OK;
}

extern "C" int mn_bitconv_fwd(const mn_conv_geom* g, const uint32_t* table, const uint32_t* x_bits, uint32_t* y_bits, int pool, mn_stream_t stream) {
    mn_bits::Geom q;
    if (!table || !x_bits || !y_bits) MN_FAIL(MN_EINVAL, "mn_bitconv_fwd: null argument");
    if (!mn_bits::make_geom(g, q)) MN_FAIL(MN_ENOTSUP, "mn_bitconv_fwd: geometry not covered (1x1, 3x3 / padding 1 or dense 5x5 / padding 2 of at most 256 channels; stride 1, no input shuffle)");
    const int alt = pool & MN_BITCONV_ALT;          // measurement only: the other kernel for the same table (tiled <-> global re-read)
    pool &= ~MN_BITCONV_ALT;
    if (pool < 0 || pool > 2) MN_FAIL(MN_EINVAL, "mn_bitconv_fwd: pool must be 0, 1 (2x2 / stride 2) or 2 (3x3 / stride 2 / padding 1)");
    if (pool == 1 && q.KS == 5) MN_FAIL(MN_ENOTSUP, "mn_bitconv_fwd: a max-pool is not folded into the 5x5 block (use mn_bits_maxpool behind it)");
    if (pool == 2 && q.KS != 1) MN_FAIL(MN_ENOTSUP, "mn_bitconv_fwd: the 3x3 / stride 2 max-pool is folded into 1x1 blocks only (use mn_bits_maxpool behind it)");
    if (alt && (pool || !q.tiled)) MN_FAIL(MN_ENOTSUP, "mn_bitconv_fwd: no alternative kernel for this geometry");
    if (pool == 1 && ((q.H & 1) || (q.W & 1))) MN_FAIL(MN_EINVAL, "mn_bitconv_fwd: the folded 2x2 max-pool needs even H and W");
    mn_bits::Fwd f;
    f.Cw = q.Cw; f.H = q.H; f.W = q.W; f.OW = q.OW; f.nw = q.NW; f.stride = q.stride;
    f.Ho = pool == 1 ? q.H / 2 : pool == 2 ? (q.H - 1) / 2 + 1 : q.H;
    f.Wo = pool == 1 ? q.W / 2 : pool == 2 ? (q.W - 1) / 2 + 1 : q.W;
    f.total = q.N * f.Ho * f.Wo;
    const bool tile = q.tiled && (q.KS == 5) != (alt != 0);          // 5x5: always; the dense 3x3 with several words: only when asked for
    mn_bits::Tile t;
    int bx = (f.total + 255) / 256;
    if (tile) {
        t.N = q.N; t.Cw = q.Cw; t.H = q.H; t.W = q.W; t.OW = q.OW; t.stride = q.stride;
        t.tw = q.W <= 8 ? 8 : 16; t.th = q.H <= 8 ? 8 : 16; t.ipb = 256 / (t.tw * t.th);
        t.tx = (q.W + t.tw - 1) / t.tw; t.ty = (q.H + t.th - 1) / t.th;
        const int64_t blocks = (int64_t)((q.N + t.ipb - 1) / t.ipb) * t.tx * t.ty;
        if (blocks > INT_MAX || t.ipb * q.Cw * (t.tw + q.KS - 1) * (t.th + q.KS - 1) > mn_bits::TILE_WORDS) MN_FAIL(MN_ENOTSUP, "mn_bitconv_fwd: tile does not fit");
        bx = (int)blocks;
    }
    const dim3 grid(bx, mn_sets::grid_deal(bx, q.OW, f.owpb));          // the output words over grid.y
    t.owpb = f.owpb;
    const hipStream_t s = (hipStream_t)stream;
    const int nwsel = (q.NW == 1 || (q.KS == 1 && (q.NW == 2 || q.NW == 4))) ? q.NW : 0;
    const int tsel = q.KS == 5 ? (q.Cw == 3 ? 3 : 0) : (q.Cw == 6 ? 6 : 0);
    const int psel = (q.groups == 1 && q.Cw <= 8) ? 8 : 0;
    if (tile) mn_set_last_kernel("k_bitconv_tile<%d,%d>", q.KS, tsel);
    else if (alt) mn_set_last_kernel("k_bitconv_direct<%d>", q.KS);
    else if (pool == 2) mn_set_last_kernel("k_bitconv1_pool3<%d>", psel);
    else mn_set_last_kernel("k_bitconv<%d,%d,%d>", q.KS, nwsel, pool ? 1 : 0);
    mn_prof_bytes(4.0 * q.N * q.Cw * q.H * q.W + 4.0 * q.N * q.OW * f.Ho * f.Wo + 4.0 * (mn_bits::HDR + (double)q.OW * 32 * q.stride));
    mn_prof_begin(s);
    if (tile) {
        if (q.KS == 5) {
            if (tsel) hipLaunchKernelGGL((mn_bits::k_bitconv_tile<5, 3>), grid, dim3(256), 0, s, table, x_bits, y_bits, t);
            else hipLaunchKernelGGL((mn_bits::k_bitconv_tile<5, 0>), grid, dim3(256), 0, s, table, x_bits, y_bits, t);
        } else {
            if (tsel) hipLaunchKernelGGL((mn_bits::k_bitconv_tile<3, 6>), grid, dim3(256), 0, s, table, x_bits, y_bits, t);
            else hipLaunchKernelGGL((mn_bits::k_bitconv_tile<3, 0>), grid, dim3(256), 0, s, table, x_bits, y_bits, t);
        }
    } else if (alt) {
        hipLaunchKernelGGL((mn_bits::k_bitconv_direct<5>), grid, dim3(256), 0, s, table, x_bits, y_bits, f);
    } else if (pool == 2) {
        if (psel) hipLaunchKernelGGL((mn_bits::k_bitconv1_pool3<8>), grid, dim3(256), 0, s, table, x_bits, y_bits, f);
        else hipLaunchKernelGGL((mn_bits::k_bitconv1_pool3<0>), grid, dim3(256), 0, s, table, x_bits, y_bits, f);
    } else if (q.KS == 1) {
        if (pool) mn_bits::launch_nw<1, true>(nwsel, grid, s, table, x_bits, y_bits, f);
        else mn_bits::launch_nw<1, false>(nwsel, grid, s, table, x_bits, y_bits, f);
    } else {
        if (pool) mn_bits::launch_nw<3, true>(nwsel, grid, s, table, x_bits, y_bits, f);
        else mn_bits::launch_nw<3, false>(nwsel, grid, s, table, x_bits, y_bits, f);
    }
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_bitconv_fwd");
    return MN_OK;
}

// the launch rule of every bit / code / byte forward (qgemm_mfma_sets.h), for a caller that wants to know how a geometry is dealt: host only, nothing is launched
extern "C" int mn_deploy_grid_rows(int bx, int units) {
    if (bx < 1 || units < 1) MN_FAIL(MN_EINVAL, "mn_deploy_grid_rows: bx and units must be at least 1");
    return mn_sets::grid_rows(bx, units);
}

extern "C" int mn_deploy_grid_deal(int bx, int units, int* per) {
    if (bx < 1 || units < 1 || !per) MN_FAIL(MN_EINVAL, "mn_deploy_grid_deal: bx and units must be at least 1, per not null");
    return mn_sets::grid_deal(bx, units, *per);
}

extern "C" int mn_bits_maxpool(const uint32_t* bits_in, int64_t N, int64_t Cw, int64_t H, int64_t W, int k, int stride, int pad, uint32_t* bits_out, mn_stream_t stream) {
    if (!bits_in || !bits_out || N <= 0 || Cw <= 0 || H <= 0 || W <= 0 || H > (1 << 15) || W > (1 << 15)) MN_FAIL(MN_EINVAL, "mn_bits_maxpool: null / empty argument");
    if ((k != 2 && k != 3) || stride != 2 || pad < 0 || pad > 1) MN_FAIL(MN_ENOTSUP, "mn_bits_maxpool: window not covered (k in {2, 3}, stride 2, padding in {0, 1}, floor mode)");
    if (H + 2 * pad < k || W + 2 * pad < k) MN_FAIL(MN_EINVAL, "mn_bits_maxpool: image smaller than the window");
    const int Ho = (int)((H + 2 * pad - k) / stride + 1), Wo = (int)((W + 2 * pad - k) / stride + 1);
    const int64_t total = N * Cw * Ho * Wo;
    if (N * Cw * H * W >= (1ll << 31)) MN_FAIL(MN_ENOTSUP, "mn_bits_maxpool: tensor too large");
    mn_set_last_kernel("k_bits_maxpool"); mn_prof_bytes(4.0 * N * Cw * H * W + 4.0 * total); mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_bits::k_bits_maxpool, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bits_in, bits_out, total, (int)H, (int)W, Ho, Wo, k,
                       stride, pad);
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_bits_maxpool");
    return MN_OK;
}

#include "qgemm_codes.h"          // mn_codes_* / mn_codeconv_*: the code-packed deployment of the k-bit blocks
#include "qgemm_codes_mfma.h"     // mn_codeconv_mfma_*: the int8-MFMA form of the 1x1 hidden code blocks
#include "qgemm_codes_mfma3.h"    // mn_codeconv_mfma3_*: the int8-MFMA form of the 3x3 hidden code blocks
#include "qgemm_bits_mfma.h"      // mn_bitconv_mfma_*: the int8-MFMA form of the 1x1 hidden bit blocks
#include "qgemm_bits_mfma3.h"     // mn_bitconv_mfma3_*: the int8-MFMA form of the 3x3 hidden bit blocks
#include "qgemm_iao8.h"           // mn_i8conv_* / mn_i8_*: the int8 deployment of the BN-folded IAO hidden blocks (byte codes, i8 MFMA)
#include "qgemm_iao8_zp.h"        // mn_i8zconv_* / mn_i8z_*: the same blocks with zero points (asymmetric quantizers)
#include "qgemm_iao8_ends.h"      // mn_i8first_* / mn_i8conv_fwd_f32: the two ends of that deployment (fp32 image in, fp32 map out)
#include "qgemm_iao8_res.h"       // mn_i8res_*: the residual stages of that deployment (strided convs, QuantAdd on bytes)
#include "qgemm_iao8_e2e.h"       // mn_i8first_fwd2 / mn_i8poolfc_*: a ResNet's two ends (two-output first conv, pooled classifier on bytes)
