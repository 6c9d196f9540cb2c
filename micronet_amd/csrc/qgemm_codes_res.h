// The residual stages of the DoReFa W2A2 code plan (mn_coderes_quant_map, mn_coderes_conv_*, mn_coderes_add_*): a ResNet BasicBlock
//   x -> conv_a (3x3, stride 1 | 2) -> bn_a -> relu -> conv_b (3x3) -> bn_b -> (+ shortcut(x)) -> relu,      shortcut = identity | bn_s(conv_s 1x1, stride 1 | 2)
// on plane maps.  Included by qgemm_bits.hip behind qgemm_codes_mfma3.h.  The plane-map counterpart of qgemm_codes_w8_res.h, with a data path of its own.
//
//   layout      : every map is pack_codes' -- int32 words [N][ceil(C/32)][2 planes][H*W], bit c & 31 of plane p in word group c >> 5 = bit p of channel c's code, tail
//                 bits 0.
//   contraction : v_mfma_i32_16x16x64_i8 (mn_mfma_i8) as an implicit GEMM over (tap, channel).  A = weight bytes 2k - 3 (M = 16 output channels), B = activation codes
//                 0 .. 3 as bytes (N = 16 pixels), spread from the two plane half-words by the multiply-and-mask of k_codeconv_mfma (spread16): acc = sum j (2k - 3), the
//                 exact integer.  The K order is tap-major in SLOTS of 16 channels, slot = tap * ceil(C/16) + chunk, four slots per k-step; the last k-step is padded
//                 with slots that read the centre tap against zero weight bytes.  A tap outside the input map, or a pixel outside the batch, reads a zero word (code
//                 0): no border mask and no correction term.  Tail channels of a 1x1 with C % 16 != 0 are tail bits of the map (code 0) against zero weight bytes.
//   decision    : NOT thresholds.  z = qa_eval<0>((float)acc, QaCh) with the [9][O] constants (alpha = fl(1/3 * 1/3), the conv's bias), the fp32 chain of the byte plan:
//                 C * taps * 9 < 2^24 makes (float)acc exact, and that bound -- not the 16-bit range of the threshold kernels -- is the range.  The add stage needs the
//                 chain itself, since its code is no threshold function of one accumulator.
//   weight table: (private layout, 16-byte aligned) 8 header words -- [0] rows whose constants fail qa_chan_finite, [1] k-steps, [2] tiles per span (4), [3] tile stride,
//                 [4] O, [5] spans, [6] 2 | 2 << 8 | 2 << 16, [7] rows with a weight off the grid (2k - 3) / 3 -- then one word per slot
//                 (dy + 1 | (dx + 1) << 2 | chunk << 4), then per SPAN (two output words = 64 channels) four tiles of
//                   [0 .. 96) alpha[16], bias[16], mean[16], invstd[16], gamma[16], beta[16];  [96 ..) per k-step 64 lanes x 16 bytes in the A-operand order of mn_mfma_i8
//                   (lane = 16 kq + row).
//                 Rows are in identity order: row r of tile i IS channel 16 i + r, so tile i fills bits 16 (i & 1) .. + 15 of output word i >> 1, and a span's four
//                 tiles fill two whole words.  Rows >= O are dead (zero weights and constants, never a bit, never stored); O = 64 .. 512 has none.
//   quant       : k_coderes_quant -- fp32 NCHW -> the plane map at the consumer's quantizer qa_code(a, fl(1/3)), in one launch.  One thread = one (image, word group,
//                 pixel): per channel the loads of a wave are 64 consecutive floats, the two plane words are built in registers and stored once, whole; tail channels
//                 write 0 bits.  It replaces k_qa_fwd + mn_codes_pack_planes behind the stem.
//   conv        : k_coderes_conv<KS, STRIDE> -- conv_a -> bn_a -> relu -> 2-bit code, planes in, planes out; output pixel (h, w) reads input pixel (s h + dy, s w + dx).
//   add         : k_coderes_add<KS, SC> -- the block's end in ONE launch: z = chain_b(acc_b), r = SC == 1 ? res_f32[n][o][p] : chain_s(acc_s), a = relu(z + r); writes the
//                 next block's planes and / or a itself into an fp32 NCHW map; an output that is not requested is not touched.
//     work split  : a wave owns 64 pixels as four N tiles and one span at a time: the four M tiles of the span run with the k-steps outermost, so the four B operands are
//                   spread ONCE per k-step for 64 output channels and the weight bytes stream from the L2-resident table.  grid.x = blocks of four waves (256 pixels),
//                   grid.y deals the spans round-robin.  The waves of a block share nothing: no block barrier.
//     SC == 2     : the shortcut's K is short (ceil(C_in/16) slots).  It runs FIRST into the 16 accumulators of the span and is collapsed at once to fp32 r; only then
//                   the branch loop starts into the same registers: two int32 accumulator sets are never live together.
//     SC == 1     : the lane's residual loads are issued in front of the branch k-loop and land behind it; for a fixed channel the 16 lanes of an N tile read 16
//                   consecutive pixels (one 64-byte segment).
//     LDS         : per wave an image [2 words][2 planes][64 pixels] (1 KB; 4 KB per block).  The lane's 16 code bits of an N tile (four rows of four tiles) are merged
//                   in registers, ORed over the four kq lanes of a pixel by two wave shuffles, and the kq == 0 lane writes the finished word: every image word is
//                   written whole, once per span, so the image needs no clearing and no LDS atomic.  Behind a wave barrier lane l reads the words of pixel l.
//     stores      : every output plane word is stored exactly once, whole, coalesced along pixels -- one (span, pixel) has one owner wave, and a word >= ceil(O/32) is
//                   not stored.  The fp32 map is stored DIRECTLY from the accumulator layout: for a fixed (tile, row, N tile) the 16 lanes of a kq group store 16
//                   consecutive pixels of one channel, whole 64-byte segments, each element once.  No atomics, no read-modify-write on global memory.
// Covered: a_in = w_bits = a_out = 2; groups 1, dilation 1, no in_shuffle; 3x3 / padding 1 with C % 16 == 0 or 1x1 / padding 0 with any C; stride 1 | 2 (both directions
// equal); any O; C * taps * 9 < 2^24.  The add stage: shortcut 1 | 2, the branch conv at stride 1; an identity shortcut needs O == C; a conv shortcut is 1x1 / padding 0
// with the branch's N and O and an output map of the branch's size.
#pragma once
#include "qgemm_codes_mfma3.h"

namespace mn_coderes {

using mn_codes_mfma::spread16;
enum { HDR = 8, THDR = 96, STEPW = 256, MB = 4 };          // header words, constants of a tile, words of a k-step, M tiles of a span

struct RGeom {
    int N, C, H, W, O, KS, stride, Ho, Wo;
    int Cw, OW;                                    // word groups of the input / output map
    int chunks, nslots, nsteps, nspans, tstride, tiles_off;
};

static inline bool make_rgeom(const mn_conv_geom* g, int a_in, int w_bits, int a_out, RGeom& m) {
    if (!g || g->N <= 0 || g->C <= 0 || g->H <= 0 || g->W <= 0 || g->O <= 0) return false;
    if (a_in != 2 || w_bits != 2 || a_out != 2) return false;
    if (g->KH != g->KW || (g->KH != 1 && g->KH != 3)) return false;
    const int pad = (g->KH - 1) / 2;
    if (g->stride_h != g->stride_w || (g->stride_h != 1 && g->stride_h != 2)) return false;
    if (g->dil_h != 1 || g->dil_w != 1 || g->pad_h != pad || g->pad_w != pad || g->groups != 1 || g->in_shuffle != 0) return false;
    if ((g->C & 15) && g->KH != 1) return false;
    const int taps = g->KH * g->KW;
    if ((int64_t)g->C * taps * 9 >= (1ll << 24)) return false;          // |acc| <= C taps 3 * 3: (float)acc is exact
    m.N = g->N; m.C = g->C; m.H = g->H; m.W = g->W; m.O = g->O; m.KS = g->KH; m.stride = g->stride_h;
    m.Ho = (g->H - 1) / m.stride + 1; m.Wo = (g->W - 1) / m.stride + 1;          // (H + 2 pad - KS) / stride + 1 of either form
    m.Cw = (g->C + 31) >> 5; m.OW = (g->O + 31) >> 5;
    m.chunks = (g->C + 15) >> 4;
    m.nslots = taps * m.chunks;
    m.nsteps = (m.nslots + 3) >> 2;
    m.nspans = (m.OW + 1) >> 1;
    m.tstride = THDR + STEPW * m.nsteps;
    m.tiles_off = HDR + 4 * m.nsteps;
    if ((int64_t)m.tiles_off + (int64_t)m.nspans * MB * m.tstride >= (1ll << 30)) return false;
    const int64_t win = (int64_t)g->N * m.Cw * 2 * g->H * g->W, wout = (int64_t)g->N * m.OW * 2 * m.Ho * m.Wo;          // plane words: indexed in int
    return win < (1ll << 30) && wout < (1ll << 30);          // (the fp32 maps are indexed in int64)
}
static inline int64_t table_words(const RGeom& m) { return (int64_t)m.tiles_off + (int64_t)m.nspans * MB * m.tstride; }

// ---------------------------------------------------------------- weight table
// the two counters of the header, zeroed in front of the packer's atomics
__global__ __launch_bounds__(64) void k_coderes_clear(uint32_t* __restrict__ tab) {
    if (threadIdx.x < HDR) tab[threadIdx.x] = 0u;
}

// one block per tile: channels 16 tile .. 16 tile + 15
__global__ __launch_bounds__(256) void k_coderes_wpack(RGeom m, const float* __restrict__ w, const float* __restrict__ chan, uint32_t* __restrict__ tab) {
    __shared__ int s_off[16];
    const int tile = blockIdx.x, tid = threadIdx.x, taps = m.KS * m.KS;
    if (tile == 0) {
        for (int i = tid; i < 4 * m.nsteps; i += 256) {
            const bool real = i < m.nslots;
            const int tap = real ? i / m.chunks : 0, chunk = real ? i - tap * m.chunks : 0;
            const int dy = (m.KS == 1 || !real) ? 1 : tap / 3, dx = (m.KS == 1 || !real) ? 1 : tap % 3;          // a padding slot: the centre tap against zero bytes
            tab[HDR + i] = (uint32_t)(dy | (dx << 2) | (chunk << 4));
        }
        if (tid == 0) {
            tab[1] = (uint32_t)m.nsteps; tab[2] = (uint32_t)MB; tab[3] = (uint32_t)m.tstride; tab[4] = (uint32_t)m.O; tab[5] = (uint32_t)m.nspans;
            tab[6] = (uint32_t)(2 | (2 << 8) | (2 << 16));
        }
    }
    uint32_t* T = tab + m.tiles_off + (int64_t)tile * m.tstride;
    for (int i = tid; i < m.tstride; i += 256) T[i] = 0u;          // dead rows, tail channels and padding slots: zero constants, zero weight bytes
    if (tid < 16) s_off[tid] = 0;
    __syncthreads();
    // weight bytes 2k - 3, k = (3 w + 3) / 2: thread = 4 consecutive channels of one row at one tap, one dword of the A operand (lane 16 (slot & 3) + row of k-step
    // slot >> 2)
    const int dpr = m.nslots * 4;          // dwords per row
    for (int idx = tid; idx < 16 * dpr; idx += 256) {
        const int row = idx / dpr, d = idx - row * dpr, slot = d >> 2, e4 = d & 3;
        const int o = tile * 16 + row;
        if (o >= m.O) continue;
        const int tap = slot / m.chunks, c0 = (slot - tap * m.chunks) * 16 + e4 * 4;
        if (c0 >= m.C) continue;
        const float* wr = w + ((int64_t)o * m.C + c0) * taps + tap;          // [O][C][taps]
        uint32_t v = 0u;
        int off = 0;
        for (int e = 0; e < 4 && c0 + e < m.C; ++e) {
            const float kf = (wr[e * taps] * 3.f + 3.f) * 0.5f;          // w = (2k - 3) / 3
            const float kr = rintf(kf);
            if (!(fabsf(kf - kr) <= 1e-3f) || kr < 0.f || kr > 3.f) off = 1;
            const int kc = (int)(kr < 0.f ? 0.f : kr > 3.f ? 3.f : kr == kr ? kr : 0.f);
            v |= ((uint32_t)(2 * kc - 3) & 0xffu) << (8 * e);
        }
        if (off) s_off[row] = 1;
        T[THDR + (slot >> 2) * STEPW + ((slot & 3) * 16 + row) * 4 + e4] = v;
    }
    // the row constants of the forward chain
    if (tid < 16 && tile * 16 + tid < m.O) {
        const int o = tile * 16 + tid;
        for (int j = 0; j < 6; ++j) T[16 * j + tid] = mn_f2u(chan[(int64_t)j * m.O + o]);
        if (!qa_chan_finite(qa_load_ch(chan, m.O, o))) atomicAdd(tab + 0, 1u);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t nbad = 0;
        for (int i = 0; i < 16; ++i) nbad += (uint32_t)(s_off[i] != 0);
        if (nbad) atomicAdd(tab + 7, nbad);
    }
}

// ---------------------------------------------------------------- fp32 NCHW -> the plane map at the consumer's 2-bit quantizer
// one thread = one (image, word group, pixel): 32 channels of a pixel (reads coalesced along pixels per channel), the two plane words stored once, whole
__global__ __launch_bounds__(256) void k_coderes_quant(const float* __restrict__ x, uint32_t* __restrict__ out, int64_t total, int C, int Cw, int HW, float s) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int pix = (int)(i % HW);
    const int64_t t = i / HW;
    const int wg = (int)(t % Cw);
    const int64_t nimg = t / Cw;
    uint32_t p0 = 0u, p1 = 0u;
#pragma unroll 8
    for (int d = 0; d < 32; ++d) {
        const int c = wg * 32 + d;
        const uint32_t j = c < C ? qa_code(x[(nimg * C + c) * HW + pix], s) : 0u;          // tail channels: 0 bits
        p0 |= (j & 1u) << d;
        p1 |= ((j >> 1) & 1u) << d;
    }
    uint32_t* const o = out + (t * 2) * HW + pix;
    o[0] = p0;
    o[HW] = p1;
}

// ---------------------------------------------------------------- the contraction of one span, shared by the three uses below
// the map a contraction reads and its k-steps
struct RSrc {
    int Cw, H, W, nsteps;
};

// the lane's output pixel of every N tile and the input pixel under its centre tap: ph / pw = row and column in the INPUT map (stride h, stride w; a pixel outside
// the batch has row -4: every tap is outside), xoff = plane 0 of word group 0 at that pixel.  HWo / Wo: the output map.
__device__ __forceinline__ void res_pixels(int stride, int total, int pb, int n, int Cw, int H, int W, int HWo, int Wo, int (&ph)[4], int (&pw)[4], int (&xoff)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = pb + 16 * t + n;
        const int pc = p < total ? p : 0;
        const int im = pc / HWo, r = pc - im * HWo;
        const int h = r / Wo, wc = r - h * Wo;
        ph[t] = p < total ? stride * h : -4; pw[t] = stride * wc;
        xoff[t] = im * Cw * 2 * H * W + stride * h * W + stride * wc;
    }
}

// acc[mt][t] = the 16 rows of the span's tile mt against the 16 pixels of N tile t, over every k-step.  The k-steps run outermost: lane (n, kq) loads the two plane
// words of slot 4 s + kq at its four pixels and spreads its half-word to 16 code bytes once for the four tiles.
__device__ __forceinline__ void span_acc(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ tiles, int tstride, const uint32_t* __restrict__ x, const RSrc& q,
                                         int lane, int kq, const int (&ph)[4], const int (&pw)[4], const int (&xoff)[4], i32x4 (&acc)[MB][4]) {
    const int HW = q.H * q.W;
#pragma unroll
    for (int mt = 0; mt < MB; ++mt)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[mt][t] = i32x4{0, 0, 0, 0};
    const uint32_t* ap = tiles + THDR + lane * 4;
#pragma unroll 1
    for (int s = 0; s < q.nsteps; ++s) {
        const uint32_t sl = tab[HDR + 4 * s + kq];
        const int dy = (int)(sl & 3u) - 1, dx = (int)((sl >> 2) & 3u) - 1, chunk = (int)(sl >> 4);
        const bool real = (chunk >> 1) < q.Cw;          // (a word group past the map is never addressed, whatever the table says)
        const int woff = (chunk >> 1) * 2 * HW + dy * q.W + dx, sh = 16 * (chunk & 1);
        u32x4 b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            uint32_t p0 = 0u, p1 = 0u;          // outside the map or the batch: the zero word, code 0
            if (real && (unsigned)(ph[t] + dy) < (unsigned)q.H && (unsigned)(pw[t] + dx) < (unsigned)q.W) {
                const uint32_t* xp = x + xoff[t] + woff;
                p0 = xp[0]; p1 = xp[HW];
            }
            b[t] = spread16((p0 >> sh) & 0xffffu, (p1 >> sh) & 0xffffu);
        }
#pragma unroll
        for (int mt = 0; mt < MB; ++mt) {
            const u32x4 a = *reinterpret_cast<const u32x4*>(ap + mt * tstride + s * STEPW);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[mt][t] = mn_mfma_i8(a, b[t], acc[mt][t]);
        }
    }
}

// the forward-chain constants of the lane's rows 4 kq .. 4 kq + 3 of a tile (D[row = 4 kq + reg][col = n])
struct RowCh {
    f32x4 ch[6];
};
__device__ __forceinline__ RowCh load_rows(const uint32_t* __restrict__ tile, int kq) {
    RowCh c;
#pragma unroll
    for (int j = 0; j < 6; ++j) c.ch[j] = *reinterpret_cast<const f32x4*>(tile + 16 * j + 4 * kq);
    return c;
}
// z of row r on the exact accumulator
__device__ __forceinline__ float row_z(const RowCh& c, int r, int acc) {
    QaCh k;
    k.alpha = c.ch[0][r]; k.bias = c.ch[1][r]; k.mean = c.ch[2][r]; k.invstd = c.ch[3][r]; k.ga = c.ch[4][r]; k.be = c.ch[5][r];
    k.A = k.B = k.gi = 0.f;          // (not part of the forward chain)
    float zh, z;
    qa_eval<0>((float)acc, k, zh, z);
    return z;
}

// The span's plane words of the lane's rows: pl[2 word + plane][t] collects bit `pos` of tile mt's row r.  merge_store ORs them over the four kq lanes of a pixel
// (every lane of the wave takes part), the kq == 0 lane writes the finished words into the wave's image, and behind a wave barrier lane l stores the four words of
// pixel pb + l: each once, whole, coalesced along pixels.
__device__ __forceinline__ void put_code(uint32_t (&pl)[4][4], int mt, int pos, int t, uint32_t code) {
    pl[2 * (mt >> 1)][t] |= (code & 1u) << pos;
    pl[2 * (mt >> 1) + 1][t] |= ((code >> 1) & 1u) << pos;
}
__device__ __forceinline__ void merge_store(uint32_t (&pl)[4][4], uint32_t* __restrict__ img, uint32_t* __restrict__ ybase, int lane, int n, int kq, int span, int OW,
                                            int HWo, bool sok) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            uint32_t v = pl[i][t];
            v |= (uint32_t)__shfl_xor((int)v, 16, 64);
            v |= (uint32_t)__shfl_xor((int)v, 32, 64);
            if (kq == 0) img[i * 64 + 16 * t + n] = v;
        }
    MN_WAVE_SYNC();          // every word of the span is in the image
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t v = img[i * 64 + lane];
        const int word = 2 * span + (i >> 1);
        if (sok && word < OW) ybase[(int64_t)(word * 2 + (i & 1)) * HWo] = v;
    }
    MN_WAVE_SYNC();          // ... and read back before the next span writes into it
}

struct RFwd {
    RSrc b;
    int total, Ho, Wo, O, OW, nspans, tstride, tiles_off;
    float s;          // fl(1 / 3), the step of the consumer's quantizer
};

// ---------------------------------------------------------------- conv_a: planes in, planes out, stride 1 | 2
template <int KS, int STRIDE>
__global__ __launch_bounds__(256) void k_coderes_conv(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, uint32_t* __restrict__ y, RFwd q) {
    __shared__ uint32_t s_img[4][4 * 64];          // per wave: [2 words][2 planes][64 pixels]
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HWo = q.Ho * q.Wo;
    const int pb = ((int)blockIdx.x * 4 + wave) * 64;
    int ph[4], pw[4], xoff[4];
    res_pixels(STRIDE, q.total, pb, n, q.b.Cw, q.b.H, q.b.W, HWo, q.Wo, ph, pw, xoff);
    // what this lane stores: the words of output pixel pb + lane
    const int ps = pb + lane;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HWo;
    uint32_t* const ybase = y + (int64_t)simg * q.OW * 2 * HWo + (psc - simg * HWo);
    for (int span = (int)blockIdx.y; span < q.nspans; span += (int)gridDim.y) {
        const uint32_t* tiles = tab + q.tiles_off + (int64_t)span * MB * q.tstride;
        i32x4 acc[MB][4];
        span_acc(tab, tiles, q.tstride, x, q.b, lane, kq, ph, pw, xoff, acc);
        uint32_t pl[4][4] = {};
#pragma unroll
        for (int mt = 0; mt < MB; ++mt) {
            const RowCh c = load_rows(tiles + mt * q.tstride, kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (span * 64 + mt * 16 + 4 * kq + r >= q.O) continue;          // a dead row: no bit
#pragma unroll
                for (int t = 0; t < 4; ++t) put_code(pl, mt, 16 * (mt & 1) + 4 * kq + r, t, qa_code(qa_relu(row_z(c, r, acc[mt][t][r])), q.s));
            }
        }
        merge_store(pl, s_img[wave], ybase, lane, n, kq, span, q.OW, HWo, sok);
    }
}

// ---------------------------------------------------------------- conv_b -> bn_b -> + shortcut -> relu -> planes and / or fp32
struct RAdd {
    RFwd b;                  // the branch: stride 1, Ho = H, Wo = W
    // SC == 2: conv_s on the block input's plane map, and its table's layout
    RSrc s;
    int s_stride, s_tstride, s_tiles_off;
};

template <int KS, int SC>
__global__ __launch_bounds__(256) void k_coderes_add(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, const uint32_t* __restrict__ tab_s,
                                                     const uint32_t* __restrict__ xs, const float* __restrict__ res, uint32_t* __restrict__ yp, float* __restrict__ yf,
                                                     RAdd p) {
    static_assert(SC == 1 || SC == 2, "the shortcut is the identity (1) or a conv (2)");
    __shared__ uint32_t s_img[4][4 * 64];          // per wave: [2 words][2 planes][64 pixels]
    const RFwd& q = p.b;
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HW = q.b.H * q.b.W;          // (stride 1: the output map is the branch's input map)
    const int pb = ((int)blockIdx.x * 4 + wave) * 64;
    int ph[4], pw[4], xoff[4];
    res_pixels(1, q.total, pb, n, q.b.Cw, q.b.H, q.b.W, HW, q.b.W, ph, pw, xoff);
    int sph[4], spw[4], sxoff[4];          // SC == 2: the same pixels in the block input's map
    if (SC == 2) res_pixels(p.s_stride, q.total, pb, n, p.s.Cw, p.s.H, p.s.W, HW, q.b.W, sph, spw, sxoff);
    int64_t foff[4];          // channel 0 of the fp32 maps at the pixel of N tile t, -1 outside the batch
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int pp = pb + 16 * t + n;
        const int pc = pp < q.total ? pp : 0, im = pc / HW;
        foff[t] = pp < q.total ? (int64_t)im * q.O * HW + (pc - im * HW) : -1;
    }
    const int ps = pb + lane;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HW;
    uint32_t* const ybase = yp + (int64_t)simg * q.OW * 2 * HW + (psc - simg * HW);
    for (int span = (int)blockIdx.y; span < q.nspans; span += (int)gridDim.y) {
        const uint32_t* tiles = tab + q.tiles_off + (int64_t)span * MB * q.tstride;
        const int o0 = span * 64 + 4 * kq;          // the lane's row 0 of tile 0
        i32x4 acc[MB][4];
        float rr[MB][4][4];          // r of (tile, N tile, row)
        if (SC == 2) {
            const uint32_t* tiles_s = tab_s + p.s_tiles_off + (int64_t)span * MB * p.s_tstride;
            span_acc(tab_s, tiles_s, p.s_tstride, xs, p.s, lane, kq, sph, spw, sxoff, acc);
#pragma unroll
            for (int mt = 0; mt < MB; ++mt) {
                const RowCh cs = load_rows(tiles_s + mt * p.s_tstride, kq);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) rr[mt][t][r] = row_z(cs, r, acc[mt][t][r]);
            }
        } else {
#pragma unroll
            for (int mt = 0; mt < MB; ++mt)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = o0 + 16 * mt + r;
                        rr[mt][t][r] = (o < q.O && foff[t] >= 0) ? res[foff[t] + (int64_t)o * HW] : 0.f;
                    }
        }
        span_acc(tab, tiles, q.tstride, x, q.b, lane, kq, ph, pw, xoff, acc);
        uint32_t pl[4][4] = {};
#pragma unroll
        for (int mt = 0; mt < MB; ++mt) {
            const RowCh c = load_rows(tiles + mt * q.tstride, kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = o0 + 16 * mt + r;
                if (o >= q.O) continue;          // a dead row: no bit, nothing stored
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float a = qa_relu(row_z(c, r, acc[mt][t][r]) + rr[mt][t][r]);          // the op order of k_qr_fwd: two rounded values, then their sum
                    if (yf && foff[t] >= 0) yf[foff[t] + (int64_t)o * HW] = a;
                    put_code(pl, mt, 16 * (mt & 1) + 4 * kq + r, t, qa_code(a, q.s));
                }
            }
        }
        if (yp) merge_store(pl, s_img[wave], ybase, lane, n, kq, span, q.OW, HW, sok);          // (kernel-uniform)
    }
}

// [a, a + na) and [b, b + nb) share a byte
static inline bool ranges_meet(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

// the geometries of an add stage: the branch at stride 1; shortcut 1: O == C; shortcut 2: a 1x1 conv with the branch's N, O and output size
static inline bool make_ageom(const mn_conv_geom* g, int shortcut, const mn_conv_geom* gs, int a_in, int w_bits, int a_out, RGeom& r, RGeom& rs) {
    if (shortcut != 1 && shortcut != 2) return false;
    if (!make_rgeom(g, a_in, w_bits, a_out, r) || r.stride != 1) return false;
    if (shortcut == 1 && g->O != g->C) return false;
    if (shortcut == 2) {
        if (!make_rgeom(gs, a_in, w_bits, a_out, rs) || rs.KS != 1) return false;
        if (rs.N != r.N || rs.O != r.O || rs.Ho != r.H || rs.Wo != r.W) return false;
    }
    return true;
}

static inline void make_rfwd(const RGeom& m, RFwd& f) {
    f.b.Cw = m.Cw; f.b.H = m.H; f.b.W = m.W; f.b.nsteps = m.nsteps;
    f.Ho = m.Ho; f.Wo = m.Wo; f.O = m.O; f.OW = m.OW; f.nspans = m.nspans; f.tstride = m.tstride; f.tiles_off = m.tiles_off;
    f.total = m.N * m.Ho * m.Wo;
    f.s = 1.0f / 3.0f;
}

}  // namespace mn_coderes

// (passed as an argument of "%s", never as a format)
#define MN_CODERES_COVER "geometry or width not covered (2-bit codes and weights throughout; groups 1, dilation 1, no in_shuffle, 1x1 / padding 0 with any C or 3x3 / padding 1 with C % 16 == 0, stride 1 or 2 in both directions, C * taps * 9 < 2^24)"

extern "C" int mn_coderes_quant_map(const float* x, int64_t N, int64_t C, int64_t HW, uint32_t* planes, mn_stream_t stream) {
    if (!x || !planes || ((((uintptr_t)x) | ((uintptr_t)planes)) & 3) || N <= 0 || C <= 0 || HW <= 0)
        MN_FAIL(MN_EINVAL, "mn_coderes_quant_map: null / empty argument, or a pointer that is not 4-byte aligned");
    const int64_t Cw = (C + 31) / 32;
    if (C >= (1ll << 24) || HW >= (1ll << 30) || N * Cw * 2 * HW >= (1ll << 30)) MN_FAIL(MN_ENOTSUP, "mn_coderes_quant_map: tensor too large");
    const int64_t total = N * Cw * HW;
    mn_set_last_kernel("k_coderes_quant");
    mn_prof_bytes(4.0 * N * C * HW + 8.0 * (double)total);
    mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_coderes::k_coderes_quant, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, planes, total, (int)C, (int)Cw, (int)HW,
                       1.0f / 3.0f);
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_coderes_quant_map");
    return MN_OK;
}

extern "C" int mn_coderes_conv_supported(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_coderes::RGeom r;
    return mn_coderes::make_rgeom(g, a_bits_in, w_bits, a_bits_out, r) ? 1 : 0;
}

extern "C" int64_t mn_coderes_conv_table_bytes(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_coderes::RGeom r;
    if (!mn_coderes::make_rgeom(g, a_bits_in, w_bits, a_bits_out, r)) return 0;
    return 4 * mn_coderes::table_words(r);
}

extern "C" int mn_coderes_conv_pack(const mn_conv_geom* g, const float* w, const float* chan, int a_bits_in, int w_bits, int a_bits_out, uint32_t* table,
                                    mn_stream_t stream) {
    mn_coderes::RGeom r;
    if (!w || !chan || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)chan) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_coderes_conv_pack: null / unaligned argument (the table is 16-byte aligned) or invalid geometry");
    if (!mn_coderes::make_rgeom(g, a_bits_in, w_bits, a_bits_out, r)) MN_FAIL(MN_ENOTSUP, "mn_coderes_conv_pack: %s", MN_CODERES_COVER);
    mn_set_last_kernel("k_coderes_wpack");
    hipLaunchKernelGGL(mn_coderes::k_coderes_clear, dim3(1), dim3(64), 0, (hipStream_t)stream, table);
    hipLaunchKernelGGL(mn_coderes::k_coderes_wpack, dim3(r.nspans * mn_coderes::MB), dim3(256), 0, (hipStream_t)stream, r, w, chan, table);
    MN_CHECK_LAUNCH("mn_coderes_conv_pack");
    return MN_OK;
}

extern "C" int mn_coderes_conv_fwd(const mn_conv_geom* g, const uint32_t* table, const uint32_t* in_planes, uint32_t* out_planes, mn_stream_t stream) {
    mn_coderes::RGeom r;
    if (!table || !in_planes || !out_planes || !aligned16(table) || ((((uintptr_t)in_planes) | ((uintptr_t)out_planes)) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_coderes_conv_fwd: null / unaligned argument (the table is 16-byte, the plane maps 4-byte aligned) or invalid geometry");
    if (!mn_coderes::make_rgeom(g, 2, 2, 2, r)) MN_FAIL(MN_ENOTSUP, "mn_coderes_conv_fwd: %s", MN_CODERES_COVER);
    const int64_t nin = 8ll * r.N * r.Cw * r.H * r.W, nout = 8ll * r.N * r.OW * r.Ho * r.Wo;
    if (mn_coderes::ranges_meet(out_planes, nout, in_planes, nin)) MN_FAIL(MN_EINVAL, "mn_coderes_conv_fwd: the output overlaps the input");
    mn_coderes::RFwd f;
    mn_coderes::make_rfwd(r, f);
    const int bx = (f.total + 255) / 256;          // four waves of four N tiles
    const dim3 grid(bx, mn_sets::grid_rows(bx, r.nspans));          // the spans round-robin over grid.y
    const hipStream_t s = (hipStream_t)stream;
    mn_set_last_kernel("k_coderes_conv<%d,%d>", r.KS, r.stride);
    mn_prof_bytes((double)nin + (double)nout + 4.0 * (double)mn_coderes::table_words(r));
    mn_prof_begin(s);
    if (r.KS == 3) {
        if (r.stride == 2) hipLaunchKernelGGL((mn_coderes::k_coderes_conv<3, 2>), grid, dim3(256), 0, s, table, in_planes, out_planes, f);
        else hipLaunchKernelGGL((mn_coderes::k_coderes_conv<3, 1>), grid, dim3(256), 0, s, table, in_planes, out_planes, f);
    } else {
        if (r.stride == 2) hipLaunchKernelGGL((mn_coderes::k_coderes_conv<1, 2>), grid, dim3(256), 0, s, table, in_planes, out_planes, f);
        else hipLaunchKernelGGL((mn_coderes::k_coderes_conv<1, 1>), grid, dim3(256), 0, s, table, in_planes, out_planes, f);
    }
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_coderes_conv_fwd");
    return MN_OK;
}

extern "C" int mn_coderes_add_supported(const mn_conv_geom* g, int shortcut, const mn_conv_geom* gs, int a_bits_in, int w_bits, int a_bits_out) {
    mn_coderes::RGeom r, rs;
    return mn_coderes::make_ageom(g, shortcut, gs, a_bits_in, w_bits, a_bits_out, r, rs) ? 1 : 0;
}

extern "C" int mn_coderes_add_fwd(const mn_conv_geom* g, const uint32_t* table, const uint32_t* in_planes, int shortcut, const float* res_f32, const mn_conv_geom* gs,
                                  const uint32_t* table_s, const uint32_t* sc_planes, uint32_t* out_planes, float* out_f32, mn_stream_t stream) {
    mn_coderes::RGeom r, rs;
    if (!table || !in_planes || !aligned16(table) || ((((uintptr_t)in_planes) | ((uintptr_t)out_planes) | ((uintptr_t)out_f32)) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_coderes_add_fwd: null / unaligned argument (tables are 16-byte, plane and fp32 maps 4-byte aligned) or invalid geometry");
    if (!out_planes && !out_f32) MN_FAIL(MN_EINVAL, "mn_coderes_add_fwd: no output requested (out_planes and out_f32 are both null)");
    if (shortcut == 1 && (!res_f32 || (((uintptr_t)res_f32) & 3))) MN_FAIL(MN_EINVAL, "mn_coderes_add_fwd: the identity shortcut needs res_f32 (4-byte aligned)");
    if (shortcut == 2 && (!table_s || !sc_planes || !aligned16(table_s) || (((uintptr_t)sc_planes) & 3) || !tile_geom_valid(gs)))
        MN_FAIL(MN_EINVAL, "mn_coderes_add_fwd: the conv shortcut needs its geometry, table (16-byte aligned) and input map (4-byte aligned)");
    if (!mn_coderes::make_ageom(g, shortcut, gs, 2, 2, 2, r, rs))
        MN_FAIL(MN_ENOTSUP, "mn_coderes_add_fwd: %s; the add stage: shortcut 1 / 2, the branch conv at stride 1, an identity shortcut with O == C, a conv shortcut "
                            "1x1 / padding 0 with the branch's N and O and an output map of the branch's size", MN_CODERES_COVER);
    const int64_t nin = 8ll * r.N * r.Cw * r.H * r.W, nout = 8ll * r.N * r.OW * r.H * r.W, nf = 4ll * r.N * r.O * r.H * r.W;
    const int64_t nsc = shortcut == 2 ? 8ll * rs.N * rs.Cw * rs.H * rs.W : 0;
    const void* const ins[3] = {in_planes, shortcut == 1 ? (const void*)res_f32 : nullptr, shortcut == 2 ? (const void*)sc_planes : nullptr};
    const int64_t nins[3] = {nin, nf, nsc};
    for (int k = 0; k < 3; ++k)
        if (mn_coderes::ranges_meet(out_planes, nout, ins[k], nins[k]) || mn_coderes::ranges_meet(out_f32, nf, ins[k], nins[k]))
            MN_FAIL(MN_EINVAL, "mn_coderes_add_fwd: an output overlaps an input");
    if (mn_coderes::ranges_meet(out_planes, nout, out_f32, nf)) MN_FAIL(MN_EINVAL, "mn_coderes_add_fwd: the two outputs overlap");
    mn_coderes::RAdd p;
    mn_coderes::make_rfwd(r, p.b);
    p.s.Cw = p.s.H = p.s.W = p.s.nsteps = 0;
    p.s_stride = 1; p.s_tstride = p.s_tiles_off = 0;
    if (shortcut == 2) {
        p.s.Cw = rs.Cw; p.s.H = rs.H; p.s.W = rs.W; p.s.nsteps = rs.nsteps;
        p.s_stride = rs.stride; p.s_tstride = rs.tstride; p.s_tiles_off = rs.tiles_off;
    }
    const int bx = (p.b.total + 255) / 256;          // four waves of four N tiles
    const dim3 grid(bx, mn_sets::grid_rows(bx, r.nspans));          // the spans round-robin over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t* xsc = shortcut == 2 ? sc_planes : nullptr;
    const uint32_t* ts = shortcut == 2 ? table_s : nullptr;
    const float* rf = shortcut == 1 ? res_f32 : nullptr;
    mn_set_last_kernel("k_coderes_add<%d,%d>", r.KS, shortcut);
    mn_prof_bytes((double)nin + (double)nsc + (shortcut == 1 ? (double)nf : 0.0) + (out_planes ? (double)nout : 0.0) + (out_f32 ? (double)nf : 0.0) +
                  4.0 * (double)mn_coderes::table_words(r) + (shortcut == 2 ? 4.0 * (double)mn_coderes::table_words(rs) : 0.0));
    mn_prof_begin(s);
#define MN_CODERES_ADD(KS, SC) hipLaunchKernelGGL((mn_coderes::k_coderes_add<KS, SC>), grid, dim3(256), 0, s, table, in_planes, ts, xsc, rf, out_planes, out_f32, p)
    if (r.KS == 3) {
        if (shortcut == 2) MN_CODERES_ADD(3, 2); else MN_CODERES_ADD(3, 1);
    } else {
        if (shortcut == 2) MN_CODERES_ADD(1, 2); else MN_CODERES_ADD(1, 1);
    }
#undef MN_CODERES_ADD
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_coderes_add_fwd");
    return MN_OK;
}
#undef MN_CODERES_COVER
