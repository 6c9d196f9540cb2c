// The byte form of the DoReFa W8A8 hidden block (mn_code8conv_*, mn_code8_*): byte maps in, byte maps out, one kernel per hidden stage
//   [channel shuffle] -> QuantConv2d (stored weights on the grid (2k - 255) / 255) -> BatchNorm -> ReLU -> [2x2 max-pool] -> the next conv's 8-bit activation quantizer.
// Included by qgemm_bits.hip behind the code headers (whose route into both builds it shares).  Neither the planes nor the thresholds of the 2 / 4-bit forms stretch to
// 8 bits (255 thresholds per channel over a range of 2e9), and neither operand fits a signed byte as it is: activation codes j are 0 .. 255, weights the odd integers
// 2k - 255 in [-255, 255].  So both are stored with an offset and the block's fp32 chain is evaluated on the exact int32 sum.
//
//   identity     : with a = j - 128 and w' = k - 128 (both int8), j (2k - 255) = (a + 128)(2 w' + 1) = 2 a w' + a + 256 w' + 128, so over the T (tap, channel)
//                  positions of an output      acc = sum j (2k - 255) = 2 sum a w' + sum a + Kc[o],      Kc[o] = 256 sum w'[o] + 128 T.
//                  sum a w' comes from v_mfma_i32_16x16x64_i8, sum a from byte-wise dot products of the B operands the lane already holds against 0x01010101
//                  (v_dot4_i32_i8), Kc from the packer.  A position whose activation byte is 0x80 (a = -128, the code 0) contributes (a + 128)(2 w' + 1) = 0 whatever
//                  its weight byte, which settles every edge by ONE rule:
//                    - a tap outside the map reads as 0x80 bytes: zero padding needs no mask;
//                    - the tail channels of a 16-channel block are 0x80 by layout (k_code8_pack and this kernel write them so), their weight bytes are 0, and they ARE
//                      counted into T: T = taps * ceil(Cg / 16) * 16;
//                    - the padding slots of the last k-step read NOTHING: their B operand is the zero byte (a = 0) against zero weight bytes, so they add 0 to
//                      sum a w' and 0 to sum a, and are NOT counted into T.  The slot word says which slots they are (bit 31).
//                  Every partial sum is exact in int32 when Cg * taps * 255 * 255 <= INT_MAX, i.e. Cg * taps <= 33025 (make_geom checks it); the three terms are added
//                  in unsigned arithmetic, the total lies within int32.
//   chain        : code = qa_code_of<0>((float)acc, QaCh, 1 / 255) -- the ONE copy of k_qa_fwd's chain in qa_thresholds.h, evaluated per element: no threshold table,
//                  no search.  With the folded 2x2 pool the maximum of the four sub-pixels' post-ReLU values is taken first, then the code.  Output byte = code - 128.
//   activations  : int8 [N][ceil(C/16)][H*W][16]; byte d of the 16-byte block cb at a pixel is code - 128 of channel 16 cb + d, tail channels 0x80.  One 16-byte load
//                  per lane is the B operand for 16 channels of one pixel, coalesced over the 16 pixel lanes.
//   contraction  : an implicit GEMM over (tap, channel): A = weight bytes of 16 output rows of ONE group, B = activation bytes of 16 pixels.  The K order is tap-major
//                  in SLOTS of 16 channels, slot = tap * chunks + chunk (chunks = ceil(C / groups / 16)), four slots per k-step.  A 1x1 block is the one-tap case.
//   weight table : (private layout, 16-byte aligned: the set / tile table of qgemm_mfma_sets.h, a set = four 16-byte output blocks) 16 header words -- [0] rows whose
//                  constants fail qa_chan_finite, [1] k-steps, [2] tile slots per set, [3] tile stride, [4] sets, [5] chunks, [6] 8 | 8 << 8 | 8 << 16, [7] bad
//                  out_order entries + rows with a weight off the grid, [8] T -- then one word per slot (dy + 1 | (dx + 1) << 2 | chunk << 4, bit 31: a padding slot; the 5x5 tables
//                  of qgemm_codes_w8_tile.h: dy + 2 | (dx + 2) << 3 | chunk << 6),
//                  then the tile count of every set, then the tiles:
//                    [0] first 16-channel block of the tile's group, [1] 1: first tile of its group in the set, [16 ..) the nine QaCh rows of 16 output rows each,
//                    [160 ..) Kc[16], [176 ..) dest[16] (position in the set, -1: a dead row), [192 ..) per k-step 64 lanes x 16 bytes in the A-operand order of
//                    mn_mfma_i8 (lane = 16 kq + row).
//                  A dead row: zero weights, no destination.  The bytes of positions without a row are 0x80, as the layout wants of tail channels.
//   kernel       : a wave owns 64 pixels as four N tiles (pool: the four sub-pixels of the 2x2 windows of 16 pooled pixels, so the window's maximum is taken inside a
//                  lane) and walks the tiles of a set; the weight bytes stream from the L2-resident table, the activation bytes from L1 / L2.
//                    - sum a depends on the pixel and the GROUP only.  It is formed while the first tile of a group in the set runs (four dot products per B operand
//                      in that tile's k-loop, then ONE reduction over the four kq lanes of a pixel: two shuffles per N tile) and stays in four registers for
//                      the group's other tiles, whose k-loops are loads and MFMAs alone.
//                    - the waves of a block share nothing: each assembles its set in an LDS image of its own, [4 blocks][pixels][16 bytes], filled with 0x80.  Every
//                      lane writes the code bytes of its four rows; the image is handed over inside the wave (a wave's DS operations execute in order, so a wave
//                      barrier is all it takes: no block barrier anywhere in the kernel), read back as whole 16-byte blocks and stored once, coalesced along pixels:
//                      no atomics and no read-modify-write on global memory.
// Covered: a_in = w_bits = a_out = 8; 1x1 / stride 1 / padding 0 with groups == 1 and any C, or C / groups % 16 == 0; 3x3 / stride 1 / padding 1 with
// C / groups % 16 == 0; dilation 1; any O; Cg * taps <= 33025; pool 0 / 1 (even H and W).
#pragma once
#include "qgemm_codes.h"
#include "qgemm_mfma_sets.h"
#include "qa_thresholds.h"

namespace mn_code8 {

using mn_sets::SETROWS;
using mn_sets::table_words;
enum { HDR = 16, T_CH = 16, T_KC = 160, T_DEST = 176, THDR = 192, STEPW = 256, KMAX = 33025 };
static const uint32_t PADSLOT = 0x80000000u;          // bit 31 of a slot word: a padding slot of the last k-step

struct W8Geom {
    int N, C, H, W, O, KS, groups, Cg, Og, taps;
    int CB, OB;                                   // 16-channel blocks of the input / output map
    int chunks, nslots, nsteps, nsets, slots, tstride, slot_off, cnt_off, tiles_off;
    int T;                                        // (tap, channel) positions that enter sum a: tail channels counted, padding slots not
};

static inline bool make_geom(const mn_conv_geom* g, int a_in, int w_bits, int a_out, W8Geom& m) {
    if (!g || g->N <= 0 || g->C <= 0 || g->H <= 0 || g->W <= 0 || g->O <= 0 || g->groups <= 0) return false;
    if (a_in != 8 || w_bits != 8 || a_out != 8) return false;
    if (g->KH != g->KW || (g->KH != 1 && g->KH != 3)) return false;
    const int pad = (g->KH - 1) / 2;
    if (g->stride_h != 1 || g->stride_w != 1 || g->dil_h != 1 || g->dil_w != 1 || g->pad_h != pad || g->pad_w != pad) return false;
    if (g->C % g->groups || g->O % g->groups || g->in_shuffle > 1) return false;      // a channel shuffle is folded into the PRODUCER's row order, never gathered here
    m.N = g->N; m.C = g->C; m.H = g->H; m.W = g->W; m.O = g->O; m.KS = g->KH; m.groups = g->groups;
    m.Cg = g->C / g->groups; m.Og = g->O / g->groups; m.taps = g->KH * g->KW;
    if ((m.Cg & 15) && (m.KS != 1 || m.groups != 1)) return false;          // every group starts on a 16-channel block
    if ((int64_t)m.Cg * m.taps > KMAX) return false;                        // acc and its three terms are exact in int32
    m.CB = (g->C + 15) >> 4; m.OB = (g->O + 15) >> 4;
    m.chunks = (m.Cg + 15) >> 4;
    m.nslots = m.taps * m.chunks;
    m.T = m.nslots * 16;
    m.nsteps = (m.nslots + 3) >> 2;
    m.nsets = (m.OB + 3) >> 2;
    m.tstride = THDR + STEPW * m.nsteps;
    m.slot_off = HDR;
    m.cnt_off = HDR + 4 * m.nsteps;
    if (!mn_sets::table_layout(m, m.groups, m.cnt_off)) return false;
    const int64_t blocks = (int64_t)g->N * (m.CB > m.OB ? m.CB : m.OB) * g->H * g->W;          // 16-byte blocks: indexed in int
    return blocks < (1ll << 27);
}

// acc += the four signed bytes of v
__device__ __forceinline__ int bytesum(uint32_t v, int acc) {
#ifdef MN_EMULATION
    for (int e = 0; e < 4; ++e) acc += (int)(int8_t)((v >> (8 * e)) & 0xffu);
    return acc;
#else
    return __builtin_amdgcn_sdot4((int)v, 0x01010101, acc, false);
#endif
}

// ---------------------------------------------------------------- weight table
// the two counters of the header, zeroed in front of the packer's atomics (a launch like every other: nothing here is a memset)
__global__ __launch_bounds__(64) void k_code8_clear(uint32_t* __restrict__ tab) {
    if (threadIdx.x < HDR) tab[threadIdx.x] = 0u;
}

// one block per set
__global__ __launch_bounds__(256) void k_code8_wpack(W8Geom m, const float* __restrict__ w, const float* __restrict__ chan, const int32_t* __restrict__ order,
                                                     uint32_t* __restrict__ tab) {
    __shared__ mn_sets::SetPlan sp;
    __shared__ int s_sw[SETROWS];          // sum w' of the set's rows
    const int set = blockIdx.x, tid = threadIdx.x;
    if (set == 0) {
        for (int i = tid; i < 4 * m.nsteps; i += 256) {
            const bool real = i < m.nslots;
            const int tap = real ? i / m.chunks : 0, chunk = real ? i - tap * m.chunks : 0;
            const int dy = m.KS == 1 ? 1 : tap / m.KS, dx = m.KS == 1 ? 1 : tap % m.KS;
            const int word = m.KS == 5 ? dy | (dx << 3) | (chunk << 6) : dy | (dx << 2) | (chunk << 4);          // (5x5: qgemm_codes_w8_tile.h, three bits per tap offset)
            tab[m.slot_off + i] = real ? (uint32_t)word : PADSLOT;
        }
        if (tid == 0) {
            tab[1] = (uint32_t)m.nsteps; tab[2] = (uint32_t)m.slots; tab[3] = (uint32_t)m.tstride; tab[4] = (uint32_t)m.nsets; tab[5] = (uint32_t)m.chunks;
            tab[6] = (uint32_t)(8 | (8 << 8) | (8 << 16));
            tab[8] = (uint32_t)m.T;
        }
    }
    uint32_t* tiles = tab + m.tiles_off + (int64_t)set * m.slots * m.tstride;
    // every slot starts as a tile of dead rows: zero weight bytes, zero constants, no destination
    for (int i = tid; i < m.slots * m.tstride; i += 256) {
        const int r = i % m.tstride;
        tiles[i] = (r >= T_DEST && r < T_DEST + 16) ? 0xffffffffu : 0u;
    }
    if (tid < SETROWS) s_sw[tid] = 0;
    int nt;
    const int before = mn_sets::plan_set(order, m.O, m.Og, set, tab + 7, sp, nt);
    if (tid == 0) tab[m.cnt_off + set] = (uint32_t)nt;
    // weight bytes w' = k - 128, k = (255 w + 255) / 2: thread = 4 consecutive channels of one row at one tap, one dword of the A operand (lane 16 (slot & 3) + row of
    // k-step slot >> 2).  Tail channels keep the zero byte.
    const int dpr = m.nslots * 4;          // dwords per row
    for (int idx = tid; idx < SETROWS * dpr; idx += 256) {
        const int pos = idx / dpr, d = idx - pos * dpr, slot = d >> 2, e4 = d & 3;
        const int o = sp.chan[pos];
        if (o < 0) continue;
        const int tap = slot / m.chunks, c0 = (slot - tap * m.chunks) * 16 + e4 * 4;
        if (c0 >= m.Cg) continue;
        const float* wr = w + ((int64_t)o * m.Cg + c0) * m.taps + tap;          // [O][Cg][taps]
        uint32_t v = 0u;
        int off = 0, sum = 0;
        for (int e = 0; e < 4 && c0 + e < m.Cg; ++e) {
            const float kf = (wr[e * m.taps] * 255.f + 255.f) * 0.5f;          // w = (2k - 255) / 255
            const float kr = rintf(kf);
            if (!(fabsf(kf - kr) <= 1e-3f) || kr < 0.f || kr > 255.f) off = 1;
            const int kc = (int)(kr < 0.f ? 0.f : kr > 255.f ? 255.f : kr == kr ? kr : 0.f);
            v |= ((uint32_t)(kc - 128) & 0xffu) << (8 * e);
            sum += kc - 128;
        }
        if (off) sp.off[pos] = 1;
        atomicAdd(&s_sw[pos], sum);
        uint32_t* A = tiles + (int64_t)sp.tile[pos] * m.tstride + THDR;
        A[(slot >> 2) * STEPW + ((slot & 3) * 16 + sp.row[pos]) * 4 + e4] = v;
    }
    __syncthreads();
    // the row constants
    if (tid < SETROWS && sp.chan[tid] >= 0) {
        const int o = sp.chan[tid], r = sp.row[tid];
        uint32_t* T = tiles + (int64_t)sp.tile[tid] * m.tstride;
        for (int j = 0; j < QA_NCH; ++j) T[T_CH + 16 * j + r] = mn_f2u(chan[(int64_t)j * m.O + o]);
        T[T_KC + r] = (uint32_t)(256 * s_sw[tid] + 128 * m.T);
        T[T_DEST + r] = (uint32_t)tid;
        if (!qa_chan_finite(qa_load_ch(chan, m.O, o))) atomicAdd(tab + 0, 1u);
        if (r == 0) {
            T[0] = (uint32_t)(sp.grp[tid] * m.Cg >> 4);          // (groups == 1 with any C: group 0 starts at block 0)
            T[1] = (uint32_t)((before >> 4) == 0);
        }
    }
    mn_sets::tally_off(sp, tab + 7);
}

// ---------------------------------------------------------------- MFMA contraction + sum a + Kc -> the block's chain -> output bytes
struct W8Fwd {
    int total, CB, OB, H, W, Ho, Wo, nsteps, nsets, slots, tstride, slot_off, cnt_off, tiles_off, spb;
    float s;          // 1 / 255, the step of the consumer's quantizer
};

template <int KS, bool POOL>
__global__ __launch_bounds__(256) void k_code8conv(const uint32_t* __restrict__ tab, const u32x4* __restrict__ x, u32x4* __restrict__ y, W8Fwd q) {
    constexpr int NPIX = POOL ? 16 : 64;          // output pixels of a wave
    __shared__ u32x4 s_img[4][4 * NPIX];          // per wave: [4 blocks of the set][pixels][16 bytes]
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HW = q.H * q.W, HWo = q.Ho * q.Wo;
    const int pb = ((int)blockIdx.x * 4 + wave) * NPIX;
    int ph[4], pw[4], xoff[4];          // row, column and block 0 at the pixel of N tile t; a pixel outside the batch has row -4: every tap is outside
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = POOL ? pb + n : pb + 16 * t + n;
        const int pc = p < q.total ? p : 0;
        const int im = pc / HWo, r = pc - im * HWo;
        int h = r / q.Wo, wc = r - h * q.Wo;
        if (POOL) { h = 2 * h + (t >> 1); wc = 2 * wc + (t & 1); }
        ph[t] = p < q.total ? h : -4; pw[t] = wc;
        xoff[t] = im * q.CB * HW + h * q.W + wc;
    }
    // what this lane stores: the blocks of pixel pb + lane (pool: block kq of the set at pooled pixel pb + n)
    const int ps = POOL ? pb + n : pb + lane;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HWo;
    u32x4* const ybase = y + (int64_t)simg * q.OB * HWo + (psc - simg * HWo);
    u32x4* const img = s_img[wave];
    int8_t* const imgb = reinterpret_cast<int8_t*>(img);
    const u32x4 fill = u32x4{0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};          // sixteen codes 0
    for (int i = lane; i < 4 * NPIX; i += 64) img[i] = fill;
    int sa[4] = {0, 0, 0, 0};          // sum a of the current group at the pixel of N tile t (the same in the four kq lanes of a pixel)
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        MN_WAVE_SYNC();          // the image is filled before any lane writes into it
        const int cnt = (int)tab[q.cnt_off + set];
        const int nt = mn_uniform(cnt < q.slots ? cnt : q.slots);
        for (int i = 0; i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            const int cb0 = (int)tile[0];
            const bool first = mn_uniform((int)tile[1]) != 0;          // a new group: sum a is formed along with this tile
            i32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = i32x4{0, 0, 0, 0};
            if (first) sa[0] = sa[1] = sa[2] = sa[3] = 0;
            const uint32_t* ap = tile + THDR + lane * 4;
#pragma unroll 1
            for (int s = 0; s < q.nsteps; ++s) {
                const uint32_t sl = tab[q.slot_off + 4 * s + kq];
                const bool real = (sl & PADSLOT) == 0u;
                const int dy = KS == 3 ? (int)(sl & 3u) - 1 : 0, dx = KS == 3 ? (int)((sl >> 2) & 3u) - 1 : 0, cb = cb0 + (int)((sl >> 4) & 0xffffu);
                const int boff = cb * HW + dy * q.W + dx;
                const u32x4 a = *reinterpret_cast<const u32x4*>(ap + s * STEPW);
                u32x4 b[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    b[t] = real ? fill : u32x4{0u, 0u, 0u, 0u};          // outside the map: codes 0; a padding slot: the zero byte
                    if (real && (unsigned)(ph[t] + dy) < (unsigned)q.H && (unsigned)(pw[t] + dx) < (unsigned)q.W) b[t] = x[xoff[t] + boff];
                }
                if (first) {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int e = 0; e < 4; ++e) sa[t] = bytesum(b[t][e], sa[t]);
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = mn_mfma_i8(a, b[t], acc[t]);
            }
            if (first) {          // the four kq lanes of a pixel hold the four quarters of every k-step
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    sa[t] += __shfl_xor(sa[t], 16, 64);
                    sa[t] += __shfl_xor(sa[t], 32, 64);
                }
            }
            // the lane's rows 4 kq .. 4 kq + 3 of the tile (D[row = 4 kq + reg][col = n])
            f32x4 ch[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) ch[j] = *reinterpret_cast<const f32x4*>(tile + T_CH + 16 * j + 4 * kq);
            const i32x4 kc = *reinterpret_cast<const i32x4*>(tile + T_KC + 4 * kq);
            const i32x4 ds = *reinterpret_cast<const i32x4*>(tile + T_DEST + 4 * kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (ds[r] < 0 || ds[r] >= SETROWS) continue;          // a dead row
                QaCh k;
                k.alpha = ch[0][r]; k.bias = ch[1][r]; k.mean = ch[2][r]; k.invstd = ch[3][r]; k.ga = ch[4][r]; k.be = ch[5][r];
                k.A = k.B = k.gi = 0.f;          // (not part of the forward chain)
                int8_t* const dst = imgb + ((ds[r] >> 4) * NPIX + n) * 16 + (ds[r] & 15);
                if (POOL) {
                    float mx = 0.f;          // post-ReLU values are >= 0
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int full = (int)(2u * (uint32_t)acc[t][r] + (uint32_t)sa[t] + (uint32_t)kc[r]);
                        float zh, z;
                        qa_eval<0>((float)full, k, zh, z);
                        mx = fmaxf(mx, qa_relu(z));
                    }
                    dst[0] = (int8_t)(uint8_t)(qa_code(mx, q.s) ^ 0x80u);
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int full = (int)(2u * (uint32_t)acc[t][r] + (uint32_t)sa[t] + (uint32_t)kc[r]);
                        dst[256 * t] = (int8_t)(uint8_t)(qa_code_of<0>((float)full, k, q.s) ^ 0x80u);
                    }
                }
            }
        }
        MN_WAVE_SYNC();          // every byte of the set is in the image
        if (POOL) {
            const u32x4 v = img[kq * NPIX + n];
            img[kq * NPIX + n] = fill;
            const int ob = 4 * set + kq;
            if (sok && ob < q.OB) ybase[(int64_t)ob * HWo] = v;
        } else {
#pragma unroll
            for (int bk = 0; bk < 4; ++bk) {
                const u32x4 v = img[bk * NPIX + lane];
                img[bk * NPIX + lane] = fill;
                const int ob = 4 * set + bk;
                if (sok && ob < q.OB) ybase[(int64_t)ob * HWo] = v;
            }
        }
    }
}

// ---------------------------------------------------------------- NCHW uint8 codes <-> the blocked byte map
// one thread = one 16-byte block: 16 channels of one pixel (reads coalesced along pixels per channel); tail channels 0x80
__global__ __launch_bounds__(256) void k_code8_pack(const uint8_t* __restrict__ codes, u32x4* __restrict__ out, int64_t total, int C, int CB, int HW) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int pix = (int)(i % HW);
    const int64_t t = i / HW;
    const int cb = (int)(t % CB);
    const int64_t nimg = t / CB;
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        const int c = cb * 16 + d;
        const uint32_t j = c < C ? (uint32_t)codes[(nimg * C + c) * HW + pix] : 0u;
        v[d >> 2] |= (j ^ 0x80u) << (8 * (d & 3));
    }
    out[i] = v;
}

// one thread = one code of the NCHW tensor
__global__ __launch_bounds__(256) void k_code8_unpack(const uint8_t* __restrict__ in, uint8_t* __restrict__ codes, int64_t total, int C, int CB, int HW) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int pix = (int)(i % HW);
    const int64_t t = i / HW;
    const int c = (int)(t % C);
    const int64_t nimg = t / C;
    codes[i] = (uint8_t)(in[((nimg * CB + (c >> 4)) * HW + pix) * 16 + (c & 15)] ^ 0x80u);
}

}  // namespace mn_code8

// (passed as an argument of "%s", never as a format)
#define MN_CODE8_COVER "geometry or width not covered (8-bit codes and weights throughout; 1x1 / stride 1 / padding 0 with groups 1 or C / groups % 16 == 0, or 3x3 / stride 1 / padding 1 with C / groups % 16 == 0; C / groups * taps <= 33025)"

extern "C" int mn_code8conv_supported(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_code8::W8Geom m;
    return mn_code8::make_geom(g, a_bits_in, w_bits, a_bits_out, m) ? 1 : 0;
}

extern "C" int64_t mn_code8conv_table_bytes(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_code8::W8Geom m;
    if (!mn_code8::make_geom(g, a_bits_in, w_bits, a_bits_out, m)) return 0;
    return 4 * mn_code8::table_words(m);
}

extern "C" int mn_code8conv_pack(const mn_conv_geom* g, const float* w, const float* chan, int a_bits_in, int w_bits, int a_bits_out, const int32_t* out_order,
                                 uint32_t* table, mn_stream_t stream) {
    mn_code8::W8Geom m;
    if (!w || !chan || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)chan | (uintptr_t)out_order) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_code8conv_pack: null / unaligned argument (the table is 16-byte aligned) or invalid geometry");
    if (!mn_code8::make_geom(g, a_bits_in, w_bits, a_bits_out, m)) MN_FAIL(MN_ENOTSUP, "mn_code8conv_pack: %s", MN_CODE8_COVER);
    mn_set_last_kernel("k_code8_wpack");
    hipLaunchKernelGGL(mn_code8::k_code8_clear, dim3(1), dim3(64), 0, (hipStream_t)stream, table);
    hipLaunchKernelGGL(mn_code8::k_code8_wpack, dim3(m.nsets), dim3(256), 0, (hipStream_t)stream, m, w, chan, out_order, table);
    MN_CHECK_LAUNCH("mn_code8conv_pack");
    return MN_OK;
}

extern "C" int mn_code8conv_fwd(const mn_conv_geom* g, const uint32_t* table, const int8_t* in_codes, int8_t* out_codes, int pool, mn_stream_t stream) {
    mn_code8::W8Geom m;
    if (!table || !in_codes || !out_codes || !aligned16(table) || !aligned16(in_codes) || !aligned16(out_codes) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_code8conv_fwd: null / unaligned argument (table and maps are 16-byte aligned) or invalid geometry");
    if (!mn_code8::make_geom(g, 8, 8, 8, m)) MN_FAIL(MN_ENOTSUP, "mn_code8conv_fwd: %s", MN_CODE8_COVER);
    if (pool < 0 || pool > 1) MN_FAIL(MN_ENOTSUP, "mn_code8conv_fwd: pool must be 0 or 1 (2x2 / stride 2)");
    if (pool && ((m.H & 1) || (m.W & 1))) MN_FAIL(MN_EINVAL, "mn_code8conv_fwd: the folded 2x2 max-pool needs even H and W");
    mn_code8::W8Fwd f;
    f.CB = m.CB; f.OB = m.OB; f.H = m.H; f.W = m.W; f.nsteps = m.nsteps; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride;
    f.slot_off = m.slot_off; f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off;
    f.Ho = pool ? m.H / 2 : m.H; f.Wo = pool ? m.W / 2 : m.W;
    f.total = m.N * f.Ho * f.Wo;
    f.s = 1.0f / 255.0f;
    const int ppb = pool ? 64 : 256;          // (pooled) pixels per block: four waves of four N tiles
    const int bx = (f.total + ppb - 1) / ppb;
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const u32x4* xin = reinterpret_cast<const u32x4*>(in_codes);
    u32x4* yout = reinterpret_cast<u32x4*>(out_codes);
    mn_set_last_kernel("k_code8conv<%d,%d>", m.KS, pool);
    mn_prof_bytes(16.0 * m.N * m.CB * m.H * m.W + 16.0 * m.N * m.OB * f.Ho * f.Wo + 4.0 * (double)mn_code8::table_words(m));
    mn_prof_begin(s);
    if (m.KS == 3) {
        if (pool) hipLaunchKernelGGL((mn_code8::k_code8conv<3, true>), grid, dim3(256), 0, s, table, xin, yout, f);
        else hipLaunchKernelGGL((mn_code8::k_code8conv<3, false>), grid, dim3(256), 0, s, table, xin, yout, f);
    } else {
        if (pool) hipLaunchKernelGGL((mn_code8::k_code8conv<1, true>), grid, dim3(256), 0, s, table, xin, yout, f);
        else hipLaunchKernelGGL((mn_code8::k_code8conv<1, false>), grid, dim3(256), 0, s, table, xin, yout, f);
    }
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_code8conv_fwd");
    return MN_OK;
}
#undef MN_CODE8_COVER

static int code8_map_args(const char* who, const void* codes, const void* map, int64_t N, int64_t C, int64_t HW) {
    if (!codes || !map || !aligned16(map) || N <= 0 || C <= 0 || HW <= 0) MN_FAIL(MN_EINVAL, "%s: null / empty argument, or a map that is not 16-byte aligned", who);
    if (N * ((C + 15) / 16) * HW >= (1ll << 27)) MN_FAIL(MN_ENOTSUP, "%s: tensor too large", who);
    return MN_OK;
}

extern "C" int mn_code8_pack_codes(const uint8_t* codes, int64_t N, int64_t C, int64_t HW, int8_t* map, mn_stream_t stream) {
    const int rc = code8_map_args("mn_code8_pack_codes", codes, map, N, C, HW);
    if (rc != MN_OK) return rc;
    const int CB = (int)((C + 15) / 16);
    const int64_t total = N * CB * HW;
    mn_set_last_kernel("k_code8_pack");
    mn_prof_bytes(1.0 * N * C * HW + 16.0 * (double)total);
    mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_code8::k_code8_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codes, reinterpret_cast<u32x4*>(map), total, (int)C, CB,
                       (int)HW);
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_code8_pack_codes");
    return MN_OK;
}

extern "C" int mn_code8_unpack_codes(const int8_t* map, int64_t N, int64_t C, int64_t HW, uint8_t* codes, mn_stream_t stream) {
    const int rc = code8_map_args("mn_code8_unpack_codes", codes, map, N, C, HW);
    if (rc != MN_OK) return rc;
    const int CB = (int)((C + 15) / 16);
    const int64_t total = N * C * HW;
    mn_set_last_kernel("k_code8_unpack");
    mn_prof_bytes(16.0 * N * CB * HW + 1.0 * (double)total);
    mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_code8::k_code8_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint8_t*>(map), codes, total,
                       (int)C, CB, (int)HW);
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_code8_unpack_codes");
    return MN_OK;
}
