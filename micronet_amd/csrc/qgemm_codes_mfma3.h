// The int8-MFMA form of the 3x3 hidden code block (mn_codeconv_mfma3_*): planes in, planes out, thresholds and bits of qgemm_codes.h -- only the contraction differs.
// Included by qgemm_bits.hip behind qgemm_codes_mfma.h.
//
//   contraction  : v_mfma_i32_16x16x64_i8 (mn_mfma_i8) as an implicit GEMM over (tap, channel).  A = weights as signed bytes 2k - 3 (M = 16 output rows of ONE group),
//                  B = activation codes j in [0, 3] as bytes (N = 16 pixels): acc = sum j (2k - 3), the integer k_codeconv forms as 2 sum j k - 3 sum j.  The K order is
//                  tap-major in SLOTS of 16 channels, slot = tap * (Cg / 16) + chunk, four slots per k-step, padded to a multiple of four with zero weight bytes.  A
//                  group starts on a half-word (C / groups % 16 == 0), so the 16 B bytes of lane (n, kq) at step s are one half of the two plane words of word group
//                  (hw0 + chunk) >> 1 at pixel n + (dy, dx) of slot 4 s + kq, spread to bytes by the multiply-and-mask of k_codeconv_mfma.  A tap outside the image (or
//                  a pixel outside the batch) is a zero word = code 0: no border mask, no correction term.  A padding slot reads the centre tap against zero bytes.
//   weight table : (private layout, 16-byte aligned) 8 header words -- [0] rows whose channel constants fail qa_finite, [1] k-steps, [2] SPAN (output words a wave
//                  assembles at once, chosen by the packer), [3] tile stride, [4] rows, [5] dead rows, [6] a_in | w_bits << 8 | a_out << 16, [7] bad out_order entries +
//                  rows with a weight off the grid -- then one word per slot (dy + 1 | (dx + 1) << 2 | chunk << 4), then the tile count of every span (room for the
//                  spans of two words), then per span `slots` tiles of
//                    [0] hw0 (first half-word of the group), [1] M tiles of the batch this tile starts (1 .. 4; the tiles of a group in a span run in batches that
//                    share the expanded B operand), [16 ..) flip[16], T_1[16] <= T_2[16] <= T_3[16], dest[16] (32 * word in span + bit),
//                    [96 ..) per k-step 64 lanes x 16 bytes in the A-operand order of mn_mfma_i8 (lane = 16 kq + row).
//                  The rows of a span are sorted by group and cut into tiles of 16 inside a group; a tile is padded with dead rows (T = INT_MAX, zero weights: never
//                  a bit).  The span is the smallest of 2, 4, 8, 16 words with the fewest dead rows: under nin_gc's "shuffle 16" (O = 512) 8 words, under "shuffle 32"
//                  (O = 1024) 16 words give every group 16 rows; identity order with O / groups % 16 == 0 takes 2.  Positions >= O and bad out_order entries have no row.
//   kernel       : a wave owns 64 pixels as four N tiles and, per span, an LDS image [span words][2 planes][64 pixels].  Per batch of up to four M tiles of a group the
//                  k-steps run outermost: the four B operands are expanded once, the weight bytes stream from the L2-resident table.  Every lane ORs the bits of its
//                  four rows into the image (LDS only); behind a barrier every output word is read back and stored once, whole, coalesced along pixels: no atomics and
//                  no read-modify-write on global memory.
//   width        : every kernel here is a template on the code width B = a_in = w_bits = a_out, instantiated for 2 (everything above, unchanged) and 4 (weight bytes
//                  2k - 15, fifteen thresholds per row, the binary search of k_codeconv_mfma's code_planes).  The LDS image is [span][B planes][64 pixels] per wave: at
//                  B = 4 the packer chooses the span among 2, 4, 8 (maxspan), which keeps the 32 KB per block of the 2-bit form; a layer whose groups would need 16
//                  words to fill their tiles (nin_gc's "shuffle 32": 8 rows per group in 8 words) pays with half-dead tiles.
// Covered: a_in = w_bits = a_out = 2 or 4; 3x3, padding 1, stride 1; C / groups % 16 == 0; any O; K * n * n <= 32767 with n = 2^B - 1 (at 2 bits at most 400 channels per
// group, at 4 bits exactly 16); pool 0.
#pragma once
#include "qgemm_codes_mfma.h"

namespace mn_codes_mfma3 {

using mn_codes::Geom;
using mn_codes_mfma::spread16;
using mn_codes_mfma::nthr;
using mn_codes_mfma::ta;
using mn_codes_mfma::code_planes;
enum { HDR = mn_codes::HDR, THDR = 16, STEPW = 256, MAXSPAN = 16, MAXROWS = 32 * MAXSPAN, MB = 4 };
// The widest span the packer may choose at code width B: the kernel's per-wave LDS image is [span][B planes][64 pixels], so four planes halve the span for the 32 KB per
// block the 2-bit form has.
constexpr int maxspan(int B) { return B == 2 ? MAXSPAN : MAXSPAN / 2; }

struct M3Geom {
    Geom q;
    int chunks, nslots, nsteps, tstride, cnt_off, tiles_off;          // 16-channel chunks per group, slots, k-steps of four slots, words per tile, span counts, first tile
    int64_t max_tiles;
    int bits;          // the code width B = a_in = w_bits = a_out: 2 or 4
};

__host__ __device__ static inline int slots_of(int span, int groups, int OW) {          // sum over the groups of a span of ceil(rows / 16), at most
    const int rows = 32 * (span < OW ? span : OW), gp = groups < rows ? groups : rows;
    return (rows + 15 * gp) / 16;
}

static inline bool make_m3geom(const mn_conv_geom* g, int a_in, int w_bits, int a_out, M3Geom& m) {
    if (!mn_codes::make_geom(g, a_in, w_bits, a_out, m.q, false, true) || m.q.KS != 3) return false;
    if (m.q.Cg & 15) return false;          // every group starts on a half-word
    m.bits = a_in;
    m.chunks = m.q.Cg >> 4;
    m.nslots = 9 * m.chunks;
    m.nsteps = (m.nslots + 3) >> 2;
    m.tstride = ta(m.bits) + STEPW * m.nsteps;
    m.cnt_off = HDR + 4 * m.nsteps;
    m.tiles_off = (m.cnt_off + ((m.q.OW + 1) >> 1) + 3) & ~3;
    m.max_tiles = 0;
    for (int span = 2; span <= maxspan(m.bits); span *= 2) {
        const int64_t t = (int64_t)((m.q.OW + span - 1) / span) * slots_of(span, m.q.groups, m.q.OW);
        if (t > m.max_tiles) m.max_tiles = t;
    }
    if ((int64_t)m.tiles_off + m.max_tiles * m.tstride >= (1ll << 30)) return false;
    return true;
}
static inline int64_t table_words(const M3Geom& m) { return (int64_t)m.tiles_off + m.max_tiles * m.tstride; }

// the channel at output position jj: -1 for a position past O or a bad out_order entry (G: mn_codes::Geom, or mn_bits::Geom for qgemm_bits_mfma3.h)
template <class G>
__device__ __forceinline__ int chan_at(const G& q, const int32_t* order, int jj) {
    const int o = jj < q.O ? (order ? order[jj] : jj) : -1;
    return (o >= 0 && o < q.O) ? o : -1;
}

// ---------------------------------------------------------------- the span, the header and the slot words: one block
// (MG: M3Geom, or the 1-bit form's geometry of qgemm_bits_mfma3.h, which shares the planner: `word6` is what header word 6 carries, `badword` the header word that counts
// the bad out_order entries; B: the code width, which bounds the span -- maxspan(B))
template <class MG, int B = 2>
__global__ __launch_bounds__(256) void k_codes_mfma3_plan(MG m, const int32_t* __restrict__ order, uint32_t* __restrict__ tab, uint32_t word6, int badword) {
    __shared__ int s_dead[4], s_bad;
    constexpr int NC = B == 2 ? 4 : 3;          // candidate spans 2 << c, c < NC
    const auto& q = m.q;
    const int tid = threadIdx.x;
    if (tid < 4) s_dead[tid] = 0;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int j = tid; j < q.OW * 32; j += 256) {
        const int o = chan_at(q, order, j);
        if (j < q.O && o < 0) atomicAdd(&s_bad, 1);
        if (o < 0) continue;
        const int grp = o / q.Og;
        for (int c = 0; c < NC; ++c) {          // the first row of its group in its span counts what the group's last tile lacks
            const int rows = 64 << c, j0 = j / rows * rows;
            int cnt = 0, before = 0;
            for (int jj = j0; jj < j0 + rows; ++jj) {
                const int oo = chan_at(q, order, jj);
                const int same = oo >= 0 && oo / q.Og == grp;
                cnt += same; before += same && jj < j;
            }
            if (before == 0 && (cnt & 15)) atomicAdd(&s_dead[c], 16 - (cnt & 15));
        }
    }
    __syncthreads();
    for (int i = tid; i < 4 * m.nsteps; i += 256) {
        const int tap = i < m.nslots ? i / m.chunks : 4, chunk = i < m.nslots ? i - tap * m.chunks : 0;          // a padding slot: the centre tap against zero bytes
        tab[HDR + i] = (uint32_t)((tap / 3) | ((tap % 3) << 2) | (chunk << 4));
    }
    if (tid == 0) {
        int best = 0;
        for (int c = 1; c < NC; ++c)
            if (s_dead[c] < s_dead[best]) best = c;
        tab[1] = (uint32_t)m.nsteps; tab[2] = (uint32_t)(2 << best); tab[3] = (uint32_t)m.tstride; tab[4] = (uint32_t)(q.OW * 32); tab[5] = (uint32_t)s_dead[best];
        tab[6] = word6;
        if (s_bad) atomicAdd(tab + badword, (uint32_t)s_bad);
    }
}

// ---------------------------------------------------------------- weight table: one block per span (blocks past the last span of the chosen width leave)
template <int B>
__global__ __launch_bounds__(256) void k_codes_mfma3_wpack(M3Geom m, const float* __restrict__ w, const float* __restrict__ chan, const int32_t* __restrict__ order,
                                                           uint32_t* __restrict__ tab) {
    constexpr int NTHR = nthr(B), TA = ta(B);
    __shared__ int s_chan[MAXROWS], s_grp[MAXROWS], s_cnt[MAXROWS], s_before[MAXROWS], s_tile[MAXROWS], s_off[MAXROWS];
    const Geom& q = m.q;
    const int sp = blockIdx.x, tid = threadIdx.x;
    const int span = (int)tab[2], rows = 32 * span;          // (written by k_codes_mfma3_plan, earlier on the stream)
    if (sp * span >= q.OW) return;
    const int slots = slots_of(span, q.groups, q.OW);
    uint32_t* tiles = tab + m.tiles_off + (int64_t)sp * slots * m.tstride;
    // every slot starts as a tile of dead rows: flip 1, T = INT_MAX, zero weight bytes
    for (int i = tid; i < slots * m.tstride; i += 256) {
        const int r = i % m.tstride;
        tiles[i] = (r >= THDR + 16 && r < THDR + 16 * (NTHR + 1)) ? 0x7fffffffu : (r >= THDR && r < THDR + 16) ? 1u : 0u;
    }
    for (int p = tid; p < rows; p += 256) {
        const int o = chan_at(q, order, sp * rows + p);
        s_chan[p] = o; s_grp[p] = o < 0 ? INT_MAX : o / q.Og; s_off[p] = 0;
    }
    __syncthreads();
    for (int p = tid; p < rows; p += 256) {
        int cnt = 0, before = 0;
        for (int jj = 0; jj < rows; ++jj) {
            const int same = s_chan[jj] >= 0 && s_grp[jj] == s_grp[p];
            cnt += same; before += same && jj < p;
        }
        s_cnt[p] = cnt; s_before[p] = before;
    }
    __syncthreads();
    for (int p = tid; p < rows; p += 256) {
        int tb = 0;          // tiles of the groups in front of this row's
        for (int jj = 0; jj < rows; ++jj)
            if (s_chan[jj] >= 0 && s_before[jj] == 0 && s_grp[jj] < s_grp[p]) tb += (s_cnt[jj] + 15) >> 4;
        s_tile[p] = tb + (s_before[p] >> 4);
    }
    if (tid == 0) {
        int nt = 0;
        for (int jj = 0; jj < rows; ++jj)
            if (s_chan[jj] >= 0 && s_before[jj] == 0) nt += (s_cnt[jj] + 15) >> 4;
        tab[m.cnt_off + sp] = (uint32_t)nt;
    }
    __syncthreads();
    // weight bytes 2k - (2^B - 1): thread = 4 consecutive channels of one row at one tap, one dword of the A operand (lane 16 (slot & 3) + row of k-step slot >> 2)
    const int dpr = m.nslots * 4;          // dwords per row
    const float nf = (float)NTHR;
    for (int idx = tid; idx < rows * dpr; idx += 256) {
        const int pos = idx / dpr, d = idx - pos * dpr, slot = d >> 2, e4 = d & 3;
        const int o = s_chan[pos];
        if (o < 0) continue;
        const int tap = slot / m.chunks, c0 = (slot - tap * m.chunks) * 16 + e4 * 4;
        const float* wr = w + ((int64_t)o * q.Cg + c0) * 9 + tap;          // [O][Cg][9]
        uint32_t v = 0u;
        int off = 0;
        for (int e = 0; e < 4; ++e) {
            const float kf = (wr[e * 9] * nf + nf) * 0.5f;          // w = (2k - n) / n
            const float kr = rintf(kf);
            if (!(fabsf(kf - kr) <= 1e-3f) || kr < 0.f || kr > nf) off = 1;
            const int kc = (int)(kr < 0.f ? 0.f : kr > nf ? nf : kr == kr ? kr : 0.f);
            v |= ((uint32_t)(2 * kc - NTHR) & 0xffu) << (8 * e);
        }
        if (off) s_off[pos] = 1;
        uint32_t* A = tiles + (int64_t)s_tile[pos] * m.tstride + TA;
        A[(slot >> 2) * STEPW + ((slot & 3) * 16 + (s_before[pos] & 15)) * 4 + e4] = v;
    }
    // thresholds: the search of k_qa_fwd on the block's eval-mode constants (qa_thresholds.h, as k_codes_wpack)
    for (int p = tid; p < rows; p += 256) {
        const int o = s_chan[p];
        if (o < 0) continue;
        const int r = s_before[p] & 15, tg = s_before[p] >> 4;
        uint32_t* T = tiles + (int64_t)s_tile[p] * m.tstride;
        const QaCh k = qa_load_ch(chan, q.O, o);
        const float s = q.s;
        const bool fin = qa_chan_finite(k);
        const float flip = fin ? qa_flip_of(k, s) : 1.f;
        T[THDR + r] = (uint32_t)(flip < 0.f ? -1 : 1);
        int th[NTHR];
        for (int l = 0; l < NTHR; ++l) th[l] = fin ? qa_threshold_of(k, s, flip, (uint32_t)l + 1u) : 0x7fffffff;
        // code = #{k : u >= T_k} does not depend on the order of the T_k: stored sorted (they are, where the chain is monotone), which the kernel's select form needs
        for (int a = 0; a < NTHR; ++a)
            for (int l = 0; l + 1 < NTHR; ++l)
                if (th[l] > th[l + 1]) { const int x = th[l]; th[l] = th[l + 1]; th[l + 1] = x; }
        for (int l = 0; l < NTHR; ++l) T[THDR + 16 * (l + 1) + r] = (uint32_t)th[l];
        T[THDR + 16 * (NTHR + 1) + r] = (uint32_t)p;          // 32 * word in span + bit
        if (!fin) atomicAdd(tab + 0, 1u);
        if (r == 0) {
            const int left = ((s_cnt[p] + 15) >> 4) - tg;          // tiles of the group from this one on
            T[0] = (uint32_t)(s_grp[p] * q.Cg >> 4);
            T[1] = (uint32_t)((tg % MB) ? 0 : left < MB ? left : MB);
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t nbad = 0;
        for (int i = 0; i < rows; ++i) nbad += (uint32_t)(s_off[i] != 0);
        if (nbad) atomicAdd(tab + 7, nbad);
    }
}

// ---------------------------------------------------------------- MFMA contraction + thresholds -> output planes
struct M3Fwd {
    int total, Cw, H, W, OW, groups, nsteps, tstride, cnt_off, tiles_off;
};

// (one OS thread in the emulation build: a plain read-modify-write is atomic there)
__device__ __forceinline__ void lds_or(uint32_t* p, uint32_t v) {
#ifdef MN_EMULATION
    *p |= v;
#else
    atomicOr(p, v);
#endif
}

// B: the code width; B == 2 is the kernel as it was.  At B == 4 the binary search of the epilogue holds the masks of three levels beside the batch's accumulators: two
// blocks per CU instead of four keep it out of scratch.
template <int B, int POOL>
__global__ __launch_bounds__(256, B == 2 ? 4 : 2) void k_codeconv_mfma3(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, uint32_t* __restrict__ y, M3Fwd q) {
    static_assert(POOL == 0, "the 2x2 pool is not folded into the 3x3 MFMA form");
    constexpr int TA = ta(B), MAXSP = maxspan(B);
    __shared__ uint32_t s_img[4][MAXSP * B * 64];          // per wave: [span words][B planes][64 pixels]
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HW = q.H * q.W;
    const int pb = ((int)blockIdx.x * 4 + wave) * 64;
    int ph[4], pw[4], xoff[4];          // row, column and plane 0 of word group 0 at the pixel of N tile t; a pixel outside the batch has row -4: every tap is outside
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = pb + 16 * t + n;
        const int pc = p < q.total ? p : 0;
        const int img = pc / HW, r = pc - img * HW;
        const int h = r / q.W;
        ph[t] = p < q.total ? h : -4; pw[t] = r - h * q.W;
        xoff[t] = img * q.Cw * B * HW + r;
    }
    // what this lane stores: the words of pixel pb + lane
    const int ps = pb + lane;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HW;
    uint32_t* const ybase = y + (int64_t)simg * q.OW * B * HW + (psc - simg * HW);
    uint32_t* const img = s_img[wave];
    const int span = (int)tab[2];          // wave-uniform
    if (span < 2 || span > MAXSP) return;          // (not a packed table)
    const int slots = slots_of(span, q.groups, q.OW);
    const int nspans = (q.OW + span - 1) / span;
    for (int i = 0; i < span * B; ++i) img[i * 64 + lane] = 0u;
    for (int sp = (int)blockIdx.y; sp < nspans; sp += (int)gridDim.y) {
        __syncthreads();          // the image is zero before any lane ORs into it
        const int nt = (int)tab[q.cnt_off + sp] < slots ? (int)tab[q.cnt_off + sp] : slots;
        for (int i = 0; i < nt;) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(sp * slots + i) * q.tstride;
            const int hw0 = (int)tile[0], nb = tile[1] - 1u < (uint32_t)(nt - i < MB ? nt - i : MB) ? (int)tile[1] : 1;          // (wave-uniform) a batch of nb M tiles of one group: its codes are expanded once
            i32x4 acc[MB][4];
#pragma unroll
            for (int mt = 0; mt < MB; ++mt)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[mt][t] = i32x4{0, 0, 0, 0};
            const uint32_t* ap = tile + TA + lane * 4;
#pragma unroll 1
            for (int s = 0; s < q.nsteps; ++s) {
                const uint32_t sl = tab[HDR + 4 * s + kq];
                const int dy = (int)(sl & 3u) - 1, dx = (int)((sl >> 2) & 3u) - 1, hw = hw0 + (int)(sl >> 4);
                const int woff = (hw >> 1) * B * HW + dy * q.W + dx, sh = 16 * (hw & 1);
                u32x4 b[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    uint32_t p[B];
#pragma unroll
                    for (int pl = 0; pl < B; ++pl) p[pl] = 0u;
                    if ((unsigned)(ph[t] + dy) < (unsigned)q.H && (unsigned)(pw[t] + dx) < (unsigned)q.W) {
                        const uint32_t* xp = x + xoff[t] + woff;
#pragma unroll
                        for (int pl = 0; pl < B; ++pl) p[pl] = xp[pl * HW];
                    }
#pragma unroll
                    for (int pl = 0; pl < B; ++pl) p[pl] = (p[pl] >> sh) & 0xffffu;
                    b[t] = spread16<B>(p);
                }
#pragma unroll
                for (int mt = 0; mt < MB; ++mt)
                    if (mt < nb) {
                        const u32x4 a = *reinterpret_cast<const u32x4*>(ap + (int64_t)mt * q.tstride + s * STEPW);
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc[mt][t] = mn_mfma_i8(a, b[t], acc[mt][t]);
                    }
            }
#pragma unroll
            for (int mt = 0; mt < MB; ++mt)
                if (mt < nb) {
                    // the lane's rows 4 kq .. 4 kq + 3 of the tile (D[row = 4 kq + reg][col = n]); the select form of k_codeconv_mfma
                    const uint32_t* tl = tile + (int64_t)mt * q.tstride;
                    const i32x4 fl = *reinterpret_cast<const i32x4*>(tl + THDR + 4 * kq);
                    if constexpr (B == 2) {
                        const i32x4 t1 = *reinterpret_cast<const i32x4*>(tl + THDR + 16 + 4 * kq);
                        const i32x4 t2 = *reinterpret_cast<const i32x4*>(tl + THDR + 32 + 4 * kq);
                        const i32x4 t3 = *reinterpret_cast<const i32x4*>(tl + THDR + 48 + 4 * kq);
                        const u32x4 ds = *reinterpret_cast<const u32x4*>(tl + THDR + 64 + 4 * kq);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int ng = fl[r] >> 31;
                            const int e1 = (t1[r] < 40000 ? t1[r] : 40000) - 1 + ng, e2 = (t2[r] < 40000 ? t2[r] : 40000) - 1 + ng, e3 = (t3[r] < 40000 ? t3[r] : 40000) - 1 + ng;
                            const uint32_t bit = 1u << (ds[r] & 31u);
                            uint32_t* const wp = img + ((ds[r] >> 5) & (MAXSP - 1)) * (B * 64) + n;          // ds < 32 * span
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                const int sv = acc[mt][t][r] ^ ng;
                                const uint32_t g2 = (uint32_t)((e2 - sv) >> 31);
                                const uint32_t g0 = (uint32_t)((int)((g2 & (uint32_t)(e3 - sv)) | (~g2 & (uint32_t)(e1 - sv))) >> 31);
                                lds_or(wp + 16 * t, g0 & bit);
                                lds_or(wp + 64 + 16 * t, g2 & bit);
                            }
                        }
                    } else {
                        // B > 2: the select deepened to a B-step binary search over the sorted thresholds (code_planes of k_codeconv_mfma)
                        int ngv[4], sv[4][4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            ngv[r] = fl[r] >> 31;
#pragma unroll
                            for (int t = 0; t < 4; ++t) sv[r][t] = acc[mt][t][r] ^ ngv[r];
                        }
                        uint32_t gm[B][4][4];
                        code_planes<B, 4>(tl, kq, ngv, sv, gm);
                        const u32x4 ds = *reinterpret_cast<const u32x4*>(tl + THDR + 16 * (nthr(B) + 1) + 4 * kq);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const uint32_t bit = 1u << (ds[r] & 31u);
                            uint32_t* const wp = img + ((ds[r] >> 5) & (MAXSP - 1)) * (B * 64) + n;          // ds < 32 * span
#pragma unroll
                            for (int t = 0; t < 4; ++t)
#pragma unroll
                                for (int pl = 0; pl < B; ++pl) lds_or(wp + 64 * pl + 16 * t, gm[B - 1 - pl][r][t] & bit);
                        }
                    }
                }
            i += nb;
        }
        __syncthreads();          // every bit of the span is in the image
        for (int i = 0; i < span * B; ++i) {
            const uint32_t v = img[i * 64 + lane];
            img[i * 64 + lane] = 0u;
            const int word = sp * span + i / B;
            if (sok && word < q.OW) ybase[(int64_t)(word * B + i % B) * HW] = v;
        }
    }
}

}  // namespace mn_codes_mfma3

// (passed as an argument of "%s", never as a format)
#define MN_CODEMFMA3_COVER "geometry not covered (2-bit codes and weights; 3x3, stride 1, padding 1, C / groups % 16 == 0, K * 9 <= 32767)"
#define MN_CODEMFMA3_COVER_BITS "geometry or width not covered (codes and weights of 2 or of 4 bits throughout; 3x3, stride 1, padding 1, C / groups % 16 == 0, K * n * n <= 32767 with n = 2^bits - 1: at 4 bits C / groups == 16)"

extern "C" int mn_codeconv_mfma3_supported(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_codes_mfma3::M3Geom m;
    return mn_codes_mfma3::make_m3geom(g, a_bits_in, w_bits, a_bits_out, m) ? 1 : 0;
}

extern "C" int64_t mn_codeconv_mfma3_table_bytes(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_codes_mfma3::M3Geom m;
    if (!mn_codes_mfma3::make_m3geom(g, a_bits_in, w_bits, a_bits_out, m)) return 0;
    return 4 * mn_codes_mfma3::table_words(m);
}

extern "C" int mn_codeconv_mfma3_pack(const mn_conv_geom* g, const float* w, const float* chan, int a_bits_in, int w_bits, int a_bits_out, const int32_t* out_order,
                                      uint32_t* table, mn_stream_t stream) {
    mn_codes_mfma3::M3Geom m;
    if (!w || !chan || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)chan | (uintptr_t)out_order) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_codeconv_mfma3_pack: null / unaligned argument (the table is 16-byte aligned) or invalid geometry");
    if (!mn_codes_mfma3::make_m3geom(g, a_bits_in, w_bits, a_bits_out, m)) MN_FAIL(MN_ENOTSUP, "mn_codeconv_mfma3_pack: %s", MN_CODEMFMA3_COVER_BITS);
    if (hipMemsetAsync(table, 0, 4 * mn_codes_mfma3::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_codeconv_mfma3_pack: header reset failed");          // the two counters
    const uint32_t word6 = (uint32_t)(m.bits | (m.bits << 8) | (m.bits << 16));
    const dim3 spans((m.q.OW + 1) >> 1);
    if (m.bits == 4) {
        hipLaunchKernelGGL((mn_codes_mfma3::k_codes_mfma3_plan<mn_codes_mfma3::M3Geom, 4>), dim3(1), dim3(256), 0, (hipStream_t)stream, m, out_order, table, word6, 7);
        mn_set_last_kernel("k_codes_mfma3_wpack");
        hipLaunchKernelGGL(mn_codes_mfma3::k_codes_mfma3_wpack<4>, spans, dim3(256), 0, (hipStream_t)stream, m, w, chan, out_order, table);
    } else {
        hipLaunchKernelGGL((mn_codes_mfma3::k_codes_mfma3_plan<mn_codes_mfma3::M3Geom, 2>), dim3(1), dim3(256), 0, (hipStream_t)stream, m, out_order, table, word6, 7);
        mn_set_last_kernel("k_codes_mfma3_wpack");
        hipLaunchKernelGGL(mn_codes_mfma3::k_codes_mfma3_wpack<2>, spans, dim3(256), 0, (hipStream_t)stream, m, w, chan, out_order, table);
    }
    MN_CHECK_LAUNCH("mn_codeconv_mfma3_pack");
    return MN_OK;
}

// (who: the entry point's name in its messages; cover: what it says it covers)
static int codeconv_mfma3_fwd_impl(const char* who, const char* cover, const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out, const uint32_t* table,
                                   const uint32_t* in_planes, uint32_t* out_planes, int pool, mn_stream_t stream) {
    mn_codes_mfma3::M3Geom m;
    if (!table || !in_planes || !out_planes || !aligned16(table) || ((((uintptr_t)in_planes) | ((uintptr_t)out_planes)) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "%s: null / unaligned argument (the table is 16-byte aligned) or invalid geometry", who);
    if (!mn_codes_mfma3::make_m3geom(g, a_bits_in, w_bits, a_bits_out, m)) MN_FAIL(MN_ENOTSUP, "%s: %s", who, cover);
    if (pool != 0) MN_FAIL(MN_ENOTSUP, "%s: pool must be 0 (no max-pool is folded into the 3x3 MFMA form)", who);
    const mn_codes::Geom& q = m.q;
    mn_codes_mfma3::M3Fwd f;
    f.Cw = q.Cw; f.H = q.H; f.W = q.W; f.OW = q.OW; f.groups = q.groups; f.nsteps = m.nsteps; f.tstride = m.tstride; f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off;
    f.total = q.N * q.H * q.W;
    const int bx = (f.total + 255) / 256;          // four waves of four N tiles
    const dim3 grid(bx, mn_sets::grid_rows(bx, (q.OW + 1) >> 1));          // the spans (the table says how wide; at most one per two output words) round-robin over grid.y
    const hipStream_t s = (hipStream_t)stream;
    mn_set_last_kernel("k_codeconv_mfma3<%d>", pool);
    mn_prof_bytes(4.0 * m.bits * q.N * q.Cw * q.H * q.W + 4.0 * m.bits * q.N * q.OW * q.H * q.W + 4.0 * (double)mn_codes_mfma3::table_words(m));
    mn_prof_begin(s);
    if (m.bits == 4) hipLaunchKernelGGL((mn_codes_mfma3::k_codeconv_mfma3<4, 0>), grid, dim3(256), 0, s, table, in_planes, out_planes, f);
    else hipLaunchKernelGGL((mn_codes_mfma3::k_codeconv_mfma3<2, 0>), grid, dim3(256), 0, s, table, in_planes, out_planes, f);
    mn_prof_end(s);
    MN_CHECK_LAUNCH(who);
    return MN_OK;
}

extern "C" int mn_codeconv_mfma3_fwd(const mn_conv_geom* g, const uint32_t* table, const uint32_t* in_planes, uint32_t* out_planes, int pool, mn_stream_t stream) {
    return codeconv_mfma3_fwd_impl("mn_codeconv_mfma3_fwd", MN_CODEMFMA3_COVER, g, mn_codes::A, mn_codes::WB, 2, table, in_planes, out_planes, pool, stream);
}

extern "C" int mn_codeconv_mfma3_fwd_bits(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out, const uint32_t* table, const uint32_t* in_planes,
                                          uint32_t* out_planes, int pool, mn_stream_t stream) {
    return codeconv_mfma3_fwd_impl("mn_codeconv_mfma3_fwd_bits", MN_CODEMFMA3_COVER_BITS, g, a_bits_in, w_bits, a_bits_out, table, in_planes, out_planes, pool, stream);
}
#undef MN_CODEMFMA3_COVER
#undef MN_CODEMFMA3_COVER_BITS
