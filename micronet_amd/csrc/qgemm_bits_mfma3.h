// The int8-MFMA form of the 3x3 hidden bit block (mn_bitconv_mfma3_*): bits in, bits out, the layout, out_order, decision and header word 0 of qgemm_bits.hip -- only the
// contraction differs, so the output words equal mn_bitconv_fwd's word for word.  Included by qgemm_bits.hip behind qgemm_bits_mfma.h; the 1-bit counterpart of
// qgemm_codes_mfma3.h, whose slot words, span planner (k_codes_mfma3_plan) and LDS image it shares.
//
//   contraction  : v_mfma_i32_16x16x64_i8 (mn_mfma_i8) as an implicit GEMM over (tap, channel).  A = the weight signs t in {-1, 0, +1} as bytes (M = 16 output rows of
//                  ONE group), B = the activations as bytes (N = 16 pixels): +1 for a set bit, -1 for a clear bit of a tap inside the image, 0 for a tap OUTSIDE the
//                  image (or a pixel outside the batch).  acc = sum a t is then the integer k_bitconv forms as 2 popc(~(x ^ s) & m & valid) - popc(m & valid): no nnz
//                  term, no group mask, no border correction.  The K order is tap-major in SLOTS of 16 channels, slot = tap * (Cg / 16) + chunk, four slots per
//                  k-step, padded to a multiple of four with zero weight bytes.  A group starts on a half-word (C / groups % 16 == 0), so the 16 B bytes of lane
//                  (n, kq) at step s are one half of input word (hw0 + chunk) >> 1 at pixel n + (dy, dx) of slot 4 s + kq: one dword load and the multiply-and-mask
//                  spread of k_codeconv_mfma, then 0 / 1 -> -1 / +1 by one multiply and one xor per dword.  A padding slot reads the centre tap against zero bytes.
//   weight table : (private layout, 16-byte aligned) 8 header words -- [0] rows whose decision is not monotone in acc + bad out_order entries, [1] k-steps, [2] SPAN
//                  (output words a wave assembles at once, chosen by the planner), [3] tile stride, [4] rows, [5] dead rows -- then one word per slot
//                  (dy + 1 | (dx + 1) << 2 | chunk << 4), then the tile count of every span (room for the spans of two words), then per span `slots` tiles of
//                    [0] hw0 (first half-word of the group), [1] M tiles of the batch this tile starts (1 .. 4; the tiles of a group in a span run in batches that
//                    share the expanded B operand), [16 ..) T[16], dest[16] (32 * word in span + bit),
//                    [48 ..) per k-step 64 lanes x 16 bytes in the A-operand order of mn_mfma_i8 (lane = 16 kq + row).
//                  The rows of a span are sorted by group and cut into tiles of 16 inside a group; a tile is padded with dead rows (T = INT_MAX, zero weights: never
//                  a bit).  The span is the smallest of 2, 4, 8, 16 words with the fewest dead rows.  Positions >= O and bad out_order entries have no row.
//   kernel       : a wave owns 64 pixels as four N tiles and, per span, an LDS image [span words][64 pixels].  Per batch of up to four M tiles of a group the k-steps
//                  run outermost: the four B operands are expanded once, the weight bytes stream from the L2-resident table.  Every lane ORs the bits of its four rows
//                  into the image (LDS only); behind a barrier every output word is read back and stored once, whole, coalesced along pixels: no atomics and no
//                  read-modify-write on global memory.
// Covered: 3x3, padding 1, stride 1, in_shuffle 0 / 1; C / groups % 16 == 0; any O; pool 0; W = 3 and W = 2 weights alike.
#pragma once
#include "qgemm_bits_mfma.h"
#include "qgemm_codes_mfma3.h"

namespace mn_bits_mfma3 {

using mn_bits::Geom;
using mn_codes_mfma3::chan_at;
using mn_codes_mfma3::lds_or;
using mn_codes_mfma3::slots_of;
enum { HDR = mn_bits::HDR, THDR = 16, TMETA = 32, TA = THDR + TMETA, STEPW = 256, MAXSPAN = mn_codes_mfma3::MAXSPAN, MAXROWS = 32 * MAXSPAN, MB = 4 };

struct M3Geom {
    Geom q;
    int chunks, nslots, nsteps, tstride, cnt_off, tiles_off;          // 16-channel chunks per group, slots, k-steps of four slots, words per tile, span counts, first tile
    int64_t max_tiles;
};

static inline bool make_m3geom(const mn_conv_geom* g, M3Geom& m) {
    if (!mn_bits::make_geom(g, m.q, false) || m.q.KS != 3) return false;
    if (m.q.Cg & 15) return false;          // every group starts on a half-word
    m.chunks = m.q.Cg >> 4;
    m.nslots = 9 * m.chunks;
    m.nsteps = (m.nslots + 3) >> 2;
    m.tstride = TA + STEPW * m.nsteps;
    m.cnt_off = HDR + 4 * m.nsteps;
    m.tiles_off = (m.cnt_off + ((m.q.OW + 1) >> 1) + 3) & ~3;
    m.max_tiles = 0;
    for (int span = 2; span <= MAXSPAN; span *= 2) {
        const int64_t t = (int64_t)((m.q.OW + span - 1) / span) * slots_of(span, m.q.groups, m.q.OW);
        if (t > m.max_tiles) m.max_tiles = t;
    }
    if ((int64_t)m.tiles_off + m.max_tiles * m.tstride >= (1ll << 30)) return false;
    return true;
}
static inline int64_t table_words(const M3Geom& m) { return (int64_t)m.tiles_off + m.max_tiles * m.tstride; }

// ---------------------------------------------------------------- weight table: one block per span (blocks past the last span of the chosen width leave)
__global__ __launch_bounds__(256) void k_bits_mfma3_wpack(M3Geom m, const float* __restrict__ w, const float* __restrict__ bias, const int32_t* __restrict__ order,
                                                          uint32_t* __restrict__ tab) {
    __shared__ int s_chan[MAXROWS], s_grp[MAXROWS], s_cnt[MAXROWS], s_before[MAXROWS], s_tile[MAXROWS];
    const Geom& q = m.q;
    const int sp = blockIdx.x, tid = threadIdx.x;
    const int span = (int)tab[2], rows = 32 * span;          // (written by k_codes_mfma3_plan, earlier on the stream)
    if (sp * span >= q.OW) return;
    const int slots = slots_of(span, q.groups, q.OW);
    uint32_t* tiles = tab + m.tiles_off + (int64_t)sp * slots * m.tstride;
    // every slot starts as a tile of dead rows: T = INT_MAX, zero weight bytes
    for (int i = tid; i < slots * m.tstride; i += 256) {
        const int r = i % m.tstride;
        tiles[i] = (r >= THDR && r < THDR + 16) ? 0x7fffffffu : 0u;
    }
    for (int p = tid; p < rows; p += 256) {
        const int o = chan_at(q, order, sp * rows + p);
        s_chan[p] = o; s_grp[p] = o < 0 ? INT_MAX : o / q.Og;
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
    // weight signs: thread = 4 consecutive channels of one row at one tap, one dword of the A operand (lane 16 (slot & 3) + row of k-step slot >> 2)
    const int dpr = m.nslots * 4;          // dwords per row
    for (int idx = tid; idx < rows * dpr; idx += 256) {
        const int pos = idx / dpr, d = idx - pos * dpr, slot = d >> 2, e4 = d & 3;
        const int o = s_chan[pos];
        if (o < 0) continue;
        const int tap = slot / m.chunks, c0 = (slot - tap * m.chunks) * 16 + e4 * 4;
        const float* wr = w + ((int64_t)o * q.Cg + c0) * 9 + tap;          // [O][Cg][9]
        uint32_t v = 0u;
        for (int e = 0; e < 4; ++e) v |= ((uint32_t)mn_bits_mfma::sign_of(wr[e * 9]) & 0xffu) << (8 * e);
        uint32_t* A = tiles + (int64_t)s_tile[pos] * m.tstride + TA;
        A[(slot >> 2) * STEPW + ((slot & 3) * 16 + (s_before[pos] & 15)) * 4 + e4] = v;
    }
    // thresholds: T of k_bits_wpack, on acc itself
    for (int p = tid; p < rows; p += 256) {
        const int o = s_chan[p];
        if (o < 0) continue;
        const int r = s_before[p] & 15, tg = s_before[p] >> 4;
        uint32_t* T = tiles + (int64_t)s_tile[p] * m.tstride;
        int st;
        bool mono;
        const int th = mn_bits_mfma::row_threshold(w + (int64_t)o * q.K, q.K, bias ? bias[o] : 0.f, st, mono);
        if (!mono) atomicAdd(tab + 0, 1u);
        T[THDR + r] = (uint32_t)th;
        T[THDR + 16 + r] = (uint32_t)p;          // 32 * word in span + bit
        if (r == 0) {
            const int left = ((s_cnt[p] + 15) >> 4) - tg;          // tiles of the group from this one on
            T[0] = (uint32_t)(s_grp[p] * q.Cg >> 4);
            T[1] = (uint32_t)((tg % MB) ? 0 : left < MB ? left : MB);
        }
    }
}

// ---------------------------------------------------------------- MFMA contraction + threshold -> output bits
struct M3Fwd {
    int total, Cw, H, W, OW, groups, nsteps, tstride, cnt_off, tiles_off;
};

// 16 bits -> 16 bytes: +1 for a set bit, -1 for a clear one (0 / 1 bytes times 0xfe, inverted: 0x01 / 0xff; no carries between bytes)
__device__ __forceinline__ u32x4 spread16_pm(uint32_t h) {
    u32x4 r = mn_codes_mfma::spread16(h, 0u);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = ~(r[i] * 0xfeu);
    return r;
}

template <int POOL>
__global__ __launch_bounds__(256, 4) void k_bitconv_mfma3(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, uint32_t* __restrict__ y, M3Fwd q) {
    static_assert(POOL == 0, "the 2x2 pool is not folded into the 3x3 MFMA form");
    __shared__ uint32_t s_img[4][MAXSPAN * 64];          // per wave: [span words][64 pixels]
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HW = q.H * q.W;
    const int pb = ((int)blockIdx.x * 4 + wave) * 64;
    int ph[4], pw[4], xoff[4];          // row, column and word 0 at the pixel of N tile t; a pixel outside the batch has row -4: every tap is outside
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = pb + 16 * t + n;
        const int pc = p < q.total ? p : 0;
        const int img = pc / HW, r = pc - img * HW;
        const int h = r / q.W;
        ph[t] = p < q.total ? h : -4; pw[t] = r - h * q.W;
        xoff[t] = img * q.Cw * HW + r;
    }
    // what this lane stores: the words of pixel pb + lane
    const int ps = pb + lane;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HW;
    uint32_t* const ybase = y + (int64_t)simg * q.OW * HW + (psc - simg * HW);
    uint32_t* const img = s_img[wave];
    const int span = (int)tab[2];          // wave-uniform
    if (span < 2 || span > MAXSPAN) return;          // (not a packed table)
    const int slots = slots_of(span, q.groups, q.OW);
    const int nspans = (q.OW + span - 1) / span;
    for (int i = 0; i < span; ++i) img[i * 64 + lane] = 0u;
    for (int sp = (int)blockIdx.y; sp < nspans; sp += (int)gridDim.y) {
        __syncthreads();          // the image is zero before any lane ORs into it
        const int nt = (int)tab[q.cnt_off + sp] < slots ? (int)tab[q.cnt_off + sp] : slots;
        for (int i = 0; i < nt;) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(sp * slots + i) * q.tstride;
            const int hw0 = (int)tile[0], nb = tile[1] - 1u < (uint32_t)(nt - i < MB ? nt - i : MB) ? (int)tile[1] : 1;          // (wave-uniform) a batch of nb M tiles of one group: its bits are expanded once
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
                const int woff = (hw >> 1) * HW + dy * q.W + dx, sh = 16 * (hw & 1);
                u32x4 b[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    b[t] = u32x4{0u, 0u, 0u, 0u};          // a tap outside the image: 0, not -1
                    if ((unsigned)(ph[t] + dy) < (unsigned)q.H && (unsigned)(pw[t] + dx) < (unsigned)q.W) b[t] = spread16_pm((x[xoff[t] + woff] >> sh) & 0xffffu);
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
                    // the lane's rows 4 kq .. 4 kq + 3 of the tile (D[row = 4 kq + reg][col = n])
                    const uint32_t* tl = tile + (int64_t)mt * q.tstride;
                    const i32x4 th = *reinterpret_cast<const i32x4*>(tl + THDR + 4 * kq);
                    const u32x4 ds = *reinterpret_cast<const u32x4*>(tl + THDR + 16 + 4 * kq);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t bit = 1u << (ds[r] & 31u);
                        uint32_t* const wp = img + ((ds[r] >> 5) & (MAXSPAN - 1)) * 64 + n;          // ds < 32 * span
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            if (acc[mt][t][r] >= th[r]) lds_or(wp + 16 * t, bit);
                    }
                }
            i += nb;
        }
        __syncthreads();          // every bit of the span is in the image
        for (int i = 0; i < span; ++i) {
            const uint32_t v = img[i * 64 + lane];
            img[i * 64 + lane] = 0u;
            const int word = sp * span + i;
            if (sok && word < q.OW) ybase[(int64_t)word * HW] = v;
        }
    }
}

}  // namespace mn_bits_mfma3

#define MN_BITMFMA3_COVER "geometry not covered (3x3, stride 1, padding 1, no input shuffle, C / groups %% 16 == 0)"

extern "C" int mn_bitconv_mfma3_supported(const mn_conv_geom* g) {
    mn_bits_mfma3::M3Geom m;
    return mn_bits_mfma3::make_m3geom(g, m) ? 1 : 0;
}

extern "C" int64_t mn_bitconv_mfma3_table_bytes(const mn_conv_geom* g) {
    mn_bits_mfma3::M3Geom m;
    if (!mn_bits_mfma3::make_m3geom(g, m)) return 0;
    return 4 * mn_bits_mfma3::table_words(m);
}

extern "C" int mn_bitconv_mfma3_pack(const mn_conv_geom* g, const float* w, const float* bias, const int32_t* out_order, uint32_t* table, mn_stream_t stream) {
    mn_bits_mfma3::M3Geom m;
    if (!w || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)bias | (uintptr_t)out_order) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_bitconv_mfma3_pack: null / unaligned argument (the table is 16-byte aligned) or invalid geometry");
    if (!mn_bits_mfma3::make_m3geom(g, m)) MN_FAIL(MN_ENOTSUP, "mn_bitconv_mfma3_pack: " MN_BITMFMA3_COVER);
    if (hipMemsetAsync(table, 0, 4 * mn_bits_mfma3::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_bitconv_mfma3_pack: header reset failed");          // word 0: bad-row count
    hipLaunchKernelGGL((mn_codes_mfma3::k_codes_mfma3_plan<mn_bits_mfma3::M3Geom>), dim3(1), dim3(256), 0, (hipStream_t)stream, m, out_order, table, 0u, 0);
    mn_set_last_kernel("k_bits_mfma3_wpack");
    hipLaunchKernelGGL(mn_bits_mfma3::k_bits_mfma3_wpack, dim3((m.q.OW + 1) >> 1), dim3(256), 0, (hipStream_t)stream, m, w, bias, out_order, table);
    MN_CHECK_LAUNCH("mn_bitconv_mfma3_pack");
    return MN_OK;
}

extern "C" int mn_bitconv_mfma3_fwd(const mn_conv_geom* g, const uint32_t* table, const uint32_t* x_bits, uint32_t* y_bits, int pool, mn_stream_t stream) {
    mn_bits_mfma3::M3Geom m;
    if (!table || !x_bits || !y_bits || !aligned16(table) || ((((uintptr_t)x_bits) | ((uintptr_t)y_bits)) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_bitconv_mfma3_fwd: null / unaligned argument (the table is 16-byte aligned) or invalid geometry");
    if (!mn_bits_mfma3::make_m3geom(g, m)) MN_FAIL(MN_ENOTSUP, "mn_bitconv_mfma3_fwd: " MN_BITMFMA3_COVER);
    if (pool != 0) MN_FAIL(MN_ENOTSUP, "mn_bitconv_mfma3_fwd: pool must be 0 (no max-pool is folded into the 3x3 MFMA form)");
    const mn_bits::Geom& q = m.q;
    mn_bits_mfma3::M3Fwd f;
    f.Cw = q.Cw; f.H = q.H; f.W = q.W; f.OW = q.OW; f.groups = q.groups; f.nsteps = m.nsteps; f.tstride = m.tstride; f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off;
    f.total = q.N * q.H * q.W;
    const int bx = (f.total + 255) / 256;          // four waves of four N tiles
    const dim3 grid(bx, mn_sets::grid_rows(bx, (q.OW + 1) >> 1));          // the spans (the table says how wide; at most one per two output words) round-robin over grid.y
    const hipStream_t s = (hipStream_t)stream;
    mn_set_last_kernel("k_bitconv_mfma3<%d>", pool);
    mn_prof_bytes(4.0 * q.N * q.Cw * q.H * q.W + 4.0 * q.N * q.OW * q.H * q.W + 4.0 * (double)mn_bits_mfma3::table_words(m));
    mn_prof_begin(s);
    hipLaunchKernelGGL((mn_bits_mfma3::k_bitconv_mfma3<0>), grid, dim3(256), 0, s, table, x_bits, y_bits, f);
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_bitconv_mfma3_fwd");
    return MN_OK;
}
#undef MN_BITMFMA3_COVER
