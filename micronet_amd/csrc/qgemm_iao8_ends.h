// The two ends of the int8 deployment of the BN-folded IAO graph (mn_i8first_*, mn_i8conv_fwd_f32): the first conv reads the fp32 image and writes byte codes, the
// last conv reads byte codes and writes the fp32 map of the model's tail.  Included by qgemm_bits.hip behind qgemm_iao8.h, whose layout, chain, table and set / tile
// planner it shares (namespace mn_iao8).
//
//   first block  : x fp32 NCHW -> j = clamp(rha(fl(x / s_a)), -2^(in-1), 2^(in-1) - 1) (mn_i8_pack_codes' arithmetic; NaN -> 0), acc = sum j k exact in int32 over
//                  (c, dy, dx) with zero padding the code 0, then the hidden stage's un-pooled chain y = fl(fl(float(acc) * al) + b), r = max(y, 0),
//                  c = clamp(rha(fl(r / s_out))) at the second conv's scale and width -> int8 [N][ceil(O/16)][H*W][16].
//   K order      : k = (c * KS + dy) * KS + dx, the order of the stored weights [O][C][KS][KS], K = C KS^2 <= 128 padded with zero weight bytes to one or two k-steps
//                  of v_mfma_i32_16x16x64_i8.  K is no multiple of 16 channels, so the B operand is GATHERED byte by byte, not loaded as 16-channel slots.
//   weight table : the set / tile table of qgemm_iao8.h with one group and no slot words: 16 header words -- [0] and [7] the two counters of mn_i8conv_pack, [1] k-steps,
//                  [2] tile slots per set, [3] tile stride, [4] sets, [5] K, [6] a_bits | w_bits << 8 | in_bits << 16, [8] [9] s_out, [10] [11] the output code range,
//                  [12] s_a, [13] [14] the image code range -- then the tile count of every set, then the tiles as in qgemm_iao8.h.
//   k_i8first    : a 256-thread block owns 256 consecutive pixels of ONE image.  It first quantises the image rows it needs -- its own and (KS - 1) / 2 halo rows and
//                  columns on either side, zero outside the map -- ONCE into an LDS byte tile [C][rows][W + KS - 1]: every image value is divided once, not KS^2
//                  times.  The byte of K index (c, dy, dx) then stands at a pixel-independent offset from the pixel's own, so every lane gathers the B operands of
//                  its four N tiles (16 K-bytes per k-step) into registers once; they do not depend on the output channel, so the loop over the sets and tiles of
//                  the weight table (A streams from L2 as in k_i8conv) is MFMAs and the chain alone.  The epilogue is k_i8conv's: code bytes into the wave's LDS
//                  image, every 16-byte block stored once and whole.
//   last block   : k_i8conv_f32<KS> is k_i8conv<KS, 0> (the same tile_acc over the same table, packed by mn_i8conv_pack with s_p = s_out = 1) with the chain cut
//                  after r: every lane stores r = relu ? max(y, 0) : y of its rows as fp32 [N][O][H*W], position j holding channel out_order[j]; dead rows and
//                  positions >= O store nothing.  No LDS, no barrier.
// Covered (first): groups 1, no in_shuffle, KS in {3, 5}, stride 1, dilation 1, padding (KS - 1) / 2, C KS^2 <= 128, any O, H, W whose LDS tile
// C * (min(H, 255 / W + 2) + KS - 1) * (W + KS - 1) stays within 32 KB (true for every W <= 512), widths 2 .. 8.
#pragma once
#include "qgemm_iao8.h"

namespace mn_iao8 {

enum { FIRST_KMAX = 128, FIRST_LDS = 32 * 1024 };

struct FGeom {
    int N, C, H, W, O, KS, K, OB;
    int nsteps, nsets, slots, tstride, cnt_off, tiles_off;
    int bpi, rows, TW, lds;                       // blocks per image; rows, width and bytes of the LDS tile
    int in_bits, a_bits, w_bits;
};

static inline bool make_fgeom(const mn_conv_geom* g, int in_bits, int a_bits, int w_bits, FGeom& m) {
    if (!g || g->N <= 0 || g->C <= 0 || g->H <= 0 || g->W <= 0 || g->O <= 0) return false;
    if (in_bits < 2 || in_bits > 8 || a_bits < 2 || a_bits > 8 || w_bits < 2 || w_bits > 8) return false;
    if (g->KH != g->KW || (g->KH != 3 && g->KH != 5)) return false;
    const int pad = (g->KH - 1) / 2;
    if (g->stride_h != 1 || g->stride_w != 1 || g->dil_h != 1 || g->dil_w != 1 || g->pad_h != pad || g->pad_w != pad) return false;
    if (g->groups != 1 || g->in_shuffle != 0) return false;
    if ((int64_t)g->C * g->KH * g->KW > FIRST_KMAX) return false;
    m.N = g->N; m.C = g->C; m.H = g->H; m.W = g->W; m.O = g->O; m.KS = g->KH; m.K = g->C * g->KH * g->KW;
    m.in_bits = in_bits; m.a_bits = a_bits; m.w_bits = w_bits;
    m.OB = (g->O + 15) >> 4;
    m.nsteps = (m.K + 63) >> 6;
    m.nsets = (m.OB + 3) >> 2;
    m.tstride = THDR + STEPW * m.nsteps;
    m.cnt_off = HDR;
    if (!mn_sets::table_layout(m, 1, m.cnt_off)) return false;
    const int64_t HW = (int64_t)g->H * g->W;
    if ((int64_t)g->N * m.OB * HW >= (1ll << 27) || (int64_t)g->N * g->C * HW >= (1ll << 31)) return false;          // 16-byte blocks and image elements: indexed in int
    m.bpi = (int)((HW + 255) / 256);
    const int own = 255 / g->W + 2;          // rows that 256 consecutive pixels can touch
    m.rows = (own < g->H ? own : g->H) + m.KS - 1;
    m.TW = g->W + m.KS - 1;
    const int64_t lds = (int64_t)g->C * m.rows * m.TW;
    if (lds > FIRST_LDS) return false;
    m.lds = (int)((lds + 15) & ~15ll);
    return true;
}

// the weight code k = rint(w / s) as a byte; off: not on the grid, or beyond kmax
__device__ __forceinline__ uint32_t weight_code(float wv, float s, float kmax, int& off) {
    const float kf = wv / s;
    const float kr = rintf(kf);
    if (!(fabsf(kf - kr) <= 1e-3f) || !(fabsf(kr) <= kmax)) off = 1;
    const int kc = (int)(kr < -kmax ? -kmax : kr > kmax ? kmax : kr == kr ? kr : 0.f);
    return (uint32_t)kc & 0xffu;
}

// ---------------------------------------------------------------- weight table of the first block: one block per set
__global__ __launch_bounds__(256) void k_i8first_wpack(FGeom m, const float* __restrict__ w, const float* __restrict__ sw, int sw_stride, const float* __restrict__ bias,
                                                       float s_a, float s_out, const int32_t* __restrict__ order, uint32_t* __restrict__ tab) {
    __shared__ mn_sets::SetPlan sp;
    const int set = blockIdx.x, tid = threadIdx.x;
    if (set == 0 && tid == 0) {
        tab[1] = (uint32_t)m.nsteps; tab[2] = (uint32_t)m.slots; tab[3] = (uint32_t)m.tstride; tab[4] = (uint32_t)m.nsets; tab[5] = (uint32_t)m.K;
        tab[6] = (uint32_t)(m.a_bits | (m.w_bits << 8) | (m.in_bits << 16));
        tab[8] = mn_f2u(s_out); tab[9] = mn_f2u(s_out);
        tab[10] = mn_f2u(-(float)(1 << (m.a_bits - 1))); tab[11] = mn_f2u((float)((1 << (m.a_bits - 1)) - 1));
        tab[12] = mn_f2u(s_a);
        tab[13] = mn_f2u(-(float)(1 << (m.in_bits - 1))); tab[14] = mn_f2u((float)((1 << (m.in_bits - 1)) - 1));
        const uint32_t nbad = (uint32_t)!scale_ok(s_a) + (uint32_t)!scale_ok(s_out);
        if (nbad) atomicAdd(tab + 0, nbad);
    }
    uint32_t* tiles = tab + m.tiles_off + (int64_t)set * m.slots * m.tstride;
    // every slot starts as a tile of dead rows: zero weight bytes, al = b = 0, no destination
    for (int i = tid; i < m.slots * m.tstride; i += 256) {
        const int r = i % m.tstride;
        tiles[i] = (r >= T_DEST && r < T_DEST + 16) ? 0xffffffffu : 0u;
    }
    int nt;
    mn_sets::plan_set(order, m.O, m.O, set, tab + 7, sp, nt);
    if (tid == 0) tab[m.cnt_off + set] = (uint32_t)nt;
    // thread = 4 consecutive K indices of one row, one dword of the A operand (lane 16 ((k >> 4) & 3) + row of k-step k >> 6); the stored weights are in K order
    const int dpr = m.nsteps * 16;          // dwords per row
    const float kmax = (float)((1 << (m.w_bits - 1)) - 1);
    for (int idx = tid; idx < SETROWS * dpr; idx += 256) {
        const int pos = idx / dpr, d = idx - pos * dpr, k0 = 4 * d;
        const int o = sp.chan[pos];
        if (o < 0 || k0 >= m.K) continue;
        const float* wr = w + (int64_t)o * m.K + k0;
        const float s = sw[(int64_t)o * sw_stride];
        uint32_t v = 0u;
        int off = 0;
        for (int e = 0; e < 4 && k0 + e < m.K; ++e) v |= weight_code(wr[e], s, kmax, off) << (8 * e);
        if (off) sp.off[pos] = 1;
        uint32_t* A = tiles + (int64_t)sp.tile[pos] * m.tstride + THDR;
        A[(d >> 4) * STEPW + (((d >> 2) & 3) * 16 + sp.row[pos]) * 4 + (d & 3)] = v;
    }
    // the row constants
    if (tid < SETROWS && sp.chan[tid] >= 0) {
        const int o = sp.chan[tid], r = sp.row[tid];
        uint32_t* T = tiles + (int64_t)sp.tile[tid] * m.tstride;
        const float s = sw[(int64_t)o * sw_stride];
        const float al = s_a * s, b = bias ? bias[o] : 0.f;
        T[T_AL + r] = mn_f2u(al); T[T_B + r] = mn_f2u(b); T[T_DEST + r] = (uint32_t)tid;
        if (!fin(al) || !fin(b) || !scale_ok(s)) atomicAdd(tab + 0, 1u);
    }
    mn_sets::tally_off(sp, tab + 7);
}

// ---------------------------------------------------------------- first block: quantise once into LDS, gather B once, MFMA + chain -> output bytes
struct FFwd {
    int C, H, W, HW, OB, K, nsteps, nsets, slots, tstride, cnt_off, tiles_off, spb, bpi, rows, TW;
};

template <int KS>
__global__ __launch_bounds__(256) void k_i8first(const uint32_t* __restrict__ tab, const float* __restrict__ x, u32x4* __restrict__ y, FFwd q) {
    constexpr int P = (KS - 1) / 2, T2 = KS * KS;
    __shared__ u32x4 s_img[4][4 * 64];          // per wave: [4 blocks of the set][pixels][16 bytes]
    HIP_DYNAMIC_SHARED(int8_t, s_tile)          // [C][q.rows][q.TW] image codes; tile row 0 is image row r0 - P, tile column 0 is image column -P
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int nimg = (int)blockIdx.x / q.bpi, p0 = ((int)blockIdx.x - nimg * q.bpi) * 256;          // the block's image and its first pixel there
    const int r0 = p0 / q.W;
    const int pl = p0 + 255 < q.HW ? p0 + 255 : q.HW - 1;
    const int nrows = pl / q.W - r0 + 1 + 2 * P;          // <= q.rows
    const int plane = q.rows * q.TW;
    {
        const float s_a = mn_u2f(tab[12]), imin = mn_u2f(tab[13]), imax = mn_u2f(tab[14]);
        const float* xi = x + (int64_t)nimg * q.C * q.HW;
        const int per = nrows * q.TW;
        for (int i = tid; i < q.C * per; i += 256) {
            const int c = i / per, rem = i - c * per, tr = rem / q.TW, tc = rem - tr * q.TW;
            const int h = r0 - P + tr, wc = tc - P;
            int ci = 0;          // outside the map: the code 0
            if ((unsigned)h < (unsigned)q.H && (unsigned)wc < (unsigned)q.W) {
                const float cf = mn_clamp(mn_rha(xi[(int64_t)c * q.HW + h * q.W + wc] / s_a), imin, imax);
                ci = cf == cf ? (int)cf : 0;
            }
            s_tile[c * plane + rem] = (int8_t)ci;
        }
    }
    u32x4* const img = s_img[wave];
    int8_t* const imgb = reinterpret_cast<int8_t*>(img);
    for (int i = lane; i < 4 * 64; i += 64) img[i] = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();          // the tile is complete, the image is zero
    const int pw0 = p0 + wave * 64;          // the wave's first pixel
    const bool live = pw0 < q.HW;            // (wave-uniform) a wave behind the image's last pixel only keeps the barriers
    // B: the lane's 16 K-bytes per k-step at the pixel of N tile t, gathered once for every set
    u32x4 b[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) b[s][t] = u32x4{0u, 0u, 0u, 0u};
    if (live) {
        int base[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int p = pw0 + 16 * t + n;
            const int h = p / q.W;
            base[t] = p < q.HW ? (h - r0) * q.TW + (p - h * q.W) : 0;          // a pixel behind the image reads the tile's first bytes; nothing of it is stored
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s >= q.nsteps) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int k = 64 * s + 16 * kq + e;
                if (k >= q.K) continue;          // K padding: zero bytes against zero weight bytes
                const int c = k / T2, rr = k - c * T2, dy = rr / KS;
                const int off = c * plane + dy * q.TW + (rr - dy * KS);
#pragma unroll
                for (int t = 0; t < 4; ++t) b[s][t][e >> 2] |= (uint32_t)(uint8_t)s_tile[base[t] + off] << (8 * (e & 3));
            }
        }
    }
    const bool sok = pw0 + lane < q.HW;
    u32x4* const ybase = y + (int64_t)nimg * q.OB * q.HW + (sok ? pw0 + lane : 0);
    const float s_out = mn_u2f(tab[9]), qmin = mn_u2f(tab[10]), qmax = mn_u2f(tab[11]);
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        __syncthreads();          // the image is zero before any lane writes into it
        const int nt = (int)tab[q.cnt_off + set] < q.slots ? (int)tab[q.cnt_off + set] : q.slots;          // wave-uniform
        for (int i = 0; live && i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            const uint32_t* ap = tile + THDR + lane * 4;
            i32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = i32x4{0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (s >= q.nsteps) continue;
                const u32x4 a = *reinterpret_cast<const u32x4*>(ap + s * STEPW);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = mn_mfma_i8(a, b[s][t], acc[t]);
            }
            // the lane's rows 4 kq .. 4 kq + 3 of the tile (D[row = 4 kq + reg][col = n])
            const f32x4 al = *reinterpret_cast<const f32x4*>(tile + T_AL + 4 * kq);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(tile + T_B + 4 * kq);
            const i32x4 ds = *reinterpret_cast<const i32x4*>(tile + T_DEST + 4 * kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (ds[r] < 0 || ds[r] >= SETROWS) continue;          // a dead row
                int8_t* const dst = imgb + ((ds[r] >> 4) * 64 + n) * 16 + (ds[r] & 15);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float yv = (float)acc[t][r] * al[r] + bb[r];
                    dst[256 * t] = (int8_t)(int)code_of(fmaxf(yv, 0.f), s_out, qmin, qmax);
                }
            }
        }
        __syncthreads();          // every byte of the set is in the image
#pragma unroll
        for (int bk = 0; bk < 4; ++bk) {
            const u32x4 v = img[bk * 64 + lane];
            img[bk * 64 + lane] = u32x4{0u, 0u, 0u, 0u};
            const int ob = 4 * set + bk;
            if (sok && ob < q.OB) ybase[(int64_t)ob * q.HW] = v;
        }
    }
}

// ---------------------------------------------------------------- last block: k_i8conv<KS, 0> cut after r, fp32 NCHW out
// acc[t] = the tile's 16 rows against the 16 pixels of N tile t over every k-step: the contraction loop of k_i8conv, statement for statement (ph / pw / xoff: row,
// column and block 0 at the lane's pixel of N tile t).  k_i8conv keeps its own copy, so that the hidden kernels compile to what was measured.
template <int KS>
__device__ __forceinline__ void tile_acc(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ tile, const u32x4* __restrict__ x, const IFwd& q, int HW, int lane,
                                         int kq, const int (&ph)[4], const int (&pw)[4], const int (&xoff)[4], i32x4 (&acc)[4]) {
    const int cb0 = (int)tile[0];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = i32x4{0, 0, 0, 0};
    const uint32_t* ap = tile + THDR + lane * 4;
#pragma unroll 1
    for (int s = 0; s < q.nsteps; ++s) {
        const uint32_t sl = tab[q.slot_off + 4 * s + kq];
        const int dy = KS == 3 ? (int)(sl & 3u) - 1 : 0, dx = KS == 3 ? (int)((sl >> 2) & 3u) - 1 : 0, cb = cb0 + (int)(sl >> 4);
        const int boff = cb * HW + dy * q.W + dx;
        const u32x4 a = *reinterpret_cast<const u32x4*>(ap + s * STEPW);
        u32x4 b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            b[t] = u32x4{0u, 0u, 0u, 0u};
            if ((unsigned)(ph[t] + dy) < (unsigned)q.H && (unsigned)(pw[t] + dx) < (unsigned)q.W && cb < q.CB) b[t] = x[xoff[t] + boff];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = mn_mfma_i8(a, b[t], acc[t]);
    }
}

template <int KS>
__global__ __launch_bounds__(256) void k_i8conv_f32(const uint32_t* __restrict__ tab, const u32x4* __restrict__ x, float* __restrict__ y, IFwd q, int O, int relu) {
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HW = q.H * q.W;
    const int pb = ((int)blockIdx.x * 4 + wave) * 64;
    int ph[4], pw[4], xoff[4];          // as in k_i8conv: a pixel outside the batch has row -4
    int64_t yoff[4];                    // position 0 at the pixel of N tile t
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = pb + 16 * t + n;
        const int pc = p < q.total ? p : 0;
        const int img = pc / HW, r = pc - img * HW;
        const int h = r / q.W, wc = r - h * q.W;
        ph[t] = p < q.total ? h : -4; pw[t] = wc;
        xoff[t] = img * q.CB * HW + h * q.W + wc;
        yoff[t] = (int64_t)img * O * HW + r;
    }
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        const int nt = (int)tab[q.cnt_off + set] < q.slots ? (int)tab[q.cnt_off + set] : q.slots;          // wave-uniform
        for (int i = 0; i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            i32x4 acc[4];
            tile_acc<KS>(tab, tile, x, q, HW, lane, kq, ph, pw, xoff, acc);
            const f32x4 al = *reinterpret_cast<const f32x4*>(tile + T_AL + 4 * kq);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(tile + T_B + 4 * kq);
            const i32x4 ds = *reinterpret_cast<const i32x4*>(tile + T_DEST + 4 * kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (ds[r] < 0 || ds[r] >= SETROWS) continue;          // a dead row
                const int j = set * SETROWS + ds[r];
                if (j >= O) continue;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (ph[t] < 0) continue;
                    const float yv = (float)acc[t][r] * al[r] + bb[r];
                    y[yoff[t] + (int64_t)j * HW] = (relu && !(yv > 0.f)) ? 0.f : yv;
                }
            }
        }
    }
}

}  // namespace mn_iao8

// (passed as an argument of "%s", never as a format)
#define MN_I8FIRST_COVER "geometry or width not covered (code widths 2 .. 8; groups 1, no in_shuffle, 3x3 or 5x5 / stride 1 / dilation 1 / padding (KS - 1) / 2, C * KS * KS <= 128, an LDS tile C * (min(H, 255 / W + 2) + KS - 1) * (W + KS - 1) of at most 32 KB: every W <= 512)"

extern "C" int mn_i8first_supported(const mn_conv_geom* g, int in_bits, int a_bits, int w_bits) {
    mn_iao8::FGeom m;
    return mn_iao8::make_fgeom(g, in_bits, a_bits, w_bits, m) ? 1 : 0;
}

extern "C" int64_t mn_i8first_table_bytes(const mn_conv_geom* g, int in_bits, int a_bits, int w_bits) {
    mn_iao8::FGeom m;
    if (!mn_iao8::make_fgeom(g, in_bits, a_bits, w_bits, m)) return 0;
    return 4 * mn_iao8::table_words(m);
}

extern "C" int mn_i8first_pack(const mn_conv_geom* g, const float* w, const float* s_w, int s_w_stride, const float* bias, float s_a, float s_out, int in_bits, int a_bits,
                               int w_bits, const int32_t* out_order, uint32_t* table, mn_stream_t stream) {
    mn_iao8::FGeom m;
    if (!w || !s_w || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)s_w | (uintptr_t)bias | (uintptr_t)out_order) & 3) || s_w_stride < 0 || s_w_stride > 1 ||
        !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_i8first_pack: null / unaligned argument (the table is 16-byte aligned), s_w_stride outside 0 / 1 or invalid geometry");
    if (!mn_iao8::make_fgeom(g, in_bits, a_bits, w_bits, m)) MN_FAIL(MN_ENOTSUP, "mn_i8first_pack: %s", MN_I8FIRST_COVER);
    if (hipMemsetAsync(table, 0, 4 * mn_iao8::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_i8first_pack: header reset failed");          // the two counters
    mn_set_last_kernel("k_i8first_wpack");
    hipLaunchKernelGGL(mn_iao8::k_i8first_wpack, dim3(m.nsets), dim3(256), 0, (hipStream_t)stream, m, w, s_w, s_w_stride, bias, s_a, s_out, out_order, table);
    MN_CHECK_LAUNCH("mn_i8first_pack");
    return MN_OK;
}

extern "C" int mn_i8first_fwd(const mn_conv_geom* g, int in_bits, int a_bits, int w_bits, const uint32_t* table, const float* x, int8_t* out_codes, mn_stream_t stream) {
    mn_iao8::FGeom m;
    if (!table || !x || !out_codes || !aligned16(table) || (((uintptr_t)x) & 3) || !aligned16(out_codes) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_i8first_fwd: null / unaligned argument (x 4-byte, table and codes 16-byte aligned) or invalid geometry");
    if (!mn_iao8::make_fgeom(g, in_bits, a_bits, w_bits, m)) MN_FAIL(MN_ENOTSUP, "mn_i8first_fwd: %s", MN_I8FIRST_COVER);
    mn_iao8::FFwd f;
    f.C = m.C; f.H = m.H; f.W = m.W; f.HW = m.H * m.W; f.OB = m.OB; f.K = m.K; f.nsteps = m.nsteps; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride;
    f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off; f.bpi = m.bpi; f.rows = m.rows; f.TW = m.TW;
    const int bx = m.N * m.bpi;          // (< 2^27: make_fgeom bounds N * OB * H * W)
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    u32x4* yout = reinterpret_cast<u32x4*>(out_codes);
    mn_set_last_kernel("k_i8first<%d>", m.KS);
    mn_prof_bytes(4.0 * m.N * m.C * f.HW + 16.0 * m.N * m.OB * f.HW + 4.0 * (double)mn_iao8::table_words(m));
    mn_prof_begin(s);
    if (m.KS == 5) hipLaunchKernelGGL((mn_iao8::k_i8first<5>), grid, dim3(256), (size_t)m.lds, s, table, x, yout, f);
    else hipLaunchKernelGGL((mn_iao8::k_i8first<3>), grid, dim3(256), (size_t)m.lds, s, table, x, yout, f);
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_i8first_fwd");
    return MN_OK;
}
#undef MN_I8FIRST_COVER

extern "C" int mn_i8conv_fwd_f32(const mn_conv_geom* g, int a_bits, int w_bits, const uint32_t* table, const int8_t* in_codes, float* y, int relu, mn_stream_t stream) {
    mn_iao8::IGeom m;
    if (!table || !in_codes || !y || !aligned16(table) || !aligned16(in_codes) || (((uintptr_t)y) & 3) || !tile_geom_valid(g) || relu < 0 || relu > 1)
        MN_FAIL(MN_EINVAL, "mn_i8conv_fwd_f32: null / unaligned argument (y 4-byte, table and codes 16-byte aligned), invalid geometry or relu outside 0 / 1");
    if (!mn_iao8::make_igeom(g, a_bits, w_bits, m))
        MN_FAIL(MN_ENOTSUP, "mn_i8conv_fwd_f32: geometry or width not covered (what mn_i8conv_supported covers: code widths 2 .. 8; 1x1 / stride 1 / padding 0 with groups 1 "
                            "or C / groups %% 16 == 0, or 3x3 / stride 1 / padding 1 with C / groups %% 16 == 0)");
    mn_iao8::IFwd f;
    f.CB = m.CB; f.OB = m.OB; f.H = m.H; f.W = m.W; f.nsteps = m.nsteps; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride;
    f.slot_off = m.slot_off; f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off;
    f.Ho = m.H; f.Wo = m.W;
    f.total = m.N * m.H * m.W;
    const int bx = (f.total + 255) / 256;          // four waves of four N tiles
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const u32x4* xin = reinterpret_cast<const u32x4*>(in_codes);
    mn_set_last_kernel("k_i8conv_f32<%d>", m.KS);
    mn_prof_bytes(16.0 * m.N * m.CB * m.H * m.W + 4.0 * m.N * m.O * m.H * m.W + 4.0 * (double)mn_iao8::table_words(m));
    mn_prof_begin(s);
    if (m.KS == 3) hipLaunchKernelGGL((mn_iao8::k_i8conv_f32<3>), grid, dim3(256), 0, s, table, xin, y, f, m.O, relu);
    else hipLaunchKernelGGL((mn_iao8::k_i8conv_f32<1>), grid, dim3(256), 0, s, table, xin, y, f, m.O, relu);
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_i8conv_fwd_f32");
    return MN_OK;
}
