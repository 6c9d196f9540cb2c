// The two ends of the int8 deployment of BN-folded IAO ResNets (mn_i8first_fwd2, mn_i8poolfc_*): the first conv reads the fp32 image and writes one code map per
// consumer quantizer of its output, the classifier reads the last block's codes and writes the fp32 logits -- QuantAdaptiveAvgPool2d((1, 1)) and QuantLinear in one
// launch.  Included by qgemm_bits.hip behind qgemm_iao8_res.h, whose layout, chain and helpers it shares (namespace mn_iao8).
//
//   first block  : k_i8first<KS>'s contract (qgemm_iao8_ends.h) bit for bit up to r = max(fl(fl(float(acc) * al) + b), 0); then out_k = Q(r; s_k, bits_k),
//                  Q(v; s, a) = clamp(rha(fl(v / s)), -2^(a-1), 2^(a-1) - 1), k = 0 .. NOUT - 1, each int8 [N][ceil(O/16)][H*W][16].  The table is mn_i8first_pack's own
//                  (packed with s_out = s_0, a_bits = bits_0): al and b do not depend on the consumer, and the kernel does not read the table's words 8 .. 11 -- the
//                  output quantizers arrive by value (mn_i8first_outs, read on the host at the call).
//   k_i8first2   : k_i8first<KS> with NOUT LDS images per wave (NOUT * 16 KB + the tile): the B gather is hoisted once per block, the chain is evaluated once per
//                  accumulator up to r with NOUT divisions behind it, every 16-byte block of either map is stored once and whole, positions >= O are 0.  k_i8first
//                  itself keeps its own code, so that it compiles to what was measured.
//   pooled fc    : input codes c at avg_pool's quantizer s_p, [N][ceil(C/16)][HW][16].  m[n, ch] = (float)(sum_p (double)fl(float(c) * s_p) / (double)HW) -- what
//                  k_fq_gap_fwd (iao_ops.hip) computes on the de-quantised map; for HW <= 4096 and |c| <= 128 the double sum is exact in any order (24 + 7 + 12 bits
//                  < 53) -- j = Q(m; s_fc, a_fc), acc[n, o] = sum_ch j k[o, ch] exact in int32, k = rint(w / s_w[o]), y[n, o] = fl(fl(float(acc) * al[o]) + b[o]),
//                  al = fl(s_fc * s_w[o]), a null bias 0, stored as fp32 [N][O].
//   fc table     : 16 header words -- [0] the count of non-finite or non-positive constants (al, b, s_w per row; s_p, s_fc), [1] C, [2] O, [3] the row stride in
//                  16-byte blocks, [6] a_bits | w_bits << 8 | p_bits << 16, [7] the rows with a weight off the grid or beyond 2^(w-1) - 1 (weight_code's rule),
//                  [8] s_p, [9] s_fc, [10] [11] the fc code range -- then al[64], b[64], then the weight bytes [O][ceil(C/16)][16], tail channels 0.
//   k_i8poolfc   : one 256-thread block per image.  The channels are walked in chunks of 4096 (one chunk for every net of the reference).  Phase 1: sixteen lanes
//                  per channel block, a 16-byte load per lane and pixel, sixteen fp64 sums per lane, a shuffle reduction over the sixteen lanes, the j bytes into
//                  LDS.  Phase 2: wave w owns the rows o = w, w + 4, ...; a lane dots 16 LDS bytes against 16 table bytes per step (v_dot4_i32_i8) for every row of
//                  its wave, the sums stay in registers across the chunks; then a wave-level integer reduction and one lane stores.  No atomics.
// Covered (pooled fc): 1 <= O <= 64, 1 <= HW <= 4096, widths 2 .. 8, C * 2^(a-1) * (2^(w-1) - 1) <= INT_MAX, N * ceil(C/16) * HW < 2^40 blocks.
#pragma once
#include "qgemm_iao8_res.h"

namespace mn_iao8 {

// the output quantizers of the first block, by value
struct FOuts {
    float s[2], qmin[2], qmax[2];
};

template <int KS, int NOUT>
__global__ __launch_bounds__(256) void k_i8first2(const uint32_t* __restrict__ tab, const float* __restrict__ x, u32x4* __restrict__ ya, u32x4* __restrict__ yb, FFwd q,
                                                  FOuts p) {
    constexpr int P = (KS - 1) / 2, T2 = KS * KS;
    __shared__ u32x4 s_img[NOUT][4][4 * 64];          // per output map and wave: [4 blocks of the set][pixels][16 bytes]
    HIP_DYNAMIC_SHARED(int8_t, s_tile)                // [C][q.rows][q.TW] image codes; tile row 0 is image row r0 - P, tile column 0 is image column -P
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
    u32x4* const img0 = s_img[0][wave];
    u32x4* const img1 = s_img[NOUT - 1][wave];
    int8_t* const imgb0 = reinterpret_cast<int8_t*>(img0);
    int8_t* const imgb1 = reinterpret_cast<int8_t*>(img1);
    for (int i = lane; i < 4 * 64; i += 64) {
        img0[i] = u32x4{0u, 0u, 0u, 0u};
        if (NOUT == 2) img1[i] = u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();          // the tile is complete, the images are zero
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
            const int px = pw0 + 16 * t + n;
            const int h = px / q.W;
            base[t] = px < q.HW ? (h - r0) * q.TW + (px - h * q.W) : 0;          // a pixel behind the image reads the tile's first bytes; nothing of it is stored
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
    const int64_t ybase = (int64_t)nimg * q.OB * q.HW + (sok ? pw0 + lane : 0);
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        __syncthreads();          // the images are zero before any lane writes into them
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
                const int at = ((ds[r] >> 4) * 64 + n) * 16 + (ds[r] & 15);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float yv = (float)acc[t][r] * al[r] + bb[r];
                    const float rv = fmaxf(yv, 0.f);          // the chain once, a division per consumer
                    imgb0[at + 256 * t] = (int8_t)(int)code_of(rv, p.s[0], p.qmin[0], p.qmax[0]);
                    if (NOUT == 2) imgb1[at + 256 * t] = (int8_t)(int)code_of(rv, p.s[1], p.qmin[1], p.qmax[1]);
                }
            }
        }
        __syncthreads();          // every byte of the set is in the images
#pragma unroll
        for (int bk = 0; bk < 4; ++bk) {
            const u32x4 v0 = img0[bk * 64 + lane];
            img0[bk * 64 + lane] = u32x4{0u, 0u, 0u, 0u};
            u32x4 v1 = v0;
            if (NOUT == 2) {
                v1 = img1[bk * 64 + lane];
                img1[bk * 64 + lane] = u32x4{0u, 0u, 0u, 0u};
            }
            const int ob = 4 * set + bk;
            if (sok && ob < q.OB) {
                ya[ybase + (int64_t)ob * q.HW] = v0;
                if (NOUT == 2) yb[ybase + (int64_t)ob * q.HW] = v1;
            }
        }
    }
}

// ---------------------------------------------------------------- pooled classifier
enum { PF_AL = HDR, PF_B = HDR + 64, PF_W = HDR + 128, PF_OMAX = 64, PF_HWMAX = 4096, PF_CHUNK = 256 };          // PF_CHUNK: channel blocks per LDS chunk

struct PGeom {
    int64_t N, CB;
    int C, HW, O;
    int p_bits, a_bits, w_bits;
};

static inline bool make_pgeom(int64_t N, int64_t C, int64_t HW, int64_t O, int p_bits, int a_bits, int w_bits, PGeom& m) {
    if (N <= 0 || C <= 0 || HW <= 0 || O <= 0 || O > PF_OMAX || HW > PF_HWMAX) return false;
    if (p_bits < 2 || p_bits > 8 || a_bits < 2 || a_bits > 8 || w_bits < 2 || w_bits > 8) return false;
    if (C > (int64_t)INT_MAX || C * (1ll << (a_bits - 1)) * ((1ll << (w_bits - 1)) - 1) > (int64_t)INT_MAX) return false;          // acc is exact in int32
    m.N = N; m.C = (int)C; m.HW = (int)HW; m.O = (int)O; m.CB = (C + 15) >> 4;
    if (N > (1ll << 40) / (m.CB * HW)) return false;
    m.p_bits = p_bits; m.a_bits = a_bits; m.w_bits = w_bits;
    return true;
}
static inline int64_t pf_table_words(const PGeom& m) { return (int64_t)PF_W + (int64_t)m.O * m.CB * 4; }

// one block per output row
__global__ __launch_bounds__(256) void k_i8poolfc_wpack(PGeom m, const float* __restrict__ w, const float* __restrict__ sw, int sw_stride, const float* __restrict__ bias,
                                                        float s_p, float s_fc, uint32_t* __restrict__ tab) {
    __shared__ int s_off;
    const int o = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_off = 0;
    __syncthreads();
    const float s = sw[(int64_t)o * sw_stride];
    if (tid == 0) {
        if (o == 0) {
            tab[1] = (uint32_t)m.C; tab[2] = (uint32_t)m.O; tab[3] = (uint32_t)m.CB;
            tab[6] = (uint32_t)(m.a_bits | (m.w_bits << 8) | (m.p_bits << 16));
            tab[8] = mn_f2u(s_p); tab[9] = mn_f2u(s_fc);
            tab[10] = mn_f2u(-(float)(1 << (m.a_bits - 1))); tab[11] = mn_f2u((float)((1 << (m.a_bits - 1)) - 1));
            const uint32_t nbad = (uint32_t)!scale_ok(s_p) + (uint32_t)!scale_ok(s_fc);
            if (nbad) atomicAdd(tab + 0, nbad);
            for (int i = m.O; i < PF_OMAX; ++i) { tab[PF_AL + i] = 0u; tab[PF_B + i] = 0u; }
        }
        const float al = s_fc * s, b = bias ? bias[o] : 0.f;
        tab[PF_AL + o] = mn_f2u(al); tab[PF_B + o] = mn_f2u(b);
        if (!fin(al) || !fin(b) || !scale_ok(s)) atomicAdd(tab + 0, 1u);
    }
    const float kmax = (float)((1 << (m.w_bits - 1)) - 1);
    const float* wr = w + (int64_t)o * m.C;
    uint32_t* row = tab + PF_W + (int64_t)o * m.CB * 4;
    int off = 0;
    for (int64_t d = tid; d < m.CB * 4; d += 256) {
        uint32_t v = 0u;
        for (int e = 0; e < 4 && 4 * d + e < m.C; ++e) v |= weight_code(wr[4 * d + e], s, kmax, off) << (8 * e);
        row[d] = v;
    }
    if (off) s_off = 1;          // (every writer stores the same value)
    __syncthreads();
    if (tid == 0 && s_off) atomicAdd(tab + 7, 1u);
}

// the dot product of 16 signed bytes with 16 signed bytes, added to s
__device__ __forceinline__ int dot16(const u32x4& a, const u32x4& b, int s) {
#ifdef MN_EMULATION
    for (int i = 0; i < 4; ++i)
        for (int e = 0; e < 4; ++e) s += (int)(int8_t)(a[i] >> (8 * e)) * (int)(int8_t)(b[i] >> (8 * e));
#else
#pragma unroll
    for (int i = 0; i < 4; ++i) s = __builtin_amdgcn_sdot4((int)a[i], (int)b[i], s, false);
#endif
    return s;
}

struct PFwd {
    int64_t CB;
    int HW, O;
};

__global__ __launch_bounds__(256) void k_i8poolfc(const uint32_t* __restrict__ tab, const u32x4* __restrict__ x, float* __restrict__ y, PFwd q) {
    __shared__ u32x4 s_j[PF_CHUNK];          // the fc input codes of one chunk of channel blocks
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), grp = tid >> 4, gl = tid & 15;
    const float s_p = mn_u2f(tab[8]), s_fc = mn_u2f(tab[9]), qmin = mn_u2f(tab[10]), qmax = mn_u2f(tab[11]);
    const u32x4* xi = x + (int64_t)blockIdx.x * q.CB * q.HW;
    const u32x4* wt = reinterpret_cast<const u32x4*>(tab + PF_W);
    const double hw = (double)q.HW;
    int acc[16];          // row o = wave + 4 r
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
    for (int64_t c0 = 0; c0 < q.CB; c0 += PF_CHUNK) {
        const int nb = q.CB - c0 < PF_CHUNK ? (int)(q.CB - c0) : PF_CHUNK;          // channel blocks of this chunk
        // phase 1: the sixteen lanes of a group walk the pixels of one channel block
        for (int cb = grp; cb < ((nb + 15) & ~15); cb += 16) {          // (every lane of a wave keeps the shuffles' company)
            double sum[16];
#pragma unroll
            for (int d = 0; d < 16; ++d) sum[d] = 0.0;
            if (cb < nb) {
                const u32x4* src = xi + (c0 + cb) * q.HW;
                for (int px = gl; px < q.HW; px += 16) {
                    const u32x4 v = src[px];
#pragma unroll
                    for (int d = 0; d < 16; ++d) sum[d] += (double)((float)(int8_t)(v[d >> 2] >> (8 * (d & 3))) * s_p);
                }
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1)
#pragma unroll
                for (int d = 0; d < 16; ++d) sum[d] += __shfl_down(sum[d], o, 64);          // lane 0 of a group only ever takes its own group's sums
            if (gl == 0 && cb < nb) {
                u32x4 jv = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int d = 0; d < 16; ++d) {
                    const float mv = (float)(sum[d] / hw);
                    jv[d >> 2] |= ((uint32_t)(int)code_of(mv, s_fc, qmin, qmax) & 0xffu) << (8 * (d & 3));
                }
                s_j[cb] = jv;
            }
        }
        __syncthreads();          // the chunk's codes are in LDS
        // phase 2: a lane's 16-byte steps against every row of its wave
        for (int i = lane; i < nb; i += 64) {
            const u32x4 jv = s_j[i];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = wave + 4 * r;
                if (o < q.O) acc[r] = dot16(jv, wt[(int64_t)o * q.CB + c0 + i], acc[r]);
            }
        }
        __syncthreads();          // the codes are read before the next chunk overwrites them
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = wave + 4 * r;
        if (o >= q.O) continue;          // (wave-uniform)
        int s = acc[r];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
        if (lane == 0) y[(int64_t)blockIdx.x * q.O + o] = (float)s * mn_u2f(tab[PF_AL + o]) + mn_u2f(tab[PF_B + o]);
    }
}

}  // namespace mn_iao8

extern "C" int mn_i8first_fwd2(const mn_conv_geom* g, int in_bits, int w_bits, const uint32_t* table, const float* x, const mn_i8first_outs* q, int8_t* out_a, int8_t* out_b,
                               mn_stream_t stream) {
    mn_iao8::FGeom m;
    if (!table || !x || !q || !out_a || !aligned16(table) || (((uintptr_t)x) & 3) || !aligned16(out_a) || !aligned16(out_b) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_i8first_fwd2: null / unaligned argument (x 4-byte, table and codes 16-byte aligned) or invalid geometry");
    if (q->nout < 1 || q->nout > 2 || (q->nout == 2) != (out_b != nullptr)) MN_FAIL(MN_EINVAL, "mn_i8first_fwd2: nout must be 1 (out_b null) or 2 (out_b set)");
    const float sk[2] = {q->s_out0, q->s_out1};
    const int bk[2] = {q->bits0, q->bits1};
    for (int k = 0; k < q->nout; ++k)
        if (!mn_iao8::scale_ok(sk[k]) || bk[k] < 2 || bk[k] > 8) MN_FAIL(MN_EINVAL, "mn_i8first_fwd2: output %d: the scale must be finite and positive, the width 2 .. 8", k);
    if (!mn_iao8::make_fgeom(g, in_bits, q->bits0, w_bits, m))
        MN_FAIL(MN_ENOTSUP, "mn_i8first_fwd2: geometry or width not covered (what mn_i8first_supported covers: 3x3 or 5x5 / stride 1 / dilation 1 / padding (KS - 1) / 2, "
                            "groups 1, C * KS * KS <= 128, code widths 2 .. 8)");
    const int64_t nx = 4ll * m.N * m.C * m.H * m.W, nout = 16ll * m.N * m.OB * m.H * m.W, ntab = 4 * mn_iao8::table_words(m);
    int8_t* const outs[2] = {out_a, out_b};
    for (int k = 0; k < q->nout; ++k)
        if (mn_iao8::ranges_meet(outs[k], nout, x, nx) || mn_iao8::ranges_meet(outs[k], nout, table, ntab) || (k == 1 && mn_iao8::ranges_meet(out_a, nout, out_b, nout)))
            MN_FAIL(MN_EINVAL, "mn_i8first_fwd2: output %d overlaps the image, the table or the other output", k);
    mn_iao8::FFwd f;
    f.C = m.C; f.H = m.H; f.W = m.W; f.HW = m.H * m.W; f.OB = m.OB; f.K = m.K; f.nsteps = m.nsteps; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride;
    f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off; f.bpi = m.bpi; f.rows = m.rows; f.TW = m.TW;
    mn_iao8::FOuts p;
    for (int k = 0; k < 2; ++k) {
        const int kk = k < q->nout ? k : 0;
        p.s[k] = sk[kk]; p.qmin[k] = -(float)(1 << (bk[kk] - 1)); p.qmax[k] = (float)((1 << (bk[kk] - 1)) - 1);
    }
    const int bx = m.N * m.bpi;          // (< 2^27: make_fgeom bounds N * OB * H * W)
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    u32x4* ya = reinterpret_cast<u32x4*>(out_a);
    u32x4* yb = reinterpret_cast<u32x4*>(out_b);
    mn_set_last_kernel("k_i8first2<%d,%d>", m.KS, q->nout);
    mn_prof_bytes((double)nx + (double)nout * q->nout + (double)ntab);
    mn_prof_begin(s);
#define MN_I8FIRST2_LAUNCH(KS, NO) hipLaunchKernelGGL((mn_iao8::k_i8first2<KS, NO>), grid, dim3(256), (size_t)m.lds, s, table, x, ya, yb, f, p)
    if (m.KS == 5) { if (q->nout == 2) MN_I8FIRST2_LAUNCH(5, 2); else MN_I8FIRST2_LAUNCH(5, 1); }
    else { if (q->nout == 2) MN_I8FIRST2_LAUNCH(3, 2); else MN_I8FIRST2_LAUNCH(3, 1); }
#undef MN_I8FIRST2_LAUNCH
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_i8first_fwd2");
    return MN_OK;
}

// (passed as an argument of "%s", never as a format)
#define MN_I8POOLFC_COVER "shape or width not covered (1 <= O <= 64, 1 <= HW <= 4096, code widths 2 .. 8, C * 2^(a-1) * (2^(w-1) - 1) <= INT_MAX)"

extern "C" int mn_i8poolfc_supported(int64_t N, int64_t C, int64_t HW, int64_t O, int p_bits, int a_bits, int w_bits) {
    mn_iao8::PGeom m;
    return mn_iao8::make_pgeom(N, C, HW, O, p_bits, a_bits, w_bits, m) ? 1 : 0;
}

extern "C" int64_t mn_i8poolfc_table_bytes(int64_t C, int64_t O, int p_bits, int a_bits, int w_bits) {
    mn_iao8::PGeom m;
    if (!mn_iao8::make_pgeom(1, C, 1, O, p_bits, a_bits, w_bits, m)) return 0;
    return 4 * mn_iao8::pf_table_words(m);
}

extern "C" int mn_i8poolfc_pack(int64_t C, int64_t O, const float* w, const float* s_w, int s_w_stride, const float* bias, float s_p, float s_fc, int p_bits, int a_bits,
                                int w_bits, uint32_t* table, mn_stream_t stream) {
    mn_iao8::PGeom m;
    if (!w || !s_w || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)s_w | (uintptr_t)bias) & 3) || s_w_stride < 0 || s_w_stride > 1 || C <= 0 || O <= 0)
        MN_FAIL(MN_EINVAL, "mn_i8poolfc_pack: null / unaligned argument (the table is 16-byte aligned), s_w_stride outside 0 / 1 or C, O <= 0");
    if (!mn_iao8::make_pgeom(1, C, 1, O, p_bits, a_bits, w_bits, m)) MN_FAIL(MN_ENOTSUP, "mn_i8poolfc_pack: %s", MN_I8POOLFC_COVER);
    if (hipMemsetAsync(table, 0, 4 * mn_iao8::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_i8poolfc_pack: header reset failed");          // the two counters
    mn_set_last_kernel("k_i8poolfc_wpack");
    hipLaunchKernelGGL(mn_iao8::k_i8poolfc_wpack, dim3(m.O), dim3(256), 0, (hipStream_t)stream, m, w, s_w, s_w_stride, bias, s_p, s_fc, table);
    MN_CHECK_LAUNCH("mn_i8poolfc_pack");
    return MN_OK;
}

extern "C" int mn_i8poolfc_fwd(int64_t N, int64_t C, int64_t HW, int64_t O, int p_bits, int a_bits, int w_bits, const uint32_t* table, const int8_t* in_codes, float* y,
                               mn_stream_t stream) {
    mn_iao8::PGeom m;
    if (!table || !in_codes || !y || !aligned16(table) || !aligned16(in_codes) || (((uintptr_t)y) & 3) || N <= 0 || C <= 0 || HW <= 0 || O <= 0)
        MN_FAIL(MN_EINVAL, "mn_i8poolfc_fwd: null / unaligned argument (y 4-byte, table and codes 16-byte aligned) or N, C, HW, O <= 0");
    if (!mn_iao8::make_pgeom(N, C, HW, O, p_bits, a_bits, w_bits, m) || N > 0x7fffffffll) MN_FAIL(MN_ENOTSUP, "mn_i8poolfc_fwd: %s", MN_I8POOLFC_COVER);
    const int64_t nin = 16 * m.N * m.CB * m.HW, ny = 4 * m.N * m.O;
    if (mn_iao8::ranges_meet(y, ny, in_codes, nin) || mn_iao8::ranges_meet(y, ny, table, 4 * mn_iao8::pf_table_words(m)))
        MN_FAIL(MN_EINVAL, "mn_i8poolfc_fwd: the output overlaps the input or the table");
    mn_iao8::PFwd f;
    f.CB = m.CB; f.HW = m.HW; f.O = m.O;
    const hipStream_t s = (hipStream_t)stream;
    mn_set_last_kernel("k_i8poolfc");
    mn_prof_bytes((double)nin + (double)ny + 4.0 * (double)mn_iao8::pf_table_words(m));
    mn_prof_begin(s);
    hipLaunchKernelGGL(mn_iao8::k_i8poolfc, dim3((unsigned)m.N), dim3(256), 0, s, table, reinterpret_cast<const u32x4*>(in_codes), y, f);
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_i8poolfc_fwd");
    return MN_OK;
}
#undef MN_I8POOLFC_COVER
