// The int8-MFMA form of the 1x1 hidden bit block (mn_bitconv_mfma_*): bits in, bits out, the layout, out_order, decision and header word 0 of qgemm_bits.hip -- only the
// contraction differs, so the output words equal mn_bitconv_fwd's word for word.  Included by qgemm_bits.hip behind the three code headers; the 1-bit counterpart of
// qgemm_codes_mfma.h, whose set / tile layout and bit spread it shares.
//
//   contraction  : v_mfma_i32_16x16x64_i8 (mn_mfma_i8).  A = the weight signs t in {-1, 0, +1} as bytes (M = 16 output rows of ONE group), B = the activation BITS
//                  b in {0, 1} as bytes (N = 16 pixels): the MFMA forms P = sum b t, and the accumulator k_bitconv forms is acc = sum (2 b - 1) t = 2 P - sum t.  The
//                  pack folds sum t into the stored threshold, T' = ceil((T + sum t) / 2): P >= T' iff acc >= T for every integer P -- no nnz term, no group mask.
//                  K is the group's channels in their own order, padded with zero weight bytes to a multiple of 64; a group starts on an input word (groups == 1, or
//                  C / groups % 32 == 0), so byte e of lane (n, kq) at step s is bit 16 (kq & 1) + e of word w0 + 2 s + (kq >> 1): ONE dword load and a
//                  multiply-and-mask bit spread per step.  Tail bits, channels of a neighbouring group inside the last step and words past the pixel's last (read as
//                  0) meet zero weight bytes.
//   weight table : (private layout, 16-byte aligned: the set / tile table of qgemm_mfma_sets.h, a set = two consecutive output words) 8 header words -- [0] rows
//                  whose decision is not monotone in acc + bad out_order entries, [1] k-steps, [2] tile slots per set, [3] tile stride, [4] rows, [5] Cw -- then the
//                  tile count of every set, then the tiles:
//                    [0] w0, [1] 1: first tile of its group in the set, [16 ..) T'[16], dest[16] (32 * word in set + bit),
//                    [48 ..) per k-step 64 lanes x 16 bytes in the A-operand order of mn_mfma_i8 (lane = 16 kq + row).
//                  A dead row: T' = INT_MAX, zero weights: never a bit.  The bits of positions without a row stay 0.
//   kernel       : a wave owns 64 pixels as four N tiles (pool: the four sub-pixels of the 2x2 windows of 16 pooled pixels -- OR of four decisions = the window's
//                  largest P >= T', a maximum over four accumulators in the lane).  The expanded bits of the wave's pixels stay in registers across all M tiles of a
//                  group (up to three k-steps; beyond that they are re-expanded per tile from L1 / L2); the weight bytes stream from the L2-resident table.  Every lane
//                  ORs the bits of its four rows into the set's two words at its pixels, the four lane groups are combined by two shuffle steps, and every output word
//                  is stored once, whole, coalesced along pixels: no atomics, no read-modify-write.
// Covered: 1x1, stride 1, padding 0, in_shuffle 0 / 1; groups == 1 with any C or C / groups % 32 == 0; any O; pool 0 / 1; W = 3 and W = 2 weights alike.
#pragma once
#include "qgemm_codes_mfma.h"

namespace mn_bits_mfma {

using mn_bits::Geom;
using mn_sets::SETROWS;
using mn_sets::table_words;
enum { HDR = mn_bits::HDR, THDR = 16, TMETA = 32, TA = THDR + TMETA, STEPW = 256, MAXNK = 3 };

struct MGeom {
    Geom q;
    int nsteps, nsets, slots, tstride, tiles_off;          // k-steps of 64 channels, sets of two output words, tile slots per set, words per tile, first tile
};

static inline bool make_mgeom(const mn_conv_geom* g, MGeom& m) {
    if (!mn_bits::make_geom(g, m.q, false) || m.q.KS != 1) return false;
    if (m.q.groups > 1 && (m.q.Cg & 31)) return false;          // every group starts on a word
    m.nsteps = (m.q.Cg + 63) >> 6;
    m.nsets = (m.q.OW + 1) >> 1;
    m.tstride = TA + STEPW * m.nsteps;
    return mn_sets::table_layout(m, m.q.groups, HDR);
}

// the weight sign k_bits_wpack's planes encode: m = (v != 0), s = (v > 0)
__device__ __forceinline__ int sign_of(float v) { return v > 0.f ? 1 : v != 0.f ? -1 : 0; }

// One thread, one row of K weights at stride `ws`: the threshold T of k_bits_wpack (alpha = max |w|, NaN if any weight is; the shared search) and sum t.
__device__ __forceinline__ int row_threshold(const float* wr, int K, float b, int& st, bool& mono) {
    float mx = 0.f;
    int nan = 0;
    st = 0;
    for (int i = 0; i < K; ++i) {
        const float v = wr[i];
        mx = fmaxf(mx, fabsf(v));
        nan |= v != v;
        st += sign_of(v);
    }
    const float alpha = nan ? mn_u2f(0x7fc00000u) : mx;
    int tmin, cnt;
    mn_bits::decision_scan(K, alpha, b, 0, 1, tmin, cnt);
    mono = mn_bits::decision_monotone(K, tmin, cnt);
    return mn_bits::decision_threshold(K, tmin, cnt);
}

// ---------------------------------------------------------------- weight table: one block per set
__global__ __launch_bounds__(256) void k_bits_mfma_wpack(MGeom m, const float* __restrict__ w, const float* __restrict__ bias, const int32_t* __restrict__ order,
                                                         uint32_t* __restrict__ tab) {
    __shared__ mn_sets::SetPlan sp;
    const Geom& q = m.q;
    const int set = blockIdx.x, tid = threadIdx.x;
    if (set == 0 && tid == 0) { tab[1] = (uint32_t)m.nsteps; tab[2] = (uint32_t)m.slots; tab[3] = (uint32_t)m.tstride; tab[4] = (uint32_t)(q.OW * 32); tab[5] = (uint32_t)q.Cw; }
    uint32_t* tiles = tab + m.tiles_off + (int64_t)set * m.slots * m.tstride;
    // every slot starts as a tile of dead rows: T' = INT_MAX, zero weight bytes
    for (int i = tid; i < m.slots * m.tstride; i += 256) {
        const int r = i % m.tstride;
        tiles[i] = (r >= THDR && r < THDR + 16) ? 0x7fffffffu : 0u;
    }
    int nt;
    const int before = mn_sets::plan_set(order, q.O, q.Og, set, tab + 0, sp, nt);
    if (tid == 0) tab[HDR + set] = (uint32_t)nt;
    // weight signs: thread = 4 consecutive channels of one row, one dword of the A operand (lane 16 kq + row, byte e = channel & 15 of k-step channel >> 6)
    const int kq4 = m.nsteps * 16;          // dwords per row
    for (int idx = tid; idx < SETROWS * kq4; idx += 256) {
        const int pos = idx / kq4, k4 = (idx - pos * kq4) * 4;
        const int o = sp.chan[pos];
        if (o < 0 || k4 >= q.Cg) continue;
        const float* wr = w + (int64_t)o * q.Cg + k4;
        uint32_t v = 0u;
        for (int e = 0; e < 4 && k4 + e < q.Cg; ++e) v |= ((uint32_t)sign_of(wr[e]) & 0xffu) << (8 * e);
        uint32_t* A = tiles + (int64_t)sp.tile[pos] * m.tstride + TA;
        A[(k4 >> 6) * STEPW + ((((k4 >> 4) & 3) * 16 + sp.row[pos]) * 4) + ((k4 & 15) >> 2)] = v;
    }
    // thresholds: T of k_bits_wpack on acc = 2 P - sum t, stored for P
    if (tid < SETROWS && sp.chan[tid] >= 0) {
        const int o = sp.chan[tid], r = sp.row[tid];
        uint32_t* T = tiles + (int64_t)sp.tile[tid] * m.tstride;
        int st;
        bool mono;
        const int th = row_threshold(w + (int64_t)o * q.Cg, q.Cg, bias ? bias[o] : 0.f, st, mono);
        if (!mono) atomicAdd(tab + 0, 1u);
        T[THDR + r] = (uint32_t)((th + st + 1) >> 1);          // ceil((T + sum t) / 2); |T + sum t| <= 2 K + 1
        T[THDR + 16 + r] = (uint32_t)tid;                      // 32 * word in set + bit
        if (r == 0) {
            T[0] = (uint32_t)(sp.grp[tid] * q.Cg >> 5);
            T[1] = (uint32_t)((before >> 4) == 0);
        }
    }
}

// ---------------------------------------------------------------- MFMA contraction + threshold -> output bits
struct MFwd {
    int total, Cw, H, W, Ho, Wo, OW, nsteps, nsets, slots, tstride, tiles_off, spb;
};

// NK > 0: exactly NK k-steps, the expanded B operands of the wave's four N tiles in registers across the tiles of a group; NK == 0: any number, re-expanded per tile.
template <int NK, bool POOL>
__global__ __launch_bounds__(256) void k_bitconv_mfma(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, uint32_t* __restrict__ y, MFwd q) {
    constexpr int NKR = NK ? NK : 1, NA = POOL ? 1 : 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HW = q.H * q.W, HWo = q.Ho * q.Wo;
    const int pb = ((int)blockIdx.x * 4 + wave) * (POOL ? 16 : 64);
    int xoff[4];          // word 0 at the pixel of N tile t, -1 past the end
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = POOL ? pb + n : pb + 16 * t + n;
        const int pc = p < q.total ? p : 0;
        const int img = pc / HWo, r = pc - img * HWo;
        int pix = r;
        if (POOL) { const int oh = r / q.Wo, ow = r - oh * q.Wo; pix = (2 * oh + (t >> 1)) * q.W + 2 * ow + (t & 1); }
        xoff[t] = p < q.total ? img * q.Cw * HW + pix : -1;
    }
    // what this lane stores: N tile kq (pool: word kq >> 1 of pooled pixel n, lane groups 0 and 2)
    const int ps = POOL ? pb + n : pb + 16 * kq + n;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HWo;
    uint32_t* const ybase = y + (int64_t)simg * q.OW * HWo + (psc - simg * HWo);
    const int sh = 16 * (kq & 1);
    auto loadb = [&](int t, int s, int w0) {
        const int wg = w0 + 2 * s + (kq >> 1);
        uint32_t p0 = 0u;
        if (xoff[t] >= 0 && wg < q.Cw) p0 = x[xoff[t] + (int64_t)wg * HW];
        return mn_codes_mfma::spread16((p0 >> sh) & 0xffffu, 0u);
    };
    u32x4 breg[NKR][4];
#pragma unroll
    for (int s = 0; s < NKR; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) breg[s][t] = u32x4{0u, 0u, 0u, 0u};
    const int nsteps = NK ? NK : q.nsteps;
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        const int nt = (int)tab[HDR + set] < q.slots ? (int)tab[HDR + set] : q.slots;          // wave-uniform
        uint32_t wa[NA][2];          // [word 0, word 1] of the set at the lane's pixels: the bits of this lane's rows
#pragma unroll
        for (int t = 0; t < NA; ++t) wa[t][0] = wa[t][1] = 0u;
        for (int i = 0; i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            const int w0 = (int)tile[0];
            if (NK && tile[1]) {          // (wave-uniform) a new group: expand its bits once
#pragma unroll
                for (int s = 0; s < NKR; ++s)
#pragma unroll
                    for (int t = 0; t < 4; ++t) breg[s][t] = loadb(t, s, w0);
            }
            i32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = i32x4{0, 0, 0, 0};
            const uint32_t* ap = tile + TA + lane * 4;
            if (NK) {
                u32x4 a[NKR];
#pragma unroll
                for (int s = 0; s < NKR; ++s) a[s] = *reinterpret_cast<const u32x4*>(ap + s * STEPW);
#pragma unroll
                for (int s = 0; s < NKR; ++s)
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = mn_mfma_i8(a[s], breg[s][t], acc[t]);
            } else {
#pragma unroll 1
                for (int s = 0; s < nsteps; ++s) {
                    const u32x4 a = *reinterpret_cast<const u32x4*>(ap + s * STEPW);
                    u32x4 b[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) b[t] = loadb(t, s, w0);
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = mn_mfma_i8(a, b[t], acc[t]);
                }
            }
            // the lane's rows 4 kq .. 4 kq + 3 of the tile (D[row = 4 kq + reg][col = n])
            const i32x4 th = *reinterpret_cast<const i32x4*>(tile + THDR + 4 * kq);
            const u32x4 ds = *reinterpret_cast<const u32x4*>(tile + THDR + 16 + 4 * kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t m0 = ds[r] < 32u ? 1u << (ds[r] & 31u) : 0u, m1 = ds[r] < 32u ? 0u : 1u << (ds[r] & 31u);
#pragma unroll
                for (int t = 0; t < NA; ++t) {
                    int sv;
                    if (POOL) {
                        sv = acc[0][r];
#pragma unroll
                        for (int tt = 1; tt < 4; ++tt) sv = acc[tt][r] > sv ? acc[tt][r] : sv;
                    } else {
                        sv = acc[t][r];
                    }
                    const uint32_t hit = sv >= th[r] ? 0xffffffffu : 0u;
                    wa[t][0] |= hit & m0; wa[t][1] |= hit & m1;
                }
            }
        }
        // combine the four lane groups (rows 4 kq .. of every tile)
        const bool hi = (kq & 2) != 0, odd = (kq & 1) != 0;
        if (POOL) {
            // [word 0, word 1] of the lane's pooled pixel: lane groups 0 / 1 end with word 0, 2 / 3 with word 1
            uint32_t val = hi ? wa[0][1] : wa[0][0];
            val |= (uint32_t)__shfl_xor((int)(hi ? wa[0][0] : wa[0][1]), 32, 64);
            val |= (uint32_t)__shfl_xor((int)val, 16, 64);
            const int word = 2 * set + (kq >> 1);
            if (sok && !odd && word < q.OW) ybase[(int64_t)word * HWo] = val;
        } else {
            // a reduce-scatter: lane group kq ends with the words of N tile kq -- keep two tiles across xor 32, one across xor 16
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint32_t v[4] = {wa[0][c], wa[1 % NA][c], wa[2 % NA][c], wa[3 % NA][c]};
                uint32_t ka = hi ? v[2] : v[0], kb = hi ? v[3] : v[1];
                ka |= (uint32_t)__shfl_xor((int)(hi ? v[0] : v[2]), 32, 64);
                kb |= (uint32_t)__shfl_xor((int)(hi ? v[1] : v[3]), 32, 64);
                uint32_t val = odd ? kb : ka;
                val |= (uint32_t)__shfl_xor((int)(odd ? ka : kb), 16, 64);
                const int word = 2 * set + c;
                if (sok && word < q.OW) ybase[(int64_t)word * HWo] = val;
            }
        }
    }
}

template <bool POOL>
static void launch(int nk, dim3 grid, hipStream_t s, const uint32_t* tab, const uint32_t* x, uint32_t* y, const MFwd& f) {
    switch (nk) {
    case 1: hipLaunchKernelGGL((k_bitconv_mfma<1, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    case 2: hipLaunchKernelGGL((k_bitconv_mfma<2, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    case 3: hipLaunchKernelGGL((k_bitconv_mfma<3, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    default: hipLaunchKernelGGL((k_bitconv_mfma<0, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    }
}

}  // namespace mn_bits_mfma

#define MN_BITMFMA_COVER "geometry not covered (1x1, stride 1, no padding, no input shuffle, groups 1 or C / groups %% 32 == 0)"

extern "C" int mn_bitconv_mfma_supported(const mn_conv_geom* g) {
    mn_bits_mfma::MGeom m;
    return mn_bits_mfma::make_mgeom(g, m) ? 1 : 0;
}

extern "C" int64_t mn_bitconv_mfma_table_bytes(const mn_conv_geom* g) {
    mn_bits_mfma::MGeom m;
    if (!mn_bits_mfma::make_mgeom(g, m)) return 0;
    return 4 * mn_bits_mfma::table_words(m);
}

extern "C" int mn_bitconv_mfma_pack(const mn_conv_geom* g, const float* w, const float* bias, const int32_t* out_order, uint32_t* table, mn_stream_t stream) {
    mn_bits_mfma::MGeom m;
    if (!w || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)bias | (uintptr_t)out_order) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_bitconv_mfma_pack: null / unaligned argument (the table is 16-byte aligned) or invalid geometry");
    if (!mn_bits_mfma::make_mgeom(g, m)) MN_FAIL(MN_ENOTSUP, "mn_bitconv_mfma_pack: " MN_BITMFMA_COVER);
    if (hipMemsetAsync(table, 0, 4 * mn_bits_mfma::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_bitconv_mfma_pack: header reset failed");          // word 0: bad-row count
    mn_set_last_kernel("k_bits_mfma_wpack");
    hipLaunchKernelGGL(mn_bits_mfma::k_bits_mfma_wpack, dim3(m.nsets), dim3(256), 0, (hipStream_t)stream, m, w, bias, out_order, table);
    MN_CHECK_LAUNCH("mn_bitconv_mfma_pack");
    return MN_OK;
}

extern "C" int mn_bitconv_mfma_fwd(const mn_conv_geom* g, const uint32_t* table, const uint32_t* x_bits, uint32_t* y_bits, int pool, mn_stream_t stream) {
    mn_bits_mfma::MGeom m;
    if (!table || !x_bits || !y_bits || !aligned16(table) || ((((uintptr_t)x_bits) | ((uintptr_t)y_bits)) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_bitconv_mfma_fwd: null / unaligned argument (the table is 16-byte aligned) or invalid geometry");
    if (!mn_bits_mfma::make_mgeom(g, m)) MN_FAIL(MN_ENOTSUP, "mn_bitconv_mfma_fwd: " MN_BITMFMA_COVER);
    if (pool < 0 || pool > 1) MN_FAIL(MN_ENOTSUP, "mn_bitconv_mfma_fwd: pool must be 0 or 1 (2x2 / stride 2); the 3x3 / stride 2 fold stays on mn_bitconv_fwd");
    const mn_bits::Geom& q = m.q;
    if (pool && ((q.H & 1) || (q.W & 1))) MN_FAIL(MN_EINVAL, "mn_bitconv_mfma_fwd: the folded 2x2 max-pool needs even H and W");
    mn_bits_mfma::MFwd f;
    f.Cw = q.Cw; f.H = q.H; f.W = q.W; f.OW = q.OW; f.nsteps = m.nsteps; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride; f.tiles_off = m.tiles_off;
    f.Ho = pool ? q.H / 2 : q.H; f.Wo = pool ? q.W / 2 : q.W;
    f.total = q.N * f.Ho * f.Wo;
    const int ppb = pool ? 64 : 256;          // (pooled) pixels per block: four waves of four N tiles
    const int bx = (f.total + ppb - 1) / ppb;
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const int nk = m.nsteps <= mn_bits_mfma::MAXNK ? m.nsteps : 0;
    mn_set_last_kernel("k_bitconv_mfma<%d>", pool);
    mn_prof_bytes(4.0 * q.N * q.Cw * q.H * q.W + 4.0 * q.N * q.OW * f.Ho * f.Wo + 4.0 * (double)mn_bits_mfma::table_words(m));
    mn_prof_begin(s);
    if (pool) mn_bits_mfma::launch<true>(nk, grid, s, table, x_bits, y_bits, f);
    else mn_bits_mfma::launch<false>(nk, grid, s, table, x_bits, y_bits, f);
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_bitconv_mfma_fwd");
    return MN_OK;
}
#undef MN_BITMFMA_COVER
