// The int8-MFMA form of the 1x1 hidden code block (mn_codeconv_mfma_*): planes in, planes out, thresholds and bits of qgemm_codes.h -- only the contraction differs.
// Included by qgemm_bits.hip behind qgemm_codes.h.
//
//   contraction  : v_mfma_i32_16x16x64_i8 (mn_mfma_i8).  A = weights as signed bytes 2k - 3 (M = 16 output rows of ONE group), B = activation codes j in [0, 3] as
//                  bytes (N = 16 pixels), so acc = sum_c j_c (2 k_c - 3) is the integer k_codeconv forms as 2 sum j k - 3 sum j: no sum j term, no group mask.  K is
//                  the group's channels in their own order, padded with zero weight bytes to a multiple of 64; a group starts on an input word (groups == 1, or
//                  C / groups % 32 == 0), so byte e of lane (n, kq) at step s is bit 16 (kq & 1) + e of word group w0 + 2 s + (kq >> 1): two dword loads (plane 0,
//                  plane 1) and a multiply-and-mask bit spread per step, no per-bit loop.  Tail channels, channels of a neighbouring group inside the last step and
//                  word groups past the pixel's last (read as 0) meet zero weight bytes: no mask.
//   weight table : (private layout, 16-byte aligned: the set / tile table of qgemm_mfma_sets.h, a set = two consecutive output words) 8 header words -- [0] rows
//                  whose channel constants fail qa_finite, [1] k-steps, [2] tile slots per set, [3] tile stride, [4] rows, [5] Cw, [6] a_in | w_bits << 8 | a_out << 16,
//                  [7] bad out_order entries + rows with a weight off the grid -- then the tile count of every set, then the tiles:
//                    [0] w0, [1] 1: first tile of its group in the set, [16 ..) flip[16], T_1[16] <= T_2[16] <= T_3[16], dest[16] (32 * word in set + bit),
//                    [96 ..) per k-step 64 lanes x 16 bytes in the A-operand order of mn_mfma_i8 (lane = 16 kq + row).
//                  A dead row: T = INT_MAX, zero weights: never a bit.  Under nin_gc's "shuffle 2" a word holds 16 + 16 rows, under "shuffle 4" 8 per group -- 16
//                  per group in a set of two words: no dead rows.  The bits of positions without a row stay 0.
//   kernel       : a wave owns 64 pixels as four N tiles (pool: the four sub-pixels of the 2x2 windows of 16 pooled pixels, so the window's largest u = flip * acc is a
//                  maximum over four accumulators in the lane).  The expanded codes of the wave's pixels stay in registers across all M tiles of a group (up to three
//                  k-steps; beyond that they are re-expanded per tile from L1 / L2); the weight bytes stream from the L2-resident table, 16 bytes per lane.  Every
//                  lane ORs the bits of its four rows into the set's two words x two planes at its pixels, the four lane groups are combined by two shuffle steps,
//                  and every output word is stored once, whole, coalesced along pixels: no atomics, no read-modify-write.
//   width        : every kernel here is a template on the code width B = a_in = w_bits = a_out, instantiated for 2 (everything above, unchanged) and 4: weight bytes
//                  2k - 15, B dword loads per (pixel, word group) spread to bytes j = sum_p b_p << p, fifteen sorted thresholds per row (tile metadata 16 (2^B + 1)
//                  words) searched in B branchless steps (code_planes), B planes per output word through the reduce-scatter (pool: B / 2 words per lane group).
// Covered: a_in = w_bits = a_out = 2 or 4; 1x1, stride 1, padding 0; groups == 1 with any C or C / groups % 32 == 0; any O; K * n * n <= 32767 with n = 2^B - 1 (K * 9 at
// 2 bits; at 4 bits dense C <= 145 or C / groups in {32, 64, 96, 128}); pool 0 / 1.
#pragma once
#include "qgemm_codes.h"
#include "qgemm_mfma_sets.h"

namespace mn_codes_mfma {

using mn_codes::Geom;
using mn_sets::SETROWS;
using mn_sets::table_words;
enum { HDR = mn_codes::HDR, THDR = 16, STEPW = 256, MAXNK = 3 };
// per code width B: thresholds per row, words of tile metadata (flip[16], T_1 .. T_(2^B - 1)[16], dest[16]) and the offset of the A operand (a multiple of 4 words)
constexpr int nthr(int B) { return (1 << B) - 1; }
constexpr int tmeta(int B) { return 16 * ((1 << B) + 1); }
constexpr int ta(int B) { return THDR + tmeta(B); }

struct MGeom {
    Geom q;
    int nsteps, nsets, slots, tstride, tiles_off;          // k-steps of 64 channels, sets of two output words, tile slots per set, words per tile, first tile
    int bits;          // the code width B = a_in = w_bits = a_out: 2 or 4
};

static inline bool make_mgeom(const mn_conv_geom* g, int a_in, int w_bits, int a_out, MGeom& m) {
    if (!mn_codes::make_geom(g, a_in, w_bits, a_out, m.q, false, true) || m.q.KS != 1) return false;
    if (m.q.groups > 1 && (m.q.Cg & 31)) return false;          // every group starts on a word
    m.bits = a_in;
    m.nsteps = (m.q.Cg + 63) >> 6;
    m.nsets = (m.q.OW + 1) >> 1;
    m.tstride = ta(m.bits) + STEPW * m.nsteps;
    return mn_sets::table_layout(m, m.q.groups, HDR);
}

// ---------------------------------------------------------------- weight table: one block per set
template <int B>
__global__ __launch_bounds__(256) void k_codes_mfma_wpack(MGeom m, const float* __restrict__ w, const float* __restrict__ chan, const int32_t* __restrict__ order,
                                                          uint32_t* __restrict__ tab) {
    constexpr int NTHR = nthr(B), TA = ta(B);
    __shared__ mn_sets::SetPlan sp;
    const Geom& q = m.q;
    const int set = blockIdx.x, tid = threadIdx.x;
    if (set == 0 && tid == 0) {
        tab[1] = (uint32_t)m.nsteps; tab[2] = (uint32_t)m.slots; tab[3] = (uint32_t)m.tstride; tab[4] = (uint32_t)(q.OW * 32); tab[5] = (uint32_t)q.Cw;
        tab[6] = (uint32_t)(B | (B << 8) | (B << 16));
    }
    uint32_t* tiles = tab + m.tiles_off + (int64_t)set * m.slots * m.tstride;
    // every slot starts as a tile of dead rows: flip 1, T = INT_MAX, zero weight bytes
    for (int i = tid; i < m.slots * m.tstride; i += 256) {
        const int r = i % m.tstride;
        tiles[i] = (r >= THDR + 16 && r < THDR + 16 * (NTHR + 1)) ? 0x7fffffffu : (r >= THDR && r < THDR + 16) ? 1u : 0u;
    }
    int nt;
    const int before = mn_sets::plan_set(order, q.O, q.Og, set, tab + 7, sp, nt);
    if (tid == 0) tab[HDR + set] = (uint32_t)nt;
    // weight bytes 2k - (2^B - 1): thread = 4 consecutive channels of one row, one dword of the A operand (lane 16 kq + row, byte e = channel & 15 of k-step channel >> 6)
    const int kq4 = m.nsteps * 16;          // dwords per row
    const float nf = (float)NTHR;
    for (int idx = tid; idx < SETROWS * kq4; idx += 256) {
        const int pos = idx / kq4, k4 = (idx - pos * kq4) * 4;
        const int o = sp.chan[pos];
        if (o < 0 || k4 >= q.Cg) continue;
        const float* wr = w + (int64_t)o * q.Cg + k4;
        uint32_t v = 0u;
        int off = 0;
        for (int e = 0; e < 4 && k4 + e < q.Cg; ++e) {
            const float kf = (wr[e] * nf + nf) * 0.5f;          // w = (2k - n) / n
            const float kr = rintf(kf);
            if (!(fabsf(kf - kr) <= 1e-3f) || kr < 0.f || kr > nf) off = 1;
            const int kc = (int)(kr < 0.f ? 0.f : kr > nf ? nf : kr == kr ? kr : 0.f);
            v |= ((uint32_t)(2 * kc - NTHR) & 0xffu) << (8 * e);
        }
        if (off) sp.off[pos] = 1;
        uint32_t* A = tiles + (int64_t)sp.tile[pos] * m.tstride + TA;
        A[(k4 >> 6) * STEPW + ((((k4 >> 4) & 3) * 16 + sp.row[pos]) * 4) + ((k4 & 15) >> 2)] = v;
    }
    // thresholds: the search of k_qa_fwd on the block's eval-mode constants (qa_thresholds.h, as k_codes_wpack)
    if (tid < SETROWS && sp.chan[tid] >= 0) {
        const int o = sp.chan[tid], r = sp.row[tid];
        uint32_t* T = tiles + (int64_t)sp.tile[tid] * m.tstride;
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
        T[THDR + 16 * (NTHR + 1) + r] = (uint32_t)tid;          // 32 * word in set + bit
        if (!fin) atomicAdd(tab + 0, 1u);
        if (r == 0) {
            const int c0 = sp.grp[tid] * q.Cg;
            T[0] = (uint32_t)(c0 >> 5);
            T[1] = (uint32_t)((before >> 4) == 0);
        }
    }
    mn_sets::tally_off(sp, tab + 7);
}

// ---------------------------------------------------------------- MFMA contraction + thresholds -> output planes
struct MFwd {
    int total, Cw, H, W, Ho, Wo, OW, nsteps, nsets, slots, tstride, tiles_off, spb;
};

// 16 bits of plane 0 / plane 1 -> 16 bytes j = b0 + 2 b1: a nibble times 0x00204081 puts bit i at 8 i (the products 7 a + i are distinct: no carries)
__device__ __forceinline__ u32x4 spread16(uint32_t p0, uint32_t p1) {
    u32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        r[i] = ((((p0 >> (4 * i)) & 0xfu) * 0x00204081u) & 0x01010101u) | (((((p1 >> (4 * i)) & 0xfu) * 0x00204081u) & 0x01010101u) << 1);
    return r;
}
// the same for B planes: byte = sum_p b_p << p (B == 2 is spread16 itself)
template <int B>
__device__ __forceinline__ u32x4 spread16(const uint32_t (&p)[B]) {
    if constexpr (B == 2) {
        return spread16(p[0], p[1]);
    } else {
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t v = 0u;
#pragma unroll
            for (int b = 0; b < B; ++b) v |= ((((p[b] >> (4 * i)) & 0xfu) * 0x00204081u) & 0x01010101u) << b;
            r[i] = v;
        }
        return r;
    }
}

// The B plane masks (all-ones / zero per lane) of the codes of the lane's rows 4 kq .. 4 kq + 3 of tile `tl` at NT values each: code = #{k : u >= T_k} with the row's
// thresholds sorted, so bit B - 1 of the code is (u >= T_(2^(B-1))) and every further bit is one compare against the threshold in the middle of the interval the bits
// above it have left: a B-step branchless binary search, the generalisation of the g2 / g0 select of the 2-bit form (which is this with B = 2).  As there, s = acc ^ ng
// (ng = 0 / -1 by flip) and E_k = min(T_k, 40000) - 1 + ng, so u >= T_k iff E_k - s < 0.  Level l loads its 2^l threshold vectors (four rows each) only when it runs,
// and selects among their E by the masks of the levels above: g[l] is plane B - 1 - l.
template <int B, int NT>
__device__ __forceinline__ void code_planes(const uint32_t* tl, int kq, const int (&ng)[4], const int (&sv)[4][NT], uint32_t (&g)[B][4][NT]) {
    constexpr int HALF = 1 << (B - 1);
#pragma unroll
    for (int l = 0; l < B; ++l) {
        i32x4 tv[HALF];
#pragma unroll
        for (int j = 0; j < HALF; ++j)
            if (j < (1 << l)) tv[j] = *reinterpret_cast<const i32x4*>(tl + THDR + 16 * ((2 * j + 1) << (B - 1 - l)) + 4 * kq);          // T_k, k = (2 j + 1) 2^(B-1-l)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int e[HALF];
#pragma unroll
            for (int j = 0; j < HALF; ++j)
                if (j < (1 << l)) e[j] = (tv[j][r] < 40000 ? tv[j][r] : 40000) - 1 + ng[r];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                uint32_t c[HALF];
#pragma unroll
                for (int j = 0; j < HALF; ++j) c[j] = j < (1 << l) ? (uint32_t)e[j] : 0u;
                // j's bits are the masks of the levels above, g[0] the most significant: fold the least significant first
#pragma unroll
                for (int b = l - 1, w = (1 << l) >> 1; b >= 0; --b, w >>= 1)
#pragma unroll
                    for (int j = 0; j < HALF / 2; ++j)
                        if (j < w) c[j] = (g[b][r][t] & c[2 * j + 1]) | (~g[b][r][t] & c[2 * j]);
                g[l][r][t] = (uint32_t)(((int)c[0] - sv[r][t]) >> 31);
            }
        }
    }
}

// NK > 0: exactly NK k-steps, the expanded B operands of the wave's four N tiles in registers across the tiles of a group; NK == 0: any number, re-expanded per tile.
// B: the code width (planes per word group in and out, thresholds per row); B == 2 is the kernel as it was.
template <int B, int NK, bool POOL>
__global__ __launch_bounds__(256) void k_codeconv_mfma(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ x, uint32_t* __restrict__ y, MFwd q) {
    constexpr int NKR = NK ? NK : 1, NA = POOL ? 1 : 4, TA = ta(B), LB = B == 2 ? 1 : 2;          // LB = log2(B)
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HW = q.H * q.W, HWo = q.Ho * q.Wo;
    const int pb = ((int)blockIdx.x * 4 + wave) * (POOL ? 16 : 64);
    int xoff[4];          // plane 0 of word group 0 at the pixel of N tile t, -1 past the end
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = POOL ? pb + n : pb + 16 * t + n;
        const int pc = p < q.total ? p : 0;
        const int img = pc / HWo, r = pc - img * HWo;
        int pix = r;
        if (POOL) { const int oh = r / q.Wo, ow = r - oh * q.Wo; pix = (2 * oh + (t >> 1)) * q.W + 2 * ow + (t & 1); }
        xoff[t] = p < q.total ? img * q.Cw * B * HW + pix : -1;
    }
    // what this lane stores: N tile kq (pool: entries kq, kq + 4, .. of the 2 B (word, plane) pairs of pooled pixel n)
    const int ps = POOL ? pb + n : pb + 16 * kq + n;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HWo;
    uint32_t* const ybase = y + (int64_t)simg * q.OW * B * HWo + (psc - simg * HWo);
    const int sh = 16 * (kq & 1);
    auto loadb = [&](int t, int s, int w0) {
        const int wg = w0 + 2 * s + (kq >> 1);
        uint32_t p[B];
#pragma unroll
        for (int b = 0; b < B; ++b) p[b] = 0u;
        if (xoff[t] >= 0 && wg < q.Cw) {
            const uint32_t* xp = x + xoff[t] + (int64_t)wg * B * HW;
#pragma unroll
            for (int b = 0; b < B; ++b) p[b] = xp[b * HW];
        }
#pragma unroll
        for (int b = 0; b < B; ++b) p[b] = (p[b] >> sh) & 0xffffu;
        return spread16<B>(p);
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
        const int nt = (int)tab[HDR + set];          // wave-uniform
        uint32_t wa[NA][2 * B];          // [word 0 plane 0 .. B - 1, word 1 plane 0 .. B - 1] of the set at the lane's pixels: the bits of this lane's rows
#pragma unroll
        for (int t = 0; t < NA; ++t) {
            wa[t][0] = wa[t][1] = wa[t][2] = wa[t][3] = 0u;          // (spelled out, not a loop over 2 B: the loop form costs the 2-bit instantiations two VGPRs)
            if constexpr (B == 4) wa[t][4] = wa[t][5] = wa[t][6] = wa[t][7] = 0u;
        }
        for (int i = 0; i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            const int w0 = (int)tile[0];
            if (NK && tile[1]) {          // (wave-uniform) a new group: expand its codes once
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
            const i32x4 fl = *reinterpret_cast<const i32x4*>(tile + THDR + 4 * kq);
            if constexpr (B == 2) {
                const i32x4 t1 = *reinterpret_cast<const i32x4*>(tile + THDR + 16 + 4 * kq);
                const i32x4 t2 = *reinterpret_cast<const i32x4*>(tile + THDR + 32 + 4 * kq);
                const i32x4 t3 = *reinterpret_cast<const i32x4*>(tile + THDR + 48 + 4 * kq);
                const u32x4 ds = *reinterpret_cast<const u32x4*>(tile + THDR + 64 + 4 * kq);
                // No multiply by flip and no count of compares: with s = acc ^ ng (ng = 0 / -1 by flip: u = s - ng) and E_k = min(T_k, 40000) - 1 + ng, u >= T_k iff E_k - s < 0.  The row's
                // thresholds are sorted (T_1 <= T_2 <= T_3), so plane 1 = (u >= T_2) and plane 0 = (u >= T_2) ? (u >= T_3) : (u >= T_1); the all-ones / zero lane masks of
                // the two planes are ANDed with the row's bit in word 0 / word 1 of the set.  (|E_k - s| < 2^17: no overflow; the pool's maximum may be taken over s.)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ng = fl[r] >> 31;
                    const int e1 = (t1[r] < 40000 ? t1[r] : 40000) - 1 + ng, e2 = (t2[r] < 40000 ? t2[r] : 40000) - 1 + ng, e3 = (t3[r] < 40000 ? t3[r] : 40000) - 1 + ng;
                    const uint32_t m0 = ds[r] < 32u ? 1u << (ds[r] & 31u) : 0u, m1 = ds[r] < 32u ? 0u : 1u << (ds[r] & 31u);
#pragma unroll
                    for (int t = 0; t < NA; ++t) {
                        int sv;
                        if (POOL) {
                            sv = acc[0][r] ^ ng;
#pragma unroll
                            for (int tt = 1; tt < 4; ++tt) { const int v = acc[tt][r] ^ ng; sv = v > sv ? v : sv; }
                        } else {
                            sv = acc[t][r] ^ ng;
                        }
                        const uint32_t g2 = (uint32_t)((e2 - sv) >> 31);
                        const uint32_t g0 = (uint32_t)((int)((g2 & (uint32_t)(e3 - sv)) | (~g2 & (uint32_t)(e1 - sv))) >> 31);
                        wa[t][0] |= g0 & m0; wa[t][1] |= g2 & m0;
                        wa[t][2] |= g0 & m1; wa[t][3] |= g2 & m1;
                    }
                }
            } else {
                // B > 2: the same with the select deepened to a B-step binary search over the sorted thresholds (code_planes)
                int ngv[4], sv[4][NA];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ngv[r] = fl[r] >> 31;
#pragma unroll
                    for (int t = 0; t < NA; ++t) {
                        if (POOL) {
                            sv[r][t] = acc[0][r] ^ ngv[r];
#pragma unroll
                            for (int tt = 1; tt < 4; ++tt) { const int v = acc[tt][r] ^ ngv[r]; sv[r][t] = v > sv[r][t] ? v : sv[r][t]; }
                        } else {
                            sv[r][t] = acc[t][r] ^ ngv[r];
                        }
                    }
                }
                uint32_t gm[B][4][NA];
                code_planes<B, NA>(tile, kq, ngv, sv, gm);
                const u32x4 ds = *reinterpret_cast<const u32x4*>(tile + THDR + 16 * (nthr(B) + 1) + 4 * kq);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t m0 = ds[r] < 32u ? 1u << (ds[r] & 31u) : 0u, m1 = ds[r] < 32u ? 0u : 1u << (ds[r] & 31u);
#pragma unroll
                    for (int t = 0; t < NA; ++t)
#pragma unroll
                        for (int pl = 0; pl < B; ++pl) {
                            wa[t][pl] |= gm[B - 1 - pl][r][t] & m0;
                            wa[t][B + pl] |= gm[B - 1 - pl][r][t] & m1;
                        }
                }
            }
        }
        // combine the four lane groups (rows 4 kq .. of every tile) by a reduce-scatter: lane group kq ends with the whole words it stores
        const bool hi = (kq & 2) != 0, odd = (kq & 1) != 0;
        if (POOL) {
            // the 2 B entries [word 0 plane 0 .. B - 1, word 1 plane 0 .. B - 1] of the lane's pooled pixel, four at a time: lane group kq ends with entry 4 h + kq,
            // B / 2 whole words per lane group
#pragma unroll
            for (int h = 0; h < B / 2; ++h) {
                const uint32_t v0 = wa[0][4 * h], v1 = wa[0][4 * h + 1], v2 = wa[0][4 * h + 2], v3 = wa[0][4 * h + 3];
                uint32_t ka = hi ? v2 : v0, kb = hi ? v3 : v1;
                ka |= (uint32_t)__shfl_xor((int)(hi ? v0 : v2), 32, 64);
                kb |= (uint32_t)__shfl_xor((int)(hi ? v1 : v3), 32, 64);
                uint32_t val = odd ? kb : ka;
                val |= (uint32_t)__shfl_xor((int)(odd ? ka : kb), 16, 64);
                const int word = 2 * set + (4 * h + kq) / B;
                if (sok && word < q.OW) ybase[(int64_t)(word * B + (4 * h + kq) % B) * HWo] = val;
            }
        } else {
            // lane group kq ends with the words of N tile kq: keep two tiles across xor 32, one across xor 16
#pragma unroll
            for (int c = 0; c < 2 * B; ++c) {
                const uint32_t v[4] = {wa[0][c], wa[1 % NA][c], wa[2 % NA][c], wa[3 % NA][c]};
                uint32_t ka = hi ? v[2] : v[0], kb = hi ? v[3] : v[1];
                ka |= (uint32_t)__shfl_xor((int)(hi ? v[0] : v[2]), 32, 64);
                kb |= (uint32_t)__shfl_xor((int)(hi ? v[1] : v[3]), 32, 64);
                uint32_t val = odd ? kb : ka;
                val |= (uint32_t)__shfl_xor((int)(odd ? ka : kb), 16, 64);
                const int word = 2 * set + (c >> LB);
                if (sok && word < q.OW) ybase[(int64_t)(word * B + (c & (B - 1))) * HWo] = val;
            }
        }
    }
}

template <int B, bool POOL>
static void launch(int nk, dim3 grid, hipStream_t s, const uint32_t* tab, const uint32_t* x, uint32_t* y, const MFwd& f) {
    switch (nk) {
    case 1: hipLaunchKernelGGL((k_codeconv_mfma<B, 1, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    case 2: hipLaunchKernelGGL((k_codeconv_mfma<B, 2, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    case 3: hipLaunchKernelGGL((k_codeconv_mfma<B, 3, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    default: hipLaunchKernelGGL((k_codeconv_mfma<B, 0, POOL>), grid, dim3(256), 0, s, tab, x, y, f); break;
    }
}

}  // namespace mn_codes_mfma

// (passed as an argument of "%s", never as a format)
#define MN_CODEMFMA_COVER "geometry not covered (2-bit codes and weights; 1x1, stride 1, no padding, groups 1 or C / groups % 32 == 0, K * 9 <= 32767)"
#define MN_CODEMFMA_COVER_BITS "geometry or width not covered (codes and weights of 2 or of 4 bits throughout; 1x1, stride 1, no padding, groups 1 or C / groups % 32 == 0, K * n * n <= 32767 with n = 2^bits - 1)"

extern "C" int mn_codeconv_mfma_supported(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_codes_mfma::MGeom m;
    return mn_codes_mfma::make_mgeom(g, a_bits_in, w_bits, a_bits_out, m) ? 1 : 0;
}

extern "C" int64_t mn_codeconv_mfma_table_bytes(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_codes_mfma::MGeom m;
    if (!mn_codes_mfma::make_mgeom(g, a_bits_in, w_bits, a_bits_out, m)) return 0;
    return 4 * mn_codes_mfma::table_words(m);
}

extern "C" int mn_codeconv_mfma_pack(const mn_conv_geom* g, const float* w, const float* chan, int a_bits_in, int w_bits, int a_bits_out, const int32_t* out_order,
                                     uint32_t* table, mn_stream_t stream) {
    mn_codes_mfma::MGeom m;
    if (!w || !chan || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)chan | (uintptr_t)out_order) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_codeconv_mfma_pack: null / unaligned argument (the table is 16-byte aligned) or invalid geometry");
    if (!mn_codes_mfma::make_mgeom(g, a_bits_in, w_bits, a_bits_out, m)) MN_FAIL(MN_ENOTSUP, "mn_codeconv_mfma_pack: %s", MN_CODEMFMA_COVER_BITS);
    if (hipMemsetAsync(table, 0, 4 * mn_codes_mfma::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_codeconv_mfma_pack: header reset failed");          // the two counters
    mn_set_last_kernel("k_codes_mfma_wpack");
    if (m.bits == 4) hipLaunchKernelGGL(mn_codes_mfma::k_codes_mfma_wpack<4>, dim3(m.nsets), dim3(256), 0, (hipStream_t)stream, m, w, chan, out_order, table);
    else hipLaunchKernelGGL(mn_codes_mfma::k_codes_mfma_wpack<2>, dim3(m.nsets), dim3(256), 0, (hipStream_t)stream, m, w, chan, out_order, table);
    MN_CHECK_LAUNCH("mn_codeconv_mfma_pack");
    return MN_OK;
}

// (who: the entry point's name in its messages; cover: what it says it covers)
static int codeconv_mfma_fwd_impl(const char* who, const char* cover, const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out, const uint32_t* table,
                                  const uint32_t* in_planes, uint32_t* out_planes, int pool, mn_stream_t stream) {
    mn_codes_mfma::MGeom m;
    if (!table || !in_planes || !out_planes || !aligned16(table) || ((((uintptr_t)in_planes) | ((uintptr_t)out_planes)) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "%s: null / unaligned argument (the table is 16-byte aligned) or invalid geometry", who);
    if (!mn_codes_mfma::make_mgeom(g, a_bits_in, w_bits, a_bits_out, m)) MN_FAIL(MN_ENOTSUP, "%s: %s", who, cover);
    if (pool < 0 || pool > 1) MN_FAIL(MN_ENOTSUP, "%s: pool must be 0 or 1 (2x2 / stride 2); the 3x3 / stride 2 pool is not folded", who);
    const mn_codes::Geom& q = m.q;
    if (pool && ((q.H & 1) || (q.W & 1))) MN_FAIL(MN_EINVAL, "%s: the folded 2x2 max-pool needs even H and W", who);
    mn_codes_mfma::MFwd f;
    f.Cw = q.Cw; f.H = q.H; f.W = q.W; f.OW = q.OW; f.nsteps = m.nsteps; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride; f.tiles_off = m.tiles_off;
    f.Ho = pool ? q.H / 2 : q.H; f.Wo = pool ? q.W / 2 : q.W;
    f.total = q.N * f.Ho * f.Wo;
    const int ppb = pool ? 64 : 256;          // (pooled) pixels per block: four waves of four N tiles
    const int bx = (f.total + ppb - 1) / ppb;
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const int nk = m.nsteps <= mn_codes_mfma::MAXNK ? m.nsteps : 0;
    mn_set_last_kernel("k_codeconv_mfma<%d>", pool);
    mn_prof_bytes(4.0 * m.bits * q.N * q.Cw * q.H * q.W + 4.0 * m.bits * q.N * q.OW * f.Ho * f.Wo + 4.0 * (double)mn_codes_mfma::table_words(m));
    mn_prof_begin(s);
    if (m.bits == 4) {
        if (pool) mn_codes_mfma::launch<4, true>(nk, grid, s, table, in_planes, out_planes, f);
        else mn_codes_mfma::launch<4, false>(nk, grid, s, table, in_planes, out_planes, f);
    } else {
        if (pool) mn_codes_mfma::launch<2, true>(nk, grid, s, table, in_planes, out_planes, f);
        else mn_codes_mfma::launch<2, false>(nk, grid, s, table, in_planes, out_planes, f);
    }
    mn_prof_end(s);
    MN_CHECK_LAUNCH(who);
    return MN_OK;
}

extern "C" int mn_codeconv_mfma_fwd(const mn_conv_geom* g, const uint32_t* table, const uint32_t* in_planes, uint32_t* out_planes, int pool, mn_stream_t stream) {
    return codeconv_mfma_fwd_impl("mn_codeconv_mfma_fwd", MN_CODEMFMA_COVER, g, mn_codes::A, mn_codes::WB, 2, table, in_planes, out_planes, pool, stream);
}

extern "C" int mn_codeconv_mfma_fwd_bits(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out, const uint32_t* table, const uint32_t* in_planes,
                                         uint32_t* out_planes, int pool, mn_stream_t stream) {
    return codeconv_mfma_fwd_impl("mn_codeconv_mfma_fwd_bits", MN_CODEMFMA_COVER_BITS, g, a_bits_in, w_bits, a_bits_out, table, in_planes, out_planes, pool, stream);
}
#undef MN_CODEMFMA_COVER
#undef MN_CODEMFMA_COVER_BITS
