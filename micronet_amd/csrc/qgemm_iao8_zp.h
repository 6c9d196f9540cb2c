// The int8 deployment of the BN-folded IAO hidden blocks with ZERO POINTS (mn_i8zconv_*, mn_i8z_*): the stage of qgemm_iao8.h where any of its quantizers -- the
// conv's activation quantizer, its weight quantizer, the folded pool's, the consumer's -- is asymmetric.  Included by qgemm_bits.hip behind qgemm_iao8.h, whose
// activation layout, K order in slots, set / tile planner (qgemm_mfma_sets.h), grid rule, LDS image and whole-block stores it shares.
//
//   quantizer    : (s, z, asymmetric, bits).  Code range [lo, hi]: symmetric activation -2^(b-1) .. 2^(b-1) - 1, symmetric weight +-(2^(b-1) - 1), asymmetric activation
//                  0 .. 2^b - 1, asymmetric weight 0 .. 2^b - 2.  code(r; s, z) = clamp(rha(fl(fl(r / s) - z)), lo, hi); the value of a code c is fl(fl(c + z) * s).
//                  The stored BYTE is c - h with h = 0 (symmetric), 2^(b-1) (asymmetric activation), 2^(b-1) - 1 (asymmetric weight): every byte lies in the signed
//                  range of the symmetric form.  e = z + h is an integer and the represented value is (byte + e) * s.
//   contraction  : S[o, pixel] = sum over the in-bounds taps and the group's real channels of (j + e_a)(k + e_w[o]), j an activation byte, k a weight byte.  The MFMA
//                  gives acc = sum j k over ALL taps, an out-of-bounds tap loaded as the padding byte -e_a (the byte of the value 0) broadcast over the 16 channels,
//                  so that S = acc + e_w[o] * B + Kc[o] with
//                    B     = the sum of the bytes j of the lane's pixel over every real slot (the padding slots of the last k-step are skipped by slot index; tail
//                            channels hold the byte 0 by layout), formed from the B operands the lane holds -- four byte-wise dot products with 0x01010101 per 16-byte
//                            operand -- and reduced over the four kq lanes of a pixel once per tile,
//                    Kc[o] = e_a * (sum k[o] + e_w[o] * Cg * taps), formed by the packer.
//                  A padded tap then adds (-e_a + e_a)(k + e_w) = 0.  The packer checks per row Cg * taps * (2^(a-1) + |e_a|) * (2^(w-1) - 1 + |e_w[o]|) <= INT_MAX
//                  (a the width of the input codes): the product expands into the four partial sums, so each of them and S are exact in int32.
//   chain        : y = fl(fl(float(S) * al) + b), al = fl(s_a * s_w[o]), r = max(y, 0), c = code(r; s_out, z_out); with the pool c1 = code(r; s_p, z_p) per sub-pixel,
//                  m = the window's largest c1, v = fl(fl(m + z_p) * s_p), c = code(v; s_out, z_out).  The output byte is c - h_out.  With every z = 0 and every
//                  quantizer symmetric this is the chain of qgemm_iao8.h bit for bit.
//   weight table : (private layout, 16-byte aligned) 32 header words --
//                    [0] rows with a non-finite al or b or a bad s_w, plus each of s_a, s_p, s_out that is non-finite or <= 0
//                    [1] k-steps  [2] tile slots per set  [3] tile stride  [4] sets  [5] chunks  [6] a_bits | w_bits << 8 | in_bits << 16
//                    [7] bad out_order entries + rows with a weight off the grid (|w / s_w - z_w - rint| > 1e-3 or a code outside lo .. hi)
//                    [8] s_p  [9] s_out  [10] lo_out  [11] hi_out  [12] s_a (fp32 bit patterns)
//                    [13] zero points that are not integers of magnitude <= 65535: each of z_a, z_p, z_out, plus the rows with such a z_w
//                    [14] rows beyond the int32 bound  [15] 1: a 3x3 stage whose input quantizer has no code for the value 0 (zero padding has no byte)
//                    [16] z_p  [17] z_out  [18] lo_p  [19] hi_p  [20] h_out (fp32)  [21] e_a (int32)  [22] the padding byte in each of its four bytes
//                    [23] real slots (taps * chunks)  [24] asymmetric flags: input | pool << 1 | consumer << 2 | weight << 3  [25] z_a (fp32)
//                  -- then one word per slot, the tile count of every set and the tiles as in qgemm_iao8.h, a tile's header grown to 96 words:
//                    [0] first 16-channel block of the tile's group, [16 ..) al[16], [32 ..) b[16], [48 ..) dest[16] (-1: a dead row), [64 ..) e_w[16], [80 ..) Kc[16]
//                    (int32), [96 ..) per k-step 64 lanes x 16 bytes in the A-operand order of mn_mfma_i8.
//                  A table with any of the words 0, 7, 13, 14, 15 non-zero must not be used.
// Covered: what mn_i8conv_supported covers (the geometry rule sees no zero point).
// k_i8zconv_wpack and k_i8zconv follow k_i8conv_wpack and k_i8conv of qgemm_iao8.h line for line outside the zero-point terms (the symmetric kernels and their table
// stay as they are, bit for bit and at their speed): a fix to the planner's use, the pixel mapping, the LDS image or the stores of one family belongs in both.
#pragma once
#include "qgemm_iao8.h"

namespace mn_iao8z {

using mn_iao8::IGeom;
using mn_iao8::fin;
using mn_iao8::scale_ok;
using mn_sets::SETROWS;
using mn_sets::table_words;
enum { HDR = 32, THDR = 96, T_AL = 16, T_B = 32, T_DEST = 48, T_EW = 64, T_KC = 80, STEPW = 256 };

// one quantizer as the kernels take it (mn_i8z_quant read on the host)
struct ZQ {
    float s, z;
    int asym, bits;
};

__host__ __device__ static inline int q_lo(int act, int asym, int bits) { return asym ? 0 : act ? -(1 << (bits - 1)) : -((1 << (bits - 1)) - 1); }
__host__ __device__ static inline int q_hi(int act, int asym, int bits) { return asym ? (act ? (1 << bits) - 1 : (1 << bits) - 2) : (1 << (bits - 1)) - 1; }
__host__ __device__ static inline int q_h(int act, int asym, int bits) { return asym ? (act ? 1 << (bits - 1) : (1 << (bits - 1)) - 1) : 0; }
__host__ __device__ static inline bool z_ok(float z) { return fabsf(z) <= 65535.f && z == rintf(z); }          // false for NaN

// the geometry of qgemm_iao8.h with this family's header and tile header
static inline bool make_zgeom(const mn_conv_geom* g, int a_bits, int w_bits, IGeom& m) {
    if (!mn_iao8::make_igeom(g, a_bits, w_bits, m)) return false;
    m.tstride = THDR + STEPW * m.nsteps;
    m.slot_off = HDR;
    m.cnt_off = HDR + 4 * m.nsteps;
    return mn_sets::table_layout(m, m.groups, m.cnt_off);
}

// ---------------------------------------------------------------- weight table: one block per set
__global__ __launch_bounds__(256) void k_i8zconv_wpack(IGeom m, const float* __restrict__ w, const float* __restrict__ sw, const float* __restrict__ zw, int sw_stride,
                                                       const float* __restrict__ bias, ZQ qa, ZQ qp, ZQ qo, int w_asym, const int32_t* __restrict__ order,
                                                       uint32_t* __restrict__ tab) {
    __shared__ mn_sets::SetPlan sp;
    __shared__ int ksum[SETROWS];          // the sum of a row's weight bytes
    const int set = blockIdx.x, tid = threadIdx.x;
    const int h_a = q_h(1, qa.asym, qa.bits);
    const int e_a = (z_ok(qa.z) ? (int)qa.z : 0) + h_a;
    if (set == 0) {
        for (int i = tid; i < 4 * m.nsteps; i += 256) {
            const int tap = i < m.nslots ? i / m.chunks : m.taps / 2, chunk = i < m.nslots ? i - tap * m.chunks : 0;          // a padding slot: the centre tap against zero bytes
            const int dy = m.KS == 3 ? tap / 3 : 1, dx = m.KS == 3 ? tap % 3 : 1;
            tab[m.slot_off + i] = (uint32_t)(dy | (dx << 2) | (chunk << 4));
        }
        if (tid == 0) {
            tab[1] = (uint32_t)m.nsteps; tab[2] = (uint32_t)m.slots; tab[3] = (uint32_t)m.tstride; tab[4] = (uint32_t)m.nsets; tab[5] = (uint32_t)m.chunks;
            tab[6] = (uint32_t)(m.a_bits | (m.w_bits << 8) | (qa.bits << 16));
            tab[8] = mn_f2u(qp.s); tab[9] = mn_f2u(qo.s);
            tab[10] = mn_f2u((float)q_lo(1, qo.asym, qo.bits)); tab[11] = mn_f2u((float)q_hi(1, qo.asym, qo.bits));
            tab[12] = mn_f2u(qa.s);
            tab[16] = mn_f2u(qp.z); tab[17] = mn_f2u(qo.z);
            tab[18] = mn_f2u((float)q_lo(1, qp.asym, qp.bits)); tab[19] = mn_f2u((float)q_hi(1, qp.asym, qp.bits));
            tab[20] = mn_f2u((float)q_h(1, qo.asym, qo.bits));
            tab[21] = (uint32_t)e_a;
            // the byte of the value 0 under the input quantizer: the code -z_a, stored as -z_a - h_a = -e_a (a 1x1 stage has no padding and never loads it)
            const bool has0 = z_ok(qa.z) && -qa.z >= (float)q_lo(1, qa.asym, qa.bits) && -qa.z <= (float)q_hi(1, qa.asym, qa.bits);
            const uint32_t pb = (m.KS == 3 && has0) ? ((uint32_t)(-e_a) & 0xffu) : 0u;
            tab[22] = pb * 0x01010101u;
            tab[23] = (uint32_t)m.nslots;
            tab[24] = (uint32_t)((qa.asym ? 1 : 0) | (qp.asym ? 2 : 0) | (qo.asym ? 4 : 0) | (w_asym ? 8 : 0));
            tab[25] = mn_f2u(qa.z);
            const uint32_t nbad = (uint32_t)!scale_ok(qa.s) + (uint32_t)!scale_ok(qp.s) + (uint32_t)!scale_ok(qo.s);
            if (nbad) atomicAdd(tab + 0, nbad);
            const uint32_t zbad = (uint32_t)!z_ok(qa.z) + (uint32_t)!z_ok(qp.z) + (uint32_t)!z_ok(qo.z);
            if (zbad) atomicAdd(tab + 13, zbad);
            if (m.KS == 3 && z_ok(qa.z) && !has0) atomicAdd(tab + 15, 1u);
        }
    }
    uint32_t* tiles = tab + m.tiles_off + (int64_t)set * m.slots * m.tstride;
    // every slot starts as a tile of dead rows: zero weight bytes, al = b = 0, e_w = Kc = 0, no destination
    for (int i = tid; i < m.slots * m.tstride; i += 256) {
        const int r = i % m.tstride;
        tiles[i] = (r >= T_DEST && r < T_DEST + 16) ? 0xffffffffu : 0u;
    }
    if (tid < SETROWS) ksum[tid] = 0;
    int nt;
    mn_sets::plan_set(order, m.O, m.Og, set, tab + 7, sp, nt);
    if (tid == 0) tab[m.cnt_off + set] = (uint32_t)nt;
    // weight codes cw = rint(w / s_w - z_w), stored as the byte cw - h_w: thread = 4 consecutive channels of one row at one tap, one dword of the A operand
    const int dpr = m.nslots * 4;          // dwords per row
    const int h_w = q_h(0, w_asym, m.w_bits);
    const float wlo = (float)q_lo(0, w_asym, m.w_bits), whi = (float)q_hi(0, w_asym, m.w_bits);
    for (int idx = tid; idx < SETROWS * dpr; idx += 256) {
        const int pos = idx / dpr, d = idx - pos * dpr, slot = d >> 2, e4 = d & 3;
        const int o = sp.chan[pos];
        if (o < 0) continue;
        const int tap = slot / m.chunks, c0 = (slot - tap * m.chunks) * 16 + e4 * 4;
        if (c0 >= m.Cg) continue;
        const float* wr = w + ((int64_t)o * m.Cg + c0) * m.taps + tap;          // [O][Cg][taps]
        const float s = sw[(int64_t)o * sw_stride];
        const float z = zw ? zw[(int64_t)o * sw_stride] : 0.f;
        uint32_t v = 0u;
        int off = 0, ks = 0;
        for (int e = 0; e < 4 && c0 + e < m.Cg; ++e) {
            const float kf = wr[e * m.taps] / s - z;
            const float kr = rintf(kf);
            if (!(fabsf(kf - kr) <= 1e-3f) || !(kr >= wlo && kr <= whi)) off = 1;
            const int kc = (int)(kr < wlo ? wlo : kr > whi ? whi : kr == kr ? kr : wlo) - h_w;
            ks += kc;
            v |= ((uint32_t)kc & 0xffu) << (8 * e);
        }
        if (off) sp.off[pos] = 1;
        atomicAdd(&ksum[pos], ks);
        uint32_t* A = tiles + (int64_t)sp.tile[pos] * m.tstride + THDR;
        A[(slot >> 2) * STEPW + ((slot & 3) * 16 + sp.row[pos]) * 4 + e4] = v;
    }
    __syncthreads();          // the byte sums of the rows are complete
    // the row constants
    if (tid < SETROWS && sp.chan[tid] >= 0) {
        const int o = sp.chan[tid], r = sp.row[tid];
        uint32_t* T = tiles + (int64_t)sp.tile[tid] * m.tstride;
        const float s = sw[(int64_t)o * sw_stride];
        const float z = zw ? zw[(int64_t)o * sw_stride] : 0.f;
        const float al = qa.s * s, b = bias ? bias[o] : 0.f;
        const int e_w = (z_ok(z) ? (int)z : 0) + h_w;
        const int64_t K = (int64_t)m.Cg * m.taps;
        const double bound = (double)K * (double)((1 << (qa.bits - 1)) + (e_a < 0 ? -e_a : e_a)) * (double)(((1 << (m.w_bits - 1)) - 1) + (e_w < 0 ? -e_w : e_w));
        const bool fits = bound <= 2147483647.0;
        const int64_t kc = fits ? (int64_t)e_a * ((int64_t)ksum[tid] + (int64_t)e_w * K) : 0;
        T[T_AL + r] = mn_f2u(al); T[T_B + r] = mn_f2u(b); T[T_DEST + r] = (uint32_t)tid;
        T[T_EW + r] = (uint32_t)e_w; T[T_KC + r] = (uint32_t)(int32_t)kc;
        if (!fin(al) || !fin(b) || !scale_ok(s)) atomicAdd(tab + 0, 1u);
        if (!z_ok(z)) atomicAdd(tab + 13, 1u);
        if (!fits) atomicAdd(tab + 14, 1u);
        if (r == 0) T[0] = (uint32_t)(sp.grp[tid] * m.Cg >> 4);          // (groups == 1 with any C: group 0 starts at block 0)
    }
    mn_sets::tally_off(sp, tab + 7);
}

// ---------------------------------------------------------------- MFMA contraction + box sum + the requantisation chain -> output bytes
struct ZFwd {
    int total, CB, OB, H, W, Ho, Wo, nsteps, nslots, nsets, slots, tstride, slot_off, cnt_off, tiles_off, spb;
};

// clamp(rha(fl(fl(r / s) - z)), lo, hi) of a finite r
__device__ __forceinline__ float zcode_of(float r, float s, float z, float lo, float hi) { return fminf(fmaxf(mn_rha(r / s - z), lo), hi); }

// the sum of the 16 signed bytes of a B operand
__device__ __forceinline__ int byte_sum16(const u32x4& v) {
    int s = 0;
#ifdef MN_EMULATION
    for (int i = 0; i < 4; ++i)
        for (int e = 0; e < 4; ++e) s += (int)(int8_t)(v[i] >> (8 * e));
#else
#pragma unroll
    for (int i = 0; i < 4; ++i) s = __builtin_amdgcn_sdot4((int)v[i], 0x01010101, s, false);
#endif
    return s;
}

template <int KS, bool POOL>
__global__ __launch_bounds__(256) void k_i8zconv(const uint32_t* __restrict__ tab, const u32x4* __restrict__ x, u32x4* __restrict__ y, ZFwd q) {
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
        const int img = pc / HWo, r = pc - img * HWo;
        int h = r / q.Wo, wc = r - h * q.Wo;
        if (POOL) { h = 2 * h + (t >> 1); wc = 2 * wc + (t & 1); }
        ph[t] = p < q.total ? h : -4; pw[t] = wc;
        xoff[t] = img * q.CB * HW + h * q.W + wc;
    }
    // what this lane stores: the blocks of pixel pb + lane (pool: block kq of the set at pooled pixel pb + n)
    const int ps = POOL ? pb + n : pb + lane;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HWo;
    u32x4* const ybase = y + (int64_t)simg * q.OB * HWo + (psc - simg * HWo);
    u32x4* const img = s_img[wave];
    int8_t* const imgb = reinterpret_cast<int8_t*>(img);
    const float s_p = mn_u2f(tab[8]), s_out = mn_u2f(tab[9]), lo = mn_u2f(tab[10]), hi = mn_u2f(tab[11]);
    const float z_p = mn_u2f(tab[16]), z_out = mn_u2f(tab[17]), lo_p = mn_u2f(tab[18]), hi_p = mn_u2f(tab[19]), h_out = mn_u2f(tab[20]);
    const uint32_t pw4 = tab[22];
    const u32x4 padv = u32x4{pw4, pw4, pw4, pw4};          // an out-of-bounds tap: the byte of the value 0 on all 16 channels
    for (int i = lane; i < 4 * NPIX; i += 64) img[i] = u32x4{0u, 0u, 0u, 0u};
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        __syncthreads();          // the image is zero before any lane writes into it
        const int nt = (int)tab[q.cnt_off + set] < q.slots ? (int)tab[q.cnt_off + set] : q.slots;          // wave-uniform
        for (int i = 0; i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            const int cb0 = (int)tile[0];
            i32x4 acc[4];
            int bs[4];          // the lane's share of the box sum of N tile t: the bytes of its slots
#pragma unroll
            for (int t = 0; t < 4; ++t) { acc[t] = i32x4{0, 0, 0, 0}; bs[t] = 0; }
            const uint32_t* ap = tile + THDR + lane * 4;
#pragma unroll 1
            for (int s = 0; s < q.nsteps; ++s) {
                const uint32_t sl = tab[q.slot_off + 4 * s + kq];
                const int dy = KS == 3 ? (int)(sl & 3u) - 1 : 0, dx = KS == 3 ? (int)((sl >> 2) & 3u) - 1 : 0, cb = cb0 + (int)(sl >> 4);
                const int boff = cb * HW + dy * q.W + dx;
                const u32x4 a = *reinterpret_cast<const u32x4*>(ap + s * STEPW);
                const bool real = 4 * s + kq < q.nslots;          // (a padding slot reads real bytes against zero weights: they must not enter the box sum)
                u32x4 b[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    b[t] = KS == 3 ? padv : u32x4{0u, 0u, 0u, 0u};
                    if ((unsigned)(ph[t] + dy) < (unsigned)q.H && (unsigned)(pw[t] + dx) < (unsigned)q.W && cb < q.CB) b[t] = x[xoff[t] + boff];
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    acc[t] = mn_mfma_i8(a, b[t], acc[t]);
                    if (real) bs[t] += byte_sum16(b[t]);
                }
            }
            // the four kq lanes of a pixel hold the four slots of every k-step: their sum is the pixel's box sum, in all four
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                bs[t] += __shfl_xor(bs[t], 16, 64);
                bs[t] += __shfl_xor(bs[t], 32, 64);
            }
            // the lane's rows 4 kq .. 4 kq + 3 of the tile (D[row = 4 kq + reg][col = n])
            const f32x4 al = *reinterpret_cast<const f32x4*>(tile + T_AL + 4 * kq);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(tile + T_B + 4 * kq);
            const i32x4 ds = *reinterpret_cast<const i32x4*>(tile + T_DEST + 4 * kq);
            const i32x4 ew = *reinterpret_cast<const i32x4*>(tile + T_EW + 4 * kq);
            const i32x4 kc = *reinterpret_cast<const i32x4*>(tile + T_KC + 4 * kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (ds[r] < 0 || ds[r] >= SETROWS) continue;          // a dead row
                int8_t* const dst = imgb + ((ds[r] >> 4) * NPIX + n) * 16 + (ds[r] & 15);
                if (POOL) {
                    float mx = lo_p;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int S = acc[t][r] + ew[r] * bs[t] + kc[r];
                        const float yv = (float)S * al[r] + bb[r];
                        mx = fmaxf(mx, zcode_of(fmaxf(yv, 0.f), s_p, z_p, lo_p, hi_p));
                    }
                    dst[0] = (int8_t)(int)(zcode_of((mx + z_p) * s_p, s_out, z_out, lo, hi) - h_out);
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int S = acc[t][r] + ew[r] * bs[t] + kc[r];
                        const float yv = (float)S * al[r] + bb[r];
                        dst[256 * t] = (int8_t)(int)(zcode_of(fmaxf(yv, 0.f), s_out, z_out, lo, hi) - h_out);
                    }
                }
            }
        }
        __syncthreads();          // every byte of the set is in the image
        if (POOL) {
            const u32x4 v = img[kq * NPIX + n];
            img[kq * NPIX + n] = u32x4{0u, 0u, 0u, 0u};
            const int ob = 4 * set + kq;
            if (sok && ob < q.OB) ybase[(int64_t)ob * HWo] = v;
        } else {
#pragma unroll
            for (int bk = 0; bk < 4; ++bk) {
                const u32x4 v = img[bk * NPIX + lane];
                img[bk * NPIX + lane] = u32x4{0u, 0u, 0u, 0u};
                const int ob = 4 * set + bk;
                if (sok && ob < q.OB) ybase[(int64_t)ob * HWo] = v;
            }
        }
    }
}

// ---------------------------------------------------------------- fp32 NCHW <-> blocked bytes
// k_i8_pack with a zero point: the byte code(x; s, z) - h of the consumer's quantizer; tail channels and bad entries stay the byte 0 (they must add nothing to a box sum)
__global__ __launch_bounds__(256) void k_i8z_pack(const float* __restrict__ x, u32x4* __restrict__ out, int64_t total, int C, int CB, int HW, float s, float z, float lo,
                                                  float hi, float h, const int32_t* __restrict__ order) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int pix = (int)(i % HW);
    const int64_t t = i / HW;
    const int cb = (int)(t % CB);
    const int64_t nimg = t / CB;
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        const int j = cb * 16 + d;
        int c = j < C ? (order ? order[j] : j) : -1;
        c = (c >= 0 && c < C) ? c : -1;
        if (c < 0) continue;
        const float xv = x[(nimg * C + c) * HW + pix];
        const float cf = mn_clamp(mn_rha(xv / s - z), lo, hi) - h;
        const int ci = cf == cf ? (int)cf : 0;
        v[d >> 2] |= ((uint32_t)ci & 0xffu) << (8 * (d & 3));
    }
    out[i] = v;
}

// one thread = one element of the fp32 NCHW tensor: fl(fl(c + z) * s) with c = byte + h
__global__ __launch_bounds__(256) void k_i8z_unpack(const int8_t* __restrict__ in, float* __restrict__ y, int64_t total, int C, int CB, int HW, float s, float z, float h) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int pix = (int)(i % HW);
    const int64_t t = i / HW;
    const int c = (int)(t % C);
    const int64_t nimg = t / C;
    const float code = (float)in[((nimg * CB + (c >> 4)) * HW + pix) * 16 + (c & 15)] + h;
    y[i] = (code + z) * s;
}

static inline bool quant_valid(const mn_i8z_quant* q) { return q && q->bits >= 2 && q->bits <= 8 && (q->asym == 0 || q->asym == 1); }
static inline ZQ zq_of(const mn_i8z_quant* q) { return ZQ{q->s, q->z, q->asym, q->bits}; }

}  // namespace mn_iao8z

// (passed as an argument of "%s", never as a format)
#define MN_I8ZCONV_COVER "geometry or width not covered (code widths 2 .. 8; 1x1 / stride 1 / padding 0 with groups 1 or C / groups % 16 == 0, or 3x3 / stride 1 / padding 1 with C / groups % 16 == 0)"

extern "C" int mn_i8zconv_supported(const mn_conv_geom* g, int a_bits, int w_bits) {
    mn_iao8::IGeom m;
    return mn_iao8z::make_zgeom(g, a_bits, w_bits, m) ? 1 : 0;
}

extern "C" int64_t mn_i8zconv_table_bytes(const mn_conv_geom* g, int a_bits, int w_bits) {
    mn_iao8::IGeom m;
    if (!mn_iao8z::make_zgeom(g, a_bits, w_bits, m)) return 0;
    return 4 * mn_iao8z::table_words(m);
}

extern "C" int mn_i8zconv_pack(const mn_conv_geom* g, const float* w, const float* s_w, const float* z_w, int s_w_stride, const float* bias, const mn_i8z_quant* q_a,
                               const mn_i8z_quant* q_p, const mn_i8z_quant* q_out, int w_asym, int w_bits, const int32_t* out_order, uint32_t* table, mn_stream_t stream) {
    mn_iao8::IGeom m;
    if (!w || !s_w || !table || !q_a || !q_p || !q_out || !aligned16(table) ||
        (((uintptr_t)w | (uintptr_t)s_w | (uintptr_t)z_w | (uintptr_t)bias | (uintptr_t)out_order) & 3) || s_w_stride < 0 || s_w_stride > 1 || w_asym < 0 || w_asym > 1 ||
        q_a->asym < 0 || q_a->asym > 1 || q_p->asym < 0 || q_p->asym > 1 || q_out->asym < 0 || q_out->asym > 1 || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_i8zconv_pack: null / unaligned argument (the table is 16-byte aligned), s_w_stride or an asymmetric flag outside 0 / 1 or invalid geometry");
    if (!mn_iao8z::quant_valid(q_a) || !mn_iao8z::quant_valid(q_p) || !mn_iao8z::quant_valid(q_out) || q_p->bits != q_out->bits ||
        !mn_iao8z::make_zgeom(g, q_out->bits, w_bits, m))
        MN_FAIL(MN_ENOTSUP, "mn_i8zconv_pack: %s, or a pool quantizer of another width than the consumer's", MN_I8ZCONV_COVER);
    if (hipMemsetAsync(table, 0, 4 * mn_iao8z::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_i8zconv_pack: header reset failed");          // the counters
    mn_set_last_kernel("k_i8zconv_wpack");
    hipLaunchKernelGGL(mn_iao8z::k_i8zconv_wpack, dim3(m.nsets), dim3(256), 0, (hipStream_t)stream, m, w, s_w, z_w, s_w_stride, bias, mn_iao8z::zq_of(q_a),
                       mn_iao8z::zq_of(q_p), mn_iao8z::zq_of(q_out), w_asym, out_order, table);
    MN_CHECK_LAUNCH("mn_i8zconv_pack");
    return MN_OK;
}

extern "C" int mn_i8zconv_fwd(const mn_conv_geom* g, int a_bits, int w_bits, const uint32_t* table, const int8_t* in_codes, int8_t* out_codes, int pool, mn_stream_t stream) {
    mn_iao8::IGeom m;
    if (!table || !in_codes || !out_codes || !aligned16(table) || !aligned16(in_codes) || !aligned16(out_codes) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_i8zconv_fwd: null / unaligned argument (table and codes are 16-byte aligned) or invalid geometry");
    if (!mn_iao8z::make_zgeom(g, a_bits, w_bits, m)) MN_FAIL(MN_ENOTSUP, "mn_i8zconv_fwd: %s", MN_I8ZCONV_COVER);
    if (pool < 0 || pool > 1) MN_FAIL(MN_ENOTSUP, "mn_i8zconv_fwd: pool must be 0 or 1 (2x2 / stride 2)");
    if (pool && ((m.H & 1) || (m.W & 1))) MN_FAIL(MN_EINVAL, "mn_i8zconv_fwd: the folded 2x2 max-pool needs even H and W");
    mn_iao8z::ZFwd f;
    f.CB = m.CB; f.OB = m.OB; f.H = m.H; f.W = m.W; f.nsteps = m.nsteps; f.nslots = m.nslots; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride;
    f.slot_off = m.slot_off; f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off;
    f.Ho = pool ? m.H / 2 : m.H; f.Wo = pool ? m.W / 2 : m.W;
    f.total = m.N * f.Ho * f.Wo;
    const int ppb = pool ? 64 : 256;          // (pooled) pixels per block: four waves of four N tiles
    const int bx = (f.total + ppb - 1) / ppb;
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const u32x4* xin = reinterpret_cast<const u32x4*>(in_codes);
    u32x4* yout = reinterpret_cast<u32x4*>(out_codes);
    mn_set_last_kernel("k_i8zconv<%d,%d>", m.KS, pool);
    mn_prof_bytes(16.0 * m.N * m.CB * m.H * m.W + 16.0 * m.N * m.OB * f.Ho * f.Wo + 4.0 * (double)mn_iao8z::table_words(m));
    mn_prof_begin(s);
    if (m.KS == 3) {
        if (pool) hipLaunchKernelGGL((mn_iao8z::k_i8zconv<3, true>), grid, dim3(256), 0, s, table, xin, yout, f);
        else hipLaunchKernelGGL((mn_iao8z::k_i8zconv<3, false>), grid, dim3(256), 0, s, table, xin, yout, f);
    } else {
        if (pool) hipLaunchKernelGGL((mn_iao8z::k_i8zconv<1, true>), grid, dim3(256), 0, s, table, xin, yout, f);
        else hipLaunchKernelGGL((mn_iao8z::k_i8zconv<1, false>), grid, dim3(256), 0, s, table, xin, yout, f);
    }
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_i8zconv_fwd");
    return MN_OK;
}
#undef MN_I8ZCONV_COVER

static int i8z_codes_args(const char* who, const void* a, const void* b, int64_t N, int64_t C, int64_t HW, const mn_i8z_quant* q) {
    if (!a || !b || !q || N <= 0 || C <= 0 || HW <= 0 || !mn_iao8::scale_ok(q->s) || !mn_iao8z::z_ok(q->z) || q->asym < 0 || q->asym > 1)
        MN_FAIL(MN_EINVAL, "%s: null / empty argument, a scale that is not finite and positive, a zero point that is not an integer of magnitude <= 65535 or an asymmetric flag outside 0 / 1", who);
    if (q->bits < 2 || q->bits > 8) MN_FAIL(MN_ENOTSUP, "%s: code widths 2 .. 8", who);
    if (N * ((C + 15) / 16) * HW >= (1ll << 27)) MN_FAIL(MN_ENOTSUP, "%s: tensor too large", who);
    return MN_OK;
}

extern "C" int mn_i8z_pack_codes(const float* x, int64_t N, int64_t C, int64_t HW, const mn_i8z_quant* q, const int32_t* out_order, int8_t* codes, mn_stream_t stream) {
    if ((((uintptr_t)x | (uintptr_t)out_order) & 3) || !aligned16(codes)) MN_FAIL(MN_EINVAL, "mn_i8z_pack_codes: unaligned argument (x 4-byte, codes 16-byte aligned)");
    const int rc = i8z_codes_args("mn_i8z_pack_codes", x, codes, N, C, HW, q);
    if (rc != MN_OK) return rc;
    const int CB = (int)((C + 15) / 16);
    const int64_t total = N * CB * HW;
    mn_set_last_kernel("k_i8z_pack");
    mn_prof_bytes(4.0 * N * C * HW + 16.0 * (double)total);
    mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_iao8z::k_i8z_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, reinterpret_cast<u32x4*>(codes), total, (int)C, CB,
                       (int)HW, q->s, q->z, (float)mn_iao8z::q_lo(1, q->asym, q->bits), (float)mn_iao8z::q_hi(1, q->asym, q->bits), (float)mn_iao8z::q_h(1, q->asym, q->bits),
                       out_order);
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_i8z_pack_codes");
    return MN_OK;
}

extern "C" int mn_i8z_unpack_codes(const int8_t* codes, int64_t N, int64_t C, int64_t HW, const mn_i8z_quant* q, float* y, mn_stream_t stream) {
    if ((((uintptr_t)y) & 3) || !aligned16(codes)) MN_FAIL(MN_EINVAL, "mn_i8z_unpack_codes: unaligned argument (y 4-byte, codes 16-byte aligned)");
    const int rc = i8z_codes_args("mn_i8z_unpack_codes", codes, y, N, C, HW, q);
    if (rc != MN_OK) return rc;
    const int CB = (int)((C + 15) / 16);
    const int64_t total = N * C * HW;
    mn_set_last_kernel("k_i8z_unpack");
    mn_prof_bytes(16.0 * N * CB * HW + 4.0 * (double)total);
    mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_iao8z::k_i8z_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codes, y, total, (int)C, CB, (int)HW, q->s, q->z,
                       (float)mn_iao8z::q_h(1, q->asym, q->bits));
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_i8z_unpack_codes");
    return MN_OK;
}
