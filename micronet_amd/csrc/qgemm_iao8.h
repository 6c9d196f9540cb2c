// The int8 deployment of the BN-folded IAO hidden blocks (mn_i8conv_*, mn_i8_*): byte codes in, byte codes out, one kernel per hidden stage
//   [channel shuffle] -> QuantConv2d (folded, stored weights on the grid) -> ReLU -> [QuantMaxPool2d 2x2 / 2] -> the next conv's activation quantizer,
// every quantizer symmetric (zero point 0).  Included by qgemm_bits.hip behind the bit and code headers (whose route into both builds it shares).
//
//   activations  : int8 [N][ceil(C/16)][H*W][16]; byte d of the 16-byte block cb at a pixel is the code of channel 16 cb + d, tail channels 0.  One 16-byte load per
//                  lane is the B operand of mn_mfma_i8 for 16 channels of one pixel, coalesced over the 16 pixel lanes; a 3x3 tap of a 16-channel chunk is the same
//                  load at a shifted pixel, or zeros outside the map (a zero byte is the value 0: zero padding needs no mask).
//   contraction  : v_mfma_i32_16x16x64_i8 as an implicit GEMM over (tap, channel).  A = weight codes k = rint(w / s_w) as signed bytes (M = 16 output rows of ONE
//                  group), B = activation codes j (N = 16 pixels), acc = sum j k exact in int32.  The K order is tap-major in SLOTS of 16 channels, slot = tap *
//                  chunks + chunk (chunks = ceil(C / groups / 16)), four slots per k-step, padded to a multiple of four with zero weight bytes; a padding slot
//                  reads the centre tap of chunk 0 against zero bytes.  A 1x1 block is the one-tap case.
//   chain        : y = fl(fl(float(acc) * al) + b), r = max(y, 0), c = clamp(rha(fl(r / s_out)), qmin, qmax); with the pool c1 = clamp(rha(fl(r / s_p))) per sub-pixel,
//                  m = the window's largest c1, v = fl(float(m) * s_p), c = clamp(rha(fl(v / s_out))) -- codes first, then the maximum, as the modules do it.  `/`
//                  is the IEEE quotient; al = fl(s_a * s_w) is formed once by the packer.
//   weight table : (private layout, 16-byte aligned: the set / tile table of qgemm_mfma_sets.h, a set = four 16-byte output blocks) 16 header words -- [0] rows
//                  with a non-finite al or b or a bad s_w, plus each of s_a, s_p, s_out that is non-finite or <= 0, [1] k-steps, [2] tile slots per set, [3] tile
//                  stride, [4] sets, [5] chunks, [6] a_bits | w_bits << 8, [7] bad out_order entries + rows with a weight off the grid, [8] s_p, [9] s_out,
//                  [10] qmin, [11] qmax, [12] s_a (fp32 bit patterns) -- then one word per slot (dy + 1 | (dx + 1) << 2 | chunk << 4), then the tile count of every
//                  set, then the tiles:
//                    [0] first 16-channel block of the tile's group, [16 ..) al[16], [32 ..) b[16], [48 ..) dest[16] (position in the set, -1: a dead row),
//                    [64 ..) per k-step 64 lanes x 16 bytes in the A-operand order of mn_mfma_i8 (lane = 16 kq + row).
//                  A dead row: zero weights, no destination.  The bytes of positions without a row are 0.
//   kernel       : a wave owns 64 pixels as four N tiles (pool: the four sub-pixels of the 2x2 windows of 16 pooled pixels, so the window's maximum is taken
//                  inside a lane).  Every lane writes the code bytes of its four rows into the wave's LDS image [4 blocks][pixels][16 bytes] (zero where no row
//                  writes); behind a barrier every 16-byte block is read back and stored once, whole, coalesced along pixels: no atomics and no read-modify-write
//                  on global memory.
// Covered: code widths 2 .. 8; 1x1 / stride 1 / padding 0 with groups == 1 and any C, or C / groups % 16 == 0; 3x3 / stride 1 / padding 1 with C / groups % 16 == 0;
// any O; pool 0 / 1 (even H and W).
#pragma once
#include "qgemm_codes.h"
#include "qgemm_mfma_sets.h"

namespace mn_iao8 {

using mn_sets::SETROWS;
using mn_sets::table_words;
enum { HDR = 16, THDR = 64, T_AL = 16, T_B = 32, T_DEST = 48, STEPW = 256 };

struct IGeom {
    int N, C, H, W, O, KS, groups, Cg, Og, taps;
    int CB, OB;                                   // 16-channel blocks of the input / output layout
    int chunks, nslots, nsteps, nsets, slots, tstride, slot_off, cnt_off, tiles_off;
    int a_bits, w_bits;
};

static inline bool make_igeom(const mn_conv_geom* g, int a_bits, int w_bits, IGeom& m) {
    if (!g || g->N <= 0 || g->C <= 0 || g->H <= 0 || g->W <= 0 || g->O <= 0 || g->groups <= 0) return false;
    if (a_bits < 2 || a_bits > 8 || w_bits < 2 || w_bits > 8) return false;
    if (g->KH != g->KW || (g->KH != 1 && g->KH != 3)) return false;
    const int pad = (g->KH - 1) / 2;
    if (g->stride_h != 1 || g->stride_w != 1 || g->dil_h != 1 || g->dil_w != 1 || g->pad_h != pad || g->pad_w != pad) return false;
    if (g->C % g->groups || g->O % g->groups || g->in_shuffle > 1) return false;      // a channel shuffle is folded into the PRODUCER's row order, never gathered here
    m.N = g->N; m.C = g->C; m.H = g->H; m.W = g->W; m.O = g->O; m.KS = g->KH; m.groups = g->groups;
    m.Cg = g->C / g->groups; m.Og = g->O / g->groups; m.taps = g->KH * g->KW;
    if ((m.Cg & 15) && (m.KS != 1 || m.groups != 1)) return false;          // every group starts on a 16-channel block
    m.a_bits = a_bits; m.w_bits = w_bits;
    if ((int64_t)m.Cg * m.taps * (1 << (a_bits - 1)) * ((1 << (w_bits - 1)) - 1) > (int64_t)INT_MAX) return false;          // acc is exact in int32
    m.CB = (g->C + 15) >> 4; m.OB = (g->O + 15) >> 4;
    m.chunks = (m.Cg + 15) >> 4;
    m.nslots = m.taps * m.chunks;
    m.nsteps = (m.nslots + 3) >> 2;
    m.nsets = (m.OB + 3) >> 2;
    m.tstride = THDR + STEPW * m.nsteps;
    m.slot_off = HDR;
    m.cnt_off = HDR + 4 * m.nsteps;
    if (!mn_sets::table_layout(m, m.groups, m.cnt_off)) return false;
    const int64_t blocks = (int64_t)g->N * (m.CB > m.OB ? m.CB : m.OB) * g->H * g->W;          // 16-byte blocks: indexed in int
    if (blocks >= (1ll << 27)) return false;
    return true;
}

__host__ __device__ static inline bool fin(float v) { return fabsf(v) <= 3.402823466e38f; }          // false for NaN
__host__ __device__ static inline bool scale_ok(float s) { return fin(s) && s > 0.f; }

// ---------------------------------------------------------------- weight table: one block per set
__global__ __launch_bounds__(256) void k_i8conv_wpack(IGeom m, const float* __restrict__ w, const float* __restrict__ sw, int sw_stride, const float* __restrict__ bias,
                                                      float s_a, float s_p, float s_out, const int32_t* __restrict__ order, uint32_t* __restrict__ tab) {
    __shared__ mn_sets::SetPlan sp;
    const int set = blockIdx.x, tid = threadIdx.x;
    if (set == 0) {
        for (int i = tid; i < 4 * m.nsteps; i += 256) {
            const int tap = i < m.nslots ? i / m.chunks : m.taps / 2, chunk = i < m.nslots ? i - tap * m.chunks : 0;          // a padding slot: the centre tap against zero bytes
            const int dy = m.KS == 3 ? tap / 3 : 1, dx = m.KS == 3 ? tap % 3 : 1;
            tab[m.slot_off + i] = (uint32_t)(dy | (dx << 2) | (chunk << 4));
        }
        if (tid == 0) {
            tab[1] = (uint32_t)m.nsteps; tab[2] = (uint32_t)m.slots; tab[3] = (uint32_t)m.tstride; tab[4] = (uint32_t)m.nsets; tab[5] = (uint32_t)m.chunks;
            tab[6] = (uint32_t)(m.a_bits | (m.w_bits << 8));
            tab[8] = mn_f2u(s_p); tab[9] = mn_f2u(s_out);
            tab[10] = mn_f2u(-(float)(1 << (m.a_bits - 1))); tab[11] = mn_f2u((float)((1 << (m.a_bits - 1)) - 1));
            tab[12] = mn_f2u(s_a);
            const uint32_t nbad = (uint32_t)!scale_ok(s_a) + (uint32_t)!scale_ok(s_p) + (uint32_t)!scale_ok(s_out);
            if (nbad) atomicAdd(tab + 0, nbad);
        }
    }
    uint32_t* tiles = tab + m.tiles_off + (int64_t)set * m.slots * m.tstride;
    // every slot starts as a tile of dead rows: zero weight bytes, al = b = 0, no destination
    for (int i = tid; i < m.slots * m.tstride; i += 256) {
        const int r = i % m.tstride;
        tiles[i] = (r >= T_DEST && r < T_DEST + 16) ? 0xffffffffu : 0u;
    }
    int nt;
    mn_sets::plan_set(order, m.O, m.Og, set, tab + 7, sp, nt);
    if (tid == 0) tab[m.cnt_off + set] = (uint32_t)nt;
    // weight codes k = rint(w / s_w): thread = 4 consecutive channels of one row at one tap, one dword of the A operand (lane 16 (slot & 3) + row of k-step slot >> 2)
    const int dpr = m.nslots * 4;          // dwords per row
    const float kmax = (float)((1 << (m.w_bits - 1)) - 1);
    for (int idx = tid; idx < SETROWS * dpr; idx += 256) {
        const int pos = idx / dpr, d = idx - pos * dpr, slot = d >> 2, e4 = d & 3;
        const int o = sp.chan[pos];
        if (o < 0) continue;
        const int tap = slot / m.chunks, c0 = (slot - tap * m.chunks) * 16 + e4 * 4;
        if (c0 >= m.Cg) continue;
        const float* wr = w + ((int64_t)o * m.Cg + c0) * m.taps + tap;          // [O][Cg][taps]
        const float s = sw[(int64_t)o * sw_stride];
        uint32_t v = 0u;
        int off = 0;
        for (int e = 0; e < 4 && c0 + e < m.Cg; ++e) {
            const float kf = wr[e * m.taps] / s;
            const float kr = rintf(kf);
            if (!(fabsf(kf - kr) <= 1e-3f) || !(fabsf(kr) <= kmax)) off = 1;
            const int kc = (int)(kr < -kmax ? -kmax : kr > kmax ? kmax : kr == kr ? kr : 0.f);
            v |= ((uint32_t)kc & 0xffu) << (8 * e);
        }
        if (off) sp.off[pos] = 1;
        uint32_t* A = tiles + (int64_t)sp.tile[pos] * m.tstride + THDR;
        A[(slot >> 2) * STEPW + ((slot & 3) * 16 + sp.row[pos]) * 4 + e4] = v;
    }
    // the row constants
    if (tid < SETROWS && sp.chan[tid] >= 0) {
        const int o = sp.chan[tid], r = sp.row[tid];
        uint32_t* T = tiles + (int64_t)sp.tile[tid] * m.tstride;
        const float s = sw[(int64_t)o * sw_stride];
        const float al = s_a * s, b = bias ? bias[o] : 0.f;
        T[T_AL + r] = mn_f2u(al); T[T_B + r] = mn_f2u(b); T[T_DEST + r] = (uint32_t)tid;
        if (!fin(al) || !fin(b) || !scale_ok(s)) atomicAdd(tab + 0, 1u);
        if (r == 0) T[0] = (uint32_t)(sp.grp[tid] * m.Cg >> 4);          // (groups == 1 with any C: group 0 starts at block 0)
    }
    mn_sets::tally_off(sp, tab + 7);
}

// ---------------------------------------------------------------- MFMA contraction + the requantisation chain -> output bytes
struct IFwd {
    int total, CB, OB, H, W, Ho, Wo, nsteps, nsets, slots, tstride, slot_off, cnt_off, tiles_off, spb;
};

// clamp(rha(fl(r / s)), qmin, qmax) of a finite r
__device__ __forceinline__ float code_of(float r, float s, float qmin, float qmax) { return fminf(fmaxf(mn_rha(r / s), qmin), qmax); }

template <int KS, bool POOL>
__global__ __launch_bounds__(256) void k_i8conv(const uint32_t* __restrict__ tab, const u32x4* __restrict__ x, u32x4* __restrict__ y, IFwd q) {
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
    const float s_p = mn_u2f(tab[8]), s_out = mn_u2f(tab[9]), qmin = mn_u2f(tab[10]), qmax = mn_u2f(tab[11]);
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
            // the lane's rows 4 kq .. 4 kq + 3 of the tile (D[row = 4 kq + reg][col = n])
            const f32x4 al = *reinterpret_cast<const f32x4*>(tile + T_AL + 4 * kq);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(tile + T_B + 4 * kq);
            const i32x4 ds = *reinterpret_cast<const i32x4*>(tile + T_DEST + 4 * kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (ds[r] < 0 || ds[r] >= SETROWS) continue;          // a dead row
                int8_t* const dst = imgb + ((ds[r] >> 4) * NPIX + n) * 16 + (ds[r] & 15);
                if (POOL) {
                    float mx = qmin;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float yv = (float)acc[t][r] * al[r] + bb[r];
                        mx = fmaxf(mx, code_of(fmaxf(yv, 0.f), s_p, qmin, qmax));
                    }
                    dst[0] = (int8_t)(int)code_of(mx * s_p, s_out, qmin, qmax);
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float yv = (float)acc[t][r] * al[r] + bb[r];
                        dst[256 * t] = (int8_t)(int)code_of(fmaxf(yv, 0.f), s_out, qmin, qmax);
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

// ---------------------------------------------------------------- fp32 NCHW <-> blocked codes
// one thread = one 16-byte block: 16 channels of one pixel (reads coalesced along pixels per channel), the code clamp(rha(x / s)) of the consumer's quantizer; position
// j of the output holds channel out_order[j] (the consumer's channel shuffle), 0 past C or for a bad entry
__global__ __launch_bounds__(256) void k_i8_pack(const float* __restrict__ x, u32x4* __restrict__ out, int64_t total, int C, int CB, int HW, float s, float qmin, float qmax,
                                                 const int32_t* __restrict__ order) {
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
        const float cf = mn_clamp(mn_rha(xv / s), qmin, qmax);
        const int ci = cf == cf ? (int)cf : 0;
        v[d >> 2] |= ((uint32_t)ci & 0xffu) << (8 * (d & 3));
    }
    out[i] = v;
}

// one thread = one element of the fp32 NCHW tensor: fl(float(c) * s)
__global__ __launch_bounds__(256) void k_i8_unpack(const int8_t* __restrict__ in, float* __restrict__ y, int64_t total, int C, int CB, int HW, float s) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int pix = (int)(i % HW);
    const int64_t t = i / HW;
    const int c = (int)(t % C);
    const int64_t nimg = t / C;
    y[i] = (float)in[((nimg * CB + (c >> 4)) * HW + pix) * 16 + (c & 15)] * s;
}

}  // namespace mn_iao8

// (passed as an argument of "%s", never as a format)
#define MN_I8CONV_COVER "geometry or width not covered (code widths 2 .. 8; 1x1 / stride 1 / padding 0 with groups 1 or C / groups % 16 == 0, or 3x3 / stride 1 / padding 1 with C / groups % 16 == 0)"

extern "C" int mn_i8conv_supported(const mn_conv_geom* g, int a_bits, int w_bits) {
    mn_iao8::IGeom m;
    return mn_iao8::make_igeom(g, a_bits, w_bits, m) ? 1 : 0;
}

extern "C" int64_t mn_i8conv_table_bytes(const mn_conv_geom* g, int a_bits, int w_bits) {
    mn_iao8::IGeom m;
    if (!mn_iao8::make_igeom(g, a_bits, w_bits, m)) return 0;
    return 4 * mn_iao8::table_words(m);
}

extern "C" int mn_i8conv_pack(const mn_conv_geom* g, const float* w, const float* s_w, int s_w_stride, const float* bias, float s_a, float s_p, float s_out, int a_bits,
                              int w_bits, const int32_t* out_order, uint32_t* table, mn_stream_t stream) {
    mn_iao8::IGeom m;
    if (!w || !s_w || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)s_w | (uintptr_t)bias | (uintptr_t)out_order) & 3) || s_w_stride < 0 || s_w_stride > 1 ||
        !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_i8conv_pack: null / unaligned argument (the table is 16-byte aligned), s_w_stride outside 0 / 1 or invalid geometry");
    if (!mn_iao8::make_igeom(g, a_bits, w_bits, m)) MN_FAIL(MN_ENOTSUP, "mn_i8conv_pack: %s", MN_I8CONV_COVER);
    if (hipMemsetAsync(table, 0, 4 * mn_iao8::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_i8conv_pack: header reset failed");          // the two counters
    mn_set_last_kernel("k_i8conv_wpack");
    hipLaunchKernelGGL(mn_iao8::k_i8conv_wpack, dim3(m.nsets), dim3(256), 0, (hipStream_t)stream, m, w, s_w, s_w_stride, bias, s_a, s_p, s_out, out_order, table);
    MN_CHECK_LAUNCH("mn_i8conv_pack");
    return MN_OK;
}

extern "C" int mn_i8conv_fwd(const mn_conv_geom* g, int a_bits, int w_bits, const uint32_t* table, const int8_t* in_codes, int8_t* out_codes, int pool, mn_stream_t stream) {
    mn_iao8::IGeom m;
    if (!table || !in_codes || !out_codes || !aligned16(table) || !aligned16(in_codes) || !aligned16(out_codes) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_i8conv_fwd: null / unaligned argument (table and codes are 16-byte aligned) or invalid geometry");
    if (!mn_iao8::make_igeom(g, a_bits, w_bits, m)) MN_FAIL(MN_ENOTSUP, "mn_i8conv_fwd: %s", MN_I8CONV_COVER);
    if (pool < 0 || pool > 1) MN_FAIL(MN_ENOTSUP, "mn_i8conv_fwd: pool must be 0 or 1 (2x2 / stride 2)");
    if (pool && ((m.H & 1) || (m.W & 1))) MN_FAIL(MN_EINVAL, "mn_i8conv_fwd: the folded 2x2 max-pool needs even H and W");
    mn_iao8::IFwd f;
    f.CB = m.CB; f.OB = m.OB; f.H = m.H; f.W = m.W; f.nsteps = m.nsteps; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride;
    f.slot_off = m.slot_off; f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off;
    f.Ho = pool ? m.H / 2 : m.H; f.Wo = pool ? m.W / 2 : m.W;
    f.total = m.N * f.Ho * f.Wo;
    const int ppb = pool ? 64 : 256;          // (pooled) pixels per block: four waves of four N tiles
    const int bx = (f.total + ppb - 1) / ppb;
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const u32x4* xin = reinterpret_cast<const u32x4*>(in_codes);
    u32x4* yout = reinterpret_cast<u32x4*>(out_codes);
    mn_set_last_kernel("k_i8conv<%d,%d>", m.KS, pool);
    mn_prof_bytes(16.0 * m.N * m.CB * m.H * m.W + 16.0 * m.N * m.OB * f.Ho * f.Wo + 4.0 * (double)mn_iao8::table_words(m));
    mn_prof_begin(s);
    if (m.KS == 3) {
        if (pool) hipLaunchKernelGGL((mn_iao8::k_i8conv<3, true>), grid, dim3(256), 0, s, table, xin, yout, f);
        else hipLaunchKernelGGL((mn_iao8::k_i8conv<3, false>), grid, dim3(256), 0, s, table, xin, yout, f);
    } else {
        if (pool) hipLaunchKernelGGL((mn_iao8::k_i8conv<1, true>), grid, dim3(256), 0, s, table, xin, yout, f);
        else hipLaunchKernelGGL((mn_iao8::k_i8conv<1, false>), grid, dim3(256), 0, s, table, xin, yout, f);
    }
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_i8conv_fwd");
    return MN_OK;
}
#undef MN_I8CONV_COVER

static int i8_codes_args(const char* who, const void* a, const void* b, int64_t N, int64_t C, int64_t HW, float s) {
    if (!a || !b || N <= 0 || C <= 0 || HW <= 0 || !mn_iao8::scale_ok(s)) MN_FAIL(MN_EINVAL, "%s: null / empty argument or a scale that is not finite and positive", who);
    if (N * ((C + 15) / 16) * HW >= (1ll << 27)) MN_FAIL(MN_ENOTSUP, "%s: tensor too large", who);
    return MN_OK;
}

extern "C" int mn_i8_pack_codes(const float* x, int64_t N, int64_t C, int64_t HW, float s, int a_bits, const int32_t* out_order, int8_t* codes, mn_stream_t stream) {
    if ((((uintptr_t)x | (uintptr_t)out_order) & 3) || !aligned16(codes)) MN_FAIL(MN_EINVAL, "mn_i8_pack_codes: unaligned argument (x 4-byte, codes 16-byte aligned)");
    const int rc = i8_codes_args("mn_i8_pack_codes", x, codes, N, C, HW, s);
    if (rc != MN_OK) return rc;
    if (a_bits < 2 || a_bits > 8) MN_FAIL(MN_ENOTSUP, "mn_i8_pack_codes: code widths 2 .. 8");
    const int CB = (int)((C + 15) / 16);
    const int64_t total = N * CB * HW;
    mn_set_last_kernel("k_i8_pack");
    mn_prof_bytes(4.0 * N * C * HW + 16.0 * (double)total);
    mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_iao8::k_i8_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, reinterpret_cast<u32x4*>(codes), total, (int)C, CB,
                       (int)HW, s, -(float)(1 << (a_bits - 1)), (float)((1 << (a_bits - 1)) - 1), out_order);
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_i8_pack_codes");
    return MN_OK;
}

extern "C" int mn_i8_unpack_codes(const int8_t* codes, int64_t N, int64_t C, int64_t HW, float s, float* y, mn_stream_t stream) {
    if ((((uintptr_t)y) & 3) || !aligned16(codes)) MN_FAIL(MN_EINVAL, "mn_i8_unpack_codes: unaligned argument (y 4-byte, codes 16-byte aligned)");
    const int rc = i8_codes_args("mn_i8_unpack_codes", codes, y, N, C, HW, s);
    if (rc != MN_OK) return rc;
    const int CB = (int)((C + 15) / 16);
    const int64_t total = N * C * HW;
    mn_set_last_kernel("k_i8_unpack");
    mn_prof_bytes(16.0 * N * CB * HW + 4.0 * (double)total);
    mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_iao8::k_i8_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codes, y, total, (int)C, CB, (int)HW, s);
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_i8_unpack_codes");
    return MN_OK;
}
