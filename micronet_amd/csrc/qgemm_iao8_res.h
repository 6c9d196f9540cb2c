// The residual stages of the int8 deployment of BN-folded IAO ResNets (mn_i8res_*): strided convs with an optional ReLU, and the last conv of a block's
// residual_function fused with the block's QuantAdd, its ReLU and the quantizers of the block's (up to two) consumers -- bytes in, bytes out.  Included by
// qgemm_bits.hip behind qgemm_iao8_ends.h, whose layout, chain, weight table (k_i8conv_wpack) and set / tile planner it shares (namespace mn_iao8).
//
//   conv stage   : y = fl(fl(float(acc) * al) + b), r = relu ? max(y, 0) : y, c = clamp(rha(fl(r / s_out)), qmin, qmax).  Output pixel (h, w) reads input pixel
//                  (stride h + dy, stride w + dx), dy, dx in -1 .. 1 for the 3x3 / padding 1 and 0 for the 1x1 / padding 0, zero bytes outside the INPUT map.
//   add stage    : c_r = clamp(rha(fl(y / s_add))) (no ReLU), c_s = the shortcut's byte of the same channel and pixel (already a code at s_add),
//                  t = fl(fl(float(c_r) * s_add) + fl(float(c_s) * s_add)), v = max(t, 0), out_k = clamp(rha(fl(v / s_k)), -2^(a_k-1), 2^(a_k-1) - 1), k = A [, B].
//   weight table : mn_i8conv_pack's, built by k_i8conv_wpack with s_p = s_out (the add stage: s_out = s_add, the width of the add); the geometry check alone is new.
//                  k_i8res_add reads s_add and its range from its by-value struct, never from the table's words 9 .. 11: the entry cannot compare the two without a
//                  device read, so packing the table at s_add / add_bits is the caller's duty (the header says so).
//   kernels      : k_i8res_conv<KS, STRIDE, RELU> is k_i8conv<KS, 0> with the pixel -> input-offset rule above.  k_i8res_add<KS, NOUT> runs the same contraction and
//                  writes the bytes of c_r into the wave's LDS image; behind the block barrier a lane holds the four whole 16-byte blocks of one pixel, loads the
//                  matching 16-byte shortcut block (one coalesced load), evaluates t, v and out_k on the 16 byte pairs and stores one 16-byte block per output map.
//                  Positions >= O: the image is zero there and so is the shortcut's tail, t = 0, the code 0.  No atomics, no read-modify-write on global memory,
//                  every output byte stored exactly once.  Both kernels keep their own copy of the contraction loop (res_acc): k_i8conv's is left as measured.
// Covered: groups 1, dilation 1, no in_shuffle, 1x1 / padding 0 with any C or 3x3 / padding 1 with C % 16 == 0, stride 1 or 2 (both directions equal; the add stage:
// stride 1), any O, H, W >= 1, code widths 2 .. 8.
#pragma once
#include "qgemm_iao8_ends.h"

namespace mn_iao8 {

struct RGeom {
    IGeom m;                    // H, W: the input map
    int stride, Ho, Wo;
};

static inline bool make_rgeom(const mn_conv_geom* g, int in_bits, int out_bits, int w_bits, RGeom& r) {
    IGeom& m = r.m;
    if (!g || g->N <= 0 || g->C <= 0 || g->H <= 0 || g->W <= 0 || g->O <= 0) return false;
    if (in_bits < 2 || in_bits > 8 || out_bits < 2 || out_bits > 8 || w_bits < 2 || w_bits > 8) return false;
    if (g->KH != g->KW || (g->KH != 1 && g->KH != 3)) return false;
    const int pad = (g->KH - 1) / 2;
    if (g->stride_h != g->stride_w || (g->stride_h != 1 && g->stride_h != 2)) return false;
    if (g->dil_h != 1 || g->dil_w != 1 || g->pad_h != pad || g->pad_w != pad || g->groups != 1 || g->in_shuffle != 0) return false;
    if ((g->C & 15) && g->KH != 1) return false;
    m.N = g->N; m.C = g->C; m.H = g->H; m.W = g->W; m.O = g->O; m.KS = g->KH; m.groups = 1;
    m.Cg = g->C; m.Og = g->O; m.taps = g->KH * g->KW;
    if ((int64_t)m.Cg * m.taps * (1 << (in_bits - 1)) * ((1 << (w_bits - 1)) - 1) > (int64_t)INT_MAX) return false;          // acc is exact in int32
    m.a_bits = out_bits; m.w_bits = w_bits;          // (the table's code range is the OUTPUT's)
    m.CB = (g->C + 15) >> 4; m.OB = (g->O + 15) >> 4;
    m.chunks = m.CB;
    m.nslots = m.taps * m.chunks;
    m.nsteps = (m.nslots + 3) >> 2;
    m.nsets = (m.OB + 3) >> 2;
    m.tstride = THDR + STEPW * m.nsteps;
    m.slot_off = HDR;
    m.cnt_off = HDR + 4 * m.nsteps;
    if (!mn_sets::table_layout(m, 1, m.cnt_off)) return false;
    r.stride = g->stride_h;
    r.Ho = (g->H - 1) / r.stride + 1; r.Wo = (g->W - 1) / r.stride + 1;          // (H + 2 pad - KS) / stride + 1 of either form
    const int64_t bin = (int64_t)g->N * m.CB * g->H * g->W, bout = (int64_t)g->N * m.OB * r.Ho * r.Wo;          // 16-byte blocks: indexed in int
    if (bin >= (1ll << 27) || bout >= (1ll << 27)) return false;
    return true;
}

static inline void make_rfwd(const RGeom& r, IFwd& f) {
    const IGeom& m = r.m;
    f.CB = m.CB; f.OB = m.OB; f.H = m.H; f.W = m.W; f.nsteps = m.nsteps; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride;
    f.slot_off = m.slot_off; f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off;
    f.Ho = r.Ho; f.Wo = r.Wo;
    f.total = m.N * r.Ho * r.Wo;
}

// the quantizers of the add stage, by value
struct RAdd {
    float s_add, amin, amax;
    float s[2], qmin[2], qmax[2];
};

// acc[t] = the tile's 16 rows against the 16 pixels of N tile t over every k-step.  ph / pw: row and column of the INPUT pixel under the centre tap (stride * h,
// stride * w; a pixel outside the batch has row -4: every tap is outside), xoff: block 0 at that pixel.  The loop of k_i8conv, with its own copy here.
template <int KS>
__device__ __forceinline__ void res_acc(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ tile, const u32x4* __restrict__ x, const IFwd& q, int HW, int lane,
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

// the input pixel under the centre tap of the lane's output pixel of every N tile
template <int STRIDE>
__device__ __forceinline__ void res_pixels(const IFwd& q, int pb, int n, int HW, int HWo, int (&ph)[4], int (&pw)[4], int (&xoff)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = pb + 16 * t + n;
        const int pc = p < q.total ? p : 0;
        const int img = pc / HWo, r = pc - img * HWo;
        const int h = r / q.Wo, wc = r - h * q.Wo;
        ph[t] = p < q.total ? STRIDE * h : -4; pw[t] = STRIDE * wc;
        xoff[t] = img * q.CB * HW + STRIDE * h * q.W + STRIDE * wc;
    }
}

template <int KS, int STRIDE, bool RELU>
__global__ __launch_bounds__(256) void k_i8res_conv(const uint32_t* __restrict__ tab, const u32x4* __restrict__ x, u32x4* __restrict__ y, IFwd q) {
    __shared__ u32x4 s_img[4][4 * 64];          // per wave: [4 blocks of the set][pixels][16 bytes]
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HW = q.H * q.W, HWo = q.Ho * q.Wo;
    const int pb = ((int)blockIdx.x * 4 + wave) * 64;
    int ph[4], pw[4], xoff[4];
    res_pixels<STRIDE>(q, pb, n, HW, HWo, ph, pw, xoff);
    // what this lane stores: the blocks of output pixel pb + lane
    const int ps = pb + lane;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HWo;
    u32x4* const ybase = y + (int64_t)simg * q.OB * HWo + (psc - simg * HWo);
    u32x4* const img = s_img[wave];
    int8_t* const imgb = reinterpret_cast<int8_t*>(img);
    const float s_out = mn_u2f(tab[9]), qmin = mn_u2f(tab[10]), qmax = mn_u2f(tab[11]);
    for (int i = lane; i < 4 * 64; i += 64) img[i] = u32x4{0u, 0u, 0u, 0u};
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        __syncthreads();          // the image is zero before any lane writes into it
        const int nt = (int)tab[q.cnt_off + set] < q.slots ? (int)tab[q.cnt_off + set] : q.slots;          // wave-uniform
        for (int i = 0; i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            i32x4 acc[4];
            res_acc<KS>(tab, tile, x, q, HW, lane, kq, ph, pw, xoff, acc);
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
                    dst[256 * t] = (int8_t)(int)code_of(RELU ? fmaxf(yv, 0.f) : yv, s_out, qmin, qmax);
                }
            }
        }
        __syncthreads();          // every byte of the set is in the image
#pragma unroll
        for (int bk = 0; bk < 4; ++bk) {
            const u32x4 v = img[bk * 64 + lane];
            img[bk * 64 + lane] = u32x4{0u, 0u, 0u, 0u};
            const int ob = 4 * set + bk;
            if (sok && ob < q.OB) ybase[(int64_t)ob * HWo] = v;
        }
    }
}

// the 16 byte pairs (c_r, c_s) of one block -> the 16 output bytes at one consumer's quantizer
__device__ __forceinline__ u32x4 add_block(const u32x4 cr, const u32x4 cs, float s_add, float s, float qmin, float qmax) {
    u32x4 o = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        const float fr = (float)(int8_t)(cr[d >> 2] >> (8 * (d & 3))), fs = (float)(int8_t)(cs[d >> 2] >> (8 * (d & 3)));
        const float t = fr * s_add + fs * s_add;          // (no contraction: two products, each rounded, then their sum)
        const int c = (int)code_of(fmaxf(t, 0.f), s, qmin, qmax);
        o[d >> 2] |= ((uint32_t)c & 0xffu) << (8 * (d & 3));
    }
    return o;
}

template <int KS, int NOUT>
__global__ __launch_bounds__(256) void k_i8res_add(const uint32_t* __restrict__ tab, const u32x4* __restrict__ x, const u32x4* __restrict__ sc, u32x4* __restrict__ ya,
                                                   u32x4* __restrict__ yb, IFwd q, RAdd p) {
    __shared__ u32x4 s_img[4][4 * 64];          // per wave: [4 blocks of the set][pixels][16 bytes] of c_r
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HW = q.H * q.W;          // (stride 1: the output map is the input map)
    const int pb = ((int)blockIdx.x * 4 + wave) * 64;
    int ph[4], pw[4], xoff[4];
    res_pixels<1>(q, pb, n, HW, HW, ph, pw, xoff);
    const int ps = pb + lane;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HW;
    const int64_t obase = (int64_t)simg * q.OB * HW + (psc - simg * HW);          // block 0 of the lane's pixel in the shortcut and in every output map
    u32x4* const img = s_img[wave];
    int8_t* const imgb = reinterpret_cast<int8_t*>(img);
    for (int i = lane; i < 4 * 64; i += 64) img[i] = u32x4{0u, 0u, 0u, 0u};
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        __syncthreads();          // the image is zero before any lane writes into it
        const int nt = (int)tab[q.cnt_off + set] < q.slots ? (int)tab[q.cnt_off + set] : q.slots;          // wave-uniform
        for (int i = 0; i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            i32x4 acc[4];
            res_acc<KS>(tab, tile, x, q, HW, lane, kq, ph, pw, xoff, acc);
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
                    dst[256 * t] = (int8_t)(int)code_of(yv, p.s_add, p.amin, p.amax);          // c_r: no ReLU in front of the add
                }
            }
        }
        __syncthreads();          // every byte of the set is in the image
#pragma unroll 1
        for (int bk = 0; bk < 4; ++bk) {
            const u32x4 cr = img[bk * 64 + lane];
            img[bk * 64 + lane] = u32x4{0u, 0u, 0u, 0u};
            const int ob = 4 * set + bk;
            if (sok && ob < q.OB) {
                const int64_t at = obase + (int64_t)ob * HW;
                const u32x4 cs = sc[at];
                ya[at] = add_block(cr, cs, p.s_add, p.s[0], p.qmin[0], p.qmax[0]);
                if (NOUT == 2) yb[at] = add_block(cr, cs, p.s_add, p.s[1], p.qmin[1], p.qmax[1]);
            }
        }
    }
}

// [a, a + na) and [b, b + nb) share a byte
static inline bool ranges_meet(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

}  // namespace mn_iao8

// (passed as an argument of "%s", never as a format)
#define MN_I8RES_COVER "geometry or width not covered (code widths 2 .. 8; groups 1, dilation 1, no in_shuffle, 1x1 / padding 0 with any C or 3x3 / padding 1 with C % 16 == 0, stride 1 or 2 in both directions)"

extern "C" int mn_i8res_supported(const mn_conv_geom* g, int in_bits, int out_bits, int w_bits) {
    mn_iao8::RGeom r;
    return mn_iao8::make_rgeom(g, in_bits, out_bits, w_bits, r) ? 1 : 0;
}

extern "C" int64_t mn_i8res_table_bytes(const mn_conv_geom* g, int in_bits, int out_bits, int w_bits) {
    mn_iao8::RGeom r;
    if (!mn_iao8::make_rgeom(g, in_bits, out_bits, w_bits, r)) return 0;
    return 4 * mn_iao8::table_words(r.m);
}

extern "C" int mn_i8res_pack(const mn_conv_geom* g, const float* w, const float* s_w, int s_w_stride, const float* bias, float s_a, float s_out, int in_bits, int out_bits,
                             int w_bits, uint32_t* table, mn_stream_t stream) {
    mn_iao8::RGeom r;
    if (!w || !s_w || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)s_w | (uintptr_t)bias) & 3) || s_w_stride < 0 || s_w_stride > 1 || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_i8res_pack: null / unaligned argument (the table is 16-byte aligned), s_w_stride outside 0 / 1 or invalid geometry");
    if (!mn_iao8::make_rgeom(g, in_bits, out_bits, w_bits, r)) MN_FAIL(MN_ENOTSUP, "mn_i8res_pack: %s", MN_I8RES_COVER);
    if (hipMemsetAsync(table, 0, 4 * mn_iao8::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_i8res_pack: header reset failed");          // the two counters
    mn_set_last_kernel("k_i8conv_wpack");
    hipLaunchKernelGGL(mn_iao8::k_i8conv_wpack, dim3(r.m.nsets), dim3(256), 0, (hipStream_t)stream, r.m, w, s_w, s_w_stride, bias, s_a, s_out, s_out,
                       (const int32_t*)nullptr, table);
    MN_CHECK_LAUNCH("mn_i8res_pack");
    return MN_OK;
}

extern "C" int mn_i8res_conv_fwd(const mn_conv_geom* g, int in_bits, int out_bits, int w_bits, const uint32_t* table, const int8_t* in_codes, int8_t* out_codes, int relu,
                                 mn_stream_t stream) {
    mn_iao8::RGeom r;
    if (!table || !in_codes || !out_codes || !aligned16(table) || !aligned16(in_codes) || !aligned16(out_codes) || !tile_geom_valid(g) || relu < 0 || relu > 1)
        MN_FAIL(MN_EINVAL, "mn_i8res_conv_fwd: null / unaligned argument (table and codes are 16-byte aligned), invalid geometry or relu outside 0 / 1");
    if (!mn_iao8::make_rgeom(g, in_bits, out_bits, w_bits, r)) MN_FAIL(MN_ENOTSUP, "mn_i8res_conv_fwd: %s", MN_I8RES_COVER);
    const mn_iao8::IGeom& m = r.m;
    const int64_t nin = 16ll * m.N * m.CB * m.H * m.W, nout = 16ll * m.N * m.OB * r.Ho * r.Wo;
    if (mn_iao8::ranges_meet(out_codes, nout, in_codes, nin)) MN_FAIL(MN_EINVAL, "mn_i8res_conv_fwd: the output overlaps the input");
    mn_iao8::IFwd f;
    mn_iao8::make_rfwd(r, f);
    const int bx = (f.total + 255) / 256;          // four waves of four N tiles
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const u32x4* xin = reinterpret_cast<const u32x4*>(in_codes);
    u32x4* yout = reinterpret_cast<u32x4*>(out_codes);
    mn_set_last_kernel("k_i8res_conv<%d,%d,%d>", m.KS, r.stride, relu);
    mn_prof_bytes((double)nin + (double)nout + 4.0 * (double)mn_iao8::table_words(m));
    mn_prof_begin(s);
#define MN_I8RES_LAUNCH(KS, ST, RL) hipLaunchKernelGGL((mn_iao8::k_i8res_conv<KS, ST, RL>), grid, dim3(256), 0, s, table, xin, yout, f)
    if (m.KS == 3) {
        if (r.stride == 2) { if (relu) MN_I8RES_LAUNCH(3, 2, true); else MN_I8RES_LAUNCH(3, 2, false); }
        else { if (relu) MN_I8RES_LAUNCH(3, 1, true); else MN_I8RES_LAUNCH(3, 1, false); }
    } else {
        if (r.stride == 2) { if (relu) MN_I8RES_LAUNCH(1, 2, true); else MN_I8RES_LAUNCH(1, 2, false); }
        else { if (relu) MN_I8RES_LAUNCH(1, 1, true); else MN_I8RES_LAUNCH(1, 1, false); }
    }
#undef MN_I8RES_LAUNCH
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_i8res_conv_fwd");
    return MN_OK;
}

extern "C" int mn_i8res_add_fwd(const mn_conv_geom* g, int in_bits, int w_bits, const uint32_t* table, const int8_t* in_codes, const int8_t* shortcut_codes,
                                const mn_i8res_add* q, int8_t* out_a, int8_t* out_b, mn_stream_t stream) {
    mn_iao8::RGeom r;
    if (!table || !in_codes || !shortcut_codes || !q || !out_a || !aligned16(table) || !aligned16(in_codes) || !aligned16(shortcut_codes) || !aligned16(out_a) ||
        !aligned16(out_b) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_i8res_add_fwd: null / unaligned argument (table and codes are 16-byte aligned) or invalid geometry");
    if (q->nout < 1 || q->nout > 2 || (q->nout == 2) != (out_b != nullptr)) MN_FAIL(MN_EINVAL, "mn_i8res_add_fwd: nout must be 1 (out_b null) or 2 (out_b set)");
    const float sk[2] = {q->s_out0, q->s_out1};
    const int bk[2] = {q->bits0, q->bits1};
    if (!mn_iao8::scale_ok(q->s_add) || q->add_bits < 2 || q->add_bits > 8)
        MN_FAIL(MN_EINVAL, "mn_i8res_add_fwd: s_add must be finite and positive, add_bits 2 .. 8");
    for (int k = 0; k < q->nout; ++k)
        if (!mn_iao8::scale_ok(sk[k]) || bk[k] < 2 || bk[k] > 8) MN_FAIL(MN_EINVAL, "mn_i8res_add_fwd: output %d: the scale must be finite and positive, the width 2 .. 8", k);
    if (!mn_iao8::make_rgeom(g, in_bits, q->add_bits, w_bits, r)) MN_FAIL(MN_ENOTSUP, "mn_i8res_add_fwd: %s", MN_I8RES_COVER);
    if (r.stride != 1) MN_FAIL(MN_ENOTSUP, "mn_i8res_add_fwd: the add stage is stride 1 (the residual and the shortcut share one map)");
    const mn_iao8::IGeom& m = r.m;
    const int64_t nin = 16ll * m.N * m.CB * m.H * m.W, nout = 16ll * m.N * m.OB * m.H * m.W;
    int8_t* const outs[2] = {out_a, out_b};
    for (int k = 0; k < q->nout; ++k)
        if (mn_iao8::ranges_meet(outs[k], nout, in_codes, nin) || mn_iao8::ranges_meet(outs[k], nout, shortcut_codes, nout) ||
            (k == 1 && mn_iao8::ranges_meet(out_a, nout, out_b, nout)))
            MN_FAIL(MN_EINVAL, "mn_i8res_add_fwd: output %d overlaps an input or the other output", k);
    mn_iao8::IFwd f;
    mn_iao8::make_rfwd(r, f);
    mn_iao8::RAdd p;
    p.s_add = q->s_add; p.amin = -(float)(1 << (q->add_bits - 1)); p.amax = (float)((1 << (q->add_bits - 1)) - 1);
    for (int k = 0; k < 2; ++k) {
        const int kk = k < q->nout ? k : 0;
        p.s[k] = sk[kk]; p.qmin[k] = -(float)(1 << (bk[kk] - 1)); p.qmax[k] = (float)((1 << (bk[kk] - 1)) - 1);
    }
    const int bx = (f.total + 255) / 256;
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));
    const hipStream_t s = (hipStream_t)stream;
    const u32x4* xin = reinterpret_cast<const u32x4*>(in_codes);
    const u32x4* sin = reinterpret_cast<const u32x4*>(shortcut_codes);
    u32x4* ya = reinterpret_cast<u32x4*>(out_a);
    u32x4* yb = reinterpret_cast<u32x4*>(out_b);
    mn_set_last_kernel("k_i8res_add<%d,%d>", m.KS, q->nout);
    mn_prof_bytes((double)nin + (double)nout * (1 + q->nout) + 4.0 * (double)mn_iao8::table_words(m));
    mn_prof_begin(s);
    if (m.KS == 3) {
        if (q->nout == 2) hipLaunchKernelGGL((mn_iao8::k_i8res_add<3, 2>), grid, dim3(256), 0, s, table, xin, sin, ya, yb, f, p);
        else hipLaunchKernelGGL((mn_iao8::k_i8res_add<3, 1>), grid, dim3(256), 0, s, table, xin, sin, ya, yb, f, p);
    } else {
        if (q->nout == 2) hipLaunchKernelGGL((mn_iao8::k_i8res_add<1, 2>), grid, dim3(256), 0, s, table, xin, sin, ya, yb, f, p);
        else hipLaunchKernelGGL((mn_iao8::k_i8res_add<1, 1>), grid, dim3(256), 0, s, table, xin, sin, ya, yb, f, p);
    }
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_i8res_add_fwd");
    return MN_OK;
}
#undef MN_I8RES_COVER
