// The residual stages of the DoReFa W8A8 byte plan (mn_code8_quant_map, mn_code8res_conv_*, mn_code8res_add_*): a ResNet BasicBlock
//   x -> conv_a (3x3, stride 1 | 2) -> bn_a -> relu -> conv_b (3x3) -> bn_b -> (+ shortcut(x)) -> relu,      shortcut = identity | bn_s(conv_s 1x1, stride 1 | 2)
// on byte maps.  Included by qgemm_bits.hip behind qgemm_codes_w8_ends.h; layout (int8 [N][ceil(C/16)][H*W][16], byte = code - 128, tails 0x80), identity
// (acc = 2 sum a w' + sum a + Kc[o]), the one edge rule (a 0x80 byte contributes nothing) and the set / tile table are those of qgemm_codes_w8.h, and the table is built by
// its packer k_code8_wpack, unchanged: the geometry gate alone is new (make_rgeom: stride 1 | 2, groups 1).  k_code8conv is left as measured; the contraction loop
// below (res_acc) is a copy of its own.
//
//   quant     : k_code8_quant -- fp32 NCHW -> the byte map in one launch, byte = qa_code(a, 1/255) ^ 0x80 (the 8-bit DoReFa activation quantizer of the consumer on the
//               stem's fp32 output), tail channels 0x80.  One thread = one 16-byte block (16 channels of a pixel): per channel the loads of a wave are 64 consecutive
//               floats, the store is one whole block, coalesced along pixels.  It replaces k_qa_fwd + k_code8_pack.
//   conv      : k_code8res_conv<KS, STRIDE> -- conv_a -> bn_a -> relu -> the 8-bit code of conv_b's quantizer.  k_code8conv's wave with the pixel rule of a strided conv:
//               output pixel (h, w) reads input pixel (s h + dy, s w + dx); a tap outside the INPUT map reads 0x80; sum a runs over the B operands actually loaded,
//               so it is formed over the taps addressed, whatever the stride.
//   add       : k_code8res_add<KS, SC> -- the block's end in ONE launch.  Per output channel o and pixel p
//                   z = qa_eval<0>((float)acc_b, QaCh_b)                      conv_b (stride 1) on the mid byte map -> bn_b
//                   r = SC == 1 ? res_f32[n][o][p]                            the block's fp32 input (NCHW)
//                     : SC == 2 ? qa_eval<0>((float)acc_s, QaCh_s) : 0        conv_s (1x1 / padding 0 / stride 1 | 2) on the block INPUT's byte map -> bn_s: a second table
//                   a = qa_relu(z + r)                                        the op order of k_qr_fwd: two rounded values, then their sum
//               and writes qa_code(a, 1/255) ^ 0x80 into the byte map the next block's convs read and / or a itself into the fp32 NCHW map the next block's identity
//               shortcut (or avg_pool) reads.  Both tables are packed with a null out_order: position j of a set IS channel 64 set + j, in the branch's table and in the
//               shortcut's alike, so tile i of a set holds the same 16 channels in both.
//     work split  : a wave owns 64 pixels as four N tiles and one set (four output blocks) at a time, as k_code8conv does; the waves of a block share nothing and there
//                   is no block barrier.
//     SC == 2     : the shortcut's K is short (C_in / 16 slots: ONE k-step for 64 -> 128).  Per tile it runs FIRST, with its own sum a_s (formed with the set's first
//                   tile) and Kc_s, and is collapsed at once to the 16 fp32 values r[t][reg] of the lane; only then the long branch loop starts, into the same 16
//                   accumulator registers' worth: two int32 accumulator sets are never live together.
//     SC == 1     : the lane's 16 residual loads are issued in front of the branch k-loop and land behind it; for a fixed channel the 16 lanes of an N tile read 16
//                   consecutive pixels (one 64-byte segment), the four kq lane groups four consecutive channels.
//     byte output : through the per-wave LDS image [4 blocks][64 pixels][16 bytes] of k_code8conv (0x80-filled, handed over by a wave barrier), read back as whole blocks
//                   and stored once, coalesced along pixels.
//     fp32 output : stored DIRECTLY from the accumulator layout -- for a fixed (reg, N tile) the 16 lanes of a kq group store 16 consecutive pixels of one channel: whole
//                   64-byte segments, each written once.  Staging 64 x 64 floats per wave for longer rows would cost 16 KB of LDS per wave (64 KB per block, one block
//                   per CU's worth of waves) for maps whose rows are 4 .. 32 pixels: not taken.
//     stores      : every output element is stored exactly once: no atomics, no read-modify-write on global memory.  Positions >= O of the byte map are 0x80 (the image's
//                   fill); the fp32 map has no tail and nothing is written past channel O or past the batch.
// Covered: a_in = w_bits = a_out = 8; groups 1, dilation 1, no in_shuffle; 3x3 / padding 1 with C % 16 == 0 or 1x1 / padding 0 with any C; stride 1 | 2 (both directions
// equal); any O; C * taps <= 33025.  The add stage: the branch conv at stride 1; an identity shortcut needs O == C (a BasicBlock's mid map has the channels of its
// output); a conv shortcut is 1x1 / padding 0 with the branch's N and O and an output map of the branch's size.
#pragma once
#include "qgemm_codes_w8_ends.h"

namespace mn_code8 {

struct RGeom {
    W8Geom m;                   // H, W: the input map
    int stride, Ho, Wo;
};

static inline bool make_rgeom(const mn_conv_geom* g, int a_in, int w_bits, int a_out, RGeom& r) {
    W8Geom& m = r.m;
    if (!g || g->N <= 0 || g->C <= 0 || g->H <= 0 || g->W <= 0 || g->O <= 0) return false;
    if (a_in != 8 || w_bits != 8 || a_out != 8) return false;
    if (g->KH != g->KW || (g->KH != 1 && g->KH != 3)) return false;
    const int pad = (g->KH - 1) / 2;
    if (g->stride_h != g->stride_w || (g->stride_h != 1 && g->stride_h != 2)) return false;
    if (g->dil_h != 1 || g->dil_w != 1 || g->pad_h != pad || g->pad_w != pad || g->groups != 1 || g->in_shuffle != 0) return false;
    if ((g->C & 15) && g->KH != 1) return false;
    m.N = g->N; m.C = g->C; m.H = g->H; m.W = g->W; m.O = g->O; m.KS = g->KH; m.groups = 1;
    m.Cg = g->C; m.Og = g->O; m.taps = g->KH * g->KW;
    if ((int64_t)m.Cg * m.taps > KMAX) return false;          // acc and its three terms are exact in int32
    m.CB = (g->C + 15) >> 4; m.OB = (g->O + 15) >> 4;
    m.chunks = m.CB;
    m.nslots = m.taps * m.chunks;
    m.T = m.nslots * 16;
    m.nsteps = (m.nslots + 3) >> 2;
    m.nsets = (m.OB + 3) >> 2;
    m.tstride = THDR + STEPW * m.nsteps;
    m.slot_off = HDR;
    m.cnt_off = HDR + 4 * m.nsteps;
    if (!mn_sets::table_layout(m, 1, m.cnt_off)) return false;
    r.stride = g->stride_h;
    r.Ho = (g->H - 1) / r.stride + 1; r.Wo = (g->W - 1) / r.stride + 1;          // (H + 2 pad - KS) / stride + 1 of either form
    const int64_t bin = (int64_t)g->N * m.CB * g->H * g->W, bout = (int64_t)g->N * m.OB * r.Ho * r.Wo;          // 16-byte blocks: indexed in int
    return bin < (1ll << 27) && bout < (1ll << 27);          // (the fp32 maps are indexed in int64)
}

static inline void make_rfwd(const RGeom& r, W8Fwd& f) {
    const W8Geom& m = r.m;
    f.CB = m.CB; f.OB = m.OB; f.H = m.H; f.W = m.W; f.nsteps = m.nsteps; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride;
    f.slot_off = m.slot_off; f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off;
    f.Ho = r.Ho; f.Wo = r.Wo;
    f.total = m.N * r.Ho * r.Wo;
    f.s = 1.0f / 255.0f;
}

// ---------------------------------------------------------------- fp32 NCHW -> the byte map at the consumer's 8-bit quantizer
// one thread = one 16-byte block: 16 channels of one pixel (reads coalesced along pixels per channel); tail channels 0x80
__global__ __launch_bounds__(256) void k_code8_quant(const float* __restrict__ x, u32x4* __restrict__ out, int64_t total, int C, int CB, int HW, float s) {
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
        const uint32_t j = c < C ? qa_code(x[(nimg * C + c) * HW + pix], s) : 0u;
        v[d >> 2] |= ((j & 0xffu) ^ 0x80u) << (8 * (d & 3));
    }
    out[i] = v;
}

// ---------------------------------------------------------------- the contraction of one tile, shared by the three uses below
// the map a contraction reads and the part of its table's layout the loop needs
struct W8Src {
    int CB, H, W, nsteps, slot_off;
};

// the lane's output pixel of every N tile and the input pixel under its centre tap: ph / pw = row and column in the INPUT map (stride h, stride w; a pixel outside
// the batch has row -4: every tap is outside), xoff = block 0 at that pixel.  HWo / Wo: the output map.
__device__ __forceinline__ void res_pixels(int stride, int total, int pb, int n, int CB, int H, int W, int HWo, int Wo, int (&ph)[4], int (&pw)[4], int (&xoff)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = pb + 16 * t + n;
        const int pc = p < total ? p : 0;
        const int im = pc / HWo, r = pc - im * HWo;
        const int h = r / Wo, wc = r - h * Wo;
        ph[t] = p < total ? stride * h : -4; pw[t] = stride * wc;
        xoff[t] = im * CB * H * W + stride * h * W + stride * wc;
    }
}

// acc[t] = the tile's 16 rows against the 16 pixels of N tile t over every k-step; with `first` (wave-uniform) sum a of the four pixels is formed along with it from the
// B operands the lane holds and reduced over the four kq lanes of a pixel.  The loop of k_code8conv, with its own copy here.
template <int KS>
__device__ __forceinline__ void res_acc(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ tile, const u32x4* __restrict__ x, const W8Src& q, int lane, int kq,
                                        const int (&ph)[4], const int (&pw)[4], const int (&xoff)[4], bool first, int (&sa)[4], i32x4 (&acc)[4]) {
    const u32x4 fill = u32x4{0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};          // sixteen codes 0
    const int HW = q.H * q.W;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = i32x4{0, 0, 0, 0};
    if (first) sa[0] = sa[1] = sa[2] = sa[3] = 0;
    const uint32_t* ap = tile + THDR + lane * 4;
#pragma unroll 1
    for (int s = 0; s < q.nsteps; ++s) {
        const uint32_t sl = tab[q.slot_off + 4 * s + kq];
        const int dy = KS == 3 ? (int)(sl & 3u) - 1 : 0, dx = KS == 3 ? (int)((sl >> 2) & 3u) - 1 : 0, cb = (int)((sl >> 4) & 0xffffu);
        const bool real = (sl & PADSLOT) == 0u && cb < q.CB;          // (a block past the map is never addressed, whatever the table says)
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
}

// the forward-chain constants of the lane's rows 4 kq .. 4 kq + 3 of a tile (D[row = 4 kq + reg][col = n])
struct RowCh {
    f32x4 ch[6];
    i32x4 kc;
};
__device__ __forceinline__ RowCh load_rows(const uint32_t* __restrict__ tile, int kq) {
    RowCh c;
#pragma unroll
    for (int j = 0; j < 6; ++j) c.ch[j] = *reinterpret_cast<const f32x4*>(tile + T_CH + 16 * j + 4 * kq);
    c.kc = *reinterpret_cast<const i32x4*>(tile + T_KC + 4 * kq);
    return c;
}
// z of row r on the three terms of the identity
__device__ __forceinline__ float row_z(const RowCh& c, int r, int acc, int sa) {
    QaCh k;
    k.alpha = c.ch[0][r]; k.bias = c.ch[1][r]; k.mean = c.ch[2][r]; k.invstd = c.ch[3][r]; k.ga = c.ch[4][r]; k.be = c.ch[5][r];
    k.A = k.B = k.gi = 0.f;          // (not part of the forward chain)
    const int full = (int)(2u * (uint32_t)acc + (uint32_t)sa + (uint32_t)c.kc[r]);
    float zh, z;
    qa_eval<0>((float)full, k, zh, z);
    return z;
}

// the set's image -> global memory: whole 16-byte blocks of the lane's pixel, the image re-filled behind them
__device__ __forceinline__ void store_set(u32x4* __restrict__ img, u32x4* __restrict__ ybase, int lane, int set, int OB, int HWo, bool sok) {
    const u32x4 fill = u32x4{0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
#pragma unroll
    for (int bk = 0; bk < 4; ++bk) {
        const u32x4 v = img[bk * 64 + lane];
        img[bk * 64 + lane] = fill;
        const int ob = 4 * set + bk;
        if (sok && ob < OB) ybase[(int64_t)ob * HWo] = v;
    }
}

// ---------------------------------------------------------------- conv_a: bytes in, bytes out, stride 1 | 2
template <int KS, int STRIDE>
__global__ __launch_bounds__(256) void k_code8res_conv(const uint32_t* __restrict__ tab, const u32x4* __restrict__ x, u32x4* __restrict__ y, W8Fwd q) {
    __shared__ u32x4 s_img[4][4 * 64];          // per wave: [4 blocks of the set][pixels][16 bytes]
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HWo = q.Ho * q.Wo;
    const int pb = ((int)blockIdx.x * 4 + wave) * 64;
    W8Src src;
    src.CB = q.CB; src.H = q.H; src.W = q.W; src.nsteps = q.nsteps; src.slot_off = q.slot_off;
    int ph[4], pw[4], xoff[4];
    res_pixels(STRIDE, q.total, pb, n, q.CB, q.H, q.W, HWo, q.Wo, ph, pw, xoff);
    // what this lane stores: the blocks of output pixel pb + lane
    const int ps = pb + lane;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HWo;
    u32x4* const ybase = y + (int64_t)simg * q.OB * HWo + (psc - simg * HWo);
    u32x4* const img = s_img[wave];
    int8_t* const imgb = reinterpret_cast<int8_t*>(img);
    for (int i = lane; i < 4 * 64; i += 64) img[i] = u32x4{0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
    int sa[4] = {0, 0, 0, 0};          // sum a at the pixel of N tile t (the same in the four kq lanes of a pixel)
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        MN_WAVE_SYNC();          // the image is filled before any lane writes into it
        const int cnt = (int)tab[q.cnt_off + set];
        const int nt = mn_uniform(cnt < q.slots ? cnt : q.slots);
        for (int i = 0; i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            const bool first = mn_uniform((int)tile[1]) != 0;          // groups 1: the set's first tile forms sum a, the other three reuse it
            i32x4 acc[4];
            res_acc<KS>(tab, tile, x, src, lane, kq, ph, pw, xoff, first, sa, acc);
            const RowCh c = load_rows(tile, kq);
            const i32x4 ds = *reinterpret_cast<const i32x4*>(tile + T_DEST + 4 * kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (ds[r] < 0 || ds[r] >= SETROWS) continue;          // a dead row
                int8_t* const dst = imgb + ((ds[r] >> 4) * 64 + n) * 16 + (ds[r] & 15);
#pragma unroll
                for (int t = 0; t < 4; ++t) dst[256 * t] = (int8_t)(uint8_t)(qa_code(qa_relu(row_z(c, r, acc[t][r], sa[t])), q.s) ^ 0x80u);
            }
        }
        MN_WAVE_SYNC();          // every byte of the set is in the image
        store_set(img, ybase, lane, set, q.OB, HWo, sok);
    }
}

// ---------------------------------------------------------------- conv_b -> bn_b -> + shortcut -> relu -> bytes and / or fp32
struct W8Add {
    W8Fwd b;                 // the branch: stride 1, H = Ho, W = Wo
    int O;                   // channels of the fp32 maps (residual in, activation out)
    // SC == 2: conv_s on the block input's byte map, and its table's layout
    W8Src s;
    int s_stride, s_slots, s_tstride, s_cnt_off, s_tiles_off;
};

template <int KS, int SC>
__global__ __launch_bounds__(256) void k_code8res_add(const uint32_t* __restrict__ tab, const u32x4* __restrict__ x, const uint32_t* __restrict__ tab_s,
                                                      const u32x4* __restrict__ xs, const float* __restrict__ res, u32x4* __restrict__ yb, float* __restrict__ yf, W8Add p) {
    __shared__ u32x4 s_img[4][4 * 64];          // per wave: [4 blocks of the set][pixels][16 bytes]
    const W8Fwd& q = p.b;
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HW = q.H * q.W;          // (stride 1: the output map is the branch's input map)
    const int pb = ((int)blockIdx.x * 4 + wave) * 64;
    W8Src src;
    src.CB = q.CB; src.H = q.H; src.W = q.W; src.nsteps = q.nsteps; src.slot_off = q.slot_off;
    int ph[4], pw[4], xoff[4];
    res_pixels(1, q.total, pb, n, q.CB, q.H, q.W, HW, q.W, ph, pw, xoff);
    int sph[4], spw[4], sxoff[4];          // SC == 2: the same pixels in the block input's map
    if (SC == 2) res_pixels(p.s_stride, q.total, pb, n, p.s.CB, p.s.H, p.s.W, HW, q.W, sph, spw, sxoff);
    int64_t foff[4];          // channel 0 of the fp32 maps at the pixel of N tile t, -1 outside the batch
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int pp = pb + 16 * t + n;
        const int pc = pp < q.total ? pp : 0, im = pc / HW;
        foff[t] = pp < q.total ? (int64_t)im * p.O * HW + (pc - im * HW) : -1;
    }
    const int ps = pb + lane;
    const bool sok = ps < q.total;
    const int psc = sok ? ps : 0;
    const int simg = psc / HW;
    u32x4* const ybase = yb + (int64_t)simg * q.OB * HW + (psc - simg * HW);
    u32x4* const img = s_img[wave];
    int8_t* const imgb = reinterpret_cast<int8_t*>(img);
    if (yb)
        for (int i = lane; i < 4 * 64; i += 64) img[i] = u32x4{0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u};
    int sa[4] = {0, 0, 0, 0}, sas[4] = {0, 0, 0, 0};          // sum a of the branch / of the shortcut at the pixel of N tile t
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        if (yb) MN_WAVE_SYNC();          // the image is filled before any lane writes into it
        int cnt = (int)tab[q.cnt_off + set];
        cnt = cnt < q.slots ? cnt : q.slots;
        if (SC == 2) {          // (the same O and a null order in both tables: the same count)
            const int cs = (int)tab_s[p.s_cnt_off + set];
            cnt = cnt < cs ? cnt : cs;
            cnt = cnt < p.s_slots ? cnt : p.s_slots;
        }
        const int nt = mn_uniform(cnt);
        for (int i = 0; i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            const bool first = mn_uniform((int)tile[1]) != 0;          // groups 1: the set's first tile forms sum a (and sum a_s), the other three reuse them
            const i32x4 ds = *reinterpret_cast<const i32x4*>(tile + T_DEST + 4 * kq);
            i32x4 acc[4];
            float rr[4][4];          // r of (N tile, row)
            if (SC == 2) {
                const uint32_t* tile_s = tab_s + p.s_tiles_off + (int64_t)(set * p.s_slots + i) * p.s_tstride;
                res_acc<1>(tab_s, tile_s, xs, p.s, lane, kq, sph, spw, sxoff, first, sas, acc);
                const RowCh cs = load_rows(tile_s, kq);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) rr[t][r] = row_z(cs, r, acc[t][r], sas[t]);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = set * SETROWS + ds[r];          // (a null out_order: position = channel)
                        rr[t][r] = 0.f;
                        if (SC == 1 && ds[r] >= 0 && ds[r] < SETROWS && o < p.O && foff[t] >= 0) rr[t][r] = res[foff[t] + (int64_t)o * HW];
                    }
            }
            res_acc<KS>(tab, tile, x, src, lane, kq, ph, pw, xoff, first, sa, acc);
            const RowCh c = load_rows(tile, kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = set * SETROWS + ds[r];
                if (ds[r] < 0 || ds[r] >= SETROWS || o >= p.O) continue;          // a dead row
                int8_t* const dst = imgb + ((ds[r] >> 4) * 64 + n) * 16 + (ds[r] & 15);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float z = row_z(c, r, acc[t][r], sa[t]);
                    const float a = qa_relu(SC ? z + rr[t][r] : z);
                    if (yf && foff[t] >= 0) yf[foff[t] + (int64_t)o * HW] = a;
                    if (yb) dst[256 * t] = (int8_t)(uint8_t)(qa_code(a, q.s) ^ 0x80u);
                }
            }
        }
        if (yb) {
            MN_WAVE_SYNC();          // every byte of the set is in the image
            store_set(img, ybase, lane, set, q.OB, HW, sok);
        }
    }
}

// [a, a + na) and [b, b + nb) share a byte
static inline bool ranges_meet(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

// the geometries of an add stage: the branch at stride 1; shortcut 1: O == C; shortcut 2: a 1x1 conv with the branch's N, O and output size
static inline bool make_ageom(const mn_conv_geom* g, int shortcut, const mn_conv_geom* gs, int a_in, int w_bits, int a_out, RGeom& r, RGeom& rs) {
    if (shortcut < 0 || shortcut > 2) return false;
    if (!make_rgeom(g, a_in, w_bits, a_out, r) || r.stride != 1) return false;
    if (shortcut == 1 && g->O != g->C) return false;
    if (shortcut == 2) {
        if (!make_rgeom(gs, a_in, w_bits, a_out, rs) || rs.m.KS != 1) return false;
        if (rs.m.N != r.m.N || rs.m.O != r.m.O || rs.Ho != r.m.H || rs.Wo != r.m.W) return false;
    }
    return true;
}

}  // namespace mn_code8

// (passed as an argument of "%s", never as a format)
#define MN_CODE8RES_COVER "geometry or width not covered (8-bit codes and weights throughout; groups 1, dilation 1, no in_shuffle, 1x1 / padding 0 with any C or 3x3 / padding 1 with C % 16 == 0, stride 1 or 2 in both directions, C * taps <= 33025)"

extern "C" int mn_code8_quant_map(const float* x, int64_t N, int64_t C, int64_t HW, int8_t* map, mn_stream_t stream) {
    const int rc = code8_map_args("mn_code8_quant_map", x, map, N, C, HW);
    if (rc != MN_OK) return rc;
    if (((uintptr_t)x) & 3) MN_FAIL(MN_EINVAL, "mn_code8_quant_map: x is not 4-byte aligned");
    const int CB = (int)((C + 15) / 16);
    const int64_t total = N * CB * HW;
    mn_set_last_kernel("k_code8_quant");
    mn_prof_bytes(4.0 * N * C * HW + 16.0 * (double)total);
    mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_code8::k_code8_quant, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, reinterpret_cast<u32x4*>(map), total, (int)C, CB,
                       (int)HW, 1.0f / 255.0f);
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_code8_quant_map");
    return MN_OK;
}

extern "C" int mn_code8res_conv_supported(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_code8::RGeom r;
    return mn_code8::make_rgeom(g, a_bits_in, w_bits, a_bits_out, r) ? 1 : 0;
}

extern "C" int64_t mn_code8res_conv_table_bytes(const mn_conv_geom* g, int a_bits_in, int w_bits, int a_bits_out) {
    mn_code8::RGeom r;
    if (!mn_code8::make_rgeom(g, a_bits_in, w_bits, a_bits_out, r)) return 0;
    return 4 * mn_code8::table_words(r.m);
}

extern "C" int mn_code8res_conv_pack(const mn_conv_geom* g, const float* w, const float* chan, int a_bits_in, int w_bits, int a_bits_out, uint32_t* table,
                                     mn_stream_t stream) {
    mn_code8::RGeom r;
    if (!w || !chan || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)chan) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_code8res_conv_pack: null / unaligned argument (the table is 16-byte aligned) or invalid geometry");
    if (!mn_code8::make_rgeom(g, a_bits_in, w_bits, a_bits_out, r)) MN_FAIL(MN_ENOTSUP, "mn_code8res_conv_pack: %s", MN_CODE8RES_COVER);
    mn_set_last_kernel("k_code8_wpack");
    hipLaunchKernelGGL(mn_code8::k_code8_clear, dim3(1), dim3(64), 0, (hipStream_t)stream, table);
    hipLaunchKernelGGL(mn_code8::k_code8_wpack, dim3(r.m.nsets), dim3(256), 0, (hipStream_t)stream, r.m, w, chan, (const int32_t*)nullptr, table);
    MN_CHECK_LAUNCH("mn_code8res_conv_pack");
    return MN_OK;
}

extern "C" int mn_code8res_conv_fwd(const mn_conv_geom* g, const uint32_t* table, const int8_t* in_codes, int8_t* out_codes, mn_stream_t stream) {
    mn_code8::RGeom r;
    if (!table || !in_codes || !out_codes || !aligned16(table) || !aligned16(in_codes) || !aligned16(out_codes) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_code8res_conv_fwd: null / unaligned argument (table and maps are 16-byte aligned) or invalid geometry");
    if (!mn_code8::make_rgeom(g, 8, 8, 8, r)) MN_FAIL(MN_ENOTSUP, "mn_code8res_conv_fwd: %s", MN_CODE8RES_COVER);
    const mn_code8::W8Geom& m = r.m;
    const int64_t nin = 16ll * m.N * m.CB * m.H * m.W, nout = 16ll * m.N * m.OB * r.Ho * r.Wo;
    if (mn_code8::ranges_meet(out_codes, nout, in_codes, nin)) MN_FAIL(MN_EINVAL, "mn_code8res_conv_fwd: the output overlaps the input");
    mn_code8::W8Fwd f;
    mn_code8::make_rfwd(r, f);
    const int bx = (f.total + 255) / 256;          // four waves of four N tiles
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const u32x4* xin = reinterpret_cast<const u32x4*>(in_codes);
    u32x4* yout = reinterpret_cast<u32x4*>(out_codes);
    mn_set_last_kernel("k_code8res_conv<%d,%d>", m.KS, r.stride);
    mn_prof_bytes((double)nin + (double)nout + 4.0 * (double)mn_code8::table_words(m));
    mn_prof_begin(s);
    if (m.KS == 3) {
        if (r.stride == 2) hipLaunchKernelGGL((mn_code8::k_code8res_conv<3, 2>), grid, dim3(256), 0, s, table, xin, yout, f);
        else hipLaunchKernelGGL((mn_code8::k_code8res_conv<3, 1>), grid, dim3(256), 0, s, table, xin, yout, f);
    } else {
        if (r.stride == 2) hipLaunchKernelGGL((mn_code8::k_code8res_conv<1, 2>), grid, dim3(256), 0, s, table, xin, yout, f);
        else hipLaunchKernelGGL((mn_code8::k_code8res_conv<1, 1>), grid, dim3(256), 0, s, table, xin, yout, f);
    }
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_code8res_conv_fwd");
    return MN_OK;
}

extern "C" int mn_code8res_add_supported(const mn_conv_geom* g, int shortcut, const mn_conv_geom* gs, int a_bits_in, int w_bits, int a_bits_out) {
    mn_code8::RGeom r, rs;
    return mn_code8::make_ageom(g, shortcut, gs, a_bits_in, w_bits, a_bits_out, r, rs) ? 1 : 0;
}

extern "C" int mn_code8res_add_fwd(const mn_conv_geom* g, const uint32_t* table, const int8_t* in_codes, int shortcut, const float* res_f32, const mn_conv_geom* gs,
                                   const uint32_t* table_s, const int8_t* sc_codes, int8_t* out_codes, float* out_f32, mn_stream_t stream) {
    mn_code8::RGeom r, rs;
    if (!table || !in_codes || !aligned16(table) || !aligned16(in_codes) || !aligned16(out_codes) || (((uintptr_t)out_f32) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_code8res_add_fwd: null / unaligned argument (tables and byte maps are 16-byte aligned, fp32 maps 4-byte) or invalid geometry");
    if (!out_codes && !out_f32) MN_FAIL(MN_EINVAL, "mn_code8res_add_fwd: no output requested (out_codes and out_f32 are both null)");
    if (shortcut == 1 && (!res_f32 || (((uintptr_t)res_f32) & 3))) MN_FAIL(MN_EINVAL, "mn_code8res_add_fwd: the identity shortcut needs res_f32 (4-byte aligned)");
    if (shortcut == 2 && (!table_s || !sc_codes || !aligned16(table_s) || !aligned16(sc_codes) || !tile_geom_valid(gs)))
        MN_FAIL(MN_EINVAL, "mn_code8res_add_fwd: the conv shortcut needs its geometry, table and input map (16-byte aligned)");
    if (!mn_code8::make_ageom(g, shortcut, gs, 8, 8, 8, r, rs))
        MN_FAIL(MN_ENOTSUP, "mn_code8res_add_fwd: %s; the add stage: shortcut 0 / 1 / 2, the branch conv at stride 1, an identity shortcut with O == C, a conv shortcut "
                            "1x1 / padding 0 with the branch's N and O and an output map of the branch's size", MN_CODE8RES_COVER);
    const mn_code8::W8Geom& m = r.m;
    const int64_t nin = 16ll * m.N * m.CB * m.H * m.W, nout = 16ll * m.N * m.OB * m.H * m.W, nf = 4ll * m.N * m.O * m.H * m.W;
    const int64_t nsc = shortcut == 2 ? 16ll * rs.m.N * rs.m.CB * rs.m.H * rs.m.W : 0;
    const void* const ins[3] = {in_codes, shortcut == 1 ? (const void*)res_f32 : nullptr, shortcut == 2 ? (const void*)sc_codes : nullptr};
    const int64_t nins[3] = {nin, nf, nsc};
    for (int k = 0; k < 3; ++k)
        if (mn_code8::ranges_meet(out_codes, nout, ins[k], nins[k]) || mn_code8::ranges_meet(out_f32, nf, ins[k], nins[k]))
            MN_FAIL(MN_EINVAL, "mn_code8res_add_fwd: an output overlaps an input");
    if (mn_code8::ranges_meet(out_codes, nout, out_f32, nf)) MN_FAIL(MN_EINVAL, "mn_code8res_add_fwd: the two outputs overlap");
    mn_code8::W8Add p;
    mn_code8::make_rfwd(r, p.b);
    p.O = m.O;
    p.s.CB = p.s.H = p.s.W = p.s.nsteps = p.s.slot_off = 0;
    p.s_stride = 1; p.s_slots = p.s_tstride = p.s_cnt_off = p.s_tiles_off = 0;
    if (shortcut == 2) {
        const mn_code8::W8Geom& ms = rs.m;
        p.s.CB = ms.CB; p.s.H = ms.H; p.s.W = ms.W; p.s.nsteps = ms.nsteps; p.s.slot_off = ms.slot_off;
        p.s_stride = rs.stride; p.s_slots = ms.slots; p.s_tstride = ms.tstride; p.s_cnt_off = ms.cnt_off; p.s_tiles_off = ms.tiles_off;
    }
    const int bx = (p.b.total + 255) / 256;          // four waves of four N tiles
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, p.b.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    const u32x4* xin = reinterpret_cast<const u32x4*>(in_codes);
    const u32x4* xsc = reinterpret_cast<const u32x4*>(shortcut == 2 ? sc_codes : nullptr);
    const uint32_t* ts = shortcut == 2 ? table_s : nullptr;
    const float* rf = shortcut == 1 ? res_f32 : nullptr;
    u32x4* yb = reinterpret_cast<u32x4*>(out_codes);
    mn_set_last_kernel("k_code8res_add<%d,%d>", m.KS, shortcut);
    mn_prof_bytes((double)nin + (double)nsc + (shortcut == 1 ? (double)nf : 0.0) + (out_codes ? (double)nout : 0.0) + (out_f32 ? (double)nf : 0.0) +
                  4.0 * (double)mn_code8::table_words(m) + (shortcut == 2 ? 4.0 * (double)mn_code8::table_words(rs.m) : 0.0));
    mn_prof_begin(s);
#define MN_CODE8RES_ADD(KS, SC) hipLaunchKernelGGL((mn_code8::k_code8res_add<KS, SC>), grid, dim3(256), 0, s, table, xin, ts, xsc, rf, yb, out_f32, p)
    if (m.KS == 3) {
        if (shortcut == 2) MN_CODE8RES_ADD(3, 2); else if (shortcut == 1) MN_CODE8RES_ADD(3, 1); else MN_CODE8RES_ADD(3, 0);
    } else {
        if (shortcut == 2) MN_CODE8RES_ADD(1, 2); else if (shortcut == 1) MN_CODE8RES_ADD(1, 1); else MN_CODE8RES_ADD(1, 0);
    }
#undef MN_CODE8RES_ADD
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_code8res_add_fwd");
    return MN_OK;
}
#undef MN_CODE8RES_COVER
