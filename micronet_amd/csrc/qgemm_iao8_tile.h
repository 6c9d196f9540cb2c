// What plain nin adds to the int8 deployment of the BN-folded IAO graph (mn_i8conv5_*, mn_i8_maxpool): the dense 5x5 / padding 2 hidden block on an LDS-resident halo
// tile, and the 3x3 / 2 / 1 and 2x2 / 2 / 0 QuantMaxPool2d as a stage of its own on the code map.  Included by qgemm_bits.hip behind qgemm_iao8_e2e.h.  Layout (int8
// [N][ceil(C/16)][H*W][16], tail channels 0), contraction (acc = sum j k, exact in int32), the set / tile table, the chain and the output path are those of qgemm_iao8.h,
// and the table is built by its packer k_i8conv_wpack -- whose slot word for a 5x5 geometry has three bits per tap offset (dy | dx << 3 | chunk << 6); the tables of the
// 1x1 and 3x3 geometries are as they were.  Work split and staging are those of k_code8conv5 (qgemm_codes_w8_tile.h).
//
//   why a tile  : k_i8conv gathers every B operand from global memory behind a bounds test per tap.  A 5x5 window reuses each input pixel 25 times, so here the block's
//                 input is staged ONCE in LDS and the k-loop reads nothing else.
//   work split  : a 256-thread block owns a tile of at most 256 output pixels: IMG whole images where a map has at most 256 pixels (IMG = 256 / (H W), less where LDS or
//                 the batch says so), else a band of TH output rows of one image at full width (TH = 256 / W, less where LDS says so; W <= 256).  Block pixel p is
//                 (image p / (TH W), row p % (TH W) / W, column p % W); a wave takes 64 of them as four 16-pixel N tiles and walks the sets dealt to blockIdx.y by
//                 mn_sets::grid_deal.  Pixels past the tile, the image or the batch are computed on a valid address and never stored.
//   staging     : all 256 threads copy the tile's input with its halo of 2 into LDS with 16-byte loads, consecutive threads consecutive pixels of a row:
//                 s_in[chunk][image][TH + 4][W + 4] sixteen-byte blocks.  A zero byte is the value 0, so halo cells, cells outside the image and images outside the
//                 batch are zero bytes: zero padding is DATA, an image boundary inside a block a halo like any other, and the k-loop has no bounds test and no mask.
//                 A padding slot of the last k-step reads the lane's own pixel of chunk 0 against zero weight bytes, as in k_i8conv; a slot word that names a tap or a
//                 chunk outside the geometry is read there too, so nothing outside the staged tile is addressed whatever the table says.  ONE __syncthreads() behind
//                 the staging; no block barrier after it.
//   k-loop      : A operands stream from the L2-resident table; the B operand of N tile t is ONE ds_read_b128 at (the lane's pixel) + (the slot's tap / chunk offset):
//                 the 16 pixel lanes of an N tile that lie in one row read 256 contiguous bytes.
//   output      : the per-wave LDS image [4 blocks][64 pixels][16 bytes] of k_i8conv between wave barriers, read back as whole 16-byte blocks: every output byte is
//                 stored exactly once, no atomics, no read-modify-write on global memory.
//   LDS         : at most 3071 blocks of staged tile (48 KB less one block) + 16 KB of output images.  The host picks IMG and TH from the geometry (make_tgeom); a
//                 geometry whose one-row tile does not fit -- ceil(C/16) * 5 * (W + 4) > 3071 -- is refused.  nin's block (96 channels, 16 x 16) stages a whole image:
//                 6 * 20 * 20 blocks = 38.4 KB.
//   max-pool    : k_i8_maxpool -- one thread per 16-byte output block; per byte m = the signed maximum over the in-map taps of the window (a tap outside the map is
//                 skipped; every window holds a real pixel), then c = clamp(rha(fl(fl(float(m) * s_p) / s_out))): the pooled tail of k_i8conv's chain.  Exact, because
//                 the modules quantise at s_p first and take the maximum of the quantised values; the block in front is packed with s_p as its s_out.  A tail byte is
//                 0 in every tap and stays 0.  Not in place.
// Covered: code widths 2 .. 8; 5x5 / stride 1 / padding 2 / dilation 1, groups 1, C % 16 == 0, any O; C * 25 * 2^(a-1) * (2^(w-1) - 1) <= INT_MAX; W <= 256 and
// ceil(C/16) * 5 * (W + 4) <= 3071; any H, any N.  No folded pool, no in_shuffle gather; an out_order for a consumer's shuffle as in mn_i8conv_pack.
#pragma once
#include "qgemm_iao8_e2e.h"

namespace mn_iao8 {

enum { T5_PIX = 256, T5_LDS = 3071 };          // output pixels of a block tile; 16-byte blocks of the staged tile

struct TGeom {
    IGeom m;
    int IMG, TH, bands;          // whole images per block tile (TH == H, bands == 1) or output rows of the band (IMG == 1); tiles per image
};

static inline bool make_tgeom(const mn_conv_geom* g, int a_bits, int w_bits, TGeom& r) {
    IGeom& m = r.m;
    if (!g || g->N <= 0 || g->C <= 0 || g->H <= 0 || g->W <= 0 || g->O <= 0) return false;
    if (a_bits < 2 || a_bits > 8 || w_bits < 2 || w_bits > 8) return false;
    if (g->KH != 5 || g->KW != 5 || g->stride_h != 1 || g->stride_w != 1 || g->dil_h != 1 || g->dil_w != 1 || g->pad_h != 2 || g->pad_w != 2) return false;
    if (g->groups != 1 || g->in_shuffle > 1 || (g->C & 15)) return false;
    m.N = g->N; m.C = g->C; m.H = g->H; m.W = g->W; m.O = g->O; m.KS = 5; m.groups = 1;
    m.Cg = g->C; m.Og = g->O; m.taps = 25;
    m.a_bits = a_bits; m.w_bits = w_bits;
    if ((int64_t)m.Cg * m.taps * (1 << (a_bits - 1)) * ((1 << (w_bits - 1)) - 1) > (int64_t)INT_MAX) return false;          // acc is exact in int32
    m.CB = g->C >> 4; m.OB = (g->O + 15) >> 4;
    m.chunks = m.CB;
    m.nslots = m.taps * m.chunks;
    m.nsteps = (m.nslots + 3) >> 2;
    m.nsets = (m.OB + 3) >> 2;
    m.tstride = THDR + STEPW * m.nsteps;
    m.slot_off = HDR;
    m.cnt_off = HDR + 4 * m.nsteps;
    if (!mn_sets::table_layout(m, 1, m.cnt_off)) return false;
    const int64_t blocks = (int64_t)g->N * (m.CB > m.OB ? m.CB : m.OB) * g->H * g->W;          // 16-byte blocks: indexed in int
    if (blocks >= (1ll << 27) || g->W > T5_PIX) return false;
    // the tile shape: as many pixels as the block has lanes for and LDS has room for
    const int HW = g->H * g->W;
    const auto staged = [&](int img, int th) { return (int64_t)m.CB * img * (th + 4) * (g->W + 4); };
    r.IMG = HW <= T5_PIX ? T5_PIX / HW : 1;
    r.IMG = r.IMG < g->N ? r.IMG : g->N;
    r.TH = HW <= T5_PIX ? g->H : T5_PIX / g->W;
    while (r.IMG > 1 && staged(r.IMG, r.TH) > T5_LDS) --r.IMG;
    while (r.TH > 0 && staged(r.IMG, r.TH) > T5_LDS) --r.TH;
    if (r.TH < 1) return false;          // a single row with its halo does not fit
    r.bands = (g->H + r.TH - 1) / r.TH;
    return true;
}

// ---------------------------------------------------------------- the 5x5 block: LDS halo tile -> MFMA contraction -> the block's chain -> output bytes
struct ITile {
    int N, CB, OB, H, W;
    int IMG, TH, bands;
    int LH, LW, cstride, nstage;          // staged rows and columns of an image (TH + 4, W + 4), blocks of a chunk (IMG LH LW), blocks of the tile
    int nsteps, nsets, slots, tstride, slot_off, cnt_off, tiles_off, spb;
};

template <int KS>
__global__ __launch_bounds__(256) void k_i8conv5(const uint32_t* __restrict__ tab, const u32x4* __restrict__ x, u32x4* __restrict__ y, ITile q) {
    constexpr int R = KS / 2;          // the halo
    __shared__ u32x4 s_in[T5_LDS];          // [chunk][image][LH][LW]
    __shared__ u32x4 s_img[4][4 * 64];          // per wave: [4 blocks of the set][pixels][16 bytes]
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int HW = q.H * q.W, tpix = q.TH * q.W;
    const int tb = (int)blockIdx.x / q.bands;
    const int img0 = tb * q.IMG, row0 = ((int)blockIdx.x - tb * q.bands) * q.TH;
    const u32x4 zero = u32x4{0u, 0u, 0u, 0u};          // sixteen codes 0
    // ---- the tile with its halo: consecutive threads, consecutive pixels of a staged row
    for (int i = tid; i < q.nstage; i += 256) {
        const int t0 = i / q.LW, cc = i - t0 * q.LW;
        const int t1 = t0 / q.LH, rr = t0 - t1 * q.LH;
        const int cb = t1 / q.IMG, li = t1 - cb * q.IMG;
        const int im = img0 + li, h = row0 + rr - R, w = cc - R;
        u32x4 v = zero;
        if (im < q.N && (unsigned)h < (unsigned)q.H && (unsigned)w < (unsigned)q.W) v = x[(im * q.CB + cb) * HW + h * q.W + w];
        s_in[i] = v;
    }
    u32x4* const img = s_img[wave];
    int8_t* const imgb = reinterpret_cast<int8_t*>(img);
    for (int i = lane; i < 4 * 64; i += 64) img[i] = zero;
    __syncthreads();
    // ---- the centre tap of the lane's pixel of every N tile in the staged tile (a pixel past the tile: the first pixel's, computed and never stored)
    int paddr[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = wave * 64 + 16 * t + n;
        const int li = p / tpix, r = p - li * tpix;
        const int row = r / q.W, col = r - row * q.W;
        paddr[t] = li < q.IMG ? (li * q.LH + row + R) * q.LW + col + R : R * q.LW + R;
    }
    // what this lane stores: the blocks of block pixel 64 wave + lane
    const int ps = wave * 64 + lane;
    const int sli = ps / tpix, sr = ps - sli * tpix;
    const int sim = img0 + sli, sh = row0 + sr / q.W;
    const bool sok = sli < q.IMG && sim < q.N && sh < q.H;
    u32x4* const ybase = y + (sok ? (int64_t)sim * q.OB * HW + row0 * q.W + sr : 0);
    const float s_out = mn_u2f(tab[9]), qmin = mn_u2f(tab[10]), qmax = mn_u2f(tab[11]);
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        MN_WAVE_SYNC();          // the image is zero before any lane writes into it
        const int cnt = (int)tab[q.cnt_off + set];
        const int nt = mn_uniform(cnt < q.slots ? cnt : q.slots);
        for (int i = 0; i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            i32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = i32x4{0, 0, 0, 0};
            const uint32_t* ap = tile + THDR + lane * 4;
#pragma unroll 1
            for (int s = 0; s < q.nsteps; ++s) {
                const uint32_t sl = tab[q.slot_off + 4 * s + kq];
                const int dy = (int)(sl & 7u), dx = (int)((sl >> 3) & 7u), cb = (int)(sl >> 6);
                const bool real = dy < KS && dx < KS && cb < q.CB;          // (nothing outside the staged tile is addressed, whatever the table says)
                const int off = real ? cb * q.cstride + (dy - R) * q.LW + (dx - R) : 0;
                const u32x4 a = *reinterpret_cast<const u32x4*>(ap + s * STEPW);
                u32x4 b[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) b[t] = s_in[paddr[t] + off];
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
                int8_t* const dst = imgb + ((ds[r] >> 4) * 64 + n) * 16 + (ds[r] & 15);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float yv = (float)acc[t][r] * al[r] + bb[r];
                    dst[256 * t] = (int8_t)(int)code_of(fmaxf(yv, 0.f), s_out, qmin, qmax);
                }
            }
        }
        MN_WAVE_SYNC();          // every byte of the set is in the image
#pragma unroll
        for (int bk = 0; bk < 4; ++bk) {
            const u32x4 v = img[bk * 64 + lane];
            img[bk * 64 + lane] = zero;
            const int ob = 4 * set + bk;
            if (sok && ob < q.OB) ybase[(int64_t)ob * HW] = v;
        }
    }
}

// ---------------------------------------------------------------- max-pool with requantisation on the code map
// one thread = one 16-byte output block (consecutive threads: consecutive output pixels of a row)
__global__ __launch_bounds__(256) void k_i8_maxpool(const u32x4* __restrict__ in, u32x4* __restrict__ out, int64_t total, int H, int W, int Ho, int Wo, int k, int s,
                                                    int pad, float s_p, float s_out, float qmin, float qmax) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ow = (int)(i % Wo);
    const int64_t t = i / Wo;
    const int oh = (int)(t % Ho);
    const u32x4* src = in + (t / Ho) * H * W;          // (image, 16-channel block)
    int m[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) m[d] = -128;          // no byte is smaller, and every window holds a real pixel
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
            const int ih = oh * s - pad + dy, iw = ow * s - pad + dx;
            if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
            const u32x4 v = src[ih * W + iw];
#pragma unroll
            for (int d = 0; d < 16; ++d) {
                const int c = (int)(int8_t)((v[d >> 2] >> (8 * (d & 3))) & 0xffu);
                m[d] = c > m[d] ? c : m[d];
            }
        }
    u32x4 r = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        const int c = (int)code_of((float)m[d] * s_p, s_out, qmin, qmax);
        r[d >> 2] |= ((uint32_t)c & 0xffu) << (8 * (d & 3));
    }
    out[i] = r;
}

}  // namespace mn_iao8

// (passed as an argument of "%s", never as a format)
#define MN_I8CONV5_COVER "geometry or width not covered (code widths 2 .. 8; dense 5x5 / stride 1 / padding 2 / dilation 1 with C % 16 == 0, W <= 256 and ceil(C / 16) * 5 * (W + 4) <= 3071: one output row with its halo in 48 KB of LDS)"

extern "C" int mn_i8conv5_supported(const mn_conv_geom* g, int a_bits, int w_bits) {
    mn_iao8::TGeom r;
    return mn_iao8::make_tgeom(g, a_bits, w_bits, r) ? 1 : 0;
}

extern "C" int64_t mn_i8conv5_table_bytes(const mn_conv_geom* g, int a_bits, int w_bits) {
    mn_iao8::TGeom r;
    if (!mn_iao8::make_tgeom(g, a_bits, w_bits, r)) return 0;
    return 4 * mn_iao8::table_words(r.m);
}

extern "C" int mn_i8conv5_pack(const mn_conv_geom* g, const float* w, const float* s_w, int s_w_stride, const float* bias, float s_a, float s_out, int a_bits, int w_bits,
                               const int32_t* out_order, uint32_t* table, mn_stream_t stream) {
    mn_iao8::TGeom r;
    if (!w || !s_w || !table || !aligned16(table) || (((uintptr_t)w | (uintptr_t)s_w | (uintptr_t)bias | (uintptr_t)out_order) & 3) || s_w_stride < 0 || s_w_stride > 1 ||
        !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_i8conv5_pack: null / unaligned argument (the table is 16-byte aligned), s_w_stride outside 0 / 1 or invalid geometry");
    if (!mn_iao8::make_tgeom(g, a_bits, w_bits, r)) MN_FAIL(MN_ENOTSUP, "mn_i8conv5_pack: %s", MN_I8CONV5_COVER);
    if (hipMemsetAsync(table, 0, 4 * mn_iao8::HDR, (hipStream_t)stream) != hipSuccess) MN_FAIL(MN_EHIP, "mn_i8conv5_pack: header reset failed");          // the two counters
    mn_set_last_kernel("k_i8conv_wpack");
    hipLaunchKernelGGL(mn_iao8::k_i8conv_wpack, dim3(r.m.nsets), dim3(256), 0, (hipStream_t)stream, r.m, w, s_w, s_w_stride, bias, s_a, s_out, s_out, out_order, table);
    MN_CHECK_LAUNCH("mn_i8conv5_pack");
    return MN_OK;
}

extern "C" int mn_i8conv5_fwd(const mn_conv_geom* g, int a_bits, int w_bits, const uint32_t* table, const int8_t* in_codes, int8_t* out_codes, mn_stream_t stream) {
    mn_iao8::TGeom r;
    if (!table || !in_codes || !out_codes || !aligned16(table) || !aligned16(in_codes) || !aligned16(out_codes) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_i8conv5_fwd: null / unaligned argument (table and codes are 16-byte aligned) or invalid geometry");
    if (!mn_iao8::make_tgeom(g, a_bits, w_bits, r)) MN_FAIL(MN_ENOTSUP, "mn_i8conv5_fwd: %s", MN_I8CONV5_COVER);
    const mn_iao8::IGeom& m = r.m;
    const int64_t nin = 16ll * m.N * m.CB * m.H * m.W, nout = 16ll * m.N * m.OB * m.H * m.W;
    if (mn_iao8::ranges_meet(out_codes, nout, in_codes, nin)) MN_FAIL(MN_EINVAL, "mn_i8conv5_fwd: the output overlaps the input");
    mn_iao8::ITile f;
    f.N = m.N; f.CB = m.CB; f.OB = m.OB; f.H = m.H; f.W = m.W;
    f.IMG = r.IMG; f.TH = r.TH; f.bands = r.bands;
    f.LH = r.TH + 4; f.LW = m.W + 4; f.cstride = r.IMG * f.LH * f.LW; f.nstage = m.CB * f.cstride;
    f.nsteps = m.nsteps; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride; f.slot_off = m.slot_off; f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off;
    const int bx = (m.N + r.IMG - 1) / r.IMG * r.bands;          // the block tiles
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    mn_set_last_kernel("k_i8conv5<%d>", m.KS);
    mn_prof_bytes((double)nin + (double)nout + 4.0 * (double)mn_iao8::table_words(m));
    mn_prof_begin(s);
    hipLaunchKernelGGL((mn_iao8::k_i8conv5<5>), grid, dim3(256), 0, s, table, reinterpret_cast<const u32x4*>(in_codes), reinterpret_cast<u32x4*>(out_codes), f);
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_i8conv5_fwd");
    return MN_OK;
}
#undef MN_I8CONV5_COVER

extern "C" int mn_i8_maxpool(const int8_t* map_in, int64_t N, int64_t C, int64_t H, int64_t W, int k, int stride, int pad, float s_p, float s_out, int a_bits,
                             int8_t* map_out, mn_stream_t stream) {
    if (!map_in || !map_out || !aligned16(map_in) || !aligned16(map_out) || N <= 0 || C <= 0 || H <= 0 || W <= 0 || !mn_iao8::scale_ok(s_p) || !mn_iao8::scale_ok(s_out))
        MN_FAIL(MN_EINVAL, "mn_i8_maxpool: null / empty argument, a map that is not 16-byte aligned or a scale that is not finite and positive");
    if (!((k == 2 && stride == 2 && pad == 0) || (k == 3 && stride == 2 && pad == 1)))
        MN_FAIL(MN_ENOTSUP, "mn_i8_maxpool: window not covered (2x2 / stride 2 / padding 0 or 3x3 / stride 2 / padding 1, floor mode)");
    if (a_bits < 2 || a_bits > 8) MN_FAIL(MN_ENOTSUP, "mn_i8_maxpool: code widths 2 .. 8");
    const int64_t CB = (C + 15) / 16;
    if (H > (1 << 15) || W > (1 << 15) || N * CB * H * W >= (1ll << 27)) MN_FAIL(MN_ENOTSUP, "mn_i8_maxpool: tensor too large");
    if (H + 2 * pad < k || W + 2 * pad < k) MN_FAIL(MN_EINVAL, "mn_i8_maxpool: image smaller than the window");
    const int Ho = (int)((H + 2 * pad - k) / stride + 1), Wo = (int)((W + 2 * pad - k) / stride + 1);
    const int64_t total = N * CB * Ho * Wo;
    if (mn_iao8::ranges_meet(map_out, 16 * total, map_in, 16 * N * CB * H * W)) MN_FAIL(MN_EINVAL, "mn_i8_maxpool: the output overlaps the input (not an in-place kernel)");
    mn_set_last_kernel("k_i8_maxpool");
    mn_prof_bytes(16.0 * N * CB * H * W + 16.0 * (double)total);
    mn_prof_begin((hipStream_t)stream);
    hipLaunchKernelGGL(mn_iao8::k_i8_maxpool, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const u32x4*>(map_in),
                       reinterpret_cast<u32x4*>(map_out), total, (int)H, (int)W, Ho, Wo, k, stride, pad, s_p, s_out, -(float)(1 << (a_bits - 1)),
                       (float)((1 << (a_bits - 1)) - 1));
    mn_prof_end((hipStream_t)stream);
    MN_CHECK_LAUNCH("mn_i8_maxpool");
    return MN_OK;
}
