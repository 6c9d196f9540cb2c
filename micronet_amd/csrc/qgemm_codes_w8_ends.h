// The classifier end of the DoReFa W8A8 byte plan (mn_code8conv_fwd_f32): the last quantised conv -- 1x1, stride 1, one group -- reads the byte map of the last hidden
// stage and writes the fp32 map its own BatchNorm + ReLU takes.  Included by qgemm_bits.hip behind qgemm_codes_w8.h, whose layout, identity and weight table
// (k_code8_wpack, unchanged) it shares; the first-conv end is k_c1b_fwd<MT, 5> in conv_first.hip.
//
//   result   : acc = 2 sum a w' + sum a + Kc[o], exact in int32 (the identity of k_code8conv), then y[n][o][p] = fl(fl((float)acc * alpha) + bias[o]): plain NCHW fp32, no
//              ReLU, no code.  alpha and bias are rows 0 and 1 of the constants the table was packed from; the BatchNorm rows are not read.  The table is packed with a
//              null out_order: position j of a set IS channel 64 set + j.
//   why not k_code8conv with a float store : a classifier has ONE M tile (O = 10), a long K (1024 channels = 16 k-steps) and few pixels (64 per image).  A wave of
//              k_code8conv owns 64 pixels and walks all of K alone, and its set of four output blocks would leave three quarters of the schedule dead rows.
//   kernel   : a BLOCK owns 64 pixels as four N tiles and SPLITS K over its four waves: wave w takes the k-steps w, w + 4, ... of every M tile, runs the MFMAs of its
//              share for all four N tiles and forms its share of sum a by dot products on the B operands it holds.  With at most four k-steps per wave (C <= 1024) the B
//              operands are loaded ONCE into 64 registers and serve every M tile of the launch; a longer K streams them per tile from L1 / L2.  The four partial
//              accumulators (and, once, the partial sum a) meet in LDS -- integer addition: the result does not depend on the split -- and wave 0 applies alpha and
//              bias and stores: for a fixed channel the 16 lanes of an N tile store 16 consecutive pixels; rows past O and pixels past the batch are not written.
//              A wave without a k-step (fewer k-steps than waves) contributes zeros and still joins both barriers; a padding slot reads the zero byte against zero
//              weight bytes, a 0x80 byte contributes nothing whatever its weight byte: the edge rules of qgemm_codes_w8.h carry over unchanged.
// Covered: what mn_code8conv_supported covers with KH = KW = 1 and groups == 1: any C <= 33025, any O >= 1.
#pragma once
#include "qgemm_codes_w8.h"

namespace mn_code8 {

enum { F32_KEEP = 4 };          // k-steps of a wave whose B operands stay in registers (16 registers each)

struct W8F32 {
    int total, HW, CB, O, nsteps, nsets, slots, tstride, slot_off, cnt_off, tiles_off, spb;
};

__global__ __launch_bounds__(256) void k_code8conv_f32(const uint32_t* __restrict__ tab, const u32x4* __restrict__ x, float* __restrict__ y, W8F32 q) {
    __shared__ i32x4 s_acc[3][4][64];          // the accumulators of waves 1 .. 3: [wave - 1][N tile][lane]
    __shared__ int s_sa[3][4][16];             // their shares of sum a: [wave - 1][N tile][pixel]
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), n = lane & 15, kq = lane >> 4;
    const int pb = (int)blockIdx.x * 64;
    bool pok[4];
    int xoff[4];          // block 0 at the pixel of N tile t
    int64_t yoff[4];      // channel 0 at that pixel
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = pb + 16 * t + n;
        pok[t] = p < q.total;
        const int pc = pok[t] ? p : 0, im = pc / q.HW, r = pc - im * q.HW;
        xoff[t] = im * q.CB * q.HW + r;
        yoff[t] = (int64_t)im * q.O * q.HW + r;
    }
    const u32x4 fill = u32x4{0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u}, zero = u32x4{0u, 0u, 0u, 0u};
    // the B operand of k-step s at N tile t: a pixel past the batch reads as codes 0, a padding slot as the zero byte
    auto load_b = [&](int s, int t) -> u32x4 {
        const uint32_t sl = tab[q.slot_off + 4 * s + kq];
        if (sl & PADSLOT) return zero;
        return pok[t] ? x[xoff[t] + (int)((sl >> 4) & 0xffffu) * q.HW] : fill;
    };
    const bool keep = mn_uniform((int)(q.nsteps <= 4 * F32_KEEP)) != 0;
    u32x4 breg[F32_KEEP][4];
    int sa[4] = {0, 0, 0, 0};          // this wave's share of sum a at the pixel of N tile t; in wave 0, behind the first combine, the whole sum
    if (keep) {
#pragma unroll
        for (int ks = 0; ks < F32_KEEP; ++ks) {
            const int s = wave + 4 * ks;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                breg[ks][t] = s < q.nsteps ? load_b(s, t) : zero;
#pragma unroll
                for (int e = 0; e < 4; ++e) sa[t] = bytesum(breg[ks][t][e], sa[t]);
            }
        }
    }
    bool first = true;          // sum a is formed (keep: combined) along with the first tile
    const int set0 = (int)blockIdx.y * q.spb;
    const int set1 = set0 + q.spb < q.nsets ? set0 + q.spb : q.nsets;
    for (int set = set0; set < set1; ++set) {
        const int cnt = (int)tab[q.cnt_off + set];
        const int nt = mn_uniform(cnt < q.slots ? cnt : q.slots);
        for (int i = 0; i < nt; ++i) {
            const uint32_t* tile = tab + q.tiles_off + (int64_t)(set * q.slots + i) * q.tstride;
            const uint32_t* ap = tile + THDR + lane * 4;
            i32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = i32x4{0, 0, 0, 0};
            if (keep) {
#pragma unroll
                for (int ks = 0; ks < F32_KEEP; ++ks) {
                    const int s = wave + 4 * ks;
                    if (s < q.nsteps) {
                        const u32x4 a = *reinterpret_cast<const u32x4*>(ap + s * STEPW);
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc[t] = mn_mfma_i8(a, breg[ks][t], acc[t]);
                    }
                }
            } else {
#pragma unroll 1
                for (int s = wave; s < q.nsteps; s += 4) {
                    const u32x4 a = *reinterpret_cast<const u32x4*>(ap + s * STEPW);
                    u32x4 b[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) b[t] = load_b(s, t);
                    if (first) {
#pragma unroll
                        for (int t = 0; t < 4; ++t)
#pragma unroll
                            for (int e = 0; e < 4; ++e) sa[t] = bytesum(b[t][e], sa[t]);
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = mn_mfma_i8(a, b[t], acc[t]);
                }
            }
            if (first) {          // the four kq lanes of a pixel hold the four quarters of every k-step
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    sa[t] += __shfl_xor(sa[t], 16, 64);
                    sa[t] += __shfl_xor(sa[t], 32, 64);
                }
            }
            if (wave) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    s_acc[wave - 1][t][lane] = acc[t];
                    if (first && kq == 0) s_sa[wave - 1][t][n] = sa[t];
                }
            }
            __syncthreads();
            if (wave == 0) {
                // the lane's rows 4 kq .. 4 kq + 3 of the tile (D[row = 4 kq + reg][col = n])
                const f32x4 alpha = *reinterpret_cast<const f32x4*>(tile + T_CH + 4 * kq), bias = *reinterpret_cast<const f32x4*>(tile + T_CH + 16 + 4 * kq);
                const i32x4 kc = *reinterpret_cast<const i32x4*>(tile + T_KC + 4 * kq);
                const i32x4 ds = *reinterpret_cast<const i32x4*>(tile + T_DEST + 4 * kq);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    u32x4 sum = u32x4{(uint32_t)acc[t][0], (uint32_t)acc[t][1], (uint32_t)acc[t][2], (uint32_t)acc[t][3]};
#pragma unroll
                    for (int w = 0; w < 3; ++w) {
                        const i32x4 part = s_acc[w][t][lane];
#pragma unroll
                        for (int r = 0; r < 4; ++r) sum[r] += (uint32_t)part[r];
                        if (first) sa[t] += s_sa[w][t][n];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = set * SETROWS + ds[r];          // (a null out_order: position = channel)
                        if (ds[r] < 0 || ds[r] >= SETROWS || o >= q.O || !pok[t]) continue;
                        const int full = (int)(2u * sum[r] + (uint32_t)sa[t] + (uint32_t)kc[r]);
                        y[yoff[t] + (int64_t)o * q.HW] = (float)full * alpha[r] + bias[r];
                    }
                }
            }
            first = false;
            __syncthreads();          // the partials are consumed before the next tile's are written
        }
    }
}

static inline bool make_geom_f32(const mn_conv_geom* g, W8Geom& m) {
    return make_geom(g, 8, 8, 8, m) && m.KS == 1 && m.groups == 1;
}

}  // namespace mn_code8

extern "C" int mn_code8conv_f32_supported(const mn_conv_geom* g) {
    mn_code8::W8Geom m;
    return mn_code8::make_geom_f32(g, m) ? 1 : 0;
}

extern "C" int mn_code8conv_fwd_f32(const mn_conv_geom* g, const uint32_t* table, const int8_t* in_codes, float* y, mn_stream_t stream) {
    mn_code8::W8Geom m;
    if (!table || !in_codes || !y || !aligned16(table) || !aligned16(in_codes) || (((uintptr_t)y) & 3) || !tile_geom_valid(g))
        MN_FAIL(MN_EINVAL, "mn_code8conv_fwd_f32: null / unaligned argument (table and map are 16-byte aligned) or invalid geometry");
    if (!mn_code8::make_geom_f32(g, m))
        MN_FAIL(MN_ENOTSUP, "mn_code8conv_fwd_f32: geometry not covered (1x1 / stride 1 / padding 0 / groups 1 on 8-bit codes and weights, C <= 33025)");
    mn_code8::W8F32 f;
    f.total = m.N * m.H * m.W; f.HW = m.H * m.W; f.CB = m.CB; f.O = m.O; f.nsteps = m.nsteps; f.nsets = m.nsets; f.slots = m.slots; f.tstride = m.tstride;
    f.slot_off = m.slot_off; f.cnt_off = m.cnt_off; f.tiles_off = m.tiles_off;
    const int bx = (f.total + 63) / 64;          // 64 pixels per block: four N tiles, K split over the four waves
    const dim3 grid(bx, mn_sets::grid_deal(bx, m.nsets, f.spb));          // the sets over grid.y
    const hipStream_t s = (hipStream_t)stream;
    mn_set_last_kernel("k_code8conv_f32");
    mn_prof_bytes(16.0 * m.N * m.CB * f.HW + 4.0 * m.N * m.O * f.HW + 4.0 * (double)mn_code8::table_words(m));
    mn_prof_begin(s);
    hipLaunchKernelGGL(mn_code8::k_code8conv_f32, grid, dim3(256), 0, s, table, reinterpret_cast<const u32x4*>(in_codes), y, f);
    mn_prof_end(s);
    MN_CHECK_LAUNCH("mn_code8conv_fwd_f32");
    return MN_OK;
}
