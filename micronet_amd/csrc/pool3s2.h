// max_pool2d(kernel 3, stride 2, padding 1, dilation 1, floor mode) for gfx950: the two pools of the reference's plain nin (models/nin.py), forward and backward,
// on fp32 maps (k_pool3_f32_*<0>), fused with the IAO activation quantizer (k_pool3_f32_*<1>: max_pool2d(Q(x)), Q(x) never written) and on int8 sign codes
// (k_pool3_sign8_*).  Map [planes][H][W] -> [planes][Ho][Wo], Ho = (H - 1) / 2 + 1: window (oh, ow) covers rows 2 oh - 1 .. 2 oh + 1 and columns 2 ow - 1 .. 2 ow + 1,
// cells outside the map are never candidates; scan row-major, a later cell replaces the maximum iff v > m || v != v (ATen's rule, k_pool2_f32_fwd's).
//
// Work split: a 256-thread block takes one TILE at a time -- a run of `ppt` whole planes while a plane has at most P3_TILE elements (4 planes of 32 x 32, 16 of
// 16 x 16), else a band of R output rows of one plane with its halo (P3Geom).  The tile's input is one contiguous span of global memory: it is staged into LDS once
// with whole 16-byte loads (p3_stage; the span keeps its 16-byte phase in LDS, so a base that is not aligned or a W that is no multiple of 4 costs scalar loads for the
// first and last vector only), every cell is then read by its up to four windows from LDS instead of 2.25 x from global memory.
//   forward : thread = 4 consecutive outputs of a row: 3 rows x 9 staged columns, values and argmax bytes (0..8 in the unclipped window) stored whole.
//   backward: a GATHER -- an input cell lies in at most 2 x 2 windows; the block stages the tile's gy and argmax bytes, thread = 4 consecutive input cells of a row:
//             6 windows, summed in window order (oh, ow ascending), one 16-byte dx store.  Every dx element is written once: no atomics, no zero fill.
// The sign form keeps no argmax: its backward stages the input codes and recomputes every window's winner (first +1 in scan order, else the first in-map cell).
#pragma once
#include "common.h"

#include <math.h>

#define P3_TILE 4096          // elements of the map staged per tile (16 KB of fp32)
#define P3_SLACK 32           // elements behind them: the 16-byte phase of the span (<= 15) + the 8-column row read of the last quad

struct P3Geom {
    int H, W, Ho, Wo;
    int ppt;                  // whole planes per tile (1 in band mode)
    int R, bands;             // output rows per band, bands per plane (whole planes: R = Ho, bands = 1)
    int64_t planes, tiles;
};
// Every H, W >= 1 whose plane fits a tile; beyond that a band needs 2 R + 3 input rows (the sign backward: the windows of R + 1 output rows) of a tile: W <= P3_TILE / 5.
static inline int p3_geom(int64_t planes, int64_t H, int64_t W, P3Geom* g) {
    if (planes <= 0 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return 0;
    g->H = (int)H; g->W = (int)W; g->Ho = (int)((H - 1) / 2 + 1); g->Wo = (int)((W - 1) / 2 + 1); g->planes = planes;
    if (H * W <= P3_TILE) {
        g->ppt = (int)(P3_TILE / (H * W)); g->R = g->Ho; g->bands = 1;
        g->tiles = (planes + g->ppt - 1) / g->ppt;
    } else {
        if (5 * W > P3_TILE) return 0;
        g->ppt = 1; g->R = (int)((P3_TILE / W - 3) / 2); g->bands = (g->Ho + g->R - 1) / g->R;
        g->tiles = planes * g->bands;
    }
    return 1;
}
static inline int p3_grid(const P3Geom& g) { return mn_grid_for(g.tiles, 1, 8192); }

struct P3Tile { int64_t p0; int np, r0, nr; };          // planes p0 .. p0 + np, output rows r0 .. r0 + nr
__device__ __forceinline__ P3Tile p3_tile(const P3Geom& g, int64_t t) {
    P3Tile tl;
    if (g.bands == 1) {
        tl.p0 = t * g.ppt; tl.r0 = 0; tl.nr = g.Ho;
        const int64_t left = g.planes - tl.p0;
        tl.np = left < g.ppt ? (int)left : g.ppt;
    } else {
        tl.p0 = t / g.bands; tl.np = 1;
        tl.r0 = (int)(t - tl.p0 * g.bands) * g.R;
        tl.nr = g.Ho - tl.r0 < g.R ? g.Ho - tl.r0 : g.R;
    }
    return tl;
}

// n elements from src into s, element e at s[lead + e] with lead = the span's phase inside its first 16-byte vector: vectors that lie inside the span move whole,
// the first and last one element-wise.  `f` maps every element on the way (the quantizer of the fused form).  Returns lead.
struct P3Id { template <typename U> __device__ __forceinline__ void operator()(U&) const {} };
struct P3Fq {
    float sc, zp, qmin, qmax;
    __device__ __forceinline__ void operator()(float& v) const { v = iao_fq(v, sc, zp, qmin, qmax); }
    __device__ __forceinline__ void operator()(float4& q) const { (*this)(q.x); (*this)(q.y); (*this)(q.z); (*this)(q.w); }
};
template <typename T, typename F>
__device__ __forceinline__ int p3_stage(const T* __restrict__ src, int n, T* s, const F& f) {
    constexpr int V = 16 / (int)sizeof(T);
    const int lead = (int)((((uintptr_t)src) / sizeof(T)) & (uintptr_t)(V - 1));
    const int nv = (lead + n + V - 1) / V;
    for (int v = threadIdx.x; v < nv; v += 256) {
        const int e0 = v * V - lead;
        if (e0 >= 0 && e0 + V <= n) {
            float4 q = *reinterpret_cast<const float4*>(src + e0);
            f(q);
            *reinterpret_cast<float4*>(s + v * V) = q;
        } else {
            for (int k = 0; k < V; ++k) {
                const int e = e0 + k;
                if (e >= 0 && e < n) { T a = src[e]; f(a); s[v * V + k] = a; }
            }
        }
    }
    return lead;
}

// ---------------------------------------------------------------- fp32 (FQ = 1: of the fake-quantised input)
// mm != NULL (FQ): per-block (min, max) of y, mm[block] / mm[grid + block], for mn_iao_observe_partials.
template <int FQ>
__global__ __launch_bounds__(256) void k_pool3_f32_fwd(const float* __restrict__ x, float* __restrict__ y, unsigned char* __restrict__ idx, const P3Geom g,
                                                       const float* __restrict__ qp, float qmin, float qmax, float* __restrict__ mm) {
    __shared__ float4 s4[(P3_TILE + P3_SLACK) / 4];
    __shared__ float scf[16];
    float* s = reinterpret_cast<float*>(s4);
    P3Fq fq = {1.f, 0.f, qmin, qmax};
    if (FQ) { fq.sc = qp[0]; fq.zp = qp[1]; }
    const int H = g.H, W = g.W, Ho = g.Ho, Wo = g.Wo, nq = (Wo + 3) >> 2;
    float mlo = INFINITY, mhi = -INFINITY;
    for (int64_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const P3Tile tl = p3_tile(g, t);
        // staged input rows ir0 .. ir0 + rows of every plane of the tile (whole planes: all H)
        const int ir0 = tl.r0 > 0 ? 2 * tl.r0 - 1 : 0, ir1 = 2 * (tl.r0 + tl.nr) < H ? 2 * (tl.r0 + tl.nr) : H, rows = ir1 - ir0;
        const float* src = x + (tl.p0 * H + ir0) * W;
        const int n = tl.np * rows * W;
        int lead;
        if (FQ) lead = p3_stage(src, n, s, fq); else lead = p3_stage(src, n, s, P3Id());
        __syncthreads();
        const bool vrow = lead == 0 && (W & 3) == 0;          // every staged row starts on a 16-byte boundary of LDS
        const int items = tl.np * tl.nr * nq;
        for (int it = threadIdx.x; it < items; it += 256) {
            const int rowid = it / nq, qc = it - rowid * nq, q = rowid / tl.nr, oh = tl.r0 + (rowid - q * tl.nr);
            const int c0 = 8 * qc;                              // the quad's windows cover columns c0 - 1 .. c0 + 7
            float m[4];
            uint32_t k[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { m[j] = -INFINITY; k[j] = (oh == 0 ? 3u : 0u) + ((qc | j) == 0 ? 1u : 0u); }          // the first in-map cell
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int ih = 2 * oh - 1 + kh;
                if (ih < 0 || ih >= H) continue;
                const float* row = s + lead + (q * rows + ih - ir0) * W;
                float v[9];
                v[0] = c0 > 0 ? row[c0 - 1] : 0.f;
                if (vrow) {          // (may run past the row's end into the next row or the slack: masked below)
                    const float4 a = *reinterpret_cast<const float4*>(row + c0), b = *reinterpret_cast<const float4*>(row + c0 + 4);
                    v[1] = a.x; v[2] = a.y; v[3] = a.z; v[4] = a.w; v[5] = b.x; v[6] = b.y; v[7] = b.z; v[8] = b.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[1 + e] = c0 + e < W ? row[c0 + e] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const int col = c0 + 2 * j - 1 + kw;
                        const float a = v[2 * j + kw];
                        if (col >= 0 && col < W && (a > m[j] || a != a)) { m[j] = a; k[j] = (uint32_t)(kh * 3 + kw); }
                    }
            }
            const int64_t oo = ((tl.p0 + q) * Ho + oh) * Wo + 4 * qc;
            if (4 * qc + 3 < Wo && aligned16(y + oo)) *reinterpret_cast<float4*>(y + oo) = make_float4(m[0], m[1], m[2], m[3]);
            else for (int j = 0; j < 4; ++j) if (4 * qc + j < Wo) y[oo + j] = m[j];
            if (4 * qc + 3 < Wo && (((uintptr_t)(idx + oo)) & 3) == 0) *reinterpret_cast<uint32_t*>(idx + oo) = k[0] | (k[1] << 8) | (k[2] << 16) | (k[3] << 24);
            else for (int j = 0; j < 4; ++j) if (4 * qc + j < Wo) idx[oo + j] = (unsigned char)k[j];
            if (FQ) for (int j = 0; j < 4; ++j) if (4 * qc + j < Wo) { mlo = OpMinF()(mlo, m[j]); mhi = OpMaxF()(mhi, m[j]); }
        }
        __syncthreads();          // the next tile overwrites the staged rows
    }
    if (FQ && mm) {
        mlo = block_reduce(mlo, OpMinF(), INFINITY, scf);
        mhi = block_reduce(mhi, OpMaxF(), -INFINITY, scf);
        if (threadIdx.x == 0) { mm[blockIdx.x] = mlo; mm[gridDim.x + blockIdx.x] = mhi; }
    }
}

// One row of windows (kb = 3 * (the cell row's position in those windows)) into the four cells j0 .. j0 + 3: window columns
// w0 = j0 / 2 .. w0 + 2; an even cell is the centre of one window, an odd cell the right edge of one and the left edge of the next.
// gv / kv: gradient and argmax byte of the three windows (255: no such window).
__device__ __forceinline__ void p3_gather_row(const float (&gv)[3], const uint32_t (&kv)[3], uint32_t kb, float (&acc)[4]) {
    acc[0] += kv[0] == kb + 1u ? gv[0] : 0.f;
    acc[1] += kv[0] == kb + 2u ? gv[0] : 0.f;
    acc[1] += kv[1] == kb ? gv[1] : 0.f;
    acc[2] += kv[1] == kb + 1u ? gv[1] : 0.f;
    acc[3] += kv[1] == kb + 2u ? gv[1] : 0.f;
    acc[3] += kv[2] == kb ? gv[2] : 0.f;
}
// The backward tile of output rows r0 .. r0 + nr owns input rows 2 r0 .. 2 (r0 + nr) and stages one output row more: the lower windows of its last odd row.
// FQ: dx = clip-STE of the quantizer at x [* the mask [x > 0] of the ReLU in front, relu_mask] of the gathered gradient.
template <int FQ>
__global__ __launch_bounds__(256) void k_pool3_f32_bwd(const float* __restrict__ gy, const unsigned char* __restrict__ idx, const float* __restrict__ x,
                                                       float* __restrict__ dx, const P3Geom g, const float* __restrict__ qp, float qmin, float qmax, int relu_mask) {
    __shared__ float4 sg4[(P3_TILE + P3_SLACK) / 4];
    __shared__ float4 sk4[(P3_TILE + P3_SLACK) / 16];
    float* sg = reinterpret_cast<float*>(sg4);
    unsigned char* sk = reinterpret_cast<unsigned char*>(sk4);
    float sc = 1.f, zp = 0.f, lo = 0.f, hi = 0.f;
    if (FQ) { sc = qp[0]; zp = qp[1]; lo = qp[2]; hi = qp[3]; }
    const int H = g.H, W = g.W, Ho = g.Ho, Wo = g.Wo, nq = (W + 3) >> 2;
    for (int64_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const P3Tile tl = p3_tile(g, t);
        const int r1 = tl.r0 + tl.nr + 1 < Ho ? tl.r0 + tl.nr + 1 : Ho, orows = r1 - tl.r0;
        const int i0 = 2 * tl.r0, i1 = 2 * (tl.r0 + tl.nr) < H ? 2 * (tl.r0 + tl.nr) : H;
        const int64_t so = (tl.p0 * Ho + tl.r0) * Wo;
        const int n = tl.np * orows * Wo;
        const int lg = p3_stage(gy + so, n, sg, P3Id()), lk = p3_stage(idx + so, n, sk, P3Id());
        __syncthreads();
        const int items = tl.np * (i1 - i0) * nq;
        for (int it = threadIdx.x; it < items; it += 256) {
            const int rowid = it / nq, qc = it - rowid * nq, q = rowid / (i1 - i0), i = i0 + (rowid - q * (i1 - i0));
            const int olo = i >> 1, w0 = 2 * qc;                // cell row i: centre of window row i / 2 (even), bottom of (i - 1) / 2 and top of (i + 1) / 2 (odd)
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int r = 0; r < 2; ++r) {
                const int oh = olo + r;
                if (r == 1 && (!(i & 1) || oh >= Ho)) break;
                const int ro = (q * orows + oh - tl.r0) * Wo + w0;
                float gv[3];
                uint32_t kv[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { const bool in = w0 + c < Wo; gv[c] = in ? sg[lg + ro + c] : 0.f; kv[c] = in ? (uint32_t)sk[lk + ro + c] : 255u; }
                p3_gather_row(gv, kv, r ? 0u : ((i & 1) ? 6u : 3u), acc);
            }
            const int64_t xo = ((tl.p0 + q) * H + i) * W + 4 * qc;
            const bool whole = 4 * qc + 3 < W && aligned16(dx + xo);
            if (FQ) {
                float xv[4] = {0.f, 0.f, 0.f, 0.f};
                if (whole && aligned16(x + xo)) { const float4 a = *reinterpret_cast<const float4*>(x + xo); xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w; }
                else for (int j = 0; j < 4; ++j) if (4 * qc + j < W) xv[j] = x[xo + j];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[j] = iao_fq_grad(acc[j], xv[j], sc, zp, lo, hi, qmin, qmax);
                    if (relu_mask) acc[j] = xv[j] > 0.f ? acc[j] : 0.f;
                }
            }
            if (whole) *reinterpret_cast<float4*>(dx + xo) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            else for (int j = 0; j < 4; ++j) if (4 * qc + j < W) dx[xo + j] = acc[j];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- int8 sign codes (+1 = 0x01, -1 = 0xFF): one byte per element both ways
// The maximum of +-1 codes is +1 unless every in-map cell of the window is -1.  Thread = 4 consecutive outputs, one 4-byte store.
#ifdef P3_SIGN_FORM          // (plain kernels, no templates: defined by the one translation unit that launches them, norm_kernels.hip)
__global__ __launch_bounds__(256) void k_pool3_sign8_fwd(const signed char* __restrict__ a, signed char* __restrict__ out, const P3Geom g) {
    __shared__ float4 s4[(P3_TILE + P3_SLACK) / 16];
    signed char* s = reinterpret_cast<signed char*>(s4);
    const int H = g.H, W = g.W, Ho = g.Ho, Wo = g.Wo, nq = (Wo + 3) >> 2;
    for (int64_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const P3Tile tl = p3_tile(g, t);
        const int ir0 = tl.r0 > 0 ? 2 * tl.r0 - 1 : 0, ir1 = 2 * (tl.r0 + tl.nr) < H ? 2 * (tl.r0 + tl.nr) : H, rows = ir1 - ir0;
        const int lead = p3_stage(a + (tl.p0 * H + ir0) * W, tl.np * rows * W, s, P3Id());
        __syncthreads();
        const int items = tl.np * tl.nr * nq;
        for (int it = threadIdx.x; it < items; it += 256) {
            const int rowid = it / nq, qc = it - rowid * nq, q = rowid / tl.nr, oh = tl.r0 + (rowid - q * tl.nr);
            const int c0 = 8 * qc;
            uint32_t pos = 0u;                                   // bit e: column c0 - 1 + e holds a +1 in one of the window's in-map rows
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int ih = 2 * oh - 1 + kh;
                if (ih < 0 || ih >= H) continue;
                const signed char* row = s + lead + (q * rows + ih - ir0) * W;
#pragma unroll
                for (int e = 0; e < 9; ++e) { const int col = c0 - 1 + e; if (col >= 0 && col < W && row[col] >= 0) pos |= 1u << e; }
            }
            uint32_t o = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) o |= (((pos >> (2 * j)) & 7u) ? 0x01u : 0xFFu) << (8 * j);
            const int64_t oo = ((tl.p0 + q) * Ho + oh) * Wo + 4 * qc;
            if (4 * qc + 3 < Wo && (((uintptr_t)(out + oo)) & 3) == 0) *reinterpret_cast<uint32_t*>(out + oo) = o;
            else for (int j = 0; j < 4; ++j) if (4 * qc + j < Wo) out[oo + j] = (signed char)(o >> (8 * j));
        }
        __syncthreads();
    }
}
// The argmax byte of window (oh, ow) from the staged codes of its plane (`pl`: row ir0 of the plane): the first +1 in scan order, else the first in-map cell.
__device__ __forceinline__ uint32_t p3_sign_winner(const signed char* pl, int ir0, int oh, int ow, int H, int W) {
    uint32_t k = (oh == 0 ? 3u : 0u) + (ow == 0 ? 1u : 0u);
    bool found = false;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int ih = 2 * oh - 1 + kh;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int iw = 2 * ow - 1 + kw;
            if (!found && ih >= 0 && ih < H && iw >= 0 && iw < W && pl[(ih - ir0) * W + iw] >= 0) { found = true; k = (uint32_t)(kh * 3 + kw); }
        }
    }
    return k;
}
// backward: the tile of k_pool3_f32_bwd; instead of argmax bytes it stages the input rows its (nr + 1) rows of windows read and recomputes the winners.
__global__ __launch_bounds__(256) void k_pool3_sign8_bwd(const float* __restrict__ gy, const signed char* __restrict__ a, float* __restrict__ dx, const P3Geom g) {
    __shared__ float4 sg4[(P3_TILE + P3_SLACK) / 4];
    __shared__ float4 sa4[(P3_TILE + P3_SLACK) / 16];
    float* sg = reinterpret_cast<float*>(sg4);
    signed char* sa = reinterpret_cast<signed char*>(sa4);
    const int H = g.H, W = g.W, Ho = g.Ho, Wo = g.Wo, nq = (W + 3) >> 2;
    for (int64_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const P3Tile tl = p3_tile(g, t);
        const int r1 = tl.r0 + tl.nr + 1 < Ho ? tl.r0 + tl.nr + 1 : Ho, orows = r1 - tl.r0;
        const int i0 = 2 * tl.r0, i1 = 2 * (tl.r0 + tl.nr) < H ? 2 * (tl.r0 + tl.nr) : H;
        const int ir0 = tl.r0 > 0 ? 2 * tl.r0 - 1 : 0, ir1 = 2 * r1 < H ? 2 * r1 : H, rows = ir1 - ir0;
        const int lg = p3_stage(gy + (tl.p0 * Ho + tl.r0) * Wo, tl.np * orows * Wo, sg, P3Id());
        const int la = p3_stage(a + (tl.p0 * H + ir0) * W, tl.np * rows * W, sa, P3Id());
        __syncthreads();
        const int items = tl.np * (i1 - i0) * nq;
        for (int it = threadIdx.x; it < items; it += 256) {
            const int rowid = it / nq, qc = it - rowid * nq, q = rowid / (i1 - i0), i = i0 + (rowid - q * (i1 - i0));
            const int olo = i >> 1, w0 = 2 * qc;
            const signed char* pl = sa + la + q * rows * W;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int r = 0; r < 2; ++r) {
                const int oh = olo + r;
                if (r == 1 && (!(i & 1) || oh >= Ho)) break;
                const int ro = (q * orows + oh - tl.r0) * Wo + w0;
                float gv[3];
                uint32_t kv[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { const bool in = w0 + c < Wo; gv[c] = in ? sg[lg + ro + c] : 0.f; kv[c] = in ? p3_sign_winner(pl, ir0, oh, w0 + c, H, W) : 255u; }
                p3_gather_row(gv, kv, r ? 0u : ((i & 1) ? 6u : 3u), acc);
            }
            const int64_t xo = ((tl.p0 + q) * H + i) * W + 4 * qc;
            if (4 * qc + 3 < W && aligned16(dx + xo)) *reinterpret_cast<float4*>(dx + xo) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            else for (int j = 0; j < 4; ++j) if (4 * qc + j < W) dx[xo + j] = acc[j];
        }
        __syncthreads();
    }
}
#endif
