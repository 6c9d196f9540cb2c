// The fused k-bit block of qact_kernels.hip through a 3x3 / stride 2 / padding 1 max-pool (floor mode; the two pools of the reference's plain nin, models/nin.py):
//   forward   k_qa3_fwd  stash / y -> a = relu(bn(y)) -> 3x3/2 max -> code of the next quantizer (1 B per POOLED element) or the pooled fp32 activation
//   backward  k_qa3_bwd  (pooled dq, stash) -> dz through the windows' first maxima -> sum dz, sum dz zhat (APPLY 0)  /  dy = gi (dz - k1 - zhat k2) (APPLY 1)
// Included by qact_kernels.hip behind its QaGeom / qa_load8 / QA_MAXTHR; semantics of the POOL 1 kernels there with the window changed: Ho = H / 2, Wo = W / 2, padded
// cells are never candidates, the winner is the first maximum in row-major scan order (v > m || v != v), an input element receives the gradient of every window it wins
// (up to four), summed in ascending (oh, ow) order.
//
// The windows overlap, so this is no streaming kernel: the grid stays (C, S), and a 256-thread block walks TILES of channel c -- ppt = P3_TILE / (H W) whole planes of
// consecutive images (4 of 32 x 32, 16 of 16 x 16; H even, W % 8 == 0, H W <= P3_TILE: only the top row and left column of windows are clipped).  g.n8 counts tiles.
//   stage    a thread owns up to two RUNS of 8 consecutive elements (run r = tid + 256 j at tile offset 8 r: one 16-byte load of a 16-bit stash), evaluates the chain
//            once per element and writes a (the integer-threshold forward: flip * acc) to the fp32 LDS tile; the backward keeps z and zhat of its runs in registers.
//   forward  thread = 4 consecutive windows of a pooled row: 3 rows x 9 LDS columns, one dword of codes / one float4 stored.
//   backward winner pre-pass: thread = the same 4 windows, finds each winner ONCE, writes its position byte (kh * 3 + kw) and d = quant ? clip-STE core of dq : dq to
//            LDS; then thread = its own runs again: 2 x 5 windows cover the 8 cells (p3_gather_row twice per window row), the cell's own masks (z > 0, the clamp
//            test of qa_dz_m) are applied to the sum.  Every dy element is written once: no atomics, no zero fill.
// A thread's run and window coordinates do not depend on the tile, so the divisions are done once per kernel.
#pragma once
#include "pool3s2.h"          // P3_TILE, p3_gather_row

struct Qa3Map {
    int ppt, Ho, Wo;
    int rq[2], ro[2], ri[2], rc[2];          // run j: plane of the tile, element offset in the plane, row, 8-column group
    int wq, wh, wc;                          // window quad: plane of the tile, pooled row, quad of the row
};
__device__ __forceinline__ Qa3Map qa3_map(const QaGeom& g) {
    Qa3Map m;
    m.ppt = P3_TILE / g.HW; m.Ho = g.H >> 1; m.Wo = g.W >> 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t r = threadIdx.x + 256u * j, q = fd_div(r, g.fd_hw8), o8 = r - q * (uint32_t)g.HW8, i = fd_div(o8, g.fd_w8);
        m.rq[j] = (int)q; m.ro[j] = (int)o8 * 8; m.ri[j] = (int)i; m.rc[j] = (int)(o8 - i * (uint32_t)g.W8);
    }
    const uint32_t rowid = fd_div(threadIdx.x, g.fd_w8);
    m.wc = (int)(threadIdx.x - rowid * (uint32_t)g.W8); m.wq = (int)rowid / m.Ho; m.wh = (int)rowid - m.wq * m.Ho;
    return m;
}
__device__ __forceinline__ int64_t qa3_plane(const QaGeom& g, int c, int64_t n) { return n * g.C + c; }
// The quad's four windows from the staged tile: m = the maximum, kx = its position byte (the first in-map cell if nothing replaces -inf: cannot happen behind a ReLU).
__device__ __forceinline__ void qa3_scan(const float* pl, int W, int oh, int qc, float (&m)[4], uint32_t (&kx)[4]) {
    const int c0 = 8 * qc;
#pragma unroll
    for (int j = 0; j < 4; ++j) { m[j] = -INFINITY; kx[j] = (oh == 0 ? 3u : 0u) + ((qc | j) == 0 ? 1u : 0u); }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int ih = 2 * oh - 1 + kh;          // (<= H - 1: H is even)
        if (ih < 0) continue;
        const float* row = pl + ih * W + c0;
        const float4 a = *reinterpret_cast<const float4*>(row), b = *reinterpret_cast<const float4*>(row + 4);
        const float v[9] = {c0 > 0 ? row[-1] : 0.f, a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const float x = v[2 * j + kw];
                if ((2 * j + kw > 0 || c0 > 0) && (x > m[j] || x != x)) { m[j] = x; kx[j] = (uint32_t)(kh * 3 + kw); }
            }
    }
}

template <int IN, int OUT>
__global__ __launch_bounds__(256) void k_qa3_fwd(const QaGeom g, const void* __restrict__ in, const float* __restrict__ chan, unsigned char* __restrict__ codes,
                                                 float* __restrict__ af) {
    __shared__ float4 s4[P3_TILE / 4];
    __shared__ float thr[QA_MAXTHR + 1];
    float* s = reinterpret_cast<float*>(s4);
    const int c = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
    const QaCh k = qa_load_ch(chan, g.C, c);
    // the integer-threshold forward of k_qa_fwd (block-uniform): the tile holds u = flip * acc, the window's largest activation is the one with the largest u
    const bool ithr = !IN && !OUT && g.nthr > 0 && qa_chan_finite(k);
    float flip = 1.f, T[QA_MAXTHR];
    if (ithr) {
        flip = qa_flip_of(k, g.s);
        if ((int)threadIdx.x < g.nthr) thr[threadIdx.x] = (float)qa_threshold_of(k, g.s, flip, threadIdx.x + 1u);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < QA_MAXTHR; ++q) T[q] = q < g.nthr ? thr[q] : 40000.f;
    }
    const Qa3Map mp = qa3_map(g);
    for (int64_t t = sp; t < g.n8; t += S) {
        const int64_t n0 = t * mp.ppt;
        const int np = g.N - n0 < mp.ppt ? (int)(g.N - n0) : mp.ppt;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (mp.rq[j] >= np) continue;
            float v[8], a[8];
            qa_load8<IN>(in, qa3_plane(g, c, n0 + mp.rq[j]) * g.HW + mp.ro[j], v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (ithr) a[e] = v[e] * flip;
                else { float zh, z; qa_eval<IN>(v[e], k, zh, z); a[e] = qa_relu(z); }
            }
            float* d = s + mp.rq[j] * g.HW + mp.ro[j];
            *reinterpret_cast<float4*>(d) = make_float4(a[0], a[1], a[2], a[3]);
            *reinterpret_cast<float4*>(d + 4) = make_float4(a[4], a[5], a[6], a[7]);
        }
        __syncthreads();
        if (mp.wq < np) {
            float m[4];
            uint32_t kx[4];
            qa3_scan(s + mp.wq * g.HW, g.W, mp.wh, mp.wc, m, kx);
            const int64_t po = qa3_plane(g, c, n0 + mp.wq) * (g.HW >> 2) + mp.wh * mp.Wo + 4 * mp.wc;
            if (OUT) *reinterpret_cast<float4*>(af + po) = make_float4(m[0], m[1], m[2], m[3]);
            else {
                uint32_t w4 = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint32_t code = 0u;
                    if (ithr) {
#pragma unroll
                        for (int q = 0; q < QA_MAXTHR; ++q) if (q < 3 || g.nthr > 3) code += (m[j] >= T[q]) ? 1u : 0u;
                    } else code = qa_code(m[j], g.s);
                    w4 |= code << (8 * j);
                }
                *reinterpret_cast<uint32_t*>(codes + po) = w4;
            }
        }
        __syncthreads();          // the next tile overwrites the staged planes
    }
}

// APPLY 0: part[c][sp] = (sum dz, sum dz zhat) of this block's tiles (k_qa_partial's layout, read by k_qa_final_bwd / the folded finish below);
// APPLY 1: dy, with k_qa_apply's head (sums as finished values, or g.fin_part: every block finishes the partial rows itself, block sp == 0 writes the outputs).
template <int IN, int APPLY>
__global__ __launch_bounds__(256) void k_qa3_bwd(const QaGeom g, const void* __restrict__ in, const float* __restrict__ chan, const float* __restrict__ dq,
                                                 const float* __restrict__ sums, int training, int quant, float* __restrict__ dy, double* __restrict__ part) {
    __shared__ float4 sa4[P3_TILE / 4], sd4[P3_TILE / 16];          // a of the tile; d of its windows
    __shared__ uint32_t sk4[P3_TILE / 16];                          // winner position bytes of its windows
    __shared__ double scd[16];
    __shared__ float fs[2];
    const float* sa = reinterpret_cast<const float*>(sa4);
    const float* sd = reinterpret_cast<const float*>(sd4);
    const unsigned char* sk = reinterpret_cast<const unsigned char*>(sk4);
    const int c = blockIdx.x, sp = blockIdx.y, S = gridDim.y;
    const QaCh k = qa_load_ch(chan, g.C, c);
    float k1 = 0.f, k2 = 0.f;
    if (APPLY) {
        float s1f, s2f;
        if (g.fin_part) {          // (block-uniform)
            if (threadIdx.x == 0) {
                double sv[2] = {0.0, 0.0};
                mn_row_sums<2>(g.fin_part + (int64_t)c * g.fin_S * 2, g.fin_S, sv);
                fs[0] = (float)sv[0]; fs[1] = (float)sv[1];
                if (sp == 0) {
                    if (g.fin_dbeta) g.fin_dbeta[c] = fs[0];
                    if (g.fin_dgamma) g.fin_dgamma[c] = fs[1];
                    if (g.fin_sums) { g.fin_sums[c] = fs[0]; g.fin_sums[g.C + c] = fs[1]; }
                }
            }
            __syncthreads();
            s1f = fs[0]; s2f = fs[1];
        } else { s1f = sums[c]; s2f = sums[g.C + c]; }
        if (training) { const float n = (float)g.N * (float)g.HW; k1 = s1f / n; k2 = s2f / n; }
    }
    const Qa3Map mp = qa3_map(g);
    double s1 = 0.0, s2 = 0.0;
    for (int64_t t = sp; t < g.n8; t += S) {
        const int64_t n0 = t * mp.ppt;
        const int np = g.N - n0 < mp.ppt ? (int)(g.N - n0) : mp.ppt;
        float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (mp.wq < np) g4 = *reinterpret_cast<const float4*>(dq + qa3_plane(g, c, n0 + mp.wq) * (g.HW >> 2) + mp.wh * mp.Wo + 4 * mp.wc);
        float z[2][8], zh[2][8];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (mp.rq[j] >= np) continue;
            float v[8], a[8];
            qa_load8<IN>(in, qa3_plane(g, c, n0 + mp.rq[j]) * g.HW + mp.ro[j], v);
#pragma unroll
            for (int e = 0; e < 8; ++e) { qa_eval<IN>(v[e], k, zh[j][e], z[j][e]); a[e] = qa_relu(z[j][e]); }
            float4* d = sa4 + ((mp.rq[j] * g.HW + mp.ro[j]) >> 2);
            d[0] = make_float4(a[0], a[1], a[2], a[3]);
            d[1] = make_float4(a[4], a[5], a[6], a[7]);
        }
        __syncthreads();
        if (mp.wq < np) {          // window (wq, wh, 4 wc + j) is window 4 tid + j of the tile
            float m[4];
            uint32_t kx[4];
            qa3_scan(sa + mp.wq * g.HW, g.W, mp.wh, mp.wc, m, kx);
            const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
            float d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = quant ? dorefa_ste_core_m(gv[j], g.s, g.inv_s) : gv[j];
            sd4[threadIdx.x] = make_float4(d[0], d[1], d[2], d[3]);
            sk4[threadIdx.x] = kx[0] | (kx[1] << 8) | (kx[2] << 16) | (kx[3] << 24);
        }
        __syncthreads();          // (the next tile's stores to sa / sd lie behind its own barriers: two per tile are enough)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (mp.rq[j] >= np) continue;
            const int i = mp.ri[j], olo = i >> 1;
            float lo[4] = {0.f, 0.f, 0.f, 0.f}, hi[4] = {0.f, 0.f, 0.f, 0.f};
            for (int r = 0; r < 2; ++r) {          // cell row i: centre of window row i / 2 (even), bottom of (i - 1) / 2 and top of (i + 1) / 2 (odd)
                const int oh = olo + r;
                if (r == 1 && (!(i & 1) || oh >= mp.Ho)) break;
                const int w0 = (mp.rq[j] * mp.Ho + oh) * mp.Wo + 4 * mp.rc[j];          // the run's 8 cells lie in windows w0 .. w0 + 4 of this row
                const bool five = 4 * mp.rc[j] + 4 < mp.Wo;
                const float4 d4 = sd4[w0 >> 2];
                const uint32_t k4 = sk4[w0 >> 2];
                float ga[3] = {d4.x, d4.y, d4.z}, gb[3] = {d4.z, d4.w, five ? sd[w0 + 4] : 0.f};
                uint32_t ka[3] = {k4 & 255u, (k4 >> 8) & 255u, (k4 >> 16) & 255u}, kb[3] = {(k4 >> 16) & 255u, k4 >> 24, five ? (uint32_t)sk[w0 + 4] : 255u};
                const uint32_t kr = r ? 0u : ((i & 1) ? 6u : 3u);
                p3_gather_row(ga, ka, kr, lo);
                p3_gather_row(gb, kb, kr, hi);
            }
            const float acc[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            float o[8], t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {          // qa_dz_m's masks on the sum of the won windows' d
                const float tq = qa_relu(z[j][e]) * 0.1f;
                const float dz = (z[j][e] > 0.f && (!quant || (tq >= 0.f && tq <= 1.f))) ? acc[e] : 0.f;
                t1 += dz; t2 += dz * zh[j][e];
                o[e] = k.gi * (dz - k1 - zh[j][e] * k2);
            }
            if (APPLY) {
                float* d = dy + qa3_plane(g, c, n0 + mp.rq[j]) * g.HW + mp.ro[j];
                *reinterpret_cast<float4*>(d) = make_float4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<float4*>(d + 4) = make_float4(o[4], o[5], o[6], o[7]);
            } else { s1 += (double)t1; s2 += (double)t2; }
        }
    }
    if (!APPLY) {
        s1 = block_reduce(s1, OpAddD(), 0.0, scd);
        s2 = block_reduce(s2, OpAddD(), 0.0, scd);
        if (threadIdx.x == 0) { part[((int64_t)c * S + sp) * 2] = s1; part[((int64_t)c * S + sp) * 2 + 1] = s2; }
    }
}
