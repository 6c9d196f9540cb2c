// Dense 5 x 5 / stride 1 / padding 2 convolution on k-bit DoReFa activation codes for gfx950 (plain nin's 96 -> 192 layer behind the first max-pool, models/nin.py):
// the forward of the fused k-bit block (mn_qconv_bnq_fwd_stash) on v_mfma_i32_16x16x64_i8.
//
//   acc[n][o][oh][ow] = sum over (c, r, s) of (2 k[o][c][r][s] - n_w) * j[n][c][oh + r - 2][ow + s - 2]          (qgemm_codes.h:9; exact in int32)
//
// For a_bits, w_bits in 2 .. 7 both operands are signed bytes (j <= 127, |2k - n_w| <= 127): one MFMA chain, no correction term.  Included by qgemm_sign.hip.
//
//   tile      a 256-thread block owns <= 256 output pixels: NI whole images where H W <= 256, else a band of TH full-width rows of one image.  The tile's input with
//             its halo of 2 is staged ONCE as [chunk of 16 channels][image][PH = TH + 4 rows][PW = W + 4 columns] records of 16 bytes (the 16 channels of one pixel:
//             one ds_read_b128 = one operand fragment) and stays resident while the block walks its channel sets.  Halo columns are zeroed once; rows outside the
//             image and images past the batch are staged as zero bytes: padding is data (a zero code adds nothing), the K loop has no bounds test.
//   staging   a unit = (chunk, image, patch row, 4 columns): 16 dword loads (one per channel plane, 4 pixels each) -> v_perm_b32 transposition -> 4 records.
//   K order   slot = tap * nchunks + chunk; four slots (one per 16-lane group kg) make a k-step of 64, the last step is padded with zero WEIGHT slots.  The slot's
//             byte offset inside the patch (chunk image + (r PW + s) records) comes from a small LDS table, so a lane's operand address is base(pixel) + tab[4 ks + kg].
//   waves     wave w takes tile pixels 64 w .. 64 w + 63 (four 16-pixel fragments on the MFMA's row side) x a SET of NB 16-channel fragments: 4 NB accumulators
//             i32x4 live in registers across the whole K walk.  The weight bytes are packed once per call in fragment order [16-channel tile][k-step][lane][16]
//             (k_q5_pack) and read straight from L2 one k-step ahead: the K loop has no barrier.
//   epilogue  a lane ends with 4 consecutive pixels of one channel.  32-bit stash: one 16-byte store.  16-bit stash: lanes kg and kg ^ 1 swap halves (one
//             wave exchange of two dwords) so that each stores a 16-byte run of 8 pixels.
//   stats     sum acc and sum acc^2 per channel over the tile's valid pixels: lanes -> wave (two exchanges) -> LDS [wave] -> one thread per channel adds the four
//             waves in wave order into the block's running total; at the end part[(block * O + o) * 2 + {0, 1}] (the layout k_qa_stats_prep reads).  Integers
//             below 2^53 in doubles: exact, no atomics, bit-identical from run to run.
#pragma once

#define Q5_LDS_CAP (72 * 1024)          // two blocks per CU (160 KB of LDS)
#define Q5_MAXPARTS 512                 // blocks = statistics partials at most

struct Q5Params {
    const unsigned char* x;             // [N][C][H][W] activation codes
    const unsigned char* wpk;           // k_q5_pack
    void* stash;                        // [N][O][H][W] int16 / int32
    double* part;                       // [grid][O][2]
    int N, C, H, W, O, HW;
    int TH, NI, PH, PW, W4, tpi, ntiles, ipt, tpix;          // ipt: pixels per image of a tile (TH W), tpix = NI ipt
    int nchunks, nslots, nsteps, nsets, CS, nunits, out32;  // CS: bytes of one chunk image
    int off_tab, off_red, off_tot;      // LDS byte offsets behind the patch
    FastDiv fd_w4, fd_ph, fd_ni, fd_w, fd_ipt, fd_tpi;
};

// weight codes 2k - n_w = rint(w n_w) as signed bytes in fragment order: [tile = o / 16][ks][lane][e]: o = 16 tile + (lane & 15), slot = 4 ks + (lane >> 4),
// tap = slot / nchunks, c = 16 (slot % nchunks) + e; zero bytes for slots >= 25 nchunks and channels >= O (the padded last set)
__global__ __launch_bounds__(256) void k_q5_pack(const float* __restrict__ w, unsigned char* __restrict__ out, int O, int C, int nchunks, int nsteps, int ntile16, float wn) {
    const int gi = blockIdx.x * 256 + threadIdx.x;
    if (gi >= ntile16 * nsteps * 64) return;
    const int lane = gi & 63, t = gi >> 6, ks = t % nsteps, tile = t / nsteps;
    const int o = tile * 16 + (lane & 15), slot = 4 * ks + (lane >> 4);
    uint32_t d[4] = {0u, 0u, 0u, 0u};
    if (o < O && slot < 25 * nchunks) {
        const int tap = slot / nchunks, c0 = (slot - tap * nchunks) * 16;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int code = (int)rintf(w[((int64_t)o * C + c0 + e) * 25 + tap] * wn);
            d[e >> 2] |= ((uint32_t)code & 0xffu) << (8 * (e & 3));
        }
    }
    *reinterpret_cast<u32x4*>(out + (int64_t)gi * 16) = u32x4{d[0], d[1], d[2], d[3]};
}

template <int NB>
__global__ __launch_bounds__(256, 2) void k_q5_fwd(const Q5Params p) {
    HIP_DYNAMIC_SHARED(float, smem)
    unsigned char* patch = reinterpret_cast<unsigned char*>(smem);
    int* tab = reinterpret_cast<int*>(patch + p.off_tab);             // [4 nsteps] byte offset of a slot inside the patch
    double* red = reinterpret_cast<double*>(patch + p.off_red);      // [2][4 waves][16 NB][2]
    double* tot = reinterpret_cast<double*>(patch + p.off_tot);      // [nsets][16 NB][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = mn_uniform(tid >> 6), j = lane & 15, kg = lane >> 4;
    for (int i = tid; i < p.off_tab / 16; i += 256) *reinterpret_cast<u32x4*>(patch + 16 * i) = u32x4{0u, 0u, 0u, 0u};          // the halo columns stay zero
    for (int s = tid; s < 4 * p.nsteps; s += 256) {
        const int tap = s / p.nchunks, chunk = s - tap * p.nchunks, r = tap / 5;
        tab[s] = s < p.nslots ? chunk * p.CS + (r * p.PW + (tap - 5 * r)) * 16 : 0;          // (a padded slot meets zero weights: any valid address)
    }
    for (int i = tid; i < p.nsets * NB * 32; i += 256) tot[i] = 0.0;
    int abase[4];
#pragma unroll
    for (int mf = 0; mf < 4; ++mf) {
        int tp = wave * 64 + mf * 16 + j;
        tp = tp < p.tpix ? tp : 0;                                    // (pixels beyond the tile: a valid address, the result is dropped)
        const int img = (int)fd_div((uint32_t)tp, p.fd_ipt), rem = tp - img * p.ipt;
        const int row = (int)fd_div((uint32_t)rem, p.fd_w), col = rem - row * p.W;
        abase[mf] = ((img * p.PH + row) * p.PW + col) * 16;
    }
    int par = 0;
    for (int tile = (int)blockIdx.x; tile < p.ntiles; tile += (int)gridDim.x) {
        const int timg = (int)fd_div((uint32_t)tile, p.fd_tpi);
        const int n0 = timg * p.NI, oh0 = (tile - timg * p.tpi) * p.TH;
        __syncthreads();          // the previous tile has been read (first tile: the zero fill and the table are written)
        for (int u = tid; u < p.nunits; u += 256) {
            const int t1 = (int)fd_div((uint32_t)u, p.fd_w4), d = u - t1 * p.W4;
            const int t2 = (int)fd_div((uint32_t)t1, p.fd_ph), pr = t1 - t2 * p.PH;
            const int chunk = (int)fd_div((uint32_t)t2, p.fd_ni), img = t2 - chunk * p.NI;
            const int n = n0 + img, ih = oh0 - 2 + pr;
            uint32_t v[16];
#pragma unroll
            for (int cc = 0; cc < 16; ++cc) v[cc] = 0u;
            if (n < p.N && ih >= 0 && ih < p.H) {
                const uint32_t base = (uint32_t)((n * p.C + chunk * 16) * p.H + ih) * (uint32_t)p.W + (uint32_t)(4 * d);
#pragma unroll
                for (int cc = 0; cc < 16; ++cc) v[cc] = *reinterpret_cast<const uint32_t*>(p.x + base + (uint32_t)(cc * p.HW));
            }
            uint32_t o[4][4];          // [pixel][channel quad]: 4 channels x 4 pixels of bytes transposed (as k_qd_fwd8's staging)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t lo01 = mn_perm(v[4 * q + 1], v[4 * q], 0x05010400u), hi01 = mn_perm(v[4 * q + 1], v[4 * q], 0x07030602u);
                const uint32_t lo23 = mn_perm(v[4 * q + 3], v[4 * q + 2], 0x05010400u), hi23 = mn_perm(v[4 * q + 3], v[4 * q + 2], 0x07030602u);
                o[0][q] = mn_perm(lo23, lo01, 0x05040100u); o[1][q] = mn_perm(lo23, lo01, 0x07060302u);
                o[2][q] = mn_perm(hi23, hi01, 0x05040100u); o[3][q] = mn_perm(hi23, hi01, 0x07060302u);
            }
            unsigned char* dst = patch + chunk * p.CS + ((img * p.PH + pr) * p.PW + 2 + 4 * d) * 16;
#pragma unroll
            for (int px = 0; px < 4; ++px) *reinterpret_cast<u32x4*>(dst + 16 * px) = u32x4{o[px][0], o[px][1], o[px][2], o[px][3]};
        }
        __syncthreads();
        const int imgs = p.N - n0 < p.NI ? p.N - n0 : p.NI, rows = p.H - oh0 < p.TH ? p.H - oh0 : p.TH;
        const int nvalid = p.NI > 1 ? imgs * p.ipt : rows * p.W;          // valid pixels of this tile (a multiple of 4)
        for (int set = 0; set < p.nsets; ++set, par ^= 1) {
            i32x4 acc[4][NB];
#pragma unroll
            for (int mf = 0; mf < 4; ++mf)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[mf][nb] = i32x4{0, 0, 0, 0};
            const unsigned char* wp = p.wpk + (int64_t)set * NB * p.nsteps * 1024 + lane * 16;
            u32x4 bn[NB];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) bn[nb] = *reinterpret_cast<const u32x4*>(wp + (int64_t)nb * p.nsteps * 1024);
            for (int ks = 0; ks < p.nsteps; ++ks) {
                u32x4 b[NB], a[4];
                const int kn = ks + 1 < p.nsteps ? ks + 1 : ks;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) { b[nb] = bn[nb]; bn[nb] = *reinterpret_cast<const u32x4*>(wp + ((int64_t)nb * p.nsteps + kn) * 1024); }
                const int off = tab[4 * ks + kg];
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) a[mf] = *reinterpret_cast<const u32x4*>(patch + abase[mf] + off);
#pragma unroll
                for (int mf = 0; mf < 4; ++mf)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) acc[mf][nb] = mn_mfma_i8(a[mf], b[nb], acc[mf][nb]);
            }
            // ---- epilogue: lane (j, kg) holds pixels 64 wave + 16 mf + 4 kg + {0 .. 3} of channel 16 (set NB + nb) + j
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int o = (set * NB + nb) * 16 + j;
                const bool okc = o < p.O;
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int mf = 0; mf < 4; ++mf) {
                    if (wave * 64 + mf * 16 + 4 * kg + 4 <= nvalid) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) { const double dv = (double)acc[mf][nb][r]; s1 += dv; s2 = fma(dv, dv, s2); }
                    }
                }
                if (p.out32) {
#pragma unroll
                    for (int mf = 0; mf < 4; ++mf) {
                        const int tp = wave * 64 + mf * 16 + 4 * kg;
                        if (okc && tp + 4 <= nvalid) {
                            const int img = (int)fd_div((uint32_t)tp, p.fd_ipt), rem = tp - img * p.ipt;
                            *reinterpret_cast<u32x4*>(reinterpret_cast<int32_t*>(p.stash) + (uint32_t)(((n0 + img) * p.O + o) * p.HW + oh0 * p.W + rem)) =
                                u32x4{(uint32_t)acc[mf][nb][0], (uint32_t)acc[mf][nb][1], (uint32_t)acc[mf][nb][2], (uint32_t)acc[mf][nb][3]};
                        }
                    }
                } else {
                    const bool odd = kg & 1;
#pragma unroll
                    for (int mp = 0; mp < 2; ++mp) {          // fragments 2 mp (kept by even kg) and 2 mp + 1 (kept by odd kg): the partner's half arrives by exchange
                        uint32_t pk[2][2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const i32x4 c = acc[2 * mp + h][nb];
                            pk[h][0] = ((uint32_t)c[0] & 0xffffu) | ((uint32_t)c[1] << 16); pk[h][1] = ((uint32_t)c[2] & 0xffffu) | ((uint32_t)c[3] << 16);
                        }
                        const uint32_t k0 = odd ? pk[1][0] : pk[0][0], k1 = odd ? pk[1][1] : pk[0][1];
                        const uint32_t r0 = (uint32_t)__shfl_xor((int)(odd ? pk[0][0] : pk[1][0]), 16, 64), r1 = (uint32_t)__shfl_xor((int)(odd ? pk[0][1] : pk[1][1]), 16, 64);
                        const int tp = wave * 64 + (2 * mp + (odd ? 1 : 0)) * 16 + 4 * (kg & 2);          // the run of 8 pixels this lane stores
                        if (okc && tp + 4 <= nvalid) {
                            const int img = (int)fd_div((uint32_t)tp, p.fd_ipt), rem = tp - img * p.ipt;
                            int16_t* dst = reinterpret_cast<int16_t*>(p.stash) + (uint32_t)(((n0 + img) * p.O + o) * p.HW + oh0 * p.W + rem);
                            const uint32_t l0 = odd ? r0 : k0, l1 = odd ? r1 : k1, h0 = odd ? k0 : r0, h1 = odd ? k1 : r1;
                            if (tp + 8 <= nvalid) *reinterpret_cast<u32x4*>(dst) = u32x4{l0, l1, h0, h1};
                            else *reinterpret_cast<u32x2*>(dst) = u32x2{l0, l1};          // (a band whose pixel count is 4 mod 8)
                        }
                    }
                }
                s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
                s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
                if (kg == 0) { double* d = red + (((par * 4 + wave) * NB + nb) * 16 + j) * 2; d[0] = s1; d[1] = s2; }
            }
            __syncthreads();          // (red is double-buffered by set parity: the next set's writes go to the other half)
            if (tid < NB * 16) {
                double a1 = 0.0, a2 = 0.0;
#pragma unroll
                for (int w = 0; w < 4; ++w) { const double* s = red + ((par * 4 + w) * NB * 16 + tid) * 2; a1 += s[0]; a2 += s[1]; }
                double* d = tot + (set * NB * 16 + tid) * 2;
                d[0] += a1; d[1] += a2;
            }
        }
    }
    if (tid < NB * 16) {          // (tot is only ever touched by this thread)
        for (int set = 0; set < p.nsets; ++set) {
            const int o = set * NB * 16 + tid;
            if (o < p.O) { double* dst = p.part + ((int64_t)blockIdx.x * p.O + o) * 2; dst[0] = tot[o * 2]; dst[1] = tot[o * 2 + 1]; }
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct Q5Plan { Q5Params p; int NB, grid; size_t lds; int64_t off_part, ws_bytes; };
static int q5_geom_ok(const mn_conv_geom* g) {
    if (!g || g->groups != 1 || g->in_shuffle > 1 || g->KH != 5 || g->KW != 5 || g->stride_h != 1 || g->stride_w != 1 || g->pad_h != 2 || g->pad_w != 2 ||
        g->dil_h != 1 || g->dil_w != 1 || g->N < 1 || g->C < 16 || g->O < 16 || g->C % 16 || g->O % 16) return 0;
    if (!mn_qa_supported(g->H, g->W, 0) || g->W % 4 || g->W > 64) return 0;
    if ((int64_t)g->N * g->C * g->H * g->W >= ((int64_t)1 << 31) || (int64_t)g->N * g->O * g->H * g->W >= ((int64_t)1 << 31)) return 0;          // 32-bit element offsets
    return 1;
}
static int plan_q5(const mn_conv_geom* g, int out32, Q5Plan* pl) {
    if (!q5_geom_ok(g)) return 0;
    Q5Params& p = pl->p;
    p.N = (int)g->N; p.C = (int)g->C; p.H = (int)g->H; p.W = (int)g->W; p.O = (int)g->O; p.HW = p.H * p.W; p.out32 = out32;
    pl->NB = p.O % 64 == 0 ? 4 : 2;
    p.nchunks = p.C / 16; p.nslots = 25 * p.nchunks; p.nsteps = (p.nslots + 3) / 4; p.nsets = (p.O / 16 + pl->NB - 1) / pl->NB;
    int TH = 256 / p.W < p.H ? 256 / p.W : p.H;
    int NI = TH == p.H && 256 / p.HW > 1 ? 256 / p.HW : 1;
    if (NI > p.N) NI = p.N;
    const int64_t tail = (int64_t)qg_roundup(4 * p.nsteps * 4, 16) + 2 * 4 * pl->NB * 16 * 16 + (int64_t)p.nsets * pl->NB * 16 * 16;
    for (;;) {
        if ((int64_t)p.nchunks * NI * (TH + 4) * (p.W + 4) * 16 + tail <= Q5_LDS_CAP) break;
        if (NI > 1) --NI; else if (TH > 1) --TH; else return 0;          // (a one-row band with its halo must fit)
    }
    if (TH < p.H && (TH * p.W) % 8) { if (TH > 1) --TH; else return 0; }          // bands start on 8-pixel boundaries: 16-byte runs of a 16-bit stash stay aligned
    p.TH = TH; p.NI = NI; p.PH = TH + 4; p.PW = p.W + 4; p.W4 = p.W / 4; p.ipt = TH * p.W; p.tpix = NI * p.ipt;
    p.tpi = (p.H + TH - 1) / TH; p.ntiles = NI > 1 ? (p.N + NI - 1) / NI : p.N * p.tpi;
    p.CS = NI * p.PH * p.PW * 16; p.nunits = p.nchunks * NI * p.PH * p.W4;
    p.off_tab = p.nchunks * p.CS; p.off_red = p.off_tab + qg_roundup(4 * p.nsteps * 4, 16); p.off_tot = p.off_red + 2 * 4 * pl->NB * 16 * 16;
    pl->lds = (size_t)p.off_tot + (size_t)p.nsets * pl->NB * 16 * 16;
    p.fd_w4 = make_fastdiv((uint32_t)p.W4); p.fd_ph = make_fastdiv((uint32_t)p.PH); p.fd_ni = make_fastdiv((uint32_t)NI); p.fd_w = make_fastdiv((uint32_t)p.W);
    p.fd_ipt = make_fastdiv((uint32_t)p.ipt); p.fd_tpi = make_fastdiv((uint32_t)p.tpi);
    pl->grid = p.ntiles < Q5_MAXPARTS ? p.ntiles : Q5_MAXPARTS;
    // workspace: packed weight bytes | statistics partials [grid <= 512][O][2] doubles
    pl->off_part = ((int64_t)p.nsets * pl->NB * p.nsteps * 1024 + 255) / 256 * 256;
    pl->ws_bytes = pl->off_part + (int64_t)Q5_MAXPARTS * p.O * 2 * 8;
    return 1;
}
static int64_t q5_ws_bytes(const mn_conv_geom* g) { Q5Plan pl; return plan_q5(g, 0, &pl) ? pl.ws_bytes : 0; }
// all three directions: this forward, the generic k x k backward-data (no activation needed) and k_kk_wgrad<1, 25, MN_ACTQ_CODE8>
static int q5_supported(const mn_conv_geom* g, const mn_wq* wq, int a_bits) {
    Q5Plan pl;
    if (!wq || wq->mode != MN_WQ_DOREFA || wq->bits < 2 || wq->bits > 7 || a_bits < 2 || a_bits > 7 || !plan_q5(g, 0, &pl)) return 0;          // 8-bit operands: not signed bytes
    if ((int64_t)g->C * 25 * ((1ll << a_bits) - 1) * ((1ll << wq->bits) - 1) >= ((int64_t)1 << 31)) return 0;
    mn_actq aq; aq.mode = MN_ACTQ_CODE8; aq.bits = a_bits; aq.q_type = 0; aq.flags = 0; aq.qp = nullptr; aq.codes = nullptr; aq.stats = nullptr; aq.dx_add = nullptr; aq.ste_mask = nullptr;
    return kk_supported(g, &aq, wq, 1) && kk_wgrad_code8_supported(g, a_bits);
}
// conv on activation codes -> stash (int16 / int32) + statistics partials part[nparts][O][2]
static int q5_fwd_stash(const mn_conv_geom* g, const mn_wq* wq, const uint8_t* x, const float* w, void* stash, int out32, void* ws, int64_t ws_bytes, hipStream_t s,
                        const double** parts, int* nparts) {
    Q5Plan pl;
    if (!plan_q5(g, out32, &pl)) MN_FAIL(MN_ENOTSUP, "mn_qconv_bnq_fwd_stash(5x5): geometry not covered");
    if (!ws || ws_bytes < pl.ws_bytes || !aligned16(ws)) MN_FAIL(MN_ENOSPC, "mn_qconv_bnq_fwd_stash(5x5): workspace too small");
    Q5Params& p = pl.p;
    unsigned char* wpk = reinterpret_cast<unsigned char*>(ws);
    const int ntile16 = p.nsets * pl.NB, ngroups = ntile16 * p.nsteps * 64;
    hipLaunchKernelGGL(k_q5_pack, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, s, w, wpk, p.O, p.C, p.nchunks, p.nsteps, ntile16, (float)((1ll << wq->bits) - 1));
    p.x = x; p.wpk = wpk; p.stash = stash; p.part = reinterpret_cast<double*>((char*)ws + pl.off_part);
    mn_set_last_kernel("k_q5_fwd<%d>", pl.NB);
    { const double nx = (double)p.N * p.C * p.HW, ny = (double)p.N * p.O * p.HW; mn_prof_bytes(nx + (out32 ? 4.0 : 2.0) * ny); mn_prof_flops(2.0 * ny * p.C * 25); }
    mn_prof_begin(s);
    if (pl.NB == 4) { raise_lds_limit((const void*)k_q5_fwd<4>, pl.lds); hipLaunchKernelGGL(k_q5_fwd<4>, dim3(pl.grid), dim3(256), pl.lds, s, p); }
    else { raise_lds_limit((const void*)k_q5_fwd<2>, pl.lds); hipLaunchKernelGGL(k_q5_fwd<2>, dim3(pl.grid), dim3(256), pl.lds, s, p); }
    mn_prof_end(s);
    *parts = p.part; *nparts = pl.grid;
    MN_CHECK_LAUNCH("mn_qconv_bnq_fwd_stash(5x5)");
    return MN_OK;
}
