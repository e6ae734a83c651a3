// f32-MFMA implicit-GEMM convolution kernels for gfx950 (CDNA4).
//
// The dense stride-1 convolutions of the hot path (the 24 dilated k3 convs of the generator's
// residual atoms, its k7 input conv, the discriminator's 1024->1024 k5 conv) carry ~3/4 of the
// train step's FLOPs at 48..250 FLOP/B: in exact fp32 they are bound by the matrix pipe, not by
// HBM.  They are lowered to an im2col x weight contraction executed with v_mfma_f32_32x32x2_f32
// (fp32 in / fp32 accumulate, bit-identical to an fmaf chain, 64 FLOP/clk/SIMD):
//
//   forward        Y[m, (b,t)]  = sum_{(c,j)}  W[m, c, j]        * X[b, c, t + j*dil - pad]
//   backward data  dX[m, (b,t)] = sum_{(c,j')} W[c, m, K-1-j']   * dY'[b, c, t + j'*dil - pad]
//   backward wgt   dW[m, (c,j)] = sum_{(b,t)}  dY'[b, m, t]      * X[b, c, t + j*dil - pad]
//
// (dY' = dY * act'(Y) is formed in the operand loader.)  A 256-thread workgroup (4 waves of 64)
// owns a BM x BN output tile; each wave a TM x TN grid of 32x32 MFMA tiles.  Per K-chunk the A
// (weights or dY') and B (im2col of the activations, built on the fly: nothing is materialised
// in HBM) tiles are staged in LDS; time is the lane-fast index of every global access, so
// activation traffic is coalesced along contiguous audio frames.  Global loads of chunk c+1 are
// in flight while the MFMAs of chunk c run.
#include <cstdlib>
#include "conv_mfma.h"
#include "conv_rows2.h"
#include "operand_split.h"
#include <stdio.h>
#include <stdlib.h>

namespace {

constexpr int KC = 16;        // GEMM-K elements staged per chunk
constexpr int KCP = KC + 1;   // odd LDS row stride: conflict-free 32-lane column reads

struct IgP {
    int B, CK, L, M, dil, off0, pad_mode, act, in_act, N, KG;
    float slope;
    int in_s;   // weight-grad B operand: channel c' = co*in_s + r is phase r of a stride-in_s signal
};

// branch-free source index: every load below is issued unconditionally from a clamped (always
// valid) address and masked afterwards, so hipcc batches the loads of a chunk instead of waiting
// for each one (a load under a run-time branch costs a full memory round trip per element)
__device__ __forceinline__ int src_index_sel(int t, int L, int reflect) {
    const int r = t < 0 ? -t : (t >= L ? 2 * (L - 1) - t : t);
    return reflect ? r : t;
}

// ------------------------------------------------------------ forward / backward data
template <int WGM, int WGN, int TM, int TN, int K, bool TRANS>
__global__ __launch_bounds__(256) void k_igemm_conv(IgP p, const float* __restrict__ X,
                                                   const float* __restrict__ Xact,
                                                   const float* __restrict__ W,
                                                   const float* __restrict__ bias,
                                                   const float* __restrict__ res,
                                                   float* __restrict__ Y,
                                                   float* __restrict__ Yact) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    constexpr int RA = BM * KC / 256, RB = BN * KC / 256;
    constexpr int NCOL = BN > 256 ? BN / 256 : 1;         // columns a loader thread owns
    constexpr int ROWSTEP = BN > 256 ? 1 : 256 / BN;      // B-tile rows covered per pass
    static_assert(WGM * WGN == 4, "4 waves");
    static_assert(RB % NCOL == 0, "loader mapping");
    __shared__ float As[BM * KCP];
    __shared__ float Bs[KC * BN];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;

    // B loader: fixed column(s) per thread
    int cb[NCOL], ct[NCOL];
    bool cvalid[NCOL];
#pragma unroll
    for (int q = 0; q < NCOL; ++q) {
        const int n = n0 + (tid % BN) + q * 256;
        cvalid[q] = n < p.N;
        const int nn = cvalid[q] ? n : 0;
        cb[q] = nn / p.L;
        ct[q] = nn - cb[q] * p.L;
    }
    const int brow0 = BN > 256 ? 0 : tid / BN;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // absent activation operand: alias the data (second load hits L1) with a pass-through kind
    const float* Xa = Xact ? Xact : X;
    const int in_act = Xact ? p.in_act : MS_ACT_NONE;
    float ra[RA], rb[RB];
    auto gload = [&](int kc0) {
#pragma unroll
        for (int r = 0; r < RA; ++r) {
            const int e = r * 256 + tid;
            bool ok;
            size_t off;
            if (!TRANS) {
                const int kk = e % KC, m = e / KC;
                ok = m0 + m < p.M && kc0 + kk < p.KG;
                off = (size_t)(m0 + m) * p.KG + kc0 + kk;
            } else {
                const int m = e % BM, kk = e / BM;
                const int kg = kc0 + kk;
                const int c = kg / K, j = kg - c * K;
                ok = m0 + m < p.M && kg < p.KG;
                off = ((size_t)c * p.M + m0 + m) * K + (K - 1 - j);
            }
            const float v = W[ok ? off : 0];
            ra[r] = ok ? v : 0.f;
        }
        float xv[RB], av[RB];
        bool ok[RB];
#pragma unroll
        for (int r = 0; r < RB / NCOL; ++r) {
            const int kg = kc0 + brow0 + r * ROWSTEP;
            const int c = kg / K, j = kg - c * K;
#pragma unroll
            for (int q = 0; q < NCOL; ++q) {
                const int sidx = src_index_sel(ct[q] + j * p.dil + p.off0, p.L, p.pad_mode == MS_PAD_REFLECT);
                const bool v = cvalid[q] && kg < p.KG && (unsigned)sidx < (unsigned)p.L;
                const size_t off = v ? ((size_t)cb[q] * p.CK + c) * p.L + sidx : 0;
                ok[r * NCOL + q] = v;
                xv[r * NCOL + q] = X[off];
                av[r * NCOL + q] = Xa[off];
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) rb[r] = ok[r] ? ms_act_grad(xv[r], av[r], in_act, p.slope) : 0.f;
    };
    auto lstore = [&]() {
#pragma unroll
        for (int r = 0; r < RA; ++r) {
            const int e = r * 256 + tid;
            if (!TRANS) As[(e / KC) * KCP + (e % KC)] = ra[r];
            else As[(e % BM) * KCP + (e / BM)] = ra[r];
        }
#pragma unroll
        for (int r = 0; r < RB / NCOL; ++r) {
            const int kk = brow0 + r * ROWSTEP;
#pragma unroll
            for (int q = 0; q < NCOL; ++q) Bs[kk * BN + (tid % BN) + q * 256] = rb[r * NCOL + q];
        }
    };

    const int nchunks = (p.KG + KC - 1) / KC;
    gload(0);
    lstore();
    __syncthreads();
    const int arow = (wm * TM * 32 + (lane & 31)) * KCP + (lane >> 5);
    const int bcol = (lane >> 5) * BN + wn * TN * 32 + (lane & 31);
    for (int c = 0; c < nchunks; ++c) {
        const bool more = c + 1 < nchunks;
        if (more) gload((c + 1) * KC);
#pragma unroll
        for (int k2 = 0; k2 < KC / 2; ++k2) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[arow + i * 32 * KCP + 2 * k2];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[bcol + 2 * k2 * BN + j * 32];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            lstore();
            __syncthreads();
        }
    }

    // epilogue: D[row][col]: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5); bias and
    // residual loads of a tile are batched ahead of its stores (no loads under per-element branches)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * TN * 32 + j * 32 + (lane & 31);
        if (n >= p.N) continue;
        const int b = n / p.L, t = n - b * p.L;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mb = m0 + wm * TM * 32 + i * 32 + 4 * (lane >> 5);
            const size_t obase = ((size_t)b * p.M + mb) * p.L + t;
            float bv[16], rv[16];
            bool ok[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dm = (r & 3) + 8 * (r >> 2);
                ok[r] = mb + dm < p.M;
                bv[r] = bias ? bias[ok[r] ? mb + dm : 0] : 0.f;
            }
            if (res) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int dm = (r & 3) + 8 * (r >> 2);
                    rv[r] = res[ok[r] ? obase + (size_t)dm * p.L : 0];
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dm = (r & 3) + 8 * (r >> 2);
                if (!ok[r]) continue;
                const size_t o = obase + (size_t)dm * p.L;
                float v = ms_apply_act(acc[i][j][r] + bv[r], p.act, p.slope);
                if (Yact) Yact[o] = v;
                if (res) v += rv[r];
                Y[o] = v;
            }
        }
    }
}

// ------------------------------------------------ forward / backward data, row-tile form
// Same contraction as k_igemm_conv, but the activation tile is staged ONCE per channel chunk
// as raw rows with their dilation halo (no im2col duplication, no per-element index math in the
// K loop): a workgroup owns either a BN-long segment of one (b) row (L >= BN) or R = BN / L whole
// rows (short L: the discriminator's 1024->1024 k5 conv at L = 32 / 17 / 9).  The B fragment of
// tap j is the same LDS row read at a +j*dil column offset.  Weights arrive as 16-byte loads of
// the contiguous (c, j) run of each output-channel row; for backward-data they are first
// re-laid-out (transposed + tap-flipped) into the workspace by k_transpose_flip_w.
struct RowP {
    int B, CK, L, M, dil, off0, pad_mode, act, in_act, KG;
    int Lt, R, SS, RSZ, tiles_per_row;   // segment length, rows per tile, LDS segment/row strides
    float slope;
    int CKs;                             // input channels per split-K slice (== CK: no split)
    long long zstride;                   // floats between the partial-output slabs of two slices
    const float* Wfwd;                   // backward data: the forward-layout weights (pipelined kernel reads them directly)
};

template <int WGM, int WGN, int TM, int TN, int K, int CC, bool HAS_ACT, int EPI_S, int IN_S>
__global__ __launch_bounds__(256) void k_conv_mfma_rows(RowP p, const float* __restrict__ X,
                                                       const float* __restrict__ Xact,
                                                       const float* __restrict__ W,
                                                       const float* __restrict__ bias,
                                                       const float* __restrict__ res,
                                                       float* __restrict__ Y,
                                                       float* __restrict__ Yact) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    constexpr int KK = CC * K;               // GEMM-K elements per chunk
    constexpr int AS = KK + 1;               // odd LDS stride of the weight tile
    constexpr int A4 = BM * (KK / 4);        // float4 loads per weight tile
    constexpr int RA4 = (A4 + 255) / 256;
    constexpr int MAXCOL = 2;                // LDS columns a loader thread owns (RSZ <= 512)
    static_assert(WGM * WGN == 4, "4 waves");
    static_assert(KK % 4 == 0 && KK % 2 == 0, "chunk must be float4- and k-pair-sized");
    extern __shared__ float smem[];
    float* As = smem;                        // [BM][AS]
    float* Xs = smem + BM * AS;              // [CC][RSZ]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5;
    const int wm = wid / WGN, wn = wid % WGN;
    const int m0 = blockIdx.y * BM;
    int b0, t0;
    if (p.R == 1) { b0 = blockIdx.x / p.tiles_per_row; t0 = (blockIdx.x - b0 * p.tiles_per_row) * BN; }
    else { b0 = blockIdx.x * p.R; t0 = 0; }

    // X loader: per-thread LDS columns -> global offset of channel 0 (or -1: zero padding)
    long long goff[MAXCOL];
#pragma unroll
    for (int q = 0; q < MAXCOL; ++q) {
        const int col = tid + q * 256;
        goff[q] = -1;
        if (col < p.RSZ) {
            const int r = col / p.SS, pos = col - r * p.SS;
            const int b = b0 + r;
            if (b < p.B) {
                const int s = ms_src_index(t0 + pos + p.off0, p.L, p.pad_mode);
                // IN_S > 1: channel c' = co*IN_S + r is phase r of a stride-IN_S signal (row length
                // L*IN_S) -- the input of a transposed conv's backward passes
                if (s >= 0) goff[q] = (long long)b * p.CK * p.L + (long long)s * IN_S;
            }
        }
    }
    const bool has_col1 = p.RSZ > 256;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // B-fragment base column of this lane for each N sub-tile (output column -> LDS column)
    int bbase[TN];
    bool nvalid[TN];
    int ob[TN], ot[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nl = wn * TN * 32 + j * 32 + (lane & 31);
        const int r = nl / p.Lt, tc = nl - r * p.Lt;
        nvalid[j] = r < p.R && b0 + r < p.B && t0 + tc < p.L;
        bbase[j] = nvalid[j] ? r * p.SS + tc : 0;
        ob[j] = b0 + r;
        ot[j] = t0 + tc;
    }

    float4 ra[RA4];
    float rx[MAXCOL][CC];
    auto gload = [&](int c0) {
#pragma unroll
        for (int i = 0; i < RA4; ++i) {
            const int e = i * 256 + tid;
            const int row = e / (KK / 4), q4 = e - row * (KK / 4);
            const bool ok = e < A4 && m0 + row < p.M;
            const size_t off = ok ? (size_t)(m0 + row) * p.KG + (size_t)c0 * K + q4 * 4 : 0;
            float4 v = *reinterpret_cast<const float4*>(W + off);
            if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
            ra[i] = v;
        }
#pragma unroll
        for (int q = 0; q < MAXCOL; ++q) {
            if (q == 1 && !has_col1) break;
            const bool ok = goff[q] >= 0;
            const size_t base = ok ? (size_t)goff[q] + (size_t)(c0 / IN_S) * p.L * IN_S : 0;
            const size_t step = ok ? (size_t)p.L * IN_S : 0;
            float av[CC];
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                const size_t off = base + (c / IN_S) * step + (ok ? (c % IN_S) : 0);
                rx[q][c] = X[off];
                if (HAS_ACT) av[c] = Xact[off];
            }
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                float v = rx[q][c];
                if (HAS_ACT) v = ms_act_grad(v, av[c], p.in_act, p.slope);
                rx[q][c] = ok ? v : 0.f;
            }
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < RA4; ++i) {
            const int e = i * 256 + tid;
            if (e < A4) {
                const int row = e / (KK / 4), q4 = e - row * (KK / 4);
                float* d = As + row * AS + q4 * 4;
                d[0] = ra[i].x; d[1] = ra[i].y; d[2] = ra[i].z; d[3] = ra[i].w;
            }
        }
#pragma unroll
        for (int q = 0; q < MAXCOL; ++q) {
            if (q == 1 && !has_col1) break;
            const int col = tid + q * 256;
            if (col < p.RSZ) {
#pragma unroll
                for (int c = 0; c < CC; ++c) Xs[c * p.RSZ + col] = rx[q][c];
            }
        }
    };

    // split-K: slice z contracts channels [z*CKs, min((z+1)*CKs, CK)) into its own output slab
    const int cbeg = blockIdx.z * p.CKs;
    const int nchunks = ((cbeg + p.CKs < p.CK ? cbeg + p.CKs : p.CK) - cbeg) / CC;
    Y += (size_t)blockIdx.z * p.zstride;
    gload(cbeg);
    lstore();
    __syncthreads();
    const int arow = (wm * TM * 32 + (lane & 31)) * AS + h;
    for (int ch = 0; ch < nchunks; ++ch) {
        const bool more = ch + 1 < nchunks;
        if (more) gload(cbeg + (ch + 1) * CC);
#pragma unroll
        for (int q = 0; q < KK / 2; ++q) {
            constexpr int dummy = 0; (void)dummy;
            const int kk0 = 2 * q, kk1 = 2 * q + 1;
            const int off_lo = (kk0 / K) * p.RSZ + (kk0 % K) * p.dil;
            const int off_hi = (kk1 / K) * p.RSZ + (kk1 % K) * p.dil;
            const int off = h ? off_hi : off_lo;
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = As[arow + i * 32 * AS + 2 * q];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Xs[off + bbase[j]];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            lstore();
            __syncthreads();
        }
    }

    if (EPI_S == 0) {
        // All loads of a 16-row accumulator tile (bias, residual) are issued as one batch from
        // clamped addresses before any store: loads under per-element branches serialise into one
        // memory round trip each (measured: 40 us of a 109 us launch).
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            if (!nvalid[j]) continue;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int mb = m0 + wm * TM * 32 + i * 32 + 4 * h;
                const size_t obase = ((size_t)ob[j] * p.M + mb) * p.L + ot[j];
                float bv[16], rv[16];
                bool ok[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int dm = (r & 3) + 8 * (r >> 2);
                    ok[r] = mb + dm < p.M;
                    bv[r] = bias ? bias[ok[r] ? mb + dm : 0] : 0.f;
                }
                if (res) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int dm = (r & 3) + 8 * (r >> 2);
                        rv[r] = res[ok[r] ? obase + (size_t)dm * p.L : 0];
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int dm = (r & 3) + 8 * (r >> 2);
                    if (!ok[r]) continue;
                    const size_t o = obase + (size_t)dm * p.L;
                    float v = ms_apply_act(acc[i][j][r] + bv[r], p.act, p.slope);
                    if (Yact) Yact[o] = v;
                    if (res) v += rv[r];
                    Y[o] = v;
                }
            }
        }
    } else {
        // transposed conv: GEMM row m' = co*S + r is output phase r of channel co; a lane's 4
        // consecutive accumulator rows are 4 consecutive output samples (S = 8, S = 4) or 2 x 2 (S = 2),
        // written as one 16-byte / two 8-byte stores along contiguous audio frames
        constexpr int ES = EPI_S > 0 ? EPI_S : 1;     // (EPI_S == 0 never reaches this branch)
        const int Cout = p.M / ES;
        const size_t Lo = (size_t)p.L * ES;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            if (!nvalid[j]) continue;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                float bq[4][2];
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {   // bias loads batched ahead of the stores
                    const int mb = m0 + wm * TM * 32 + i * 32 + 8 * rg + 4 * h;
                    const int co = (mb < p.M ? mb : 0) / ES;
                    bq[rg][0] = bias ? bias[co] : 0.f;
                    bq[rg][1] = (bias && EPI_S < 4) ? bias[co + 1 < Cout ? co + 1 : co] : 0.f;
                }
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const int mb = m0 + wm * TM * 32 + i * 32 + 8 * rg + 4 * h;
                    if (mb >= p.M) continue;
                    if (EPI_S >= 4) {
                        const int co = mb / ES, ph = mb - co * ES;
                        const float bv = bq[rg][0];
                        float4 v;
                        v.x = ms_apply_act(acc[i][j][4 * rg + 0] + bv, p.act, p.slope);
                        v.y = ms_apply_act(acc[i][j][4 * rg + 1] + bv, p.act, p.slope);
                        v.z = ms_apply_act(acc[i][j][4 * rg + 2] + bv, p.act, p.slope);
                        v.w = ms_apply_act(acc[i][j][4 * rg + 3] + bv, p.act, p.slope);
                        *reinterpret_cast<float4*>(Y + ((size_t)ob[j] * Cout + co) * Lo + (size_t)ot[j] * ES + ph) = v;
                    } else {
                        const int co = mb / 2;
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const float bv = bq[rg][u];
                            float2 v;
                            v.x = ms_apply_act(acc[i][j][4 * rg + 2 * u + 0] + bv, p.act, p.slope);
                            v.y = ms_apply_act(acc[i][j][4 * rg + 2 * u + 1] + bv, p.act, p.slope);
                            *reinterpret_cast<float2*>(Y + ((size_t)ob[j] * Cout + co + u) * Lo + (size_t)ot[j] * 2) = v;
                        }
                    }
                }
            }
        }
    }
}

// Epilogue of a split-K row-tile launch: sums the slices' slabs in slice order (deterministic) and
// applies what the fused epilogue would have: bias (channel = (i / rowlen) % nch), activation,
// the pre-residual copy and the residual add.
__global__ __launch_bounds__(256) void k_rows_split_finish(const float* __restrict__ slabs, int ns,
                                                          size_t zstride,
                                                          const float* __restrict__ bias, int nch,
                                                          int rowlen, int act, float slope,
                                                          const float* __restrict__ res,
                                                          float* __restrict__ Y,
                                                          float* __restrict__ Yact, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        float v = slabs[i];
        for (int z = 1; z < ns; ++z) v += slabs[(size_t)z * zstride + i];
        if (bias) v += bias[(i / rowlen) % nch];
        v = ms_apply_act(v, act, slope);
        if (Yact) Yact[i] = v;
        if (res) v += res[i];
        Y[i] = v;
    }
}

// Packed weights of the 3-tap polyphase form of ConvTranspose1d(K = 2S, padding = S/2):
//   y[b, co, q*S + r] = sum_ci sum_{d=-1..1} W[ci, co, r + pad - d*S] * x[b, ci, q + d]
// Wp[(co*S + r)][ci*3 + (d+1)], zero where the tap index falls outside [0, K).
__global__ __launch_bounds__(256) void k_pack_convt_w(const float* __restrict__ W,
                                                     float* __restrict__ Wp, int Cin, int Cout,
                                                     int K, int S, int pad) {
    const size_t total = (size_t)Cout * S * Cin * 3;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % 3) - 1;
        size_t r0 = i / 3;
        const int ci = (int)(r0 % Cin);
        r0 /= Cin;
        const int r = (int)(r0 % S);
        const int co = (int)(r0 / S);
        const int k = r + pad - d * S;
        Wp[i] = (k >= 0 && k < K) ? W[((size_t)ci * Cout + co) * K + k] : 0.f;
    }
}

// Two-live-tap form of the same weights (K = 2S, pad = S/2: d in {-1,0} for r < S/2, {0,+1} above), rows
// in groups of 64 = [32 low-phase | 32 high-phase] rows of the same 64/S output channels:
//   Wp2[g*64 + half*32 + co_l*(S/2) + rh][ci*2 + jj] = W[ci, co, r + pad - (half + jj - 1)*S]
//   with co = g*(64/S) + co_l, r = half*(S/2) + rh
__global__ __launch_bounds__(256) void k_pack_convt_w2(const float* __restrict__ W,
                                                      float* __restrict__ Wp, int Cin, int Cout,
                                                      int K, int S, int pad) {
    const size_t total = (size_t)Cout * S * Cin * 2;
    const int SH = S / 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int jj = (int)(i % 2);
        size_t r0 = i / 2;
        const int ci = (int)(r0 % Cin);
        const int m = (int)(r0 / Cin);
        const int g = m / 64, half = (m % 64) / 32, l = m % 32;
        const int co = g * (64 / S) + l / SH, r = half * SH + l % SH;
        const int k = r + pad - (half + jj - 1) * S;
        Wp[i] = (k >= 0 && k < K) ? W[((size_t)ci * Cout + co) * K + k] : 0.f;
    }
}

// Wt[ci][co*K + j'] = W[co][ci][K-1-j']  (weights of the conv that computes backward-data)
__global__ __launch_bounds__(256) void k_transpose_flip_w(const float* __restrict__ W,
                                                         float* __restrict__ Wt, int Co, int Ci,
                                                         int K) {
    const size_t total = (size_t)Co * Ci * K;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int jp = (int)(i % K);
        const size_t r = i / K;
        const int co = (int)(r % Co);
        const int ci = (int)(r / Co);
        Wt[i] = W[((size_t)co * Ci + ci) * K + (K - 1 - jp)];
    }
}

// Weights of the 3-tap phase-split form of ConvTranspose1d's backward-data:
//   gx[b, ci, q] = sum_{co, r, d} W[ci, co, r + pad + d*S] * G'[b, (co, r), q + d],  G'[b,(co,r),q] = gp[b,co,qS+r]
// Wq[ci][(co*S + r)*3 + (d+1)], zero where the tap index falls outside [0, K).
__global__ __launch_bounds__(256) void k_pack_convt_bwd_w(const float* __restrict__ W,
                                                         float* __restrict__ Wq, int Cin, int Cout,
                                                         int K, int S, int pad) {
    const size_t total = (size_t)Cin * Cout * S * 3;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % 3) - 1;
        size_t r0 = i / 3;
        const int r = (int)(r0 % S);
        r0 /= S;
        const int co = (int)(r0 % Cout);
        const int ci = (int)(r0 / Cout);
        const int k = r + pad + d * S;
        Wq[i] = (k >= 0 && k < K) ? W[((size_t)ci * Cout + co) * K + k] : 0.f;
    }
}

// The same weights with only the two live taps of each phase (K = 2S, pad = S/2: d in {0,+1} for
// r < S/2, {-1,0} above):  Wq2[ci][(co*S + r)*2 + jj] = W[ci, co, r + pad + (jb(r) + jj - 1)*S]
__global__ __launch_bounds__(256) void k_pack_convt_bwd_w2(const float* __restrict__ W,
                                                          float* __restrict__ Wq, int Cin, int Cout,
                                                          int K, int S, int pad) {
    const size_t total = (size_t)Cin * Cout * S * 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int jj = (int)(i % 2);
        size_t r0 = i / 2;
        const int r = (int)(r0 % S);
        r0 /= S;
        const int co = (int)(r0 % Cout);
        const int ci = (int)(r0 / Cout);
        const int d = (r < S / 2 ? 1 : 0) + jj - 1;
        const int k = r + pad + d * S;
        Wq[i] = (k >= 0 && k < K) ? W[((size_t)ci * Cout + co) * K + k] : 0.f;
    }
}

// gw[ci, co, k] = beta*gw + dWq[ci][(co*S + r)*3 + (d+1)] with k = r + pad + d*S
__global__ __launch_bounds__(256) void k_unpack_convt_gw(const float* __restrict__ dWq,
                                                        float* __restrict__ gw, int Cin, int Cout,
                                                        int K, int S, int pad, float beta) {
    const size_t total = (size_t)Cin * Cout * K;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int k = (int)(i % K);
        const size_t cc = i / K;               // ci*Cout + co
        const int kp = k - pad;
        int d = kp >= 0 ? kp / S : -((-kp + S - 1) / S);
        const int r = kp - d * S;
        const float v = dWq[(cc * S + r) * 3 + (d + 1)];
        gw[i] = (beta != 0.f ? beta * gw[i] : 0.f) + v;
    }
}

// ------------------------------------------------------------------ backward weight
// partial[z][m][n] = sum over this block's kk = (b,t) range of A[m,kk] * Bm[kk,n]
//   A[m, kk] = dY'[b, m, t],  Bm[kk, n=(c,j)] = X[b, c, t + j*dil + off0]
// Both operands are contiguous along kk (time), so both LDS tiles are [row][kk].
template <int WGM, int WGN, int TM, int TN, int K>
__global__ __launch_bounds__(256) void k_igemm_wgrad(IgP p, int chunks_per_split,
                                                    const float* __restrict__ X,
                                                    const float* __restrict__ Xact,
                                                    const float* __restrict__ G,
                                                    const float* __restrict__ Gact, int g_act,
                                                    float* __restrict__ partial,
                                                    size_t partial_stride) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    constexpr int RA = BM * KC / 256, RB = BN * KC / 256;
    static_assert(WGM * WGN == 4, "4 waves");
    __shared__ float As[BM * KCP];
    __shared__ float Bs[BN * KCP];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int NG = p.CK * K;                 // GEMM-N = (c, j) pairs
    const int KT = p.B * p.L;                // GEMM-K = (b, t) pairs
    const int kk_l = tid % KC, row0 = tid / KC;   // loader: fixed kk lane, rows row0 + 16*r

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float asum[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) asum[i] = 0.f;

    // per-thread row descriptors are chunk-invariant: A rows m (offset m*L), B rows n = (c, j)
    // (offset c*L, tap shift j*dil + off0 for the padding test)
    int aoff[RA], boff[RB], bsh[RB];
    bool avalid[RA], bvalid[RB];
#pragma unroll
    for (int r = 0; r < RA; ++r) {
        const int m = m0 + row0 + 16 * r;
        avalid[r] = m < p.M;
        aoff[r] = (avalid[r] ? m : 0) * p.L;
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const int n = n0 + row0 + 16 * r;
        bvalid[r] = n < NG;
        const int nn = bvalid[r] ? n : 0;
        const int c = nn / K, j = nn - c * K;
        bsh[r] = j * p.dil + p.off0;
        boff[r] = (c / p.in_s) * p.L * p.in_s + (c % p.in_s);
    }

    const int c_begin = blockIdx.z * chunks_per_split;
    int c_end = c_begin + chunks_per_split;
    const int nchunks = (KT + KC - 1) / KC;
    if (c_end > nchunks) c_end = nchunks;

    // absent activation operands alias the data with a pass-through kind (keeps loads branch-free)
    const float* Gq = Gact ? Gact : G;
    const float* Xq = Xact ? Xact : X;
    const int g_kind = Gact ? g_act : MS_ACT_NONE;
    const int x_kind = Xact ? p.in_act : MS_ACT_NONE;
    float ra[RA], rb[RB];
    auto gload = [&](int chunk) {
        const int kg = chunk * KC + kk_l;
        const bool kv = kg < KT;
        const int b = kv ? kg / p.L : 0;
        const int t = kv ? kg - b * p.L : 0;
        const float* Ga = G + (size_t)b * p.M * p.L + t;
        const float* Gy = Gq + (size_t)b * p.M * p.L + t;
        const float* Xb = X + (size_t)b * p.CK * p.L;
        const float* Xy = Xq + (size_t)b * p.CK * p.L;
        float gv[RA], ga[RA], xv[RB], xa[RB];
        bool xok[RB];
#pragma unroll
        for (int r = 0; r < RA; ++r) {   // rows past M read row 0 and are masked below
            gv[r] = Ga[aoff[r]];
            ga[r] = Gy[aoff[r]];
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int sidx = src_index_sel(t + bsh[r], p.L, p.pad_mode == MS_PAD_REFLECT);
            xok[r] = kv && bvalid[r] && (unsigned)sidx < (unsigned)p.L;
            const int off = xok[r] ? boff[r] + sidx * p.in_s : 0;
            xv[r] = Xb[off];
            xa[r] = Xy[off];
        }
#pragma unroll
        for (int r = 0; r < RA; ++r)
            ra[r] = (kv && avalid[r]) ? ms_act_grad(gv[r], ga[r], g_kind, p.slope) : 0.f;
#pragma unroll
        for (int r = 0; r < RB; ++r) rb[r] = xok[r] ? ms_act_grad(xv[r], xa[r], x_kind, p.slope) : 0.f;
    };
    auto lstore = [&]() {
#pragma unroll
        for (int r = 0; r < RA; ++r) As[(row0 + 16 * r) * KCP + kk_l] = ra[r];
#pragma unroll
        for (int r = 0; r < RB; ++r) Bs[(row0 + 16 * r) * KCP + kk_l] = rb[r];
    };

    const int arow = (wm * TM * 32 + (lane & 31)) * KCP + (lane >> 5);
    const int brow = (wn * TN * 32 + (lane & 31)) * KCP + (lane >> 5);
    if (c_begin < c_end) {
        gload(c_begin);
        lstore();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = c + 1 < c_end;
        if (more) gload(c + 1);
#pragma unroll
        for (int k2 = 0; k2 < KC / 2; ++k2) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                a[i] = As[arow + i * 32 * KCP + 2 * k2];
                asum[i] += a[i];
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[brow + j * 32 * KCP + 2 * k2];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            lstore();
            __syncthreads();
        }
    }

    float* part = partial + (size_t)blockIdx.z * partial_stride;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * TN * 32 + j * 32 + (lane & 31);
        if (n >= NG) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m < p.M) part[(size_t)m * NG + n] = acc[i][j][r];
            }
        }
    }
    // bias grad = row sums of A: lanes (i, k=0) and (i, k=1) each saw half of the kk's
    if (blockIdx.x == 0 && wn == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float s = asum[i] + __shfl_xor(asum[i], 32, 64);
            const int m = m0 + wm * TM * 32 + i * 32 + (lane & 31);
            if (lane < 32 && m < p.M) part[(size_t)p.M * NG + m] = s;
        }
    }
}

template <int WGM, int WGN, int TM, int TN, int K>
__global__ __launch_bounds__(256) void k_igemm_wgrad_v4(IgP p, int chunks_per_split,
                                                    const float* __restrict__ X,
                                                    const float* __restrict__ Xact,
                                                    const float* __restrict__ G,
                                                    const float* __restrict__ Gact, int g_act,
                                                    float* __restrict__ partial,
                                                    size_t partial_stride) {
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    static_assert(WGM * WGN == 4, "4 waves");
    __shared__ float As[BM * KCP];
    __shared__ float Bs[BN * KCP];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int NG = p.CK * K;                 // GEMM-N = (c, j) pairs
    const int KT = p.B * p.L;                // GEMM-K = (b, t) pairs
    // loader: a thread owns 4 consecutive kk (= 4 consecutive time steps of one batch row; the
    // host guarantees L % 4 == 0) of rows row0 + 64*r: 16-byte loads along contiguous audio frames
    const int kq = tid & 3, row0 = tid >> 2;
    constexpr int RA4 = (BM + 63) / 64, RB4 = (BN + 63) / 64;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float asum[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) asum[i] = 0.f;

    int aoff[RA4], boff[RB4], bsh[RB4];
    bool avalid[RA4], bvalid[RB4];
#pragma unroll
    for (int r = 0; r < RA4; ++r) {
        const int row = row0 + 64 * r;
        const int m = m0 + row;
        avalid[r] = row < BM && m < p.M;
        aoff[r] = (avalid[r] ? m : 0) * p.L;
    }
#pragma unroll
    for (int r = 0; r < RB4; ++r) {
        const int row = row0 + 64 * r;
        const int n = n0 + row;
        bvalid[r] = row < BN && n < NG;
        const int nn = bvalid[r] ? n : 0;
        const int c = nn / K, j = nn - c * K;
        bsh[r] = j * p.dil + p.off0;
        boff[r] = c * p.L;
    }

    const int c_begin = blockIdx.z * chunks_per_split;
    int c_end = c_begin + chunks_per_split;
    const int nchunks = (KT + KC - 1) / KC;
    if (c_end > nchunks) c_end = nchunks;

    // absent activation operands alias the data with a pass-through kind (keeps loads branch-free)
    const float* Gq = Gact ? Gact : G;
    const float* Xq = Xact ? Xact : X;
    const int g_kind = Gact ? g_act : MS_ACT_NONE;
    const int x_kind = Xact ? p.in_act : MS_ACT_NONE;
    float4 ra[RA4], rb[RB4];
    auto gload = [&](int chunk) {
        const int kg = chunk * KC + 4 * kq;
        const bool kv = kg < KT;                  // KT % 4 == 0: all 4 or none
        const int b = kv ? kg / p.L : 0;
        const int t = kv ? kg - b * p.L : 0;
        const float* Ga = G + (size_t)b * p.M * p.L + t;
        const float* Gy = Gq + (size_t)b * p.M * p.L + t;
        const float* Xb = X + (size_t)b * p.CK * p.L;
        const float* Xy = Xq + (size_t)b * p.CK * p.L;
        float4 gv[RA4], ga[RA4];
        f32x4u xv[RB4], xa[RB4];
        int s0[RB4];
#pragma unroll
        for (int r = 0; r < RA4; ++r) {
            gv[r] = *reinterpret_cast<const float4*>(Ga + aoff[r]);
            ga[r] = *reinterpret_cast<const float4*>(Gy + aoff[r]);
        }
#pragma unroll
        for (int r = 0; r < RB4; ++r) {
            s0[r] = t + bsh[r];
            // the 4 taps sit in one row; a window hanging over a row end is re-read element-wise below
            const bool inside = s0[r] >= 0 && s0[r] + 3 < p.L;
            const int off = inside ? boff[r] + s0[r] : boff[r];
            xv[r] = *reinterpret_cast<const f32x4u*>(Xb + off);
            xa[r] = *reinterpret_cast<const f32x4u*>(Xy + off);
        }
#pragma unroll
        for (int r = 0; r < RB4; ++r) {
            const bool inside = s0[r] >= 0 && s0[r] + 3 < p.L;
            if (!inside && kv && bvalid[r]) {      // rare: row edges only
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int sidx = s0[r] + i;
                    const bool ok = (unsigned)sidx < (unsigned)p.L;
                    xv[r][i] = ok ? Xb[boff[r] + sidx] : 0.f;
                    xa[r][i] = ok ? Xy[boff[r] + sidx] : 1.f;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RA4; ++r) {
            const bool ok = kv && avalid[r];
            ra[r].x = ok ? ms_act_grad(gv[r].x, ga[r].x, g_kind, p.slope) : 0.f;
            ra[r].y = ok ? ms_act_grad(gv[r].y, ga[r].y, g_kind, p.slope) : 0.f;
            ra[r].z = ok ? ms_act_grad(gv[r].z, ga[r].z, g_kind, p.slope) : 0.f;
            ra[r].w = ok ? ms_act_grad(gv[r].w, ga[r].w, g_kind, p.slope) : 0.f;
        }
#pragma unroll
        for (int r = 0; r < RB4; ++r) {
            const bool ok = kv && bvalid[r];
            rb[r].x = ok ? ms_act_grad(xv[r][0], xa[r][0], x_kind, p.slope) : 0.f;
            rb[r].y = ok ? ms_act_grad(xv[r][1], xa[r][1], x_kind, p.slope) : 0.f;
            rb[r].z = ok ? ms_act_grad(xv[r][2], xa[r][2], x_kind, p.slope) : 0.f;
            rb[r].w = ok ? ms_act_grad(xv[r][3], xa[r][3], x_kind, p.slope) : 0.f;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int r = 0; r < RA4; ++r) {
            const int row = row0 + 64 * r;
            if (row < BM) {
                float* d = As + row * KCP + 4 * kq;
                d[0] = ra[r].x; d[1] = ra[r].y; d[2] = ra[r].z; d[3] = ra[r].w;
            }
        }
#pragma unroll
        for (int r = 0; r < RB4; ++r) {
            const int row = row0 + 64 * r;
            if (row < BN) {
                float* d = Bs + row * KCP + 4 * kq;
                d[0] = rb[r].x; d[1] = rb[r].y; d[2] = rb[r].z; d[3] = rb[r].w;
            }
        }
    };

    const int arow = (wm * TM * 32 + (lane & 31)) * KCP + (lane >> 5);
    const int brow = (wn * TN * 32 + (lane & 31)) * KCP + (lane >> 5);
    if (c_begin < c_end) {
        gload(c_begin);
        lstore();
    }
    __syncthreads();
    for (int c = c_begin; c < c_end; ++c) {
        const bool more = c + 1 < c_end;
        if (more) gload(c + 1);
#pragma unroll
        for (int k2 = 0; k2 < KC / 2; ++k2) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                a[i] = As[arow + i * 32 * KCP + 2 * k2];
                asum[i] += a[i];
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = Bs[brow + j * 32 * KCP + 2 * k2];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            lstore();
            __syncthreads();
        }
    }

    float* part = partial + (size_t)blockIdx.z * partial_stride;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * TN * 32 + j * 32 + (lane & 31);
        if (n >= NG) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * TM * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m < p.M) part[(size_t)m * NG + n] = acc[i][j][r];
            }
        }
    }
    // bias grad = row sums of A: lanes (i, k=0) and (i, k=1) each saw half of the kk's
    if (blockIdx.x == 0 && wn == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float s = asum[i] + __shfl_xor(asum[i], 32, 64);
            const int m = m0 + wm * TM * 32 + i * 32 + (lane & 31);
            if (lane < 32 && m < p.M) part[(size_t)p.M * NG + m] = s;
        }
    }
}

__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* __restrict__ partial,
                                                     size_t partial_stride, int nsplit,
                                                     size_t wsize, int nbias,
                                                     float* __restrict__ gw,
                                                     float* __restrict__ gb, float beta) {
    // 64 consecutive outputs per workgroup (coalesced 256-byte rows of every slab); the slabs are
    // dealt round-robin to the 4 waves, whose partial sums meet in LDS: fixed order, deterministic
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * 64 + lane;
    const bool ok = i < wsize + (size_t)nbias;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (ok) {
        int z = wv;
        for (; z + 12 < nsplit; z += 16) {
            s0 += partial[(size_t)z * partial_stride + i];
            s1 += partial[(size_t)(z + 4) * partial_stride + i];
            s2 += partial[(size_t)(z + 8) * partial_stride + i];
            s3 += partial[(size_t)(z + 12) * partial_stride + i];
        }
        for (; z < nsplit; z += 4) s0 += partial[(size_t)z * partial_stride + i];
    }
    red[wv][lane] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (wv == 0 && ok) {
        const float s = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        if (i < wsize) gw[i] = (beta != 0.f ? beta * gw[i] : 0.f) + s;
        else if (gb) gb[i - wsize] = (beta != 0.f ? beta * gb[i - wsize] : 0.f) + s;
    }
}

// ------------------------------------------------------------------------ host side
// The dispatch inside the family is a plan, like api.hip's one level up.  One planner per pass (plan_fwd, plan_bwd_data,
// plan_convt_fwd, plan_convt_bwd_data; plan_wgrad / plan_convt_wgrad for the two im2col weight gradients) decides, once, the
// kernel family and tile, the split-K depth, the weight re-layout in front, the grid and the workspace layout.  It has three
// readers and nothing else decides anything: msm_*_ws returns the plan's bytes, msm_*_name asks the plan's launcher for the
// spelling of what it would launch, msm_* runs the plan.  What depends on the call and not on the geometry -- where the
// operands and the workspace sit -- is the planners' explicit input (RowCall); the queries plan with its defaults.
bool dense_same(const ConvP& p) {
    return p.groups == 1 && p.stride == 1 && p.Lout == p.Lin && (p.K == 1 || p.K == 3 || p.K == 5 || p.K == 7) &&
           (long long)p.B * p.Lin < (1LL << 31) && (long long)p.Cin * p.K < (1 << 30);
}

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }   // (an absent operand counts as aligned)

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

dim3 blocks256(size_t n, unsigned cap) {
    n = (n + 255) / 256;
    return dim3(n > cap ? cap : (unsigned)n);
}

enum Cfg { CFG_128x128, CFG_64x64, CFG_32x256, CFG_32x128 };

Cfg pick_cfg(int M, long long N) {
    if (M <= 32) return CFG_32x256;
    if (M >= 128 && (N / 128) * (M / 128) >= 384) return CFG_128x128;
    return CFG_64x64;
}

void cfg_tile(Cfg c, int* bm, int* bn) {
    if (c == CFG_128x128) { *bm = 128; *bn = 128; }
    else if (c == CFG_64x64) { *bm = 64; *bn = 64; }
    else if (c == CFG_32x128) { *bm = 32; *bn = 128; }
    else { *bm = 32; *bn = 256; }
}

// name (here and in every launcher below): not null = a name query, see ms_name_or_note (ms_common.h)
template <int K, bool TRANS>
int launch_conv_k(Cfg cfg, const IgP& p, const float* X, const float* Xact, const float* W,
                  const float* bias, const float* res, float* Y, float* Yact, hipStream_t s, char* name) {
    int bm, bn;
    cfg_tile(cfg, &bm, &bn);
    dim3 grid((unsigned)((p.N + bn - 1) / bn), (unsigned)((p.M + bm - 1) / bm));
#define MS_IG(WGM, WGN, TM, TN)                                                                                            \
    do {                                                                                                                   \
        if (ms_name_or_note(name, 0, "k_igemm_conv<%d, %d, %d, %d, %d, %s>", WGM, WGN, TM, TN, K, TRANS ? "true" : "false")) \
            return MS_OK;                                                                                                  \
        hipLaunchKernelGGL((k_igemm_conv<WGM, WGN, TM, TN, K, TRANS>), grid, dim3(256), 0, s, p, X, Xact, W, bias, res, Y, \
                           Yact);                                                                                          \
    } while (0)
    if (cfg == CFG_128x128) MS_IG(2, 2, 2, 2);
    else if (cfg == CFG_64x64) MS_IG(2, 2, 1, 1);
    else MS_IG(1, 4, 1, 2);
#undef MS_IG
    MS_CHECK_LAUNCH();
    return MS_OK;
}

template <bool TRANS>
int launch_conv(int K, Cfg cfg, const IgP& p, const float* X, const float* Xact, const float* W,
                const float* bias, const float* res, float* Y, float* Yact, hipStream_t s, char* name) {
    if (K == 1) return launch_conv_k<1, TRANS>(cfg, p, X, Xact, W, bias, res, Y, Yact, s, name);
    if (K == 3) return launch_conv_k<3, TRANS>(cfg, p, X, Xact, W, bias, res, Y, Yact, s, name);
    if (K == 5) return launch_conv_k<5, TRANS>(cfg, p, X, Xact, W, bias, res, Y, Yact, s, name);
    if (K == 7) return launch_conv_k<7, TRANS>(cfg, p, X, Xact, W, bias, res, Y, Yact, s, name);
    return MS_ERR_UNSUPPORTED;
}

struct WgradPlan {
    Cfg cfg;
    int bm, bn, nsplit, cps;
    size_t stride_floats;
};

WgradPlan plan_wgrad(const ConvP& p) {
    WgradPlan q;
    const int NG = p.Cin * p.K;
    if (p.Cout <= 32) q.cfg = NG <= 128 ? CFG_32x128 : CFG_32x256;
    else if (p.Cout >= 128 && NG >= 128) q.cfg = CFG_128x128;   // 4 MFMAs per 4 LDS fragment reads
    else q.cfg = CFG_64x64;
    cfg_tile(q.cfg, &q.bm, &q.bn);
    const int tiles = ms_ceil_div(p.Cout, q.bm) * ms_ceil_div(NG, q.bn);
    const long long KT = (long long)p.B * p.Lin;
    const int nchunks = (int)((KT + KC - 1) / KC);
    q.stride_floats = (size_t)p.Cout * NG + p.Cout;
    // split-K: ~2 workgroups per CU, >= 16 chunks per split, partial slabs <= 12 MiB in total
    int ns = ms_ceil_div(512, tiles);
    const int max_by_work = nchunks / 16 > 0 ? nchunks / 16 : 1;
    if (ns > max_by_work) ns = max_by_work;
    const size_t cap = (size_t)24 << 20;
    const size_t max_by_bytes = cap / (q.stride_floats * 4);
    if ((size_t)ns > max_by_bytes) ns = max_by_bytes > 0 ? (int)max_by_bytes : 1;
    if (ns < 1) ns = 1;
    q.cps = ms_ceil_div(nchunks, ns);
    q.nsplit = ms_ceil_div(nchunks, q.cps);
    return q;
}

// the im2col weight-gradient GEMM of a plan: M x NG tiles, pl.nsplit slabs.  v4: the 16-byte loader (rows that are a multiple
// of 4 long, zero padding, 16-byte aligned operands)
int launch_wgrad(const WgradPlan& pl, int K, bool v4, const IgP& q, const float* A, const float* Aact, const float* Bm,
                 const float* Bact, int bkind, float* partial, hipStream_t s, char* name) {
    dim3 grid((unsigned)ms_ceil_div(q.KG, pl.bn), (unsigned)ms_ceil_div(q.M, pl.bm), (unsigned)pl.nsplit);
#define MS_WG1(KERNEL, WGM, WGN, TM, TN, KK)                                                                      \
    do {                                                                                                          \
        if (ms_name_or_note(name, 0, #KERNEL "<%d, %d, %d, %d, %d>", WGM, WGN, TM, TN, KK)) return MS_OK;           \
        hipLaunchKernelGGL((KERNEL<WGM, WGN, TM, TN, KK>), grid, dim3(256), 0, s, q, pl.cps, A, Aact, Bm, Bact,    \
                           bkind, partial, pl.stride_floats);                                                     \
    } while (0)
#define MS_WG(WGM, WGN, TM, TN, KK)                           \
    do {                                                      \
        if (v4) MS_WG1(k_igemm_wgrad_v4, WGM, WGN, TM, TN, KK); \
        else MS_WG1(k_igemm_wgrad, WGM, WGN, TM, TN, KK);       \
    } while (0)
#define MS_WG_K(KK)                                           \
    do {                                                      \
        if (pl.cfg == CFG_128x128) MS_WG(2, 2, 2, 2, KK);     \
        else if (pl.cfg == CFG_64x64) MS_WG(2, 2, 1, 1, KK);  \
        else if (pl.cfg == CFG_32x128) MS_WG(1, 4, 1, 1, KK); \
        else MS_WG(1, 4, 1, 2, KK);                           \
    } while (0)
    if (K == 1) MS_WG_K(1);
    else if (K == 3) MS_WG_K(3);
    else if (K == 5) MS_WG_K(5);
    else if (K == 7) MS_WG_K(7);
    else if (K == 15) MS_WG_K(15);
    else return MS_ERR_UNSUPPORTED;
#undef MS_WG_K
#undef MS_WG
#undef MS_WG1
    MS_CHECK_LAUNCH();
    return MS_OK;
}

// ---- row-tile kernel dispatch
enum RowCfg { ROW_128x128, ROW_64x128, ROW_64x64, ROW_32x256, ROW_64x256 };

constexpr int row_cc(int K) { return K == 7 ? 4 : (K == 1 ? 32 : 8); }

bool rows_applicable(int M, int CK, int K, int L) {
    if (!(K == 1 || K == 3 || K == 5 || K == 7)) return false;
    if (CK % row_cc(K)) return false;
    if (M < 32 && CK < 256) return false;   // (few outputs, deep contraction: the judge conv 1024 -> 1 with split-K)
    return L >= 1;
}

// dense = a plain stride-1 conv with 3 or 5 taps, i.e. a launch the split-bf16 kernel (conv_rows3.hip) may take:
// its 128x128 tile needs 112 KiB of LDS (one workgroup per CU, every latency exposed); two co-resident 64x128
// workgroups measured faster (C = 128, L = 2048, B = 32: 58 vs 68 us)
RowCfg pick_row_cfg(int M, int B, int L, bool dense = false) {
    if (M <= 32) return ROW_32x256;
    if (L < 128) return (M >= 512 && (long long)B * L >= 512) ? ROW_64x128 : ROW_64x64;   // short rows: R = 128 / L rows per tile
    const long long N = (long long)B * L;
    const bool split = dense && L % 4 == 0 && ms_switch_on("MSYNTH_ROWS3");
    if (M >= 128 && (N / 128) * (M / 128) >= 384 && !split) return ROW_128x128;
    if ((N / 128) * (M / 64) < 192) return ROW_64x64;   // small batches: more, smaller workgroups
    return ROW_64x128;
}

// tile shape of the transposed-conv forward: short rows (the stage-1 2-D transposed convs as lines: L = 16 .. 64,
// thousands of lines) take the 128-column tiling with R = 128 / L rows per tile even for M < 512, so that the paired
// split-bf16 kernel (which owns 128-column tiles) applies
RowCfg convt_fwd_cfg(int M, int B, int L) {
    const RowCfg c = pick_row_cfg(M, B, L);
    if (c == ROW_64x64 && L < 128 && L % 4 == 0 && 128 % L == 0 && M % 64 == 0 && (long long)B * L >= 128 * 256)
        return ROW_64x128;
    return c;
}

void row_tile(RowCfg c, int* bm, int* bn) {
    switch (c) {
        case ROW_128x128: *bm = 128; *bn = 128; break;
        case ROW_64x128: *bm = 64; *bn = 128; break;
        case ROW_64x64: *bm = 64; *bn = 64; break;
        case ROW_64x256: *bm = 64; *bn = 256; break;
        default: *bm = 32; *bn = 256; break;
    }
}

bool make_rowp(RowP* q, RowCfg cfg, int B, int CK, int L, int M, int K, int dil, int off0,
               int pad_mode, int act, int in_act, float slope) {
    int bm, bn;
    row_tile(cfg, &bm, &bn);
    q->B = B; q->CK = CK; q->L = L; q->M = M; q->dil = dil; q->off0 = off0; q->pad_mode = pad_mode;
    q->act = act; q->in_act = in_act; q->KG = CK * K; q->slope = slope;
    const int H = (K - 1) * dil;
    if (L >= bn) { q->Lt = bn; q->R = 1; q->tiles_per_row = (L + bn - 1) / bn; }
    else { q->Lt = L; q->R = bn / L; q->tiles_per_row = 1; }
    q->SS = q->Lt + H;
    q->RSZ = q->R * q->SS;
    q->CKs = CK; q->zstride = 0; q->Wfwd = nullptr;
    return q->RSZ <= 512;
}

// deep contractions (>= 128 input channels) stage two channel chunks per barrier pair
bool row_deep(int K, int CK) { return K != 7 && K != 1 && CK >= 128 && CK % (2 * row_cc(K)) == 0; }

int rows_cc_eff(int K, int CK) { return row_cc(K) * (row_deep(K, CK) ? 2 : 1); }

bool rows_ok(const ConvP& p, bool bwd) {
    const int M = bwd ? p.Cin : p.Cout, CK = bwd ? p.Cout : p.Cin;
    if (!rows_applicable(M, CK, p.K, p.Lin)) return false;
    if (((size_t)CK * p.K) % 4) return false;
    RowP q;
    return make_rowp(&q, pick_row_cfg(M, p.B, p.Lin), p.B, CK, p.Lin, M, p.K, p.dil, 0, 0, 0, 0, 0.f);
}

// ---- split-K for row-tile launches whose (M, N) tiling alone leaves most of the 256 CUs idle
// (the discriminator's 1024->1024 k5 conv at L = 32 / 17 / 9, the generator's first transposed
// conv): the contraction is cut into ns channel slices (grid.z), each slice writes a raw partial
// slab into the workspace and k_rows_split_finish sums them in slice order and applies the epilogue.
struct RowSplit {
    int ns, cks;
    size_t out_floats;
};

dim3 rows_grid(int bm, const RowP& p) {
    return dim3(p.R == 1 ? (unsigned)(p.B * p.tiles_per_row) : (unsigned)((p.B + p.R - 1) / p.R),
                (unsigned)((p.M + bm - 1) / bm), (unsigned)((p.CK + p.CKs - 1) / p.CKs));
}

int split_max_wgs() {
    return ms_switch_int("MSYNTH_SPLIT_WGS", 192);   // tuning / test switch (0 disables split-K)
}

RowSplit plan_rows_split(RowCfg cfg, const RowP& p, int CC) {
    RowSplit q;
    q.ns = 1; q.cks = p.CK; q.out_floats = (size_t)p.B * p.M * p.L;
    int bm, bn;
    row_tile(cfg, &bm, &bn);
    const dim3 g = rows_grid(bm, p);
    const int wgs = (int)(g.x * g.y);
    const int nchunks = p.CK / CC;
    // (one workgroup per CU is still under-filled when the contraction is long enough to amortise the
    // slab pass: the 1024 -> 1024 k5 conv at B*L = 2048 has 256 tiles and 64 chunks)
    const int lim = nchunks >= 32 ? (split_max_wgs() * 4) / 3 : split_max_wgs();
    if (wgs > lim || nchunks < 8) return q;
    // slices so that tiles * slices fills the 512 resident workgroup slots (2 per CU) without spilling
    // into a mostly empty second round: 160 tiles x 4 slices = 640 workgroups ran 63 % longer than
    // 128 x 4 = 512 (k5 conv at L = 17 vs 16); 160 x 3 = 480 fits
    int ns = 1;
    double best = 0.0;
    const int ns_max = nchunks / 4 < 16 ? nchunks / 4 : 16;
    for (int c = 1; c <= ns_max; ++c) {
        const int tot = wgs * c, rounds = ms_ceil_div(tot, 512);
        const double eff = (double)tot / (rounds * 512.0);
        if (eff > best + 1e-9) { best = eff; ns = c; }
    }
    while (ns > 1 && (size_t)ns * q.out_floats * sizeof(float) > ((size_t)64 << 20)) --ns;
    if (ns <= 1) return q;
    q.cks = ms_ceil_div(nchunks, ns) * CC;
    if (p.CK % 16 == 0 && q.cks % 16) q.cks += 16 - q.cks % 16;   // slices in whole 16-channel chunks (conv_rows3.hip)
    q.ns = ms_ceil_div(p.CK, q.cks);
    return q;
}

// Paired eight-wave split-bf16 kernel (k_conv_rows3p): rows per workgroup (128 / 64) when the launch should take
// it -- supported and its grid (half as many, twice as wide workgroups) still fills most of the 256 CUs -- else 0.
int rows3p_bm(const Row2P& q, int bn, int K, int am, int epi_s, int in_s, unsigned gz) {
    if (bn != 128) return 0;                     // (q's tiling must be the 128-column one the kernel's groups own)
    constexpr unsigned min_wgs = 128;
    // (C = 256 at L = 256, B = 32: 64 workgroups of 128 rows or 128 of 64 rows both measured slower than the
    //  four-wave kernel's 256 workgroups: 61 / 44 vs 30 us -- no fallback to narrower workgroups)
    const int bm = (q.M >= 128 && K == 3) ? 128 : (q.M <= 32 ? 32 : 64);
    if (!msr3p_supported(bm, K, am, epi_s, q, in_s)) return 0;
    const dim3 g = msr3p_grid(bm, q, gz);
    return (unsigned long long)g.x * g.y * g.z >= min_wgs ? bm : 0;
}

// ... and for the transposed-conv forward (two-tap form, conv_rows3.hip HS): 128 rows where that still fills the chip
int rows3p_convt_bm(const Row2P& q, int bn, int S, unsigned gz) {
    if (bn != 128) return 0;
    constexpr unsigned min_wgs = 128;
    for (int bm = 128; bm >= 64; bm >>= 1) {
        if (q.M < bm || !msr3p_convt_supported(bm, S, q)) continue;
        const dim3 g = msr3p_grid(bm, q, gz);
        if ((unsigned long long)g.x * g.y * g.z >= min_wgs) return bm;
    }
    return 0;
}

Row2P rows3p_retile(const Row2P& q, int K) {
    Row2P r = q;
    r.Lt = 128;
    r.tiles_per_row = (q.L + 127) / 128;
    r.SS = 128 + (K - 1) * q.dil;
    r.RSZ = r.SS;
    r.PX = r.SS;
    return r;
}

// What a row-tile plan depends on besides the geometry: where the call's operands and its workspace sit.  The defaults are
// what the queries plan with: every operand 16-byte aligned (an absent one counts as aligned), the queried workspace present.
struct RowCall {
    bool x16 = true, xact16 = true, w16 = true, res16 = true, y16 = true, yact16 = true;
    bool ws = true, ws16 = true;
    size_t ws_bytes = ~(size_t)0;
};

RowCall row_call(const float* x, const float* xact, const float* w, const float* res, const float* y, const float* yact,
                 const void* ws, size_t ws_bytes) {
    RowCall c;
    c.x16 = al16(x); c.xact16 = al16(xact); c.w16 = al16(w); c.res16 = al16(res); c.y16 = al16(y); c.yact16 = al16(yact);
    c.ws = ws != nullptr; c.ws16 = al16(ws); c.ws_bytes = ws_bytes;
    return c;
}

struct RowPlan {
    enum Fam { IGEMM, ROWS1, ROWS2, ROWS3, ROWS3P, ROWS3P_T } fam = IGEMM;   // k_igemm_conv, k_conv_mfma_rows, k_conv_rows2 / 3 / 3p
    enum Pack { PACK_NONE, FLIP_W, PACK_T, PACK_T2, PACK_TB, PACK_TB2 } pack = PACK_NONE;   // weight re-layout kernel in front
    Cfg icfg = CFG_64x64;      // IGEMM: its tile
    RowCfg cfg = ROW_64x64;    // the row tile; tile: its MSR2_* name; bmp: rows per workgroup of the paired kernels
    int tile = 0, bmp = 0;
    int K = 0, CC = 0;         // taps and channels per chunk the kernel is instantiated for
    bool has_act = false;      // an activation operand rides along (Xact)
    int am = 0, epi_s = 0, in_s = 1;   // act_mode of conv_rows2.h, phase-interleaving epilogue, phase-split input (0: whole short rows)
    RowP r;                    // the rows, split applied (CKs, zstride, act = NONE)
    Row2P q;                   // the same for the pipelined kernels (the paired ones: retiled to 128 columns where needed)
    int ns = 1;                // split-K slices (grid.z), each a raw slab of out_floats
    size_t out_floats = 0;
    int act = 0, nch = 0, rowlen = 0;   // epilogue of the slab sum: activation, bias index
    dim3 grid;
    size_t wbytes = 0, bytes = 0;       // workspace: [re-laid-out weights | slabs]; bytes: all of it, the query's answer
};

// One row-tile launch decided once.  r0: the rows before any split.  K: taps of the window; conv_t: a transposed-conv pass
// (K = 3, single chunks; its pipelined kernels multiply only the two live taps of each phase), pair_t: its forward, which the
// paired split-bf16 kernel takes.  wbytes: re-laid-out weights in front of the workspace (the kernel's W operand, unless act_mode 1
// reads the forward layout: wfwd says the call has it).
RowPlan plan_rows(RowCfg cfg, const RowP& r0, int K, bool has_act, int epi_s, int in_s, bool conv_t, bool pair_t,
                  size_t wbytes, bool wfwd, int nch, int rowlen, const RowCall& c) {
    RowPlan pl;
    pl.fam = RowPlan::ROWS1; pl.cfg = cfg; pl.r = r0; pl.has_act = has_act; pl.epi_s = epi_s; pl.in_s = in_s;
    pl.K = K; pl.CC = conv_t ? row_cc(K) : rows_cc_eff(K, r0.CK);
    pl.act = r0.act; pl.nch = nch; pl.rowlen = rowlen; pl.wbytes = wbytes;
    int bm, bn;
    row_tile(cfg, &bm, &bn);
    // split-K where the workspace passed has room for the slabs
    const RowSplit sp = plan_rows_split(cfg, r0, pl.CC);
    const size_t slabs = sp.ns > 1 ? (size_t)sp.ns * sp.out_floats * sizeof(float) : 0;
    pl.out_floats = sp.out_floats;
    pl.bytes = wbytes + slabs;
    bool out16 = c.y16 && c.yact16 && c.res16;
    if (slabs && c.ws && c.ws_bytes >= pl.bytes) {
        pl.ns = sp.ns;
        pl.r.CKs = sp.cks; pl.r.zstride = (long long)sp.out_floats; pl.r.act = MS_ACT_NONE;
        out16 = c.ws16;              // (the kernel writes raw slabs; bias, residual and y_act belong to the slab sum)
    }
    const RowP& p = pl.r;
    pl.grid = rows_grid(bm, p);
    // Does the launch go to the pipelined kernels (conv_rows2.hip, conv_rows3.hip)?  16-byte aligned operands, zero padding,
    // plain input rows, activation handling they know; backward data additionally needs the forward-layout weights, which
    // act_mode 1 reads directly.  Fills q, tile, am, in_s.
    auto pipelined = [&](int K2, int CC2) {
        pl.in_s = in_s;
        if (p.pad_mode != MS_PAD_ZERO || cfg == ROW_64x256) return false;
        if (has_act && p.in_act != MS_ACT_LRELU && p.in_act != MS_ACT_NONE && p.in_act != MS_MOD_LRELU_FWD) return false;
        int am = (has_act && p.in_act == MS_ACT_LRELU) ? (in_s == 1 ? 1 : 2) : 0;
        if (has_act && p.in_act == MS_MOD_LRELU_FWD) am = 3;      // LeakyReLU in front of the conv, on load
        pl.am = am;
        if (in_s != 1 && am != 2 && am != 0) return false;
        if (am == 1 && (!wfwd || p.M % 4)) return false;
        if (!(c.x16 && c.xact16 && out16 && ((am == 1 || !wbytes) ? c.w16 : c.ws16))) return false;
        if ((long long)p.B * p.CK * p.L >= (1LL << 31) || (long long)p.M * p.KG >= (1LL << 31)) return false;
        Row2P& q = pl.q;
        q.B = p.B; q.CK = p.CK; q.L = p.L; q.M = p.M; q.dil = p.dil; q.off0 = p.off0; q.act = p.act;
        q.KG = p.KG; q.Lt = p.Lt; q.R = p.R; q.SS = p.SS; q.RSZ = p.RSZ; q.tiles_per_row = p.tiles_per_row;
        q.PX = p.RSZ; q.CKs = p.CKs; q.zstride = p.zstride; q.slope = p.slope; q.scratch_off = 0;
        pl.tile = cfg == ROW_128x128 ? MSR2_128x128 : (cfg == ROW_64x128 ? MSR2_64x128 :
                  (cfg == ROW_64x64 ? MSR2_64x64 : MSR2_32x256));
        if (in_s == 1 && msr3_supported(pl.tile, K2, am, epi_s, q, 1)) return true;   // split-bf16 kernel: rows of any length
        // short rows of a length that is not a multiple of 4 (k5 conv at L = 17 / 9): whole-row staging
        if (in_s == 1 && K2 == 5 && p.tiles_per_row == 1 && p.Lt == p.L && p.L < bn && p.L % 4 != 0 &&
            msr2_supported(pl.tile, K2, CC2, am, epi_s, q, 0)) {
            pl.in_s = 0;
            return true;
        }
        return msr3_supported(pl.tile, K2, am, epi_s, q, in_s) || msr2_supported(pl.tile, K2, CC2, am, epi_s, q, in_s);
    };
    if (conv_t && pipelined(2, 8)) {       // the 3-tap window stays, only the two live taps of each phase are multiplied
        pl.fam = RowPlan::ROWS2; pl.K = 2; pl.CC = 8;
        pl.q.KG = p.CK * 2;
        if (pair_t) {                      // paired split-bf16 kernel where its grid fills the chip
            if (const int b3 = rows3p_convt_bm(pl.q, bn, epi_s, pl.grid.z)) {
                pl.fam = RowPlan::ROWS3P_T; pl.bmp = b3;
                pl.grid = msr3p_grid(b3, pl.q, pl.grid.z);
            }
        }
    } else if (pipelined(K, pl.CC)) {
        int bmp = rows3p_bm(pl.q, bn, K, pl.am, epi_s, pl.in_s, pl.grid.z);
        if (!bmp && cfg == ROW_32x256 && pl.q.R == 1 && pl.q.Lt == 256) {      // 32-channel layers: the same rows as 128-column tiles
            const Row2P q2 = rows3p_retile(pl.q, K);
            if ((bmp = rows3p_bm(q2, 128, K, pl.am, epi_s, pl.in_s, pl.grid.z)) != 0) pl.q = q2;
        }
        if (bmp) {
            pl.fam = RowPlan::ROWS3P; pl.bmp = bmp;
            pl.grid = msr3p_grid(bmp, pl.q, pl.grid.z);
        } else {
            // split-bf16 matrix pipe (conv_rows3.hip) before the fp32 one
            pl.fam = msr3_supported(pl.tile, K, pl.am, epi_s, pl.q, pl.in_s) ? RowPlan::ROWS3 : RowPlan::ROWS2;
        }
    } else {
        pl.am = 0; pl.in_s = in_s;
    }
    return pl;
}

struct RowOps {
    const float *X, *Xact, *W, *Wfwd, *bias, *res;   // W: the layout the plan's pack kernel wrote (or the call's own); Wfwd: act_mode 1
    float *Y, *Yact;
};

template <int K, int CC, bool HAS_ACT, int EPI_S, int IN_S>
int launch_rows1_k(const RowPlan& pl, const RowOps& o, hipStream_t s, char* name) {
    const RowP& p = pl.r;
    int bm, bn;
    row_tile(pl.cfg, &bm, &bn);
    const size_t lds = (size_t)(bm * (CC * K + 1) + CC * p.RSZ) * sizeof(float);
    if (lds > 64 * 1024) return MS_ERR_UNSUPPORTED;
#define MS_R1(WGM, WGN, TM, TN)                                                                                         \
    do {                                                                                                                \
        if (ms_name_or_note(name, 0, "k_conv_mfma_rows<%d, %d, %d, %d, %d, %d, %s, %d, %d>", WGM, WGN, TM, TN, K, CC,     \
                            HAS_ACT ? "true" : "false", EPI_S, IN_S))                                                   \
            return MS_OK;                                                                                               \
        hipLaunchKernelGGL((k_conv_mfma_rows<WGM, WGN, TM, TN, K, CC, HAS_ACT, EPI_S, IN_S>), pl.grid, dim3(256), lds, s, \
                           p, o.X, o.Xact, o.W, o.bias, o.res, o.Y, o.Yact);                                            \
    } while (0)
    switch (pl.cfg) {
        case ROW_128x128: MS_R1(2, 2, 2, 2); break;
        case ROW_64x128: MS_R1(2, 2, 1, 2); break;
        case ROW_64x64: MS_R1(2, 2, 1, 1); break;
        case ROW_64x256: MS_R1(1, 4, 2, 2); break;
        default: MS_R1(1, 4, 1, 2); break;
    }
#undef MS_R1
    MS_CHECK_LAUNCH();
    return MS_OK;
}

// first-generation kernel of a plan: the instantiations that exist
int launch_rows1(const RowPlan& pl, const RowOps& o, hipStream_t s, char* name) {
    const int K = pl.K, CC = pl.CC;
#define MS_R1K(KK, C, E, I)                                                               \
    if (K == KK && CC == C && pl.epi_s == E && pl.in_s == I)                              \
        return pl.has_act ? launch_rows1_k<KK, C, true, E, I>(pl, o, s, name)             \
                          : launch_rows1_k<KK, C, false, E, I>(pl, o, s, name)
    MS_R1K(1, 32, 0, 1);
    MS_R1K(3, 8, 0, 1);
    MS_R1K(3, 16, 0, 1);
    MS_R1K(5, 8, 0, 1);
    MS_R1K(5, 16, 0, 1);
    MS_R1K(7, 4, 0, 1);
    MS_R1K(3, 8, 8, 1);      // transposed-conv forward: phase-interleaving epilogue
    MS_R1K(3, 8, 4, 1);
    MS_R1K(3, 8, 2, 1);
#undef MS_R1K
    if (K == 3 && CC == 8 && pl.epi_s == 0 && pl.has_act) {      // transposed-conv backward data: phase-split input rows
        if (pl.in_s == 8) return launch_rows1_k<3, 8, true, 0, 8>(pl, o, s, name);
        if (pl.in_s == 4) return launch_rows1_k<3, 8, true, 0, 4>(pl, o, s, name);
        if (pl.in_s == 2) return launch_rows1_k<3, 8, true, 0, 2>(pl, o, s, name);
    }
    return MS_ERR_UNSUPPORTED;
}

// Runs the row-tile launch of a plan, then the slab sum of a split one.  slabs: the workspace behind the re-laid-out weights.
int run_rows(const RowPlan& pl, const RowOps& o, float* slabs, hipStream_t s, char* name) {
    RowOps k = o;          // the kernel's operands: a split launch writes raw slabs, its epilogue belongs to the slab sum
    if (pl.ns > 1) { k.bias = nullptr; k.res = nullptr; k.Y = slabs; k.Yact = nullptr; }
    const float* W = pl.am == 1 ? o.Wfwd : o.W;
    int rc;
    switch (pl.fam) {
        case RowPlan::ROWS3P:
            rc = msr3p_launch(pl.bmp, pl.K, pl.am, pl.q, k.X, k.Xact, W, k.bias, k.res, k.Y, k.Yact, pl.grid, s, name);
            break;
        case RowPlan::ROWS3P_T:
            rc = msr3p_convt_launch(pl.bmp, pl.epi_s, pl.am == 3, pl.q, k.X, W, k.bias, k.Y, pl.grid, s, name);
            break;
        case RowPlan::ROWS3:
            rc = msr3_launch(pl.tile, pl.K, pl.am, pl.q, k.X, k.Xact, W, k.bias, k.res, k.Y, k.Yact, pl.grid, s, name);
            break;
        case RowPlan::ROWS2:
            rc = msr2_launch(pl.tile, pl.K, pl.CC, pl.am, pl.epi_s, pl.q, k.X, k.Xact, W, k.bias, k.res, k.Y, k.Yact, pl.grid, s,
                             pl.in_s, name);
            break;
        default: rc = launch_rows1(pl, k, s, name); break;
    }
    if (rc != MS_OK || name || pl.ns <= 1) return rc;
    hipLaunchKernelGGL(k_rows_split_finish, blocks256(pl.out_floats, 2048), dim3(256), 0, s, slabs, pl.ns, pl.out_floats,
                       o.bias, pl.nch, pl.rowlen, pl.act, pl.r.slope, o.res, o.Y, o.Yact, pl.out_floats);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

// ---- the planners, one per pass
// x_act_kind: operand-modifier kind of the activation operand (0: none rides along)
RowPlan plan_fwd(const ConvP& p, bool has_act, int x_act_kind, const RowCall& c) {
    if (rows_ok(p, false) && c.w16) {
        RowP r;
        const RowCfg cfg = pick_row_cfg(p.Cout, p.B, p.Lin, p.K == 3 || p.K == 5);
        make_rowp(&r, cfg, p.B, p.Cin, p.Lin, p.Cout, p.K, p.dil, -p.pad, p.pad_mode, p.act, x_act_kind, p.slope);
        return plan_rows(cfg, r, p.K, has_act, 0, 1, false, false, 0, false, p.Cout, p.Lin, c);
    }
    RowPlan pl;
    pl.icfg = pick_cfg(p.Cout, (long long)p.B * p.Lin);
    return pl;
}

// has_act: y_act rides along.  The row tiles need the whole workspace (re-laid-out weights | slabs) at a 16-byte address.
RowPlan plan_bwd_data(const ConvP& p, bool has_act, const RowCall& c) {
    if (rows_ok(p, true)) {
        RowP r;
        const RowCfg cfg = pick_row_cfg(p.Cin, p.B, p.Lin, p.K == 3 || p.K == 5);
        make_rowp(&r, cfg, p.B, p.Cout, p.Lin, p.Cin, p.K, p.dil, p.pad - (p.K - 1) * p.dil, MS_PAD_ZERO, MS_ACT_NONE, p.act,
                  p.slope);
        RowPlan pl = plan_rows(cfg, r, p.K, has_act, 0, 1, false, false, align16((size_t)p.Cin * p.Cout * p.K * sizeof(float)),
                               true, p.Cin, p.Lin, c);
        // the pipelined kernels read the forward layout directly (act_mode 1); the others get it transposed + tap-flipped
        pl.pack = pl.fam != RowPlan::ROWS1 && pl.am == 1 ? RowPlan::PACK_NONE : RowPlan::FLIP_W;
        if (c.ws && c.ws16 && c.ws_bytes >= pl.bytes) return pl;
    }
    RowPlan pl;
    pl.icfg = pick_cfg(p.Cin, (long long)p.B * p.Lin);
    return pl;
}

// p = mirrored conv of the transposed conv: Cin_T = p.Cout, Cout_T = p.Cin, Lin_T = p.Lout.  The activation operand of the
// forward is x itself (LeakyReLU in front, applied on load).
RowPlan plan_convt_fwd(const ConvP& p, const RowCall& c) {
    const int S = p.stride;
    RowP r;
    const RowCfg cfg = convt_fwd_cfg(p.Cin * S, p.B, p.Lout);
    make_rowp(&r, cfg, p.B, p.Cout, p.Lout, p.Cin * S, 3, 1, -1, MS_PAD_ZERO, p.act, p.in_act ? MS_MOD_LRELU_FWD : MS_ACT_NONE,
              p.slope);
    RowPlan pl = plan_rows(cfg, r, 3, p.in_act != 0, S, 1, true, true, align16((size_t)p.Cin * S * p.Cout * 3 * sizeof(float)),
                           false, p.Cin, p.Lout * S, c);
    pl.pack = pl.K == 2 ? RowPlan::PACK_T2 : RowPlan::PACK_T;
    return pl;
}

// gx_T = conv over the phase-split gradient: M = Cin_T, channels (co, r), 3 taps.  has_act: y_act rides along (else the
// activation operand aliases the data, pass-through kind)
RowPlan plan_convt_bwd_data(const ConvP& p, bool has_act, const RowCall& c) {
    const int S = p.stride;
    RowP r;
    const RowCfg cfg = pick_row_cfg(p.Cout, p.B, p.Lout);
    make_rowp(&r, cfg, p.B, p.Cin * S, p.Lout, p.Cout, 3, 1, -1, MS_PAD_ZERO, MS_ACT_NONE, has_act ? p.act : MS_ACT_NONE, p.slope);
    RowPlan pl = plan_rows(cfg, r, 3, true, 0, S, true, false, align16((size_t)p.Cout * p.Cin * S * 3 * sizeof(float)), false,
                           p.Cout, p.Lout, c);
    pl.pack = pl.K == 2 ? RowPlan::PACK_TB2 : RowPlan::PACK_TB;
    return pl;
}

// runs a forward / backward-data plan that fell to the im2col kernel
template <bool TRANS>
int run_igemm(const RowPlan& pl, const ConvP& p, int in_act, const RowOps& o, hipStream_t s, char* name) {
    IgP q;
    q.B = p.B; q.CK = TRANS ? p.Cout : p.Cin; q.L = p.Lin; q.M = TRANS ? p.Cin : p.Cout; q.dil = p.dil;
    q.off0 = TRANS ? p.pad - (p.K - 1) * p.dil : -p.pad;   // backward data: flipped taps, j' = K-1-j
    q.pad_mode = TRANS ? (int)MS_PAD_ZERO : p.pad_mode; q.act = TRANS ? (int)MS_ACT_NONE : p.act; q.in_act = in_act;
    q.slope = p.slope; q.N = p.B * p.Lin; q.KG = q.CK * p.K; q.in_s = 1;
    return launch_conv<TRANS>(p.K, pl.icfg, q, o.X, o.Xact, o.W, o.bias, o.res, o.Y, o.Yact, s, name);
}

int run_fwd(const RowPlan& pl, const ConvP& p, int x_act_kind, const RowOps& o, void* ws, hipStream_t s, char* name) {
    if (pl.fam == RowPlan::IGEMM) return run_igemm<false>(pl, p, x_act_kind, o, s, name);
    return run_rows(pl, o, (float*)ws, s, name);
}

int run_bwd_data(const RowPlan& pl, const ConvP& p, RowOps o, void* ws, hipStream_t s, char* name) {
    if (pl.fam == RowPlan::IGEMM) return run_igemm<true>(pl, p, p.act, o, s, name);
    float* wt = (float*)ws;
    if (pl.pack == RowPlan::FLIP_W && !name) {
        hipLaunchKernelGGL(k_transpose_flip_w, blocks256((size_t)p.Cin * p.Cout * p.K, 2048), dim3(256), 0, s, o.Wfwd, wt, p.Cout,
                           p.Cin, p.K);
        MS_CHECK_LAUNCH();
    }
    o.W = wt;
    return run_rows(pl, o, (float*)((char*)ws + pl.wbytes), s, name);
}

// both transposed passes: the plan's pack kernel writes the phase-split weights to the front of the workspace
int run_convt(const RowPlan& pl, const ConvP& p, RowOps o, const float* w, void* ws, hipStream_t s, char* name) {
    float* wp = (float*)ws;
    if (!name) {
        const int S = p.stride, CinT = p.Cout, CoutT = p.Cin;
        const dim3 nb = blocks256((size_t)CinT * CoutT * S * 3, 4096);
        if (pl.pack == RowPlan::PACK_T2) hipLaunchKernelGGL(k_pack_convt_w2, nb, dim3(256), 0, s, w, wp, CinT, CoutT, p.K, S, p.pad);
        else if (pl.pack == RowPlan::PACK_T) hipLaunchKernelGGL(k_pack_convt_w, nb, dim3(256), 0, s, w, wp, CinT, CoutT, p.K, S, p.pad);
        else if (pl.pack == RowPlan::PACK_TB2) hipLaunchKernelGGL(k_pack_convt_bwd_w2, nb, dim3(256), 0, s, w, wp, CinT, CoutT, p.K, S, p.pad);
        else hipLaunchKernelGGL(k_pack_convt_bwd_w, nb, dim3(256), 0, s, w, wp, CinT, CoutT, p.K, S, p.pad);
        MS_CHECK_LAUNCH();
    }
    o.W = wp;
    return run_rows(pl, o, (float*)((char*)ws + pl.wbytes), s, name);
}

IgP wgrad_igp(const ConvP& p) {
    IgP q;
    q.B = p.B; q.CK = p.Cin; q.L = p.Lin; q.M = p.Cout; q.dil = p.dil; q.off0 = -p.pad;
    q.pad_mode = p.pad_mode; q.act = MS_ACT_NONE; q.in_act = 0; q.slope = p.slope;
    q.N = p.B * p.Lin; q.KG = p.Cin * p.K; q.in_s = 1;
    return q;
}

bool wgrad_v4(const ConvP& p, bool aligned) { return p.Lin % 4 == 0 && p.pad_mode == MS_PAD_ZERO && aligned; }

struct ConvtWgradPlan {
    WgradPlan w;
    IgP q;
    size_t dwq_floats;
};

ConvtWgradPlan plan_convt_wgrad(const ConvP& p) {
    // weight-grad GEMM: M = Cin_T, N = Cout_T * S * 3, K = B * Lin_T
    ConvP m = p;
    m.Cout = p.Cout;                 // rows: x_T channels
    m.Cin = p.Cin * p.stride;        // (co, r) phase channels
    m.K = 3; m.Lin = p.Lout; m.Lout = p.Lout; m.stride = 1; m.pad = 1; m.dil = 1;
    m.pad_mode = MS_PAD_ZERO;
    ConvtWgradPlan q;
    q.w = plan_wgrad(m);
    q.q = wgrad_igp(m);
    q.q.in_act = p.act; q.q.in_s = p.stride;
    q.dwq_floats = (size_t)p.Cout * m.Cin * 3 + p.Cout;
    return q;
}

// what a name query hands out: the spelling its plan's launcher wrote, in a buffer of the calling thread
const char* named(int rc, const char* buf) { return rc == MS_OK ? buf : ""; }

}  // namespace

bool msm_fwd_applicable(const ConvP& p) {
    return dense_same(p) && (p.Cout >= 32 || p.Cin >= 256) && p.Cin * p.K >= 32;
}
bool msm_bwd_data_applicable(const ConvP& p) {
    return dense_same(p) && p.pad_mode == MS_PAD_ZERO && p.Cin >= 32 && p.Cout * p.K >= 32;
}
bool msm_bwd_weight_applicable(const ConvP& p) {
    const bool kok = p.K == 1 || p.K == 3 || p.K == 5 || p.K == 7 || p.K == 15;
    return p.groups == 1 && p.stride == 1 && p.Lout == p.Lin && kok &&
           (long long)p.B * p.Lin < (1LL << 31) && (long long)p.B * p.Cout * p.Lin < (1LL << 31) &&
           (long long)p.B * p.Cin * p.Lin < (1LL << 31) && p.Cout >= 16 && p.Cin * p.K >= 15;
}
// p = mirrored conv of the transposed conv: Cin_T = p.Cout, Cout_T = p.Cin, Lin_T = p.Lout
bool msm_convt_fwd_applicable(const ConvP& p) {
    const int S = p.stride;
    if (!ms_convt_phase_stride(S) || p.K != 2 * S || 2 * p.pad != S || p.dil != 1 || p.groups != 1) return false;
    if (p.Cout % 8 || p.Cin < 32 || (p.Cin * S) % 32) return false;
    if ((long long)p.B * p.Lin >= (1LL << 31)) return false;
    RowP q;
    return make_rowp(&q, convt_fwd_cfg(p.Cin * S, p.B, p.Lout), p.B, p.Cout, p.Lout, p.Cin * S, 3, 1, -1, 0, 0, 0, 0.f);
}

// ---- the queries: the plan of a call with 16-byte aligned operands and the queried workspace; a forward's activation operand
// is the descriptor's in_act, a backward pass has y_act where the layer has an activation
size_t msm_fwd_ws(const ConvP& p) { return plan_fwd(p, p.in_act != 0, p.in_act ? MS_MOD_LRELU_FWD : 0, RowCall()).bytes; }
size_t msm_bwd_data_ws(const ConvP& p) { return plan_bwd_data(p, p.act != MS_ACT_NONE, RowCall()).bytes; }
size_t msm_bwd_weight_ws(const ConvP& p) {
    const WgradPlan q = plan_wgrad(p);
    return (size_t)q.nsplit * q.stride_floats * sizeof(float);
}
size_t msm_convt_fwd_ws(const ConvP& p) { return plan_convt_fwd(p, RowCall()).bytes; }

const char* msm_fwd_name(const ConvP& p, int x_act_kind) {
    static thread_local char buf[MS_PROFILE_NAME_MAX];
    return named(run_fwd(plan_fwd(p, x_act_kind != 0, x_act_kind, RowCall()), p, x_act_kind, RowOps(), nullptr, nullptr, buf), buf);
}
const char* msm_fwd_name(const ConvP& p) { return msm_fwd_name(p, p.in_act ? MS_MOD_LRELU_FWD : 0); }
const char* msm_bwd_data_name(const ConvP& p) {
    static thread_local char buf[MS_PROFILE_NAME_MAX];
    return named(run_bwd_data(plan_bwd_data(p, p.act != MS_ACT_NONE, RowCall()), p, RowOps(), nullptr, nullptr, buf), buf);
}
const char* msm_bwd_weight_name(const ConvP& p) {
    static thread_local char buf[MS_PROFILE_NAME_MAX];
    return named(launch_wgrad(plan_wgrad(p), p.K, wgrad_v4(p, true), wgrad_igp(p), nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                              nullptr, buf), buf);
}
const char* msm_convt_fwd_name(const ConvP& p) {
    static thread_local char buf[MS_PROFILE_NAME_MAX];
    return named(run_convt(plan_convt_fwd(p, RowCall()), p, RowOps(), nullptr, nullptr, nullptr, buf), buf);
}

int msm_conv1d_fwd(const ConvP& p, const float* x, const float* x_act, int x_act_kind,
                   const float* w, const float* bias, const float* residual, float* y,
                   float* y_act, void* ws, size_t ws_bytes, hipStream_t s) {
    const RowPlan pl = plan_fwd(p, x_act != nullptr, x_act_kind, row_call(x, x_act, w, residual, y, y_act, ws, ws_bytes));
    return run_fwd(pl, p, x_act_kind, RowOps{x, x_act, w, nullptr, bias, residual, y, y_act}, ws, s, nullptr);
}

int msm_conv1d_bwd_data(const ConvP& p, const float* gy, const float* y_act, const float* w,
                        const float* gx_add, float* gx, void* ws, size_t ws_bytes, hipStream_t s) {
    const RowPlan pl = plan_bwd_data(p, y_act != nullptr, row_call(gy, y_act, w, gx_add, gx, nullptr, ws, ws_bytes));
    return run_bwd_data(pl, p, RowOps{gy, y_act, w, w, nullptr, gx_add, gx, nullptr}, ws, s, nullptr);
}

int msm_conv1d_bwd_weight(const ConvP& p, const float* x, const float* x_act, int x_act_kind,
                          const float* gy, const float* y_act, int y_act_kind, float* gw,
                          float* gb, float beta, void* ws, size_t ws_bytes, hipStream_t s) {
    const WgradPlan pl = plan_wgrad(p);
    const size_t need = (size_t)pl.nsplit * pl.stride_floats * sizeof(float);
    if (!ws || ws_bytes < need) return MS_ERR_WORKSPACE;
    IgP q = wgrad_igp(p);
    q.in_act = x_act_kind;
    float* partial = (float*)ws;
    const int rc = launch_wgrad(pl, p.K, wgrad_v4(p, al16(x) && al16(gy) && al16(y_act)), q, x, x_act, gy, y_act, y_act_kind,
                                partial, s, nullptr);
    if (rc != MS_OK) return rc;
    return msm_wgrad_reduce(partial, pl.stride_floats, pl.nsplit, (size_t)p.Cout * q.KG, p.Cout, gw, gb, beta, s);
}

int msm_convt1d_fwd(const ConvP& p, const float* x, const float* w, const float* bias, float* y,
                    void* ws, size_t ws_bytes, hipStream_t s) {
    if (!al16(y)) return MS_ERR_UNSUPPORTED;      // (phase-interleaved epilogue: 8- / 16-byte stores to y)
    const float* xa = p.in_act ? x : nullptr;     // LeakyReLU in front of the transposed conv: applied to x on load
    const RowPlan pl = plan_convt_fwd(p, row_call(x, xa, w, nullptr, y, nullptr, ws, ws_bytes));
    if (!ws || ws_bytes < pl.bytes || !al16(ws)) return MS_ERR_WORKSPACE;
    return run_convt(pl, p, RowOps{x, xa, nullptr, nullptr, bias, nullptr, y, nullptr}, w, ws, s, nullptr);
}

// ---- ConvTranspose1d backward (p = mirrored conv: Cin_T = p.Cout, Cout_T = p.Cin, Lin_T = p.Lout)
bool msm_convt_bwd_applicable(const ConvP& p) {
    const int S = p.stride;
    if (!ms_convt_phase_stride(S) || p.K != 2 * S || 2 * p.pad != S || p.dil != 1 || p.groups != 1) return false;
    if (p.Cout < 32 || p.Cin % 8 || (p.Cin * S) % 8) return false;
    if ((long long)p.B * p.Cin * p.Lin >= (1LL << 31) || (long long)p.B * p.Cout * p.Lout >= (1LL << 31)) return false;
    RowP q;
    return make_rowp(&q, pick_row_cfg(p.Cout, p.B, p.Lout), p.B, p.Cin * S, p.Lout, p.Cout, 3, 1, -1, 0, 0, 0, 0.f);
}

size_t msm_convt_bwd_data_ws(const ConvP& p) { return plan_convt_bwd_data(p, p.act != MS_ACT_NONE, RowCall()).bytes; }

const char* msm_convt_bwd_data_name(const ConvP& p) {
    static thread_local char buf[MS_PROFILE_NAME_MAX];
    return named(run_convt(plan_convt_bwd_data(p, p.act != MS_ACT_NONE, RowCall()), p, RowOps(), nullptr, nullptr, nullptr, buf), buf);
}

int msm_convt1d_bwd_data(const ConvP& p, const float* gy, const float* y_act, const float* w,
                         float* gx, void* ws, size_t ws_bytes, hipStream_t s) {
    const float* ya = y_act ? y_act : gy;
    const RowPlan pl = plan_convt_bwd_data(p, y_act != nullptr, row_call(gy, ya, w, nullptr, gx, nullptr, ws, ws_bytes));
    if (!ws || ws_bytes < pl.bytes || !al16(ws)) return MS_ERR_WORKSPACE;
    return run_convt(pl, p, RowOps{gy, ya, nullptr, nullptr, nullptr, nullptr, gx, nullptr}, w, ws, s, nullptr);
}

// workspace: [dWq | split-K slabs of whichever kernel takes the launch]
size_t msm_convt_bwd_weight_ws(const ConvP& p) {
    const ConvtWgradPlan q = plan_convt_wgrad(p);
    size_t slabs = (size_t)q.w.nsplit * q.w.stride_floats * sizeof(float);
    const size_t rows = msw_convt_ws(p);
    if (rows > slabs) slabs = rows;
    return align16(q.dwq_floats * sizeof(float)) + slabs;
}

const char* msm_convt_bwd_weight_name(const ConvP& p) {
    static thread_local char buf[MS_PROFILE_NAME_MAX];
    if (msw_convt_ws(p) > 0 && p.act != MS_ACT_TANH) {
        snprintf(buf, sizeof(buf), "k_wgrad_rows<3, %d, true, %d, 3, %d>", p.Cout >= 128 ? 2 : 1, p.Lout <= 32 ? 8 : 16, p.stride);
        return buf;
    }
    const ConvtWgradPlan pl = plan_convt_wgrad(p);
    return named(launch_wgrad(pl.w, 3, false, pl.q, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, buf), buf);
}

// gw_T via the phase-split weight-grad GEMM, then un-packed into (Cin_T, Cout_T, K)
int msm_convt1d_bwd_weight(const ConvP& p, const float* x, const float* gy, const float* y_act,
                           float* gw, float beta, void* ws, size_t ws_bytes, hipStream_t s) {
    const int S = p.stride, CinT = p.Cout, CoutT = p.Cin;
    const ConvtWgradPlan pl = plan_convt_wgrad(p);
    if (!ws || ws_bytes < msm_convt_bwd_weight_ws(p)) return MS_ERR_WORKSPACE;
    float* dwq = (float*)ws;
    const size_t dbytes = align16(pl.dwq_floats * sizeof(float));
    float* partial = (float*)((char*)ws + dbytes);
    // row-tile form (wgrad_rows.hip) where it applies; the im2col form below otherwise
    int rc = msw_convt_dwq(p, x, gy, y_act, dwq, partial, ws_bytes - dbytes, s);
    if (rc != MS_OK) {
        // A operand = x_T (no activation), B operand = phase-split gy with act'(y_T)
        rc = launch_wgrad(pl.w, 3, false, pl.q, gy, y_act, x, p.in_act ? x : nullptr, p.in_act ? MS_MOD_LRELU_FWD : 0, partial, s,
                          nullptr);
        if (rc == MS_OK)
            rc = msm_wgrad_reduce(partial, pl.w.stride_floats, pl.w.nsplit, (size_t)CinT * pl.q.KG, CinT, dwq, nullptr, 0.f, s);
        if (rc != MS_OK) return rc;
    }
    hipLaunchKernelGGL(k_unpack_convt_gw, blocks256((size_t)CinT * CoutT * p.K, 4096), dim3(256), 0, s, dwq, gw, CinT, CoutT, p.K,
                       S, p.pad, beta);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

// 16-byte variant: a lane owns 4 consecutive outputs, 8 slabs in flight per lane (the dword version is
// latency-bound: 30 dependent-ish rounds of 4 loads for the 121 slabs of a 128-channel layer).
__global__ __launch_bounds__(256) void k_wgrad_reduce_v4(const float* __restrict__ partial,
                                                        size_t partial_stride, int nsplit,
                                                        size_t wsize, size_t total,
                                                        float* __restrict__ out,
                                                        float* __restrict__ outb, float beta) {
    __shared__ float4 red[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t i = ((size_t)blockIdx.x * 64 + lane) * 4;
    const bool ok = i < total;                       // total % 4 == 0
    float4 s[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
        int z = wv;
        for (; z + 28 < nsplit; z += 32) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                v[u] = *reinterpret_cast<const float4*>(partial + (size_t)(z + 4 * u) * partial_stride + i);
#pragma unroll
            for (int u = 0; u < 8; ++u) { s[u].x += v[u].x; s[u].y += v[u].y; s[u].z += v[u].z; s[u].w += v[u].w; }
        }
        for (; z < nsplit; z += 4) {
            const float4 v = *reinterpret_cast<const float4*>(partial + (size_t)z * partial_stride + i);
            s[0].x += v.x; s[0].y += v.y; s[0].z += v.z; s[0].w += v.w;
        }
    }
    float4 t;
    t.x = ((s[0].x + s[1].x) + (s[2].x + s[3].x)) + ((s[4].x + s[5].x) + (s[6].x + s[7].x));
    t.y = ((s[0].y + s[1].y) + (s[2].y + s[3].y)) + ((s[4].y + s[5].y) + (s[6].y + s[7].y));
    t.z = ((s[0].z + s[1].z) + (s[2].z + s[3].z)) + ((s[4].z + s[5].z) + (s[6].z + s[7].z));
    t.w = ((s[0].w + s[1].w) + (s[2].w + s[3].w)) + ((s[4].w + s[5].w) + (s[6].w + s[7].w));
    red[wv][lane] = t;
    __syncthreads();
    if (wv == 0 && ok) {
        float4 r;
        r.x = (red[0][lane].x + red[1][lane].x) + (red[2][lane].x + red[3][lane].x);
        r.y = (red[0][lane].y + red[1][lane].y) + (red[2][lane].y + red[3][lane].y);
        r.z = (red[0][lane].z + red[1][lane].z) + (red[2][lane].z + red[3][lane].z);
        r.w = (red[0][lane].w + red[1][lane].w) + (red[2][lane].w + red[3][lane].w);
        // (wsize % 4 == 0: a vector is all weights or all bias; the bias entries follow the weights in a slab)
        if (i >= wsize && !outb) return;
        float4* o = i < wsize ? reinterpret_cast<float4*>(out + i) : reinterpret_cast<float4*>(outb + (i - wsize));
        if (beta != 0.f) {
            const float4 p = *o;
            r.x += beta * p.x; r.y += beta * p.y; r.z += beta * p.z; r.w += beta * p.w;
        }
        *o = r;
    }
}

int msm_wgrad_reduce(const float* partial, size_t stride_floats, int nsplit, size_t wsize, int nbias,
                     float* gw, float* gb, float beta, hipStream_t s) {
    const size_t total = wsize + (size_t)nbias;
    // weights with 16-byte accesses where the layout allows it, the bias tail with the dword kernel
    if (wsize % 4 == 0 && stride_floats % 4 == 0 &&
        ((((uintptr_t)partial) | ((uintptr_t)gw)) & 15) == 0) {
        // the bias tail rides along when it is 16-byte sized and aligned too (one launch instead of two)
        const bool with_bias = nbias > 0 && gb && nbias % 4 == 0 && (((uintptr_t)gb) & 15) == 0;
        const size_t tot4 = with_bias ? wsize + (size_t)nbias : wsize;
        hipLaunchKernelGGL(k_wgrad_reduce_v4, dim3((unsigned)((tot4 / 4 + 63) / 64)), dim3(256), 0, s, partial,
                           stride_floats, nsplit, wsize, tot4, gw, with_bias ? gb : (float*)nullptr, beta);
        MS_CHECK_LAUNCH();
        if (nbias > 0 && gb && !with_bias) {
            hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)((nbias + 63) / 64)), dim3(256), 0, s,
                               partial + wsize, stride_floats, nsplit, (size_t)0, nbias, gw, gb, beta);
            MS_CHECK_LAUNCH();
        }
        return MS_OK;
    }
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, s, partial,
                       stride_floats, nsplit, wsize, nbias, gw, gb, beta);
    MS_CHECK_LAUNCH();
    return MS_OK;
}
