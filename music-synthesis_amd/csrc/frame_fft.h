// The in-LDS radix-2 FFT pair of the frame kernels (audio2mel.hip, stft_mag.hip): one 256-thread workgroup transforms
// one windowed frame of n_fft = 2^log2n samples held in re / im (n_fft values each).  The kernels differ in how a
// frame's sample i is fetched (right zero-padding vs reflect padding: the `load` functor) and in the precision of the
// forward transform (`Real`).
#pragma once
#include "ms_common.h"

__device__ __forceinline__ void ms_sincospi(float x, float* s, float* c) { sincospif(x, s, c); }
__device__ __forceinline__ void ms_sincospi(double x, double* s, double* c) { sincospi(x, s, c); }
__device__ __forceinline__ float ms_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double ms_fma(double a, double b, double c) { return fma(a, b, c); }

// The windowed frame load(0 .. n_fft) * window -> X[0 .. n_fft) in natural order in re / im, in Real arithmetic
// (float: Audio2Mel; double: STFTMagnitude, whose log-magnitude loss divides by the smallest magnitudes, so the
// spectrum's rounding error is what its gradient's accuracy hangs on).  A kernel's forward and backward run this one
// body, and the butterfly spells out the fused multiply-adds the forward compiles to, so the backward's recomputed
// spectrum -- and with it every clamp mask -- is bitwise the forward's.
template <class Real, class Load>
__device__ __forceinline__ void ms_frame_fft(Load load, const float* __restrict__ window, int n_fft, int log2n,
                                             Real* re, Real* im) {
    for (int i = threadIdx.x; i < n_fft; i += 256) {
        const Real v = (Real)load(i) * (Real)window[i];
        const int r = (int)(__brev((unsigned)i) >> (32 - log2n));
        re[r] = v;
        im[r] = (Real)0;
    }
    __syncthreads();
    for (int st = 1; st <= log2n; ++st) {
        const int m = 1 << st, half = m >> 1;
        for (int j = threadIdx.x; j < (n_fft >> 1); j += 256) {
            const int grp = j / half, pos = j - grp * half;
            const int i0 = grp * m + pos, i1 = i0 + half;
            Real sn, cs;
            ms_sincospi((Real)2 * (Real)pos / (Real)m, &sn, &cs);  // w = exp(-2 pi i pos / m)
            const Real xr = re[i1], xi = im[i1];
            const Real tr = ms_fma(xr, cs, xi * sn);
            const Real ti = ms_fma(xi, cs, -(xr * sn));
            const Real ur = re[i0], ui = im[i0];
            re[i0] = ur + tr; im[i0] = ui + ti;
            re[i1] = ur - tr; im[i1] = ui - ti;
        }
        __syncthreads();
    }
}

// |X|^2 with the two products and the sum each rounded on their own (no contraction: forward and backward agree)
template <class Real>
__device__ __forceinline__ Real ms_frame_power(Real r, Real q) {
#pragma clang fp contract(off)
    return r * r + q * q;
}

// u[n] = sum_k G[k] exp(+2 pi i k n / n_fft) for G in re / im in natural order: radix-2 decimation in frequency, so the
// result lands in bit-reversed order (u[n] at slot brev(n)) and a gradient spectrum written in place needs no permutation.
__device__ __forceinline__ void ms_frame_ifft_bitrev(int n_fft, float* re, float* im) {
    for (int half = n_fft >> 1; half >= 1; half >>= 1) {
        const int m = half << 1;
        for (int j = threadIdx.x; j < (n_fft >> 1); j += 256) {
            const int grp = j / half, pos = j - grp * half;
            const int i0 = grp * m + pos, i1 = i0 + half;
            float sn, cs;
            sincospif(2.0f * (float)pos / (float)m, &sn, &cs);  // w = exp(+2 pi i pos / m)
            const float ar = re[i0], ai = im[i0], cr = re[i1], ci = im[i1];
            const float dr = ar - cr, di = ai - ci;
            re[i0] = ar + cr; im[i0] = ai + ci;
            re[i1] = dr * cs - di * sn; im[i1] = dr * sn + di * cs;
        }
        __syncthreads();
    }
}

// ... and the end of both backward frame kernels: gf[n] = window[n] * u[n], u read from its bit-reversed slot in re
__device__ __forceinline__ void ms_frame_store_bitrev(const float* __restrict__ window, const float* re, int n_fft, int log2n,
                                                      float* __restrict__ gf) {
    for (int n = threadIdx.x; n < n_fft; n += 256)
        gf[n] = window[n] * re[(int)(__brev((unsigned)n) >> (32 - log2n))];
}

// The gather step of both backward passes: the sum of g[f][q - f*hop] over the frames f that cover position q
// (q - f*hop in [0, n_fft)), in increasing f
__device__ __forceinline__ float ms_frames_over(const float* __restrict__ g, int q, int n_fft, int hop, int frames) {
    const int f_lo = q < n_fft ? 0 : (q - n_fft) / hop + 1;
    const int f_hi = min(frames - 1, q / hop);
    float acc = 0.f;
    for (int f = f_lo; f <= f_hi; ++f) acc += g[(size_t)f * n_fft + (q - f * hop)];
    return acc;
}

// log2(n_fft), or -1 when n_fft is not a power of two in [64, 4096]
static inline int ms_frame_log2(int n_fft) {
    int log2n = 0;
    while ((1 << log2n) < n_fft && log2n < 13) ++log2n;
    return ((1 << log2n) != n_fft || n_fft < 64 || n_fft > 4096) ? -1 : log2n;
}
