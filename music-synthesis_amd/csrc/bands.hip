// Multi-scale band split / merge (include/msynth_bands.h): the reference's fft_frequency_decompose / fft_resample /
// fft_frequency_recompose and their adjoints.  One workgroup owns one row; its half spectrum lives in LDS as n/2 complex
// values (re[n/2], im[n/2]: 128 KiB at n = 32768), produced and consumed by the packed real transforms below, which run
// radix-2 butterflies on n/2 points (frame_fft.h's loops with table twiddles).  Two kernels cover the four passes:
//
//   analysis   one forward transform of n samples, then per band an inverse transform of S samples from bins lo .. S/2
//              (split forward; merge backward with the band's top bin doubled)
//   synthesis  per band a forward transform of S samples whose bins lo .. S/2 are added into the n-sample half spectrum,
//              then one inverse transform of n samples (merge forward; split backward with the band's top bin halved)
//
// Everything is in place.  Analysis takes the bands in ascending size: the inverse of band S works in slots [0, S/2) and
// reads bins S/4 .. S/2, which no smaller band (S' <= S/2, slots [0, S/4)) has touched; bin S/2 sits in slot S/2 and is
// never overwritten.  Synthesis takes them in descending size: band S leaves its bins in slots [S/4, S/2] and zeros
// below, and every smaller band transforms inside those zeros.  So the LDS need is the half spectrum alone.
//
// Adjoint weights.  With irfft_ortho's transpose weighing bins 0 and S/2 by 1 (real part only) and the others by 2, and
// rfft_ortho's transpose by 1 and 1/2, every bin of every band comes out with weight 1 except a band's top bin S/2 when
// S < n: it is interior (2, or 1/2) on the n-sample side and an end bin (1) on the band's side.
#include "ms_common.h"
#include "msynth_bands.h"

namespace {

const int BAND_N_MIN = 64, BAND_N_MAX = 32768, BAND_S_MIN = 16;

__device__ __forceinline__ int band_brev(int j, int log2m) { return (int)(__brev((unsigned)j) >> (32 - log2m)); }
__device__ __forceinline__ float band_scale(int S) { return (float)(1.0 / sqrt((double)S)); }

// Twiddles.  Every angle a butterfly needs is 2 pi t / 32768 with an integer t < 16384, so cos / sin come from two
// 128-entry tables in LDS -- exp(2 pi i 128 a / 32768) and exp(2 pi i b / 32768), rounded from double -- and one complex
// product for t = 128 a + b (exact table values whenever b = 0, i.e. in every transform of 256 points or fewer), instead
// of a sincospif per butterfly as in frame_fft.h's loops (DESIGN.md "Band split / merge" has both timings).
const int TW_BITS = 7, TW_N = 1 << TW_BITS, TW_LOG2_FULL = 15;

__device__ __forceinline__ void band_tw_init(float2* tw) {
    for (int i = threadIdx.x; i < 2 * TW_N; i += blockDim.x) {
        const int t = i < TW_N ? i << TW_BITS : i - TW_N;
        double sn, cs;
        sincospi((double)t / (double)(1 << (TW_LOG2_FULL - 1)), &sn, &cs);
        tw[i] = make_float2((float)cs, (float)sn);
    }
}

__device__ __forceinline__ void band_tw(const float2* tw, int t, float* sn, float* cs) {      // of 2 pi t / 32768
    const float2 a = tw[t >> TW_BITS], b = tw[TW_N + (t & (TW_N - 1))];
    *cs = fmaf(a.x, b.x, -(a.y * b.y));
    *sn = fmaf(a.y, b.x, a.x * b.y);
}

// x[0 .. S) -> X[k] = S^-1/2 sum_t x[t] exp(-2 pi i k t / S): slots lo .. S/2-1 of re / im take bins lo .. S/2-1, the
// slots below lo zeros, *top the (real) bin S/2.  z[j] = x[2j] + i x[2j+1] is stored bit-reversed, transformed on S/2
// points (radix-2 decimation in time, natural order out) and unfolded: X[k] = E[k] + w^k O[k],
// X[S/2-k] = conj(E[k] - w^k O[k]) with E, O the even / odd halves of Z and w = exp(-2 pi i / S).
template <int NT>
__device__ __forceinline__ void band_forward(const float* __restrict__ x, int S, int lo, float* re, float* im, float* top,
                                             const float2* tw) {
    const int M = S >> 1, log2m = 31 - __clz(M);
    for (int i = threadIdx.x; i < S; i += NT) ((i & 1) ? im : re)[band_brev(i >> 1, log2m)] = x[i];
    __syncthreads();
    for (int st = 1; st <= log2m; ++st) {
        const int half = 1 << (st - 1);
        for (int j = threadIdx.x; j < (M >> 1); j += NT) {
            const int pos = j & (half - 1), i0 = ((j - pos) << 1) + pos, i1 = i0 + half;
            float sn, cs;
            band_tw(tw, pos << (TW_LOG2_FULL - st), &sn, &cs);      // w = exp(-2 pi i pos / 2^st)
            const float xr = re[i1], xi = im[i1];
            const float tr = fmaf(xr, cs, xi * sn), ti = fmaf(xi, cs, -(xr * sn));
            const float ur = re[i0], ui = im[i0];
            re[i0] = ur + tr; im[i0] = ui + ti;
            re[i1] = ur - tr; im[i1] = ui - ti;
        }
        __syncthreads();
    }
    const float sc = band_scale(S);
    for (int k = threadIdx.x; k <= (M >> 1); k += NT) {
        if (k == 0) {
            const float zr = re[0], zi = im[0];
            re[0] = lo == 0 ? (zr + zi) * sc : 0.f;
            im[0] = 0.f;
            *top = (zr - zi) * sc;
            continue;
        }
        const int k2 = M - k;
        const float ar = re[k], ai = im[k], br = re[k2], bi = im[k2];
        const float er = 0.5f * (ar + br), ei = 0.5f * (ai - bi);
        const float qr = 0.5f * (ai + bi), qi = 0.5f * (br - ar);
        float sn, cs;
        band_tw(tw, k << (TW_LOG2_FULL - 1 - log2m), &sn, &cs);
        const float tr = fmaf(cs, qr, sn * qi), ti = fmaf(cs, qi, -(sn * qr));
        const bool keep = k >= lo;
        re[k] = keep ? (er + tr) * sc : 0.f;
        im[k] = keep ? (ei + ti) * sc : 0.f;
        if (k2 != k) {
            re[k2] = (er - tr) * sc;
            im[k2] = (ti - ei) * sc;
        }
    }
    __syncthreads();
}

// out[0 .. S) = irfft_ortho(C, S) for C[k] = slot k (lo <= k < S/2), 0 below lo, and the real C[S/2] = top; works in
// slots [0, S/2).  Z[k] = A + i B, Z[S/2-k] = conj(A) + i conj(B) with A = C[k] + conj(C[S/2-k]),
// B = (C[k] - conj(C[S/2-k])) exp(+2 pi i k / S); z = sum_k Z[k] exp(+2 pi i j k / (S/2)) holds out[2j] + i out[2j+1]
// (radix-2 decimation in frequency: natural order in, bit-reversed out, undone by the store).
template <int NT>
__device__ __forceinline__ void band_inverse(float* re, float* im, int S, int lo, float top, float* __restrict__ out,
                                             const float2* tw) {
    const int M = S >> 1, log2m = 31 - __clz(M);
    for (int k = threadIdx.x; k <= (M >> 1); k += NT) {
        if (k == 0) {
            const float c0 = lo == 0 ? re[0] : 0.f;
            re[0] = c0 + top;
            im[0] = c0 - top;
            continue;
        }
        const int k2 = M - k;
        const bool has = k >= lo;
        const float ar = has ? re[k] : 0.f, ai = has ? im[k] : 0.f, br = re[k2], bi = im[k2];
        const float Ar = ar + br, Ai = ai - bi, dr = ar - br, di = ai + bi;
        float sn, cs;
        band_tw(tw, k << (TW_LOG2_FULL - 1 - log2m), &sn, &cs);
        const float Br = fmaf(dr, cs, -(di * sn)), Bi = fmaf(dr, sn, di * cs);
        re[k] = Ar - Bi;
        im[k] = Ai + Br;
        if (k2 != k) {
            re[k2] = Ar + Bi;
            im[k2] = Br - Ai;
        }
    }
    __syncthreads();
    for (int st = log2m; st >= 1; --st) {
        const int half = 1 << (st - 1);
        for (int j = threadIdx.x; j < (M >> 1); j += NT) {
            const int pos = j & (half - 1), i0 = ((j - pos) << 1) + pos, i1 = i0 + half;
            float sn, cs;
            band_tw(tw, pos << (TW_LOG2_FULL - st), &sn, &cs);      // w = exp(+2 pi i pos / 2^st)
            const float ar = re[i0], ai = im[i0], cr = re[i1], ci = im[i1];
            const float dr = ar - cr, di = ai - ci;
            re[i0] = ar + cr; im[i0] = ai + ci;
            re[i1] = fmaf(dr, cs, -(di * sn)); im[i1] = fmaf(dr, sn, di * cs);
        }
        __syncthreads();
    }
    const float sc = band_scale(S);
    for (int i = threadIdx.x; i < S; i += NT) out[i] = sc * ((i & 1) ? im : re)[band_brev(i >> 1, log2m)];
    __syncthreads();
}

__device__ __forceinline__ int band_lo(const ms_band_desc& d, int b) { return (b == 0 && d.lowest) ? 0 : d.size[b] >> 2; }

// grid (rows) or (rows, bands): in the second shape a workgroup recomputes the row's spectrum and writes one band
template <int NT>
__global__ __launch_bounds__(NT) void k_band_analysis(const float* __restrict__ x, int n, ms_band_desc bands, float top_w) {
    extern __shared__ float band_smem[];
    __shared__ float s_top;
    __shared__ float2 s_tw[2 * TW_N];
    float* re = band_smem;
    float* im = band_smem + (n >> 1);
    const size_t row = blockIdx.x;
    band_tw_init(s_tw);         // (visible after the barrier that follows band_forward's load)
    band_forward<NT>(x + row * n, n, 0, re, im, &s_top, s_tw);
    const int b0 = gridDim.y > 1 ? (int)blockIdx.y : 0, b1 = gridDim.y > 1 ? b0 + 1 : bands.count;
    for (int b = b0; b < b1; ++b) {
        float* out = bands.data[b];
        if (!out) continue;
        const int S = bands.size[b];
        const float top = S < n ? re[S >> 1] * top_w : s_top;
        band_inverse<NT>(re, im, S, band_lo(bands, b), top, out + row * S, s_tw);
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_band_synthesis(ms_band_desc bands, int n, float top_w, float* __restrict__ y) {
    extern __shared__ float band_smem[];
    __shared__ float s_top, s_ntop;
    __shared__ float2 s_tw[2 * TW_N];
    const int M = n >> 1;
    float* re = band_smem;
    float* im = band_smem + M;
    const size_t row = blockIdx.x;
    for (int i = threadIdx.x; i < M; i += NT) re[i] = im[i] = 0.f;
    if (threadIdx.x == 0) s_ntop = 0.f;
    band_tw_init(s_tw);
    __syncthreads();
    for (int b = bands.count - 1; b >= 0; --b) {
        const float* src = bands.data[b];
        if (!src) continue;
        const int S = bands.size[b];
        band_forward<NT>(src + row * S, S, band_lo(bands, b), re, im, &s_top, s_tw);
        if (threadIdx.x == 0) {             // the next band works in slots below S/4 and thread 0 rewrites s_top itself
            if (S < n) re[S >> 1] = fmaf(s_top, top_w, re[S >> 1]);
            else s_ntop = s_top;
        }
    }
    __syncthreads();
    band_inverse<NT>(re, im, n, 0, s_ntop, y + row * n, s_tw);
}

int band_log2(int v) {      // log2 of a power of two, else -1
    if (v <= 0 || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// MS_OK / MS_ERR_*: the sizes alone
int band_check(int n, const ms_band_desc* d) {
    if (!d || n <= 0 || d->count <= 0) return MS_ERR_INVALID_ARG;
    if (d->count > MS_BAND_MAX || band_log2(n) < 0 || n < BAND_N_MIN || n > BAND_N_MAX) return MS_ERR_UNSUPPORTED;
    for (int i = 0; i < d->count; ++i) {
        const int S = d->size[i];
        if (S <= 0) return MS_ERR_INVALID_ARG;
        if (band_log2(S) < 0 || S < BAND_S_MIN || S > n) return MS_ERR_UNSUPPORTED;
        if (i && S <= d->size[i - 1]) return MS_ERR_INVALID_ARG;
    }
    return MS_OK;
}

// all = true: every band pointer must be there; otherwise at least one
int band_check_ptrs(const ms_band_desc* d, bool all) {
    int have = 0;
    for (int i = 0; i < d->count; ++i) have += d->data[i] != nullptr;
    return (all ? have == d->count : have > 0) ? MS_OK : MS_ERR_INVALID_ARG;
}

ms_band_desc band_copy(const ms_band_desc* d) {     // unused entries cleared: the kernel argument is fully defined
    ms_band_desc c = {};
    c.count = d->count;
    c.lowest = d->lowest ? 1 : 0;
    for (int i = 0; i < d->count; ++i) {
        c.size[i] = d->size[i];
        c.data[i] = d->data[i];
    }
    return c;
}

template <int NT>
void band_raise_lds() {     // the 128 KiB of n = 32768 are past the 64 KiB a kernel gets without asking
    static unsigned long long attr_set = 0;
    if (ms_first_on_device(attr_set)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_band_analysis<NT>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, BAND_N_MAX * (int)sizeof(float));
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_band_synthesis<NT>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, BAND_N_MAX * (int)sizeof(float));
        ms_done_on_device(attr_set);
    }
}

// Analysis grid.  A workgroup's time is latency, not throughput (a chain of barriers between radix-2 stages), so while
// every (row, band) pair can have a CU to itself, one workgroup per pair that recomputes the row's spectrum finishes
// sooner than one per row that walks the bands; past that the recomputation is pure extra work.  Measured both ways at
// 5, 160 and 1280 pairs (DESIGN.md "Band split / merge").  MSYNTH_BAND_SPLIT = 0 / 1 forces the per-row / the
// (row, band) grid: the A/B switch of tools/band_timing.py.
bool band_split_grid(int rows, int count) {
    if (count < 2) return false;
    const int forced = ms_switch_int("MSYNTH_BAND_SPLIT", -1);
    if (forced >= 0) return forced != 0;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ms_current_device()) != hipSuccess) return false;
    return (long long)rows * count <= cus;
}

int band_analysis(const float* x, int rows, int n, const ms_band_desc* d, float top_w, hipStream_t s) {
    const ms_band_desc c = band_copy(d);
    const dim3 grid(rows, band_split_grid(rows, c.count) ? c.count : 1);
    const size_t lds = (size_t)n * sizeof(float);
    if (n >= 4096) {
        band_raise_lds<1024>();
        hipLaunchKernelGGL(k_band_analysis<1024>, grid, dim3(1024), lds, s, x, n, c, top_w);
    } else {
        hipLaunchKernelGGL(k_band_analysis<256>, grid, dim3(256), lds, s, x, n, c, top_w);
    }
    MS_CHECK_LAUNCH();
    return MS_OK;
}

int band_synthesis(const ms_band_desc* d, int rows, int n, float top_w, float* y, hipStream_t s) {
    const ms_band_desc c = band_copy(d);
    const size_t lds = (size_t)n * sizeof(float);
    if (n >= 4096) {
        band_raise_lds<1024>();
        hipLaunchKernelGGL(k_band_synthesis<1024>, dim3(rows), dim3(1024), lds, s, c, n, top_w, y);
    } else {
        hipLaunchKernelGGL(k_band_synthesis<256>, dim3(rows), dim3(256), lds, s, c, n, top_w, y);
    }
    MS_CHECK_LAUNCH();
    return MS_OK;
}

}  // namespace

extern "C" {

int ms_band_supported(int32_t n, const ms_band_desc* bands) { return band_check(n, bands) == MS_OK ? 1 : 0; }

size_t ms_band_workspace_bytes(int32_t rows, int32_t n, const ms_band_desc* bands) {
    (void)rows; (void)n; (void)bands;
    return 0;
}

int ms_band_decompose_fwd(const float* x, int32_t rows, int32_t n, const ms_band_desc* bands, void* workspace,
                          size_t workspace_bytes, ms_stream_t stream) {
    (void)workspace; (void)workspace_bytes;
    if (!x || rows <= 0) return MS_ERR_INVALID_ARG;
    const int rc = band_check(n, bands);
    if (rc != MS_OK) return rc;
    if (band_check_ptrs(bands, true) != MS_OK) return MS_ERR_INVALID_ARG;
    return band_analysis(x, rows, n, bands, 1.f, (hipStream_t)stream);
}

int ms_band_decompose_bwd(const ms_band_desc* grad_bands, int32_t rows, int32_t n, float* grad_x, void* workspace,
                          size_t workspace_bytes, ms_stream_t stream) {
    (void)workspace; (void)workspace_bytes;
    if (!grad_x || rows <= 0) return MS_ERR_INVALID_ARG;
    const int rc = band_check(n, grad_bands);
    if (rc != MS_OK) return rc;
    if (band_check_ptrs(grad_bands, false) != MS_OK) return MS_ERR_INVALID_ARG;
    return band_synthesis(grad_bands, rows, n, 0.5f, grad_x, (hipStream_t)stream);
}

int ms_band_recompose_fwd(const ms_band_desc* bands, int32_t rows, int32_t n, float* y, void* workspace,
                          size_t workspace_bytes, ms_stream_t stream) {
    (void)workspace; (void)workspace_bytes;
    if (!y || rows <= 0) return MS_ERR_INVALID_ARG;
    const int rc = band_check(n, bands);
    if (rc != MS_OK) return rc;
    if (band_check_ptrs(bands, true) != MS_OK) return MS_ERR_INVALID_ARG;
    return band_synthesis(bands, rows, n, 1.f, y, (hipStream_t)stream);
}

int ms_band_recompose_bwd(const float* grad_y, int32_t rows, int32_t n, const ms_band_desc* grad_bands, void* workspace,
                          size_t workspace_bytes, ms_stream_t stream) {
    (void)workspace; (void)workspace_bytes;
    if (!grad_y || rows <= 0) return MS_ERR_INVALID_ARG;
    const int rc = band_check(n, grad_bands);
    if (rc != MS_OK) return rc;
    if (band_check_ptrs(grad_bands, false) != MS_OK) return MS_ERR_INVALID_ARG;
    return band_analysis(grad_y, rows, n, grad_bands, 2.f, (hipStream_t)stream);
}

}  // extern "C"
