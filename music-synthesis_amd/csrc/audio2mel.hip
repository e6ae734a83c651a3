// Audio2Mel (reference feature/feature.py:39-59): hann-windowed STFT frame -> magnitude ->
// mel filterbank -> log10(clamp(., 1e-5)).  One workgroup per (batch, frame): the frame is read
// once from HBM (coalesced, contiguous audio samples), windowed into LDS in bit-reversed order,
// transformed by an in-LDS radix-2 FFT, and the mel projection is taken from the LDS magnitudes.
//
// Backward (autograd of the same graph w.r.t. the audio): each (batch, frame) workgroup recomputes its
// spectrum from the saved audio (one FFT, cheaper than saving B*F*(n_fft+2) floats), takes d loss / d mel
// through log10 and the clamp, projects it back through the filters' nonzero supports, scales by X/|X| and
// runs the inverse FFT in LDS; the windowed frame gradients land in a per-frame workspace and a gather
// kernel sums the <= n_fft/hop frames over each sample in frame order (no atomics: bitwise reproducible).
#include "frame_fft.h"

namespace {

// The windowed, right-zero-padded frame at sample `start` of row `a` -> X[0 .. n_fft) in natural order in
// re / im: the shared in-LDS FFT (frame_fft.h) fed by this kernel family's frame load.
__device__ __forceinline__ void a2m_frame_fft(const float* __restrict__ a, int N, const float* __restrict__ window,
                                              int n_fft, int log2n, int start, float* re, float* im) {
    ms_frame_fft<float>([=](int i) {
        const int s = start + i;
        return s < N ? a[s] : 0.f;  // right zero-padding, feature.py:44-45
    }, window, n_fft, log2n, re, im);
}

__device__ __forceinline__ float a2m_mag(float r, float q) {
#pragma clang fp contract(off)
    return sqrtf(r * r + q * q);
}

__global__ __launch_bounds__(256) void k_audio2mel(const float* __restrict__ audio, int N,
                                                  const float* __restrict__ window, int n_fft,
                                                  int log2n, int hop, int frames,
                                                  const float* __restrict__ basis, int n_mel,
                                                  float* __restrict__ out) {
    extern __shared__ float smem[];
    float* re = smem;
    float* im = smem + n_fft;
    const int fr = blockIdx.x, b = blockIdx.y;
    a2m_frame_fft(audio + (size_t)b * N, N, window, n_fft, log2n, fr * hop, re, im);
    const int nb = (n_fft >> 1) + 1;
    // magnitudes into re[0..nb) (bins only read their own slot, so in place is safe)
    for (int j = threadIdx.x; j < nb; j += 256) re[j] = a2m_mag(re[j], im[j]);
    __syncthreads();
    for (int mi = threadIdx.x; mi < n_mel; mi += 256) {
        const float* br = basis + (size_t)mi * nb;
        float acc = 0.f;
        for (int j = 0; j < nb; ++j) acc = fmaf(br[j], re[j], acc);
        out[((size_t)b * n_mel + mi) * frames + fr] = log10f(fmaxf(acc, 1e-5f));
    }
}

// Nonzero supports of the basis the call was handed (a buffer load_state_dict may have overwritten): the first
// ceil(nb/64) blocks give bin k's filters [lo, hi], the n_rows blocks behind them filter m's bins [lo, hi] (lo > hi:
// all zero).  Summing a filter over its support gives the full row's sum bitwise: the fma chain starts at +0 and the
// zeros outside add nothing.
__global__ __launch_bounds__(256) void k_mel_support(const float* __restrict__ basis, int n_mel, int nb, int n_rows,
                                                    int2* __restrict__ row_sup, int2* __restrict__ col_sup) {
    __shared__ int red[2][256];
    const int col_blocks = (nb + 63) / 64, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int lo, hi;
    if ((int)blockIdx.x < col_blocks) {     // 64 bins per block (coalesced), the filters split over the four waves
        const int k = (int)blockIdx.x * 64 + lane;
        lo = n_mel;
        hi = -1;
        if (k < nb) {
#pragma unroll 8
            for (int m = w; m < n_mel; m += 4) {
                const bool nz = basis[(size_t)m * nb + k] != 0.f;
                lo = nz ? min(lo, m) : lo;
                hi = nz ? m : hi;
            }
        }
        red[0][threadIdx.x] = lo;
        red[1][threadIdx.x] = hi;
        __syncthreads();
        if (w == 0 && k < nb)
            col_sup[k] = make_int2(min(min(lo, red[0][64 + lane]), min(red[0][128 + lane], red[0][192 + lane])),
                                   max(max(hi, red[1][64 + lane]), max(red[1][128 + lane], red[1][192 + lane])));
        return;
    }
    const int m = (int)blockIdx.x - col_blocks;
    const float* row = basis + (size_t)m * nb;
    lo = nb;
    hi = -1;
    for (int j = threadIdx.x; j < nb; j += 256)
        if (row[j] != 0.f) {
            lo = min(lo, j);
            hi = max(hi, j);
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
        red[0][w] = lo;
        red[1][w] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        row_sup[m] = make_int2(min(min(red[0][0], red[0][1]), min(red[0][2], red[0][3])),
                               max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3])));
}

// filter m's bins to visit: its support, or every bin for filters past the row table
__device__ __forceinline__ int2 a2m_support(const int2* __restrict__ row_sup, int n_rows, int m, int nb) {
    return m < n_rows ? row_sup[m] : make_int2(0, nb - 1);
}

// One workgroup per (batch, frame): gframes[b][fr][n] = window[n] * d loss / d u_fr[n].
// LDS: re, im (n_fft each), |X| (nb), d loss / d mel (n_mel).
__global__ __launch_bounds__(256) void k_audio2mel_bwd_frame(const float* __restrict__ audio, int N,
                                                            const float* __restrict__ window, int n_fft, int log2n,
                                                            int hop, int frames, const float* __restrict__ basis,
                                                            int n_mel, const int2* __restrict__ row_sup, int n_rows,
                                                            const int2* __restrict__ col_sup,
                                                            const float* __restrict__ grad_out,
                                                            float* __restrict__ gframes) {
    extern __shared__ float smem[];
    const int nb = (n_fft >> 1) + 1;
    float* re = smem;
    float* im = re + n_fft;
    float* mag = im + n_fft;
    float* gm = mag + nb;
    const int fr = blockIdx.x, b = blockIdx.y;
    a2m_frame_fft(audio + (size_t)b * N, N, window, n_fft, log2n, fr * hop, re, im);
    for (int j = threadIdx.x; j < nb; j += 256) mag[j] = a2m_mag(re[j], im[j]);
    __syncthreads();
    // mel exactly as the forward sums it; d/d mel of log10(clamp(mel, 1e-5)): 1 / (mel ln 10) where the clamp
    // passes the gradient (mel >= 1e-5, as torch's clamp backward), else 0
    for (int mi = threadIdx.x; mi < n_mel; mi += 256) {
        const int2 s = a2m_support(row_sup, n_rows, mi, nb);
        const float* br = basis + (size_t)mi * nb;
        float acc = 0.f;
        for (int j = s.x; j <= s.y; ++j) acc = fmaf(br[j], mag[j], acc);
        const float g = grad_out[((size_t)b * n_mel + mi) * frames + fr];
        gm[mi] = acc >= 1e-5f ? g / (acc * 2.302585093f) : 0.f;
    }
    __syncthreads();
    // d/d X[k] = (basis^T gm)[k] * X[k] / |X[k]| (0 where |X[k]| = 0: torch.abs of a complex tensor), the sum over
    // bin k's filters only; one-sided: the bins above n_fft/2 carry nothing.  In place: a bin touches only its slots.
    for (int k = threadIdx.x; k < n_fft; k += 256) {
        float sc = 0.f;
        if (k < nb) {
            const int2 c = col_sup[k];
            float acc = 0.f;
            for (int m = c.x; m <= c.y; ++m) acc = fmaf(basis[(size_t)m * nb + k], gm[m], acc);
            sc = mag[k] > 0.f ? acc / mag[k] : 0.f;
        }
        re[k] = k < nb ? re[k] * sc : 0.f;
        im[k] = k < nb ? im[k] * sc : 0.f;
    }
    __syncthreads();
    // d/d u[n] = Re sum_k G[k] exp(+2 pi i k n / n_fft), bit-reversed order out (so the gradient spectrum is written
    // in place above, with no permutation)
    ms_frame_ifft_bitrev(n_fft, re, im);
    ms_frame_store_bitrev(window, re, n_fft, log2n, gframes + ((size_t)b * frames + fr) * n_fft);
}

// grad_audio[b][s] = sum over the frames f that cover sample s (s - f*hop in [0, n_fft)), in increasing f;
// samples past N (the right padding) are dropped by construction
__global__ __launch_bounds__(256) void k_audio2mel_bwd_gather(const float* __restrict__ gframes, int N, int n_fft,
                                                             int hop, int frames, float* __restrict__ grad_audio) {
    const int b = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N) return;
    grad_audio[(size_t)b * N + s] = ms_frames_over(gframes + (size_t)b * frames * n_fft, s, n_fft, hop, frames);
}

const size_t A2M_BWD_LDS_MAX = 64 * 1024;

}  // namespace

extern "C" {

int ms_audio2mel_frames(int32_t N, int32_t n_fft, int32_t hop) {
    if (N <= 0 || n_fft <= 0 || hop <= 0) return 0;
    const int total = N + (n_fft - hop) / 2;
    return total < n_fft ? 0 : (total - n_fft) / hop + 1;
}

int ms_audio2mel_fwd(const float* audio, int32_t B, int32_t N, const float* window, int32_t n_fft,
                     int32_t hop, const float* mel_basis, int32_t n_mel, float* out,
                     ms_stream_t stream) {
    if (!audio || !window || !mel_basis || !out || B <= 0 || N <= 0 || n_mel <= 0 || hop <= 0)
        return MS_ERR_INVALID_ARG;
    const int log2n = ms_frame_log2(n_fft);
    if (log2n < 0) return MS_ERR_UNSUPPORTED;
    const int frames = ms_audio2mel_frames(N, n_fft, hop);
    if (frames <= 0) return MS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_audio2mel, dim3(frames, B), dim3(256), (size_t)2 * n_fft * sizeof(float),
                       (hipStream_t)stream, audio, N, window, n_fft, log2n, hop, frames, mel_basis,
                       n_mel, out);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

size_t ms_audio2mel_bwd_workspace_bytes(int32_t B, int32_t N, int32_t n_fft, int32_t hop) {
    if (B <= 0 || ms_frame_log2(n_fft) < 0) return 0;
    const int frames = ms_audio2mel_frames(N, n_fft, hop);
    if (frames <= 0) return 0;
    // per-frame gradients, then the supports (int2) of up to n_fft/2+1 filters and of the n_fft/2+1 bins
    return (size_t)B * frames * n_fft * sizeof(float) + (size_t)((n_fft >> 1) + 1) * 4 * sizeof(int32_t);
}

int ms_audio2mel_bwd(const float* audio, int32_t B, int32_t N, const float* window, int32_t n_fft, int32_t hop,
                     const float* mel_basis, int32_t n_mel, const float* grad_out, float* grad_audio,
                     void* workspace, size_t workspace_bytes, ms_stream_t stream) {
    if (!audio || !window || !mel_basis || !grad_out || !grad_audio || B <= 0 || N <= 0 || n_mel <= 0 || hop <= 0)
        return MS_ERR_INVALID_ARG;
    const int log2n = ms_frame_log2(n_fft);
    if (log2n < 0) return MS_ERR_UNSUPPORTED;
    const int frames = ms_audio2mel_frames(N, n_fft, hop);
    if (frames <= 0) return MS_ERR_INVALID_ARG;
    const int nb = (n_fft >> 1) + 1;
    const size_t lds = ((size_t)2 * n_fft + nb + n_mel) * sizeof(float);
    if (lds > A2M_BWD_LDS_MAX) return MS_ERR_UNSUPPORTED;
    const size_t need = ms_audio2mel_bwd_workspace_bytes(B, N, n_fft, hop);
    if (!workspace || workspace_bytes < need) return MS_ERR_WORKSPACE;
    float* gframes = (float*)workspace;
    int2* row_sup = (int2*)(gframes + (size_t)B * frames * n_fft);
    int2* col_sup = row_sup + nb;
    const int n_rows = n_mel < nb ? n_mel : nb;
    hipLaunchKernelGGL(k_mel_support, dim3((nb + 63) / 64 + n_rows), dim3(256), 0, (hipStream_t)stream, mel_basis,
                       n_mel, nb, n_rows, row_sup, col_sup);
    MS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_audio2mel_bwd_frame, dim3(frames, B), dim3(256), lds, (hipStream_t)stream, audio, N, window,
                       n_fft, log2n, hop, frames, mel_basis, n_mel, (const int2*)row_sup, n_rows,
                       (const int2*)col_sup, grad_out, gframes);
    MS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_audio2mel_bwd_gather, dim3((N + 255) / 256, B), dim3(256), 0, (hipStream_t)stream,
                       (const float*)gframes, N, n_fft, hop, frames, grad_audio);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// audio() front-end of the dataset pass (feature/feature.py:64-71): band-limited sinc resampling
// (librosa.resample's default 'kaiser_best' = resampy's interpolated Kaiser-windowed sinc table) and peak
// normalisation x / max|x| * 0.95.  One thread per output sample walks the two wings of the filter exactly as
// resampy's resample_f does (table lookup + linear interpolation between table entries); the half-window table
// and its first differences come from the host (numpy, like resampy itself builds them).
namespace {

__global__ __launch_bounds__(256) void k_resample_sinc(const float* __restrict__ x, int rows, int n_in,
                                                      float* __restrict__ y, int n_out, double ratio,
                                                      const float* __restrict__ win,
                                                      const float* __restrict__ delta, int nwin, int num_table) {
    const double scale = ratio < 1.0 ? ratio : 1.0;
    const int index_step = (int)(scale * num_table);
    const long long total = (long long)rows * n_out;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / n_out), t = (int)(i - (long long)r * n_out);
        const float* xr = x + (size_t)r * n_in;
        const double time_register = (double)t / ratio;
        const int n = (int)time_register;
        float acc = 0.f;
        // left wing
        double frac = scale * (time_register - n);
        double index_frac = frac * num_table;
        int offset = (int)index_frac;
        float eta = (float)(index_frac - offset);
        int i_max = (nwin - offset) / index_step;
        if (i_max > n + 1) i_max = n + 1;
        for (int k = 0; k < i_max; ++k) {
            const int w = offset + k * index_step;
            acc += (win[w] + eta * delta[w]) * xr[n - k];
        }
        // right wing
        frac = scale - frac;
        index_frac = frac * num_table;
        offset = (int)index_frac;
        eta = (float)(index_frac - offset);
        int k_max = (nwin - offset) / index_step;
        if (k_max > n_in - n - 1) k_max = n_in - n - 1;
        for (int k = 0; k < k_max; ++k) {
            const int w = offset + k * index_step;
            acc += (win[w] + eta * delta[w]) * xr[n + k + 1];
        }
        y[i] = acc;
    }
}

__global__ __launch_bounds__(256) void k_row_absmax(const float* __restrict__ x, int n, float* __restrict__ out) {
    __shared__ float red[4];
    const float* xr = x + (size_t)blockIdx.x * n;
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(xr[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void k_row_scale(float* __restrict__ x, int n, const float* __restrict__ amax,
                                                  float scale) {
    const float m = amax[blockIdx.y];
    const float f = m > 1.17549435e-38f ? scale / m : scale;      // librosa.util.normalize: rows below tiny stay as they are
    float* xr = x + (size_t)blockIdx.y * n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) xr[i] *= f;
}

}  // namespace

extern "C" int ms_resample_sinc_fwd(const float* x, int32_t rows, int32_t n_in, float* y, int32_t n_out, double ratio,
                                    const float* interp_win, const float* interp_delta, int32_t nwin,
                                    int32_t num_table, ms_stream_t stream) {
    if (!x || !y || !interp_win || !interp_delta || rows <= 0 || n_in <= 0 || n_out <= 0 || ratio <= 0.0 || nwin <= 0 ||
        num_table <= 0)
        return MS_ERR_INVALID_ARG;
    const double scale = ratio < 1.0 ? ratio : 1.0;
    if ((int)(scale * num_table) < 1) return MS_ERR_UNSUPPORTED;
    long long total = (long long)rows * n_out;
    unsigned nb = (unsigned)((total + 255) / 256 > 65535 ? 65535 : (total + 255) / 256);
    hipLaunchKernelGGL(k_resample_sinc, dim3(nb), dim3(256), 0, (hipStream_t)stream, x, rows, n_in, y, n_out, ratio,
                       interp_win, interp_delta, nwin, num_table);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

extern "C" int ms_peak_normalize(float* x, int32_t rows, int32_t n, float scale, float* workspace /* rows floats */,
                                 ms_stream_t stream) {
    if (!x || !workspace || rows <= 0 || n <= 0) return MS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_row_absmax, dim3(rows), dim3(256), 0, (hipStream_t)stream, x, n, workspace);
    MS_CHECK_LAUNCH();
    unsigned nbx = (unsigned)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256);
    hipLaunchKernelGGL(k_row_scale, dim3(nbx, rows), dim3(256), 0, (hipStream_t)stream, x, n, workspace, scale);
    MS_CHECK_LAUNCH();
    return MS_OK;
}
