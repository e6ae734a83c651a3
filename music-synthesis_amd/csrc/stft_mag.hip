// STFTMagnitude: sqrt(clamp(|STFT(audio)|^2, min_power)) with torch.stft's center=True / reflect framing and a window
// already zero-padded to n_fft, differentiable w.r.t. the audio, and the pair loss of a multi-resolution STFT loss on
// two such magnitude tensors (spectral convergence + log-magnitude L1).
//
// Forward: one workgroup per (row, frame), as k_audio2mel: the frame is read once with the reflect index map applied
// on load, transformed by the shared in-LDS FFT (frame_fft.h) in double, and its n_fft/2+1 magnitudes are stored
// frame-major (B, frames, n_fft/2+1), so a workgroup's stores are one contiguous run.  Double, because the loss this
// feeds weighs a bin by 1/|X| and turns its cotangent by X/|X|: the absolute rounding error of a single-precision
// 10-stage FFT (1e-7 of the frame's LARGEST bins) is a relative error of 1e-3 and more in the smallest bins, which
// are the ones that carry the log-magnitude gradient.
// Backward: saves only the audio.  Each (row, frame) workgroup recomputes its spectrum with the same FFT body (the clamp
// mask is bitwise the forward's), scales the cotangent by X/|X|, runs the inverse FFT in LDS and leaves the windowed
// frame gradient in a workspace; a gather sums, in a fixed order and without atomics, the frames over each sample --
// the sample's own padded position, then the left and the right reflect-pad positions that mirror onto it.
#include "frame_fft.h"

namespace {

// sample i of frame `fr`: padded position fr*hop + i, p = n_fft/2 reflect-padded samples on either side (N > p, so
// one reflection lands inside the row)
struct StftLoad {
    const float* a;
    int N, start;     // start = fr*hop - p
    __device__ __forceinline__ float operator()(int i) const {
        int t = start + i;
        t = t < 0 ? -t : t;
        t = t >= N ? 2 * (N - 1) - t : t;
        return a[t];
    }
};

const int STFT_BINS_PER_THREAD = 9;     // ceil((4096 / 2 + 1) / 256)

// The spectrum is taken in double (frame_fft.h): re / im hold n_fft doubles each.
__global__ __launch_bounds__(256) void k_stft_mag(const float* __restrict__ audio, int N,
                                                 const float* __restrict__ window, int n_fft, int log2n, int hop,
                                                 int frames, float min_power, float* __restrict__ mag) {
    extern __shared__ double smem[];
    double* re = smem;
    double* im = smem + n_fft;
    const int fr = blockIdx.x, b = blockIdx.y;
    ms_frame_fft<double>(StftLoad{audio + (size_t)b * N, N, fr * hop - (n_fft >> 1)}, window, n_fft, log2n, re, im);
    const int nb = (n_fft >> 1) + 1;
    float* out = mag + ((size_t)b * frames + fr) * nb;
    for (int j = threadIdx.x; j < nb; j += 256)
        out[j] = (float)sqrt(fmax(ms_frame_power(re[j], im[j]), (double)min_power));
}

// gframes[b][fr][n] = window[n] * d loss / d u_fr[n] for the cotangent gmag (B, frames, nb)
__global__ __launch_bounds__(256) void k_stft_mag_bwd_frame(const float* __restrict__ audio, int N,
                                                           const float* __restrict__ window, int n_fft, int log2n,
                                                           int hop, int frames, float min_power,
                                                           const float* __restrict__ gmag,
                                                           float* __restrict__ gframes) {
    extern __shared__ double smem[];
    double* re = smem;
    double* im = smem + n_fft;
    const int fr = blockIdx.x, b = blockIdx.y;
    ms_frame_fft<double>(StftLoad{audio + (size_t)b * N, N, fr * hop - (n_fft >> 1)}, window, n_fft, log2n, re, im);
    const int nb = (n_fft >> 1) + 1;
    const float* g = gmag + ((size_t)b * frames + fr) * nb;
    // d/d X[k] = g[k] * X[k] / |X[k]| where the clamp passes the gradient (power >= min_power, as torch's clamp
    // backward) and |X[k]| > 0 (X/|X| := 0 at an exactly-zero bin); one-sided: the bins above n_fft/2 carry nothing.
    // The gradient spectrum is single precision and reuses the LDS of the double spectrum, so a thread first takes
    // its bins (k = threadIdx.x + 256 j; n_fft <= 4096: at most STFT_BINS_PER_THREAD of the 2049) into registers.
    float gr[STFT_BINS_PER_THREAD], gi[STFT_BINS_PER_THREAD];
#pragma unroll
    for (int j = 0; j < STFT_BINS_PER_THREAD; ++j) {
        const int k = threadIdx.x + 256 * j;
        gr[j] = gi[j] = 0.f;
        if (k < nb) {
            const double pw = ms_frame_power(re[k], im[k]);
            const double sc = (pw >= (double)min_power && pw > 0.0) ? (double)g[k] / sqrt(pw) : 0.0;
            gr[j] = (float)(re[k] * sc);
            gi[j] = (float)(im[k] * sc);
        }
    }
    __syncthreads();
    float* fre = (float*)smem;
    float* fim = fre + n_fft;
    for (int k = threadIdx.x; k < n_fft; k += 256) fre[k] = fim[k] = 0.f;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < STFT_BINS_PER_THREAD; ++j) {
        const int k = threadIdx.x + 256 * j;
        if (k < nb) {
            fre[k] = gr[j];
            fim[k] = gi[j];
        }
    }
    __syncthreads();
    ms_frame_ifft_bitrev(n_fft, fre, fim);
    ms_frame_store_bitrev(window, fre, n_fft, log2n, gframes + ((size_t)b * frames + fr) * n_fft);
}

// grad_audio[b][s]: sample s sits at padded position p + s; the left pad position p - s (1 <= s <= p) and the right
// pad position p + 2(N-1) - s (N-1-p <= s <= N-2) hold copies of it.  Always summed in that order.
__global__ __launch_bounds__(256) void k_stft_mag_bwd_gather(const float* __restrict__ gframes, int N, int n_fft,
                                                            int hop, int frames, float* __restrict__ grad_audio) {
    const int b = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N) return;
    const int p = n_fft >> 1;
    const float* g = gframes + (size_t)b * frames * n_fft;
    float acc = ms_frames_over(g, p + s, n_fft, hop, frames);
    if (s >= 1 && s <= p) acc += ms_frames_over(g, p - s, n_fft, hop, frames);
    if (s >= N - 1 - p && s <= N - 2) acc += ms_frames_over(g, p + 2 * (N - 1) - s, n_fft, hop, frames);
    grad_audio[(size_t)b * N + s] = acc;
}

// ---- pair loss ------------------------------------------------------------------------------------------------
const int PAIR_BLOCKS_MAX = 1024;

int pair_blocks(int64_t n) {     // four elements per thread until the grid is PAIR_BLOCKS_MAX wide, grid-stride beyond
    const int64_t nb = (n + 1023) / 1024;
    return (int)(nb < 1 ? 1 : (nb > PAIR_BLOCKS_MAX ? PAIR_BLOCKS_MAX : nb));
}

// block-wide sums of up to three values by wave shuffles, lane 0 of wave 0 adds the four wave sums in wave order
template <int K>
__device__ __forceinline__ void pair_block_sums(float (&v)[K], float* red /* 4*K floats */, float* out, int stride) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ms_wave_sum(v[k]);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[k * 4 + w] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            out[(size_t)k * stride + blockIdx.x] = ((red[k * 4] + red[k * 4 + 1]) + red[k * 4 + 2]) + red[k * 4 + 3];
    }
}

// partial[blockIdx.x] = this block's share of sum r^2
__global__ __launch_bounds__(256) void k_stft_pair_sumsq(const float* __restrict__ r, int64_t n,
                                                        float* __restrict__ partial) {
    __shared__ float red[4];
    float v[1] = {0.f};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        v[0] = fmaf(r[i], r[i], v[0]);
    pair_block_sums<1>(v, red, partial, gridDim.x);
}

// partial[0][blk] = sum (r - f)^2, partial[1][blk] = sum |log r - log f|
__global__ __launch_bounds__(256) void k_stft_pair_partial(const float* __restrict__ f, const float* __restrict__ r,
                                                          int64_t n, float* __restrict__ partial) {
    __shared__ float red[8];
    float v[2] = {0.f, 0.f};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float rv = r[i], fv = f[i], d = rv - fv;
        v[0] = fmaf(d, d, v[0]);
        v[1] += fabsf(logf(rv) - logf(fv));
    }
    pair_block_sums<2>(v, red, partial, gridDim.x);
}

// One workgroup adds the `rows` rows of `blocks` partials in block order (each thread a fixed strided share in double,
// then a fixed tree): sums[row0 + k].  With `out`: sums = {sum (r-f)^2, sum r^2, sum |log r - log f|} are complete
// (sum r^2 copied from the target's scalar) and out[0] = sc_weight * sqrt(s0 / s1) + mag_weight * s2 / n.
__global__ __launch_bounds__(256) void k_stft_pair_finish(const float* __restrict__ partial, int blocks, int rows,
                                                         const float* __restrict__ r_sumsq, int64_t n,
                                                         float sc_weight, float mag_weight,
                                                         float* __restrict__ sums, float* __restrict__ out) {
    __shared__ double red[256];
    double tot[2] = {0.0, 0.0};
    for (int k = 0; k < rows; ++k) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < blocks; i += 256) acc += (double)partial[(size_t)k * blocks + i];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        tot[k] = red[0];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if (!out) {            // the target's sum r^2
        sums[0] = (float)tot[0];
        return;
    }
    const float s0 = (float)tot[0], s1 = r_sumsq[0], s2 = (float)tot[1];
    sums[0] = s0;
    sums[1] = s1;
    sums[2] = s2;
    const float sc = (s0 > 0.f && s1 > 0.f) ? sqrtf(s0) / sqrtf(s1) : 0.f;
    out[0] = sc_weight * sc + mag_weight * (s2 / (float)n);
}

// grad_f = gout * (sc_weight * (f - r) / (||r|| ||r - f||) + mag_weight * sign(f - r) / (n f)), the norms read from
// the forward's device scalars
__global__ __launch_bounds__(256) void k_stft_pair_bwd(const float* __restrict__ f, const float* __restrict__ r,
                                                      int64_t n, const float* __restrict__ sums,
                                                      const float* __restrict__ gout, float sc_weight,
                                                      float mag_weight, float* __restrict__ grad_f) {
    const float g = gout[0], s0 = sums[0], s1 = sums[1];
    const float c_sc = (s0 > 0.f && s1 > 0.f) ? sc_weight * g / (sqrtf(s1) * sqrtf(s0)) : 0.f;
    const float c_lm = mag_weight * g / (float)n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float rv = r[i], fv = f[i];
        const float sg = fv > rv ? 1.f : (fv < rv ? -1.f : 0.f);
        grad_f[i] = fmaf(c_sc, fv - rv, sg != 0.f ? c_lm * sg / fv : 0.f);
    }
}

}  // namespace

extern "C" {

int ms_stft_frames(int32_t N, int32_t n_fft, int32_t hop) {
    if (N <= 0 || n_fft <= 0 || hop <= 0 || N <= n_fft / 2) return 0;
    return 1 + N / hop;
}

int ms_stft_mag_fwd(const float* audio, int32_t B, int32_t N, const float* window, int32_t n_fft, int32_t hop,
                    float min_power, float* mag, ms_stream_t stream) {
    if (!audio || !window || !mag || B <= 0 || N <= 0 || hop <= 0 || !(min_power >= 0.f)) return MS_ERR_INVALID_ARG;
    const int log2n = ms_frame_log2(n_fft);
    if (log2n < 0) return MS_ERR_UNSUPPORTED;
    const int frames = ms_stft_frames(N, n_fft, hop);
    if (frames <= 0) return MS_ERR_INVALID_ARG;
    if (B > 65535) return MS_ERR_UNSUPPORTED;     // rows are the grid's y dimension
    hipLaunchKernelGGL(k_stft_mag, dim3(frames, B), dim3(256), (size_t)2 * n_fft * sizeof(double), (hipStream_t)stream,
                       audio, N, window, n_fft, log2n, hop, frames, min_power, mag);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

size_t ms_stft_mag_bwd_workspace_bytes(int32_t B, int32_t N, int32_t n_fft, int32_t hop) {
    if (B <= 0 || ms_frame_log2(n_fft) < 0) return 0;
    const int frames = ms_stft_frames(N, n_fft, hop);
    if (frames <= 0) return 0;
    return (size_t)B * frames * n_fft * sizeof(float);     // the per-frame gradients
}

int ms_stft_mag_bwd(const float* audio, int32_t B, int32_t N, const float* window, int32_t n_fft, int32_t hop,
                    float min_power, const float* grad_mag, float* grad_audio, void* workspace,
                    size_t workspace_bytes, ms_stream_t stream) {
    if (!audio || !window || !grad_mag || !grad_audio || B <= 0 || N <= 0 || hop <= 0 || !(min_power >= 0.f))
        return MS_ERR_INVALID_ARG;
    const int log2n = ms_frame_log2(n_fft);
    if (log2n < 0) return MS_ERR_UNSUPPORTED;
    const int frames = ms_stft_frames(N, n_fft, hop);
    if (frames <= 0) return MS_ERR_INVALID_ARG;
    if (B > 65535) return MS_ERR_UNSUPPORTED;     // rows are the grid's y dimension
    const size_t need = ms_stft_mag_bwd_workspace_bytes(B, N, n_fft, hop);
    if (!workspace || workspace_bytes < need) return MS_ERR_WORKSPACE;
    float* gframes = (float*)workspace;
    hipLaunchKernelGGL(k_stft_mag_bwd_frame, dim3(frames, B), dim3(256), (size_t)2 * n_fft * sizeof(double),
                       (hipStream_t)stream, audio, N, window, n_fft, log2n, hop, frames, min_power, grad_mag, gframes);
    MS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_stft_mag_bwd_gather, dim3((N + 255) / 256, B), dim3(256), 0, (hipStream_t)stream,
                       (const float*)gframes, N, n_fft, hop, frames, grad_audio);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

size_t ms_stft_pair_loss_workspace_bytes(int64_t n) {
    return n <= 0 ? 0 : (size_t)2 * pair_blocks(n) * sizeof(float);
}

int ms_stft_pair_loss_target(const float* r, int64_t n, float* r_sumsq, void* workspace, size_t workspace_bytes,
                             ms_stream_t stream) {
    if (!r || !r_sumsq || n <= 0) return MS_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < ms_stft_pair_loss_workspace_bytes(n)) return MS_ERR_WORKSPACE;
    const int blocks = pair_blocks(n);
    float* partial = (float*)workspace;
    hipLaunchKernelGGL(k_stft_pair_sumsq, dim3(blocks), dim3(256), 0, (hipStream_t)stream, r, n, partial);
    MS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_stft_pair_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, blocks, 1,
                       (const float*)nullptr, n, 0.f, 0.f, r_sumsq, (float*)nullptr);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

int ms_stft_pair_loss_fwd(const float* f, const float* r, int64_t n, const float* r_sumsq, float sc_weight,
                          float mag_weight, float* sums, float* out, void* workspace, size_t workspace_bytes,
                          ms_stream_t stream) {
    if (!f || !r || !r_sumsq || !sums || !out || n <= 0) return MS_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < ms_stft_pair_loss_workspace_bytes(n)) return MS_ERR_WORKSPACE;
    const int blocks = pair_blocks(n);
    float* partial = (float*)workspace;
    hipLaunchKernelGGL(k_stft_pair_partial, dim3(blocks), dim3(256), 0, (hipStream_t)stream, f, r, n, partial);
    MS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_stft_pair_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partial, blocks, 2,
                       r_sumsq, n, sc_weight, mag_weight, sums, out);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

int ms_stft_pair_loss_bwd(const float* f, const float* r, int64_t n, const float* sums, const float* gout,
                          float sc_weight, float mag_weight, float* grad_f, ms_stream_t stream) {
    if (!f || !r || !sums || !gout || !grad_f || n <= 0) return MS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(k_stft_pair_bwd, dim3(pair_blocks(n)), dim3(256), 0, (hipStream_t)stream, f, r, n, sums, gout,
                       sc_weight, mag_weight, grad_f);
    MS_CHECK_LAUNCH();
    return MS_OK;
}

}  // extern "C"
