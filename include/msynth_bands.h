/* Multi-scale band representation: the octave-band split and merge of the reference's audio/transform.py
 * (fft_frequency_decompose :50-82, fft_resample :85-104, fft_frequency_recompose :107-115) and their exact adjoints, as
 * HIP kernels for gfx950 (csrc/bands.hip).  Same conventions as msynth.h: caller-owned fp32 buffers, status codes
 * (ms_status), no allocation, no synchronisation; every launch goes to `stream`.
 *
 * With X[k] = n^-1/2 sum_t x[t] exp(-2 pi i k t / n), k = 0 .. n/2 (bin indices inclusive):
 *
 *   split   band_S = irfft_ortho(C_S, S),  C_S[k] = X[k] for lo_S <= k <= S/2, 0 below lo_S
 *   merge   y      = irfft_ortho(Y, n),    Y[k]   = sum over bands of rfft_ortho(band_S)[k] for lo_S <= k <= S/2
 *
 * lo_S = S/4, except for band 0 of a descriptor with lowest = 1, where it is 0.  The real-output inverse reads only the
 * real parts of bins 0 and S/2 (as torch's c2r transform does), and neighbouring bands both carry bin S/2: a split
 * followed by a merge is NOT the identity, in the reference either.
 *
 * Supported: n a power of two in [64, 32768]; 1 .. MS_BAND_MAX bands, sizes powers of two >= 16, strictly ascending,
 * none above n.  Anything else returns MS_ERR_UNSUPPORTED (sizes out of order: MS_ERR_INVALID_ARG) and writes nothing.
 * Every result is bitwise repeatable (no atomics), and no pass needs scratch: ms_band_workspace_bytes() is 0 today, the
 * workspace arguments are kept so that a later kernel may use one without an ABI change.
 */
#ifndef MSYNTH_BANDS_H
#define MSYNTH_BANDS_H

#include "msynth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MS_BAND_MAX 8

/* The bands of one call: data[i] is a contiguous (rows, size[i]) fp32 tensor, 4-byte aligned.  Copied by value into
 * the launch: the caller may reuse the struct as soon as the call returns. */
typedef struct ms_band_desc {
    int32_t count;              /* 1 .. MS_BAND_MAX */
    int32_t lowest;             /* 1: band 0 is the lowest band (bins 0 .. S/2); 0: bins S/4 .. S/2 like the others */
    int32_t size[MS_BAND_MAX];  /* strictly ascending */
    float* data[MS_BAND_MAX];
} ms_band_desc;

/* 1 when the four passes take signals of n samples with these band sizes (pointers are not looked at), else 0 */
int ms_band_supported(int32_t n, const ms_band_desc* bands);
/* bytes of workspace any of the four passes needs for `rows` rows (0: all of them run out of LDS) */
size_t ms_band_workspace_bytes(int32_t rows, int32_t n, const ms_band_desc* bands);

/* split: x (rows, n) -> bands->data[i] (rows, size[i]), all non-null.  fft_frequency_decompose(x, m) is the call with
 * sizes m, 2m, .., n and lowest = 1. */
int ms_band_decompose_fwd(const float* x, int32_t rows, int32_t n, const ms_band_desc* bands, void* workspace,
                          size_t workspace_bytes, ms_stream_t stream);
/* adjoint of the split: grad_x (rows, n) from the band cotangents grad_bands->data[i]; a null pointer is a band whose
 * cotangent is zero (at least one must be non-null). */
int ms_band_decompose_bwd(const ms_band_desc* grad_bands, int32_t rows, int32_t n, float* grad_x, void* workspace,
                          size_t workspace_bytes, ms_stream_t stream);
/* merge: bands->data[i] (rows, size[i]), all non-null -> y (rows, n): the spectra are summed in LDS and inverted once.
 * fft_frequency_recompose(d, n) is the call with lowest = 1; fft_resample(x, n, is_lowest_band) the call with one band
 * and lowest = is_lowest_band. */
int ms_band_recompose_fwd(const ms_band_desc* bands, int32_t rows, int32_t n, float* y, void* workspace,
                          size_t workspace_bytes, ms_stream_t stream);
/* adjoint of the merge: grad_bands->data[i] (rows, size[i]) from grad_y (rows, n); a null pointer is a band whose
 * gradient is not wanted (at least one must be non-null). */
int ms_band_recompose_bwd(const float* grad_y, int32_t rows, int32_t n, const ms_band_desc* grad_bands, void* workspace,
                          size_t workspace_bytes, ms_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
