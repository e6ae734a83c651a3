"""The octave-band split and merge of the reference's featuresynth/audio/transform.py:50-115, same names, argument
order, dict key order and shapes, on HIP device tensors (csrc/bands.hip).  All three functions are differentiable: a
generator with recompose=True backpropagates through the merge, a discriminator with decompose=True through the split.

With X = rfft(x, norm="ortho"): band S of the split is irfft of X's bins S/4 .. S/2 (0 .. S/2 for the smallest band) on
S samples; the merge adds the same bin ranges of every band's rfft into one spectrum and inverts it once.  Neighbouring
bands both carry bin S/2, so split-then-merge is not the identity (2-3 % on noise), as in the reference.

Limits of the kernels (an error otherwise, never another code path): fp32 tensors on a HIP device, signal lengths powers
of two in [64, 32768], band sizes powers of two >= 16, at most 8 bands."""
from .._ops import bands as B


def _device_input(x, what):
    import torch
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise RuntimeError("%s: expected a (batch, channels, samples) tensor" % what)
    return x.contiguous()


def fft_frequency_decompose(x, min_size):
    """x (B, C, N) -> {min_size: (B, C, min_size), 2 min_size: .., .., N: (B, C, N)}, keys in ascending order."""
    x = _device_input(x, "fft_frequency_decompose")
    sizes, s = [], int(min_size)
    while 0 < s <= x.shape[-1]:
        sizes.append(s)
        s *= 2
    if not sizes:
        raise RuntimeError("fft_frequency_decompose: min_size %r does not fit %d samples" % (min_size, x.shape[-1]))
    return dict(zip(sizes, B.BandDecomposeFn.apply(x, tuple(sizes), True)))


def fft_resample(x, desired_size, is_lowest_band):
    """x (B, C, S) -> (B, C, desired_size): the band's bins S/4 .. S/2 (0 .. S/2 for the lowest band) on the finer grid."""
    x = _device_input(x, "fft_resample")
    return B.BandRecomposeFn.apply((int(x.shape[-1]),), bool(is_lowest_band), int(desired_size), x)


def fft_frequency_recompose(d, desired_size):
    """{S: (B, C, S)} -> (B, C, desired_size) = sum of fft_resample(band, desired_size, S == min(d)), computed as one
    summed spectrum and one inverse transform."""
    if not d:
        raise RuntimeError("fft_frequency_recompose: no bands")
    sizes = sorted(int(k) for k in d.keys())
    bands = [_device_input(d[s], "fft_frequency_recompose") for s in sizes]
    return B.BandRecomposeFn.apply(tuple(sizes), True, int(desired_size), *bands)
