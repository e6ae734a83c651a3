"""The band split / merge of the reference's audio/transform.py (fft_frequency_decompose :50-82, fft_resample :85-104,
fft_frequency_recompose :107-115) restated on torch.fft, in the dtype of its input -- float64 is the oracle of the band
tests, float32 the stock-library yardstick their tolerance is derived from (the reference itself allocates fft_resample's
spectrum in float32 whatever it is given, so running it in double is no oracle).  Plus the adjoints written out by hand,
which is what the HIP backward passes implement; tests/test_bands_host.py holds them against autograd.

With X = rfft(x, norm="ortho") (bins 0 .. n/2, inclusive):
  split   out[S] = irfft(C_S, S, ortho), C_S[k] = X[k] for lo_S <= k <= S/2 and 0 below, S = m, 2m, .., n
  merge   y = irfft(Y, D, ortho), Y[k] = sum_S rfft(band_S, ortho)[k] over lo_S <= k <= S/2
lo_S = 0 for the lowest band and S/4 for every other one; irfft reads only the real parts of bins 0 and S/2.
"""
import torch


def band_sizes(n, min_size):
    sizes, s = [], int(min_size)
    while s <= n:
        sizes.append(s)
        s *= 2
    return sizes


def _lo(size, lowest):
    return 0 if lowest else size // 4


def decompose(x, min_size):
    """x (B, C, n) -> {S: (B, C, S)} in ascending S."""
    X = torch.fft.rfft(x, norm="ortho")
    out = {}
    for S in band_sizes(x.shape[-1], min_size):
        C = X[..., :S // 2 + 1].clone()
        C[..., :_lo(S, S == min_size)] = 0
        out[S] = torch.fft.irfft(C, n=S, norm="ortho")
    return out


def resample(x, desired_size, is_lowest_band):
    S = x.shape[-1]
    c = torch.fft.rfft(x, norm="ortho")
    Y = torch.zeros(x.shape[:-1] + (desired_size // 2 + 1,), dtype=c.dtype, device=x.device)
    lo = _lo(S, is_lowest_band)
    Y[..., lo:S // 2 + 1] = c[..., lo:]
    return torch.fft.irfft(Y, n=desired_size, norm="ortho")


def recompose(d, desired_size):
    first = min(d.keys())
    return sum(resample(band, desired_size, size == first) for size, band in d.items())


# ---- the adjoints, by hand ----------------------------------------------------------------------------------------
# <irfft_S(C), g> = sum_k w_k <C_k, G_k> with G = rfft_S(g), w = 1 at k = 0 and S/2 (real parts only), 2 between;
# <rfft_n(x), H> = <x, irfft_n(H')> with H' = H at k = 0 and n/2 (real parts only), H / 2 between.

def _irfft_t(g):
    """Transpose of irfft(., S, ortho): (.., S) -> (.., S/2+1) complex."""
    G = torch.fft.rfft(g, norm="ortho")
    w = torch.full((G.shape[-1],), 2.0, dtype=g.dtype, device=g.device)
    w[0] = w[-1] = 1.0
    G = G * w
    G[..., 0] = G[..., 0].real + 0j
    G[..., -1] = G[..., -1].real + 0j
    return G


def _rfft_t(H, n):
    """Transpose of rfft(., ortho) on n samples: (.., n/2+1) complex -> (.., n)."""
    w = torch.full((H.shape[-1],), 0.5, dtype=H.real.dtype, device=H.device)
    w[0] = w[-1] = 1.0
    return torch.fft.irfft(H * w, n=n, norm="ortho")


def decompose_adjoint(g, n, min_size):
    """g {S: (B, C, S) or None} -> grad_x (B, C, n): the transpose of decompose."""
    H = None
    for S in band_sizes(n, min_size):
        gs = g.get(S)
        if gs is None:
            continue
        G = _irfft_t(gs)
        G[..., :_lo(S, S == min_size)] = 0
        if H is None:
            H = torch.zeros(gs.shape[:-1] + (n // 2 + 1,), dtype=G.dtype, device=G.device)
        H[..., :S // 2 + 1] += G
    return _rfft_t(H, n)


def recompose_adjoint(g, sizes, desired_size):
    """g (B, C, D) -> {S: (B, C, S)}: the transpose of recompose for bands of the given sizes."""
    G = _irfft_t(g)
    first = min(sizes)
    out = {}
    for S in sizes:
        H = G[..., :S // 2 + 1].clone()
        H[..., :_lo(S, S == first)] = 0
        out[S] = _rfft_t(H, S)
    return out


def resample_adjoint(g, size, is_lowest_band):
    H = _irfft_t(g)[..., :size // 2 + 1].clone()
    H[..., :_lo(size, is_lowest_band)] = 0
    return _rfft_t(H, size)
