"""Band split / merge on the device (csrc/bands.hip through include/msynth_bands.h): the four passes as functions on
contiguous fp32 HIP tensors, and the two autograd Functions featuresynth.audio.transform is built on.  A band set is a
list of (rows..., S) tensors in ascending S; what the kernels do not take (sizes that are no powers of two, more than
BAND_MAX bands, ...) raises -- there is no torch.fft fallback."""
import ctypes

import torch
from torch.autograd import Function

from . import lib as L


def _desc(sizes, tensors, lowest):
    d = L.BandDesc()
    d.count, d.lowest = len(sizes), 1 if lowest else 0
    for i, (s, t) in enumerate(zip(sizes, tensors)):
        d.size[i] = int(s)
        d.data[i] = L.ptr(t)
    return d


def _check_sizes(sizes, n, what):
    sizes = [int(s) for s in sizes]
    if not sizes or len(sizes) > L.BAND_MAX:
        raise RuntimeError("%s: 1 .. %d bands, got %d" % (what, L.BAND_MAX, len(sizes)))
    if any(b <= a for a, b in zip(sizes, sizes[1:])):
        raise RuntimeError("%s: band sizes must be strictly ascending, got %s" % (what, sizes))
    d = _desc(sizes, [None] * len(sizes), True)
    if not L.load().ms_band_supported(int(n), d):
        raise RuntimeError("%s: signals of %d samples in bands of %s are not supported (a power of two in [64, 32768], "
                           "bands powers of two in [16, that])" % (what, n, sizes))
    return sizes


def _rows(shape):
    r = 1
    for v in shape[:-1]:
        r *= int(v)
    if r <= 0:
        raise RuntimeError("band transform: empty batch %s" % (tuple(shape),))
    return r


def _ws(rows, n, d, device):
    nws = L.load().ms_band_workspace_bytes(rows, n, d)
    return L.workspace(nws, device), nws


def analysis(name, x, sizes, lowest, wanted=None):
    """ms_band_decompose_fwd / ms_band_recompose_bwd: x (.., n) -> one (.., S) tensor per size (None where not wanted)."""
    L.require(x, name + " input")
    n, lead = int(x.shape[-1]), tuple(x.shape[:-1])
    sizes = _check_sizes(sizes, n, name)
    rows = _rows(x.shape)
    outs = [torch.empty(lead + (s,), dtype=torch.float32, device=x.device) if (wanted is None or wanted[i]) else None
            for i, s in enumerate(sizes)]
    if all(o is None for o in outs):
        return outs
    d = _desc(sizes, outs, lowest)
    ws, nws = _ws(rows, n, d, x.device)
    L.call(name, None, x.data_ptr(), rows, n, ctypes.byref(d), L.ptr(ws), nws, L.stream())
    return outs


def synthesis(name, bands, sizes, lowest, n):
    """ms_band_recompose_fwd / ms_band_decompose_bwd: one (.., S) tensor per size (None: a zero band, backward only)
    -> (.., n)."""
    have = [b for b in bands if b is not None]
    if not have:
        raise RuntimeError("%s: no band given" % name)
    lead = tuple(have[0].shape[:-1])
    for b, s in zip(bands, sizes):
        if b is None:
            continue
        L.require(b, "%s band %d" % (name, s))
        if tuple(b.shape) != lead + (int(s),):
            raise RuntimeError("%s: band %d has shape %s, expected %s" % (name, s, tuple(b.shape), lead + (int(s),)))
    sizes = _check_sizes(sizes, n, name)
    rows = _rows(have[0].shape)
    y = torch.empty(lead + (int(n),), dtype=torch.float32, device=have[0].device)
    d = _desc(sizes, bands, lowest)
    ws, nws = _ws(rows, n, d, y.device)
    L.call(name, None, ctypes.byref(d), rows, int(n), y.data_ptr(), L.ptr(ws), nws, L.stream())
    return y


class BandDecomposeFn(Function):
    """x (.., n) -> the bands of `sizes` (ascending; band 0 is the lowest band when `lowest`).  Linear: nothing is saved.
    Bands whose cotangent is None reach the kernel as null pointers."""

    @staticmethod
    def forward(ctx, x, sizes, lowest):
        ctx.geom = (tuple(sizes), bool(lowest), int(x.shape[-1]))
        ctx.set_materialize_grads(False)
        return tuple(analysis("ms_band_decompose_fwd", x, sizes, lowest))

    @staticmethod
    def backward(ctx, *grads):
        sizes, lowest, n = ctx.geom
        if not ctx.needs_input_grad[0] or all(g is None for g in grads):
            return None, None, None
        grads = [None if g is None else g.contiguous() for g in grads]
        return synthesis("ms_band_decompose_bwd", grads, sizes, lowest, n), None, None


class BandRecomposeFn(Function):
    """The bands of `sizes` (ascending) -> (.., n): spectra summed, one inverse transform.  Linear: nothing is saved."""

    @staticmethod
    def forward(ctx, sizes, lowest, n, *bands):
        ctx.geom = (tuple(sizes), bool(lowest), int(n))
        return synthesis("ms_band_recompose_fwd", list(bands), sizes, lowest, n)

    @staticmethod
    def backward(ctx, g):
        sizes, lowest, n = ctx.geom
        wanted = list(ctx.needs_input_grad[3:])
        outs = analysis("ms_band_recompose_bwd", g.contiguous(), sizes, lowest, wanted)
        return (None, None, None) + tuple(outs)
