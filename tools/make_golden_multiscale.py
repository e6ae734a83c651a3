#!/usr/bin/env python
"""Writes tests/golden/multiscale.npz: inputs and the float32 outputs of the REFERENCE's band split / merge
(featuresynth/audio/transform.py: fft_frequency_decompose, fft_resample, fft_frequency_recompose), run unmodified.

The reference file is loaded by path.  It calls torch.rfft / torch.irfft, which current torch no longer has, and imports
zounds, which its three band functions never touch: two shims map the old calls onto torch.fft (norm="ortho") and an
empty module stands in for zounds.  Nothing of the reference is copied here.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_multiscale.py --reference <checkout of the reference>

Cases (tests/test_bands_host.py, tests/test_gpu_bands.py):
  a  N = 256,  m = 16,  B = 3, C = 2: the split, its merge to D = 256 and to D = 1024, fft_resample of band 16 to D = 64
  b  N = 2048, m = 128, B = 2, C = 1: the split, its merge to D = 2048, fft_resample of band 128 to D = 512
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"a": dict(N=256, m=16, B=3, C=2, merges=(256, 1024), resample=64),
         "b": dict(N=2048, m=128, B=2, C=1, merges=(2048,), resample=512)}


def load_reference(path):
    torch.rfft = lambda input, signal_ndim, normalized: torch.view_as_real(torch.fft.rfft(input, norm="ortho"))
    torch.irfft = lambda input, signal_ndim, normalized, signal_sizes: torch.fft.irfft(torch.view_as_complex(input.contiguous()), n=signal_sizes[0], norm="ortho")
    sys.modules.setdefault("zounds", types.ModuleType("zounds"))
    spec = importlib.util.spec_from_file_location("reference_audio_transform", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "multiscale.npz"))
    args = ap.parse_args()
    ref = load_reference(os.path.join(args.reference, "featuresynth", "audio", "transform.py"))
    out = {}
    for name, c in CASES.items():
        rng = np.random.default_rng(20 + ord(name))
        x = rng.standard_normal((c["B"], c["C"], c["N"])).astype(np.float32)
        out[name + "_x"] = x
        bands = ref.fft_frequency_decompose(torch.from_numpy(x), c["m"])
        assert list(bands.keys()) == [c["m"] << i for i in range(len(bands))]
        for size, band in bands.items():
            out["%s_band_%d" % (name, size)] = band.numpy()
        for D in c["merges"]:
            out["%s_merge_%d" % (name, D)] = ref.fft_frequency_recompose(bands, D).numpy()
        for lowest in (True, False):
            out["%s_resample_%d_%s" % (name, c["resample"], "lowest" if lowest else "other")] = \
                ref.fft_resample(bands[c["m"]], c["resample"], lowest).numpy()
    for k, v in out.items():
        assert v.dtype == np.float32, k
    np.savez(args.out, **out)
    print("%s: %d arrays, %d bytes" % (args.out, len(out), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
