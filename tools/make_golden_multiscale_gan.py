#!/usr/bin/env python
"""Writes tests/golden/multiscale_gan.npz: one float32 D-step / G-step of the REFERENCE's multi-scale band GAN
(generator/multiscale.py MultiScaleGenerator, discriminator/multiscale.py MultiScaleMultiResDiscriminator, loss/loss.py),
run unmodified on the CPU.

The reference files are loaded by path at run time (tools/ref_import.py: empty parent packages whose __path__ points into
the reference tree).  `featuresynth.audio` is registered the same way, so that only audio/transform.py is imported; that
file calls torch.rfft / torch.irfft, which current torch no longer has, and imports zounds, which the band functions never
touch: two shims map the old calls onto torch.fft (norm="ortho") and an empty module stands in for zounds.  Nothing of the
reference is copied here.

    PYTHONDONTWRITEBYTECODE=1 MSYNTH_REFERENCE_ROOT=<checkout of the reference> python tools/make_golden_multiscale_gan.py

The case, the smallest the architecture admits (ReflectionPad1d(3) needs T >= 4; bands 64 .. 1024; every band's
discriminator trunk ends at length 4): T = 4 conditioning frames, N = 1024 samples, 128 mel channels, B = 2.
  generator      MultiScaleGenerator(128, 4, 1024, transposed_conv=True, recompose=True)
  discriminator  MultiScaleMultiResDiscriminator(1024, channel_judgements=True, conditioning_channels=128,
                                                 decompose=True, kernel_size=9)
  weights        default_rng(7).standard_normal(shape) * 0.02 in state_dict order, biases 0 (both networks)
  inputs         default_rng(1): normal features (B, 128, T), then uniform(-0.95, 0.95) samples (B, 1, N)

Stored (float32; tests/test_multiscale_gan_host.py, tests/test_gpu_multiscale_gan.py):
  feat, samples, fake, band_{size}                          the inputs, G(feat), the recompose=False bands of the same G
  {fake,real}_j{i}                                          the six judgements of D(fake, feat) / D(samples, feat)
  g_loss, d_loss                                            mel_gan_gen_loss / mel_gan_disc_loss, least-squares sub-losses
  families of tensors, each as {family}_names, _norms (L2 norm per tensor), _samples (the tensors' strided samples end
  to end) and _offsets (tensor i's sample is _samples[_offsets[i]:_offsets[i + 1]]):
    fake_features, real_features                            every feature map, named "{group}_{layer}"
    gstep_grads                                             generator gradients of g_loss, named by parameter
    dstep_grads                                             discriminator gradients of d_loss, named by parameter
  {g,d}_keys_{1024,8192}, {g,d}_shapes_{1024,8192}          state_dict keys and shapes at output_size 1024 and 8192
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "music-synthesis_amd")]

T, N, MELS, B = 4, 1024, 128, 2
NSAMPLE = 128


def strided_sample(a, n=NSAMPLE):
    flat = np.asarray(a).reshape(-1)
    step = max(1, flat.size // n)
    return flat[::step][:n].copy()


def record_family(out, family, named_arrays):
    names, norms, samples, offsets = [], [], [], [0]
    for name, a in named_arrays:
        a = np.asarray(a, np.float32)
        names.append(name)
        norms.append(np.linalg.norm(a.astype(np.float64)))
        samples.append(strided_sample(a))
        offsets.append(offsets[-1] + samples[-1].size)
    out[family + "_names"] = np.array(names)
    out[family + "_norms"] = np.asarray(norms, np.float32)
    out[family + "_samples"] = np.concatenate(samples).astype(np.float32)
    out[family + "_offsets"] = np.asarray(offsets, np.int64)


def load_networks():
    import ref_import
    torch.rfft = lambda input, signal_ndim, normalized: torch.view_as_real(torch.fft.rfft(input, norm="ortho"))
    torch.irfft = lambda input, signal_ndim, normalized, signal_sizes: torch.fft.irfft(
        torch.view_as_complex(input.contiguous()), n=signal_sizes[0], norm="ortho")
    ns = ref_import.load_reference()
    ref_import._pkg("featuresynth.audio", "featuresynth/audio")
    ns.gen = importlib.import_module("featuresynth.generator.multiscale")
    ns.disc = importlib.import_module("featuresynth.discriminator.multiscale")
    return ns


def synthetic_state_dict(module, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for name, v in module.state_dict().items():
        shape = tuple(v.shape)
        out[name] = np.zeros(shape, np.float32) if name.endswith("bias") \
            else (rng.standard_normal(shape) * 0.02).astype(np.float32)
    return out


def load_sd(module, sd):
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})


def networks(ns, size, frames, recompose=True):
    g = ns.gen.MultiScaleGenerator(MELS, frames, size, transposed_conv=True, recompose=recompose)
    d = ns.disc.MultiScaleMultiResDiscriminator(size, channel_judgements=True, conditioning_channels=MELS,
                                                decompose=True, kernel_size=9)
    return g, d


def record_keys(out, tag, module, size):
    sd = module.state_dict()
    out["%s_keys_%d" % (tag, size)] = np.array(list(sd.keys()))
    shapes = np.zeros((len(sd), 3), np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = v.shape
    out["%s_shapes_%d" % (tag, size)] = shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "multiscale_gan.npz"))
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    torch.manual_seed(0)
    ns = load_networks()
    L = ns.loss
    out = {}

    g, d = networks(ns, N, T)
    gsd, dsd = synthetic_state_dict(g, 7), synthetic_state_dict(d, 7)
    load_sd(g, gsd)
    load_sd(d, dsd)
    record_keys(out, "g", g, N)
    record_keys(out, "d", d, N)
    g8, d8 = networks(ns, 8192, 32)
    record_keys(out, "g", g8, 8192)
    record_keys(out, "d", d8, 8192)
    del g8, d8

    rng = np.random.default_rng(1)
    feat = rng.standard_normal((B, MELS, T)).astype(np.float32)
    samples = rng.uniform(-0.95, 0.95, (B, 1, N)).astype(np.float32)
    out["feat"], out["samples"] = feat, samples
    ft, st = torch.from_numpy(feat), torch.from_numpy(samples)

    # the bands of the same generator
    gb, _ = networks(ns, N, T, recompose=False)
    load_sd(gb, gsd)
    with torch.no_grad():
        bands = gb(ft)
    assert list(bands.keys()) == [N >> i for i in range(5)]
    for size, band in bands.items():
        out["band_%d" % size] = band.numpy()

    # G-step (train/train.py:26-42)
    g.zero_grad(); d.zero_grad()
    fake = g(ft)
    f_features, f_score = d(fake, ft)
    r_features, r_score = d(st, ft)
    g_loss = L.mel_gan_gen_loss(r_features, f_features, r_score, f_score, gan_loss=L.least_squares_generator_loss)
    g_loss.backward()
    out["fake"] = fake.detach().numpy()
    out["g_loss"] = np.float32(g_loss.item())
    assert len(f_score) == 6 and len(f_features) == 6
    for tag, feats, scores in (("fake", f_features, f_score), ("real", r_features, r_score)):
        for i, j in enumerate(scores):
            out["%s_j%d" % (tag, i)] = j.detach().numpy()
        record_family(out, tag + "_features", [("%d_%d" % (gi, li), f.detach().numpy())
                                               for gi, group in enumerate(feats) for li, f in enumerate(group)])
    record_family(out, "gstep_grads", [(name, p.grad.numpy()) for name, p in g.named_parameters()])

    # D-step (train/train.py:63-74)
    g.zero_grad(); d.zero_grad()
    fake = g(ft)
    _, f_score = d(fake, ft)
    _, r_score = d(st, ft)
    d_loss = L.mel_gan_disc_loss(r_score, f_score, gan_loss=L.least_squares_disc_loss)
    d_loss.backward()
    out["d_loss"] = np.float32(d_loss.item())
    record_family(out, "dstep_grads", [(name, p.grad.numpy()) for name, p in d.named_parameters()])

    for k, v in out.items():
        v = np.asarray(v)
        assert v.dtype in (np.float32, np.int64) or v.dtype.kind == "U", (k, v.dtype)
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print("%s: %d arrays, %d bytes" % (args.out, len(out), size))
    assert size < 200 * 1024


if __name__ == "__main__":
    main()
