"""GAN losses of the hot path with the call signatures of the reference's
featuresynth/loss/loss.py (hinge :9-18, least squares :5-14, mel_gan_disc_loss :21-25,
mel_gan_feature_loss :28-65, mel_gan_gen_loss :68-78), plus the mel-spectrogram L1 term of later MelGAN-family
training (MelReconstructionLoss, MultiResolutionSTFTLoss, SpectralLossSum; no counterpart in the reference).  Each returns a 0-d tensor with autograd;
the reductions are wavefront-shuffle HIP kernels and the composite losses are single autograd
nodes (one fused backward over the 18 feature maps).
"""
import torch
from torch import nn

from .._ops import functional as F_
from .._ops import prims as P


def least_squares_generator_loss(j):
    """0.5 * mean((j - 1)^2)"""
    return F_.LsGFn.apply(j)


def hinge_generator_loss(j):
    """mean(-j)"""
    return F_.NegMeanFn.apply(j)


def least_squares_disc_loss(r_j, f_j):
    """0.5 * (mean((r - 1)^2) + mean(f^2))"""
    return F_.LsDFn.apply(r_j, f_j)


def hinge_discriminator_loss(r_j, f_j):
    """mean(relu(1 - r) + relu(1 + f))"""
    return F_.HingeDFn.apply(r_j, f_j)


def mel_gan_disc_loss(real_judgements, fake_judgements, gan_loss=hinge_discriminator_loss):
    real_judgements, fake_judgements = list(real_judgements), list(fake_judgements)
    if gan_loss is hinge_discriminator_loss and len(real_judgements) == len(fake_judgements) > 0:
        return F_.MelGanDiscLossFn.apply(len(real_judgements), *real_judgements, *fake_judgements)
    total = None
    for r, f in zip(real_judgements, fake_judgements):
        term = gan_loss(r, f)
        total = term if total is None else total + term
    return total


def _balanced(real_features, fake_features):
    if len(real_features) != len(fake_features) or not real_features:
        return False
    n = len(real_features[0])
    return n > 0 and all(len(g) == n for g in real_features) and all(len(g) == n for g in fake_features)


def mel_gan_feature_loss(real_features, fake_features):
    """sum over discriminators d and layers l of (1/D)(1/L_d) * l1(real, fake); the reference
    settles on this scaling after the discussion in its comment block (loss.py:41-60)."""
    nd = 1.0 / len(real_features)
    total = None
    for r_group, f_group in zip(real_features, fake_features):
        nl = 1.0 / len(r_group)
        for r_f, f_f in zip(r_group, f_group):
            term = (nl * nd) * F_.L1MeanFn.apply(r_f, f_f)
            total = term if total is None else total + term
    return total


def mel_gan_gen_loss(real_features, fake_features, real_judgements, fake_judgements,
                     gan_loss=hinge_generator_loss, feature_loss_weight=10):
    real_features = [list(g) for g in real_features]
    fake_features = [list(g) for g in fake_features]
    fake_judgements = list(fake_judgements)
    if gan_loss is hinge_generator_loss and _balanced(real_features, fake_features) and \
            len(fake_judgements) == len(fake_features):
        S, Lyr = len(fake_features), len(fake_features[0])
        flat_r = [t for g in real_features for t in g]
        flat_f = [t for g in fake_features for t in g]
        return F_.MelGanGenLossFn.apply(S, Lyr, float(feature_loss_weight), *flat_r, *flat_f,
                                        *fake_judgements)
    j_loss = None
    for _, f in zip(real_judgements, fake_judgements):
        term = gan_loss(f)
        j_loss = term if j_loss is None else j_loss + term
    return j_loss + feature_loss_weight * mel_gan_feature_loss(real_features, fake_features)


class MelReconstructionLoss(object):
    """weight * mean(|A2M(fake) - A2M(samples)|) for an Audio2Mel module A2M (feature/feature.py): the mel-spectrogram
    L1 term a GAN vocoder's generator step adds to its adversarial loss (GeneratorTrainer.spectral_loss).  The real
    side carries no gradient; the fake side backpropagates through the HIP Audio2Mel backward (csrc/audio2mel.hip)."""

    def __init__(self, audio2mel, weight=45.0):
        self.audio2mel = audio2mel
        self.weight = float(weight)

    def target(self, samples):
        """A2M(samples), computed under no_grad (the trainer runs it beside D(samples) on the real-path stream)."""
        with torch.no_grad():
            return self.audio2mel(samples)

    def __call__(self, fake, samples, target=None):
        real = self.target(samples) if target is None else target
        return self.weight * F_.L1MeanFn.apply(real, self.audio2mel(fake))


class MultiResolutionSTFTLoss(nn.Module):
    """weight * (1/M) * sum_m (sc_weight * sc_m + mag_weight * lm_m) over M (n_fft, hop, win_length) resolutions, with
    F_m / R_m the feature.STFTMagnitude of the fake / real audio at resolution m:

        sc_m = ||R_m - F_m||_2 / ||R_m||_2   (spectral convergence, Frobenius norms over the batch)
        lm_m = mean |log R_m - log F_m|      (log-magnitude L1)

    The real side carries no gradient; the fake side backpropagates through the HIP STFT backward (csrc/stft_mag.hip).
    A Module, so .to(device) / .cuda() move the windows of `stfts`."""

    DEFAULT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))

    def __init__(self, resolutions=DEFAULT_RESOLUTIONS, weight=1.0, sc_weight=1.0, mag_weight=1.0, min_power=1e-7):
        super().__init__()
        from ..feature.feature import STFTMagnitude
        self.resolutions = tuple(tuple(int(v) for v in r) for r in resolutions)
        if not self.resolutions or any(len(r) != 3 for r in self.resolutions):
            raise ValueError("MultiResolutionSTFTLoss: resolutions are (n_fft, hop, win_length) triples")
        self.stfts = nn.ModuleList([STFTMagnitude(n, h, w, min_power) for n, h, w in self.resolutions])
        self.weight = float(weight)
        self.sc_weight = float(sc_weight)
        self.mag_weight = float(mag_weight)
        self.min_power = float(min_power)

    def target(self, samples):
        """((R_m, sum R_m^2) for every resolution), computed under no_grad (the trainer runs it beside D(samples) on
        the real-path stream)."""
        with torch.no_grad():
            mags = [stft(samples) for stft in self.stfts]
            return tuple((r, P.stft_pair_target(P.frame_major(r, "real magnitudes"))) for r in mags)

    def forward(self, fake, samples, target=None):
        if fake.shape != samples.shape:
            raise RuntimeError("MultiResolutionSTFTLoss: fake %s and samples %s differ in shape"
                               % (tuple(fake.shape), tuple(samples.shape)))
        target = self.target(samples) if target is None else target
        total = None
        for stft, (real, r_sumsq) in zip(self.stfts, target):
            term = F_.STFTPairLossFn.apply(stft(fake), real, r_sumsq, self.sc_weight, self.mag_weight)
            total = term if total is None else total + term
        return (self.weight / len(self.stfts)) * total


class SpectralLossSum(object):
    """The sum of several spectral terms as one GeneratorTrainer.spectral_loss, e.g.
    SpectralLossSum(MelReconstructionLoss(a2m), MultiResolutionSTFTLoss().cuda())."""

    def __init__(self, *terms):
        if not terms:
            raise ValueError("SpectralLossSum: at least one term")
        self.terms = tuple(terms)

    def target(self, samples):
        """The tuple of the terms' targets (None for a term without a target method)."""
        return tuple(t.target(samples) if callable(getattr(t, "target", None)) else None for t in self.terms)

    def __call__(self, fake, samples, target=None):
        if target is None:
            target = self.target(samples)
        if len(target) != len(self.terms):
            raise RuntimeError("SpectralLossSum: %d targets for %d terms" % (len(target), len(self.terms)))
        total = None
        for term, tgt in zip(self.terms, target):
            v = term(fake, samples) if tgt is None else term(fake, samples, target=tgt)
            total = v if total is None else total + v
        return total
