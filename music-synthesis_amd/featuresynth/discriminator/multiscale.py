"""The multi-scale band discriminator of the reference's featuresynth/discriminator/multiscale.py (ChannelDiscriminator
:11-67, MultiScaleDiscriminator :255-366, MultiScaleMultiResDiscriminator :369-410) on the gfx950 kernels: same class
names, constructor signatures (defaults included), forward return structures and state_dict keys
(`multiscale.channel_{size}.main.{i}.*`, `...mj.{i}.*`, `...judge.*`, `multiscale.final.{i}.*`, `multiscale.judge.*`).

Every band has its own trunk of strided dense convs (LeakyReLU(0.2) fused, each output a feature map); with
channel_judgements a band also judges on its own, after the conditioning frames are stacked behind its last feature
map.  The `final` head runs over the channel concatenation of all trunks (plus the conditioning, repeated to their
length).  decompose=True splits a (B, 1, N) tensor into the bands (audio.fft_frequency_decompose), decompose=False
takes the dict of bands.  torch.cat and the nearest-neighbour repeat of the conditioning are data movement and stay
torch ops.

Not built: the FilterBank* classes (they need zounds.learn.FilterBank)."""
from functools import reduce

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from ..audio.transform import fft_frequency_decompose
from ..util.modules import HipConv1d


class ChannelDiscriminator(nn.Module):
    def __init__(self, scale_factors, channels, return_judgements=False, conditioning_channels=0, kernel_size=41):
        super().__init__()
        self.kernel_size = kernel_size
        self.conditioning_channels = conditioning_channels
        self.return_judgements = return_judgements
        self.channels = channels
        self.scale_factors = scale_factors
        self.main = nn.Sequential(*[
            HipConv1d(channels[i], channels[i + 1], self.kernel_size, stride=scale_factors[i],
                      padding=self.kernel_size // 2, activation="lrelu")
            for i in range(len(scale_factors))])
        if self.return_judgements:
            start_channels = channels[-1] + (conditioning_channels if conditioning_channels > 0 else 0)
            self.mj = nn.Sequential(
                HipConv1d(start_channels, channels[-1], 3, 1, 1, activation="lrelu"),
                HipConv1d(channels[-1], channels[-1], 3, 1, 1, activation="lrelu"),
                HipConv1d(channels[-1], channels[-1], 3, 1, 1, activation="lrelu"))
            self.judge = HipConv1d(channels[-1], 1, 3, 1, 1)

    def forward(self, x, feat=None):
        features = []
        for layer in self.main:
            x = layer(x)
            features.append(x)
        if not self.return_judgements:
            return features, x
        if self.conditioning_channels > 0:
            x = torch.cat([x, feat], dim=1)
        for layer in self.mj:
            x = layer(x)
            features.append(x)
        j = self.judge(x)
        return features, x, j


class MultiScaleDiscriminator(nn.Module):
    def __init__(self, input_size, decompose=True, channel_judgements=False, conditioning_channels=0,
                 kernel_size=41):
        super().__init__()
        self.kernel_size = kernel_size
        self.conditioning_channels = conditioning_channels
        self.channel_judgements = channel_judgements
        self.decompose = decompose
        self.input_size = input_size
        band_sizes = [int(2 ** (np.log2(self.input_size) - i)) for i in range(5)]
        factors = [[4, 4, 4, 4], [4, 4, 4, 2], [4, 4, 2, 2], [4, 2, 2, 2], [2, 2, 2, 2]]
        # keys in descending order of band size, e.g. [8192, 4096, 2048, 1024, 512]
        self.spec = {bs: {'scale_factors': f, 'channels': [1, 32, 64, 128, 256]}
                     for bs, f in zip(band_sizes, factors)}
        self.smallest_band = min(self.spec.keys())

        self.channel_discs = {}
        for key, value in self.spec.items():
            disc = ChannelDiscriminator(**value, return_judgements=self.channel_judgements,
                                        conditioning_channels=self.conditioning_channels, kernel_size=kernel_size)
            self.add_module('channel_%d' % key, disc)
            self.channel_discs[key] = disc

        final_channels = sum(v['channels'][-1] for v in self.spec.values())
        channels = 512
        self.final = nn.Sequential(
            HipConv1d(final_channels + self.conditioning_channels, channels, 3, 1, 1, activation="lrelu"),
            HipConv1d(channels, channels, 3, 1, 1, activation="lrelu"),
            HipConv1d(channels, channels, 3, 1, 1, activation="lrelu"))
        self.judge = HipConv1d(channels, 1, 3, 1, 1)
        self.recon = None

    def forward(self, x, feat=None):
        features = []
        channels = []
        judgements = []
        bands = fft_frequency_decompose(x, self.smallest_band) if self.decompose else x
        for size, layer in self.channel_discs.items():
            if self.channel_judgements:
                f, x, j = layer(bands[size], feat)
                judgements.append(j)
            else:
                f, x = layer(bands[size])
            features.append(f)
            channels.append(x)
        x = torch.cat(channels, dim=1)
        if self.conditioning_channels > 0:
            feat = F.interpolate(feat, size=x.shape[-1])       # (nearest: the reference's F.upsample default)
            x = torch.cat([x, feat], dim=1)
        final_features = []
        for layer in self.final:
            x = layer(x)
            final_features.append(x)
        features.append(final_features)
        x = self.judge(x)
        judgements.append(x)
        return features, judgements


class MultiScaleMultiResDiscriminator(nn.Module):
    _ms_native = True   # featuresynth.train: skip-discarded-work + hipGraph path applies

    def __init__(self, input_size, flatten_multiscale_features=False, decompose=True, channel_judgements=False,
                 conditioning_channels=0, kernel_size=41):
        super().__init__()
        self.kernel_size = kernel_size
        self.conditioning_channels = conditioning_channels
        self.input_size = input_size
        self.flatten_multiscale_features = flatten_multiscale_features
        self.multiscale = MultiScaleDiscriminator(input_size, decompose, channel_judgements, conditioning_channels,
                                                  kernel_size)

    def forward(self, x, feat=None):
        features = []
        judgements = []
        f, j = self.multiscale(x, feat)
        if self.flatten_multiscale_features:
            # the features of every band as a single group, so that they do not dominate the feature-matching loss
            features.append(reduce(lambda a, b: a + b, f, []))
        else:
            features.extend(f)
        judgements.extend(j)
        return features, judgements
