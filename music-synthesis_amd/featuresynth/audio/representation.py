"""Audio representations with the surface of the reference's featuresynth/audio/representation.py: the base class
(:12-23), RawAudio (:38-54) and MultiScale (:82-103).  The display / listen helpers (zounds) and the MDCT / STFT /
phase-recovery classes are not part of this build.

MultiScale runs the band split and merge on the device (audio/transform.py).  numpy in gives numpy out, as in the
reference; in addition, device tensors are accepted and then stay on the device."""
import numpy as np
import torch

from ..util.device import device as DEVICE
from .transform import fft_frequency_decompose, fft_frequency_recompose


class BaseAudioRepresentation(object):
    def __init__(self, data, samplerate):
        super().__init__()
        self.samplerate = samplerate
        self.data = data

    @classmethod
    def from_audio(cls, samples, samplerate):
        raise NotImplementedError()

    def to_audio(self):
        raise NotImplementedError()


class RawAudio(BaseAudioRepresentation):
    @classmethod
    def from_audio(cls, samples, samplerate):
        return cls(samples, samplerate)

    def _reshape(self):
        batch, _, samples = self.data.shape
        return self.data.reshape((batch, samples))

    def to_audio(self):
        return self._reshape()


def _to_device(a):
    """-> (fp32 device tensor, whether `a` already was a tensor)"""
    if isinstance(a, torch.Tensor):
        return a.float(), True
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEVICE), False


class MultiScale(BaseAudioRepresentation):
    """data: {size: (B, 1, size)} over five octave bands, the largest 2^floor(log2 T) samples long."""
    levels = 5

    def to_audio(self):
        with torch.no_grad():
            mx = max(v.shape[-1] for v in self.data.values())
            moved = {k: _to_device(v) for k, v in self.data.items()}
            samples = fft_frequency_recompose({k: t for k, (t, _) in moved.items()}, mx).reshape((-1, mx))
            return samples if all(was for _, was in moved.values()) else samples.cpu().numpy()

    @classmethod
    def from_audio(cls, samples, samplerate):
        with torch.no_grad():
            time = samples.shape[-1]
            start = int(np.log2(time))
            levels = [2 ** i for i in range(start, start - cls.levels, -1)]
            t, was_tensor = _to_device(samples)
            data = fft_frequency_decompose(t, levels[-1])
            if not was_tensor:
                data = {k: v.cpu().numpy() for k, v in data.items()}
            return cls(data, samplerate)
