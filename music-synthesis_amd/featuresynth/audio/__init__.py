from .representation import BaseAudioRepresentation, MultiScale, RawAudio  # noqa: F401
from .transform import fft_frequency_decompose, fft_frequency_recompose, fft_resample  # noqa: F401
