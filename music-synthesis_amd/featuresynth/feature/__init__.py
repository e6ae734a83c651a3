from .feature import Audio2Mel, STFTMagnitude, audio_from_samples, resample  # noqa: F401
