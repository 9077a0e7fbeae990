"""Drop-in import shim for `from audio_utils import WhisperSegFeatureExtractor, get_n_fft_given_sr, get_sampling_rate, get_audio_duration`."""
from whisperseg_amd.audio_utils import (WhisperSegFeatureExtractor, get_audio_duration, get_n_fft_given_sr,  # noqa: F401
                                        get_sampling_rate)
