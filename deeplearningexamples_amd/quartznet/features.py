"""The log-mel front end of QuartzNet on the host CPU, in torch: FilterbankFeatures.calculate_features of
SpeechRecognition/QuartzNet/common/features.py:200-288 up to and including the logarithm.  What follows there -- normalize_batch
"per_feature", the mask and the cast (features.py:158-170, 290-302) -- runs on the device (functional.qn_normalize_pack).

Per utterance, in fp32: dither (x + dither * randn, under the caller's seed; 0 switches it off), preemphasis 0.97 (the first sample
kept), torch.stft(n_fft, hop, window length, Hann window with periodic=False; centred, reflect padding: torch's defaults, as
features.py:252-257 calls it), power spectrum re^2 + im^2, the mel bank, log(x + 1e-20).  get_seq_len is ceil(samples / hop)
(features.py:247-249); the STFT gives samples // hop + 1 frames, the frames behind the length are dropped here (the reference
masks them).

The mel bank is tacotron2.audio.mel_filter_bank (Slaney scale, Slaney normalisation: what librosa.filters.mel computes by default);
librosa is not installed, so its parity with librosa stays UNPINNED here exactly as it is for Tacotron2.
"""
import math

import torch

from ..tacotron2.audio import mel_filter_bank

WINDOWS = {"hann": torch.hann_window, "hamming": torch.hamming_window, "blackman": torch.blackman_window,
           "bartlett": torch.bartlett_window}


class FilterbankFeatures:
    def __init__(self, sample_rate=16000, window_size=0.02, window_stride=0.01, window="hann", normalize="per_feature", n_fft=None,
                 preemph=0.97, n_filt=64, lowfreq=0, highfreq=None, log=True, dither=1e-5, pad_align=16, frame_splicing=1, **ignored):
        if normalize != "per_feature":
            raise ValueError("normalize %r: only per_feature is built" % (normalize,))
        if frame_splicing != 1:
            raise ValueError("frame_splicing %r: only 1 is built" % (frame_splicing,))
        if not log:
            raise ValueError("log false: only log features are built")
        if window not in WINDOWS:
            raise ValueError("window %r: one of %s" % (window, ", ".join(sorted(WINDOWS))))
        self.sample_rate = int(sample_rate)
        self.win_length = int(self.sample_rate * window_size)
        self.hop_length = int(self.sample_rate * window_stride)
        self.n_fft = int(n_fft) if n_fft else 2 ** math.ceil(math.log2(self.win_length))
        self.n_filt, self.preemph, self.dither = int(n_filt), preemph, float(dither)
        self.window = WINDOWS[window](self.win_length, periodic=False, dtype=torch.float32)
        self.fb = torch.from_numpy(mel_filter_bank(self.sample_rate, self.n_fft, self.n_filt, lowfreq,
                                                   highfreq or self.sample_rate / 2)).to(torch.float32)

    def get_seq_len(self, samples):
        return int(math.ceil(samples / self.hop_length))

    @torch.no_grad()
    def log_mel(self, wave, generator=None):
        """fp32 samples [T] -> fp32 log-mel [n_filt, get_seq_len(T)]."""
        x = torch.as_tensor(wave).detach().to("cpu", torch.float32).reshape(1, -1).clone()
        n = self.get_seq_len(x.shape[1])
        if self.dither > 0:
            x = x + self.dither * torch.randn(x.shape, generator=generator, dtype=torch.float32)
        if self.preemph is not None:
            x = torch.cat((x[:, 0].unsqueeze(1), x[:, 1:] - self.preemph * x[:, :-1]), dim=1)
        spec = torch.view_as_real(torch.stft(x, n_fft=self.n_fft, hop_length=self.hop_length, win_length=self.win_length,
                                             window=self.window, return_complex=True))
        power = spec.pow(2).sum(-1)
        mel = torch.log(torch.matmul(self.fb, power) + 1e-20)
        return mel[0, :, :n].contiguous()

    def __call__(self, waves, generator=None):
        """a list of fp32 waveforms -> (list of fp32 log-mel [n_filt, len_b], list of lengths)."""
        feats = [self.log_mel(w, generator) for w in waves]
        return feats, [int(f.shape[1]) for f in feats]
