"""References of the Whisper log-mel front end (include/ext/x2i_logmel.h; a helper of the logmel tests, it holds no tests).

ref64: the definition in float64 -- the waveform's float32 samples extended by zeros to N_max, reflect-padded by 200, frames of 400 every
160 (the extractor's extra last frame left out), the periodic Hann window, numpy's float64 FFT, the float32 filter bank's values, log10
with the floor 1e-10, the maximum over ALL frames, the clamp and (x + 4) / 4.
restate32: the same formulas in float32 with torch CPU matmuls (the window folded into float32 cos / sin tables): what float32 arithmetic
in another summation order gives, the yardstick of the kernel's error.
"""
import functools

import numpy as np
import torch

N_FFT, HOP, BINS, PAD = 400, 160, 201, 200


def kept_frames(n, N_max):
    """L: ceil(n / 160), at most N_max / 160 -- the ones of the extractor's attention mask"""
    return min(-(-n // HOP), N_max // HOP)


def seen_frames(n, N_max):
    """A: the frames whose 400 samples reach below n (frame t starts at 160 t - 200)"""
    return min(N_max // HOP, (n + 199) // HOP + 1)


@functools.lru_cache(maxsize=None)
def mel_filters(n_mels):
    """float32 [201, n_mels]: WhisperFeatureExtractor's own filter bank, rounded as its torch path rounds it"""
    from transformers import WhisperFeatureExtractor
    return np.asarray(WhisperFeatureExtractor(feature_size=n_mels).mel_filters).astype(np.float32)


def frames64(x, N_max):
    """float64 [T, 400]: the frames of the definition, before the window"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    assert x.ndim == 1 and x.shape[0] <= N_max and N_max % HOP == 0
    sig = np.zeros(N_max, dtype=np.float64)
    sig[:x.shape[0]] = x
    sig = np.pad(sig, PAD, mode="reflect")
    T = N_max // HOP
    return np.lib.stride_tricks.sliding_window_view(sig, N_FFT)[::HOP][:T]


def window64():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT)


def power64(x, N_max):
    """float64 [T, 201]: |X_t[k]|^2"""
    X = np.fft.rfft(frames64(x, N_max) * window64()[None, :], axis=1)
    return X.real ** 2 + X.imag ** 2


def finish64(lg, max_frames=None):
    """lg [n_mels, T] -> (max(lg, mx - 8) + 4) / 4 with mx over the first max_frames frames (default: all of them)"""
    mx = lg.max() if max_frames is None else lg[:, :max_frames].max()
    return (np.maximum(lg, mx - 8.0) + 4.0) / 4.0


def ref64(x, N_max, filters, power=None):
    """-> (lg, out): float64 [n_mels, T] each, every frame computed, the maximum over all of them"""
    p = power64(x, N_max) if power is None else power
    lg = np.log10(np.maximum(p @ np.asarray(filters, dtype=np.float64), 1e-10)).T
    return lg, finish64(lg)


@functools.lru_cache(maxsize=None)
def tables32():
    """float32 [400, 201] x 2: w[j] cos(2 pi j k / 400) and -w[j] sin(2 pi j k / 400), made in float64 with the angle reduced in integers"""
    j, k = np.arange(N_FFT, dtype=np.int64)[:, None], np.arange(BINS, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((j * k) % N_FFT).astype(np.float64) / N_FFT
    w = window64()[:, None]
    return torch.from_numpy(w * np.cos(ang)).float(), torch.from_numpy(-w * np.sin(ang)).float()


def restate32(x, N_max, filters):
    """float32 [n_mels, T]: the formulas of ref64 in float32 arithmetic"""
    fr = torch.from_numpy(np.ascontiguousarray(frames64(x, N_max))).float()
    cos, sin = tables32()
    re, im = fr @ cos, fr @ sin
    mel = (re * re + im * im) @ torch.from_numpy(np.asarray(filters, dtype=np.float32))
    lg = torch.clamp(mel, min=1e-10).log10().T
    return ((torch.maximum(lg, lg.max() - 8.0) + 4.0) / 4.0).numpy()


def _rand(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def dropped_frame_case(background=1e-6):
    """n = 960: a weak background and a burst in the last 24 samples.  L = 6 frames are kept and frame 6, which is dropped, holds the
    maximum: it sees the burst under the window's peak, frame 5 under its tail"""
    x = background * _rand(960, 11)
    x[-24:] += 0.9 * _rand(24, 12)
    return x.astype(np.float32)


def six_signals():
    """name -> float32 waveform: the signals the float64 reference is checked on against WhisperFeatureExtractor"""
    t = np.arange(112077, dtype=np.float64) / 16000.0
    chirp = 0.5 * (1.0 + 0.8 * np.sin(2 * np.pi * 3.0 * t)) * np.sin(2 * np.pi * (200.0 * t + 0.5 * 1000.0 * t * t))
    burst = 1e-5 * _rand(160000, 4)
    burst[:4000] += 0.9 * _rand(4000, 5)
    tt = np.arange(320000, dtype=np.float64) / 16000.0
    sig = {
        "noise": 0.1 * _rand(480000, 1),
        "tone": 0.5 * np.sin(2 * np.pi * 440.0 * tt) + 1e-4 * _rand(320000, 2),
        "clip": 0.3 * _rand(1000, 3),
        "burst": burst,
        "chirp": chirp,
        "zeros": np.zeros(5000),
    }
    return {k: v.astype(np.float32) for k, v in sig.items()}


def edge_batch(N_max):
    """The batch of the GPU tests: n = 1, 159, 160, 161, 960 (the dropped-frame case), 1000, N_max - 1 and N_max (a burst in the last 24
    samples, so the right-hand reflection matters), and an all-zero sample"""
    out = [np.array([0.7]), 0.3 * _rand(159, 21), 0.3 * _rand(160, 22), 0.3 * _rand(161, 23), dropped_frame_case(1e-3), 0.3 * _rand(1000, 24)]
    for n, seed in ((N_max - 1, 25), (N_max, 26)):
        x = 1e-3 * _rand(n, seed)
        x[-24:] += 0.9 * _rand(24, seed + 10)
        out.append(x)
    out.append(np.zeros(min(5000, N_max - 400)))
    return [np.asarray(x, dtype=np.float32) for x in out]


def ulp_bf16(v):
    """The spacing of bfloat16 at |v| (8 significant bits), elementwise; the smallest normal's where v is 0"""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)
