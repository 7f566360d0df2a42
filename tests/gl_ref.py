"""fp64 restatement of the reference's Griffin-Lim mel inversion (audio/stft.py:15-157, audio/audio_processing.py:7-82,
audio/tools.py:18-34), in numpy.  The bars of tests/golden/griffin_lim.npz are 4 x the max-abs distance between the
reference's float32 results and this evaluation of the same formulas (tests/golden/make_golden_griffin_lim.py), so
tests/test_griffin_lim_cpu.py pins this file to the reference and the GPU tests can measure against either.

Shapes follow the reference: magnitude / phase (B, cutoff, F), signals (B, hop * (F - 1)), log-mel (n_mel, T)."""
import numpy as np

TINY32 = np.finfo(np.float32).tiny


def window(win_length, filter_length):
    """periodic hann (scipy.signal.get_window('hann', win_length, fftbins=True)) centre-padded to filter_length"""
    n = np.arange(win_length)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
    lpad = (filter_length - win_length) // 2
    return np.pad(w, (lpad, filter_length - win_length - lpad))


def fourier_basis(filter_length):
    fb = np.fft.fft(np.eye(filter_length))
    cutoff = filter_length // 2 + 1
    return np.vstack([np.real(fb[:cutoff]), np.imag(fb[:cutoff])])


def bases(filter_length, hop_length, win_length):
    """(forward (2*cutoff, filter), inverse (2*cutoff, filter)) in fp64: stft.py:26-46 without the float32 casts."""
    fb = fourier_basis(filter_length)
    w = window(win_length, filter_length)
    inv = np.linalg.pinv(filter_length / hop_length * fb).T
    return fb * w, inv * w


def window_sumsquare(n_frames, hop_length, win_length, n_fft):
    n = n_fft + hop_length * (n_frames - 1)
    x = np.zeros(n)
    w2 = window(win_length, n_fft) ** 2
    for i in range(n_frames):
        x[i * hop_length:i * hop_length + n_fft] += w2
    return x


class STFT:
    def __init__(self, filter_length=1024, hop_length=256, win_length=1024):
        self.filter_length, self.hop_length, self.win_length = filter_length, hop_length, win_length
        self.cutoff = filter_length // 2 + 1
        self.forward_basis, self.inverse_basis = bases(filter_length, hop_length, win_length)

    def transform(self, x):
        x = np.asarray(x, dtype=np.float64)
        P, hop = self.filter_length // 2, self.hop_length
        xp = np.pad(x, ((0, 0), (P, P)), mode="reflect")
        F = 1 + x.shape[1] // hop
        frames = np.stack([xp[:, f * hop:f * hop + self.filter_length] for f in range(F)], axis=1)     # (B, F, filter)
        ft = frames @ self.forward_basis.T                                                            # (B, F, 2*cutoff)
        re, im = ft[..., :self.cutoff], ft[..., self.cutoff:]
        return np.sqrt(re ** 2 + im ** 2).transpose(0, 2, 1), np.arctan2(im, re).transpose(0, 2, 1)

    def inverse(self, mag, phase):
        mag, phase = np.asarray(mag, dtype=np.float64), np.asarray(phase, dtype=np.float64)
        B, _, F = mag.shape
        hop, n = self.hop_length, self.filter_length
        g = np.concatenate([mag * np.cos(phase), mag * np.sin(phase)], axis=1).transpose(0, 2, 1)    # (B, F, 2*cutoff)
        seg = g @ self.inverse_basis                                                                  # (B, F, filter)
        y = np.zeros((B, n + hop * (F - 1)))
        for f in range(F):
            y[:, f * hop:f * hop + n] += seg[:, f]
        env = window_sumsquare(F, hop, self.win_length, n)
        nz = env > TINY32
        y[:, nz] /= env[nz]
        y *= n / hop
        return y[:, n // 2:y.shape[1] - n // 2]


def griffin_lim(mag, stft, n_iters, angles):
    """audio_processing.py:59-82 from given initial angles -> (B, hop * (F - 1))"""
    signal = stft.inverse(mag, angles)
    for _ in range(n_iters):
        _, angles = stft.transform(signal)
        signal = stft.inverse(mag, angles)
    return signal


def spec_from_mel(mel, mel_basis):
    """tools.py:19-26: exp(mel)^T mel_basis * 1000, transposed -> (cutoff, T)"""
    return (np.exp(np.asarray(mel, dtype=np.float64)).T @ np.asarray(mel_basis, dtype=np.float64)).T * 1000.0


def spectral_convergence(signal, mag, stft):
    """|| |STFT(x)| - M ||_F / || M ||_F"""
    m, _ = stft.transform(signal)
    mag = np.asarray(mag, dtype=np.float64)
    return float(np.linalg.norm(m - mag) / np.linalg.norm(mag))


def phase_distance(a, b):
    """|a - b| modulo 2 pi, in [0, pi]"""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)
