"""float64 numpy restatement of fastspeech2_amd/envelope.py's docstring (CheapTrick envelope, mel-cepstrum by `freqt`), one utterance
at a time, written from the specification and not from the kernels: `np.fft.rfft` / `irfft`, `np.interp`, matrix products (and `np.cumsum` for the running-integral form of the smoothing).  Only
constants come from the product module.  `MatrixFft` is the same pair of transforms as O(N^2) products with an explicit DFT matrix:
a second summation order of the same fp64 quantities, from which the GPU tests' bars are measured (tests/golden/make_world_bars.py)."""
import math

import numpy as np

from fastspeech2_amd.envelope import ALPHA, DEFAULT_F0, F0_FLOOR, FLOOR, Q1            # constants only

MCD_SCALE = 10.0 / math.log(10.0) * math.sqrt(2.0)


class MatrixFft:
    """rfft / irfft of length n as matrix products (angles reduced exactly: k i mod n)"""

    def __init__(self):
        self._w = {}

    def _matrix(self, n):
        if n not in self._w:
            k = np.arange(n // 2 + 1)[:, None]
            i = np.arange(n)[None, :]
            self._w[n] = np.exp(-2j * np.pi * ((k * i) % n) / n)
        return self._w[n]

    def rfft(self, x, n):
        v = np.zeros(n)
        v[:len(x)] = x
        return self._matrix(n) @ v

    def irfft(self, X, n):
        """real x with rfft(x) = X (X[0], X[n / 2] real)"""
        W = self._matrix(n)
        wgt = np.full(n // 2 + 1, 2.0)
        wgt[0] = wgt[-1] = 1.0
        return ((wgt * X) @ W.conj()).real / n


def fft_size(fs):
    return 2 ** int(math.ceil(math.log2(3.0 * fs / F0_FLOOR + 1.0)))


def matlab_round(v):
    return int(v + 0.5) if v > 0 else int(v - 0.5)


def frame_f0(f0, fs, n):
    return f0 if (f0 > 3.0 * fs / (n - 3.0) and f0 <= fs / 8.0) else DEFAULT_F0


def windowed(x, fs, g, t):
    h = matlab_round(1.5 * fs / g)
    o = matlab_round(t * fs + 0.001)
    base = np.arange(-h, h + 1)
    s = np.asarray(x, np.float64)[np.clip(o + base, 0, len(x) - 1)]
    w = 0.5 * np.cos(np.pi * g * base / (1.5 * fs)) + 0.5
    w = w / np.sqrt(np.sum(w * w))
    y = s * w
    return y - w * (np.sum(y) / np.sum(w))


def dc_correction(P, g, fs, n):
    top = int(g * n / fs)
    k = np.arange(top + 1)
    out = P.copy()
    out[k] = P[k] + np.interp(g * n / fs - k, np.arange(len(P)), P)
    return out


def linear_smoothing(P, wd, fs, n):
    """every output bin as one row of a (bins, mirrored bins) matrix of shared lengths in Hz, times the mirrored spectrum"""
    df = fs / n
    b = int(wd * n / fs) + 1
    j = np.arange(n // 2 + 2 * b + 1) - b
    M = P[np.where(j <= n // 2, np.abs(j), n - j)]
    f = np.arange(n // 2 + 1)[:, None] * df
    share = np.minimum(f + wd / 2, (j[None, :] + 0.5) * df) - np.maximum(f - wd / 2, (j[None, :] - 0.5) * df)
    return (np.maximum(share, 0.0) @ M) / wd


def linear_smoothing_by_running_integral(P, wd, fs, n):
    """the same quantity as the difference of two interpolated running integrals, the form the WORLD program uses: equal in exact
    arithmetic, but it loses eps S / E to cancellation (tests/test_world_cpu.py measures the two against each other)"""
    df = fs / n
    b = int(wd * n / fs) + 1
    j = np.arange(n // 2 + 2 * b + 1) - b
    M = P[np.where(j <= n // 2, np.abs(j), n - j)]
    S = np.cumsum(M * df)
    axis = (j + 0.5) * df
    f = np.arange(n // 2 + 1) * df
    return (np.interp(f + wd / 2, axis, S) - np.interp(f - wd / 2, axis, S)) / wd


def smoothing_with_recovery(E, g, fs, n, fft):
    q = np.arange(n // 2 + 1) / fs
    ls = np.ones(n // 2 + 1)
    ls[1:] = np.sin(np.pi * g * q[1:]) / (np.pi * g * q[1:])
    lc = (1.0 - 2.0 * Q1) + 2.0 * Q1 * np.cos(2.0 * np.pi * g * q)
    C = fft.irfft(np.log(E).astype(complex), n)[:n // 2 + 1] * ls * lc
    return np.exp(fft.rfft(np.concatenate([C, C[-2:0:-1]]), n).real)


def envelope(x, f0, fs, frame_period, fft=None):
    """x (n,) samples, f0 (F,) -> the power envelope (F, N / 2 + 1)"""
    fft = fft or NumpyFft()
    n = fft_size(fs)
    out = np.empty((len(f0), n // 2 + 1))
    for f, v in enumerate(f0):
        g = frame_f0(float(v), fs, n)
        P = np.abs(fft.rfft(windowed(x, fs, g, f * frame_period / 1000.0), n)) ** 2
        E = linear_smoothing(dc_correction(P, g, fs, n), 2.0 * g / 3.0, fs, n) + FLOOR
        out[f] = smoothing_with_recovery(E, g, fs, n, fft)
    return out


class NumpyFft:
    def rfft(self, x, n):
        return np.fft.rfft(x, n)

    def irfft(self, X, n):
        return np.fft.irfft(X, n)


def plain_cepstrum(env, fft=None):
    """power envelope (F, N / 2 + 1) -> the one-sided cepstrum c_0 .. c_{N/2} of 0.5 ln envelope, (F, N / 2 + 1)"""
    fft = fft or NumpyFft()
    n = 2 * (env.shape[1] - 1)
    c = np.stack([fft.irfft((0.5 * np.log(row)).astype(complex), n)[:n // 2 + 1] for row in env])
    c[:, 1:-1] *= 2.0
    return c


def freqt(c, K, a):
    """c (F, M + 1) -> c~ (F, K + 1): the SPTK recursion, rows side by side"""
    c = np.atleast_2d(np.asarray(c, np.float64))
    g = np.zeros((c.shape[0], K + 1))
    for i in range(c.shape[1] - 1, -1, -1):
        d = g.copy()
        g[:, 0] = c[:, i] + a * d[:, 0]
        if K >= 1:
            g[:, 1] = (1.0 - a * a) * d[:, 0] + a * d[:, 1]
        for j in range(2, K + 1):
            g[:, j] = d[:, j - 1] + a * (d[:, j] - g[:, j - 1])
    return g


def mel_cepstra(env, K=24, alpha=None, fs=None, fft=None):
    """-> c~_1 .. c~_K, (F, K)"""
    a = ALPHA[int(fs)] if alpha is None else alpha
    return freqt(plain_cepstrum(env, fft), K, a)[:, 1:]


def world_cepstra(x, f0, fs, frame_period, K=24, alpha=None, fft=None):
    return mel_cepstra(envelope(x, f0, fs, frame_period, fft), K, alpha, fs, fft)


def warped(w, a):
    """the all-pass frequency map w -> w~"""
    return w + 2.0 * np.arctan(a * np.sin(w) / (1.0 - a * np.cos(w)))
