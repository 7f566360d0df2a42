"""Mel-cepstra of an F0-adaptive spectral envelope on the GPU: CheapTrick (Morise 2015) followed by the SPTK frequency transformation
`freqt`, the quantity published mel-cepstral-distortion tables are computed from.  HIP kernels in fp64 over ragged batches
(csrc/fs2_world.hip).  Written from the published descriptions of CheapTrick and of WORLD (Morise, Yokomori, Ozawa 2016) and of the
mel-cepstrum (Tokuda et al. 1994).  The specification below is what the kernels and the numpy oracle (tests/world_ref.py) implement;
the oracle is held against analytic answers (tests/test_world_cpu.py).  Agreement with the pyworld / pysptk binaries is UNMEASURED:
neither package is available where this was built.

Inputs.  x[0, n) the samples of one utterance (float32, taken to double), fs its rate, f0[f] one F0 value per frame (0 = unvoiced;
DIO + StoneMask of `pitch`), frame f centred at t_f = f * frame_period / 1000 s.  matlab_round(v) = int(v + 0.5) for v > 0.

Envelope (CheapTrick), per frame, N / 2 + 1 bins of width df = fs / N
  0. Size.  N = 2^ceil(log2(3 fs / f0_floor + 1)), f0_floor = 71 Hz: 1024 at 16 / 22.05 / 24 kHz, 2048 at 44.1 / 48 kHz.  A rate that
     needs N > 2048 is a ValueError before any launch.
  1. F0.  g = f0[f] when 3 fs / (N - 3) < f0[f] <= fs / 8, else the default 500 Hz (unvoiced frames, values too low for the window to
     fit N, NaN, and values so high that the smoothing widths below would leave the spectrum).
  2. Window.  h = matlab_round(1.5 fs / g); o = matlab_round(t_f fs + 0.001); for i in [0, 2h]: sample s_i = x[clamp(o + i - h, 0,
     n - 1)], Hann w_i = 0.5 cos(pi g (i - h) / (1.5 fs)) + 0.5, normalised w_i <- w_i / sqrt(sum w^2); y_i = s_i w_i;
     y_i <- y_i - w_i (sum y / sum w) (the window-weighted mean removed).  The random 1e-12 "safety offset" WORLD adds to y is NOT
     taken over.
  3. Power.  P[k] = |sum_i y_i exp(-2 pi i k i / N)|^2, k in [0, N / 2].
  4. DC correction.  With u_k = g N / fs - k: for every k <= int(g N / fs), P'[k] = P[k] + lerp(P, u_k), lerp(P, u) =
     P[int(u)] + (P[int(u) + 1] - P[int(u)]) (u - int(u)) (the power at g - k df, read from the uncorrected P); other bins unchanged.
  5. Linear smoothing of width wd = 2 g / 3.  b = int(wd N / fs) + 1; the mirrored spectrum M[j], j in [0, N / 2 + 2 b], is
     P'[|j - b|] below N / 2 + b and P'[N - (j - b)] above, taken as piecewise constant: M[j] on the df around (j - b) df.
     E[k] = (1 / wd) the integral of that function over [k df - wd / 2, k df + wd / 2] = sum_j M[j] * (the length bin j shares with
     the interval) / wd, j ascending.  This is the number WORLD forms as (S(k df + wd / 2) - S(k df - wd / 2)) / wd from the running
     integral S[j] = sum_{m <= j} M[m] df, linearly interpolated; the two are equal in exact arithmetic, but the difference of two
     running integrals carries an error of eps S / (wd E), measured at 3e-8 relative where the spectrum spans 70 dB, so the short
     sum is what is specified and computed.
  6. Floor.  E[k] <- E[k] + 2.2e-16.  This one deterministic floor stands in place of both random "infinitesimal noise" terms of the
     WORLD program; it is applied here, after the linear smoothing and before the logarithm, and nowhere else, so `log` never sees
     zero (E >= 0 before it: a sum of non-negative terms) and two runs are byte-identical.
  7. Smoothing with recovery.  v = ln E extended evenly to N points; cepstrum C[q] = (1 / N) sum_k v[k] cos(2 pi k q / N), q in
     [0, N / 2]; C'[q] = C[q] ls[q] lc[q] with ls[q] = sin(pi g q / fs) / (pi g q / fs) (1 at q = 0) and lc[q] = (1 - 2 q1) +
     2 q1 cos(2 pi g q / fs), q1 = -0.15; envelope[k] = exp(sum over the even extension of C' of C'[q] cos(2 pi k q / N)).  The
     envelope is a POWER spectrum.

Mel-cepstrum, per frame
  L[k] = 0.5 ln envelope[k] (log amplitude); r = its real cepstrum, r[q] = (1 / N) sum over the even extension of L[k] cos(2 pi k q
  / N); one-sided c_0 = r_0, c_q = 2 r_q (0 < q < N / 2), c_{N/2} = r_{N/2}, so that L(w) = sum_q c_q cos(q w).  `freqt` with
  all-pass constant a maps c_0 .. c_{N/2} to c~_0 .. c~_K with L(w) = sum_m c~_m cos(m w~), w~ = w + 2 atan(a sin w / (1 - a cos w)):
  state g = 0; for i = N / 2 down to 0: d <- g; g_0 = c_i + a d_0; g_1 = (1 - a^2) d_0 + a d_1; g_j = d_{j-1} + a (d_j - g_{j-1}),
  j = 2 .. K; c~ = the final g.  Equivalently c~_0 = (1 / pi) int_0^pi L cos(0) dw~ and c~_m = (2 / pi) int_0^pi L cos(m w~) dw~.
  K = n_mcep defaults to 24 and is at most 40.  c~_0 (the level) is computed and dropped: the output is c~_1 .. c~_K, the rows
  `metrics.local_cost` reads.  a comes from `ALPHA` by sampling rate (0.410 at 16 kHz, 0.455 at 22.05 kHz, 0.466 at 24 kHz, 0.544 at
  44.1 kHz, 0.554 at 48 kHz) unless given; a rate outside the table without `alpha` (`--alpha`) is a ValueError.  a = 0 returns c.

Transforms are radix-2 FFTs in LDS with a twiddle table built on the host in numpy float64 (`twiddle_table`) and uploaded once: the
device evaluates no sine for them.  `freqt` is linear in c, so the host applies the recursion above once to the unit vectors
(`freqt_table`, numpy float64, per N, K and a) and the device forms c~_m = sum_q table[m][q] c_q, q ascending per lane.  No atomics,
sums in a fixed order: a frame does not depend on the rest of its batch or on the run.
"""
import math

import numpy as np
import torch

from . import _lib, ops, ragged
from .pitch import frame_count

WHO = "fastspeech2_amd.envelope"
F0_FLOOR, DEFAULT_F0, Q1, FLOOR = 71.0, 500.0, -0.15, 2.2e-16
MAX_FFT, MAX_MCEP, DEFAULT_MCEP = 2048, 40, 24
ALPHA = {16000: 0.410, 22050: 0.455, 24000: 0.466, 44100: 0.544, 48000: 0.554}


def fft_size(fs):
    """CheapTrick's transform length for `fs`; ValueError above MAX_FFT."""
    if not fs > 0:
        raise ValueError(f"sampling rate {fs} is not positive")
    n = 1 << int(math.ceil(math.log2(3.0 * fs / F0_FLOOR + 1.0)))
    if n > MAX_FFT:
        raise ValueError(f"a sampling rate of {fs} Hz needs a {n}-point envelope transform, more than the supported {MAX_FFT}")
    return max(n, 256)


def alpha_for(fs, alpha=None):
    """The all-pass constant: `alpha` when given (|alpha| < 1), else the table's value for `fs`."""
    if alpha is None:
        if int(fs) != fs or int(fs) not in ALPHA:
            raise ValueError(f"no all-pass constant is tabulated for {fs} Hz ({sorted(ALPHA)}): pass alpha= (score.py: --alpha)")
        return ALPHA[int(fs)]
    if not -1.0 < float(alpha) < 1.0:
        raise ValueError(f"alpha must lie in (-1, 1), got {alpha}")
    return float(alpha)


def check_mcep(n_mcep):
    if not 1 <= int(n_mcep) <= MAX_MCEP:
        raise ValueError(f"n_mcep must be in [1, {MAX_MCEP}], got {n_mcep}")
    return int(n_mcep)


def twiddle_table(n):
    """(n / 2, 2) float64: cos(2 pi k / n), -sin(2 pi k / n)."""
    k = np.arange(n // 2, dtype=np.float64)
    return np.stack([np.cos(2.0 * np.pi * k / n), -np.sin(2.0 * np.pi * k / n)], axis=1)


def freqt_table(n, n_mcep, alpha):
    """(n_mcep, n / 2 + 1) float64: row m - 1 holds the weights of c_0 .. c_{n/2} in c~_m, the `freqt` recursion of the module
    docstring applied to the unit vectors (column q carries the input that is 1 at q)."""
    M, a = n // 2, float(alpha)
    g = np.zeros((n_mcep + 1, M + 1))
    for i in range(M, -1, -1):
        d = g.copy()
        g[0] = a * d[0]
        g[0, i] += 1.0
        g[1] = (1.0 - a * a) * d[0] + a * d[1]
        for j in range(2, n_mcep + 1):
            g[j] = d[j - 1] + a * (d[j] - g[j - 1])
    return np.ascontiguousarray(g[1:])


_tables = {}


def _freqt(dev, n, n_mcep, alpha):
    key = (str(dev), n, n_mcep, float(alpha))
    if key not in _tables:
        _tables[key] = torch.from_numpy(freqt_table(n, n_mcep, alpha)).to(dev)
    return _tables[key]


def _twiddles(dev, n):
    key = (str(dev), n)
    if key not in _tables:
        _tables[key] = torch.from_numpy(twiddle_table(n)).to(dev)
    return _tables[key]


def _dev(t, dtype, what, dim):
    ragged.require_device(t, WHO)
    if t.dtype != dtype or t.dim() != dim or (t.numel() and t.stride(-1) != 1):
        raise ValueError(f"{what} must be a {dim}-D {dtype} tensor with unit inner stride, got {t.dtype} {tuple(t.shape)}")
    return t


def _out(out, shape, what, device):
    """A caller's float64 output buffer (any batch / row strides, at least `shape`) or a fresh one."""
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    out = _dev(out, torch.float64, what, len(shape))
    if out.device != device or out.shape[0] != shape[0] or any(o < s for o, s in zip(out.shape[1:], shape[1:])):
        raise ValueError(f"{what} {tuple(out.shape)} is too small for {tuple(shape)}")
    return out


def _args(y, lens, f0, frames, fs, frame_period):
    """Everything checked before a launch: -> (y, lens on the device, f0, frames on the host and the device, Fmax, N)."""
    n = fft_size(fs)
    if not frame_period > 0:
        raise ValueError(f"frame_period {frame_period} is not positive")
    if not isinstance(y, torch.Tensor) or not isinstance(f0, torch.Tensor) or not y.is_cuda or not f0.is_cuda:
        raise ValueError(f"{WHO} runs on an AMD GPU only (no CPU fallback): y and f0 must be tensors on the device")
    y = _dev(y, torch.float32, "y", 2)
    f0 = _dev(f0, torch.float64, "f0", 2)
    B = y.shape[0]
    if f0.device != y.device or f0.shape[0] != B:
        raise ValueError(f"f0 {tuple(f0.shape)} must hold one row per row of y {tuple(y.shape)} on the same device")
    lens_h, lens_d = ragged.lengths(lens, B, y.shape[1], "lens", y.device)
    frames_h, frames_d = ragged.lengths(frames, B, f0.shape[1], "frames", y.device)
    for b, (nb, fb) in enumerate(zip(lens_h, frames_h)):
        if fb > (frame_count(nb, fs, frame_period) if nb else 0):
            raise ValueError(f"row {b}: {fb} frames, but {nb} samples at a frame period of {frame_period} ms hold at most "
                             f"{frame_count(nb, fs, frame_period) if nb else 0}")
    return y, lens_d, f0, frames_h, frames_d, max(frames_h, default=0), n


def envelope(y, lens, f0, frames, fs, frame_period, out=None):
    """CheapTrick over a ragged batch: y (B, >= max lens) float32, f0 (B, >= Fmax) float64, both on the GPU; row b has lens[b]
    samples and frames[b] frames.  -> the power envelope (B, Fmax, N / 2 + 1) float64; rows beyond frames[b] are left alone."""
    y, lens_d, f0, _, frames_d, Fmax, n = _args(y, lens, f0, frames, fs, frame_period)
    B = y.shape[0]
    env = _out(out, (B, Fmax, n // 2 + 1), "out", y.device)
    tw, st = _twiddles(y.device, n), ops._stream()
    _lib.call("fs2_env_spectrum", y.data_ptr(), y.stride(0), lens_d.data_ptr(), f0.data_ptr(), f0.stride(0), frames_d.data_ptr(),
              float(fs), float(frame_period), tw.data_ptr(), n, env.data_ptr(), env.stride(0), env.stride(1), B, Fmax, y.shape[1], st)
    _lib.call("fs2_env_smooth", f0.data_ptr(), f0.stride(0), frames_d.data_ptr(), float(fs), tw.data_ptr(), n, Q1, FLOOR,
              env.data_ptr(), env.stride(0), env.stride(1), B, Fmax, st)
    return env


def mel_cepstra(env, frames, fft_size, alpha, n_mcep=DEFAULT_MCEP, out=None):
    """Power envelope (B, >= Fmax, fft_size / 2 + 1) float64 on the GPU -> c~_1 .. c~_K (B, Fmax, n_mcep) float64."""
    K = check_mcep(n_mcep)
    alpha = alpha_for(0, alpha)
    if fft_size not in (256, 512, 1024, 2048):
        raise ValueError(f"fft_size must be 256, 512, 1024 or 2048, got {fft_size}")
    env = _dev(env, torch.float64, "env", 3)
    B = env.shape[0]
    if env.shape[2] != fft_size // 2 + 1:
        raise ValueError(f"env {tuple(env.shape)} does not hold {fft_size // 2 + 1} bins per frame")
    frames_h, frames_d = ragged.lengths(frames, B, env.shape[1], "frames", env.device)
    Fmax = max(frames_h, default=0)
    c = _out(out, (B, Fmax, K), "out", env.device)
    _lib.call("fs2_env_mcep", env.data_ptr(), env.stride(0), env.stride(1), frames_d.data_ptr(), _twiddles(env.device, fft_size).data_ptr(),
              fft_size, _freqt(env.device, fft_size, K, alpha).data_ptr(), K, c.data_ptr(), c.stride(0), c.stride(1), B, Fmax,
              ops._stream())
    return c


def world_cepstra(y, lens, f0, frames, fs, frame_period, n_mcep=DEFAULT_MCEP, alpha=None, out=None):
    """Envelope, then mel-cepstra: -> (B, Fmax, n_mcep) float64 in the row layout `metrics.local_cost` reads."""
    check_mcep(n_mcep)
    alpha = alpha_for(fs, alpha)
    _args(y, lens, f0, frames, fs, frame_period)
    return mel_cepstra(envelope(y, lens, f0, frames, fs, frame_period), frames, fft_size(fs), alpha, n_mcep, out)
