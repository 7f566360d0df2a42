"""fp64 restatement of the reference's Griffin-Lim mel inversion (audio/stft.py:15-157, audio/audio_processing.py:7-82,
audio/tools.py:18-34), in numpy.  The bars of tests/golden/griffin_lim.npz are 4 x the max-abs distance between the
reference's float32 results and this evaluation of the same formulas (tests/golden/make_golden_griffin_lim.py), so
tests/test_griffin_lim_cpu.py pins this file to the reference and the GPU tests can measure against either.

Shapes follow the reference: magnitude / phase (B, cutoff, F), signals (B, hop * (F - 1)), log-mel (n_mel, T).

Below the reference's functions stand the contracts of the kernels of csrc/fs2_griffin_lim.hip one by one (recombine, project,
mag_phase, ola), as that file's comments state them, on frame-major rows.  Everything takes `dtype`: np.float64 (the default) is
the oracle; np.float32 evaluates the same formula with every operation rounded to float32 - each product, sum, quotient and square
root as numpy rounds it, each cos / sin / arctan2 as the float32 nearest the function of its float32 argument - which is how the
reference computes, and whose distance from the fp64 evaluation the bars of tests/golden/gl_kernel_bars.json are taken from."""
import numpy as np

TINY32 = np.finfo(np.float32).tiny


def _fn(f, dtype):
    """cos / sin / arctan2 rounded once to dtype (evaluated in fp64 on the dtype-valued arguments)"""
    return lambda *a: f(*(np.asarray(x, dtype=np.float64) for x in a)).astype(dtype)


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


def bases32(filter_length, hop_length, win_length):
    """the same in float32 with the reference's casts (stft.py:38-46): float32(basis) * float32(window)"""
    fb = fourier_basis(filter_length)
    w = window(win_length, filter_length).astype(np.float32)
    inv = np.linalg.pinv(filter_length / hop_length * fb).T
    return fb.astype(np.float32) * w, inv.astype(np.float32) * w


def window_sumsquare(n_frames, hop_length, win_length, n_fft, dtype=np.float64):
    """dtype float32: the reference's float32 array += float64 window^2, each add done in double and rounded"""
    n = n_fft + hop_length * (n_frames - 1)
    x = np.zeros(n, dtype=dtype)
    w2 = window(win_length, n_fft) ** 2
    for i in range(n_frames):
        x[i * hop_length:i * hop_length + n_fft] += w2
    return x


class STFT:
    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, dtype=np.float64):
        self.filter_length, self.hop_length, self.win_length, self.dtype = filter_length, hop_length, win_length, dtype
        self.cutoff = filter_length // 2 + 1
        self.forward_basis, self.inverse_basis = (bases if dtype == np.float64 else bases32)(filter_length, hop_length, win_length)

    def transform(self, x):
        if self.dtype != np.float64:
            return self._transform32(x)
        x = np.asarray(x, dtype=np.float64)
        P, hop = self.filter_length // 2, self.hop_length
        xp = np.pad(x, ((0, 0), (P, P)), mode="reflect")
        F = 1 + x.shape[1] // hop
        frames = np.stack([xp[:, f * hop:f * hop + self.filter_length] for f in range(F)], axis=1)     # (B, F, filter)
        ft = frames @ self.forward_basis.T                                                            # (B, F, 2*cutoff)
        re, im = ft[..., :self.cutoff], ft[..., self.cutoff:]
        return np.sqrt(re ** 2 + im ** 2).transpose(0, 2, 1), np.arctan2(im, re).transpose(0, 2, 1)

    def frames_of(self, x):
        """the reflect-padded signal cut into (B, F, filter) frames"""
        x = np.asarray(x, dtype=self.dtype)
        P, hop = self.filter_length // 2, self.hop_length
        xp = np.pad(x, ((0, 0), (P, P)), mode="reflect")
        return np.stack([xp[:, f * hop:f * hop + self.filter_length] for f in range(1 + x.shape[1] // hop)], axis=1)

    def _transform32(self, x):
        return mag_phase(self.frames_of(x) @ self.forward_basis.T, dtype=self.dtype)

    def inverse(self, mag, phase):
        if self.dtype != np.float64:
            m, p = (np.asarray(a, dtype=self.dtype).transpose(0, 2, 1) for a in (mag, phase))
            seg = recombine(m, p, dtype=self.dtype) @ self.inverse_basis
            F = seg.shape[1]
            w2 = window(self.win_length, self.filter_length) ** 2
            return ola(seg, None, w2, self.filter_length, self.hop_length, 0, self.hop_length * (F - 1), dtype=self.dtype)[1]
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


# ---------------------------------------------------------------------------------------------- the kernels' own contracts
def _frames(frames, B, Fmax):
    return [Fmax] * B if frames is None else [min(max(int(f), 0), Fmax) for f in frames]


def recombine(mag, phase, frames=None, ldg=None, dtype=np.float64):
    """fs2_gl_recombine: mag, phase (B, Fmax, NF) frame-major -> G (B, Fmax, ldg), rows [m cos(phi) | m sin(phi) | 0 ...]; rows
    f >= frames[b] are zero whatever mag and phase hold there (frames=None: all rows)."""
    mag, phase = np.asarray(mag, dtype=dtype), np.asarray(phase, dtype=dtype)
    B, Fmax, NF = mag.shape
    ldg = 2 * NF if ldg is None else ldg
    G = np.zeros((B, Fmax, ldg), dtype=dtype)
    for b, F in enumerate(_frames(frames, B, Fmax)):
        G[b, :F, :NF] = mag[b, :F] * _fn(np.cos, dtype)(phase[b, :F])
        G[b, :F, NF:2 * NF] = mag[b, :F] * _fn(np.sin, dtype)(phase[b, :F])
    return G


def project(ft, mag, frames=None, ldg=None, dtype=np.float64):
    """fs2_gl_project: ft (B, S >= Fmax, >= 2 NF) forward-DFT rows [Re | Im | ...], mag (B, Fmax, NF) the target magnitude ->
    recombine(mag, arctan2(Im, Re)), arctan2(0, 0) = 0; rows f >= frames[b] of ft are not read."""
    ft, mag = np.asarray(ft, dtype=dtype), np.asarray(mag, dtype=dtype)
    B, Fmax, NF = mag.shape
    phase = np.zeros((B, Fmax, NF), dtype=dtype)
    for b, F in enumerate(_frames(frames, B, Fmax)):
        phase[b, :F] = _fn(np.arctan2, dtype)(ft[b, :F, NF:2 * NF], ft[b, :F, :NF])
    return recombine(mag, phase, frames, ldg, dtype)


def mag_phase(ft, dtype=np.float64):
    """fs2_gl_mag_phase: ft (B, F, 2 NF) rows [Re | Im] -> (sqrt(Re^2 + Im^2), arctan2(Im, Re)), each channel-major (B, NF, F)"""
    ft = np.asarray(ft, dtype=dtype)
    NF = ft.shape[-1] // 2
    re, im = ft[..., :NF], ft[..., NF:]
    return np.sqrt(re * re + im * im).transpose(0, 2, 1), _fn(np.arctan2, dtype)(im, re).transpose(0, 2, 1)


def ola(seg, frames, win_sq, filt, hop, row_len, ldy, dtype=np.float64):
    """fs2_gl_ola: seg (B, Fmax, >= filt) per-frame segments -> (xp (B, row_len), y (B, ldy)).  Row b: the F_b = frames[b]
    (clamped to [0, Fmax]) segments overlap-added in increasing f, divided by the squared-window envelope where it exceeds
    TINY32, times filt / hop, trimmed by filt / 2 at both ends: N_b = hop (F_b - 1) samples, y zero beyond them.  xp is that
    signal reflect-padded by filt / 2 at its own ends, zero beyond N_b + filt, and all zero when N_b <= filt / 2.  The envelope
    in float32 is window_sumsquare's: a float32 array to which the float64 win_sq is added frame by frame."""
    seg, win_sq = np.asarray(seg, dtype=dtype), np.asarray(win_sq, dtype=np.float64)
    B, Fmax = seg.shape[:2]
    P, scale = filt // 2, dtype(filt / hop)
    xp, y = np.zeros((B, row_len), dtype=dtype), np.zeros((B, ldy), dtype=dtype)
    for b, F in enumerate(_frames(frames, B, Fmax)):
        N = hop * (F - 1)
        if N <= 0:
            continue
        acc, env = np.zeros(filt + N, dtype=dtype), np.zeros(filt + N, dtype=dtype)
        for f in range(F):
            acc[f * hop:f * hop + filt] += seg[b, f, :filt]
            env[f * hop:f * hop + filt] += win_sq
        nz = env > TINY32
        acc[nz] /= env[nz]
        acc *= scale
        sig = acc[P:P + N]
        y[b, :N] = sig
        if N > P and row_len:
            xp[b, :N + 2 * P] = np.pad(sig, (P, P), mode="reflect")
    return xp, y
