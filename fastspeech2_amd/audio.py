"""Mel extraction (reference audio/stft.py:130-178 TacotronSTFT, audio/tools.py:8-15 get_mel_from_wav) on the GPU.

`TacotronSTFT(filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin, mel_fmax)
 .mel_spectrogram(y (B, N) in [-1, 1]) -> (mel (B, n_mel, frames), energy (B, frames))`, frames = 1 + N // hop.

The reference computes the STFT as a strided conv1d with a windowed DFT basis (stft.py:66-72).  Here the
reflect-padded signal is viewed as rows of `hop` samples, which turns the framed DFT into a (filter/hop)-tap
implicit GEMM  ft[B*rows][2*cutoff] = sum_j X[m + j][:] . basis[:, j*hop:(j+1)*hop]^T  on the exact-fp32 MFMA
(`v_mfma_f32_32x32x2_f32`, same products and fp32 accumulation as the reference's dot products), followed by one
fused pass: magnitude -> mel filterbank (non-zero band of each filter only) -> log(clamp) and the per-frame
energy norm.

The mel filterbank is `librosa.filters.mel` (Slaney scale + area normalisation, librosa==0.7.2, the reference's
requirements.txt:3).  librosa is not available here; the formula is restated in `slaney_mel_filterbank` from its
published definition ("parity unpinned" at this one boundary — DESIGN.md §6).  A caller holding librosa can pass
`mel_basis=` explicitly.

The other half, spectrogram -> audio (audio/stft.py:15-122 STFT, audio/audio_processing.py:7-82, audio/tools.py:18-34): `STFT`,
`griffin_lim`, `inv_mel_spec` and the batched, ragged `mels_to_wavs_griffin_lim`.  Both contractions of a Griffin-Lim iteration
run on the same exact-fp32 MFMA GEMM (the framed DFT above; the inverse as a one-tap GEMM of frames x inverse_basis into
per-frame segments); the phase projection and the overlap-add with the window_sumsquare division are
csrc/fs2_griffin_lim.hip.  One iteration = 4 launches on the current stream, buffers sized once per call.

Sample-rate conversion and peak normalisation of ragged batches (`resample_poly`, `peak_abs`, `peaknorm_pcm`) live in
fastspeech2_amd/resample.py and are re-exported here.
"""
import functools

import numpy as np
import torch

from . import _lib, ops, ragged
from .resample import peak_abs, peaknorm_pcm, resample_poly  # noqa: F401


def slaney_mel_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """Slaney-style mel filterbank (htk=False, norm=1): linear below 1 kHz, log above, triangles normalised to unit area."""
    if fmax is None:
        fmax = sr / 2.0
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0

    def to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)

    def to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)

    n_freq = 1 + n_fft // 2
    fft_f = np.linspace(0, sr / 2.0, n_freq)
    mel_f = to_hz(np.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    # rounding order of the float32 table librosa returns: triangles -> float32, x float64 area norm -> float32
    w = np.maximum(0, np.minimum(lower, upper)).astype(np.float32)
    w = (w.astype(np.float64) * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]).astype(np.float32)
    return w


def _fourier_basis(filter_length):
    fb = np.fft.fft(np.eye(filter_length))
    cutoff = filter_length // 2 + 1
    return np.vstack([np.real(fb[:cutoff]), np.imag(fb[:cutoff])])       # (2*cutoff, filter_length) float64


def _window(window, win_length, filter_length):
    """scipy.signal.get_window(window, win_length, fftbins=True) centre-padded to filter_length (librosa.util.pad_center), float64."""
    from scipy.signal import get_window

    win = get_window(window, win_length, fftbins=True)
    if win_length < filter_length:
        lpad = (filter_length - win_length) // 2
        win = np.pad(win, (lpad, filter_length - win_length - lpad))
    return win


def dft_basis(filter_length, win_length, window="hann"):
    """audio/stft.py:26-50: rows [Re(0..cutoff) ; Im(0..cutoff)] of the DFT matrix times a periodic window
    (scipy.signal.get_window(window, win_length, fftbins=True), centre-padded to filter_length), float32."""
    fb = _fourier_basis(filter_length)
    return torch.FloatTensor(fb) * torch.from_numpy(_window(window, win_length, filter_length)).float()   # (2*cutoff, filter_length)


@functools.lru_cache(maxsize=8)
def _pinv_fourier(filter_length, hop_length):
    """np.linalg.pinv(scale * fourier_basis).T in float64 (stft.py:34-36), scale = filter / hop: (2*cutoff, filter_length)."""
    return np.linalg.pinv(filter_length / hop_length * _fourier_basis(filter_length)).T


def inverse_basis(filter_length, hop_length, win_length, window="hann"):
    """stft.py:34-46: float32(pinv(scale * fourier_basis).T) * float32 window -> (2*cutoff, filter_length) float32."""
    return torch.FloatTensor(_pinv_fourier(filter_length, hop_length)) * torch.from_numpy(_window(window, win_length, filter_length)).float()


def window_sumsquare(window, n_frames, hop_length, win_length, n_fft):
    """audio/audio_processing.py:7-56 (norm=None, dtype float32): the squared-window envelope of n_frames frames, frames
    added in increasing order into a float32 array.  The kernels rebuild it per sample (fs2_gl_ola); this host form is the
    statement they are checked against."""
    n = n_fft + hop_length * (n_frames - 1)
    x = np.zeros(n, dtype=np.float32)
    win_sq = _window(window, win_length, n_fft) ** 2
    for i in range(n_frames):
        sample = i * hop_length
        x[sample:min(n, sample + n_fft)] += win_sq[:max(0, min(n_fft, n - sample))]
    return x


def _row_len(filter_length):
    return (2 * (filter_length // 2 + 1) + 3) // 4 * 4            # 2*cutoff padded to the f32 GEMM's multiple of 4 (16-B rows)


def _framed_dft(forward_basis, y, B, N, lens, filter_length, hop):
    """reflect pad (stft.py:60-66) + the strided DFT as a (filter/hop)-tap implicit GEMM over rows of `hop` samples:
    -> (ft [B*S][2*cutoff] view of 16-B aligned rows, S); frame t of utterance b is row b*S + t."""
    taps, P = filter_length // hop, filter_length // 2
    S = N // hop + 1 + taps - 1                                         # rows of `hop` samples per utterance
    xp = torch.empty(B, S * hop, device=y.device, dtype=torch.float32)
    if lens is None:
        _lib.call("fs2_reflect_pad", y.data_ptr(), xp.data_ptr(), B, N, P, S * hop, ops._stream())
    else:
        _lib.call("fs2_reflect_pad_ragged", y.data_ptr(), N, lens.data_ptr(), xp.data_ptr(), B, P, S * hop, ops._stream())
    nft = forward_basis.shape[0]
    ft = torch.empty(B * S, _row_len(filter_length), device=y.device, dtype=torch.float32)[:, :nft]
    ops.conv_gemm(xp.view(B * S, hop), forward_basis, None, S, taps=taps, pad=0, out=ft)
    return ft, S


class STFT(torch.nn.Module):
    """audio/stft.py:15-127 on the GPU: `transform(x (B, N))` -> (magnitude, phase), each (B, cutoff, 1 + N // hop);
    `inverse(magnitude, phase)` -> (B, 1, hop * (F - 1)); `forward(x)` = inverse(*transform(x)).  fp32 throughout: the framed
    DFT and the inverse's per-frame segments are exact-fp32 MFMA contractions (fs2_conv_gemm), the overlap-add, the
    window_sumsquare division and the trim are fs2_gl_ola (csrc/fs2_griffin_lim.hip)."""

    def __init__(self, filter_length, hop_length, win_length, window="hann"):
        super().__init__()
        if window is None:
            raise ValueError("STFT: only the windowed form (window is not None) is implemented")
        assert filter_length % hop_length == 0, "framed-DFT GEMM needs hop | filter_length (every reference config)"
        assert filter_length >= win_length and filter_length % 2 == 0
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        self.cutoff = filter_length // 2 + 1
        taps = filter_length // hop_length
        basis = dft_basis(filter_length, win_length, window)
        self.register_buffer("forward_basis", basis.view(2 * self.cutoff, taps, hop_length).contiguous())
        inv = inverse_basis(filter_length, hop_length, win_length, window)                 # (2*cutoff, filter_length)
        # packed for the one-tap GEMM seg[f][n] = sum_c G[f][c] W[n][c]: W = inverse_basis^T, K padded with zero columns
        w = torch.zeros(filter_length, 1, _row_len(filter_length), dtype=torch.float32)
        w[:, 0, :2 * self.cutoff] = inv.t()
        self.register_buffer("inverse_weight", w)
        self.register_buffer("win_sq", torch.from_numpy(_window(window, win_length, filter_length) ** 2))   # float64

    def _to(self, dev):
        if self.forward_basis.device != dev:
            self.to(dev)

    def transform(self, input_data):
        """stft.py:52-81 -> (magnitude, phase), each (B, cutoff, 1 + N // hop); needs N > filter_length / 2 (reflect pad)."""
        ragged.require_device(input_data, "fastspeech2_amd.audio.STFT")
        self._to(input_data.device)
        x = input_data.contiguous().float()
        B, N = x.shape
        if N <= self.filter_length // 2:
            raise ValueError(f"STFT.transform: {N} samples; reflect padding needs more than filter_length/2 = {self.filter_length // 2}")
        ft, S = _framed_dft(self.forward_basis, x, B, N, None, self.filter_length, self.hop_length)
        F = N // self.hop_length + 1
        mag = torch.empty(B, self.cutoff, F, device=x.device, dtype=torch.float32)
        phase = torch.empty_like(mag)
        _lib.call("fs2_gl_mag_phase", ft.data_ptr(), ft.stride(0), S, mag.data_ptr(), phase.data_ptr(), B, F, self.cutoff, ops._stream())
        return mag, phase

    def inverse(self, magnitude, phase):
        """stft.py:83-122: (B, cutoff, F) magnitude and phase -> (B, 1, hop * (F - 1))."""
        ragged.require_device(magnitude, "fastspeech2_amd.audio.STFT")
        self._to(magnitude.device)
        magnitude = magnitude.float()
        phase = torch.as_tensor(phase, dtype=torch.float32, device=magnitude.device)
        B, NF, F = magnitude.shape
        if NF != self.cutoff or phase.shape != magnitude.shape or F < 2:
            raise ValueError(f"STFT.inverse: magnitude {tuple(magnitude.shape)} / phase {tuple(phase.shape)}: need (B, {self.cutoff}, F >= 2)")
        ws = self.workspace(B, F, magnitude.device)
        _lib.call("fs2_gl_recombine", magnitude.data_ptr(), magnitude.stride(0), magnitude.stride(2), magnitude.stride(1),
                  phase.data_ptr(), phase.stride(0), phase.stride(2), phase.stride(1), None, ws["G"].data_ptr(), ws["G"].stride(0),
                  B, F, self.cutoff, ops._stream())
        self._inverse_rows(ws, None, B, F, y=True)
        return ws["y"].view(B, 1, -1)

    def forward(self, input_data):
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)

    # ---------------------------------------------------------------------------------------------- Griffin-Lim on the device
    def workspace(self, B, Fmax, device):
        """Every buffer of a Griffin-Lim call over B utterances of up to Fmax frames, sized once (no allocation in the loop):
        G (B*Fmax, ld) inverse-GEMM input rows, seg (B*Fmax, filter) its per-frame segments, xp (B, S*hop) the reflect-padded
        signal rows, ft (B*S, ld) the forward DFT, y (B, hop*(Fmax-1)) the signal; S = Fmax + filter/hop - 1.  Contents on
        entry do not matter: every entry a kernel reads is written first, padding included."""
        ld, hop, S = _row_len(self.filter_length), self.hop_length, Fmax + self.filter_length // self.hop_length - 1
        e = functools.partial(torch.empty, device=device, dtype=torch.float32)
        return {"G": e(B * Fmax, ld), "seg": e(B * Fmax, self.filter_length), "xp": e(B, S * hop), "ft": e(B * S, ld),
                "y": e(B, hop * (Fmax - 1))}

    def _inverse_rows(self, ws, frames, B, Fmax, xp=False, y=False):
        """inverse GEMM G -> seg, then overlap-add -> ws['xp'] (next forward DFT's rows) and / or ws['y']."""
        G, seg = ws["G"], ws["seg"]
        ops.conv_gemm(G, self.inverse_weight, None, Fmax, taps=1, pad=0, out=seg)
        _lib.call("fs2_gl_ola", seg.data_ptr(), seg.stride(0), ops._p(frames), self.win_sq.data_ptr(),
                  ws["xp"].data_ptr() if xp else None, ws["xp"].stride(0), ws["y"].data_ptr() if y else None, ws["y"].stride(0),
                  B, Fmax, self.filter_length, self.hop_length, ops._stream())

    def griffin_lim_rows(self, mag, mag_strides, frames, angles, angle_strides, n_iters, ws=None):
        """The device loop.  mag / angles: (b, f, k) elements at strides mag_strides = (sb, sf, sk, Fmax) / angle_strides = (sb, sf, sk);
        frames (B,) int32 on the device: utterance b's frame count (each >= 4, checked by the callers).  Returns ws['y']
        (B, hop*(Fmax-1)); row b's first hop*(frames[b]-1) samples are its signal.  Per iteration: forward GEMM, project,
        inverse GEMM, overlap-add - four launches on the current stream, no synchronisation."""
        B, Fmax = frames.numel(), mag_strides[3]
        if ws is None:
            ws = self.workspace(B, Fmax, mag.device)
        msb, msf, msk = mag_strides[:3]
        G, xp, ft = ws["G"], ws["xp"], ws["ft"]
        taps = self.filter_length // self.hop_length
        S = Fmax + taps - 1
        _lib.call("fs2_gl_recombine", mag.data_ptr(), msb, msf, msk, angles.data_ptr(), *angle_strides, frames.data_ptr(),
                  G.data_ptr(), G.stride(0), B, Fmax, self.cutoff, ops._stream())
        self._inverse_rows(ws, frames, B, Fmax, xp=n_iters > 0, y=n_iters == 0)
        ftv = ft[:, :2 * self.cutoff]
        for i in range(n_iters):
            ops.conv_gemm(xp.view(B * S, self.hop_length), self.forward_basis, None, S, taps=taps, pad=0, out=ftv)
            _lib.call("fs2_gl_project", ft.data_ptr(), ft.stride(0), S, mag.data_ptr(), msb, msf, msk, frames.data_ptr(),
                      G.data_ptr(), G.stride(0), B, Fmax, self.cutoff, ops._stream())
            last = i == n_iters - 1
            self._inverse_rows(ws, frames, B, Fmax, xp=not last, y=last)
        return ws["y"]


def _draw_angles(shape):
    """audio_processing.py:71-72: phases drawn from numpy's global generator, as float32."""
    return np.angle(np.exp(2j * np.pi * np.random.rand(*shape))).astype(np.float32)


def _check_frames(frames, hop, filter_length):
    bad = [f for f in frames if hop * (f - 1) <= filter_length // 2]
    if bad:
        raise ValueError(f"Griffin-Lim needs hop*(F-1) > filter_length/2 (reflect padding): F = {bad} frame(s) too short "
                         f"(at least {filter_length // (2 * hop) + 2} frames, i.e. {filter_length // (2 * hop) + 3} mel frames)")


def griffin_lim(magnitudes, stft_fn, n_iters=30, angles=None):
    """audio/audio_processing.py:59-82: magnitudes (B, cutoff, F) -> signal (B, hop*(F-1)).  angles=None draws the initial
    phases from numpy's global generator exactly as the reference does (same shape, same call), so a seeded numpy gives the
    reference's start; otherwise angles (B, cutoff, F)."""
    if not isinstance(stft_fn, STFT):
        raise TypeError("griffin_lim: stft_fn must be a fastspeech2_amd.audio.STFT")
    B, NF, F = magnitudes.shape
    if NF != stft_fn.cutoff:
        raise ValueError(f"griffin_lim: magnitudes {tuple(magnitudes.shape)}: need (B, {stft_fn.cutoff}, F)")
    _check_frames([F], stft_fn.hop_length, stft_fn.filter_length)
    ragged.require_device(magnitudes, "fastspeech2_amd.audio.griffin_lim")
    stft_fn._to(magnitudes.device)
    mag = magnitudes.float()
    if angles is None:
        angles = _draw_angles(mag.size())
    ang = torch.as_tensor(angles, dtype=torch.float32).to(mag.device)
    assert ang.shape == mag.shape
    frames = torch.full((B,), F, dtype=torch.int32, device=mag.device)
    return stft_fn.griffin_lim_rows(mag, (mag.stride(0), mag.stride(2), mag.stride(1), F), frames, ang,
                                    (ang.stride(0), ang.stride(2), ang.stride(1)), int(n_iters)).clone()


def mels_to_wavs_griffin_lim(mels, mel_lens, _stft, n_iters=60, angles=None, ws=None):
    """Batched, ragged `inv_mel_spec`: mels (B, n_mel, T) log-mel (any strides), utterance b = its first mel_lens[b] frames ->
    list of B float32 arrays of hop*(mel_lens[b] - 2) samples.  The initial phases are drawn per utterance, in batch order,
    each as inv_mel_spec draws them (angles=None), so the batch equals successive inv_mel_spec calls on the same numpy
    generator; every utterance's result is bit-identical to the utterance processed alone.  angles (optional): list of B
    (cutoff, mel_lens[b] - 1) arrays.  ws (optional): a workspace(B, max(mel_lens) - 1, device) to run in."""
    stft = _stft.stft_fn
    B, n_mel, T = mels.shape
    if n_mel != _stft.n_mel_channels:
        raise ValueError(f"mels_to_wavs_griffin_lim: mels {tuple(mels.shape)}: need (B, {_stft.n_mel_channels}, T)")
    lens, lens_d = ragged.lengths(mel_lens, B, T, "mel_lens", mels.device)
    frames = [n - 1 for n in lens]
    _check_frames(frames, stft.hop_length, stft.filter_length)
    ragged.require_device(mels, "fastspeech2_amd.audio.mels_to_wavs_griffin_lim")
    _stft._to(mels.device)
    mels = mels.float()
    dev, NF, Fmax = mels.device, stft.cutoff, max(frames)
    if angles is None:
        angles = [_draw_angles((1, NF, f))[0] for f in frames]
    host = np.zeros((B, NF, Fmax), dtype=np.float32)
    for b, (a, f) in enumerate(zip(angles, frames)):
        host[b, :, :f] = np.asarray(a, dtype=np.float32).reshape(NF, f)
    ang = torch.from_numpy(host).to(dev)
    frames_d = lens_d - 1
    mag = torch.empty(B, Fmax, NF, device=dev, dtype=torch.float32)                    # frame-major target magnitude
    _lib.call("fs2_gl_mel_to_mag", mels.data_ptr(), mels.stride(0), mels.stride(1), mels.stride(2), lens_d.data_ptr(),
              _stft.mel_basis.data_ptr(), _stft.mel_span.data_ptr(), mag.data_ptr(), mag.stride(1), B, Fmax, n_mel, NF, ops._stream())
    y = stft.griffin_lim_rows(mag, (mag.stride(0), mag.stride(1), mag.stride(2), Fmax), frames_d, ang,
                              (ang.stride(0), ang.stride(2), ang.stride(1)), int(n_iters), ws=ws)
    y = y.cpu().numpy()
    return [y[b, :stft.hop_length * (f - 1)].copy() for b, f in enumerate(frames)]


def inv_mel_spec(mel, out_filename, _stft, griffin_iters=60):
    """audio/tools.py:18-34: log-mel (n_mel, T) -> Griffin-Lim (griffin_iters iterations, phases from numpy's global
    generator) over T - 1 frames -> float32 samples written unconverted by scipy.io.wavfile at the configured rate."""
    from scipy.io.wavfile import write

    mel = torch.as_tensor(mel)
    if mel.dim() != 2:
        raise ValueError(f"inv_mel_spec: mel {tuple(mel.shape)}: need (n_mel, T)")
    _check_frames([mel.shape[1] - 1], _stft.stft_fn.hop_length, _stft.stft_fn.filter_length)
    if not mel.is_cuda:
        mel = mel.to(_stft.mel_basis.device if _stft.mel_basis.is_cuda else torch.device("cuda"))
    audio = mels_to_wavs_griffin_lim(mel.unsqueeze(0), [mel.shape[1]], _stft, griffin_iters)[0]
    write(out_filename, _stft.sampling_rate, audio)
    return audio


class TacotronSTFT(torch.nn.Module):
    def __init__(self, filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin, mel_fmax,
                 mel_basis=None):
        super().__init__()
        assert filter_length % hop_length == 0, "framed-DFT GEMM needs hop | filter_length (every reference config)"
        assert filter_length >= win_length
        self.filter_length, self.hop_length, self.win_length = filter_length, hop_length, win_length
        self.n_mel_channels, self.sampling_rate = n_mel_channels, sampling_rate
        self.cutoff = filter_length // 2 + 1
        basis = dft_basis(filter_length, win_length)
        taps = filter_length // hop_length
        # packed for the implicit GEMM: W[n][tap][c] = basis[n][tap*hop + c]
        self.register_buffer("forward_basis", basis.view(2 * self.cutoff, taps, hop_length).contiguous())
        if mel_basis is None:
            mel_basis = slaney_mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)
        mel_basis = torch.as_tensor(np.asarray(mel_basis), dtype=torch.float32)
        self.register_buffer("mel_basis", mel_basis.contiguous())
        nz = mel_basis != 0
        span = torch.zeros(n_mel_channels, 2, dtype=torch.int32)
        for k in range(n_mel_channels):
            idx = torch.nonzero(nz[k]).flatten()
            if idx.numel():
                span[k, 0], span[k, 1] = int(idx[0]), int(idx[-1]) + 1
        self.register_buffer("mel_span", span)
        # stft.py:144: the STFT object; the reference's inv_mel_spec reads it as `_stft_fn` (tools.py:28), hence the alias
        self.stft_fn = STFT(filter_length, hop_length, win_length)

    @property
    def _stft_fn(self):
        return self.stft_fn

    def _to(self, dev):
        if self.forward_basis.device != dev:
            self.to(dev)

    def spectral_de_normalize(self, magnitudes):
        """stft.py:155-157 (audio_processing.py:94-100, C = 1): exp(x)."""
        ragged.require_device(magnitudes, "fastspeech2_amd.audio.TacotronSTFT")
        return torch.exp(magnitudes)

    def mel_spectrogram(self, y):
        """audio/stft.py:159-178."""
        assert torch.min(y.data) >= -1 and torch.max(y.data) <= 1          # stft.py:170-171
        ragged.require_device(y, "fastspeech2_amd.audio.TacotronSTFT")
        self._to(y.device)
        y = y.contiguous().float()
        B, N = y.shape
        return self._framed_mel(y, B, N, None)

    def mel_spectrogram_ragged(self, y, lens):
        """Corpus form of `mel_spectrogram` (preprocessor/preprocessor.py:194 calls it once per utterance): y (B, Nmax) holds
        B utterances of `lens[b]` samples each (anything beyond is ignored).  Every row is reflected at its OWN end, so
        frames [0, lens[b] // hop + 1) of row b are bit-identical to the utterance processed alone; later frames are padding.
        Returns (mel (B, n_mel, Nmax // hop + 1), energy (B, Nmax // hop + 1), frames (B,) int64)."""
        ragged.require_device(y, "fastspeech2_amd.audio.TacotronSTFT")
        self._to(y.device)
        y = y.contiguous().float()
        B, N = y.shape
        lens_h, lens = ragged.lengths(lens, B, N, "lens", y.device)
        assert lens_h and min(lens_h) > self.filter_length // 2, "each utterance needs more than filter_length/2 samples (reflect padding)"
        mel, energy = self._framed_mel(y, B, N, lens)
        return mel, energy, lens.to(torch.int64) // self.hop_length + 1

    def _framed_mel(self, y, B, N, lens):
        frames = N // self.hop_length + 1
        ft, S = _framed_dft(self.forward_basis, y, B, N, lens, self.filter_length, self.hop_length)
        mel = torch.empty(B, self.n_mel_channels, frames, device=y.device, dtype=torch.float32)
        energy = torch.empty(B, frames, device=y.device, dtype=torch.float32)
        _lib.call("fs2_stft_mel_epilogue", ft.data_ptr(), ft.stride(0), self.mel_basis.data_ptr(), self.mel_span.data_ptr(),
                  mel.data_ptr(), energy.data_ptr(), B, S, frames, self.cutoff, self.n_mel_channels, 1e-5, ops._stream())
        return mel, energy


def get_mel_from_wav(audio, _stft):
    """audio/tools.py:8-15: 1-D float array in [-1, 1] -> (mel (n_mel, frames), energy (frames,)) as float32 numpy."""
    dev = _stft.forward_basis.device if _stft.forward_basis.is_cuda else torch.device("cuda")
    a = torch.clip(torch.as_tensor(np.asarray(audio), dtype=torch.float32).unsqueeze(0), -1, 1).to(dev)
    mel, energy = _stft.mel_spectrogram(a)
    return mel[0].cpu().numpy().astype(np.float32), energy[0].cpu().numpy().astype(np.float32)
