"""Sample-rate conversion and peak normalisation on the GPU (csrc/fs2_resample.hip): what the reference's `prepare_align` does per
file with `librosa.load(path, sampling_rate)` followed by `wav / max(abs(wav)) * max_wav_value` and `astype(int16)`
(preprocessor/ljspeech.py:28-34), over ragged batches.

librosa 0.7.2's `kaiser_best` filter cannot be pinned here (neither librosa nor resampy is in this image).  The project's stand-in
is `scipy.signal.resample_poly` with its default window (`preprocess.load_wav`); the kernels implement that same filter, evaluated in
fp64.  The specification below is what the kernels and the numpy oracle (tests/resample_ref.py) implement.

Resampler.  g = gcd(sr_out, sr_in), up = sr_out / g, down = sr_in / g, m = max(up, down), half = 10 m.

    h[k]   = up * firwin(2 half + 1, cutoff = 1 / m, window = ("kaiser", 5.0))[k]      k in [0, 2 half]      (fp64, host)
    n_out  = ceil(n_in * up / down)
    y[j]   = sum over i in [0, n_in) with 0 <= j down - i up + half <= 2 half  of  x[i] * h[j down - i up + half]

Samples outside [0, n_in) are zero (scipy's edge rule).  This direct sum equals `resample_poly(x.astype(float64), sr_out, sr_in)` to
rounding (tests/test_resample_cpu.py).  `resample_poly` on a float32 input casts the taps to float32 and differs from the fp64 result
by about 6e-7 on unit-variance noise; the GPU path is specified against the fp64 evaluation, not against that.

Evaluation.  Output j touches one phase of the filter: p = (j down + half) mod up, q = (j down + half) div up, taps h[p + t up]
against x[q - t].  `phase_table` lays them out phase-major and in ascending input index, tab[p][s] = h[p + (T - 1 - s) up] (0 where
that index exceeds 2 half), T = ceil((2 half + 1) / up) rounded up to even, so y[j] = sum_{s < T} tab[p][s] * x[q - T + 1 + s].  The
kernel accumulates that in fp64 (fma, ascending s) and rounds once to float32; padded taps and out-of-range samples contribute
exact zeros.  The table goes to the device once per (up, down, device).  Any (up, down) works (a tile of input samples is staged in
LDS where it fits 64 KiB, which covers every pair of the usual rates 8 - 48 kHz; otherwise the same sum reads global memory).
sr_in == sr_out is the identity filter (tab = [0, 1]) when a window or the clamped copy is asked for, and returns its input otherwise.

Peak normalisation.  peak = max |y| (float32), pcm = int16(y / peak * max_wav_value): float32 division, float32 product, then numpy's
`astype(int16)` of a float32 (truncate toward zero to int32, keep the low 16 bits).  With max_wav_value = 32768 a POSITIVE peak sample
becomes 32768 -> -32768: the reference has that quirk (preprocessor/ljspeech.py:29-33) and it is kept.  The one deviation: a row whose
peak is 0 yields zeros (the reference divides by zero there); `prepare_align` warns when it happens.
"""
from math import gcd

import numpy as np
import torch

from . import _lib, ops, ragged

MAX_FACTOR = 1 << 16                # keeps the tap table (about 21 max(up, down) doubles) small and the kernel's 32-bit phase arithmetic exact


def ratio(sr_in, sr_out):
    """(up, down) of the conversion sr_in -> sr_out in lowest terms."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in <= 0 or sr_out <= 0:
        raise ValueError(f"sampling rates must be positive, got {sr_in} -> {sr_out}")
    g = gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    if max(up, down) > MAX_FACTOR:
        raise ValueError(f"{sr_in} -> {sr_out} Hz needs up / down = {up} / {down}: factors above {MAX_FACTOR} are not supported")
    return up, down


def filter_taps(up, down):
    """(h fp64 [2 half + 1], half): scipy.signal.resample_poly's default filter, scaled by `up`."""
    from scipy.signal import firwin
    m = max(up, down)
    half = 10 * m
    if m == 1:
        return np.ones(1), 0                                                # same rate: the identity
    return up * firwin(2 * half + 1, 1.0 / m, window=("kaiser", 5.0)), half


def phase_table(h, up):
    """h [2 half + 1] -> tab [up][T] fp64, tab[p][s] = h[p + (T - 1 - s) up] (0 beyond the last tap), T even."""
    n = len(h)
    T = -(-n // up)
    T += T % 2
    pad = np.zeros(up * T, dtype=np.float64)
    pad[:n] = h
    return np.ascontiguousarray(pad.reshape(T, up).T[:, ::-1])


def out_length(n_in, up, down):
    return -(-int(n_in) * up // down)


_tables = {}


def _device_table(dev, up, down):
    key = (str(dev), up, down)
    if key not in _tables:
        h, half = filter_taps(up, down)
        tab = phase_table(h, up)
        _tables[key] = (torch.from_numpy(tab).to(dev), half, tab.shape[1])
    return _tables[key]


def resample_poly(x, lens, sr_in, sr_out, out_begin=None, out_len=None, clip=False, in_begin=None):
    """Polyphase resampling of a ragged batch: x (B, N) float32 on the GPU, row b holds lens[b] samples at rate sr_in.
    Returns (y, out_lens) or, with clip=True, (y, y clamped to [-1, 1], out_lens): y (B, max(out_lens)) float32 on the device,
    out_lens (B,) int64 on the host; y[b, out_lens[b]:] is unspecified.

    Windows.  `out_begin` / `out_len` (per row, in output samples) select outputs [out_begin[b], out_begin[b] + out_len[b]) of the
    row's full result (default: all ceil(lens[b] * up / down) of them).  `in_begin` says that row b holds the samples
    [in_begin[b], in_begin[b] + lens[b]) of its utterance and everything else counts as zero: hand over only the span a window
    needs (`input_span`); `out_begin` and `out_len` are then required.  sr_in == sr_out without a window or clip returns (x, lens)."""
    x, lens_h, _ = ragged.rows(x, lens, "fastspeech2_amd.resample.resample_poly", device_lens=False)
    B, N = x.shape
    up, down = ratio(sr_in, sr_out)
    if in_begin is not None and (out_begin is None or out_len is None):
        raise ValueError("in_begin needs out_begin and out_len: the utterance's full length is not known from a slice")
    if up == down and out_begin is None and out_len is None and not clip and in_begin is None:
        return x, torch.tensor(lens_h, dtype=torch.int64)
    cap = (1 << 31) - 1                                                       # the kernel's row arithmetic is 32-bit
    ob = ragged.lengths(out_begin if out_begin is not None else [0] * B, B, cap, "out_begin")
    ib = ragged.lengths(in_begin if in_begin is not None else [0] * B, B, cap, "in_begin")
    ol = ragged.lengths(out_len if out_len is not None else [max(out_length(n, up, down) - o, 0) for n, o in zip(lens_h, ob)],
                        B, cap, "out_len")
    dev = x.device
    tab, half, T = _device_table(dev, up, down)
    Nout = max(ol) if ol else 0
    y = torch.empty(B, Nout, dtype=torch.float32, device=dev)
    yc = torch.empty_like(y) if clip else None
    if B and Nout:
        meta = torch.tensor([ib, lens_h, ob, ol], dtype=torch.int32, device=dev)       # one H2D copy; alive until the launch is queued
        ib_d, il_d, ob_d, ol_d = (meta[k].data_ptr() for k in range(4))
        _lib.call("fs2_resample_poly", x.data_ptr(), N, ib_d if in_begin is not None else None, il_d, tab.data_ptr(), up, down,
                  half, T, ob_d if out_begin is not None else None, ol_d, y.data_ptr(), yc.data_ptr() if clip else None, Nout,
                  B, N, Nout, ops._stream())
    out_lens = torch.tensor(ol, dtype=torch.int64)
    return (y, yc, out_lens) if clip else (y, out_lens)


def input_span(out_begin, out_len, n_in, up, down):
    """[lo, hi): the input samples that outputs [out_begin, out_begin + out_len) of an n_in-sample utterance depend on."""
    if out_len <= 0:
        return 0, 0
    half = 10 * max(up, down) if max(up, down) > 1 else 0
    lo = max(0, -((half - out_begin * down) // up))                           # ceil((out_begin down - half) / up)
    hi = min(n_in, ((out_begin + out_len - 1) * down + half) // up + 1)
    return (lo, hi) if hi > lo else (0, 0)


def peak_abs(y, lens):
    """peak[b] = max |y[b, :lens[b]]| as a (B,) float32 device tensor (0 for an empty row)."""
    y, _, lens_d = ragged.rows(y, lens, "fastspeech2_amd.resample.peak_abs")
    peak = torch.empty(y.shape[0], dtype=torch.float32, device=y.device)
    _lib.call("fs2_peak_abs", y.data_ptr(), y.shape[1], lens_d.data_ptr(), peak.data_ptr(), y.shape[0], y.shape[1], ops._stream())
    return peak


def peaknorm_pcm(y, lens, peak, max_wav_value):
    """int16(y / peak * max_wav_value) per row (see the module docstring for the cast and the peak == 0 rule): (B, N) int16 on the
    device, zero beyond lens[b]."""
    y, _, lens_d = ragged.rows(y, lens, "fastspeech2_amd.resample.peaknorm_pcm")
    if not isinstance(peak, torch.Tensor) or peak.device != y.device or peak.dtype != torch.float32 or peak.numel() != y.shape[0]:
        raise ValueError("peak must be a (B,) float32 tensor on y's device")
    pcm = torch.empty(y.shape, dtype=torch.int16, device=y.device)
    peak = peak.contiguous()
    _lib.call("fs2_peaknorm_pcm", y.data_ptr(), y.shape[1], lens_d.data_ptr(), peak.data_ptr(), float(max_wav_value), pcm.data_ptr(),
              y.shape[1], y.shape[0], y.shape[1], ops._stream())
    return pcm
