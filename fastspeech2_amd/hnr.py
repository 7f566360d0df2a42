"""Harmonics-to-noise ratio on the GPU (csrc/fs2_hnr.hip): how much of a voiced frame's power repeats at the pitch period, the
published measure of a hoarse, buzzy or noisy voice (Boersma 1993: the maximum of the autocorrelation of a windowed frame, divided by
the autocorrelation of the window, is the share r of periodic power; HNR = 10 log10(r / (1 - r)) dB).  Used here to compare the
voiced speech of a synthesized utterance with the recording's, per side and along the cepstral DTW path.  It has a closed-form
known answer: a periodic signal plus white noise at S dB SNR has an HNR of S dB.  The specification below is what the kernels and
the independent numpy restatement (tests/hnr_ref.py: explicit loops, np.correlate for the lag sums) implement.

Arithmetic.  The audio is float32; everything after its load is fp64.  Every sum carries the rounding error of each addition
(two-sum) and of each product (one fma) in a second word, per lane in ascending order and then by a fixed tree or in a fixed ascending
order: the sum of the exact terms rounded once, in all but cases too rare to meet.  No atomics; padding is never read or written;
two runs give the same bytes, and a row's bytes do not depend on its batch.  Rows have 1 <= T <= MAX_FRAMES = 2048 frames (the bound
of `metrics`); anything else is a ValueError before any launch.

Constants.  F0_FLOOR = 71 Hz and F0_CEIL = 800 Hz are `pitch`'s.  PERIODS = 4.5 periods of F0_FLOOR per window is Praat's
harmonicity default as remembered: written from memory, not checked against Praat.  SEARCH = 1.2, R_LO = 1e-3, R_HI = 1 - 1e-6
(which clip HNR to about [-30, 60] dB) and SILENT = 1e-20 are this tool's choices.

Window (`window`, `tables`).  With fs the integer sampling rate: h = floor(PERIODS fs / (2 F0_FLOOR)), N = 2 h + 1 samples (1397 at
22050 Hz); LMAX = floor(fs / F0_FLOOR) + 2.  A rate with N > MAX_WINDOW = 8191 (above about 129 kHz) or with LMAX >= N is refused.
w[k] = 0.5 - 0.5 cos(2 pi (k + 1) / (N + 1)), k < N: a Hann window without its zero end points.  rw[tau] = (sum_k w[k] w[k + tau]) /
(sum_k w[k]^2), tau = 0 .. LMAX, summed from the sampled window in numpy float64, not taken from the analytic formula.  Both tables
are built on the host and uploaded once per device and rate: the device evaluates no cosine.

Frame (`frames`, kernel fs2_hnr_frames, one workgroup per frame, the frame in LDS).  y (B, >= max lens) is float32 audio, f0 (B, >=
Tmax) an F0 track in Hz on the frame grid of `pitch` and `pyin`: frame t is centred at sample c = t hop.  x[k] = y[c - h + k], k < N,
taken as 0 outside [0, n).  mu = (sum x) / N, a[k] = (x[k] - mu) w[k], r0 = sum a^2.  A frame with f0[t] not above 0, or with r0 <=
SILENT N, is invalid: r = hnr = 0, valid = 0, lag = 0.  Otherwise tau0 = fs / f0[t], l0 = max(2, ceil(tau0 / SEARCH)), l1 =
min(LMAX - 1, floor(tau0 SEARCH)), and a frame with l1 < l0 is invalid too.  For the integers tau in [l0 - 1, l1 + 1]: r'(tau) =
(sum_{k = 0}^{N - 1 - tau} a[k] a[k + tau]) / (r0 rw[tau]), the product in the denominator first.  tau* is the first integer in
[l0, l1] that maximises r'.  With d = r'(tau* - 1) - 2 r'(tau*) + r'(tau* + 1) the peak is r'(tau*) - (r'(tau* + 1) - r'(tau* - 1))^2 /
(8 d) when d < 0, else r'(tau*).  r is the peak clipped to [R_LO, R_HI] and hnr = 10 log10(r / (1 - r)).  The output is (B, Tmax, 3)
= r, hnr, valid, with tau* in an int32 side buffer (B, Tmax).  Placing the search by the scored F0 track, where Boersma's algorithm
finds its own path through the candidates of all frames, is this tool's choice: the score asks how periodic the frame is at the
pitch both sides are scored at.  So is the parabola, where he interpolates with a windowed sinc: the parabola underestimates a
sharp peak slightly, on both sides alike.

Per side (`side`, kernel fs2_hnr_side).  Over the valid frames of a row: stats (B, 3) = n_valid, the mean of hnr and, in a second
pass, the central M2 = sum (hnr - mean)^2; all 0 without a valid frame.

Path (`on_path`, kernel fs2_hnr_on_path).  Along the cepstral DTW path `metrics.dtw` returns, over the cells (i, j) whose reference
frame i and synthesized frame j are both valid, with x, y their hnr: sums (B, 7) = the count P_v, the two means of a first pass, then
Sxx, Syy, Sxy about them and Sd2 = sum (x - y)^2; all 0 when P_v = 0.

Rows (`row_scores`).  hnr_frames_ref / _syn = n_valid, hnr_mean_db_ref / _syn = the mean, hnr_std_db_ref / _syn = sqrt(M2 / n_valid)
(the last two NaN when n_valid = 0); hnr_cells = P_v; hnr_diff_db = mean y - mean x, synthesized minus reference over the shared
cells; hnr_rmse_db = sqrt(Sd2 / P_v); hnr_corr = Sxy / sqrt(Sxx Syy), NaN when P_v < 2 or one of Sxx, Syy <= 1e-24 P_v (the floor of
cwt_corr).  The three path keys are NaN when hnr_cells = 0.

Summary (`summarize`).  hnr_frames_ref / _syn the corpus totals and hnr_mean_db_ref / _syn the means weighted by them (NaN without a
valid frame); hnr_cells the total, hnr_diff_db the mean weighted by the cells, hnr_rmse_db = sqrt(sum of the rows' Sd2 / the cells),
from the rows' values (NaN without a cell); hnr_corr_mean over the rows where it is not NaN and hnr_corr_nan_utterances;
hnr_unscored_utterances, the rows with hnr_cells = 0.

What is claimed: the definitions above, held against the restatement and against known answers (ten-harmonic tones in white noise at
20, 10 and 0 dB SNR within 1 dB, clean tones above 30 dB, white noise below -5 dB, a pair against itself, noise added to one side).
Not claimed: agreement with Praat, which cannot be run here; any number on real speech; the choices of 4.5 periods, the +-20 %
search, the parabola and the clip bounds; that a higher HNR is better: only reference against synthesis, and run against run,
compare.  Out of scope: band-wise HNR, jitter and shimmer, cepstral peak prominence, D4C aperiodicity.
"""
import math
from fractions import Fraction

import numpy as np
import torch

from . import _lib, ops
from .pitch import F0_CEIL, F0_FLOOR  # noqa: F401  (F0_CEIL: the shortest period the search is meant for)

WHO = "fastspeech2_amd.hnr"
MAX_FRAMES = 2048
MAX_WINDOW = 8191
PERIODS = 4.5
SEARCH = 1.2
R_LO, R_HI = 1e-3, 1 - 1e-6
SILENT = 1e-20
CORR_FLOOR = 1e-24                                          # = metrics.CORR_FLOOR
FRAME_BYTES = 28                                            # per frame and side: r, hnr, valid in float64 and the lag in int32
PATH_SUMS, SIDE_STATS = 7, 3


# ------------------------------------------------------------------------------------------------ host
def _rates(fs, hop):
    r, p = int(fs), int(hop)
    if r != fs or p != hop or r < 1 or not 1 <= p <= 1 << 20:
        raise ValueError(f"fs and hop must be positive integers, got {fs!r}, {hop!r}")
    return r, p


def window(fs):
    """-> (h, N, LMAX) at the integer sampling rate fs; a ValueError for a rate whose window does not fit."""
    fs, _ = _rates(fs, 1)
    h = int(Fraction(PERIODS) * fs / (2 * Fraction(F0_FLOOR)))
    N, lmax = 2 * h + 1, int(fs / Fraction(F0_FLOOR)) + 2
    if N > MAX_WINDOW or lmax >= N or lmax < 3:
        raise ValueError(f"at {fs} Hz the window has {N} samples and the longest lag is {lmax}: supported are windows of at most "
                         f"{MAX_WINDOW} samples that are longer than the longest lag")
    return h, N, lmax


def tables(fs):
    """-> (w (N,), rw (LMAX + 1,)) float64: the window and its normalised autocorrelation, summed from the samples."""
    _, N, lmax = window(fs)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(N, dtype=np.float64) + 1.0) / (N + 1.0))
    rw = np.array([np.dot(w[:N - tau], w[tau:]) for tau in range(lmax + 1)], np.float64) / np.dot(w, w)
    return w, rw


# ------------------------------------------------------------------------------------------------ device
_tables = {}


def _tables_on(dev, fs):
    key = (str(dev), int(fs))
    if key not in _tables:
        w, rw = tables(fs)
        _tables[key] = (torch.from_numpy(w).to(dev), torch.from_numpy(rw).to(dev))
    return _tables[key]


def _dev(t, dtype, dim, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{what} must be a tensor on the GPU ({WHO} has no CPU fallback)")
    if t.dtype != dtype or t.dim() != dim or (t.numel() and t.stride(-1) != 1):
        raise ValueError(f"{what} must be a {dim}-D {dtype} tensor with unit inner stride, got {t.dtype} {tuple(t.shape)}")
    return t


def _lens(lens, B, width, what, cap=MAX_FRAMES):
    h = [int(v) for v in (lens.tolist() if isinstance(lens, (torch.Tensor, np.ndarray)) else lens)]
    for n in h:
        if not 1 <= n <= cap:
            raise ValueError(f"{what}: a row of {n} is outside the supported 1..{cap}")
    if len(h) != B or width < max(h, default=0):
        raise ValueError(f"{what} of width {width} does not hold {len(h)} rows of up to {max(h, default=0)} (B = {B})")
    return h, max(h, default=1)


def _no_overlap(t, shape, what):
    """Strides (in elements) under which rows of `shape` (the trailing dimension has unit stride) do not overlap."""
    span = shape[-1]
    for d in range(len(shape) - 2, -1, -1):
        if shape[d] > 1:
            if t.stride(d) < span:
                raise ValueError(f"{what} {tuple(t.shape)} has overlapping strides {t.stride()}")
            span += (shape[d] - 1) * t.stride(d)
    return t


def _ld(t, d, need):
    """The stride of dimension d for the C side, which wants it >= need: that of a dimension of one entry (or none) says nothing."""
    return t.stride(d) if t.shape[d] > 1 else max(t.stride(d), need)


def _out(out, shape, dtype, what, device):
    """A caller's output buffer (strides of its own, at least `shape`) or a fresh one."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    out = _dev(out, dtype, len(shape), what)
    if out.device != device or out.shape[0] != shape[0] or any(o < s for o, s in zip(out.shape[1:], shape[1:])):
        raise ValueError(f"{what} {tuple(out.shape)} on {out.device} cannot hold {tuple(shape)} on {device}")
    return _no_overlap(out, shape, what)


def _frames_arg(fr, lens, what):
    """A (B, >= Tmax, >= 3) float64 buffer as `frames` writes it -> (fr, host lens, Tmax)."""
    fr = _dev(fr, torch.float64, 3, what)
    h, Tmax = _lens(lens, fr.shape[0], fr.shape[1], what)
    if fr.shape[2] < 3:
        raise ValueError(f"{what} {tuple(fr.shape)} does not hold r, hnr and valid per frame")
    return _no_overlap(fr, (fr.shape[0], Tmax, 3), what), h, Tmax


def frames(y, lens, f0, f0_frames, fs, hop, out=None, out_lag=None):
    """y (B, >= max lens) float32 audio on the device, lens samples per row, f0 (B, >= Tmax) float64 on the device in Hz (not above
    0: unvoiced), f0_frames frames per row -> (fr (B, Tmax, 3) float64 = r, hnr, valid; lag (B, Tmax) int32 = tau*), on the device.
    `out` / `out_lag` are buffers of the caller, at least that large; nothing at a frame >= f0_frames[b] is written."""
    fs, hop = _rates(fs, hop)
    h, _, lmax = window(fs)                                                 # refused before the device is touched
    y, f0 = _dev(y, torch.float32, 2, "y"), _dev(f0, torch.float64, 2, "f0")
    B = y.shape[0]
    if f0.shape[0] != B or f0.device != y.device:
        raise ValueError(f"y {tuple(y.shape)} on {y.device} and f0 {tuple(f0.shape)} on {f0.device} are not B rows on one device")
    nh, Nmax = _lens(lens, B, y.shape[1], "y", cap=1 << 30)
    th, Tmax = _lens(f0_frames, B, f0.shape[1], "f0")
    _no_overlap(y, (B, Nmax), "y")
    _no_overlap(f0, (B, Tmax), "f0")
    fr = _out(out, (B, Tmax, 3), torch.float64, "out", y.device)
    lag = _out(out_lag, (B, Tmax), torch.int32, "out_lag", y.device)
    w, rw = _tables_on(y.device, fs)
    lens_d = torch.tensor(nh, dtype=torch.int32, device=y.device)
    frames_d = torch.tensor(th, dtype=torch.int32, device=y.device)
    _lib.call("fs2_hnr_frames", y.data_ptr(), _ld(y, 0, Nmax), lens_d.data_ptr(), f0.data_ptr(), _ld(f0, 0, Tmax), frames_d.data_ptr(),
              w.data_ptr(), rw.data_ptr(), float(fs), hop, h, lmax, fr.data_ptr(), _ld(fr, 0, Tmax * _ld(fr, 1, 3)), _ld(fr, 1, 3),
              lag.data_ptr(), _ld(lag, 0, Tmax), B, Tmax, ops._stream())
    return fr, lag


def side(fr, f0_frames, out=None):
    """fr (B, >= Tmax, >= 3) as `frames` writes it -> stats (B, 3) float64 = n_valid, mean, M2 of hnr over the valid frames."""
    fr, th, Tmax = _frames_arg(fr, f0_frames, "fr")
    B = fr.shape[0]
    stats = _out(out, (B, SIDE_STATS), torch.float64, "out", fr.device)
    frames_d = torch.tensor(th, dtype=torch.int32, device=fr.device)
    _lib.call("fs2_hnr_side", fr.data_ptr(), _ld(fr, 0, Tmax * _ld(fr, 1, 3)), _ld(fr, 1, 3), frames_d.data_ptr(), stats.data_ptr(),
              _ld(stats, 0, SIDE_STATS), B, Tmax, ops._stream())
    return stats


def on_path(pi, pj, path_len, fr_ref, alens, fr_syn, blens, out=None):
    """Path (pi, pj (B, L) int32, path_len (B,) int32 as `metrics.dtw` returns them) and the frames fr_ref (B, >= T1max, >= 3),
    fr_syn (B, >= T2max, >= 3) float64 on the device -> sums (B, 7) float64: P_v, the two means, Sxx, Syy, Sxy, Sd2 of hnr over the
    cells valid on both sides."""
    pi, pj = _dev(pi, torch.int32, 2, "pi"), _dev(pj, torch.int32, 2, "pj")
    path_len = _dev(path_len, torch.int32, 1, "path_len")
    B = pi.shape[0]
    if pj.shape != pi.shape or pi.stride(0) != pj.stride(0) or path_len.shape[0] != B or not isinstance(fr_ref, torch.Tensor) \
            or not isinstance(fr_syn, torch.Tensor) or fr_ref.shape[:1] != (B,) or fr_syn.shape[:1] != (B,) \
            or len({t.device for t in (pi, pj, path_len, fr_ref, fr_syn)}) != 1:
        raise ValueError(f"path {tuple(pi.shape)} {tuple(pj.shape)} {tuple(path_len.shape)} and the frames of the two sides are not "
                         f"B pairs on one device")
    fr_ref, ah, T1 = _frames_arg(fr_ref, alens, "fr_ref")
    fr_syn, bh, T2 = _frames_arg(fr_syn, blens, "fr_syn")
    sums = _out(out, (B, PATH_SUMS), torch.float64, "out", pi.device)
    ad = torch.tensor(ah, dtype=torch.int32, device=pi.device)
    bd = torch.tensor(bh, dtype=torch.int32, device=pi.device)
    _lib.call("fs2_hnr_on_path", pi.data_ptr(), pj.data_ptr(), pi.stride(0), path_len.data_ptr(), fr_ref.data_ptr(),
              _ld(fr_ref, 0, T1 * _ld(fr_ref, 1, 3)), _ld(fr_ref, 1, 3), fr_syn.data_ptr(), _ld(fr_syn, 0, T2 * _ld(fr_syn, 1, 3)),
              _ld(fr_syn, 1, 3), ad.data_ptr(), bd.data_ptr(), sums.data_ptr(), _ld(sums, 0, PATH_SUMS), B, T1, T2, ops._stream())
    return sums


def measure(y, lens, f0, f0_frames, fs, hop):
    """The two per-side kernels chained -> (fr (B, Tmax, 3), stats (B, 3)) on the device."""
    fr, _ = frames(y, lens, f0, f0_frames, fs, hop)
    return fr, side(fr, f0_frames)


# ------------------------------------------------------------------------------------------------ scores
def row_keys():
    return ("hnr_mean_db_ref", "hnr_mean_db_syn", "hnr_std_db_ref", "hnr_std_db_syn", "hnr_frames_ref", "hnr_frames_syn", "hnr_cells",
            "hnr_diff_db", "hnr_rmse_db", "hnr_corr")


def row_scores(sums, stats_ref, stats_syn):
    """The HNR keys of a pair's row (module docstring) from the device results copied to the host: the path sums (7,) and per side
    the stats (3,)."""
    nan = float("nan")
    row = {}
    for name, q in (("ref", stats_ref), ("syn", stats_syn)):
        n = int(q[0])
        row["hnr_mean_db_" + name] = float(q[1]) if n else nan
        row["hnr_std_db_" + name] = math.sqrt(float(q[2]) / n) if n else nan
        row["hnr_frames_" + name] = n
    P, xm, ym, sxx, syy, sxy, sd2 = (float(v) for v in np.asarray(sums, np.float64).reshape(PATH_SUMS))
    P = int(P)
    ok = P >= 2 and sxx > CORR_FLOOR * P and syy > CORR_FLOOR * P
    row["hnr_cells"] = P
    row["hnr_diff_db"] = ym - xm if P else nan
    row["hnr_rmse_db"] = math.sqrt(sd2 / P) if P else nan
    row["hnr_corr"] = sxy / math.sqrt(sxx * syy) if ok else nan
    return {k: row[k] for k in row_keys()}


def summarize(rows):
    """The corpus keys of the module docstring from rows that carry the HNR keys."""
    nan = float("nan")
    out = {}
    for name in ("ref", "syn"):
        n = np.array([r["hnr_frames_" + name] for r in rows], np.float64)
        m = np.array([r["hnr_mean_db_" + name] for r in rows], np.float64)
        ok = n > 0
        out["hnr_frames_" + name] = int(n.sum())
        out["hnr_mean_db_" + name] = float((m[ok] * n[ok]).sum() / n[ok].sum()) if ok.any() else nan
    cells = np.array([r["hnr_cells"] for r in rows], np.float64)
    ok = cells > 0
    diff = np.array([r["hnr_diff_db"] for r in rows], np.float64)
    rmse = np.array([r["hnr_rmse_db"] for r in rows], np.float64)
    out["hnr_cells"] = int(cells.sum())
    out["hnr_diff_db"] = float((diff[ok] * cells[ok]).sum() / cells[ok].sum()) if ok.any() else nan
    out["hnr_rmse_db"] = float(math.sqrt((rmse[ok] ** 2 * cells[ok]).sum() / cells[ok].sum())) if ok.any() else nan
    corr = np.array([r["hnr_corr"] for r in rows], np.float64)
    fine = ~np.isnan(corr)
    out["hnr_corr_mean"] = float(corr[fine].mean()) if fine.any() else nan
    out["hnr_corr_nan_utterances"] = int((~fine).sum())
    out["hnr_unscored_utterances"] = int((~ok).sum())
    return out
