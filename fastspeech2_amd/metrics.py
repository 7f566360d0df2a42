"""Objective scoring of synthesized against recorded speech on the GPU: mel-cepstral distortion (MCD) along a dynamic-time-warping
(DTW) path, and F0 RMSE and voiced / unvoiced (V/UV) error on the same path.  HIP kernels in fp64 over ragged batches of pairs
(csrc/fs2_dtw.hip).  The specification below is what the kernels and the numpy oracle (tests/dtw_ref.py) implement.

WHAT THE NUMBERS ARE.  The cepstra are a DCT of this project's own 80-band natural-log mel spectrogram (`audio.TacotronSTFT`), not
WORLD / SPTK mel-cepstra of a spectral envelope.  The dB values compare two runs of this tool with each other; they are not
comparable with MCD figures published elsewhere.  That is `cepstra="mel"`, the default.  With `cepstra="world"` (`score.py --cepstra
world`) the cepstra are instead the mel-cepstra c~_1 .. c~_K of the CheapTrick spectral envelope at the utterance's own F0
(`envelope`, specified in full in its docstring): the published definition, independent of pitch, held against an fp64 numpy
restatement and analytic answers; its agreement with the pyworld / pysptk binaries is unmeasured.  Everything from the DTW on is the
same for both.

Cepstra.  x[m][t] is the log-mel (B, n_mel, T) exactly as `TacotronSTFT.mel_spectrogram_ragged` returns it, with its frame counts.
c[k][t] = sum_m x[m][t] C[k][m], m ascending, with the orthonormal DCT-II rows C[k][m] = sqrt(2 / n_mel) cos(pi k (2 m + 1) / (2 n_mel)),
k = 1 .. K (c0, the level, is excluded).  K = n_mcep defaults to 13 and is at most 40; n_mel is at most 128.  C is built on the host
in numpy float64 (`dct_table`) and uploaded: the device evaluates no cosine.  All arithmetic from here on is float64.

DTW, per pair (a: T1 reference frames, index i; b: T2 synthesized frames, index j).
  local cost    d(i, j) = sqrt(sum_k (a_k[i] - b_k[j])^2), k ascending, the products not fused into the sum, the root correctly rounded
  accumulated   D(0, 0) = d(0, 0);  D(i, j) = d(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), a missing neighbour = +inf
  backpointer   0 = (i-1, j-1), 1 = (i-1, j), 2 = (i, j-1); the lowest code wins ties (the aligner's rule); (0, 0) has code 0
  path          from (0, 0) to (T1-1, T2-1), P cells, max(T1, T2) <= P <= T1 + T2 - 1
There is no band (no Sakoe-Chiba window) and there are no slope weights.  1 <= T1, T2 <= 2048 (`max_frames()`); a longer sequence is
a ValueError before any launch.

Scores per pair.  mcd_db = (10 / ln 10) sqrt(2) D(T1-1, T2-1) / P.  With r = f0_ref[i], s = f0_syn[j] over the P path cells (i, j):
vuv_error = the share of cells where exactly one of r, s is 0;  f0_rmse_cents = sqrt(mean over the cells with r > 0 and s > 0 of
(1200 log2(s / r))^2), NaN when there is no such cell; n_voiced_pairs is their number.  Also path_len = P, frames_ref = T1,
frames_syn = T2.  F0 is DIO + StoneMask (`pitch`), or probabilistic YIN (`pyin`) with f0_estimator="pyin" (then every row says
so), with frame_period = hop / sampling_rate * 1000 as in `Preprocessor._extract_pitch`,
on the unclamped audio; the mel is taken of the audio clamped to [-1, 1].  F0 frame f and mel frame f are both centred at sample
f * hop.  Where the two frame counts of an utterance differ (the last frame), both are cut to the smaller before the DTW.

Corpus summary (`summarize`).  For mcd_db, f0_rmse_cents and vuv_error the mean of the per-utterance values and the mean weighted by
path_len (F0: over the utterances whose value is not NaN, weighted by n_voiced_pairs), and the number of utterances whose F0 score
is NaN.

Prosody (`prosody=True`, `score.py --prosody`; needs F0).  The numbers FastSpeech 2 reports for its variance adaptor: the moments of
the voiced F0 and the DTW distance between the pitch contours (its Table 3), the error of the frame energy (Table 4), and the
pitch-tracking error rates usually printed next to F0 RMSE.  The paper states neither how it treats unvoiced frames nor the unit of
its DTW distance: voiced-only contours in Hz, a distance normalised by the path length and energy in the preprocessor's
un-normalised units are this tool's choices, so the numbers compare runs of this tool and only roughly compare with the paper's.
All arithmetic is float64, sums are in a fixed order without atomics, padding is never read or written, two runs are byte-identical.
  On the path (`prosody_on_path`, kernel fs2_dtw_prosody).  The pair's path has P cells (i, j); r = f0_ref[i], s = f0_syn[j]; V is
  the set of cells with r > 0 and s > 0, n = |V| = n_voiced_pairs; e is the float32 STFT energy `mel_spectrogram_ragged` returns for
  the clamped audio (the L2 norm of the magnitudes of a frame, what `Preprocessor` extracts), cut to the pair's frame counts and
  promoted to float64.
    gross          the number of V cells with fabs(s - r) > 0.2 * r, evaluated as written: one subtraction, one product, nothing fused
    gpe            gross / n, NaN when n = 0
    ffe            (gross + V/UV mismatches) / P
    f0_corr        with x = ln r, y = ln s over V: xm = (sum x) / n, ym = (sum y) / n in a first pass, then Sxx = sum (x - xm)^2,
                   Syy = sum (y - ym)^2, Sxy = sum (x - xm)(y - ym); f0_corr = Sxy / sqrt(Sxx Syy), NaN when n < 2 or one of
                   Sxx, Syy <= 1e-24 n.  That floor is a standard deviation of ln F0 below 1e-12, a constant track: the rounding of
                   the mean alone leaves about 1e-29 per term, and no real track comes near 1e-12.
    energy_mae     sum |e_ref[i] - e_syn[j]| / P
    energy_mae_rel sum |e_ref[i] - e_syn[j]| / sum e_ref[i] over the same cells, NaN when that denominator is 0
  Per side, off the path (`voiced_contours`, kernel fs2_prosody_voiced).  The frames with f0 > 0 among the side's T frames, in order,
  are the contour u of n_v values in Hz.  Its mean um = (sum u) / n_v, then in a second pass M2 = sum (u - um)^2, M3 = sum (u - um)^3,
  M4 = sum (u - um)^4; with n_v = 0 all four are 0.  Rows carry them as f0_stats_ref / f0_stats_syn = {n, mean, m2, m3, m4}.
  Pitch-contour DTW (`contour_dtw`).  The recurrence, tie rule and kernels above with K = 1 on the two contours u (n_r values) and w
  (n_s values): the local cost sqrt((u - w)^2) is |u - w|.  f0_dtw_hz = D(n_r - 1, n_s - 1) / P', P' that path's length, reported as
  f0_dtw_path_len; NaN and 0 when a side has no voiced frame (such a pair is left out of the launch).  It runs after the cepstral
  DTW's cost and backpointer buffers are released and is no larger, n_v <= T.
  Summary.  For gpe, ffe, f0_corr, f0_dtw_hz, energy_mae and energy_mae_rel the mean and the weighted mean over the utterances whose
  value is not NaN (gpe and f0_corr weighted by n, ffe and the energy errors by P, f0_dtw_hz by P') and the number of NaN utterances
  (`<key>_nan_utterances`).  Corpus pitch moments per side: the per-utterance (n, mean, M2, M3, M4) merged pairwise in row order by
  Pebay's update formulas (`merge_moments`), then sigma = sqrt(M2 / N), gamma = (M3 / N) / sigma^3, K = (M4 / N) / sigma^4 - 3:
  population moments, excess kurtosis (the paper's K of about 1 for natural speech is an excess value), as f0_std_hz_ref,
  f0_skew_ref, f0_kurt_ref, the `_syn` three and the voiced frames N as f0_voiced_frames_ref / _syn; NaN where N = 0 (the skewness
  and kurtosis also where sigma = 0).
Without `prosody` every row and every summary key is what it is without this section.

Over-smoothing (`smoothing=True`, `score.py --smoothing`).  The global variance and the modulation spectrum of both sides' cepstra,
per utterance and off the path, specified in full in the docstring of `modspec`: every row also carries gv_ref, gv_syn,
gv_ratio_db, ms_db_ref, ms_db_syn, ms_band_db_ref, ms_band_db_syn and ms_dist_db, the summary ms_bands_hz, ms_diff_db_by_band,
ms_dist_db_corpus, gv_ratio_db_by_coef, the means gv_ratio_db_mean and ms_dist_db_mean with their `_nan_utterances` counts, and
smoothing_too_short_utterances.  Without `smoothing` every launch, every row and the summary are what they are without this paragraph.

Wavelet prosody (`wavelet=True`, `score.py --wavelet`; needs F0, not `prosody`).  The continuous wavelet transform of both sides'
interpolated, normalised ln F0 at ten scales one octave apart, compared along the cepstral path, specified in full in the docstring
of `cwt`: every row also carries cwt_corr, cwt_rmse, cwt_level_corr, cwt_level_rmse, cwt_power_db_ref, cwt_power_db_syn,
cwt_power_ratio_db, lf0_mean_ref, lf0_mean_syn, lf0_std_ref and lf0_std_syn, the summary cwt_scales_ms, the `_mean`, `_weighted` and
`_nan_utterances` lists of the first four, cwt_power_ratio_db_by_scale and wavelet_flat_utterances.  It scores the same F0 track as
the other F0 numbers (`f0_estimator`).  Without `wavelet` every launch, every row and the summary are what they are without this
paragraph.

Harmonics-to-noise ratio (`hnr=True`, `score.py --hnr`; needs F0, not `prosody`).  How much of each voiced frame's power repeats at
the pitch period (Boersma 1993), the measure of a hoarse, buzzy or noisy voice, taken of both sides' audio at the lags around the
scored F0 track (`f0_estimator`) and compared per side and along the cepstral path, specified in full in the docstring of `hnr`:
every row also carries hnr_mean_db_ref, hnr_mean_db_syn, hnr_std_db_ref, hnr_std_db_syn, hnr_frames_ref, hnr_frames_syn, hnr_cells,
hnr_diff_db, hnr_rmse_db and hnr_corr, the summary the frame-weighted hnr_mean_db_ref / _syn with hnr_frames_ref / _syn, hnr_cells,
the cell-weighted hnr_diff_db and hnr_rmse_db, hnr_corr_mean with hnr_corr_nan_utterances, and hnr_unscored_utterances.  Without
`hnr` every launch, every row and the summary are what they are without this paragraph.

Storage.  The local costs and backpointers of a pair are held skewed, cell (i, j) at row (i + j) mod T2, column i of a (T2max, T1max)
matrix: an anti-diagonal is contiguous, the buffer is no larger than the plain one (`unskew` undoes it for a test).  The accumulated
costs never leave the chip.  Determinism: no atomics, sums in a fixed order; two runs give byte-identical scores.
"""
import math
import os

import numpy as np
import torch

from . import _lib, ops, ragged

WHO = "fastspeech2_amd.metrics"
MAX_FRAMES, MAX_MCEP, MAX_MEL = 2048, 40, 128
MCD_SCALE = 10.0 / math.log(10.0) * math.sqrt(2.0)
CELL_BYTES = 9                                              # one float64 local cost and one backpointer byte per (i, j)
PROSODY_SUMS = 8                                            # gross, n, V/UV mismatches, Sxx, Syy, Sxy, sum |de|, sum e_ref
PROSODY_FRAME_BYTES = 24                                    # per frame: the compacted contour (8 B) and its share of the second path
CORR_FLOOR = 1e-24
SMOOTHING_BANDS = 8                                         # at most: the bands of `modspec.EDGES_HZ`
WAVELET_FRAME_BYTES = 88                                    # per frame and side: z and the ten scales of its transform, float64
HNR_FRAME_BYTES = 28                                        # per frame and side: r, hnr, valid in float64 and the lag in int32
PROSODY_SCORES = ("gpe", "ffe", "f0_corr", "f0_dtw_hz", "energy_mae", "energy_mae_rel")


def max_frames():
    return _lib.load().fs2_dtw_max_frames()


def dct_table(n_mel, n_mcep=13):
    """C (n_mcep, n_mel) float64: rows k = 1 .. n_mcep of the orthonormal DCT-II."""
    if not 1 <= n_mcep <= MAX_MCEP or not 1 <= n_mel <= MAX_MEL or n_mcep >= n_mel:
        raise ValueError(f"n_mcep must be in [1, {MAX_MCEP}] and below n_mel <= {MAX_MEL}, got n_mcep={n_mcep}, n_mel={n_mel}")
    k = np.arange(1, n_mcep + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mel, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / n_mel) * np.cos(np.pi * k * (2.0 * m + 1.0) / (2.0 * n_mel))


def check_frames(*lens):
    """Every length in [1, MAX_FRAMES], else ValueError: called before anything touches the device."""
    for ls in lens:
        for n in ls:
            if not 1 <= int(n) <= MAX_FRAMES:
                raise ValueError(f"a sequence of {int(n)} frames is outside the supported 1..{MAX_FRAMES} frames")


def _host_lens(lens):
    return [int(v) for v in (lens.tolist() if isinstance(lens, (torch.Tensor, np.ndarray)) else lens)]


def _dev(t, dtype, what, dim):
    ragged.require_device(t, WHO)
    if t.dtype != dtype or t.dim() != dim or (t.numel() and t.stride(-1) != 1):
        raise ValueError(f"{what} must be a {dim}-D {dtype} tensor with unit inner stride, got {t.dtype} {tuple(t.shape)}")
    return t


def _out(out, shape, dtype, what, device):
    """A caller's output buffer (any batch / row strides, at least `shape`) or a fresh one."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    out = _dev(out, dtype, what, len(shape))
    if out.shape[0] != shape[0] or any(o < s for o, s in zip(out.shape[1:], shape[1:])):
        raise ValueError(f"{what} {tuple(out.shape)} is too small for {tuple(shape)}")
    return out


# ------------------------------------------------------------------------------------------------ kernels
_tables = {}


def cepstra(mel, lens, n_mcep=13, out=None):
    """mel (B, n_mel, frames) float32 log-mel on the device, lens frames per row -> c (B, Tmax, n_mcep) float64."""
    ragged.require_device(mel, WHO)
    if mel.dtype != torch.float32 or mel.dim() != 3 or (mel.numel() and mel.stride(2) != 1):
        raise ValueError(f"mel must be a (B, n_mel, frames) float32 tensor with unit inner stride, got {mel.dtype} {tuple(mel.shape)}")
    B, n_mel, F = mel.shape
    lens_h, lens_d = ragged.lengths(lens, B, F, "lens", mel.device)
    key = (str(mel.device), n_mel, n_mcep)
    if key not in _tables:
        _tables[key] = torch.from_numpy(dct_table(n_mel, n_mcep)).to(mel.device)
    Tmax = max(lens_h, default=0)
    c = _out(out, (B, Tmax, n_mcep), torch.float64, "out", mel.device)
    _lib.call("fs2_mcep", mel.data_ptr(), mel.stride(0), mel.stride(1), lens_d.data_ptr(), _tables[key].data_ptr(), n_mcep,
              c.data_ptr(), c.stride(0), c.stride(1), B, n_mel, Tmax, ops._stream())
    return c


def _pairs(a, alens, b, blens):
    ah, bh = _host_lens(alens), _host_lens(blens)
    check_frames(ah, bh)
    a, b = _dev(a, torch.float64, "a", 3), _dev(b, torch.float64, "b", 3)
    B, K = a.shape[0], a.shape[2]
    if b.shape[0] != B or b.shape[2] != K or not 1 <= K <= MAX_MCEP:
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} are not B pairs of up to {MAX_MCEP} coefficients")
    _, ad = ragged.lengths(ah, B, a.shape[1], "alens", a.device)
    _, bd = ragged.lengths(bh, B, b.shape[1], "blens", a.device)
    return a, b, ah, bh, ad, bd, B, K


def _pair_lens(alens, blens):
    """Host lengths of both sides, refused before the device is touched when one is outside 1..MAX_FRAMES."""
    ah, bh = _host_lens(alens), _host_lens(blens)
    check_frames(ah, bh)
    return ah, bh, max(ah, default=0), max(bh, default=0)


def _lens_dev(ah, bh, B, device):
    return ragged.lengths(ah, B, MAX_FRAMES, "alens", device)[1], ragged.lengths(bh, B, MAX_FRAMES, "blens", device)[1]


def local_cost(a, alens, b, blens, out=None):
    """a (B, >= T1max, K), b (B, >= T2max, K) float64 cepstra -> the skewed local costs (B, T2max, T1max) float64."""
    a, b, ah, bh, ad, bd, B, K = _pairs(a, alens, b, blens)
    T1, T2 = max(ah, default=0), max(bh, default=0)
    cost = _out(out, (B, T2, T1), torch.float64, "out", a.device)
    _lib.call("fs2_dtw_cost", a.data_ptr(), a.stride(0), a.stride(1), ad.data_ptr(), b.data_ptr(), b.stride(0), b.stride(1),
              bd.data_ptr(), K, cost.data_ptr(), cost.stride(0), cost.stride(1), B, T1, T2, ops._stream())
    return cost


def scan(cost, alens, blens, out=None):
    """skewed local costs (B, >= T2max, >= T1max) -> (skewed backpointers uint8 (B, T2max, T1max), total (B,) float64)."""
    ah, bh, T1, T2 = _pair_lens(alens, blens)
    cost = _dev(cost, torch.float64, "cost", 3)
    B = cost.shape[0]
    ad, bd = _lens_dev(ah, bh, B, cost.device)
    if cost.shape[1] < T2 or cost.shape[2] < T1:
        raise ValueError(f"cost {tuple(cost.shape)} does not hold pairs of up to {T1} x {T2} frames")
    bp = _out(out, (B, T2, T1), torch.uint8, "out", cost.device)
    total = torch.empty(B, dtype=torch.float64, device=cost.device)
    _lib.call("fs2_dtw_scan", cost.data_ptr(), cost.stride(0), cost.stride(1), ad.data_ptr(), bd.data_ptr(), bp.data_ptr(),
              bp.stride(0), bp.stride(1), total.data_ptr(), B, T1, T2, ops._stream())
    return bp, total


def backtrack(bp, alens, blens, out=None):
    """skewed backpointers -> (path_len (B,) int32, pi, pj (B, T1max + T2max - 1) int32): the path from (0, 0); entries beyond a
    pair's path_len and below its T1 + T2 - 1 are -1.  `out` = (pi, pj) buffers of the caller."""
    ah, bh, T1, T2 = _pair_lens(alens, blens)
    bp = _dev(bp, torch.uint8, "bp", 3)
    B = bp.shape[0]
    ad, bd = _lens_dev(ah, bh, B, bp.device)
    if bp.shape[1] < T2 or bp.shape[2] < T1:
        raise ValueError(f"bp {tuple(bp.shape)} does not hold pairs of up to {T1} x {T2} frames")
    L = max(T1 + T2 - 1, 1)
    pi = _out(None if out is None else out[0], (B, L), torch.int32, "out[0]", bp.device)
    pj = _out(None if out is None else out[1], (B, L), torch.int32, "out[1]", bp.device)
    if pi.stride(0) != pj.stride(0):
        raise ValueError("the two path buffers need the same row stride")
    plen = torch.empty(B, dtype=torch.int32, device=bp.device)
    _lib.call("fs2_dtw_backtrack", bp.data_ptr(), bp.stride(0), bp.stride(1), ad.data_ptr(), bd.data_ptr(), pi.data_ptr(),
              pj.data_ptr(), pi.stride(0), plen.data_ptr(), B, T1, T2, ops._stream())
    return plen, pi, pj


def dtw(a, alens, b, blens):
    """Cepstra a (B, T1max, K), b (B, T2max, K) float64 on the device -> (total (B,) float64 = D(T1-1, T2-1), path_len (B,) int32,
    pi, pj (B, T1max + T2max - 1) int32), all on the device."""
    cost = local_cost(a, alens, b, blens)
    bp, total = scan(cost, alens, blens)
    del cost
    plen, pi, pj = backtrack(bp, alens, blens)
    return total, plen, pi, pj


def f0_on_path(pi, pj, path_len, f0_ref, alens, f0_syn, blens, out=None):
    """Path (pi, pj, path_len as `dtw` returns them) and F0 tracks f0_ref (B, >= T1max), f0_syn (B, >= T2max) float64 on the device
    -> sums (B, 3) float64: V/UV mismatches, both-voiced cells, the sum of their squared cents."""
    ah, bh, T1, T2 = _pair_lens(alens, blens)
    pi, pj = _dev(pi, torch.int32, "pi", 2), _dev(pj, torch.int32, "pj", 2)
    B = pi.shape[0]
    ad, bd = _lens_dev(ah, bh, B, pi.device)
    f0_ref, f0_syn = _dev(f0_ref, torch.float64, "f0_ref", 2), _dev(f0_syn, torch.float64, "f0_syn", 2)
    path_len = _dev(path_len, torch.int32, "path_len", 1)
    if pj.shape != pi.shape or pi.stride(0) != pj.stride(0) or path_len.shape[0] != B or f0_ref.shape[0] != B or f0_syn.shape[0] != B \
            or f0_ref.shape[1] < T1 or f0_syn.shape[1] < T2:
        raise ValueError(f"path {tuple(pi.shape)} {tuple(pj.shape)}, f0 {tuple(f0_ref.shape)} {tuple(f0_syn.shape)} and the lengths "
                         f"do not fit together")
    sums = _out(out, (B, 3), torch.float64, "out", pi.device)
    _lib.call("fs2_dtw_f0", pi.data_ptr(), pj.data_ptr(), pi.stride(0), path_len.data_ptr(), f0_ref.data_ptr(), f0_ref.stride(0),
              f0_syn.data_ptr(), f0_syn.stride(0), ad.data_ptr(), bd.data_ptr(), sums.data_ptr(), sums.stride(0), B, T1, T2,
              ops._stream())
    return sums


def _on_device(t, dtype, what, dim):
    """`_dev` for the prosody entry points, which refuse a host tensor like every other bad argument: a ValueError."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{what} must be a tensor on the GPU ({WHO} has no CPU fallback)")
    return _dev(t, dtype, what, dim)


def voiced_contours(f0, lens, out=None):
    """F0 tracks f0 (B, >= Tmax) float64 on the device, lens frames per row -> (contour (B, Tmax) float64 holding row b's voiced
    frames, in order, in [b, :n_v[b]] and nothing written beyond, n_v (B,) int32, stats (B, 5) float64 = n_v, mean, M2, M3, M4),
    all on the device.  `out` is a caller's contour buffer, any row stride."""
    lens_h = _host_lens(lens)
    for n in lens_h:
        if n > MAX_FRAMES:
            raise ValueError(f"a sequence of {n} frames is outside the supported 0..{MAX_FRAMES} frames")
    f0 = _on_device(f0, torch.float64, "f0", 2)
    B = f0.shape[0]
    _, lens_d = ragged.lengths(lens_h, B, f0.shape[1], "lens", f0.device)
    Tmax = max(lens_h, default=0)
    contour = _out(out, (B, Tmax), torch.float64, "out", f0.device)
    n_v = torch.empty(B, dtype=torch.int32, device=f0.device)
    stats = torch.empty(B, 5, dtype=torch.float64, device=f0.device)
    _lib.call("fs2_prosody_voiced", f0.data_ptr(), f0.stride(0), lens_d.data_ptr(), contour.data_ptr(), contour.stride(0),
              n_v.data_ptr(), stats.data_ptr(), stats.stride(0), B, Tmax, ops._stream())
    return contour, n_v, stats


def prosody_on_path(pi, pj, path_len, f0_ref, alens, f0_syn, blens, e_ref, e_syn, out=None):
    """Path and F0 tracks as `f0_on_path` takes them, frame energies e_ref (B, >= T1max), e_syn (B, >= T2max) float32 on the device
    -> sums (B, 8) float64: gross pitch errors, both-voiced cells n, V/UV mismatches, Sxx, Syy, Sxy of ln F0 over the both-voiced
    cells, sum |e_ref - e_syn|, sum e_ref (module docstring)."""
    ah, bh, T1, T2 = _pair_lens(alens, blens)
    pi, pj = _on_device(pi, torch.int32, "pi", 2), _on_device(pj, torch.int32, "pj", 2)
    f0_ref, f0_syn = _on_device(f0_ref, torch.float64, "f0_ref", 2), _on_device(f0_syn, torch.float64, "f0_syn", 2)
    e_ref, e_syn = _on_device(e_ref, torch.float32, "e_ref", 2), _on_device(e_syn, torch.float32, "e_syn", 2)
    path_len = _on_device(path_len, torch.int32, "path_len", 1)
    B = pi.shape[0]
    ad, bd = _lens_dev(ah, bh, B, pi.device)
    if pj.shape != pi.shape or pi.stride(0) != pj.stride(0) or any(t.shape[0] != B for t in (path_len, f0_ref, f0_syn, e_ref, e_syn)) \
            or min(f0_ref.shape[1], e_ref.shape[1]) < T1 or min(f0_syn.shape[1], e_syn.shape[1]) < T2:
        raise ValueError(f"path {tuple(pi.shape)} {tuple(pj.shape)}, f0 {tuple(f0_ref.shape)} {tuple(f0_syn.shape)}, energy "
                         f"{tuple(e_ref.shape)} {tuple(e_syn.shape)} and the lengths do not fit together")
    sums = _out(out, (B, PROSODY_SUMS), torch.float64, "out", pi.device)
    _lib.call("fs2_dtw_prosody", pi.data_ptr(), pj.data_ptr(), pi.stride(0), path_len.data_ptr(), f0_ref.data_ptr(), f0_ref.stride(0),
              f0_syn.data_ptr(), f0_syn.stride(0), e_ref.data_ptr(), e_ref.stride(0), e_syn.data_ptr(), e_syn.stride(0),
              ad.data_ptr(), bd.data_ptr(), sums.data_ptr(), sums.stride(0), B, T1, T2, ops._stream())
    return sums


def contour_dtw(u, n_ref, w, n_syn):
    """Compacted contours u (B, >= max n_ref), w (B, >= max n_syn) float64 on the device and their voiced counts on the host ->
    (total (B,) float64 = D(n_r - 1, n_s - 1), path_len (B,) int32, pi, pj (B, L) int32, launched): `dtw` with K = 1 over the pairs
    whose two sides both have a voiced frame, whose indices are `launched`; the others get NaN, 0 and -1 and reach no kernel."""
    nr, ns = _host_lens(n_ref), _host_lens(n_syn)
    for n in nr + ns:
        if not 0 <= n <= MAX_FRAMES:
            raise ValueError(f"a contour of {n} frames is outside the supported 0..{MAX_FRAMES} frames")
    u, w = _on_device(u, torch.float64, "u", 2), _on_device(w, torch.float64, "w", 2)
    B = u.shape[0]
    if w.shape[0] != B:
        raise ValueError(f"u {tuple(u.shape)} and w {tuple(w.shape)} are not B pairs of contours")
    ragged.lengths(nr, B, u.shape[1], "n_ref")
    ragged.lengths(ns, B, w.shape[1], "n_syn")
    launched = [p for p in range(B) if nr[p] > 0 and ns[p] > 0]
    T1, T2 = max((nr[p] for p in launched), default=1), max((ns[p] for p in launched), default=1)
    L = T1 + T2 - 1
    total = torch.full((B,), float("nan"), dtype=torch.float64, device=u.device)
    plen = torch.zeros(B, dtype=torch.int32, device=u.device)
    pi = torch.full((B, L), -1, dtype=torch.int32, device=u.device)
    pj = torch.full((B, L), -1, dtype=torch.int32, device=u.device)
    if launched:
        sel = torch.tensor(launched, dtype=torch.int64, device=u.device)
        a, b = u.index_select(0, sel)[:, :T1].unsqueeze(2), w.index_select(0, sel)[:, :T2].unsqueeze(2)
        la, lb = [nr[p] for p in launched], [ns[p] for p in launched]
        cost = local_cost(a, la, b, lb)
        bp, t = scan(cost, la, lb)
        del cost
        qi, qj = pi[:len(launched)].clone(), pj[:len(launched)].clone()      # -1 everywhere: backtrack leaves a row's tail alone
        n, qi, qj = backtrack(bp, la, lb, out=(qi, qj))
        total[sel], plen[sel], pi[sel], pj[sel] = t, n, qi, qj
    return total, plen, pi, pj, launched


def unskew(m, alens, blens, fill):
    """Skewed (B, T2max, T1max) numpy array -> plain (B, T1max, T2max) with `fill` outside each pair (for tests and debugging)."""
    m = np.asarray(m)
    out = np.full((m.shape[0], m.shape[2], m.shape[1]), fill, m.dtype)
    for p, (T1, T2) in enumerate(zip(alens, blens)):
        i, j = np.meshgrid(np.arange(T1), np.arange(T2), indexing="ij")
        out[p, :T1, :T2] = m[p, (i + j) % T2, i]
    return out


# ------------------------------------------------------------------------------------------------ scores
def scores_from_sums(total, path_len, frames_ref, frames_syn, sums=None):
    """The per-pair dict of the module docstring from the device results copied to the host."""
    P = int(path_len)
    row = {"mcd_db": MCD_SCALE * float(total) / P, "path_len": P, "frames_ref": int(frames_ref), "frames_syn": int(frames_syn)}
    if sums is not None:
        nv = int(sums[1])
        row["vuv_error"] = float(sums[0]) / P
        row["f0_rmse_cents"] = math.sqrt(float(sums[2]) / nv) if nv else float("nan")
        row["n_voiced_pairs"] = nv
    return row


def prosody_scores(sums, path_len, stats_ref, stats_syn, contour_total, contour_len):
    """The prosody keys of a pair's row (module docstring) from the device results copied to the host: the 8 path sums, the 5
    per-side statistics and the pitch-contour DTW's total and path length."""
    nan = float("nan")
    P, gross, n, mism = int(path_len), int(sums[0]), int(sums[1]), int(sums[2])
    sxx, syy, sxy, de, se = (float(v) for v in sums[3:8])
    corr_ok = n >= 2 and sxx > CORR_FLOOR * n and syy > CORR_FLOOR * n
    Pc = int(contour_len)
    stat = lambda q: {"n": int(q[0]), "mean": float(q[1]), "m2": float(q[2]), "m3": float(q[3]), "m4": float(q[4])}   # noqa: E731
    return {"gpe": gross / n if n else nan, "ffe": (gross + mism) / P, "f0_corr": sxy / math.sqrt(sxx * syy) if corr_ok else nan,
            "f0_dtw_hz": float(contour_total) / Pc if Pc else nan, "f0_dtw_path_len": Pc, "energy_mae": de / P,
            "energy_mae_rel": de / se if se != 0.0 else nan, "f0_stats_ref": stat(stats_ref), "f0_stats_syn": stat(stats_syn)}


def merge_moments(a, b):
    """(n, mean, M2, M3, M4) of two disjoint sets -> those of their union (Pebay's pairwise update formulas), in float64."""
    na, ma, a2, a3, a4 = a
    nb, mb, b2, b3, b4 = b
    if na == 0:
        return b
    if nb == 0:
        return a
    n = na + nb
    d = mb - ma
    m2 = a2 + b2 + d * d * na * nb / n
    m3 = a3 + b3 + d ** 3 * na * nb * (na - nb) / n ** 2 + 3.0 * d * (na * b2 - nb * a2) / n
    m4 = a4 + b4 + d ** 4 * na * nb * (na * na - na * nb + nb * nb) / n ** 3 + 6.0 * d * d * (na * na * b2 + nb * nb * a2) / n ** 2 \
        + 4.0 * d * (na * b3 - nb * a3) / n
    return n, ma + d * nb / n, m2, m3, m4


def corpus_moments(stats):
    """Per-utterance {n, mean, m2, m3, m4} dicts, merged in the order given -> (N, sigma, skewness, excess kurtosis); NaN without
    a voiced frame, the last two also when sigma = 0."""
    acc = (0, 0.0, 0.0, 0.0, 0.0)
    for q in stats:
        acc = merge_moments(acc, (int(q["n"]), float(q["mean"]), float(q["m2"]), float(q["m3"]), float(q["m4"])))
    N, _, m2, m3, m4 = acc
    nan = float("nan")
    if N == 0:
        return 0, nan, nan, nan
    sigma = math.sqrt(m2 / N)
    if sigma == 0.0:
        return N, 0.0, nan, nan
    return N, sigma, (m3 / N) / sigma ** 3, (m4 / N) / sigma ** 4 - 3.0


def _summarize_prosody(rows, out):
    weights = {"gpe": "n_voiced_pairs", "f0_corr": "n_voiced_pairs", "ffe": "path_len", "energy_mae": "path_len",
               "energy_mae_rel": "path_len", "f0_dtw_hz": "f0_dtw_path_len"}
    for key in PROSODY_SCORES:
        v = np.array([r[key] for r in rows], np.float64)
        w = np.array([r[weights[key]] for r in rows], np.float64)
        ok = ~np.isnan(v)
        out[key + "_mean"] = float(v[ok].mean()) if ok.any() else float("nan")
        out[key + "_weighted"] = float((v[ok] * w[ok]).sum() / w[ok].sum()) if ok.any() and w[ok].sum() > 0 else float("nan")
        out[key + "_nan_utterances"] = int((~ok).sum())
    for side in ("ref", "syn"):
        N, sigma, skew, kurt = corpus_moments([r["f0_stats_" + side] for r in rows])
        out["f0_voiced_frames_" + side], out["f0_std_hz_" + side] = N, sigma
        out["f0_skew_" + side], out["f0_kurt_" + side] = skew, kurt


def summarize(rows):
    """Corpus summary of per-utterance score dicts (module docstring)."""
    out = {"utterances": len(rows)}
    if not rows:
        return out
    w = np.array([r["path_len"] for r in rows], np.float64)
    mcd = np.array([r["mcd_db"] for r in rows], np.float64)
    out["mcd_db_mean"] = float(mcd.mean())
    out["mcd_db_weighted"] = float((mcd * w).sum() / w.sum())
    if "vuv_error" in rows[0]:
        vuv = np.array([r["vuv_error"] for r in rows], np.float64)
        f0 = np.array([r["f0_rmse_cents"] for r in rows], np.float64)
        nv = np.array([r["n_voiced_pairs"] for r in rows], np.float64)
        ok = ~np.isnan(f0)
        out["vuv_error_mean"] = float(vuv.mean())
        out["vuv_error_weighted"] = float((vuv * w).sum() / w.sum())
        out["f0_rmse_cents_mean"] = float(f0[ok].mean()) if ok.any() else float("nan")
        out["f0_rmse_cents_weighted"] = float((f0[ok] * nv[ok]).sum() / nv[ok].sum()) if ok.any() else float("nan")
        out["f0_nan_utterances"] = int((~ok).sum())
    if "gpe" in rows[0]:
        _summarize_prosody(rows, out)
    if "gv_ratio_db" in rows[0]:
        from . import modspec as Modspec
        out.update(Modspec.summarize(rows))
    if "cwt_corr" in rows[0]:
        from . import cwt as Cwt
        out.update(Cwt.summarize(rows))
    if "hnr_cells" in rows[0]:
        from . import hnr as Hnr
        out.update(Hnr.summarize(rows))
    return out


def batch_bytes(n, T1, T2, n_mcep=13, hop_length=256, fft_size=0, prosody=False, smoothing=False, wavelet=False, hnr=False):
    """What a batch of n pairs padded to (T1, T2) frames holds on the device: 9 B per (i, j) cell (local cost + backpointer), the
    audio, its STFT workspace and mel (about 40 B per sample), cepstra, F0 and the path; with `fft_size` (cepstra="world") also the
    spectral envelope, fft_size / 2 + 1 float64 bins per frame and side; with `prosody` the compacted contours and the second path
    (24 B per frame; the contour DTW's cells reuse the first DTW's, released by then); with `smoothing` the moments and band values
    of both sides, (2 + SMOOTHING_BANDS) float64 per coefficient and side; with `wavelet` the normalised contour and the ten scales
    of its transform, 88 B per frame and side; with `hnr` r, hnr, valid and the lag of every frame, 28 B per frame and side."""
    return n * (T1 * T2 * CELL_BYTES + (T1 + T2) * (hop_length * 40 + n_mcep * 8 + 64 + (fft_size // 2 + 1) * 8 * (fft_size > 0)
                                                    + PROSODY_FRAME_BYTES * bool(prosody) + WAVELET_FRAME_BYTES * bool(wavelet)
                                                    + HNR_FRAME_BYTES * bool(hnr))
                + 2 * n_mcep * (2 + SMOOTHING_BANDS) * 8 * bool(smoothing))


def load_audio(path, sampling_rate):
    """float32 mono waveform of a wav file that must already be at `sampling_rate`."""
    from .preprocess import load_wav
    wav, sr = load_wav(path, resample=False)
    if sr != sampling_rate:
        raise ValueError(f"{path} is at {sr} Hz, the config's sampling_rate is {sampling_rate} Hz: scoring does not resample; convert "
                         f"the corpus with prepare_align.py (its --resample gpu path) first")
    return wav.astype(np.float32)


def frame_counts(n_samples, sampling_rate, hop_length, f0=True):
    """Frames of an utterance of n samples: the mel's n // hop + 1, cut to DIO's count where that is smaller."""
    from .pitch import frame_count
    T = n_samples // hop_length + 1
    return min(T, frame_count(n_samples, sampling_rate, hop_length / sampling_rate * 1000)) if f0 else T


def score_pairs(ref_wavs, syn_wavs, stft, sampling_rate, hop_length, n_mcep=None, f0=True, device="cuda", budget=4 << 30,
                cepstra="mel", alpha=None, prosody=False, f0_estimator="dio", smoothing=False, wavelet=False, hnr=False):
    """Scores of (recorded, synthesized) pairs of float32 waveforms at `sampling_rate` -> one dict per pair (module docstring), in
    the order given.  `stft` is the config's `audio.TacotronSTFT`.  Pairs are packed longest first into ragged batches under `budget`
    bytes of device buffers; per batch: both sides through one pinned staging buffer, mel -> cepstra -> local cost -> scan ->
    backtrack (and DIO + StoneMask -> the path sums with `f0`), one D2H copy of the scores.  With cepstra="world" the cepstra are
    `envelope.world_cepstra` (n_mcep 24 by default, all-pass constant `alpha` or the table's) of the unclamped audio at its DIO +
    StoneMask F0, which is then always extracted, on DIO's frame grid, and only reported with `f0`; no mel is taken and `stft` may
    be None.  Every row then also carries cepstra, alpha and fft_size.  With `prosody` (needs `f0` and the STFT) every row also
    carries the prosody keys of the module docstring: the STFT's frame energy is kept (with cepstra="world" the STFT is run on the
    clamped audio for it alone), both F0 tracks are compacted, with one D2H copy of the voiced counts per side, and the
    pitch-contour DTW runs once the cepstral DTW's buffers are released.  `f0_estimator` "pyin" takes the F0 track of both sides of
    every F0 and prosody score from probabilistic YIN (`pyin`, the same frame grid) instead of DIO + StoneMask, and every row then
    carries f0_estimator; with "dio" the rows are what they were before that choice existed.  CheapTrick (cepstra="world") keeps
    its own DIO + StoneMask track whatever the estimator.  The pYIN workspace of a batch (`pyin.workspace_bytes`) counts towards
    `budget`.  With `smoothing` the two kernels of `modspec` run on both sides' cepstra, whichever they are, before these are
    released, their results ride in the batch's one D2H copy, and every row also carries the over-smoothing keys of the module
    docstring.  With `wavelet` (needs `f0`) the three kernels of `cwt` run on both sides' scored F0 track, the path stays alive until
    the path sums are taken, the results ride in the same D2H copy, and every row also carries the wavelet keys.  With `hnr` (needs `f0`) the two
    per-side kernels of `hnr` run on each side's audio and scored F0 track while the audio is on the device, the path kernel before
    the path is released, the results ride in the same D2H copy, and every row also carries the HNR keys."""
    from . import cwt as Cwt
    from . import hnr as Hnr
    from . import envelope as Env
    from . import modspec as Modspec
    if f0_estimator not in ("dio", "pyin"):
        raise ValueError(f"f0_estimator must be 'dio' or 'pyin', got {f0_estimator!r}")
    if prosody and not f0:
        raise ValueError("prosody scores need F0: prosody=True cannot go with f0=False")
    if wavelet and not f0:
        raise ValueError("wavelet prosody scores need F0: wavelet=True cannot go with f0=False")
    if wavelet:
        Cwt.scales(sampling_rate, hop_length)                               # a hop above 20 ms is refused before any work
    if hnr and not f0:
        raise ValueError("the harmonics-to-noise ratio needs F0: hnr=True cannot go with f0=False")
    if hnr:
        Hnr.window(sampling_rate)                                           # a rate whose window does not fit is refused before any work
    if prosody and stft is None:
        raise ValueError("prosody scores need the STFT for the frame energy: stft=None cannot go with prosody=True")
    if cepstra not in ("mel", "world"):
        raise ValueError(f"cepstra must be 'mel' or 'world', got {cepstra!r}")
    world = cepstra == "world"
    if len(ref_wavs) != len(syn_wavs):
        raise ValueError(f"{len(ref_wavs)} reference and {len(syn_wavs)} synthesized waveforms")
    if stft is not None and hop_length != stft.hop_length:
        raise ValueError(f"hop_length {hop_length} is not the STFT's {stft.hop_length}")
    fft_size = 0
    if world:
        n_mcep = Env.check_mcep(Env.DEFAULT_MCEP if n_mcep is None else n_mcep)
        fft_size, alpha = Env.fft_size(sampling_rate), Env.alpha_for(sampling_rate, alpha)
        empty = [len(w) for w in list(ref_wavs) + list(syn_wavs) if len(w) < 1]
        if empty:
            raise ValueError("a waveform without samples has no spectral envelope")
    else:
        if stft is None or alpha is not None:
            raise ValueError("cepstra='mel' needs the STFT and takes no alpha")
        n_mcep = 13 if n_mcep is None else n_mcep
        dct_table(stft.n_mel_channels, n_mcep)                              # validates n_mcep before any work
    fr = [frame_counts(len(w), sampling_rate, hop_length, f0 or world) for w in ref_wavs]
    fs = [frame_counts(len(w), sampling_rate, hop_length, f0 or world) for w in syn_wavs]
    check_frames(fr, fs)
    bins = Modspec.band_bins(sampling_rate, hop_length)[0] if smoothing else None
    short = [] if world and not prosody else [len(w) for w in list(ref_wavs) + list(syn_wavs) if len(w) <= stft.filter_length // 2]
    if short:
        raise ValueError(f"a waveform of {short[0]} samples is too short for the STFT's reflect padding ({stft.filter_length // 2})")
    dev = ragged.require_device(torch.device(device), WHO)
    staging = ragged.Staging()
    frame_period = hop_length / sampling_rate * 1000
    rows = [None] * len(ref_wavs)
    cepstra_fn = globals()["cepstra"]                                       # the argument `cepstra` shadows the module's function

    def side(wavs, frames):
        staging.pack(wavs)
        y, lens = staging.to(dev), [len(w) for w in wavs]
        track = scored = None
        if world or (f0 and f0_estimator == "dio"):
            from . import pitch as Pitch
            f, _, f_frames = Pitch.dio(y, lens, sampling_rate, frame_period)
            track = scored = Pitch.stonemask(y, lens, f, f_frames, sampling_rate, frame_period)
        if f0 and f0_estimator == "pyin":                                   # the scores' track; CheapTrick keeps `track`
            from . import pyin as Pyin
            scored = Pyin.pyin(y, lens, sampling_rate, frame_period)[0]
        mel = energy = None
        if prosody or not world:
            mel, energy, _ = stft.mel_spectrogram_ragged(y.clamp(-1.0, 1.0), lens)
        harm = Hnr.measure(y, lens, scored, frames, sampling_rate, hop_length) if hnr else None
        if world:
            return Env.world_cepstra(y, lens, track, frames, sampling_rate, frame_period, n_mcep, alpha), scored if f0 else None, energy, harm
        return cepstra_fn(mel, frames, n_mcep), scored, energy, harm

    cost = lambda n, T1, T2: batch_bytes(n, T1, T2, n_mcep, hop_length, fft_size, prosody, smoothing, wavelet, hnr)     # noqa: E731
    if f0 and f0_estimator == "pyin":                                       # one side's pYIN chunk workspace lives at a time
        from . import pyin as Pyin
        cepstral = cost
        cost = lambda n, T1, T2: cepstral(n, T1, T2) + Pyin.workspace_bytes(n, max(T1, T2))     # noqa: E731
    for batch in ragged.greedy_batches(list(zip(fr, fs)), budget, cost):
        al, bl = [fr[i] for i in batch], [fs[i] for i in batch]
        a, f0a, ea, ha = side([ref_wavs[i] for i in batch], al)
        b, f0b, eb, hb = side([syn_wavs[i] for i in batch], bl)
        total, plen, pi, pj = dtw(a, al, b, bl)
        smooth = [v.reshape(len(batch), -1) for v in Modspec.measure(a, al, bins) + Modspec.measure(b, bl, bins)] if smoothing else []
        del a, b
        cols = [total, plen.to(torch.float64)]
        if f0:
            cols += list(f0_on_path(pi, pj, plen, f0a, al, f0b, bl).unbind(1))
        if wavelet:                                                         # before the path is released below
            Wa, pwa, sta = Cwt.measure(f0a, al, sampling_rate, hop_length)
            Wb, pwb, stb = Cwt.measure(f0b, bl, sampling_rate, hop_length)
            smooth += [Cwt.on_path(pi, pj, plen, Wa, al, Wb, bl).reshape(len(batch), -1), pwa, sta, pwb, stb]
            del Wa, Wb
        n_wave = sum(v.shape[1] for v in smooth) - (2 * n_mcep * (1 + len(bins)) if smoothing else 0)
        if hnr:                                                             # before the path is released below
            smooth += [Hnr.on_path(pi, pj, plen, ha[0], al, hb[0], bl), ha[1], hb[1]]
            del ha, hb
        if prosody:
            cols += list(prosody_on_path(pi, pj, plen, f0a, al, f0b, bl, ea, eb).unbind(1))
            del pi, pj
            u, nu, su = voiced_contours(f0a, al)
            w, nw, sw = voiced_contours(f0b, bl)
            ctotal, cplen, _, _, _ = contour_dtw(u, nu.cpu(), w, nw.cpu())    # the voiced counts: one small D2H copy per side
            cols += list(su.unbind(1)) + list(sw.unbind(1)) + [ctotal, cplen.to(torch.float64)]
        n_cols, n_smooth = len(cols), 2 * n_mcep * (1 + len(bins)) if smoothing else 0
        scores = torch.stack(cols, dim=1)
        host = (torch.cat([scores] + smooth, dim=1) if smooth else scores).cpu().numpy()     # the batch's one D2H copy of the scores
        for r, i in enumerate(batch):
            rows[i] = scores_from_sums(host[r, 0], host[r, 1], al[r], bl[r], host[r, 2:5] if f0 else None)
            if prosody:
                q = host[r, 5:n_cols]
                rows[i].update(prosody_scores(q[:8], host[r, 1], q[8:13], q[13:18], q[18], q[19]))
            if smoothing:
                m2a, ba, m2b, bb = np.split(host[r, n_cols:n_cols + n_smooth], np.cumsum([n_mcep, n_mcep * len(bins), n_mcep])[:3])
                rows[i].update(Modspec.row_scores(m2a, ba.reshape(n_mcep, -1), al[r], m2b, bb.reshape(n_mcep, -1), bl[r]))
            if wavelet:
                ws, pwa, sta, pwb, stb = np.split(host[r, n_cols + n_smooth:n_cols + n_smooth + n_wave],
                                                  np.cumsum([Cwt.COMPONENTS * 4, Cwt.SCALES, 4, Cwt.SCALES]))
                rows[i].update(Cwt.row_scores(ws, host[r, 1], pwa, al[r], sta, pwb, bl[r], stb))
            if hnr:
                hs, hsa, hsb = np.split(host[r, n_cols + n_smooth + n_wave:], np.cumsum([Hnr.PATH_SUMS, Hnr.SIDE_STATS]))
                rows[i].update(Hnr.row_scores(hs, hsa, hsb))
            if world:
                rows[i].update(cepstra="world", alpha=alpha, fft_size=fft_size)
            if f0 and f0_estimator != "dio":
                rows[i]["f0_estimator"] = f0_estimator
    return rows


# ------------------------------------------------------------------------------------------------ the corpus pass
def collect(config, result_path, source, syn_dir=None, ref_dir=None, trim=True):
    """The pairs of `source`'s lines (`basename|speaker|...`): -> (items [dict(basename, speaker, ref, syn, window)], skipped
    [(basename, reason)]).  The reference is `{raw_path}/{speaker}/{basename}.wav` (or `{ref_dir}/{basename}.wav`), the synthesized
    file `{result_path}/{basename}.wav` (or in `syn_dir`).  With `trim` and a TextGrid the reference is cut to the speech window
    `Preprocessor.get_alignment` gives (the window the training mel came from): window = "textgrid"; else "whole"."""
    from .preprocess import Preprocessor, read_textgrid
    sr = config["preprocessing"]["audio"]["sampling_rate"]
    hop = config["preprocessing"]["stft"]["hop_length"]
    half = config["preprocessing"]["stft"]["filter_length"] // 2
    items, skipped = [], []
    with open(source, encoding="utf-8") as f:
        lines = [ln.strip("\n") for ln in f if ln.strip()]
    for ln in lines:
        parts = ln.split("|")
        if len(parts) < 2:
            skipped.append((parts[0], "no speaker field"))
            continue
        basename, speaker = parts[0], parts[1]
        ref = os.path.join(ref_dir, basename + ".wav") if ref_dir else os.path.join(config["path"]["raw_path"], speaker, basename + ".wav")
        syn = os.path.join(syn_dir or result_path, basename + ".wav")
        missing = [p for p in (ref, syn) if not os.path.exists(p)]
        if missing:
            skipped.append((basename, "missing " + ", ".join(missing)))
            continue
        r, s = load_audio(ref, sr), load_audio(syn, sr)
        window = "whole"
        tg = os.path.join(config["path"]["preprocessed_path"], "TextGrid", speaker, basename + ".TextGrid")
        if trim and os.path.exists(tg):
            tiers = read_textgrid(tg)
            if "phones" in tiers:
                _, _, start, end = Preprocessor.get_alignment(_Rates(sr, hop), tiers["phones"])
                if start < end:
                    r, window = r[int(sr * start):int(sr * end)], "textgrid"
        reason = None
        for name, w in (("reference", r), ("synthesized", s)):
            if len(w) <= half:
                reason = f"{name} has {len(w)} samples, the STFT needs more than {half}"
            elif len(w) // hop + 1 > MAX_FRAMES:
                reason = f"{name} has {len(w) // hop + 1} frames, more than the supported {MAX_FRAMES}"
        if reason:
            skipped.append((basename, reason))
            continue
        items.append({"basename": basename, "speaker": speaker, "ref": r, "syn": s, "window": window})
    return items, skipped


class _Rates:
    """What `Preprocessor.get_alignment` reads of its instance."""

    def __init__(self, sampling_rate, hop_length):
        self.sampling_rate, self.hop_length = sampling_rate, hop_length


def run(config, result_path, source, out_path=None, syn_dir=None, ref_dir=None, trim=True, f0=True, n_mcep=None, score_fn=None,
        device="cuda", cepstra="mel", alpha=None, prosody=False, f0_estimator="dio", aligned=False, max_len_diff=None, aligned_fn=None,
        smoothing=False, wavelet=False, hnr=False):
    """score.py: pair, trim, score, write one JSON object per utterance to `out_path`.  `score_fn(ref_wavs, syn_wavs) -> [dict]`
    replaces the device stage (called with `prosody=True` as a keyword when that is asked for).  Returns (rows, skipped, summary).
    With cepstra="world" the rows and the summary also say cepstra, alpha and fft_size; with "mel" they are what they were before
    that choice existed.  `prosody` adds the prosody keys of the module docstring and is refused with f0=False before a file is
    read.  `f0_estimator` "pyin" (score.py --f0 pyin) scores F0 and prosody on pYIN tracks: rows and summary then say f0_estimator.
    `aligned` (score.py --aligned) is for wavs that share the recording's time axis, copysynth.py's: a pair whose two lengths differ
    by more than `max_len_diff` samples (default 2 hop_length, a choice: a copy-synthesis wav is T hop long, within one hop of the
    TextGrid window) is skipped as "not time-aligned"; every other pair, cut to its shorter side, also gets stoi, estoi,
    stoi_frames_kept, stoi_segments and aligned_samples (`stoi`), and the summary their means over the rows that are not too short
    and the number of those that are.  `aligned_fn(ref_wavs, syn_wavs) -> [dict]` replaces that device stage.  Without `aligned`
    every row, every summary key and every launch is what it is without this paragraph.  `smoothing` (score.py --smoothing) adds
    the over-smoothing keys of `modspec` to every row and to the summary, with ms_bands_hz, the band edges in Hz at this config's
    frame rate; a `score_fn` is then called with `smoothing=True` as a keyword.  `wavelet` (score.py --wavelet) adds the wavelet
    prosody keys of `cwt` to every row and to the summary, is refused with f0=False before a file is read, and reaches a `score_fn`
    as `wavelet=True`.  `hnr` (score.py --hnr) adds the harmonics-to-noise keys of `hnr` to every row and to the summary, is refused with
    f0=False before a file is read, and reaches a `score_fn` as `hnr=True`."""
    import json
    pp = config["preprocessing"]
    sr, hop = pp["audio"]["sampling_rate"], pp["stft"]["hop_length"]
    if prosody and not f0:
        raise ValueError("--prosody needs F0 and cannot go with --no_f0")
    if f0_estimator not in ("dio", "pyin"):
        raise ValueError(f"f0_estimator must be 'dio' or 'pyin', got {f0_estimator!r}")
    if wavelet and not f0:
        raise ValueError("--wavelet needs F0 and cannot go with --no_f0")
    if wavelet:
        from . import cwt as Cwt
        Cwt.scales(sr, hop)                                                 # refused before a file is read
    if hnr and not f0:
        raise ValueError("--hnr needs F0 and cannot go with --no_f0")
    if hnr:
        from . import hnr as Hnr
        Hnr.window(sr)                                                      # refused before a file is read
    world_keys = {}
    if cepstra == "world":                                                  # refused before a file is read
        from . import envelope as Env
        Env.check_mcep(Env.DEFAULT_MCEP if n_mcep is None else n_mcep)
        world_keys = {"cepstra": "world", "alpha": Env.alpha_for(sr, alpha), "fft_size": Env.fft_size(sr)}
    elif cepstra != "mel" or alpha is not None:
        raise ValueError(f"cepstra must be 'mel' (without alpha) or 'world', got {cepstra!r}, alpha={alpha}")
    if aligned:
        max_len_diff = 2 * hop if max_len_diff is None else max_len_diff
        if int(max_len_diff) != max_len_diff or max_len_diff < 0:
            raise ValueError(f"max_len_diff must be a number of samples >= 0, got {max_len_diff!r}")
    items, skipped = collect(config, result_path, source, syn_dir, ref_dir, trim)
    if aligned:
        kept = []
        for it in items:
            diff = abs(len(it["ref"]) - len(it["syn"]))
            if diff > max_len_diff:
                skipped.append((it["basename"], f"not time-aligned: the reference has {len(it['ref'])} samples, the synthesized file "
                                                f"{len(it['syn'])}, {diff} apart (more than {int(max_len_diff)})"))
            else:
                kept.append(it)
        items = kept
    if score_fn is None:
        from . import audio as Audio
        stft = Audio.TacotronSTFT(pp["stft"]["filter_length"], hop, pp["stft"]["win_length"], pp["mel"]["n_mel_channels"], sr,
                                  pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"])
        score_fn = lambda r, s: score_pairs(r, s, stft, sr, hop, n_mcep=n_mcep, f0=f0, device=device, cepstra=cepstra,     # noqa: E731
                                            alpha=alpha, prosody=prosody, f0_estimator=f0_estimator, smoothing=smoothing,
                                            wavelet=wavelet, hnr=hnr)
    elif prosody or smoothing or wavelet or hnr:
        given, asked = score_fn, {k: True for k, v in (("prosody", prosody), ("smoothing", smoothing), ("wavelet", wavelet),
                                                       ("hnr", hnr)) if v}
        score_fn = lambda r, s: given(r, s, **asked)                         # noqa: E731
    scores = score_fn([it["ref"] for it in items], [it["syn"] for it in items]) if items else []
    rows = [{"basename": it["basename"], "speaker": it["speaker"], "reference_window": it["window"], **sc}
            for it, sc in zip(items, scores)]
    if aligned:
        from . import stoi as Stoi
        if aligned_fn is None:
            aligned_fn = lambda r, s: Stoi.score_pairs(r, s, sr, device=device)   # noqa: E731
        cut = [min(len(it["ref"]), len(it["syn"])) for it in items]
        more = aligned_fn([it["ref"][:n] for it, n in zip(items, cut)], [it["syn"][:n] for it, n in zip(items, cut)]) if items else []
        for row, sc in zip(rows, more):
            row.update(sc)
    if out_path:
        with open(out_path, "w", encoding="utf-8") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    summary = summarize(rows)
    summary.update(world_keys)
    if aligned:
        summary.update(Stoi.summarize(rows))
    if smoothing:
        from . import modspec as Modspec
        summary["ms_bands_hz"] = [list(b) for b in Modspec.band_bins(sr, hop)[1]]
    if f0 and f0_estimator != "dio":
        summary["f0_estimator"] = f0_estimator
    summary["skipped"] = len(skipped)
    summary["reference_window"] = {k: sum(1 for r in rows if r["reference_window"] == k) for k in ("textgrid", "whole")}
    return rows, skipped, summary
