"""Over-smoothing scores on the GPU (csrc/fs2_modspec.hip): the global variance (GV; Toda and Tokuda 2007) and the modulation
spectrum (MS; Takamichi, Toda, Black, Neubig, Sakti, Nakamura 2016) of cepstral trajectories.  An acoustic model trained with an
L1 / L2 loss predicts averaged trajectories: their variance over time is too small and their power at modulation frequencies above
a few Hz is missing, which MCD along a DTW path hardly sees.  Both measures work per utterance and per side on the cepstra
`metrics.score_pairs` already holds on the device, need no DTW, and compare a synthesized with a recorded corpus.  The
specification below is what the kernels and the independent numpy restatement (tests/modspec_ref.py, with an FFT) implement.

Arithmetic.  Everything is fp64.  Every sum runs over its terms in ascending order in one thread, with the rounding error of each
addition (two-sum) and of each product (one fma) carried in a second word that is added at the end: the sum of the exact terms
rounded once, in all but cases too rare to meet.  No atomics, no reduction across lanes; padding is never read or written; two runs
give the same bytes.

Input and limits.  c (B, Tmax, K) float64 on the device, row b holding T = lens[b] frames: 1 <= T <= MAX_FRAMES = 2048 (the bound
of `metrics`), 1 <= K <= MAX_COEF = 128 (a raw 80-band log-mel fits), any batch and frame strides in elements, unit stride in k:
what `metrics.cepstra` and `envelope.world_cepstra` return.  Anything else is a ValueError before any launch.

Moments, per (b, k) (`moments`, kernel fs2_traj_moments).  mean = (sum_t c[t]) / T in a first pass; M2 = sum_t (c[t] - mean)^2 in a
second; gv = M2 / T, the population variance Toda and Tokuda use.

Modulation spectrum, per (b, k) (`modspec`, kernel fs2_modspec).  x[t] = c[t] - mean for t < T, zero beyond, up to N = NFFT = 4096:
twice the frame bound (the paper's 2 D_s), fixed so that every utterance shares one frequency grid.  X[f] = sum_{t < T} x[t]
(cos - i sin)(2 pi ((f t) mod N) / N), f = 0 .. N / 2, against the fp64 table `twiddles()` [N][2] = {cos, sin}(2 pi j / N) built on
the host in numpy and uploaded once per device: the device evaluates no sine or cosine, and (f t) mod N is exact integer
arithmetic.  ms[f] = ln(|X[f]|^2 / T + FLOOR), |X|^2 = re re + im im.  FLOOR = 1e-12 is a choice: a power per frame far below any
cepstral trajectory of speech, which keeps exact zeros finite.  The window is rectangular, as published.

Bands (`band_bins`).  Bin f lies at f (sampling_rate / hop_length) / N Hz.  The band edges are 0, 0.5, 1, 2, 4, 8, 16, 32 Hz and the
frame-rate Nyquist sampling_rate / (2 hop_length); band j holds the bins whose frequency is >= its lower and < its upper edge, found
in integer arithmetic; the first band starts at bin 1 (DC is zero once the mean is removed), the last ends with bin N / 2, a band
without a bin or at or above the Nyquist is dropped.  The kernel gets the integer ranges and knows no rate.  band[b][k][j] = the mean
of ms[f] over the band's bins, times 10 / ln 10: dB.

Short utterances.  A pair with fewer than MIN_FRAMES = 32 frames on either side gets NaN for every MS value on both sides (32 is a
choice: below about 0.4 s there is no 4 Hz resolution) and is counted in smoothing_too_short_utterances.  The GV of a side is
reported for T >= 2 and is NaN for one frame.

Rows (`row_scores`).  gv_ref, gv_syn: K variances; gv_ratio_db: the mean over the k whose two variances are both above 0 of
10 log10(gv_syn / gv_ref), NaN without such a k, negative where the synthesized variance is too small; ms_db_ref, ms_db_syn: the
K x bands matrix of band values; ms_band_db_ref, ms_band_db_syn: its mean over k, one value per band; ms_dist_db = sqrt(mean over
(k, band) of (syn - ref)^2).

Summary (`summarize`).  With the means taken over the utterances that are not too short, of ms_db per (k, band) and side:
ms_diff_db_by_band (syn - ref, averaged over k; it goes negative towards high modulation frequencies when the model over-smooths)
and ms_dist_db_corpus = sqrt(mean over (k, band) of that difference squared).  With the means of gv per k and side over the
utterances that have a GV on both sides: gv_ratio_db_by_coef = 10 log10(syn / ref), NaN where one is not above 0.  The plain means
of gv_ratio_db and ms_dist_db over the utterances where they are not NaN, as gv_ratio_db_mean and ms_dist_db_mean, with
gv_ratio_db_nan_utterances and ms_dist_db_nan_utterances; smoothing_too_short_utterances.  `metrics.run` adds ms_bands_hz.

What is claimed: the published definitions as written above, held against the restatement and against known answers (a cosine, a
constant, a smoothed noise trajectory).  Not claimed: agreement with any other toolkit; any number on real speech; the 32-frame and
1e-12 choices; that a value near 0 means "natural".  Only two runs of this tool compare.
"""
import math

import numpy as np
import torch

from . import _lib, ops

WHO = "fastspeech2_amd.modspec"
NFFT, MAX_FRAMES, MAX_COEF, MAX_BANDS = 4096, 2048, 128, 16
FLOOR = 1e-12
MIN_FRAMES = 32
EDGES_HZ = (0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0)
DB = 10.0 / math.log(10.0)


# ------------------------------------------------------------------------------------------------ host
def twiddles():
    """[4096][2] fp64: cos and sin of 2 pi j / 4096."""
    a = 2.0 * np.pi * np.arange(NFFT, dtype=np.float64) / NFFT
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))


def band_bins(sampling_rate, hop_length):
    """-> (bins [(lo, hi)]: band j is the bins lo <= f < hi, hz [(lower, upper edge)]) of the module docstring's bands."""
    sr, hop = int(sampling_rate), int(hop_length)
    if sr != sampling_rate or hop != hop_length or sr < 1 or hop < 1:
        raise ValueError(f"sampling_rate and hop_length must be positive integers, got {sampling_rate!r}, {hop_length!r}")
    first = lambda twice_hz: -(-twice_hz * hop * NFFT // (2 * sr))          # noqa: E731  the first bin with f sr / (hop N) >= hz
    nyquist = sr / (2.0 * hop)
    bins, hz = [], []
    for j, lower in enumerate(EDGES_HZ):
        if lower >= nyquist:
            break
        upper = EDGES_HZ[j + 1] if j + 1 < len(EDGES_HZ) and EDGES_HZ[j + 1] < nyquist else nyquist
        lo = max(first(int(2 * lower)), 1)
        hi = first(int(2 * upper)) if upper < nyquist else NFFT // 2 + 1
        if lo < hi:
            bins.append((lo, hi))
            hz.append((lower, upper))
    return bins, hz


def _check_bins(bins):
    bins = [(int(lo), int(hi)) for lo, hi in bins]
    if not 1 <= len(bins) <= MAX_BANDS:
        raise ValueError(f"{len(bins)} bands, supported are 1..{MAX_BANDS}")
    end = 0
    for lo, hi in bins:
        if not end <= lo < hi <= NFFT // 2 + 1:
            raise ValueError(f"band bins must be non-empty, ascending, disjoint ranges within [0, {NFFT // 2 + 1}), got {bins}")
        end = hi
    return np.ascontiguousarray(np.array(bins, dtype=np.int32))


# ------------------------------------------------------------------------------------------------ device
_tables = {}


def _twiddles_on(dev):
    key = str(dev)
    if key not in _tables:
        _tables[key] = torch.from_numpy(twiddles()).to(dev)
    return _tables[key]


def _dev(t, dim, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{what} must be a tensor on the GPU ({WHO} has no CPU fallback)")
    if t.dtype != torch.float64 or t.dim() != dim or (t.numel() and t.stride(-1) != 1):
        raise ValueError(f"{what} must be a {dim}-D float64 tensor with unit inner stride, got {t.dtype} {tuple(t.shape)}")
    return t


def _input(c, lens):
    """c and its lengths, checked against the module docstring's limits -> (c, B, Tmax, K, lens on the device)"""
    h = [int(v) for v in (lens.tolist() if isinstance(lens, (torch.Tensor, np.ndarray)) else lens)]
    for n in h:
        if not 1 <= n <= MAX_FRAMES:
            raise ValueError(f"a trajectory of {n} frames is outside the supported 1..{MAX_FRAMES} frames")
    c = _dev(c, 3, "c")
    B, width, K = c.shape
    if not 1 <= K <= MAX_COEF:
        raise ValueError(f"{K} coefficients, supported are 1..{MAX_COEF}")
    Tmax = max(h, default=1)
    if len(h) != B or width < Tmax:
        raise ValueError(f"c {tuple(c.shape)} does not hold {len(h)} rows of up to {Tmax} frames")
    if B and (c.stride(1) < K or (B > 1 and c.stride(0) < Tmax * c.stride(1))):
        raise ValueError(f"c has overlapping strides {c.stride()}")
    return c, B, Tmax, K, torch.tensor(h, dtype=torch.int32, device=c.device)


def _out(out, shape, what, device):
    """A caller's output buffer (batch / row strides of its own, at least `shape`) or a fresh one."""
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    out = _dev(out, 3, what)
    if out.device != device or out.shape[0] != shape[0] or any(o < s for o, s in zip(out.shape[1:], shape[1:])) \
            or out.stride(1) < shape[2] or (shape[0] > 1 and out.stride(0) < shape[1] * out.stride(1)):
        raise ValueError(f"{what} {tuple(out.shape)} with strides {out.stride()} cannot hold {tuple(shape)}")
    return out


def moments(c, lens, out=None):
    """c (B, >= Tmax, K) float64 on the device, lens frames per row -> mom (B, K, 2) float64: the mean and M2 of every trajectory."""
    c, B, Tmax, K, lens_d = _input(c, lens)
    mom = _out(out, (B, K, 2), "out", c.device)
    _lib.call("fs2_traj_moments", c.data_ptr(), c.stride(0), c.stride(1), lens_d.data_ptr(), mom.data_ptr(), mom.stride(0), mom.stride(1),
              B, Tmax, K, ops._stream())
    return mom


def modspec(c, lens, mean, bins, logms=False, out=None, out_logms=None):
    """c and lens as `moments` takes them, mean (B, K) float64 on the device (any strides: `moments(c, lens)[:, :, 0]` serves), bins
    the integer ranges of `band_bins` -> bands (B, K, len(bins)) float64 in dB, or with `logms` (bands, logms (B, K, 2049) float64:
    every ms[f]).  `out` / `out_logms` are buffers of the caller, at least that large."""
    table = _check_bins(bins)
    c, B, Tmax, K, lens_d = _input(c, lens)
    if not isinstance(mean, torch.Tensor) or mean.device != c.device or mean.dtype != torch.float64 or tuple(mean.shape) != (B, K):
        raise ValueError(f"mean must be a ({B}, {K}) float64 tensor on {c.device}")
    if B and (mean.stride(1) < 1 or (B > 1 and mean.stride(0) < (K - 1) * mean.stride(1) + 1)):
        raise ValueError(f"mean has overlapping strides {mean.stride()}")
    J = len(table)
    bands = _out(out, (B, K, J), "out", c.device)
    full = _out(out_logms, (B, K, NFFT // 2 + 1), "out_logms", c.device) if logms or out_logms is not None else None
    _lib.call("fs2_modspec", c.data_ptr(), c.stride(0), c.stride(1), lens_d.data_ptr(), mean.data_ptr(), mean.stride(0), mean.stride(1),
              _twiddles_on(c.device).data_ptr(), table.ctypes.data, J, FLOOR, bands.data_ptr(), bands.stride(0), bands.stride(1),
              None if full is None else full.data_ptr(), 0 if full is None else full.stride(0), 0 if full is None else full.stride(1),
              B, Tmax, K, ops._stream())
    return bands if full is None else (bands, full)


def measure(c, lens, bins):
    """Both kernels on one side of a batch -> (m2 (B, K), bands (B, K, len(bins))) on the device."""
    mom = moments(c, lens)
    return mom[:, :, 1], modspec(c, lens, mom[:, :, 0], bins)


# ------------------------------------------------------------------------------------------------ scores
def row_scores(m2_ref, bands_ref, frames_ref, m2_syn, bands_syn, frames_syn):
    """The smoothing keys of a pair's row (module docstring) from the device results copied to the host: M2 (K,) and the band
    values (K, bands) of each side, and the two frame counts."""
    nan = float("nan")
    Tr, Ts = int(frames_ref), int(frames_syn)
    m2r, m2s = np.asarray(m2_ref, np.float64), np.asarray(m2_syn, np.float64)
    gr = m2r / Tr if Tr >= 2 else np.full_like(m2r, nan)
    gs = m2s / Ts if Ts >= 2 else np.full_like(m2s, nan)
    both = (gr > 0) & (gs > 0)
    ratio = float(np.mean(10.0 * np.log10(gs[both] / gr[both]))) if both.any() else nan
    br, bs = np.array(bands_ref, np.float64), np.array(bands_syn, np.float64)
    if min(Tr, Ts) < MIN_FRAMES:
        br[:], bs[:] = nan, nan
    return {"gv_ref": gr.tolist(), "gv_syn": gs.tolist(), "gv_ratio_db": ratio, "ms_db_ref": br.tolist(), "ms_db_syn": bs.tolist(),
            "ms_band_db_ref": br.mean(axis=0).tolist(), "ms_band_db_syn": bs.mean(axis=0).tolist(),
            "ms_dist_db": float(np.sqrt(np.mean((bs - br) ** 2)))}


def summarize(rows):
    """The corpus keys of the module docstring from rows that carry the smoothing keys."""
    nan = float("nan")
    out = {}
    ms = [r for r in rows if not np.isnan(r["ms_dist_db"])]
    if ms:
        diff = np.mean([r["ms_db_syn"] for r in ms], axis=0) - np.mean([r["ms_db_ref"] for r in ms], axis=0)     # (K, bands)
        out["ms_diff_db_by_band"] = diff.mean(axis=0).tolist()
        out["ms_dist_db_corpus"] = float(np.sqrt(np.mean(diff ** 2)))
    else:
        out["ms_diff_db_by_band"], out["ms_dist_db_corpus"] = None, nan
    gv = [r for r in rows if not (np.isnan(r["gv_ref"]).any() or np.isnan(r["gv_syn"]).any())]
    if gv:
        gr, gs = np.mean([r["gv_ref"] for r in gv], axis=0), np.mean([r["gv_syn"] for r in gv], axis=0)
        ok = (gr > 0) & (gs > 0)
        out["gv_ratio_db_by_coef"] = [float(10.0 * np.log10(s / r)) if o else nan for r, s, o in zip(gr, gs, ok)]
    else:
        out["gv_ratio_db_by_coef"] = None
    for key in ("gv_ratio_db", "ms_dist_db"):
        v = np.array([r[key] for r in rows], np.float64)
        ok = ~np.isnan(v)
        out[key + "_mean"] = float(v[ok].mean()) if ok.any() else nan
        out[key + "_nan_utterances"] = int((~ok).sum())
    out["smoothing_too_short_utterances"] = sum(1 for r in rows if min(r["frames_ref"], r["frames_syn"]) < MIN_FRAMES)
    return out
