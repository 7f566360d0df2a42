"""Wavelet prosody scores on the GPU (csrc/fs2_cwt.hip): the continuous wavelet transform of an interpolated, normalised ln F0
contour at ten scales one octave apart (Suni, Aalto, Raitio, Alku, Vainio 2013), the pitch spectrogram FastSpeech 2's pitch predictor
is trained on (Ren et al. 2021, appendix), used here to say at which time scale a synthesized contour departs from the recording:
micro-prosody, syllable accents, word or phrase movement, the utterance's declination.  The constants below (tau0 = 5 ms, ten
scales, the (i + 2.5)^(-5/2) weights, adjacent scales paired into five levels) are the papers' as remembered: they were written
from memory and not checked against the text.  The specification below is what the kernels and the independent numpy restatement
(tests/cwt_ref.py: explicit loops, an FFT convolution) implement.

Arithmetic.  Everything is fp64.  Every sum carries the rounding error of each addition (two-sum) and of each product (one fma) in a
second word, per lane in ascending order and then over the 256 lanes of a workgroup by a fixed tree: the sum of the exact terms
rounded once, in all but cases too rare to meet.  No atomics; padding is never read or written; two runs give the same bytes, and a
row's bytes do not depend on its batch.  Rows have 1 <= T <= MAX_FRAMES = 2048 frames (the bound of `metrics`); anything else is a
ValueError before any launch.

Contour (`contour`, kernel fs2_cwt_contour).  f0 (B, >= Tmax) is an F0 track in Hz, 0 (anything not above 0) meaning unvoiced, as
`pitch.stonemask` and `pyin.pyin` return it.  A voiced frame gets x[t] = ln f0[t].  An unvoiced frame between the nearest voiced
frames t0 < t < t1 gets x[t] = x[t0] + (x[t1] - x[t0]) * ((t - t0) / (t1 - t0)), evaluated as written; frames before the first voiced
frame take its value, frames after the last voiced frame take its value.  m = (sum x) / T and, in a second pass, sd = sqrt(sum (x -
m)^2 / T); z = (x - m) / sd.  Per row stats = (n_voiced, m, sd, flat): flat = 1 when n_voiced = 0 (then m = sd = 0) or sd <= FLAT_SD =
1e-12, and z is then 0 over [0, T).  The previous and the next voiced frame are a forward max-scan and a backward min-scan over the
row, one workgroup per utterance, the row in LDS.

Transform (`transform`, kernel fs2_cwt_transform).  Scales i = 1 .. 10, a_i = 2^(i+1) * 0.005 * sampling_rate / hop_length frames,
taken as the float64 nearest to the exact ratio 2^(i+1) sampling_rate / (200 hop_length) of the two integers; a_1 < 1 (a hop above
20 ms) is refused.  Mexican hat psi(x) = 2 / (sqrt(3) pi^(1/4)) * (1 - x^2) * exp(-x^2 / 2).  `tables` builds tab_i[d] = a_i^(-1/2) *
(i + 2.5)^(-5/2) * psi(d / a_i) for 0 <= d <= min(2047, floor(10 a_i)) (the floor in integer arithmetic) in numpy float64; beyond
that range the table is DEFINED as 0: the cut-off is part of the specification (the first neglected term is below 1e-19 of the
peak).  The tables are uploaded once per device and rate pair; the device evaluates no exponential.  W[b][i][t] = sum over u in
[0, T), ascending, of z[u] tab_i[|u - t|]: a direct sum, the contour taken as 0 (its mean) outside [0, T), no other edge treatment.
power[b][i] = sum_t W[b][i][t]^2.  The sampling step is one frame: at a_1 of about 1.7 frames the wavelet is coarsely sampled and its
samples do not sum to exactly zero.  That is a choice: the scales are kept as stated and the frame grid is not refined for the smallest of them.

Path sums (`on_path`, kernel fs2_cwt_on_path).  Along the cepstral DTW path `metrics.dtw` returns, P cells (i, j), for 15
components: the ten scales and the five levels L_j = W_(2j-1) + W_(2j), j = 1 .. 5, formed at every cell and never stored.  With x
the reference's component at frame i and y the synthesized one's at frame j: the two means over the P cells in a first pass, then
Sxx, Syy, Sxy about them and Sd2 = sum (x - y)^2: sums (B, 15, 4).

Rows (`row_scores`).  cwt_corr (10) = Sxy / sqrt(Sxx Syy), NaN when one of Sxx, Syy <= 1e-24 P (the floor of f0_corr) or P < 2;
cwt_rmse (10) = sqrt(Sd2 / P); cwt_level_corr and cwt_level_rmse (5 each) the same of the levels; cwt_power_db_ref, cwt_power_db_syn
(10 each) = 10 log10(power / T) of each side off the path, cwt_power_ratio_db = syn - ref; lf0_mean_ref, lf0_mean_syn, lf0_std_ref,
lf0_std_syn = m and sd of each side.  Each side is normalised by its own mean and deviation, as published, so a contour with the
right shape and half the range scores a correlation of 1: level and range show up in the lf0 keys only.  If either side is flat,
every one of these keys is NaN and the summary counts the row in wavelet_flat_utterances.

Summary (`summarize`).  cwt_scales_ms = 2^(i+1) * 5 ms.  For cwt_corr, cwt_rmse, cwt_level_corr and cwt_level_rmse, per component:
the mean (`_mean`) and the path_len-weighted mean (`_weighted`) over the utterances whose value is not NaN, and the number of those
where it is (`_nan_utterances`).  cwt_power_ratio_db_by_scale: the mean of cwt_power_ratio_db over the utterances where it is
finite.  wavelet_flat_utterances.

What is claimed: the definitions above, held against the restatement and against known answers (a two-point interpolation, a pair
against itself, a contour with halved excursions, cosines at the scales' peak periods, a moving average, a flat side).  Not claimed:
agreement with any other toolkit; any number on real speech; that the constants match the papers' text beyond this statement of
them.  Out of scope: recomposing F0 from the components, CWT targets for the model, the energy contour, sequences over 2048 frames.
"""
import math

import numpy as np
import torch

from . import _lib, ops

WHO = "fastspeech2_amd.cwt"
SCALES, LEVELS, COMPONENTS = 10, 5, 15
MAX_FRAMES = 2048
TAU0_INV = 200                                              # 1 / tau0, tau0 = 5 ms
SUPPORT = 10                                                # the table of scale i ends at floor(SUPPORT a_i) frames
FLAT_SD = 1e-12
CORR_FLOOR = 1e-24                                          # = metrics.CORR_FLOOR
PSI_NORM = 2.0 / (math.sqrt(3.0) * math.pi ** 0.25)
PATH_KEYS = ("cwt_corr", "cwt_rmse", "cwt_level_corr", "cwt_level_rmse")


# ------------------------------------------------------------------------------------------------ host
def _rates(sampling_rate, hop_length):
    sr, hop = int(sampling_rate), int(hop_length)
    if sr != sampling_rate or hop != hop_length or sr < 1 or hop < 1:
        raise ValueError(f"sampling_rate and hop_length must be positive integers, got {sampling_rate!r}, {hop_length!r}")
    if 4 * sr < TAU0_INV * hop:
        raise ValueError(f"the smallest scale, 20 ms, is {4 * sr / (TAU0_INV * hop):.3f} frames of {hop} samples at {sr} Hz: below one frame")
    return sr, hop


def scales(sampling_rate, hop_length):
    """a_i in frames, i = 1 .. 10 (float64 (10,)); a ValueError when a_1 < 1."""
    sr, hop = _rates(sampling_rate, hop_length)
    return np.array([(2 ** (i + 1) * sr) / (TAU0_INV * hop) for i in range(1, SCALES + 1)], np.float64)


def scales_ms():
    return [2 ** (i + 1) * 5 for i in range(1, SCALES + 1)]


def scale_weights():
    """(i + 2.5)^(-5/2), i = 1 .. 10: the weight of scale i in the published recomposition, carried by its table."""
    return (np.arange(1, SCALES + 1, dtype=np.float64) + 2.5) ** -2.5


def psi(x):
    x = np.asarray(x, np.float64)
    return PSI_NORM * (1.0 - x * x) * np.exp(-0.5 * x * x)


def tables(sampling_rate, hop_length):
    """-> (tab (10, 2048) float64, zero beyond each scale's cut-off; support (10,) int32: the entries d = 0 .. support[i] - 1 of
    scale i + 1 count; a (10,) the scales in frames)."""
    sr, hop = _rates(sampling_rate, hop_length)
    a = scales(sr, hop)
    w = a ** -0.5 * scale_weights()
    tab = np.zeros((SCALES, MAX_FRAMES), np.float64)
    support = np.zeros(SCALES, np.int32)
    for k in range(SCALES):
        cut = min(MAX_FRAMES - 1, (SUPPORT * 2 ** (k + 2) * sr) // (TAU0_INV * hop))
        d = np.arange(cut + 1, dtype=np.float64)
        tab[k, :cut + 1] = w[k] * psi(d / a[k])
        support[k] = cut + 1
    return tab, support, a


# ------------------------------------------------------------------------------------------------ device
_tables = {}


def _tables_on(dev, sampling_rate, hop_length):
    key = (str(dev), int(sampling_rate), int(hop_length))
    if key not in _tables:
        tab, support, _ = tables(sampling_rate, hop_length)
        _tables[key] = (torch.from_numpy(tab).to(dev), np.ascontiguousarray(support))
    return _tables[key]


def _dev(t, dtype, dim, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{what} must be a tensor on the GPU ({WHO} has no CPU fallback)")
    if t.dtype != dtype or t.dim() != dim or (t.numel() and t.stride(-1) != 1):
        raise ValueError(f"{what} must be a {dim}-D {dtype} tensor with unit inner stride, got {t.dtype} {tuple(t.shape)}")
    return t


def _lens(lens, B, width, what):
    h = [int(v) for v in (lens.tolist() if isinstance(lens, (torch.Tensor, np.ndarray)) else lens)]
    for n in h:
        if not 1 <= n <= MAX_FRAMES:
            raise ValueError(f"a contour of {n} frames is outside the supported 1..{MAX_FRAMES} frames")
    if len(h) != B or width < max(h, default=0):
        raise ValueError(f"{what} of width {width} does not hold {len(h)} rows of up to {max(h, default=0)} frames (B = {B})")
    return h, max(h, default=1)


def _no_overlap(t, shape, what):
    """Strides (in elements) under which rows of `shape` (the trailing dimension has unit stride) do not overlap."""
    span = shape[-1]                                                        # the elements one entry of dimension d spans
    for d in range(len(shape) - 2, -1, -1):
        if shape[d] > 1:
            if t.stride(d) < span:
                raise ValueError(f"{what} {tuple(t.shape)} has overlapping strides {t.stride()}")
            span += (shape[d] - 1) * t.stride(d)
    return t


def _ld(t, d, need):
    """The stride of dimension d for the C side, which wants it >= need: that of a dimension of one entry (or none) says nothing."""
    return t.stride(d) if t.shape[d] > 1 else max(t.stride(d), need)


def _out(out, shape, what, device):
    """A caller's output buffer (strides of its own, at least `shape`) or a fresh one."""
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    out = _dev(out, torch.float64, len(shape), what)
    if out.device != device or out.shape[0] != shape[0] or any(o < s for o, s in zip(out.shape[1:], shape[1:])):
        raise ValueError(f"{what} {tuple(out.shape)} on {out.device} cannot hold {tuple(shape)} on {device}")
    return _no_overlap(out, shape, what)


def contour(f0, lens, out=None):
    """f0 (B, >= Tmax) float64 on the device in Hz (not above 0: unvoiced), lens frames per row -> (z (B, Tmax) float64, stats
    (B, 4) float64 = n_voiced, m, sd, flat), on the device.  `out` is a caller's z buffer, at least that large."""
    f0 = _dev(f0, torch.float64, 2, "f0")
    B = f0.shape[0]
    h, Tmax = _lens(lens, B, f0.shape[1], "f0")
    _no_overlap(f0, (B, Tmax), "f0")
    z = _out(out, (B, Tmax), "out", f0.device)
    stats = torch.empty(B, 4, dtype=torch.float64, device=f0.device)
    lens_d = torch.tensor(h, dtype=torch.int32, device=f0.device)
    _lib.call("fs2_cwt_contour", f0.data_ptr(), _ld(f0, 0, Tmax), lens_d.data_ptr(), z.data_ptr(), _ld(z, 0, Tmax), stats.data_ptr(), 4, B,
              Tmax, ops._stream())
    return z, stats


def transform(z, lens, sampling_rate, hop_length, out=None, out_power=None):
    """z (B, >= Tmax) float64 on the device (what `contour` returns), lens frames per row -> (W (B, 10, Tmax) float64, power (B, 10)
    float64) on the device.  `out` / `out_power` are buffers of the caller, at least that large."""
    _rates(sampling_rate, hop_length)                                       # refused before the device is touched
    z = _dev(z, torch.float64, 2, "z")
    B = z.shape[0]
    h, Tmax = _lens(lens, B, z.shape[1], "z")
    _no_overlap(z, (B, Tmax), "z")
    W = _out(out, (B, SCALES, Tmax), "out", z.device)
    power = _out(out_power, (B, SCALES), "out_power", z.device)
    tab, support = _tables_on(z.device, sampling_rate, hop_length)
    lens_d = torch.tensor(h, dtype=torch.int32, device=z.device)
    _lib.call("fs2_cwt_transform", z.data_ptr(), _ld(z, 0, Tmax), lens_d.data_ptr(), tab.data_ptr(), tab.stride(0), support.ctypes.data,
              W.data_ptr(), _ld(W, 0, SCALES * W.stride(1)), W.stride(1), power.data_ptr(), _ld(power, 0, SCALES), B, Tmax, ops._stream())
    return W, power


def on_path(pi, pj, path_len, W_ref, alens, W_syn, blens, out=None):
    """Path (pi, pj (B, L) int32, path_len (B,) int32 as `metrics.dtw` returns them) and the transforms W_ref (B, 10, >= T1max),
    W_syn (B, 10, >= T2max) float64 on the device -> sums (B, 15, 4) float64: Sxx, Syy, Sxy, Sd2 of the ten scales and five levels."""
    pi, pj = _dev(pi, torch.int32, 2, "pi"), _dev(pj, torch.int32, 2, "pj")
    path_len = _dev(path_len, torch.int32, 1, "path_len")
    W_ref, W_syn = _dev(W_ref, torch.float64, 3, "W_ref"), _dev(W_syn, torch.float64, 3, "W_syn")
    B = pi.shape[0]
    if pj.shape != pi.shape or pi.stride(0) != pj.stride(0) or path_len.shape[0] != B or W_ref.shape[:2] != (B, SCALES) \
            or W_syn.shape[:2] != (B, SCALES) or len({t.device for t in (pi, pj, path_len, W_ref, W_syn)}) != 1:
        raise ValueError(f"path {tuple(pi.shape)} {tuple(pj.shape)} {tuple(path_len.shape)} and the transforms {tuple(W_ref.shape)} "
                         f"{tuple(W_syn.shape)} are not B pairs of {SCALES} scales on one device")
    ah, T1 = _lens(alens, B, W_ref.shape[2], "W_ref")
    bh, T2 = _lens(blens, B, W_syn.shape[2], "W_syn")
    _no_overlap(W_ref, (B, SCALES, T1), "W_ref")
    _no_overlap(W_syn, (B, SCALES, T2), "W_syn")
    sums = _out(out, (B, COMPONENTS, 4), "out", pi.device)
    ad = torch.tensor(ah, dtype=torch.int32, device=pi.device)
    bd = torch.tensor(bh, dtype=torch.int32, device=pi.device)
    _lib.call("fs2_cwt_on_path", pi.data_ptr(), pj.data_ptr(), pi.stride(0), path_len.data_ptr(), W_ref.data_ptr(),
              _ld(W_ref, 0, SCALES * W_ref.stride(1)), W_ref.stride(1), W_syn.data_ptr(), _ld(W_syn, 0, SCALES * W_syn.stride(1)),
              W_syn.stride(1), ad.data_ptr(), bd.data_ptr(), sums.data_ptr(), _ld(sums, 0, COMPONENTS * sums.stride(1)), sums.stride(1), B, T1,
              T2, ops._stream())
    return sums


def measure(f0, lens, sampling_rate, hop_length):
    """The two per-side kernels chained -> (W (B, 10, Tmax), power (B, 10), stats (B, 4)) on the device."""
    z, stats = contour(f0, lens)
    W, power = transform(z, lens, sampling_rate, hop_length)
    return W, power, stats


# ------------------------------------------------------------------------------------------------ scores
def row_keys():
    return PATH_KEYS + ("cwt_power_db_ref", "cwt_power_db_syn", "cwt_power_ratio_db", "lf0_mean_ref", "lf0_mean_syn", "lf0_std_ref",
                        "lf0_std_syn")


def row_scores(sums, path_len, power_ref, frames_ref, stats_ref, power_syn, frames_syn, stats_syn):
    """The wavelet keys of a pair's row (module docstring) from the device results copied to the host: the path sums (15, 4), the
    path length, and per side the power (10,), the frame count and the contour's stats (4,)."""
    nan = float("nan")
    if float(stats_ref[3]) != 0.0 or float(stats_syn[3]) != 0.0:
        row = {k: [nan] * (LEVELS if "level" in k else SCALES) for k in row_keys()[:7]}
        row.update({k: nan for k in row_keys()[7:]})
        return row
    P = int(path_len)
    s = np.asarray(sums, np.float64).reshape(COMPONENTS, 4)
    corr, rmse = [], []
    for sxx, syy, sxy, sd2 in s.tolist():
        ok = P >= 2 and sxx > CORR_FLOOR * P and syy > CORR_FLOOR * P
        corr.append(sxy / math.sqrt(sxx * syy) if ok else nan)
        rmse.append(math.sqrt(sd2 / P) if P else nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        dbr = 10.0 * np.log10(np.asarray(power_ref, np.float64) / int(frames_ref))
        dbs = 10.0 * np.log10(np.asarray(power_syn, np.float64) / int(frames_syn))
        ratio = dbs - dbr
    return {"cwt_corr": corr[:SCALES], "cwt_rmse": rmse[:SCALES], "cwt_level_corr": corr[SCALES:], "cwt_level_rmse": rmse[SCALES:],
            "cwt_power_db_ref": dbr.tolist(), "cwt_power_db_syn": dbs.tolist(), "cwt_power_ratio_db": ratio.tolist(),
            "lf0_mean_ref": float(stats_ref[1]), "lf0_mean_syn": float(stats_syn[1]), "lf0_std_ref": float(stats_ref[2]),
            "lf0_std_syn": float(stats_syn[2])}


def summarize(rows):
    """The corpus keys of the module docstring from rows that carry the wavelet keys and path_len."""
    nan = float("nan")
    out = {"cwt_scales_ms": scales_ms()}
    w = np.array([r["path_len"] for r in rows], np.float64)
    for key in PATH_KEYS:
        v = np.array([r[key] for r in rows], np.float64).reshape(len(rows), -1)
        ok = ~np.isnan(v)
        mean, weighted = [], []
        for c in range(v.shape[1]):
            o = ok[:, c]
            mean.append(float(v[o, c].mean()) if o.any() else nan)
            weighted.append(float((v[o, c] * w[o]).sum() / w[o].sum()) if o.any() and w[o].sum() > 0 else nan)
        out[key + "_mean"], out[key + "_weighted"] = mean, weighted
        out[key + "_nan_utterances"] = (~ok).sum(axis=0).astype(int).tolist()
    ratio = np.array([r["cwt_power_ratio_db"] for r in rows], np.float64).reshape(len(rows), -1)
    ok = np.isfinite(ratio)
    out["cwt_power_ratio_db_by_scale"] = [float(ratio[ok[:, c], c].mean()) if ok[:, c].any() else nan for c in range(ratio.shape[1])]
    out["wavelet_flat_utterances"] = sum(1 for r in rows if math.isnan(r["lf0_mean_ref"]))
    return out
